// The open boundary's arithmetic and host checks (csrc/hp_open.hpp: open_impose, open_record, validate_open, open_strip_keeps) without
// a GPU: the header under a plain host compiler, the very definitions the kernel bdy_open and hp_boundary_add_open use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     I edge  zmax_r bed_r  z_i zmax_i qn_i qs_i bed_i  dt dx  F  volume active
//         -> inert  lvl (fp64)  lvl (rounded once to fp32, widened)  qn  qs  dry capped zeroed  q_last  volume  active
//     V cols global_rows existing n_taken taken... count  {edge reserved first last} x count
//         -> "ok <cells listed on the domain>" or "bad <message>"        (no segment on the line passes a NULL pointer)
//     S ring_row inner_row local_lo local_hi      -> 1 kept, 0 not
// tests/test_open.py holds the results to frontend.Open bit for bit.
#include "hp_open.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static double from_bits(const std::string& s)
{
	const unsigned long long u = std::stoull(s, nullptr, 16);
	double v;
	std::memcpy(&v, &u, 8);
	return v;
}
static unsigned long long bits(const double v)
{
	unsigned long long u;
	std::memcpy(&u, &v, 8);
	return u;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string what, w;
		if (!(in >> what)) continue;
		if (what == "I") {
			int edge;
			in >> edge;
			std::vector<double> v;
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 12) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const hp::OpenRing R = {v[0], v[1]};
			const hp::OpenInner I = {v[2], v[3], v[4], v[5], v[6]};
			const hp::OpenImposed o = hp::open_impose(edge, R, I, v[7]);
			hp_open_record_t rec = {-1.0, v[10], (uint64_t)v[11], 0};
			hp::open_record(rec, o.inert, edge, v[9], v[7], v[8]);
			std::printf("%d %016llx %016llx %016llx %016llx %d %d %d %016llx %016llx %llu\n", o.inert ? 1 : 0, bits(o.lvl), bits((double)(float)o.lvl), bits(o.qn),
			            bits(o.qs), o.dry ? 1 : 0, o.capped ? 1 : 0, o.zeroed ? 1 : 0, bits(rec.q_last), bits(rec.volume), (unsigned long long)rec.active);
		} else if (what == "V") {
			long long cols, rows;
			unsigned long long existing, n_taken, count;
			in >> cols >> rows >> existing >> n_taken;
			std::vector<uint64_t> taken(n_taken), after;
			for (auto& t : taken) in >> t;
			in >> count;
			std::vector<hp_open_segment_t> segments;
			long long e, r, first, last;
			while (in >> e >> r >> first >> last) segments.push_back(hp_open_segment_t{(int32_t)e, (int32_t)r, first, last});
			std::string why;
			const bool ok = hp::validate_open(segments.empty() ? nullptr : segments.data(), (uint32_t)count, (uint32_t)existing, cols, rows, taken, after, why);
			if (ok) std::printf("ok %zu\n", after.size()); else std::printf("bad %s\n", why.c_str());
		} else if (what == "S") {
			long long v[4];
			for (auto& x : v) in >> x;
			std::printf("%d\n", hp::open_strip_keeps(v[0], v[1], v[2], v[3]) ? 1 : 0);
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
