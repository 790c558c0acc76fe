// The link groups' arithmetic and host checks (csrc/hp_links.hpp: link_flow, link_record, validate_links, links_strip_verdict)
// without a GPU: the header under a plain host compiler, the very definitions the kernel bdy_links and hp_boundary_add_links use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     L kind one_way  level size coeff limit  za zmax_a bed_a  zb zmax_b bed_b  dt dx  volume active
//         -> za zb (fp64)  za zb (rounded once to fp32, widened)  dz  q_last  volume  active  inert
//     V cols global_rows reach existing n_taken taken... count  {cell_a cell_b kind one_way level size coeff limit} x count
//         -> "ok" or "bad <message>"        (count 0 with no link passes a NULL pointer)
//     S row_a row_b local_lo local_hi stale_lo stale_hi      -> 0 neither, 1 one, 2 both
// tests/test_links.py holds the results to frontend.Links bit for bit.
#include "hp_links.hpp"

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
		if (what == "L") {
			int kind, one_way;
			in >> kind >> one_way;
			std::vector<double> v;
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 14) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const hp::LinkEnd A = {v[4], v[5], v[6]}, B = {v[7], v[8], v[9]};
			const hp::LinkFlow f = hp::link_flow(kind, one_way, v[0], v[1], v[2], v[3], A, B, v[10], v[11]);
			hp_link_record_t rec = {-1.0, v[12], (uint64_t)v[13], 0};
			hp::link_record(rec, f, v[10], v[11]);
			std::printf("%016llx %016llx %016llx %016llx %016llx %016llx %016llx %llu %d\n", bits(f.za), bits(f.zb), bits((double)(float)f.za),
			            bits((double)(float)f.zb), bits(f.dz), bits(rec.q_last), bits(rec.volume), (unsigned long long)rec.active, f.inert ? 1 : 0);
		} else if (what == "V") {
			unsigned long long cols, rows, reach, existing, n_taken, count;
			in >> cols >> rows >> reach >> existing >> n_taken;
			std::vector<uint64_t> taken(n_taken), after;
			for (auto& t : taken) in >> t;
			in >> count;
			std::vector<hp_link_t> links;
			hp_link_t l;
			while (in >> l.cell_a >> l.cell_b >> l.kind >> l.one_way) {
				double* d[4] = {&l.level, &l.size, &l.coeff, &l.limit};
				for (double* p : d) { in >> w; *p = from_bits(w); }
				links.push_back(l);
			}
			std::string why;
			const bool ok = hp::validate_links(links.empty() ? nullptr : links.data(), count, existing, cols, rows, reach, taken, after, why);
			if (ok) std::printf("ok %zu\n", after.size()); else std::printf("bad %s\n", why.c_str());
		} else if (what == "S") {
			long long v[6];
			for (auto& x : v) in >> x;
			std::printf("%d\n", hp::links_strip_verdict(v[0], v[1], v[2], v[3], v[4], v[5]));
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
