// The tracer's fp64 arithmetic and host checks (csrc/hp_tracer.hpp: tracer_conc, tracer_update, tracer_source_add, tracer_rate,
// validate_tracer_enable, validate_tracer_source) without a GPU: the header under a plain host compiler, the very definitions the
// kernels tracer_step / tracer_sources and hp_tracer_enable / hp_tracer_add_source use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     U M MN MS ME MW  hC hN hS hE hW  FN FS FE FW  dt dx      -> M' (steps 3 to 5 given the four fluxes and the five raw depths)
//     S M dt dx t  n_entries {time rate} x n_entries           -> the rate at t, and M after the source step
//     E struct_size cells n_initial initial...                 -> "ok" or "bad <message>"  (struct_size 0 stands for the right one,
//                                                                  "null" for the whole line for a NULL descriptor)
//     A cols rows  n_have have...  n_have_sources  n_cells cells...  n_entries {time rate} x n_entries
//                                                              -> "ok" or "bad <message>"  (n_cells 0 / n_entries 0 pass NULL;
//                                                                  `have`: the cells other sources list already, sorted)
// tests/test_tracer.py holds the results to frontend.Tracer bit for bit.
#include "hp_tracer.hpp"

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
		if (what == "U") {
			std::vector<double> v;
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 16) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const double cC = hp::tracer_conc(v[0], v[5]), cN = hp::tracer_conc(v[1], v[6]), cS = hp::tracer_conc(v[2], v[7]);
			const double cE = hp::tracer_conc(v[3], v[8]), cW = hp::tracer_conc(v[4], v[9]);
			std::printf("%016llx\n", bits(hp::tracer_update(v[0], cC, cN, cS, cE, cW, v[10], v[11], v[12], v[13], v[14], v[15])));
		} else if (what == "S") {
			double head[4];
			for (double& h : head) { in >> w; h = from_bits(w); }
			unsigned n;
			in >> n;
			std::vector<double> series(2 * (size_t)n);
			for (double& s : series) { in >> w; s = from_bits(w); }
			if (!in || n < 1) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const double rate = hp::tracer_rate(series.data(), n, head[3]);
			std::printf("%016llx %016llx\n", bits(rate), bits(hp::tracer_source_add(head[0], rate, head[1], head[2])));
		} else if (what == "E") {
			std::string first, why;
			in >> first;
			if (first == "null") {
				const bool ok = hp::validate_tracer_enable(nullptr, 0, why);
				std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
				continue;
			}
			hp_tracer_desc_t desc;
			unsigned long long cells, n_initial;
			desc.struct_size = (uint32_t)std::stoul(first);
			if (desc.struct_size == 0) desc.struct_size = sizeof desc;
			desc.reserved = 0;
			in >> cells >> n_initial;
			std::vector<double> initial(n_initial);
			for (double& m : initial) { in >> w; m = from_bits(w); }
			if (!in || (n_initial && n_initial != cells)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			desc.initial = initial.empty() ? nullptr : initial.data();
			const bool ok = hp::validate_tracer_enable(&desc, cells, why);
			std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
		} else if (what == "A") {
			unsigned long long cols, rows, n_have, n_sources, n_cells;
			unsigned n_entries;
			in >> cols >> rows >> n_have;
			hp::TracerHost have;
			have.listed.resize(n_have);
			for (auto& c : have.listed) in >> c;
			in >> n_sources;
			have.series_off.resize(n_sources + 1, 0u);
			in >> n_cells;
			std::vector<uint64_t> cells(n_cells);
			for (auto& c : cells) in >> c;
			in >> n_entries;
			std::vector<double> series(2 * (size_t)n_entries);
			for (double& s : series) { in >> w; s = from_bits(w); }
			if (!in) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			std::vector<uint64_t> listed;
			std::string why;
			const bool ok = hp::validate_tracer_source(cells.empty() ? nullptr : cells.data(), n_cells, series.empty() ? nullptr : series.data(), n_entries,
			                                           have, cols, rows, listed, why);
			std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
