// The tracer set's fp64 arithmetic and host checks (csrc/hp_tracer.hpp: tracer_decay, tracer_source_add, validate_tracer_set_enable and
// validate_tracer_source with a species) without a GPU: the header under a plain host compiler, the very definitions the kernels
// tracer_step_set / tracer_sources and hp_tracer_enable_set / hp_tracer_add_source_to use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     D M lambda dt                                            -> M'' (step 6)
//     S M dt dx t lambda  n_entries {time rate} x n_entries    -> M of a listed cell after the source step and, the cell being a copy
//                                                                  case, step 6: what one species' plane holds after the iteration
//     E struct_size species  n_decay decay...  cells n_initial initial...
//                                                              -> "ok" or "bad <message>"  (struct_size 0 stands for the right one,
//                                                                  "null" for the whole line for a NULL descriptor)
//     A species species_count cols rows  n_have have...  n_have_sources  n_cells cells...  n_entries {time rate} x n_entries
//                                                              -> "ok <keys listed afterwards>" or "bad <message>"  (`have`: the keys
//                                                                  species * cols * rows + cell listed already, sorted)
// tests/test_tracer_set.py holds the results to frontend.Tracer(decay=...) bit for bit.
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
		if (what == "D") {
			double v[3];
			for (double& x : v) { in >> w; x = from_bits(w); }
			if (!in) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			std::printf("%016llx\n", bits(hp::tracer_decay(v[0], v[1], v[2])));
		} else if (what == "S") {
			double head[5];
			for (double& h : head) { in >> w; h = from_bits(w); }
			unsigned n;
			in >> n;
			std::vector<double> series(2 * (size_t)n);
			for (double& s : series) { in >> w; s = from_bits(w); }
			if (!in || n < 1) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			double M = head[0];
			if (head[1] > 0.0) M = hp::tracer_source_add(M, hp::tracer_rate(series.data(), n, head[3]), head[1], head[2]);
			std::printf("%016llx\n", bits(hp::tracer_decay(M, head[4], head[1])));
		} else if (what == "E") {
			std::string first, why;
			in >> first;
			if (first == "null") {
				const bool ok = hp::validate_tracer_set_enable(nullptr, 0, why);
				std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
				continue;
			}
			hp_tracer_set_desc_t desc;
			unsigned long long cells, n_decay, n_initial;
			desc.struct_size = (uint32_t)std::stoul(first);
			if (desc.struct_size == 0) desc.struct_size = sizeof desc;
			in >> desc.species >> n_decay;
			std::vector<double> decay(n_decay);
			for (double& l : decay) { in >> w; l = from_bits(w); }
			in >> cells >> n_initial;
			std::vector<double> initial(n_initial);
			for (double& m : initial) { in >> w; m = from_bits(w); }
			const bool in_range = desc.species >= 1 && desc.species <= HP_TRACER_MAX_SPECIES;      // (otherwise the arrays are never read)
			if (!in || (in_range && n_decay && n_decay != desc.species) || (in_range && n_initial && n_initial != cells * desc.species)) {
				std::fprintf(stderr, "bad case: %s\n", line.c_str());
				return 2;
			}
			desc.decay = decay.empty() ? nullptr : decay.data();
			desc.initial = initial.empty() ? nullptr : initial.data();
			const bool ok = hp::validate_tracer_set_enable(&desc, cells, why);
			std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
		} else if (what == "A") {
			unsigned species, species_count, n_entries;
			unsigned long long cols, rows, n_have, n_sources, n_cells;
			in >> species >> species_count >> cols >> rows >> n_have;
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
			                                           have, cols, rows, listed, why, species, species_count, "hp_tracer_add_source_to");
			std::string keys = "ok";
			for (const uint64_t k : listed) keys += " " + std::to_string(k);
			std::printf("%s\n", ok ? keys.c_str() : ("bad " + why).c_str());
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
