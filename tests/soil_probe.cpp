// The infiltration's arithmetic and host checks (csrc/hp_soil.hpp: soil_step, validate_infiltration) without a GPU: the header
// under a plain host compiler, the very definitions the kernel bdy_infiltration and hp_boundary_add_infiltration use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     C ks suction deficit capacity  F z zmax bed dt
//         -> dF  z1 (fp64)  z1 (rounded once to fp32, widened)  F + dF
//     V struct_size class_count n_classes {ks suction deficit capacity} x n_classes  cells n_ids ids...  n_initial initial...
//         -> "ok <pervious cells>" or "bad <message>"   (n_classes 0 / n_ids 0 pass a NULL pointer, n_initial 0 no initial;
//            struct_size 0 stands for the right one, "null" for the whole line for a NULL descriptor)
//     R x global_row cols global_rows      -> 1 on the grid's edge ring, else 0
// tests/test_infiltration.py holds the results to frontend.Infiltration bit for bit.
#include "hp_soil.hpp"

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
		if (what == "C") {
			std::vector<double> v;
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 9) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const hp_soil_class_t cls = {v[0], v[1], v[2], v[3]};
			const double S = v[1] * v[2];
			const hp::SoilStep s = hp::soil_step(cls, S, v[4], v[5], v[6], v[7], v[8]);
			const double f1 = s.dF > 0.0 ? v[4] + s.dF : v[4];
			std::printf("%016llx %016llx %016llx %016llx\n", bits(s.dF), bits(s.z1), bits((double)(float)s.z1), bits(f1));
		} else if (what == "V") {
			std::string first;
			in >> first;
			uint64_t pervious = 0;
			std::string why;
			if (first == "null") {
				const bool ok = hp::validate_infiltration(nullptr, 0, pervious, why);
				std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
				continue;
			}
			hp_infiltration_desc_t desc;
			unsigned long long n_classes, cells, n_ids, n_initial;
			desc.struct_size = (uint32_t)std::stoul(first);
			if (desc.struct_size == 0) desc.struct_size = sizeof desc;
			in >> desc.class_count >> n_classes;
			std::vector<hp_soil_class_t> classes(n_classes);
			for (auto& c : classes) {
				double* d[4] = {&c.ks, &c.suction, &c.deficit, &c.capacity};
				for (double* p : d) { in >> w; *p = from_bits(w); }
			}
			in >> cells >> n_ids;
			std::vector<uint8_t> ids(n_ids);
			for (auto& id : ids) { unsigned v; in >> v; id = (uint8_t)v; }
			in >> n_initial;
			std::vector<double> initial(n_initial);
			for (auto& f : initial) { in >> w; f = from_bits(w); }
			if (!in || (n_ids && n_ids != cells) || (n_initial && n_initial != cells)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			desc.classes = classes.empty() ? nullptr : classes.data();
			desc.soil_of_cell = ids.empty() ? nullptr : ids.data();
			desc.initial = initial.empty() ? nullptr : initial.data();
			const bool ok = hp::validate_infiltration(&desc, cells, pervious, why);
			if (ok) std::printf("ok %llu\n", (unsigned long long)pervious); else std::printf("bad %s\n", why.c_str());
		} else if (what == "R") {
			long v[4];
			for (auto& x : v) in >> x;
			std::printf("%d\n", hp::soil_on_ring(v[0], v[1], v[2], v[3]) ? 1 : 0);
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
