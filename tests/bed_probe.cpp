// The moving bed's arithmetic (csrc/hp_bed.hpp: bed_fraction, bed_level, bed_round) without a GPU: the header's HIP-free part under
// a plain host compiler, the very definition the kernel bed_apply uses.  Reads cases from standard input, one a line, every double
// as the 16 hexadecimal digits of its bit pattern:
//     F n t  t_0 f_0 ... t_n-1 f_n-1      -> the fraction at t
//     L base target f                     -> the new bed in fp64, and rounded once to fp32 (widened again)
// and prints the results' bit patterns, one line per case.  tests/test_bed_shapes.py holds them to frontend.BedShapes bit for bit.
#include "hp_bed.hpp"

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
		std::string kind, w;
		if (!(in >> kind)) continue;
		std::vector<double> v;
		if (kind == "F") {
			unsigned n;
			if (!(in >> n) || n < 1 || n > hp::BED_MAX_SERIES) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 1 + 2 * (size_t)n) { std::fprintf(stderr, "short series: %s\n", line.c_str()); return 2; }
			std::printf("%016llx\n", bits(hp::bed_fraction(v.data() + 1, n, v[0])));
		} else if (kind == "L") {
			while (in >> w) v.push_back(from_bits(w));
			if (v.size() != 3) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			std::printf("%016llx %016llx\n", bits(hp::bed_round<double>(v[0], v[1], v[2])), bits((double)hp::bed_round<float>(v[0], v[1], v[2])));
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
