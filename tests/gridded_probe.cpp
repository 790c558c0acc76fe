// The cover check of a gridded boundary (csrc/hp_gridded.hpp: gridded_covers) without a GPU: the header under a plain host compiler,
// the very function hp_boundary_add_gridded calls.  Reads cases from standard input, one a line, every double as the 16 hexadecimal
// digits of its bit pattern and the integers in decimal:
//     dx resolution off_x off_y cols global_rows grid_cols grid_rows
// and prints two digits per case: the verdict for an fp32 domain and for an fp64 domain (1 = the grid covers the interior cells).
// tests/test_gridded_lookup.py holds them to a NumPy restatement that looks at EVERY interior cell; the program may also be built
// with -fsanitize=address,undefined.
#include "hp_gridded.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

static double from_bits(const std::string& s)
{
	const unsigned long long u = std::stoull(s, nullptr, 16);
	double v;
	std::memcpy(&v, &u, 8);
	return v;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string w[4];
		long cols, rows;
		unsigned long long gcols, grows;
		if (!(in >> w[0])) continue;
		if (!(in >> w[1] >> w[2] >> w[3] >> cols >> rows >> gcols >> grows) || cols < 3 || rows < 3) {
			std::fprintf(stderr, "bad case: %s\n", line.c_str());
			return 2;
		}
		const double dx = from_bits(w[0]), res = from_bits(w[1]), ox = from_bits(w[2]), oy = from_bits(w[3]);
		std::printf("%d%d\n", hp::gridded_covers<float>(dx, res, ox, oy, cols, rows, gcols, grows) ? 1 : 0,
		            hp::gridded_covers<double>(dx, res, ox, oy, cols, rows, gcols, grows) ? 1 : 0);
	}
	return 0;
}
