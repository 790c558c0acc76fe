// The moving bed's arithmetic (csrc/hp_bed.hpp: bed_fraction, bed_level, bed_round) without a GPU: the header's HIP-free part under
// a plain host compiler, the very definition the kernel bed_apply uses.  Reads cases from standard input, one a line, every double
// as the 16 hexadecimal digits of its bit pattern:
//     F n t  t_0 f_0 ... t_n-1 f_n-1      -> the fraction at t
//     L base target f                     -> the new bed in fp64, and rounded once to fp32 (widened again)
// and prints the results' bit patterns, one line per case.  tests/test_bed_shapes.py holds them to frontend.BedShapes bit for bit.
// What hp_bed_shape_add does before it touches the device (validate_bed_shape, bed_layout, bed_image) is the same header's:
//     B esize cols global_rows row_lo row_hi shapes  { n m  id_0 .. id_n-1  target_0 .. target_n-1  t_0 f_0 .. t_m-1 f_m-1 } ...
// adds the shapes in turn on a strip that stores the global rows [row_lo, row_hi) (ids in decimal) and prints, for the last one, the
// layout's six offsets and its size in decimal and the image's bytes in hex -- or "! " and the message of the check that refused one.
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
		} else if (kind == "B") {
			// shape after shape onto an empty strip, each as hp_bed_shape_add does it in front of the upload: checks, the strip's share, layout, image, commit
			size_t esize, shapes;
			uint64_t cols, global_rows, row_lo, row_hi;
			if (!(in >> esize >> cols >> global_rows >> row_lo >> row_hi >> shapes)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			hp::BedHost host;
			hp::BedLayout l = {};
			std::vector<unsigned char> image;
			std::string why;
			for (size_t s = 0; s < shapes && why.empty(); ++s) {
				uint64_t n;
				unsigned m;
				if (!(in >> n >> m)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
				std::vector<uint64_t> ids((size_t)n), listed;
				std::vector<double> target((size_t)n), series(2 * (size_t)m);
				for (auto& c : ids) in >> c;
				for (auto& t : target) { in >> w; t = from_bits(w); }
				for (auto& t : series) { in >> w; t = from_bits(w); }
				if (!in) { std::fprintf(stderr, "short shape: %s\n", line.c_str()); return 2; }
				const hp_bed_shape_desc_t desc = {(uint32_t)sizeof(hp_bed_shape_desc_t), m, n, ids.data(), target.data(), series.data()};
				if (!hp::validate_bed_shape(&desc, &host, cols, global_rows, listed, why)) break;
				std::vector<uint64_t> cells(host.cells);
				std::vector<double> local(host.target);
				for (uint64_t k = 0; k < n; ++k) {
					const uint64_t gy = ids[k] / cols;
					if (gy < row_lo || gy >= row_hi) continue;
					cells.push_back(ids[k] - row_lo * cols);
					local.push_back(target[k]);
				}
				l = hp::bed_layout(cells.size(), host.series.size() / 2 + m, s + 1, esize);
				image = hp::bed_image(l, host, cells, local, series.data(), m);
				host.shape_of.resize(cells.size(), (unsigned char)s);
				host.listed.swap(listed);
				host.cells.swap(cells);
				host.target.swap(local);
				host.series.insert(host.series.end(), series.begin(), series.end());
				host.series_off.push_back((unsigned)(host.series.size() / 2));
			}
			if (!why.empty()) { std::printf("! %s\n", why.c_str()); continue; }
			std::printf("%zu %zu %zu %zu %zu %zu %zu ", l.cells, l.target, l.series, l.base, l.series_off, l.shape_of, l.bytes);
			for (const unsigned char c : image) std::printf("%02x", c);
			std::printf("\n");
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
