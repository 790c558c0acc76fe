// Probe of hp_tiling.hpp for tests/test_tiling.py: plain C++17, no HIP.  Reads one case per line from stdin --
//   cols rows precision cus strip [HP_NAME=value ...]
// -- and prints, as one JSON object per line, what choose_tiling decides and the TileMap of the launches the engine would
// make of it (the argument lists are those of launch_march / launch_muscl / run_pair_t in hp_engine.hip).
#include "hp_tiling.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

using namespace hp;

// what hp_engine.hip's tiling_knobs / launch_knobs make of the environment
static bool set_knob(TilingKnobs& k, LaunchKnobs& l, const std::string& name, const char* v)
{
	if (name == "HP_RSEG_REFINE") k.rseg_refine = std::atoi(v) != 0;
	else if (name == "HP_TILING_SEARCH") k.search = k.search_pair = std::atoi(v) != 0;
	else if (name == "HP_TILING_SEARCH_F32") k.search_f32 = true;
	else if (name == "HP_TILING_FILL") k.tiling_fill = std::atof(v);
	else if (name == "HP_MARCH2_FILL") k.march2_fill = std::atof(v);
	else if (name == "HP_MARCH_RSEG") k.march_rseg = std::atoi(v);
	else if (name == "HP_MUSCL_RSEG") k.muscl_rseg = std::atoi(v);
	else if (name == "HP_INERTIAL_RSEG") k.inertial_rseg = std::atoi(v);
	else if (name == "HP_MARCH2_RSEG") k.march2_rseg = std::atoi(v);
	else if (name == "HP_TAIL_RSEG") k.tail_rseg = std::atoi(v);
	else if (name == "HP_TAIL_PCT") k.tail_pct = std::atoi(v);
	else if (name == "HP_HALO_ROWS") l.halo_rows = std::atol(v);
	else if (name == "HP_NBANDS") l.nbands = std::atoi(v);
	else if (name == "HP_PRINT_TILING") k.print_tiling = true;
	else return false;
	return true;
}

static bool g_first;
static void print_map(const char* kernel, const char* part, const bool made, const TileMap& tm, const unsigned blocks)
{
	std::printf("%s{\"kernel\": \"%s\", \"part\": \"%s\", \"made\": %d", g_first ? "" : ", ", kernel, part, (int)made);
	g_first = false;
	if (made)
		std::printf(", \"nstrips\": %d, \"groups\": %d, \"y_begin\": %ld, \"y_end\": %ld, \"nbands\": %d, \"band_stride\": %ld, \"band_rows\": %d, "
		            "\"rseg\": %d, \"nbig\": %d, \"rseg_tail\": %d, \"ntail\": %d, \"price_lo\": %d, \"price_hi\": %d, \"flip\": %d, \"blocks\": %u",
		            tm.nstrips, tm.groups, tm.y_begin, tm.y_end, tm.nbands, tm.band_stride, tm.band_rows, tm.rseg, tm.nbig, tm.rseg_tail, tm.ntail,
		            tm.price_lo, tm.price_hi, tm.flip, blocks);
	std::printf("}");
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		long cols, rows;
		int precision, cus, strip;
		if (!(in >> cols >> rows >> precision >> cus >> strip)) continue;
		TilingKnobs knobs;
		LaunchKnobs launch;
		std::string kv;
		while (in >> kv) {
			const size_t eq = kv.find('=');
			if (eq == std::string::npos || !set_knob(knobs, launch, kv.substr(0, eq), kv.c_str() + eq + 1)) {
				std::fprintf(stderr, "tiling_probe: unknown knob %s\n", kv.c_str());
				return 2;
			}
		}
		const Tiling t = choose_tiling(cols, rows, precision, cus, knobs);
		std::printf("{\"tiling\": {\"march_rseg\": %d, \"muscl_rseg\": %d, \"inertial_rseg\": %d, \"march_nbands\": %d, \"muscl_nbands\": %d, "
		            "\"inertial_nbands\": %d, \"march_rseg_parts\": %d, \"inertial_rseg_parts\": %d, \"march2_rseg\": %d, \"march2_nbands\": %d, "
		            "\"march2_pays\": %d, \"tall_rseg\": %d, \"tail_rseg\": %d, \"tail_pct\": %d, \"print_tiling\": %d}, \"maps\": [",
		            t.march_rseg, t.muscl_rseg, t.inertial_rseg, t.march_nbands, t.muscl_nbands, t.inertial_nbands, t.march_rseg_parts,
		            t.inertial_rseg_parts, t.march2_rseg, t.march2_nbands, (int)t.march2_pays, t.tall_rseg, t.tail_rseg, t.tail_pct, (int)t.print_tiling);
		g_first = true;
		TileMap tm;
		unsigned blocks = 0;
		bool made;
		const int k1_strips = (int)((cols - 2 + MARCH_COLS - 1) / MARCH_COLS), k2_strips = (int)((cols - 4 + MUSCL_COLS - 1) / MUSCL_COLS);
		const int k2_tail = t.tail_rseg < 8 ? 8 : t.tail_rseg;
		// the whole-domain launches of a single domain: every row but the edge ring is updated and priced
		std::memset(&tm, 0, sizeof tm);
		made = make_tile_map(launch, 1, rows - 1, 1, PART_ALL, k1_strips, t.march_rseg, t.tail_rseg, t.tail_pct, tm, blocks, t.tall_rseg, 1, 0, rows, t.march_nbands);
		print_map("K1", "all", made, tm, blocks);
		if (rows > 4) {            // (a MUSCL-Hancock launch needs updated rows)
			std::memset(&tm, 0, sizeof tm);
			made = make_tile_map(launch, 2, rows - 2, 2, PART_ALL, k2_strips, t.muscl_rseg, k2_tail, t.tail_pct, tm, blocks, 16, 2, 0, rows, t.muscl_nbands);
			print_map("K2", "all", made, tm, blocks);
		}
		std::memset(&tm, 0, sizeof tm);
		made = make_tile_map(launch, 1, rows - 1, 1, PART_ALL, (int)((cols - 2 + MARCH2_COLS - 1) / MARCH2_COLS), t.march2_rseg, t.march2_rseg, 0, tm, blocks,
		                     t.march2_rseg, 0, 0, rows, t.march2_nbands);
		print_map("pair", "all", made, tm, blocks);
		if (strip) {               // the split step of a middle strip with one reach of ghost rows: it owns the rows [g, rows - g)
			const int parts[2] = {PART_INTERIOR, PART_HALO};
			const char* names[2] = {"interior", "halo"};
			for (int i = 0; i < 2; ++i) {
				std::memset(&tm, 0, sizeof tm);
				made = make_tile_map(launch, 1, rows - 1, 1, parts[i], k1_strips, t.march_rseg_parts, t.tail_rseg, t.tail_pct, tm, blocks, t.tall_rseg, 1, 1, rows - 1,
				                     t.march_nbands);
				print_map("K1", names[i], made, tm, blocks);
				std::memset(&tm, 0, sizeof tm);
				made = make_tile_map(launch, 2, rows - 2, 2, parts[i], k2_strips, t.muscl_rseg, k2_tail, t.tail_pct, tm, blocks, 16, 2, 2, rows - 2, t.muscl_nbands);
				print_map("K2", names[i], made, tm, blocks);
			}
		}
		std::printf("]}\n");
	}
	return 0;
}
