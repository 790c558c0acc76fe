// hp_tiling.hpp -- how a flux launch is cut into row bands and tiles: the TileMap the kernels read, the policy that picks
// tile heights and band counts for a domain (choose_tiling), and the TileMap of one launch (make_tile_map).  Host arithmetic
// only -- no HIP header or type, no getenv (hp_engine.hip: tiling_knobs fills TilingKnobs) --, so that a plain C++17 translation
// unit can include it: tests/tiling_probe.cpp pins its decisions against tests/tiling_table.json without a GPU.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace hp {

constexpr int MARCH_COLS = 62;          // godunov_march / inertial_march: updated columns per wavefront (lanes 1..62)
constexpr int MARCH2_COLS = 60;         // godunov_march2: updated columns per wavefront (lanes 2..61)
constexpr int MUSCL_COLS = 60;          // muscl_march

// How one launch's blocks map to tiles.  A launch covers the updated rows [y_begin, y_end) of the domain (all of them,
// or the interior / one halo block of a strip-decomposed step: hp_engine.hip).  The rows are cut into 8 bands, one per
// XCD (blocks are dealt round-robin to the XCDs, so blockIdx & 7 IS the XCD: its blocks walk one contiguous band and
// the halo rows of neighbouring tiles are hits in that XCD's L2).  Inside a band the first `nbig` row segments are
// `rseg` rows tall and the last `ntail` segments only `rseg_tail`: blocks start in blockIdx order, so the short
// tiles are what is running when the band drains, and the tail of the launch is one SHORT tile long instead of one
// tall tile (a tall tile lasts ~48 us at 4096^2 -- 18 % of the launch, measured as the intercept of
// time-vs-cells between 4096^2 and 16384 x 8192).
struct TileMap {
	int  nstrips, groups;        // 62/60-column strips of the grid, and 4-wave groups of them
	long y_begin, y_end;         // updated rows covered by this launch
	int  nbands;                 // 8 (one band per XCD); 2 for the halo launch of a strip (south block, north block)
	long band_stride;            // distance between band starts (= band_rows, except for the halo launch)
	int  band_rows;              // rows per band
	int  rseg, nbig;             // tall segments per band
	int  rseg_tail, ntail;       // short segments per band (after the tall ones)
	int  price_lo, price_hi;     // rows whose cells the fused CFL epilogue prices: the rows this rank OWNS (a strip with two
	                             // reaches of ghost rows also updates rows it does not own, hp_engine.hip: strip loop); 32-bit so
	                             // that the per-row test is two scalar compares
	int  flip;                   // this launch visits the tiles of every band from the top down (hp_engine.hip: sweep_flip)
};

// The tuning knobs of the tiling as plain values; the defaults are what an unset variable means (0 / -1: unset), the heights'
// range checks are force_heights'.  hp_engine.hip reads them from the environment: TilingKnobs at every hp_domain_create,
// LaunchKnobs -- what make_tile_map takes -- once per process.
struct TilingKnobs {
	bool   rseg_refine = true;                        // HP_RSEG_REFINE=0: no fine-tuning of a one-round launch's tile height
	bool   search = true, search_pair = true;         // HP_TILING_SEARCH=0: no one-round (bands, rows) search for K1 / K6; for the pair kernel
	bool   search_f32 = false;                        // HP_TILING_SEARCH_F32 set: the K1 / K6 search for fp32 domains as well
	double tiling_fill = 3.5, march2_fill = 4.0;      // HP_TILING_FILL, HP_MARCH2_FILL: a K1 / K6 / pair-kernel tile's fixed cost in row-times
	int    march_rseg = 0, muscl_rseg = 0, inertial_rseg = 0, march2_rseg = 0;   // HP_*_RSEG: forced tile heights
	int    tail_rseg = 0, tail_pct = -1;              // HP_TAIL_RSEG, HP_TAIL_PCT
	bool   print_tiling = false;                      // HP_PRINT_TILING set
};
struct LaunchKnobs {
	long   halo_rows = 0;                             // HP_HALO_ROWS: rows of the halo part of a split step
	int    nbands = 0;                                // HP_NBANDS: forced row bands of a whole-domain launch
};

// What choose_tiling decides for one domain.
struct Tiling {
	int  march_rseg = 16;                 // rows per wavefront tile of godunov_march
	int  muscl_rseg = 32;                 // ... of muscl_march (two warm-up rows per tile)
	int  inertial_rseg = 32;              // ... of inertial_march
	int  march_nbands = 8, muscl_nbands = 8, inertial_nbands = 8;   // row bands of a whole-domain launch
	int  march_rseg_parts = 16, inertial_rseg_parts = 16;            // tile height of the interior / halo parts of a split step (8 / 2 bands: the classic height)
	int  march2_rseg = 24, march2_nbands = 8;                        // the two-iterations kernel: tile height; row bands (one-round grids: searched)
	bool march2_pays = false;             // the grid is big enough for it
	int  tall_rseg = 18;                  // K1/K6 tile height where an XCD band has >= 256 rows (16 if a knob is set)
	int  tail_rseg = 8, tail_pct = 0;     // optional short tiles for the last tail_pct % of each XCD band (measured: no gain)
	bool print_tiling = false;
};

// The one-round search.  What a launch whose blocks all fit the chip at once really lasts is what its MOST LOADED CU has
// to walk: blocks are dealt to the CUs layer by layer (block b lands on CU b mod cus while every CU has room), a block costs
// its rows plus `fill` rows of pipeline fill, and the blocks of one CU share its SIMDs.  8 bands x groups x segments only
// offers coarse block counts (680 blocks on 256 CUs: 168 CUs walk three 13-row tiles, 88 walk two); with another number
// of bands the last segment of each band can be a SHORT tile, and "two tall + one short on every CU" (15 bands, 15 + 15 + 5
// rows: 765 blocks) measured 39.1 us per iteration on the 4096 x 514 strip against 43.4
// (profiles/r04b_band_sweep_4096x514.txt).  The search simulates the dealing for every (bands, rows) pair of the given
// ranges that fits `slots` blocks and takes the cheapest; a CU with fewer than three resident blocks hides less latency
// (2 blocks: +20 %, 1 block: +60 %, fitted on the same sweep).  nbands == 0: no pair fits.
struct Dealing { int nbands = 0, rseg = 0; };
inline Dealing search_dealing(const long updated_rows, const long groups, const int cus, const long slots, const int nb_lo, const int nb_hi,
                              const int r_lo, const int r_hi, const double fill, const bool nearest_to_8_bands)
{
	Dealing best;
	double best_cost = 1e30;
	long best_pref = -2;
	std::vector<double> load((size_t)cus);
	std::vector<int> count((size_t)cus);
	for (int nb = nb_lo; nb <= nb_hi; ++nb) {
		const long brows = (updated_rows + nb - 1) / nb;
		for (int r = r_lo; r <= r_hi && r <= brows; ++r) {
			const long nseg = (brows + r - 1) / r, blocks = (long)nb * groups * nseg;
			if (blocks > slots) continue;
			std::fill(load.begin(), load.end(), 0.0);
			std::fill(count.begin(), count.end(), 0);
			for (long b = 0; b < blocks; ++b) {                  // tile_rows() of hp_kernels.hpp
				const long band = b % nb, i = b / nb, seg = i / groups;
				const long y0 = band * brows + seg * r;
				const long h = std::min(y0 + r, std::min(updated_rows, (band + 1) * brows)) - y0;
				if (h <= 0) continue;
				load[(size_t)(b % cus)] += (double)h + fill;
				count[(size_t)(b % cus)] += 1;
			}
			double worst = 0.0;
			for (int c = 0; c < cus; ++c)
				worst = std::max(worst, load[(size_t)c] * (count[(size_t)c] >= 3 ? 1.0 : count[(size_t)c] == 2 ? 1.2 : 1.6));
			// Ties -- the same rows and the same number of tiles on every CU, cut differently (37 rows as 16 + 16 + 5, 15 + 15 + 7,
			// 14 + 14 + 9 ...): measured over eight one-round shapes (profiles/r05fp_tie_sweep.txt), the pair kernel wants the LAST
			// tile of a band as tall as it can be without exceeding half a full tile -- 15 + 15 + 7 is 4 % ahead of 16 + 16 + 5 and
			// 6 % ahead of 13 + 13 + 11 on the 4096 x 514 strip (30.0 against 31.4 / 32.0 us), 11 + 11 + 5 6 % ahead of 12 + 12 + 3
			// on 3072 x 514 -- and otherwise the taller tiles.  K1 the same (round 5; on the 4096 x 514 strip: 14 + 14 + 7 33.3 us,
			// 13 + 13 + 9 33.1, round 4's 15 + 15 + 5 34.3, profiles/r05fq_*), and after the taller tiles (`nearest_to_8_bands`) the
			// tiling nearest to the 8-band one, whose bands keep to their XCD's L2.
			// (bands of two or three tiles: with more the rule made 1448^2 slower)
			const long last = brows - (nseg - 1) * r;
			const long pref = (nseg >= 2 && nseg <= 3 && 2 * last <= r) ? last : -1;
			if (worst < best_cost - 1e-9 || (worst < best_cost + 1e-9 && (pref > best_pref || (pref == best_pref &&
			    (r > best.rseg || (nearest_to_8_bands && r == best.rseg && std::abs(nb - 8) < std::abs(best.nbands - 8))))))) {
				best_cost = worst; best.nbands = nb; best.rseg = r; best_pref = pref;
			}
		}
	}
	return best;
}

// Tile heights and band counts of a cols x rows domain on a device of `cus` compute units.
// Tile height: a wavefront marches its tile's rows one after the other, so a grid that yields few tiles is bound
// by that serial walk, not by bandwidth (342 x 195: 35 us per step at 16 rows, 12 us at 2).  Take the tallest
// tile that still gives every CU some blocks (tools/small_grid_probe.py: 4096^2 and 2048^2 want 16, 1024^2 8,
// 512^2 4, the 342 x 195 example 2).
inline Tiling pick_tiling(const long cols, const long rows, const int precision, const int cus, const TilingKnobs& knobs)
{
	Tiling t;
	t.print_tiling = knobs.print_tiling;
	auto pick = [&](long updated_rows, long updated_cols, int tile_cols, int tallest, int shortest, int blocks_per_cu, int& nbands_out, bool searchable,
	                int* classic_out = nullptr) {
		const long groups = ((updated_cols + tile_cols - 1) / tile_cols + 3) / 4;
		nbands_out = 8;
		int rseg = tallest;
		while (rseg > shortest && groups * ((updated_rows + rseg - 1) / rseg) < 350) rseg /= 2;
		if (rseg < shortest) rseg = shortest;
		// Round 3: a launch whose blocks all fit the chip at once (a row strip of a strong-scaling run: 4096 x 514 is 544
		// tiles of 16 rows on 768 block slots) lasts as long as ONE tile does, so the shortest tile that still fits in one
		// round wins: 13-row tiles put that strip into 680 blocks (56 -> 51 us per iteration).  Fine-tune within
		// (rseg/2, rseg] where the halving above left a middle-sized tile; launches of more than one round are left alone
		// (tools/history/r03k.sh: 2048^2, 4096 x 1026 and 8192 x 514 lose 0-9 % with shorter tiles).
		if (knobs.rseg_refine && rseg >= 8) {
			const long band_rows = (updated_rows + 7) / 8, slots = (long)cus * blocks_per_cu;
			auto cost = [&](int r) {
				const long blocks = groups * 8 * ((band_rows + r - 1) / r);
				return ((blocks + slots - 1) / slots) * (long)(2 * r + 7);        // rounds x (rows + 3.5), doubled to stay integral
			};
			if (groups * 8 * ((band_rows + rseg - 1) / rseg) <= slots) {        // measured (profiles/r03k): no gain beyond one round
				int best = rseg;
				for (int r = rseg - 1; r > rseg / 2; --r) if (cost(r) < cost(best)) best = r;
				rseg = best;
				// (Round 4, search_dealing: the searched height is only right TOGETHER with its band count, which only a whole-domain launch gets: the interior /
				// halo parts of a split step keep the classic height -- ADVICE r04)
				if (classic_out) *classic_out = rseg;
				if (knobs.search && searchable) {
					// a tile's fixed cost in row-times: 3.5 for fp64 K1 / K6 (the pipeline fill and the extra south face)
					const Dealing best_deal = search_dealing(updated_rows, groups, cus, slots, 1, 32, 4, 64, knobs.tiling_fill, true);
					if (best_deal.nbands > 0) { nbands_out = best_deal.nbands; rseg = best_deal.rseg; }
				}
			}
		}
		return rseg;
	};
	// fp32 (round 4, profiles/r04za_rseg_f32.txt, r04z_band_sweep_f32_shapes.txt): a tile's fill and extra south face want tall
	// tiles, the dispatcher wants many -- 32 rows is best only where that still leaves six rounds of blocks (8192^2: 6.8); below
	// that shorter tiles win by more than the fill costs: 4096^2 S-DAM 0.143 -> 0.129 ms and S-RAIN 0.180 -> 0.168 at 12 rows,
	// the 8192 x 1026 strip of config C5 0.113 -> 0.089 ms (S-RAIN) and 83 -> 66 us (S-DAM); 8 rows lose again.  (Round 2's "32
	// rows, 13-47 % ahead of 16" was measured on kernels with a dearer fill.)  fp64 is flat from 10 to 20 rows.
	// fp64 (profiles/r04zc_rseg_f64_shapes.txt): flat from 10 to 20 rows where a launch is many rounds (4096^2, 16384 x 1026); between
	// one round and 2.5 (2048^2, 4096 x 1026, 8192 x 1026 ...) 12 rows are 5-9 % ahead of 16 for K1, 10 rows 5-7 % ahead of 12 for K2.
	const bool f32 = precision == 4;
	auto tallest_by_rounds = [&](long updated_rows, long updated_cols, int tile_cols, int blocks_per_cu, std::initializer_list<int> tall,
	                             double rounds, int otherwise) {
		const long groups = ((updated_cols + tile_cols - 1) / tile_cols + 3) / 4, band_rows = (updated_rows + 7) / 8;
		// (fp64: a launch that fits the chip in about ONE round at the classic height belongs to the one-round logic inside pick();
		// the 4096 x 516 MUSCL strip, 1.1 rounds at 12 rows, measured 3 % behind with 10)
		if (!f32 && (double)(groups * 8 * ((band_rows + *tall.begin() - 1) / *tall.begin())) <= 1.25 * cus * blocks_per_cu) return *tall.begin();
		for (int r : tall)
			if ((double)(groups * 8 * ((band_rows + r - 1) / r)) >= rounds * cus * blocks_per_cu) return r;
		return otherwise;
	};
	const int k1_tallest = f32 ? tallest_by_rounds(rows - 2, cols - 2, MARCH_COLS, 5, {32, 24, 16}, 6.0, 12)
	                           : tallest_by_rounds(rows - 2, cols - 2, MARCH_COLS, 3, {16}, 2.5, 12);
	const int k2_tallest = f32 ? tallest_by_rounds(rows - 4, cols - 4, MUSCL_COLS, 4, {32, 24, 16}, 6.0, 12)
	                           : tallest_by_rounds(rows - 4, cols - 4, MUSCL_COLS, 3, {12}, 3.0, 10);
	int classic = 0;
	t.march_rseg    = pick(rows - 2, cols - 2, MARCH_COLS, k1_tallest, 2, f32 ? 5 : 3, t.march_nbands,
	                       !f32 || knobs.search_f32, &classic);      // (fp32: 8192 x 1026 measured 83.2 -> 84.4 us with the searched tiling: its fill is not 3.5 rows)
	t.march_rseg_parts = classic > 0 ? classic : t.march_rseg;
	t.inertial_rseg = t.march_rseg; t.inertial_nbands = t.march_nbands; t.inertial_rseg_parts = t.march_rseg_parts;
	// K2 after the inert-row cut (round 2): a tile of still water or dry land costs a fifth of a tile on the flood front,
	// so fp64 wants more, shorter tiles for the dispatcher to balance (16-20 rows: 0.319 ms against 0.355 at 32 on the
	// 4096^2 dam break, 0.355 against 0.395 on the developed flood, +2-5 % at 8192^2 and 16384 x 1028)
	// (round 4, profiles/r04l_k2_rseg.txt: 12 rows: the 4096^2 dam break 0.300 -> 0.287 ms, developed flood 0.343 -> 0.340, 2048^2 -1.4 %,
	// 8192^2 +0.6 %, every tile live +1.7 %; 10 and below lose again; fp32: as K1 -- 4096^2 dam break 0.192 -> 0.161 ms at 12 rows)
	t.muscl_rseg    = pick(rows - 4, cols - 4, MUSCL_COLS, k2_tallest, 4, f32 ? 4 : 3, t.muscl_nbands,
	                       false);                     // (K2's tiles differ fivefold in cost -- inert rows --: the searched tiling lost 20 % on the 4096 x 514 dam break)
	if (t.muscl_rseg < 4) t.muscl_rseg = 4;
	{
		// the two-iterations kernel: the tallest tile that leaves four rounds of blocks (three 4-wave blocks per CU); worth taking at
		// all from two rounds at 12-row tiles (profiles/r05n_two_step.txt)
		const long groups = ((cols - 2 + MARCH2_COLS - 1) / MARCH2_COLS + 3) / 4, band_rows = (rows - 2 + 7) / 8;
		const long slots = (long)cus * 3;
		auto blocks_at = [&](int r) { return groups * 8 * ((band_rows + r - 1) / r); };
		t.march2_rseg = 12;
		for (int r : {32, 24, 18}) if (blocks_at(r) >= 4 * slots) { t.march2_rseg = r; break; }
		t.march2_pays = blocks_at(12) >= 2 * slots;
		// One round of blocks (the 4096 x 514 strip of a strong-scaling run): as for K1 (pick: knobs.search), what such a launch
		// lasts is what its most loaded CU walks -- (bands, rows) by simulating the dealing, a tile costing its rows plus the two
		// extra first-step rows and the pipeline fill.  profiles/r05u_strip_pair_sweep.txt: 14 bands x 15 rows 31.6 us per iteration
		// against 33.7 in single iterations and 36.0 with 8 bands x 12 rows; taken from 1.5 M cells on (below: untested).
		if (!t.march2_pays && knobs.search_pair && (size_t)cols * (size_t)rows >= 1500000 && blocks_at(12) >= slots / 2) {
			// (at least a band per XCD: 4 bands x 14 rows lost 2 % at 1448^2)
			const Dealing best = search_dealing(rows - 2, groups, cus, slots, 8, 32, 8, 32, knobs.march2_fill, false);
			if (best.nbands > 0) { t.march2_rseg = best.rseg; t.march2_nbands = best.nbands; t.march2_pays = true; }
		}
	}
	return t;
}

// tuning knobs: forced rows per wavefront tile (HP_PRINT_TILING's first line shows K1 / K6 and K2 as picked, before this)
inline void force_heights(Tiling& t, const TilingKnobs& knobs)
{
	if (knobs.march_rseg >= 1 && knobs.march_rseg <= 64) { t.march_rseg = t.march_rseg_parts = knobs.march_rseg; t.tall_rseg = 16; }   // a forced 16 stays 16
	if (knobs.march2_rseg >= 2 && knobs.march2_rseg <= 32) t.march2_rseg = knobs.march2_rseg;
	if (knobs.tail_rseg >= 1 && knobs.tail_rseg <= 64) t.tail_rseg = knobs.tail_rseg;
	if (knobs.tail_pct >= 0 && knobs.tail_pct <= 100) t.tail_pct = knobs.tail_pct;
	if (knobs.inertial_rseg >= 1 && knobs.inertial_rseg <= 64) { t.inertial_rseg = t.inertial_rseg_parts = knobs.inertial_rseg; t.tall_rseg = 16; }
	if (knobs.muscl_rseg >= 1 && knobs.muscl_rseg <= 4096) t.muscl_rseg = knobs.muscl_rseg;
}

inline Tiling choose_tiling(const long cols, const long rows, const int precision, const int cus, const TilingKnobs& knobs)
{
	Tiling t = pick_tiling(cols, rows, precision, cus, knobs);
	force_heights(t, knobs);
	return t;
}

// a wavefront addresses its tile through a buffer resource whose range field is 31 bits wide: the tile's rows
// (segment + halo rows) must fit in it
inline bool tiles_addressable(const Tiling& t, const long cols, const int precision)
{
	const int rseg_max = std::max(std::max(t.march_rseg, t.march2_rseg), std::max(t.muscl_rseg, t.inertial_rseg));
	return (double)(rseg_max + 4) * (double)cols * 4.0 * (double)precision < 2147483647.0;
}

// Which rows of the domain one launch covers
enum { PART_ALL = 0, PART_HALO = 1, PART_INTERIOR = 2 };

// Row ranges of the three parts.  [lo, hi) are the updated rows of the domain; with the halo overlap the `halo` rows
// next to each ghost block (one tile height, at least the g rows the neighbours need) form the halo part -- a south
// and a north block, covered by ONE launch with two bands -- and the rest the interior part.  A domain too thin for
// an interior part runs whole in the halo part.
struct RowRange { long lo, hi; };

// TileMap of one launch: 8 XCD bands over [lo, hi), tall tiles first and optionally short tiles
// for the last `tail_pct` percent of each band; or, for the halo part, the two blocks of `halo` rows as two bands.
inline bool make_tile_map(const LaunchKnobs& knobs, long lo, long hi, int g, int part, int nstrips, int rseg, int rseg_tail, int tail_pct,
                          TileMap& tm, unsigned& blocks, int rseg_tall = 16, long need = 0, long price_lo = 0, long price_hi = 0x7fffffffL,
                          int nbands = 8)
{
	if (need < g) need = g;                                             // rows at each end that a strip neighbour is sent
	const long halo = knobs.halo_rows >= need ? knobs.halo_rows : (rseg > need ? rseg : need);
	tm.price_lo = (int)price_lo; tm.price_hi = (int)(price_hi < 0x7fffffffL ? price_hi : 0x7fffffffL);
	tm.flip = 0;
	const bool can_split = hi - lo > 2 * halo;
	tm.nstrips = nstrips;
	tm.groups = (nstrips + 3) / 4;
	if (part == PART_HALO && can_split) {
		tm.y_begin = lo; tm.y_end = hi;
		tm.nbands = 2; tm.band_stride = (hi - halo) - lo; tm.band_rows = (int)halo;
		tm.rseg = rseg < tm.band_rows ? rseg : tm.band_rows;
		tm.nbig = (tm.band_rows + tm.rseg - 1) / tm.rseg;
		tm.rseg_tail = rseg_tail; tm.ntail = 0;
		blocks = 2u * (unsigned)(tm.groups * tm.nbig);
		return true;
	}
	if (part == PART_INTERIOR) {
		if (!can_split) return false;                                   // the halo launch took everything
		lo += halo; hi -= halo;
	}
	tm.y_begin = lo; tm.y_end = hi;
	const long rows = hi - lo;
	// Row bands: 8, one per XCD -- or, for a whole-domain launch that fits the chip in ONE round, the number the tiling
	// search of choose_tiling found (such a launch is bound by its most loaded CU, and 8 x groups x segments
	// only offers coarse block counts).  HP_NBANDS forces a number (tools/history/r04_band_sweep.py).
	tm.nbands = part != PART_ALL ? 8 : (knobs.nbands >= 1 && knobs.nbands <= 64 ? knobs.nbands : (nbands >= 1 && nbands <= 64 ? nbands : 8));
	tm.band_rows = (int)((rows + tm.nbands - 1) / tm.nbands);
	tm.band_stride = tm.band_rows;
	// K1/K6 on tall bands: 18-row tiles measured 1.9 % / 2.8 % ahead of 16 at 4096^2 (band of 512 rows) and 0.6 % at
	// 8192 x 2050 (256), but 3 % behind at 16384 x 1026 (128 rows = eight exact 16-row tiles); interleaved repeats
	// on one box, tools/rseg_fine_sweep*.sh
	if (rseg == 16 && g == 1 && tm.band_rows >= 256) rseg = rseg_tall;
	tm.rseg = rseg < tm.band_rows ? rseg : tm.band_rows;
	tm.rseg_tail = rseg_tail;
	if (rseg_tail >= tm.rseg || tail_pct <= 0) {
		tm.nbig = (tm.band_rows + tm.rseg - 1) / tm.rseg;
		tm.ntail = 0;
	} else {
		const int tail_rows = (int)((long)tm.band_rows * tail_pct / 100);
		tm.nbig = (tm.band_rows - tail_rows + tm.rseg - 1) / tm.rseg;
		const int rest = tm.band_rows - tm.nbig * tm.rseg;
		tm.ntail = rest > 0 ? (rest + rseg_tail - 1) / rseg_tail : 0;
	}
	blocks = (unsigned)tm.nbands * (unsigned)(tm.groups * (tm.nbig + tm.ntail));
	return true;
}

} // namespace hp
