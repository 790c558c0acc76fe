// hp_bed.hpp -- the moving bed: at listed cells the bed elevation follows a schedule (hp_bed_shape_add / hp_bed_apply).  A SHAPE is
// a list of cells, one target elevation per cell and one progress series {time, fraction} shared by its cells; an apply evaluates
// every shape's fraction from the device's own "Time" scalar, moves the bed of the listed cells between the elevation captured when
// the shape was added (base) and the target, and shifts the cells' levels so that the depth stays.  No reference counterpart: the
// reference's bed is loaded once (CDomainCartesian::loadInitialConditions).
// The arithmetic of the fraction and of the new bed is ONE definition in plain C++ (bed_fraction, bed_level, bed_round below): the
// kernel uses it, tests/bed_probe.cpp includes this file with a host compiler, and frontend.BedShapes restates it in NumPy.  All
// of it is fp64 and uses correctly rounded multiply, add, divide and compare only; nothing is fused: hp_engine.hip's translation
// unit is built with -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  Behind the arithmetic, HIP-free as well and
// in the probe's reach: what hp_bed_shape_add (hp_actors.hpp) does before it touches the device -- its argument checks
// (validate_bed_shape), the layout of the lists' device block (bed_layout) and the block's bytes (bed_image).
#pragma once
#include "../../include/hipims_mi.h"
#include <cstdint>

#ifdef __HIPCC__
#define HP_BED_FN __host__ __device__ __forceinline__
#else
#define HP_BED_FN static inline
#endif

namespace hp {

constexpr unsigned BED_MAX_SHAPES = 64;
constexpr unsigned BED_MAX_SERIES = 4096;                 // entries of one shape's series
constexpr uint64_t BED_MAX_CELLS = 1048576;               // listed cells of all shapes of a domain together
constexpr double   BED_MAX_LEVEL = 9999.0;                // |target| at most this: above it a bed is a closed-edge wall

// -------------------------------------------------------------------------------------------------
// bed_fraction : the progress of a shape at time t.  series = n x {time, fraction}, times strictly increasing, n >= 1.
//     t <= t_0 (or a NaN t) gives f_0, t >= t_last gives f_last; otherwise, in the segment with t_k <= t < t_k+1,
//     f = f_k + (f_k+1 - f_k) * ((t - t_k) / (t_k+1 - t_k)), in that order.  Fractions need not be monotone.
// -------------------------------------------------------------------------------------------------
HP_BED_FN double bed_fraction(const double* series, const unsigned n, const double t)
{
	if (!(t > series[0])) return series[1];
	if (t >= series[2 * (n - 1)]) return series[2 * (n - 1) + 1];
	unsigned lo = 0, hi = n - 1;                          // t_lo <= t < t_hi throughout
	while (hi - lo > 1) {
		const unsigned mid = lo + (hi - lo) / 2;
		if (series[2 * mid] <= t) lo = mid; else hi = mid;
	}
	const double t0 = series[2 * lo], f0 = series[2 * lo + 1], t1 = series[2 * hi], f1 = series[2 * hi + 1];
	const double df = f1 - f0;
	const double s = (t - t0) / (t1 - t0);
	const double step = df * s;
	return f0 + step;
}

// the bed of a cell at fraction f, before it is rounded to the domain's precision.  f >= 1 gives the target itself:
// base + (target - base) need not be the target
HP_BED_FN double bed_level(const double base, const double target, const double f)
{
	if (f <= 0.0) return base;
	if (f >= 1.0) return target;
	const double rise = target - base;
	const double part = f * rise;
	return base + part;
}

// ... and rounded once: b1
template <typename T> HP_BED_FN T bed_round(const double base, const double target, const double f) { return (T)bed_level(base, target, f); }

} // namespace hp

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace hp {

// The host's copies of a domain's lists (BedShapes, hp_domain.hpp)
struct BedHost {
	std::vector<uint64_t> listed;                     // GLOBAL ids of every cell of every shape, sorted: the repeated-cell check
	std::vector<uint64_t> cells;                      // LOCAL ids, shape after shape
	std::vector<double>   target;
	std::vector<unsigned char> shape_of;
	std::vector<double>   series;
	std::vector<unsigned> series_off = {0u};          // [shapes + 1]
};

// -------------------------------------------------------------------------------------------------
// validate_bed_shape : every argument error of hp_bed_shape_add behind the descriptor's own (NULL, ABI size) that needs no device,
//     in the order the entry point has always raised them.  `have`: the domain's lists so far, NULL for a NULL domain -- then only
//     the checks in front of "null domain" run.  On success `listed_after` holds have->listed merged with the new cells.  Returns
//     false with `why` set.
// -------------------------------------------------------------------------------------------------
inline bool validate_bed_shape(const hp_bed_shape_desc_t* desc, const BedHost* have, const uint64_t cols, const uint64_t global_rows,
                               std::vector<uint64_t>& listed_after, std::string& why)
{
	const std::string who = "hp_bed_shape_add";
	if (!desc->cells || !desc->target || !desc->series) { why = who + ": cells / target / series == NULL"; return false; }
	if (desc->series_entries < 1 || desc->series_entries > BED_MAX_SERIES) { why = who + ": series_entries outside 1..4096"; return false; }
	if (desc->cell_count < 1 || desc->cell_count > BED_MAX_CELLS) { why = who + ": cell_count outside 1..1048576"; return false; }
	const uint64_t n = desc->cell_count;
	for (uint64_t k = 0; k < n; ++k)
		if (!std::isfinite(desc->target[k]) || std::fabs(desc->target[k]) > BED_MAX_LEVEL) { why = who + ": target " + std::to_string(k) + " is not a finite elevation of at most 9999"; return false; }
	for (unsigned k = 0; k < desc->series_entries; ++k) {
		const double t = desc->series[2 * k], f = desc->series[2 * k + 1];
		if (!std::isfinite(t) || (k > 0 && !(t > desc->series[2 * k - 2]))) { why = who + ": series entry " + std::to_string(k) + ": times must be finite and strictly increasing"; return false; }
		if (!(f >= 0.0 && f <= 1.0)) { why = who + ": series entry " + std::to_string(k) + ": fraction outside [0, 1]"; return false; }
	}
	std::vector<uint64_t> sorted(desc->cells, desc->cells + n);
	std::sort(sorted.begin(), sorted.end());
	auto twice = std::adjacent_find(sorted.begin(), sorted.end());
	if (twice != sorted.end()) { why = who + ": cell " + std::to_string(*twice) + " is listed twice"; return false; }
	if (!have) return true;
	if (sorted.back() >= cols * global_rows) { why = who + ": cell " + std::to_string(sorted.back()) + " lies outside the grid"; return false; }
	if (have->series_off.size() > BED_MAX_SHAPES) { why = who + ": more than 64 shapes"; return false; }
	if (have->listed.size() + n > BED_MAX_CELLS) { why = who + ": more than 1048576 cells over all shapes"; return false; }
	listed_after.resize(have->listed.size() + (size_t)n);
	std::merge(have->listed.begin(), have->listed.end(), sorted.begin(), sorted.end(), listed_after.begin());
	twice = std::adjacent_find(listed_after.begin(), listed_after.end());
	if (twice != listed_after.end()) { why = who + ": cell " + std::to_string(*twice) + " is listed twice (another shape has it)"; return false; }
	return true;
}

// The device block of the lists of n cells, `pairs` series entries and `shapes` shapes (BedLists points into it), in bytes:
// [cells: n x 8 | target: n x 8 | series: pairs x 16 | base: n elements, to 8 | series_off: (shapes + 1) x 4, to 8 | shape_of: n]
struct BedLayout { size_t cells, target, series, base, series_off, shape_of, bytes; };
inline BedLayout bed_layout(const size_t n, const size_t pairs, const size_t shapes, const size_t esize)
{
	BedLayout l;
	l.cells = 0;
	l.target = l.cells + n * 8;
	l.series = l.target + n * 8;
	l.base = l.series + pairs * 16;
	l.series_off = l.base + (n * esize + 7) / 8 * 8;
	l.shape_of = l.series_off + ((shapes + 1) * 4 + 7) / 8 * 8;
	l.bytes = l.shape_of + std::max<size_t>(n, 1);
	return l;
}

// The block's bytes for the shapes of `old` plus one more, of the m series entries `series`: `cells` and `target` are old's with
// this strip's share of the new shape behind them, `l` the layout of the lot.  (base is the device's to fill: bed_gather)
inline std::vector<unsigned char> bed_image(const BedLayout& l, const BedHost& old, const std::vector<uint64_t>& cells, const std::vector<double>& target,
                                            const double* series, const unsigned m)
{
	const size_t n_old = old.cells.size(), n_all = cells.size(), pairs_old = old.series.size() / 2, shapes = old.series_off.size();
	std::vector<unsigned char> image(l.bytes, 0);
	if (n_all) {
		std::memcpy(image.data() + l.cells, cells.data(), n_all * 8);
		std::memcpy(image.data() + l.target, target.data(), n_all * 8);
		if (n_old) std::memcpy(image.data() + l.shape_of, old.shape_of.data(), n_old);
		std::memset(image.data() + l.shape_of + n_old, (int)(shapes - 1), n_all - n_old);
	}
	if (pairs_old) std::memcpy(image.data() + l.series, old.series.data(), pairs_old * 16);
	std::memcpy(image.data() + l.series + pairs_old * 16, series, (size_t)m * 16);
	std::memcpy(image.data() + l.series_off, old.series_off.data(), shapes * 4);
	const unsigned end = (unsigned)(pairs_old + m);
	std::memcpy(image.data() + l.series_off + shapes * 4, &end, 4);
	return image;
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_math.hpp"         // State4, Scalars

namespace hp {

// The shapes' lists in device memory (one allocation, rewritten by every hp_bed_shape_add).  Cell ids are flat ids of the LOCAL
// array: the host has checked every global id against the grid and dropped the cells of other strips.
struct BedLists {
	const unsigned long long* cells;              // [count]
	const double*             target;             // [count]
	const void*               base;               // [count] elements of the domain's precision: the bed when the cell's shape was added
	const unsigned char*      shape_of;           // [count] the cell's shape
	const double*             series;             // all shapes' {time, fraction} pairs, shape after shape
	const unsigned*           series_off;         // [shapes + 1] entries (pairs) into `series`
	unsigned long long        count;
	unsigned                  shapes;             // 1 .. BED_MAX_SHAPES
};

// What the applies leave for hp_bed_info.  changed[k & 1] counts the cells apply number k changed; apply k clears the other word for
// its successor, so no fill is queued in front of a launch.
struct BedBlock {
	unsigned long long changed[2];
	unsigned long long changed_total;
	double             t_last;                    // the device time of the last apply
};

// -------------------------------------------------------------------------------------------------
// bed_apply : one launch over the listed cells.  Per block the first `shapes` threads form the shapes' fractions into LDS (a binary
//     search each), one barrier, then the cells by grid stride.  A cell is skipped if it is not counted in the sense of domain_stats
//     (Zmax > -9999 and bed <= 9999) or if its new bed b1 equals the stored one b0.  Otherwise Z1 = b1 + (Z0 - b0) (the depth raw:
//     no clamp, no wet test), Zmax1 = Zmax0 > Z1 ? Zmax0 : Z1, Qx and Qy as they are: values widened to fp64, every result rounded
//     once on store.  The state entry is loaded and stored whole (32 B / 16 B: State4 is aligned to its size).  A cell is listed
//     once over all shapes, so no two threads touch the same entry.  The counts are integers: per block one LDS word, then one
//     atomic per counter.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bed_apply(State4<T>* __restrict__ state, T* __restrict__ bed, const Scalars<T>* __restrict__ scalars,
                                                 const BedLists L, BedBlock* __restrict__ block, const unsigned slot)
{
	__shared__ double frac[BED_MAX_SHAPES];
	__shared__ unsigned block_changed;
	const double t = (double)scalars->t;                                          // the device's own "Time", in stream order
	if (threadIdx.x < L.shapes) {
		const unsigned lo = L.series_off[threadIdx.x], hi = L.series_off[threadIdx.x + 1];
		frac[threadIdx.x] = bed_fraction(L.series + 2ull * lo, hi - lo, t);
	}
	if (threadIdx.x == 0) block_changed = 0u;
	if (blockIdx.x == 0 && threadIdx.x == 0) { block->t_last = t; block->changed[slot ^ 1u] = 0ull; }
	__syncthreads();
	const T* __restrict__ base = (const T*)L.base;
	unsigned mine = 0u;
	for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < L.count; k += (unsigned long long)gridDim.x * 256u) {
		const unsigned long long cell = L.cells[k];
		const double f = frac[L.shape_of[k]];
		const T b0_ = bed[cell];
		const T b1_ = bed_round<T>((double)base[k], L.target[k], f);
		State4<T> c = state[cell];
		const double b0 = (double)b0_, b1 = (double)b1_, z0 = (double)c.z, zmax0 = (double)c.zmax;
		const bool counted = zmax0 > -9999.0 && b0 <= 9999.0;                     // as in domain_stats
		if (!counted || b1_ == b0_) continue;
		const double depth = z0 - b0;
		const double z1 = b1 + depth;
		c.z = (T)z1;
		c.zmax = (T)(zmax0 > z1 ? zmax0 : z1);
		state[cell] = c;
		bed[cell] = b1_;
		++mine;
	}
	if (mine) atomicAdd(&block_changed, mine);
	__syncthreads();
	if (threadIdx.x == 0 && block_changed) {
		atomicAdd(&block->changed[slot], (unsigned long long)block_changed);
		atomicAdd(&block->changed_total, (unsigned long long)block_changed);
	}
}

// out[k] = bed[cells[k]]: the capture of a new shape's base (hp_bed_shape_add) and a checkpoint's copy of the listed beds (hp_state_save)
template <typename T>
__global__ __launch_bounds__(256) void bed_gather(const T* __restrict__ bed, const unsigned long long* __restrict__ cells,
                                                  const unsigned long long first, const unsigned long long count, T* __restrict__ out)
{
	for (unsigned long long k = first + (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < first + count; k += (unsigned long long)gridDim.x * 256u)
		out[k] = bed[cells[k]];
}

// bed[cells[k]] = in[k]: hp_state_restore
template <typename T>
__global__ __launch_bounds__(256) void bed_scatter(T* __restrict__ bed, const unsigned long long* __restrict__ cells, const unsigned long long count,
                                                   const T* __restrict__ in)
{
	for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < count; k += (unsigned long long)gridDim.x * 256u)
		bed[cells[k]] = in[k];
}

} // namespace hp
#endif // __HIPCC__
