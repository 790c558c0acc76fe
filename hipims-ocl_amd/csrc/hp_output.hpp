// hp_output.hpp -- the output stage on the device: the rasters CDomainCartesian::writeOutputs derives on the host
// (Datasets/CRasterDataset.cpp:185-267) and the domain statistics of the progress log (CDomainCartesian::getVolume,
// CDomainCartesian.cpp:743-760), computed where the state lives.  Part of hp_engine.hip's translation unit, which is built with
// -ffp-contract=off -fno-fast-math: every operation below is a correctly rounded IEEE one (add, multiply, divide, square
// root, compare), so the rasters equal the host derivation (frontend.derive_output) bit for bit.
#pragma once
#include "hp_math.hpp"
#include <type_traits>

namespace hp {

constexpr int    OUT_VALUES = 9;                  // HP_OUT_COUNT (include/hipims_mi.h; hp_observers.hpp asserts the two agree)
constexpr double OUT_NODATA = -9999.0;
constexpr double OUT_WET    = 1e-8;               // CRasterDataset.cpp's threshold: not the scheme's dryThreshold

enum { OUT_DEPTH, OUT_MAXDEPTH, OUT_FSL, OUT_MAXFSL, OUT_DISCHARGE_X, OUT_DISCHARGE_Y, OUT_VELOCITY_X, OUT_VELOCITY_Y, OUT_FROUDE };

struct DeriveTargets {
	void*    raster[OUT_VALUES];                  // [value] -> first element of that value's raster for this launch's first cell
	unsigned mask;                                // bit v: raster[v] is written (the same in every lane: a scalar branch per value)
};

// -------------------------------------------------------------------------------------------------
// The per-cell value of every HP_OUT_* code in fp64, before any rounding: the one definition derive_rasters (which stores it)
// and overview_blocks (hp_overview.hpp, which aggregates it over blocks) share.  out_cell widens the cell and forms what the
// values have in common; out_value<V> is value V of that cell, NODATA where CRasterDataset.cpp masks it.
// -------------------------------------------------------------------------------------------------
struct OutCell {
	double z, zmax, qx, qy, zb;
	double depth, div;                            // Z - zb; the velocities' divisor
	double vx, vy;                                // Q / div (formed only where a velocity or the Froude number is asked for)
	bool   wet;                                   // depth > OUT_WET
};

constexpr unsigned OUT_NEEDS_VELOCITY = (1u << OUT_VELOCITY_X) | (1u << OUT_VELOCITY_Y) | (1u << OUT_FROUDE);

template <typename T>
__device__ __forceinline__ OutCell out_cell(const State4<T>& c, const T bed, const bool velocity)
{
	OutCell o;
	o.z = (double)c.z; o.zmax = (double)c.zmax; o.qx = (double)c.qx; o.qy = (double)c.qy;
	o.zb = (double)bed;
	o.depth = o.z - o.zb;
	o.wet = o.depth > OUT_WET;
	// a dry cell's quotient (by zero, or by a negative depth) is never formed: the divisor is replaced before the division
	o.div = o.wet ? o.depth : 1.0;
	o.vx = o.vy = 0.0;
	if (velocity) { o.vx = o.qx / o.div; o.vy = o.qy / o.div; }
	return o;
}

template <int V>
__device__ __forceinline__ double out_value(const OutCell& o, const double resolution)
{
	if constexpr (V == OUT_DEPTH) {
		const double d = o.depth > 0.0 ? o.depth : 0.0;
		return d < OUT_WET ? OUT_NODATA : d;
	} else if constexpr (V == OUT_MAXDEPTH) {
		const double dm = o.zmax - o.zb;
		const double d = dm > 0.0 ? dm : 0.0;
		return (d < OUT_WET || d <= -9990.0 || d >= 9999.0) ? OUT_NODATA : d;
	} else if constexpr (V == OUT_FSL) {
		return (o.z < o.zb + OUT_WET || o.zb > 9999.0) ? OUT_NODATA : o.z;
	} else if constexpr (V == OUT_MAXFSL) {
		return (o.zmax < o.zb + OUT_WET || o.zb > 9999.0) ? OUT_NODATA : o.zmax;
	} else if constexpr (V == OUT_DISCHARGE_X) {
		return o.qx * resolution;
	} else if constexpr (V == OUT_DISCHARGE_Y) {
		return o.qy * resolution;
	} else if constexpr (V == OUT_VELOCITY_X) {
		return o.wet ? o.vx : OUT_NODATA;
	} else if constexpr (V == OUT_VELOCITY_Y) {
		return o.wet ? o.vy : OUT_NODATA;
	} else {
		static_assert(V == OUT_FROUDE, "unknown HP_OUT_* code");
		const double fr = sqrt_(o.vx * o.vx + o.vy * o.vy) / sqrt_(9.81 * o.div);
		return o.wet ? fr : OUT_NODATA;
	}
}

// f(integral_constant<int, V>) for every value V whose bit is set in `mask` (the same in every lane: a scalar branch per value)
template <int V = 0, typename F>
__device__ __forceinline__ void out_for_each(const unsigned mask, F&& f)
{
	if constexpr (V < OUT_VALUES) {
		if (mask & (1u << V)) f(std::integral_constant<int, V>{});
		out_for_each<V + 1>(mask, f);
	}
}

// -------------------------------------------------------------------------------------------------
// derive_rasters : one pass over cells [first, first + n) (whole rows of the local array, so the range is contiguous).
//     Every cell's State4 (one or two 16-byte loads) and bed are read once; each selected raster gets one coalesced
//     store per wave (8 or 4 bytes a lane).  Bound by bytes: 40 B read + 8 B per raster written per fp64 cell.
//     T = the domain's precision (values are widened to fp64 first, as derive_output's astype(np.float64) does),
//     O = the raster's element type: the fp64 result, or that result rounded once to fp32.
// -------------------------------------------------------------------------------------------------
template <typename T, typename O>
__global__ __launch_bounds__(256) void derive_rasters(const State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                      const size_t first, const size_t n, const double resolution,
                                                      const DeriveTargets t)
{
	const unsigned mask = t.mask;
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
		const State4<T> c = state[first + k];
		const OutCell o = out_cell(c, bed[first + k], (mask & OUT_NEEDS_VELOCITY) != 0);
		out_for_each(mask, [&](auto v) { constexpr int V = decltype(v)::value; ((O*)t.raster[V])[k] = (O)out_value<V>(o, resolution); });
	}
}

// -------------------------------------------------------------------------------------------------
// domain_stats : cells, wet cells, volume of water, largest depth and speed (with the cell of each) over a row range.
//     Deterministic: a thread owns the cells its grid-stride visits (fixed by the launch shape, which is a function of
//     the range alone), the block folds its 256 partials over a fixed tree in LDS, and domain_stats_fold -- one block,
//     a second launch -- folds the block partials the same way.  No floating-point atomics; the same state gives the
//     same bits.  Maxima: the larger value wins, equal values go to the lower cell id.
// -------------------------------------------------------------------------------------------------
struct StatsPart {
	unsigned long long cells, wet;
	double             sum;                       // sum of max(0, Z - zb) over counted cells (metres; x dx^2 on the host)
	double             max_depth, max_speed;      // -1: no cell yet
	unsigned long long depth_cell, speed_cell;    // ~0: no cell yet
};

constexpr int STATS_MAX_BLOCKS = 1024;

__device__ __forceinline__ void stats_empty(StatsPart& a)
{
	a.cells = a.wet = 0; a.sum = 0.0; a.max_depth = a.max_speed = -1.0; a.depth_cell = a.speed_cell = ~0ull;
}

__device__ __forceinline__ void stats_merge(StatsPart& a, const StatsPart& b)
{
	a.cells += b.cells; a.wet += b.wet; a.sum = a.sum + b.sum;
	if (b.max_depth > a.max_depth || (b.max_depth == a.max_depth && b.depth_cell < a.depth_cell)) { a.max_depth = b.max_depth; a.depth_cell = b.depth_cell; }
	if (b.max_speed > a.max_speed || (b.max_speed == a.max_speed && b.speed_cell < a.speed_cell)) { a.max_speed = b.max_speed; a.speed_cell = b.speed_cell; }
}

__device__ __forceinline__ void stats_block_fold(StatsPart& mine, StatsPart* __restrict__ out)
{
	__shared__ StatsPart part[256];
	part[threadIdx.x] = mine;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) stats_merge(part[threadIdx.x], part[threadIdx.x + s]);
		__syncthreads();
	}
	if (threadIdx.x == 0) *out = part[0];
}

template <typename T>
__global__ __launch_bounds__(256) void domain_stats(const State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                    const size_t first, const size_t n, StatsPart* __restrict__ partial)
{
	StatsPart a;
	stats_empty(a);
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
		const size_t i = first + k;
		const State4<T> c = state[i];
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)bed[i];
		// counted: not disabled (the flux kernels' own test, hp_math.hpp: zmax > -9999) and not a closed-edge wall (bed 9999.9)
		if (!(zmax > -9999.0) || !(zb <= 9999.0)) continue;
		const double depth = z - zb;
		const double d = depth > 0.0 ? depth : 0.0;
		a.cells += 1;
		a.sum = a.sum + d;
		if (d > a.max_depth) { a.max_depth = d; a.depth_cell = i; }        // (ids rise along a thread's walk: the first one stays)
		if (depth > OUT_WET) {
			a.wet += 1;
			const double vx = qx / depth, vy = qy / depth;
			const double sp = sqrt_(vx * vx + vy * vy);                      // the froude raster's numerator
			if (sp > a.max_speed) { a.max_speed = sp; a.speed_cell = i; }
		}
	}
	stats_block_fold(a, partial + blockIdx.x);
}

__global__ __launch_bounds__(256) void domain_stats_fold(const StatsPart* __restrict__ partial, const int count, StatsPart* __restrict__ out)
{
	StatsPart a;
	stats_empty(a);
	for (int k = threadIdx.x; k < count; k += 256) stats_merge(a, partial[k]);
	stats_block_fold(a, out);
}

} // namespace hp
