// hp_output.hpp -- the output stage on the device: the rasters CDomainCartesian::writeOutputs derives on the host
// (Datasets/CRasterDataset.cpp:185-267) and the domain statistics of the progress log (CDomainCartesian::getVolume,
// CDomainCartesian.cpp:743-760), computed where the state lives.  Part of hp_engine.hip's translation unit, which is built with
// -ffp-contract=off -fno-fast-math: every operation below is a correctly rounded IEEE one (add, multiply, divide, square
// root, compare), so the rasters equal the host derivation (frontend.derive_output) bit for bit.
#pragma once
#include "hp_math.hpp"

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
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)bed[first + k];
		const double depth = z - zb;
		const bool wet = depth > OUT_WET;
		// a dry cell's quotient (by zero, or by a negative depth) is never formed: the divisor is replaced before the division
		const double div = wet ? depth : 1.0;
		if (mask & (1u << OUT_DEPTH)) {
			const double d = depth > 0.0 ? depth : 0.0;
			((O*)t.raster[OUT_DEPTH])[k] = (O)(d < OUT_WET ? OUT_NODATA : d);
		}
		if (mask & (1u << OUT_MAXDEPTH)) {
			const double dm = zmax - zb;
			const double d = dm > 0.0 ? dm : 0.0;
			((O*)t.raster[OUT_MAXDEPTH])[k] = (O)((d < OUT_WET || d <= -9990.0 || d >= 9999.0) ? OUT_NODATA : d);
		}
		if (mask & (1u << OUT_FSL))
			((O*)t.raster[OUT_FSL])[k] = (O)((z < zb + OUT_WET || zb > 9999.0) ? OUT_NODATA : z);
		if (mask & (1u << OUT_MAXFSL))
			((O*)t.raster[OUT_MAXFSL])[k] = (O)((zmax < zb + OUT_WET || zb > 9999.0) ? OUT_NODATA : zmax);
		if (mask & (1u << OUT_DISCHARGE_X))
			((O*)t.raster[OUT_DISCHARGE_X])[k] = (O)(qx * resolution);
		if (mask & (1u << OUT_DISCHARGE_Y))
			((O*)t.raster[OUT_DISCHARGE_Y])[k] = (O)(qy * resolution);
		if (mask & ((1u << OUT_VELOCITY_X) | (1u << OUT_VELOCITY_Y) | (1u << OUT_FROUDE))) {
			const double vx = qx / div, vy = qy / div;
			if (mask & (1u << OUT_VELOCITY_X))
				((O*)t.raster[OUT_VELOCITY_X])[k] = (O)(wet ? vx : OUT_NODATA);
			if (mask & (1u << OUT_VELOCITY_Y))
				((O*)t.raster[OUT_VELOCITY_Y])[k] = (O)(wet ? vy : OUT_NODATA);
			if (mask & (1u << OUT_FROUDE)) {
				const double fr = sqrt_(vx * vx + vy * vy) / sqrt_(9.81 * div);
				((O*)t.raster[OUT_FROUDE])[k] = (O)(wet ? fr : OUT_NODATA);
			}
		}
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
