// hp_peaks.hpp -- the peak tracker: run-long maxima (speed, unit discharge, hazard rating), time of first inundation and
// duration of inundation, kept as fp64 accumulator rasters in device memory and folded from the current state each time the
// host asks for a sample (hp_peaks_sample).  No reference counterpart; closest: the Zmax field the flux kernels carry,
// CLSchemeGodunov.clc.  Part of hp_engine.hip's translation unit, which is built with -ffp-contract=off -fno-fast-math: every operation
// below is a correctly rounded IEEE one (add, multiply, divide, square root, compare), so the accumulators equal the host
// restatement (frontend.PeakTracker) bit for bit.  The conventions are the output stage's (hp_output.hpp): NODATA, the 1e-8
// wet test, the counted-cell rule of domain_stats.
#pragma once
#include "hp_output.hpp"

namespace hp {

constexpr int PEAK_VALUES = 5;                    // HP_PEAK_COUNT (include/hipims_mi.h; hp_observers.hpp asserts the two agree)

enum { PEAK_SPEED, PEAK_UNIT_DISCHARGE, PEAK_HAZARD, PEAK_ARRIVAL_TIME, PEAK_WET_DURATION };

// The tracker's own block in device memory (plain fp64 words).  Sample n reads its t_previous from slot[n & 1] and one thread
// stores the sample's time into slot[(n + 1) & 1], which no thread of that launch reads: every block of a launch sees the same
// t_previous, and it advances exactly once per sample.  The host keeps n.
struct PeakBlock {
	double slot[2];
	double t_first;                               // time of the first sample since enable / reset
	double reserved;
};

struct PeakTargets {
	double*  acc[PEAK_VALUES];                    // [value] -> that value's accumulator raster (NULL: not enabled)
	unsigned mask;                                // bit v: acc[v] is tracked (the same in every lane: a scalar branch per value)
	double   arrival_depth;                       // >= OUT_WET: a cell that is dry in a sample can change nothing
};

// -------------------------------------------------------------------------------------------------
// track_peaks : one sample, one pass over all n cells of the local array (grid-stride; every cell is owned by one thread, no
//     atomics, no reductions: the result does not depend on the launch shape).  Bound by bytes: the State4 (one or two
//     16-byte loads) and the bed of every cell, 40 B in fp64; a cell that is dry in this sample, disabled or a wall touches no
//     accumulator; a wet cell reads each enabled accumulator once (8 B) and stores it only where the value changes (8 B) --
//     still water is wet, so "not larger" has to skip the store as well.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void track_peaks(const State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                   const Scalars<T>* __restrict__ scalars, PeakBlock* __restrict__ block,
                                                   const unsigned sample, const int first, const size_t n, const PeakTargets t)
{
	const unsigned mask = t.mask;
	const double now = (double)scalars->t;        // the device's own "Time", in stream order: what hp_read_scalars would report
	const double dt = now - block->slot[sample & 1u];
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		block->slot[(sample + 1u) & 1u] = now;
		if (first) block->t_first = now;
	}
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
		const State4<T> c = state[k];
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)bed[k];
		const double depth = z - zb;
		// counted as in domain_stats; dry as in the output stage.  Neither kind reads or writes an accumulator
		if (!(zmax > -9999.0) || !(zb <= 9999.0) || !(depth > OUT_WET)) continue;
		if (mask & ((1u << PEAK_SPEED) | (1u << PEAK_HAZARD))) {
			const double vx = qx / depth, vy = qy / depth;
			const double v = sqrt_(vx * vx + vy * vy);
			if (mask & (1u << PEAK_SPEED)) {
				if (v > t.acc[PEAK_SPEED][k]) t.acc[PEAK_SPEED][k] = v;
			}
			if (mask & (1u << PEAK_HAZARD)) {
				const double hz = depth * (v + 0.5);
				if (hz > t.acc[PEAK_HAZARD][k]) t.acc[PEAK_HAZARD][k] = hz;
			}
		}
		if (mask & (1u << PEAK_UNIT_DISCHARGE)) {
			const double q = sqrt_(qx * qx + qy * qy);
			if (q > t.acc[PEAK_UNIT_DISCHARGE][k]) t.acc[PEAK_UNIT_DISCHARGE][k] = q;
		}
		if ((mask & ((1u << PEAK_ARRIVAL_TIME) | (1u << PEAK_WET_DURATION))) && depth > t.arrival_depth) {
			if (mask & (1u << PEAK_ARRIVAL_TIME)) {
				if (t.acc[PEAK_ARRIVAL_TIME][k] == OUT_NODATA) t.acc[PEAK_ARRIVAL_TIME][k] = now;
			}
			if (mask & (1u << PEAK_WET_DURATION)) {
				const double old = t.acc[PEAK_WET_DURATION][k];
				const double sum = (old == OUT_NODATA ? 0.0 : old) + dt;        // right-endpoint rule, added in sample order
				if (sum != old) t.acc[PEAK_WET_DURATION][k] = sum;              // (a repeated time adds 0: nothing to store)
			}
		}
	}
}

// peaks_reset : NODATA into all n accumulator elements (the enabled rasters lie one after the other), the device time into
//     both time slots and t_first.
template <typename T>
__global__ __launch_bounds__(256) void peaks_reset(double* __restrict__ acc, const size_t n, const Scalars<T>* __restrict__ scalars,
                                                   PeakBlock* __restrict__ block)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		const double now = (double)scalars->t;
		block->slot[0] = now; block->slot[1] = now; block->t_first = now; block->reserved = 0.0;
	}
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) acc[k] = OUT_NODATA;
}

// peaks_round : n accumulator elements rounded once to fp32 (hp_peaks_read with element_bytes 4)
__global__ __launch_bounds__(256) void peaks_round(const double* __restrict__ acc, float* __restrict__ out, const size_t n)
{
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) out[k] = (float)acc[k];
}

} // namespace hp
