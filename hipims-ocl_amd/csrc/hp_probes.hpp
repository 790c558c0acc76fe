// hp_probes.hpp -- the probe recorder: time series at gauge cells (stage, depth, unit discharge) and the discharge through
// cross-sections (lists of cells with a signed weight pair each), one record of fp64 words per sample, written where the state
// lives each time the host asks for a sample (hp_probes_sample).  No reference counterpart: HiPIMS-OCL writes rasters only.
// Part of hp_engine.hip's translation unit, which is built with -ffp-contract=off -fno-fast-math: every operation below is a correctly rounded
// IEEE add, multiply or compare in fp64 and the order of every sum is fixed, so the records equal the host restatement
// (frontend.ProbeRecorder) bit for bit.  The conventions are the output stage's (hp_output.hpp): NODATA, the 1e-8 wet test,
// the counted-cell rule of domain_stats.
#pragma once
#include "hp_output.hpp"

namespace hp {

constexpr int PROBE_GAUGE_WORDS = 4;              // z, depth, qx, qy

// The recorder's lists in device memory (one allocation, written once by hp_probes_enable).  Cell ids are flat ids of the LOCAL
// array; the host has checked every one of them against cols * rows, every weight against {-1, 0, 1} and every section's length.
struct ProbeLists {
	const unsigned long long* gauge_cells;        // [gauges]
	const unsigned long long* section_offsets;    // [sections + 1] into the three arrays below
	const unsigned long long* section_cells;
	const signed char*        section_wx;
	const signed char*        section_wy;
	unsigned long long        gauges;
	unsigned                  gauge_blocks;       // ceil(gauges / 256): the blocks in front of the section blocks
	unsigned                  sections;
};

// -------------------------------------------------------------------------------------------------
// record_probes : one sample = one record [t, g0.z, g0.depth, g0.qx, g0.qy, g1.z, ..., s0.discharge, s1.discharge, ...] at
//     records + sample * stride.  Blocks [0, gauge_blocks): one thread per gauge.  Block gauge_blocks + s: section s --
//     thread j adds the terms of entries j, j + 256, j + 512, ... in that order to +0.0, the 256 partials are folded over
//     stats_block_fold's halving tree in LDS, and thread 0 stores dx * part[0].  No atomics; a section belongs to one block,
//     so the result does not depend on the launch shape.  The gathers are element-granular (a State4 and a bed value per
//     listed cell, 40 B in fp64): a section along a row is coalesced, one along a column touches a line per cell, and either
//     way the kernel moves kilobytes -- it costs a launch, not bandwidth.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void record_probes(const State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                     const Scalars<T>* __restrict__ scalars, const ProbeLists p,
                                                     double* __restrict__ records, const unsigned long long sample,
                                                     const unsigned long long stride, const double dx)
{
	double* __restrict__ rec = records + sample * stride;
	if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = (double)scalars->t;     // the device's own "Time", in stream order
	if (blockIdx.x < p.gauge_blocks) {
		const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
		if (g >= p.gauges) return;
		const unsigned long long k = p.gauge_cells[g];
		const State4<T> c = state[k];
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)bed[k];
		const bool counted = zmax > -9999.0 && zb <= 9999.0;                  // as in domain_stats
		double* __restrict__ out = rec + 1 + g * PROBE_GAUGE_WORDS;
		out[0] = counted ? z : OUT_NODATA;
		out[1] = counted ? z - zb : OUT_NODATA;                               // raw: unclamped, no wet test
		out[2] = counted ? qx : OUT_NODATA;
		out[3] = counted ? qy : OUT_NODATA;
		return;
	}
	const unsigned s = blockIdx.x - p.gauge_blocks;                           // (the whole block: the barriers below are uniform)
	const unsigned long long lo = p.section_offsets[s], hi = p.section_offsets[s + 1];
	double sum = 0.0;
	for (unsigned long long e = lo + threadIdx.x; e < hi; e += 256u) {
		const unsigned long long k = p.section_cells[e];
		const State4<T> c = state[k];
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)bed[k];
		double term = 0.0;
		if (zmax > -9999.0 && zb <= 9999.0 && z - zb > OUT_WET) {
			const double tx = (double)p.section_wx[e] * qx, ty = (double)p.section_wy[e] * qy;
			term = tx + ty;
		}
		sum = sum + term;
	}
	__shared__ double part[256];
	part[threadIdx.x] = sum;
	__syncthreads();
	for (int h = 128; h > 0; h >>= 1) {
		if ((int)threadIdx.x < h) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + h];
		__syncthreads();
	}
	if (threadIdx.x == 0) rec[1 + p.gauges * PROBE_GAUGE_WORDS + s] = dx * part[0];
}

} // namespace hp
