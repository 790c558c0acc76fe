// hp_zones.hpp -- the zone recorder: per-zone cell counts, volume of water, largest depth and speed as a time series, one record
// of 64-bit words per sample, written where the state lives each time the host asks for a sample (hp_zones_sample).  A zone is a
// set of cells carrying the same id in a 2-byte raster (0 = in no zone).  No reference counterpart: HiPIMS-OCL writes rasters only.
// Part of hp_engine.hip's translation unit, which is built with -ffp-contract=off -fno-fast-math: every floating-point operation
// below is a correctly rounded IEEE one in fp64, and what is ACCUMULATED is integers only -- counts, the two limbs of a depth in
// units of 2^-32 m, and bit patterns of non-negative doubles (which order like the doubles).  Integer sums and maxima do not
// depend on the order of their terms: the record is a pure function of the state and the id raster, whatever the launch shape,
// the arrival order of the atomics or the cut of the grid into strips (frontend.ZoneRecorder restates it in NumPy, and
// frontend.combine_zones adds the strips' records).  The conventions are the output stage's (hp_output.hpp): the 1e-8 wet test,
// the counted-cell rule and the speed of domain_stats.
#pragma once
#include "hp_output.hpp"

namespace hp {

constexpr int    ZONE_WORDS     = 7;              // cells, wet, flooded, depth_hi, depth_lo, max_depth, max_speed
constexpr double ZONE_DEPTH_CAP = 1048576.0;      // 2^20 m: the scaled depth stays below 2^52 and is an exact integer
constexpr double ZONE_SCALE     = 4294967296.0;   // 2^32: the quantum of a depth is 2^-32 m

// The whole cell in 16-byte loads issued together, in front of everything that depends on it (one for fp32, two for fp64): read
// member by member, the momenta -- needed by wet cells only -- end up as a load of their own inside the wet branch, a second
// dependent memory round trip per step.
typedef unsigned int zone_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ State4<double> zone_load_state(const State4<double>* __restrict__ p)
{
	const zone_u32x4* __restrict__ v = reinterpret_cast<const zone_u32x4*>(p);
	const zone_u32x4 a = v[0], b = v[1];
	State4<double> s;
	s.z  = __hiloint2double((int)a.y, (int)a.x); s.zmax = __hiloint2double((int)a.w, (int)a.z);
	s.qx = __hiloint2double((int)b.y, (int)b.x); s.qy   = __hiloint2double((int)b.w, (int)b.z);
	return s;
}
__device__ __forceinline__ State4<float> zone_load_state(const State4<float>* __restrict__ p)
{
	const zone_u32x4 a = *reinterpret_cast<const zone_u32x4*>(p);
	State4<float> s;
	s.z = __uint_as_float(a.x); s.zmax = __uint_as_float(a.y); s.qx = __uint_as_float(a.z); s.qy = __uint_as_float(a.w);
	return s;
}

// what a wave has gathered for the zone it is in
struct ZoneAcc {
	unsigned long long cells, wet, flooded;       // wave-uniform: popcounts of ballots
	unsigned long long hi, lo, depth, speed;      // per lane; folded across the wave when flushed
};

__device__ __forceinline__ void zone_atomics(unsigned long long* __restrict__ z, const unsigned long long cells, const unsigned long long wet,
                                             const unsigned long long flooded, const unsigned long long hi, const unsigned long long lo,
                                             const unsigned long long depth, const unsigned long long speed)
{
	// results unused: no-return atomics.  Relaxed: the host reads the record in stream order behind the kernel.
	__hip_atomic_fetch_add(z + 0, cells,   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_add(z + 1, wet,     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_add(z + 2, flooded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_add(z + 3, hi,      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_add(z + 4, lo,      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_max(z + 5, depth,   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_fetch_max(z + 6, speed,   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The wave's registers into zone `id` of the record (one lane issues the seven atomics), and empty again.  Wave-uniform call.
__device__ __forceinline__ void zone_flush(unsigned long long* __restrict__ rec, const unsigned id, ZoneAcc& a, const unsigned lane)
{
	if (id != 0 && a.cells != 0) {                // (a zone without a counted cell adds nothing: all seven are 0)
		unsigned long long hi = a.hi, lo = a.lo, depth = a.depth, speed = a.speed;
		for (int s = 32; s > 0; s >>= 1) {
			hi += __shfl_xor(hi, s, 64);
			lo += __shfl_xor(lo, s, 64);
			const unsigned long long od = __shfl_xor(depth, s, 64), os = __shfl_xor(speed, s, 64);
			depth = od > depth ? od : depth;
			speed = os > speed ? os : speed;
		}
		if (lane == 0) zone_atomics(rec + 1 + (size_t)(id - 1) * ZONE_WORDS, a.cells, a.wet, a.flooded, hi, lo, depth, speed);
	}
	a.cells = a.wet = a.flooded = 0;
	a.hi = a.lo = a.depth = a.speed = 0;
}

// -------------------------------------------------------------------------------------------------
// record_zones : one sample = one record [t | zone 1: 7 words | zone 2: 7 words | ...] at `rec`, zeroed by a fill queued in front
//     of the kernel.  A whole-grid streaming pass: 32 B of state (two 16-byte loads), 8 B of bed and 2 B of id per fp64 cell.
//     A wave owns `per_wave` contiguous cells (a multiple of 64) and walks them 64 at a time.  Zones are spatially coherent: as
//     long as all lanes of a step carry the wave's current id (readfirstlane + ballot) the figures stay in registers, the three
//     counts as wave-uniform popcounts; when the id changes, and at the end, the wave folds its registers and one lane issues
//     seven 64-bit atomics.  A step with mixed ids (a zone border) flushes and lets every counted lane with a non-zero id issue
//     its own seven: correct everywhere, slow only where it is rare.  T = the domain's precision, widened to fp64 first.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void record_zones(const State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                    const unsigned short* __restrict__ zone_of_cell, const Scalars<T>* __restrict__ scalars,
                                                    unsigned long long* __restrict__ rec, const size_t n, const size_t per_wave,
                                                    const double flood_depth)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = (unsigned long long)__double_as_longlong((double)scalars->t);   // the device's own "Time", in stream order
	const unsigned lane = threadIdx.x & 63u;
	const size_t wave = (size_t)blockIdx.x * (256 / 64) + (threadIdx.x >> 6);
	const size_t lo = wave * per_wave;
	if (lo >= n) return;                                                        // (the whole wave)
	const size_t hi = lo + per_wave < n ? lo + per_wave : n;
	ZoneAcc a;
	a.cells = a.wet = a.flooded = 0;
	a.hi = a.lo = a.depth = a.speed = 0;
	unsigned cur = 0;                                                            // the id the registers belong to (0: they are empty)
	for (size_t base = lo; base < hi; base += 64) {                             // wave-uniform: lane 0 is always inside
		const size_t k = base + lane;
		const bool inside = k < hi;
		const size_t i = inside ? k : base;                                      // (a lane past the end re-reads the step's first cell and drops it)
		const State4<T> c = zone_load_state(state + i);                         // the step's loads first, all four in flight together
		const T zb_ = bed[i];
		const unsigned id = zone_of_cell[i];
		__builtin_amdgcn_sched_barrier(0);                                       // (left alone, the fp32 build's bed load waits for the id to arrive)
		const double z = (double)c.z, zmax = (double)c.zmax, qx = (double)c.qx, qy = (double)c.qy;
		const double zb = (double)zb_;
		const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)id);
		const bool uniform = __ballot(inside && id != first) == 0ull;
		// counted as in domain_stats: not disabled and not a closed-edge wall
		const bool counted = inside && zmax > -9999.0 && zb <= 9999.0;
		const double depth = z - zb;
		double d = depth > 0.0 ? depth : 0.0;
		d = d > ZONE_DEPTH_CAP ? ZONE_DEPTH_CAP : d;
		const bool wet = counted && depth > OUT_WET;
		const bool flooded = counted && depth > flood_depth;
		// still water has speed 0, which contributes nothing: no division for it.  (Also what keeps the momenta in the loads above:
		// a value used inside the branch alone is loaded inside it.)  A NaN momentum is "moving" and is dropped by `sp > 0` below.
		const bool moving = (qx != 0.0) | (qy != 0.0);
		const unsigned long long q = counted ? (unsigned long long)__builtin_rint(d * ZONE_SCALE) : 0ull;   // exact scaling; half to even
		const unsigned long long dbits = counted ? (unsigned long long)__double_as_longlong(d) : 0ull;
		unsigned long long sbits = 0;
		if (wet & moving) {
			const double vx = qx / depth, vy = qy / depth;
			const double sp = sqrt_(vx * vx + vy * vy);                          // domain_stats' speed
			if (sp > 0.0) sbits = (unsigned long long)__double_as_longlong(sp);  // (a NaN or a zero contributes nothing)
		}
		if (uniform) {
			if (first != cur) { zone_flush(rec, cur, a, lane); cur = first; }
			if (cur != 0) {
				a.cells += (unsigned long long)__popcll(__ballot(counted));
				a.wet += (unsigned long long)__popcll(__ballot(wet));
				a.flooded += (unsigned long long)__popcll(__ballot(flooded));
				a.hi += q >> 32;
				a.lo += q & 0xffffffffull;
				a.depth = dbits > a.depth ? dbits : a.depth;
				a.speed = sbits > a.speed ? sbits : a.speed;
			}
		} else {
			zone_flush(rec, cur, a, lane);
			cur = 0;
			if (counted && id != 0)
				zone_atomics(rec + 1 + (size_t)(id - 1) * ZONE_WORDS, 1ull, wet ? 1ull : 0ull, flooded ? 1ull : 0ull, q >> 32, q & 0xffffffffull, dbits, sbits);
		}
	}
	zone_flush(rec, cur, a, lane);
}

} // namespace hp
