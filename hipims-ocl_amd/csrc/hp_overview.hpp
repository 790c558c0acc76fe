// hp_overview.hpp -- the output stage's reduced form: the nine values of hp_output.hpp aggregated over square blocks of
// factor x factor cells where the state lives (hp_domain_overview), so that a picture of the run costs 1 / factor^2 of the bytes a
// full raster moves to the host.  No reference counterpart: HiPIMS-OCL writes full rasters only.  Part of hp_engine.hip's
// translation unit (-ffp-contract=off -fno-fast-math): the per-cell value is out_value<V> of hp_output.hpp, the very expression
// derive_rasters stores, and what is ACCUMULATED is integers only -- an order-preserving 64-bit key of that double (largest,
// smallest) and a cell count.  Integer maxima and sums do not depend on the order of their terms: a block's result is a pure
// function of the state, whatever the launch shape, the arrival order of the atomics, the cut of a request into blocks of rows or
// the cut of the grid into strips (frontend.overview restates it in NumPy, frontend.combine_overviews puts parts together).
#pragma once
#include "hp_zones.hpp"        // zone_load_state: the whole cell in 16-byte loads

namespace hp {

enum { AGG_MAX, AGG_MIN, AGG_COUNT, AGG_KINDS };
constexpr int OVERVIEW_PAIRS = OUT_VALUES * AGG_KINDS;

// The doubles in their own order as unsigned integers: negative values complemented, the others with the sign bit set.  -0.0 lies
// below +0.0.  No participating value is a NaN, so a key is never 0 and never all ones: 0 is "no cell yet" for the largest key,
// and -- the smallest being kept as the largest COMPLEMENT -- for the smallest as well.  One fill with zeros starts all three.
__device__ __forceinline__ unsigned long long overview_key(const double v)
{
	const long long b = __double_as_longlong(v);
	return b < 0 ? ~(unsigned long long)b : (unsigned long long)b | 0x8000000000000000ull;
}
__device__ __forceinline__ double overview_unkey(const unsigned long long k)
{
	return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

struct OverviewPlan {
	signed char slot[OUT_VALUES][AGG_KINDS];      // [value][aggregate] -> index of that pair's accumulator raster, -1: not asked for
	unsigned    values;                           // bit v: value v is in some pair (the same in every lane: a scalar branch per value)
};

struct OverviewGeom {
	long long cols;                               // of the local array
	long long row_offset;                         // global row of local row 0
	long long g_lo, g_hi;                         // GLOBAL rows [g_lo, g_hi) this launch aggregates
	long long factor;
	long long band, nsub;                         // a block row is walked in nsub bands of `band` rows (the last one shorter)
	long long by0;                                // first block row of this launch
	long long block_cols;
	long long blocks;                             // block rows of this launch x block_cols: the length of one accumulator raster
	long long col_groups, items;                  // groups of 256 columns; bands x col_groups
	double    resolution;
};

// -------------------------------------------------------------------------------------------------
// overview_blocks : one streaming pass over the rows of the launch; 40 B read per fp64 cell whatever the number of pairs, and
//     only coarse elements written.  A work item is a band of at most `band` rows of ONE block row by 256 columns; a workgroup
//     takes items by grid stride, its four waves 64 adjacent columns each.  A lane owns a column: it walks the band's rows (the
//     next row's loads issued before the current row is worked on) with the running largest key, largest complemented key and
//     count of every value asked for in registers.  Then a segmented fold over the lanes of the same block (shuffles; at most
//     log2(min(factor, 64)) steps), and the first lane of every segment issues one integer atomic per pair into the accumulator
//     rasters, which a fill has zeroed: max, max and add.  T = the domain's precision, widened to fp64 first.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void overview_blocks(const State4<T>* __restrict__ state, const T* __restrict__ bed, const OverviewGeom g,
                                                       unsigned long long* __restrict__ acc, const OverviewPlan plan)
{
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned values = plan.values;
	const bool velocity = (values & OUT_NEEDS_VELOCITY) != 0;
	for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
		const long long bandi = item / g.col_groups, cg = item - bandi * g.col_groups;
		const long long brow = bandi / g.nsub, sub = bandi - brow * g.nsub;
		const long long top = (g.by0 + brow + 1) * g.factor;
		long long r_lo = (g.by0 + brow) * g.factor + sub * g.band, r_hi = r_lo + g.band;
		r_hi = r_hi < top ? r_hi : top;
		r_lo = r_lo > g.g_lo ? r_lo : g.g_lo;
		r_hi = r_hi < g.g_hi ? r_hi : g.g_hi;
		const long long x0 = cg * 256 + (long long)wave * 64;
		if (r_lo >= r_hi || x0 >= g.cols) continue;                                // (the whole wave)
		const long long x = x0 + lane;
		const bool inside = x < g.cols;
		const size_t first = (size_t)(r_lo - g.row_offset) * (size_t)g.cols + (size_t)(inside ? x : g.cols - 1);   // (a lane past the east edge re-reads the last column and drops it)
		unsigned long long hi[OUT_VALUES], lo[OUT_VALUES];                         // (indexed by constants only: registers)
		unsigned n[OUT_VALUES];
		out_for_each(values, [&](auto v) { constexpr int V = decltype(v)::value; hi[V] = lo[V] = 0; n[V] = 0; });
		State4<T> c = zone_load_state(state + first);
		T zb = bed[first];
		for (long long r = r_lo; r < r_hi; ++r) {
			State4<T> c_next = c;
			T zb_next = zb;
			if (r + 1 < r_hi) {                                                     // wave-uniform: the next row's loads, in flight over this row's arithmetic
				const size_t i = first + (size_t)(r + 1 - r_lo) * (size_t)g.cols;
				c_next = zone_load_state(state + i);
				zb_next = bed[i];
			}
			const OutCell o = out_cell(c, zb, velocity);
			out_for_each(values, [&](auto v) {
				constexpr int V = decltype(v)::value;
				const double val = out_value<V>(o, g.resolution);
				const bool takes_part = inside && val != OUT_NODATA && val == val;  // neither NODATA nor NaN
				const unsigned long long key = takes_part ? overview_key(val) : 0ull, nkey = takes_part ? ~key : 0ull;
				hi[V] = key > hi[V] ? key : hi[V];
				lo[V] = nkey > lo[V] ? nkey : lo[V];
				n[V] += takes_part ? 1u : 0u;
			});
			c = c_next;
			zb = zb_next;
		}
		// lanes of one block are adjacent: lane + s belongs to this lane's block while it stays left of the block's east edge
		const long long bx = x / g.factor;
		const long long room = g.factor - (x - bx * g.factor);                     // columns from this lane to the block's east edge
		const unsigned steps = g.factor < 64 ? (unsigned)g.factor : 64u;
		out_for_each(values, [&](auto v) {
			constexpr int V = decltype(v)::value;
			for (unsigned s = 1; s < steps; s <<= 1) {
				const unsigned long long h = __shfl_down(hi[V], s, 64), l = __shfl_down(lo[V], s, 64);
				const unsigned m = __shfl_down(n[V], s, 64);
				if (lane + s < 64u && (long long)s < room) {
					hi[V] = h > hi[V] ? h : hi[V];
					lo[V] = l > lo[V] ? l : lo[V];
					n[V] += m;
				}
			}
		});
		if (inside && (lane == 0 || room == g.factor)) {                           // the first lane of a segment holds its fold
			unsigned long long* const mine = acc + (size_t)(brow * g.block_cols + bx);
			out_for_each(values, [&](auto v) {
				constexpr int V = decltype(v)::value;
				if (n[V] == 0) return;                                              // (nothing took part: all three stay as the fill left them)
				// results unused: no-return atomics.  Relaxed: overview_finish reads them in stream order behind this kernel.
				if (plan.slot[V][AGG_MAX] >= 0)
					__hip_atomic_fetch_max(mine + (size_t)plan.slot[V][AGG_MAX] * (size_t)g.blocks, hi[V], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (plan.slot[V][AGG_MIN] >= 0)
					__hip_atomic_fetch_max(mine + (size_t)plan.slot[V][AGG_MIN] * (size_t)g.blocks, lo[V], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (plan.slot[V][AGG_COUNT] >= 0)
					__hip_atomic_fetch_add(mine + (size_t)plan.slot[V][AGG_COUNT] * (size_t)g.blocks, (unsigned long long)n[V], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			});
		}
	}
}

// -------------------------------------------------------------------------------------------------
// overview_finish : the accumulator rasters (pair after pair, `blocks` words each) as elements of type O behind them: the key
//     back as its double (NODATA where no cell took part), the count as a number; rounded once to fp32 where O is float.
//     kinds: two bits per pair, the pair's aggregate.  blockIdx.y = the pair.
// -------------------------------------------------------------------------------------------------
template <typename O>
__global__ __launch_bounds__(256) void overview_finish(const unsigned long long* __restrict__ acc, O* __restrict__ out, const size_t blocks,
                                                       const unsigned long long kinds)
{
	const unsigned pair = blockIdx.y;
	const unsigned agg = (unsigned)(kinds >> (2u * pair)) & 3u;
	const unsigned long long* __restrict__ a = acc + (size_t)pair * blocks;
	O* __restrict__ o = out + (size_t)pair * blocks;
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < blocks; k += (size_t)gridDim.x * blockDim.x) {
		const unsigned long long w = a[k];
		double r;
		if (agg == AGG_COUNT) r = (double)w;
		else r = w == 0 ? OUT_NODATA : overview_unkey(agg == AGG_MAX ? w : ~w);
		o[k] = (O)r;
	}
}

} // namespace hp
