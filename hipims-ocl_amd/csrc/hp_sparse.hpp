// hp_sparse.hpp -- the output stage's selected form: the nine values of hp_output.hpp at the cells that satisfy a predicate, and
// nothing else, in CSR (hp_domain_sparse).  A flood map is mostly NODATA: what crosses the host link is the selected share of a
// raster, at full resolution.  No reference counterpart: HiPIMS-OCL writes full rasters only.  Part of hp_engine.hip's translation
// unit (-ffp-contract=off -fno-fast-math): the per-cell value is out_value<V> of hp_output.hpp, the very expression derive_rasters
// stores.  A stream compaction in three passes over SEGMENTS -- 64 consecutive columns of one row, one wave each, lanes owning
// columns --: sparse_select stores the wave's ballot per segment, the sparse_scan_* kernels turn the words' population counts into
// 64-bit offsets (block sums, one block over the sums, the add: three launches, no workgroup ever waits for another), and
// sparse_scatter writes column and values of every set bit at offset + rank.  Entries ascend by (row, column) by construction;
// everything between the predicate and the store is integer arithmetic, so the result is a pure function of the state, whatever
// the launch shape, the cut of a request into runs or the cut of the grid into strips (frontend.sparse restates it in NumPy).
// The cut of a request into runs (sparse_plan_runs) needs no HIP: tests/sparse_probe.cpp includes this file with a host compiler.
#pragma once
#include <cstdint>
#include <vector>

namespace hp {

// -------------------------------------------------------------------------------------------------
// sparse_plan_runs : entries [0, row_ptr[nrows]) cut into runs that fit `budget` bytes of scratch at `bytes_per_entry` each, in
//     order.  A run is as many whole rows as fit; a single row that does not fit is split by entries (its runs name that one
//     row).  Rows without entries join the run in front of them or are left out.  Empty if there is nothing to cut or if not
//     even one entry fits.
// -------------------------------------------------------------------------------------------------
struct SparseRun {
	int64_t  row_lo, row_hi;                      // rows [row_lo, row_hi) of the range hold the run's entries
	uint64_t first, count;                        // entries [first, first + count)
};

inline std::vector<SparseRun> sparse_plan_runs(const uint64_t* row_ptr, const int64_t nrows, const uint64_t bytes_per_entry, const uint64_t budget)
{
	std::vector<SparseRun> runs;
	if (nrows < 1 || bytes_per_entry == 0) return runs;
	const uint64_t fit = budget / bytes_per_entry;
	if (fit == 0) return runs;
	int64_t r = 0;
	while (r < nrows) {
		const uint64_t first = row_ptr[r];
		if (row_ptr[nrows] == first) break;                                        // (the rest is empty)
		if (row_ptr[r + 1] == first) { ++r; continue; }                            // (an empty row in front of a run)
		if (row_ptr[r + 1] - first > fit) {                                        // this row alone does not fit: by entries
			for (uint64_t e = first; e < row_ptr[r + 1]; e += fit)
				runs.push_back({r, r + 1, e, row_ptr[r + 1] - e < fit ? row_ptr[r + 1] - e : fit});
			++r;
			continue;
		}
		int64_t hi = r + 1;
		while (hi < nrows && row_ptr[hi + 1] - first <= fit) ++hi;
		runs.push_back({r, hi, first, row_ptr[hi] - first});
		r = hi;
	}
	return runs;
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_zones.hpp"        // zone_load_state: the whole cell in 16-byte loads

namespace hp {

constexpr unsigned SPARSE_SCAN_TILE = 1024;       // segments per block of the scan: 256 threads x 4

struct SparseGeom {
	long long cols;                               // of the local array
	long long row0;                               // first local row of the range
	unsigned  segs_per_row;                       // ceil(cols / 64)
	unsigned  seg_lo, seg_hi;                     // segments [seg_lo, seg_hi) of the range this launch works on
	double    resolution;
};

struct SparseTargets {
	void*     raster[OUT_VALUES];                 // entries of value v of this run (nullptr: not asked for)
	unsigned* col;                                // the entries' columns
	unsigned  mask;                               // bit v: raster[v] is written (the same in every lane: a scalar branch per value)
	unsigned long long first, count;              // entries [first, first + count) belong to this run: entry e goes to element e - first
};

// the segment of this wave in a launch of 256-thread blocks, the same in every lane (a scalar)
__device__ __forceinline__ unsigned sparse_wave_index() { return __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)); }

// -------------------------------------------------------------------------------------------------
// sparse_select : the predicate of every cell of segments [seg_lo, seg_hi), one 64-bit word per segment.  State and bed are read
//     once (a lane past the east edge re-reads the last column and votes false); v = out_value<select> in fp64 before any
//     rounding; selected iff v != NODATA && v > above (a NaN fails the comparison).  T = the domain's precision.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sparse_select(const State4<T>* __restrict__ state, const T* __restrict__ bed, const SparseGeom g,
                                                     const int select, const double above, unsigned long long* __restrict__ words)
{
	const unsigned lane = threadIdx.x & 63u;
	const unsigned select_mask = 1u << select;
	const bool velocity = (select_mask & OUT_NEEDS_VELOCITY) != 0;
	for (unsigned seg = g.seg_lo + sparse_wave_index(); seg < g.seg_hi; seg += gridDim.x * 4u) {
		const unsigned r = seg / g.segs_per_row, s = seg - r * g.segs_per_row;
		const long long x = (long long)s * 64 + lane;
		const bool inside = x < g.cols;
		const size_t i = (size_t)(g.row0 + r) * (size_t)g.cols + (size_t)(inside ? x : g.cols - 1);
		const State4<T> c = zone_load_state(state + i);
		const OutCell o = out_cell(c, bed[i], velocity);
		double v = OUT_NODATA;
		out_for_each(select_mask, [&](auto code) { constexpr int V = decltype(code)::value; v = out_value<V>(o, g.resolution); });
		const unsigned long long word = __ballot(inside && v != OUT_NODATA && v > above);
		if (lane == 0) words[seg] = word;
	}
}

// -------------------------------------------------------------------------------------------------
// The exclusive prefix sum of the words' population counts, over `nseg` segments in tiles of SPARSE_SCAN_TILE:
//   sparse_scan_sums    : block b -> sums[b] = the entries of tile b
//   sparse_scan_top     : ONE block: sums[0 .. tiles) -> their exclusive prefix sum in place, sums[tiles] = the total
//   sparse_scan_offsets : block b -> offsets of tile b's segments (sums[b] + the prefix inside the tile); the offset of every row's
//                         first segment into row_ptr, and the total into row_ptr[nrows]
// -------------------------------------------------------------------------------------------------
// inclusive prefix sum of v over the 256 threads of the block (lds: 4 words); total = the block's sum
__device__ __forceinline__ unsigned long long sparse_block_scan(unsigned long long v, unsigned long long* lds, unsigned long long& total)
{
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (unsigned s = 1; s < 64; s <<= 1) {
		const unsigned long long up = __shfl_up(v, s, 64);
		if (lane >= s) v += up;
	}
	__syncthreads();                                                             // (the words of an earlier call have been read)
	if (lane == 63) lds[wave] = v;
	__syncthreads();
	unsigned long long before = 0;
	for (unsigned w = 0; w < 4; ++w) before += w < wave ? lds[w] : 0ull;
	total = lds[0] + lds[1] + lds[2] + lds[3];
	return v + before;
}

__global__ __launch_bounds__(256) void sparse_scan_sums(const unsigned long long* __restrict__ words, const unsigned nseg, unsigned long long* __restrict__ sums)
{
	__shared__ unsigned long long lds[4];
	const unsigned base = blockIdx.x * SPARSE_SCAN_TILE + threadIdx.x * 4u;
	unsigned long long mine = 0;
	for (unsigned k = 0; k < 4; ++k) mine += base + k < nseg ? (unsigned long long)__popcll(words[base + k]) : 0ull;
	unsigned long long total;
	sparse_block_scan(mine, lds, total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void sparse_scan_top(unsigned long long* __restrict__ sums, const unsigned tiles)
{
	__shared__ unsigned long long lds[4];
	unsigned long long carry = 0;
	for (unsigned at = 0; at < tiles; at += 256) {                               // (block-uniform trip count)
		const unsigned k = at + threadIdx.x;
		const unsigned long long mine = k < tiles ? sums[k] : 0ull;
		unsigned long long total;
		const unsigned long long incl = sparse_block_scan(mine, lds, total);
		if (k < tiles) sums[k] = carry + incl - mine;
		carry += total;
	}
	if (threadIdx.x == 0) sums[tiles] = carry;
}

__global__ __launch_bounds__(256) void sparse_scan_offsets(const unsigned long long* __restrict__ words, const unsigned nseg, const unsigned long long* __restrict__ sums,
                                                           const unsigned tiles, const unsigned segs_per_row, unsigned long long* __restrict__ offsets,
                                                           unsigned long long* __restrict__ row_ptr)
{
	__shared__ unsigned long long lds[4];
	const unsigned base = blockIdx.x * SPARSE_SCAN_TILE + threadIdx.x * 4u;
	unsigned n[4];
	unsigned long long mine = 0;
	for (unsigned k = 0; k < 4; ++k) { n[k] = base + k < nseg ? (unsigned)__popcll(words[base + k]) : 0u; mine += n[k]; }
	unsigned long long total;
	unsigned long long at = sums[blockIdx.x] + sparse_block_scan(mine, lds, total) - mine;
	for (unsigned k = 0; k < 4; ++k) {
		const unsigned seg = base + k;
		if (seg < nseg) {
			offsets[seg] = at;
			const unsigned r = seg / segs_per_row;
			if (seg == r * segs_per_row) row_ptr[r] = at;
		}
		at += n[k];
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) row_ptr[nseg / segs_per_row] = sums[tiles];
}

// -------------------------------------------------------------------------------------------------
// sparse_scatter : the entries of segments [seg_lo, seg_hi).  A segment whose word is 0 returns without touching the state: that
//     is where a mostly dry grid saves its bytes.  Otherwise the cell is loaded again and a lane whose bit is set stores its
//     column and every requested value at offset[segment] + (set bits below its own) -- the saved word is trusted, the predicate
//     is not formed again.  Only entries [t.first, t.first + t.count) are stored, at element e - t.first: the run's share of the
//     scratch.  T = the domain's precision, O = the element type of the values.
// -------------------------------------------------------------------------------------------------
template <typename T, typename O>
__global__ __launch_bounds__(256) void sparse_scatter(const State4<T>* __restrict__ state, const T* __restrict__ bed, const SparseGeom g,
                                                      const unsigned long long* __restrict__ words, const unsigned long long* __restrict__ offsets,
                                                      const SparseTargets t)
{
	const unsigned lane = threadIdx.x & 63u;
	const unsigned mask = t.mask;
	const bool velocity = (mask & OUT_NEEDS_VELOCITY) != 0;
	for (unsigned seg = g.seg_lo + sparse_wave_index(); seg < g.seg_hi; seg += gridDim.x * 4u) {
		const unsigned long long word = words[seg];
		if (word == 0) continue;                                                 // (the whole wave)
		const unsigned r = seg / g.segs_per_row, s = seg - r * g.segs_per_row;
		const long long x = (long long)s * 64 + lane;
		const size_t i = (size_t)(g.row0 + r) * (size_t)g.cols + (size_t)(x < g.cols ? x : g.cols - 1);
		const State4<T> c = zone_load_state(state + i);
		const T zb = bed[i];
		const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
		const unsigned long long e = offsets[seg] + rank - t.first;              // (wraps below t.first: fails the comparison)
		if (((word >> lane) & 1ull) == 0 || e >= t.count) continue;
		const OutCell o = out_cell(c, zb, velocity);
		t.col[e] = (unsigned)x;
		out_for_each(mask, [&](auto code) { constexpr int V = decltype(code)::value; ((O*)t.raster[V])[e] = (O)out_value<V>(o, g.resolution); });
	}
}

} // namespace hp
#endif
