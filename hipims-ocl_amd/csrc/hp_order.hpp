// hp_order.hpp -- in which order one band's blocks of a pair launch take its tiles (godunov_march2, the still-record instantiation).
// A band's tiles are groups x nseg: `groups` 4-wave column groups, `nseg` row segments.  Blocks start in blockIdx order, and without a
// hint block i of the band runs tile (i % groups, i / groups): tile-row by tile-row.  Where only a few column groups hold moving water,
// the tiles that march -- the long ones -- are then spread evenly through the band's stream of blocks, and the last of them starts only
// when every skipped tile in front has found a slot.  The hint is one bit per group, "this group did a good part of the band's
// marching in the launch before" (hp_kernels.hpp: order_build decides which): the flagged groups' tiles go first, tile-row by tile-row
// among themselves, then the others' in the same manner.  Any mask gives a permutation of the band's tiles, so a wrong hint costs time
// and never a tile; no mask or a full one is the order without a hint.
// No HIP header and no state: the launch's tail block writes the next launch's table with order_fill_group (hp_kernels.hpp: OrderHook),
// hp_engine.hip writes the identity with order_entry, which is the table's definition word by word, and tests/order_probe.cpp includes
// this file with a host compiler and holds the two to each other.
#pragma once

#ifdef __HIPCC__
#define HP_ORDER_FN __host__ __device__ __forceinline__
#else
#define HP_ORDER_FN static inline
#endif

namespace hp {

constexpr unsigned ORDER_MAX_GROUPS = 64;                 // one mask bit per group
constexpr unsigned ORDER_G_BITS = 8;                      // a table entry: g in the low 8 bits, seg above

HP_ORDER_FN unsigned order_pack(const unsigned g, const unsigned seg) { return g | (seg << ORDER_G_BITS); }
HP_ORDER_FN unsigned order_g(const unsigned e) { return e & ((1u << ORDER_G_BITS) - 1u); }
HP_ORDER_FN unsigned order_seg(const unsigned e) { return e >> ORDER_G_BITS; }

HP_ORDER_FN unsigned order_bits(const unsigned long long m) { return (unsigned)__builtin_popcountll(m); }
// the index of the k-th set bit of m, counted from 0 (k < order_bits(m))
HP_ORDER_FN unsigned order_nth(unsigned long long m, unsigned k)
{
	for (; k; --k) m &= m - 1;
	return (unsigned)__builtin_ctzll(m);
}

// The tile of position i in [0, groups * nseg) of a band whose flagged groups are the set bits of `mask` (bits from `groups` up are ignored).
HP_ORDER_FN unsigned order_entry(const unsigned groups, const unsigned nseg, unsigned long long mask, const unsigned i)
{
	const unsigned long long all = groups >= 64u ? ~0ull : ((1ull << groups) - 1ull);
	mask &= all;
	const unsigned n_m = order_bits(mask);
	if (n_m == 0u || n_m == groups) return order_pack(i % groups, i / groups);
	const unsigned first = n_m * nseg;
	if (i < first) return order_pack(order_nth(mask, i % n_m), i / n_m);
	const unsigned j = i - first, n_u = groups - n_m;
	return order_pack(order_nth(~mask & all, j % n_u), j / n_u);
}

// The same table written by columns: every entry of the k-th group (k < groups) of the sequence "flagged groups ascending, then the
// others ascending" -- nseg words of `out`, which holds the band's groups * nseg.  This is what one lane of the tail block writes: one
// walk over the mask and a store per row segment, no division (order_entry per word lengthened every launch: LAB_NOTES R18.1).
HP_ORDER_FN void order_fill_group(const unsigned groups, const unsigned nseg, unsigned long long mask, const unsigned k, unsigned* const out)
{
	const unsigned long long all = groups >= 64u ? ~0ull : ((1ull << groups) - 1ull);
	mask &= all;
	const unsigned n_m = order_bits(mask), n_u = groups - n_m;
	if (n_m == 0u || n_u == 0u) { for (unsigned seg = 0; seg < nseg; ++seg) out[seg * groups + k] = order_pack(k, seg); return; }
	if (k < n_m) { const unsigned g = order_nth(mask, k); for (unsigned seg = 0; seg < nseg; ++seg) out[seg * n_m + k] = order_pack(g, seg); return; }
	const unsigned g = order_nth(~mask & all, k - n_m);
	for (unsigned seg = 0; seg < nseg; ++seg) out[n_m * nseg + seg * n_u + (k - n_m)] = order_pack(g, seg);
}

// entries of one band's table that differ from the order without a hint (hp_pair_stats)
HP_ORDER_FN bool order_is_identity(const unsigned groups, const unsigned i, const unsigned e) { return e == order_pack(i % groups, i / groups); }

} // namespace hp
