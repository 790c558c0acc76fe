// hp_links.hpp -- link groups: the boundary kind that moves water between two distant cells as a function of their OWN levels
// (hp_boundary_add_links): a weir into a storage basin, a culvert under a road, a flap-valved outfall, a pumping station.  No
// reference counterpart: the reference moves water between face neighbours and through prescribed sources only.
// The arithmetic of one link and one iteration is ONE definition in plain C++ (link_flow, link_record below): the kernel uses
// it, tests/links_probe.cpp includes this file with a host compiler, and frontend.Links restates it in NumPy.  All of it is fp64
// and uses correctly rounded add, multiply, divide, square root and compare only; nothing is fused: hp_engine.hip's translation
// unit is built with -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  The contract is in include/hipims_mi.h;
// the host side (hp_boundary_add_links, the pass that launches bdy_links, the records' part of a checkpoint) is in hp_actors.hpp.
#pragma once
#include "../../include/hipims_mi.h"
#include <cstdint>

#ifdef __HIPCC__
#define HP_LINK_FN __host__ __device__ __forceinline__
#else
#define HP_LINK_FN static inline
#endif

namespace hp {

constexpr uint64_t LINK_MAX = 65536;                      // links of all groups of a domain together
constexpr double   LINK_G = 9.81;                         // gravity<double>() (hp_math.hpp; CLUniversalHeader.clh:33)
constexpr unsigned long long LINK_ABSENT = ~0ull;         // LinkDev::a of a link this strip does not store

struct LinkEnd { double z, zmax, bed; };                  // a cell's level, maximum level and bed, widened
struct LinkFlow {
	double za, zb;                                        // the ends' levels after the link, before they are rounded on store
	double dz;                                            // the level that went from the upstream end to the downstream end: >= 0
	double s;                                             // +1: a -> b, -1: b -> a
	bool   inert;                                         // step 1 of the contract: nothing is touched, q_last = +0
};

// counted in the sense of hp_domain_stats
HP_LINK_FN bool link_counted(const LinkEnd e) { return e.zmax > -9999.0 && e.bed <= 9999.0; }

// -------------------------------------------------------------------------------------------------
// link_flow : steps 1 to 5 of the contract for one link.  dt: the "Timestep" scalar widened, dx: the cell size as the kernels
//     hold it (rounded to the domain's precision), widened.
// -------------------------------------------------------------------------------------------------
HP_LINK_FN LinkFlow link_flow(const int kind, const int one_way, const double level, const double size, const double coeff, const double limit,
                              const LinkEnd A, const LinkEnd B, const double dt, const double dx)
{
	LinkFlow r;
	r.za = A.z; r.zb = B.z; r.dz = 0.0; r.s = 1.0; r.inert = true;
	if (dt <= 0.0 || !link_counted(A) || !link_counted(B)) return r;
	r.inert = false;
	const bool a_up = kind == HP_LINK_PUMP ? true : (A.z >= B.z);
	const double zup = a_up ? A.z : B.z, zdn = a_up ? B.z : A.z, bed_up = a_up ? A.bed : B.bed;
	r.s = a_up ? 1.0 : -1.0;
	double q = 0.0;
	if (one_way != 0 && !a_up) {
		q = 0.0;                                                              // the flap is shut
	} else if (kind == HP_LINK_WEIR) {
		const double hu = zup - level;
		if (hu > 0.0) {
			const double cw = coeff * size;
			const double cwh = cw * hu;
			q = cwh * __builtin_sqrt(hu);
			const double hd = zdn - level;
			const double lim = limit * hu;
			if (hd > lim) {                                                   // beyond the modular limit: submerged
				const double num = hu - hd;
				const double one = 1.0 - limit;
				const double den = hu * one;
				const double ratio = num / den;
				q = q * __builtin_sqrt(ratio);
			}
		}
	} else if (kind == HP_LINK_ORIFICE) {
		if (zup > level) {
			const double tail = zdn > level ? zdn : level;
			const double dh = zup - tail;
			const double ca = coeff * size;
			const double g2 = 2.0 * LINK_G;
			const double head = g2 * dh;
			const double free_q = ca * __builtin_sqrt(head);
			q = limit < free_q ? limit : free_q;
		}
	} else {
		if (A.z > level) q = size;
	}
	const double vol = q * dt;
	const double area = dx * dx;
	double dz = vol / area;
	const double sill = level > bed_up ? level : bed_up;
	const double avail = zup - sill;
	if (!(avail > 0.0)) dz = 0.0;
	else if (avail < dz) dz = avail;
	if (kind != HP_LINK_PUMP) {
		const double gap = zup - zdn;
		const double half = 0.5 * gap;
		if (half < dz) dz = half;                                             // never past equal levels
	}
	r.dz = dz;
	if (dz > 0.0) {
		const double zup1 = zup - dz, zdn1 = zdn + dz;
		r.za = a_up ? zup1 : zdn1;
		r.zb = a_up ? zdn1 : zup1;
	}
	return r;
}

// step 6: what the iteration leaves in the link's record
HP_LINK_FN void link_record(hp_link_record_t& rec, const LinkFlow f, const double dt, const double dx)
{
	if (f.inert) { rec.q_last = 0.0; return; }
	const double area = dx * dx;
	const double moved = f.dz * area;
	const double rate = moved / dt;
	rec.q_last = f.s * rate;
	const double signed_moved = f.s * moved;
	rec.volume = rec.volume + signed_moved;
	rec.active += f.dz > 0.0 ? 1u : 0u;
}

} // namespace hp

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace hp {

// -------------------------------------------------------------------------------------------------
// validate_links : every argument error of hp_boundary_add_links that needs no device, in the order the header lists them.
//     `reach`: the scheme's stencil reach (the ring test of hp_boundary_add_cell), `taken`: the ends of the domain's links so
//     far, sorted; on success `taken_after` holds them merged with the new ones.  Returns false with `why` set.
// -------------------------------------------------------------------------------------------------
inline bool validate_links(const hp_link_t* links, const uint64_t count, const uint64_t existing, const uint64_t cols, const uint64_t global_rows,
                           const uint64_t reach, const std::vector<uint64_t>& taken, std::vector<uint64_t>& taken_after, std::string& why)
{
	const std::string who = "hp_boundary_add_links";
	if (!links) { why = who + ": links == NULL"; return false; }
	if (count < 1 || count > LINK_MAX || existing + count > LINK_MAX) { why = who + ": count outside 1..65536 over all groups of the domain"; return false; }
	std::vector<uint64_t> ends;
	ends.reserve(2 * (size_t)count);
	for (uint64_t k = 0; k < count; ++k) {
		const hp_link_t& l = links[k];
		const std::string which = who + ": link " + std::to_string(k);
		if (l.kind != HP_LINK_WEIR && l.kind != HP_LINK_ORIFICE && l.kind != HP_LINK_PUMP) { why = which + ": unknown kind"; return false; }
		if (!std::isfinite(l.level) || !std::isfinite(l.size)) { why = which + ": level and size must be finite"; return false; }
		if (l.size < 0.0) { why = which + ": negative size"; return false; }
		if (l.kind != HP_LINK_PUMP) {
			if (!std::isfinite(l.coeff)) { why = which + ": coeff must be finite"; return false; }
			if (l.coeff < 0.0) { why = which + ": negative coeff"; return false; }
			if (!std::isfinite(l.coeff * l.size)) { why = which + ": coeff * size must be finite"; return false; }
			if (l.kind == HP_LINK_WEIR && !(l.limit >= 0.0 && l.limit < 1.0)) { why = which + ": a weir's modular limit lies in [0, 1)"; return false; }
			if (l.kind == HP_LINK_ORIFICE && !(l.limit >= 0.0)) { why = which + ": an orifice's discharge cap is >= 0 (+inf for none)"; return false; }
		}
		if (l.cell_a == l.cell_b) { why = which + ": cell_a == cell_b"; return false; }
		for (const uint64_t id : {l.cell_a, l.cell_b}) {
			if (id >= cols * global_rows) { why = which + ": cell " + std::to_string(id) + " lies outside the grid"; return false; }
			const uint64_t gy = id / cols, x = id - gy * cols;
			if (x < reach || x + reach >= cols || gy < reach || gy + reach >= global_rows) { why = which + ": cell " + std::to_string(id) + " lies on the grid's ring"; return false; }
			ends.push_back(id);
		}
	}
	std::sort(ends.begin(), ends.end());
	taken_after.resize(taken.size() + ends.size());
	std::merge(taken.begin(), taken.end(), ends.begin(), ends.end(), taken_after.begin());
	const auto twice = std::adjacent_find(taken_after.begin(), taken_after.end());
	if (twice != taken_after.end()) { why = who + ": cell " + std::to_string(*twice) + " is an end of two links"; return false; }
	return true;
}

// -------------------------------------------------------------------------------------------------
// links_strip_verdict : what a strip that stores the global rows [local_lo, local_hi) does with a link between rows row_a and
//     row_b.  LINK_BOTH: it computes the link (redundantly with every other such strip), LINK_NEITHER: it ignores it, LINK_ONE:
//     unsupported.  `stale_lo` / `stale_hi`: the outermost stored rows of the south / north side that hold their owners' values
//     on every second iteration only (a strip with two reaches of ghost rows: one reach each on its interior sides; otherwise 0).
//     An end on such a row with the other end on a row that is always valid is as bad as one end stored: on the odd iteration
//     the link would read a stale level into a row that reaches the owned rows.
// -------------------------------------------------------------------------------------------------
enum { LINK_NEITHER = 0, LINK_ONE = 1, LINK_BOTH = 2 };
inline int links_strip_verdict(const int64_t row_a, const int64_t row_b, const int64_t local_lo, const int64_t local_hi, const int64_t stale_lo, const int64_t stale_hi)
{
	const bool a_in = row_a >= local_lo && row_a < local_hi, b_in = row_b >= local_lo && row_b < local_hi;
	if (!a_in && !b_in) return LINK_NEITHER;
	if (a_in != b_in) return LINK_ONE;
	const bool a_stale = row_a < local_lo + stale_lo || row_a >= local_hi - stale_hi;
	const bool b_stale = row_b < local_lo + stale_lo || row_b >= local_hi - stale_hi;
	return a_stale == b_stale ? LINK_BOTH : LINK_ONE;
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_math.hpp"         // State4, Scalars, Params

namespace hp {

static_assert(LINK_G == gravity<double>(), "the links' g is the engine's own constant");

// a link as the kernel reads it: the ends are flat ids of the LOCAL array (the host has checked the global ids and the strip's verdict)
struct LinkDev {
	unsigned long long a, b;                      // a == LINK_ABSENT: this strip stores neither end
	int    kind, one_way;
	double level, size, coeff, limit;
};

// -------------------------------------------------------------------------------------------------
// bdy_links : one group, one thread per link, on the iteration's source buffer.  A cell is an end of at most one link of the
//     domain, so no two threads touch the same entry: no atomics, no order.  The two state entries are loaded and stored whole
//     (32 B / 16 B: State4 is aligned to its size); only the levels change.  The record is this thread's alone.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void bdy_links(const Params<T> p, const Scalars<T>* __restrict__ sc, const LinkDev* __restrict__ links,
                                                const unsigned long long count, State4<T>* __restrict__ state, const T* __restrict__ bed,
                                                hp_link_record_t* __restrict__ records)
{
	const unsigned long long k = (unsigned long long)blockIdx.x * 64u + threadIdx.x;
	if (k >= count) return;
	const LinkDev l = links[k];
	if (l.a == LINK_ABSENT) return;
	const double dt = (double)sc->dt, dx = (double)p.dx;
	State4<T> ca = state[l.a], cb = state[l.b];
	const LinkEnd A = {(double)ca.z, (double)ca.zmax, (double)bed[l.a]}, B = {(double)cb.z, (double)cb.zmax, (double)bed[l.b]};
	const LinkFlow f = link_flow(l.kind, l.one_way, l.level, l.size, l.coeff, l.limit, A, B, dt, dx);
	hp_link_record_t rec = records[k];
	link_record(rec, f, dt, dx);
	records[k] = rec;
	if (f.inert || !(f.dz > 0.0)) return;
	ca.z = (T)f.za;
	cb.z = (T)f.zb;
	state[l.a] = ca;
	state[l.b] = cb;
}

} // namespace hp
#endif // __HIPCC__
