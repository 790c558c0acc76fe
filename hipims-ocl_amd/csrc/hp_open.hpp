// hp_open.hpp -- the open boundary: the boundary kind that lets water leave the model (hp_boundary_add_open).  A set of segments of the
// grid's edge ring; once per iteration every listed ring cell takes the depth and the outward momentum of its inward neighbour -- a
// zero-gradient, outflow-only edge -- and records the discharge that leaves through its face.  No reference counterpart: the reference's
// edges are closed walls or never-written cells.
// The arithmetic of one ring cell and one iteration is ONE definition in plain C++ (open_impose, open_record below): the kernel uses it,
// tests/open_probe.cpp includes this file with a host compiler, and frontend.Open restates it in NumPy.  All of it is fp64 and uses
// correctly rounded add, subtract, multiply and compare only; nothing is fused: hp_engine.hip's translation unit is built with
// -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  The face flux the record is made of is the STRICT face solve of
// hp_math.hpp in the domain's precision, whatever the domain's math mode (the tracer's rule).  The contract is in include/hipims_mi.h;
// the host side (hp_boundary_add_open, the pass that launches bdy_open, the records' part of a checkpoint) is in hp_actors.hpp.
#pragma once
#include "../../include/hipims_mi.h"
#include <cstdint>

#ifdef __HIPCC__
#define HP_OPEN_FN __host__ __device__ __forceinline__
#else
#define HP_OPEN_FN static inline
#endif

namespace hp {

constexpr unsigned OPEN_MAX_SEGMENTS = 64;                // segments of a domain together
constexpr unsigned long long OPEN_ABSENT = ~0ull;         // OpenDev::r of a ring cell this strip does not store

struct OpenRing  { double zmax, bed; };                   // the ring cell r: what of it decides (its level and momentum are replaced)
struct OpenInner { double z, zmax, qn, qs, bed; };        // its inward neighbour i, widened: qn the component normal to the edge, qs the other
struct OpenImposed {
	double lvl, qn, qs;                                   // what r takes, before the level is rounded on store
	bool   inert;                                         // step 1 of the contract: nothing is touched, q_last = +0
	bool   dry, capped, zeroed;                           // which branch: d == 0; the level was capped (step 3); an inward Qn_i was not taken
};

// counted in the sense of hp_domain_stats
HP_OPEN_FN bool open_counted(const double zmax, const double bed) { return zmax > -9999.0 && bed <= 9999.0; }
// does a normal component point out of the grid on this edge?
HP_OPEN_FN bool open_outward(const int edge, const double qn) { return (edge == HP_EDGE_EAST || edge == HP_EDGE_NORTH) ? qn > 0.0 : qn < 0.0; }

// -------------------------------------------------------------------------------------------------
// open_impose : steps 1 to 4 of the contract for one ring cell.  dt: the "Timestep" scalar widened.
// -------------------------------------------------------------------------------------------------
HP_OPEN_FN OpenImposed open_impose(const int edge, const OpenRing R, const OpenInner I, const double dt)
{
	OpenImposed o;
	o.lvl = 0.0; o.qn = 0.0; o.qs = 0.0; o.inert = true; o.dry = false; o.capped = false; o.zeroed = false;
	if (dt <= 0.0 || !open_counted(R.zmax, R.bed) || !open_counted(I.zmax, I.bed)) return o;
	o.inert = false;
	double d = I.z - I.bed;
	if (!(d > 0.0)) d = 0.0;
	double lvl = R.bed + d;
	if (lvl > I.z) {
		lvl = I.z > R.bed ? I.z : R.bed;
		o.capped = true;
	}
	o.lvl = lvl;
	if (d == 0.0) {
		o.dry = true;
	} else {
		o.qs = I.qs;
		if (open_outward(edge, I.qn)) o.qn = I.qn;
		else o.zeroed = I.qn != 0.0;
	}
	return o;
}

// step 6: what the iteration leaves in the cell's record.  F: the mass flux of the face between i and r as the flux kernel orients it
// (positive towards +x / +y), widened; dx: the cell size as the kernels hold it, widened
HP_OPEN_FN void open_record(hp_open_record_t& rec, const bool inert, const int edge, const double F, const double dt, const double dx)
{
	if (inert) { rec.q_last = 0.0; return; }
	const double out = (edge == HP_EDGE_EAST || edge == HP_EDGE_NORTH) ? F : -F;
	rec.q_last = out * dx;
	const double depth = out * dt;
	const double vol = depth * dx;
	rec.volume = rec.volume + vol;
	rec.active += out > 0.0 ? 1u : 0u;
}

} // namespace hp

#include <algorithm>
#include <string>
#include <vector>

namespace hp {

// The ring cell of index `at` on `edge` and its inward neighbour, as (column, GLOBAL row) pairs
struct OpenPlace { int64_t rx, ry, ix, iy; };
inline OpenPlace open_place(const int edge, const int64_t at, const int64_t cols, const int64_t global_rows)
{
	switch (edge) {
	case HP_EDGE_SOUTH: return {at, 0, at, 1};
	case HP_EDGE_NORTH: return {at, global_rows - 1, at, global_rows - 2};
	case HP_EDGE_WEST:  return {0, at, 1, at};
	default:            return {cols - 1, at, cols - 2, at};
	}
}

// -------------------------------------------------------------------------------------------------
// validate_open : every argument error of hp_boundary_add_open that needs no device, in the order the header lists them.
//     `existing`: the domain's segments so far, `taken`: the GLOBAL flat ids of their ring cells, sorted; on success `taken_after`
//     holds them merged with the new ones.  Returns false with `why` set.
// -------------------------------------------------------------------------------------------------
inline bool validate_open(const hp_open_segment_t* segments, const uint32_t count, const uint32_t existing, const int64_t cols, const int64_t global_rows,
                          const std::vector<uint64_t>& taken, std::vector<uint64_t>& taken_after, std::string& why)
{
	const std::string who = "hp_boundary_add_open";
	if (!segments) { why = who + ": segments == NULL"; return false; }
	if (count < 1) { why = who + ": count == 0"; return false; }
	if (count > OPEN_MAX_SEGMENTS || existing + count > OPEN_MAX_SEGMENTS) { why = who + ": more than 64 segments on the domain"; return false; }
	std::vector<uint64_t> ids;
	std::vector<uint32_t> seg_of;
	for (uint32_t k = 0; k < count; ++k) {
		const hp_open_segment_t& s = segments[k];
		const std::string which = who + ": segment " + std::to_string(k);
		if (s.edge != HP_EDGE_SOUTH && s.edge != HP_EDGE_NORTH && s.edge != HP_EDGE_WEST && s.edge != HP_EDGE_EAST) { why = which + ": unknown edge"; return false; }
		if (s.reserved != 0) { why = which + ": reserved must be 0"; return false; }
		if (s.first > s.last) { why = which + ": first > last"; return false; }
		const int64_t n = (s.edge == HP_EDGE_SOUTH || s.edge == HP_EDGE_NORTH) ? cols : global_rows;
		if (s.first < 1 || s.last > n - 2) {
			const int64_t at = s.first < 1 ? s.first : n - 1;
			why = which + ": index " + std::to_string(at) + " lies outside 1.." + std::to_string(n - 2) + " (the corner cells touch no interior cell)";
			return false;
		}
		for (int64_t at = s.first; at <= s.last; ++at) {
			const OpenPlace pl = open_place(s.edge, at, cols, global_rows);
			ids.push_back((uint64_t)pl.ry * (uint64_t)cols + (uint64_t)pl.rx);
			seg_of.push_back(k);
		}
	}
	// a ring cell listed twice: among the new ones (the message names the later segment), then against the domain's
	std::vector<size_t> order(ids.size());
	for (size_t j = 0; j < order.size(); ++j) order[j] = j;
	std::stable_sort(order.begin(), order.end(), [&](const size_t a, const size_t b) { return ids[a] < ids[b]; });
	for (size_t j = 1; j < order.size(); ++j)
		if (ids[order[j]] == ids[order[j - 1]]) {
			why = who + ": segment " + std::to_string(seg_of[order[j]]) + ": cell " + std::to_string(ids[order[j]]) + " is listed twice";
			return false;
		}
	std::vector<uint64_t> sorted(ids.size());
	for (size_t j = 0; j < order.size(); ++j) sorted[j] = ids[order[j]];
	for (size_t j = 0; j < sorted.size(); ++j)
		if (std::binary_search(taken.begin(), taken.end(), sorted[j])) {
			why = who + ": segment " + std::to_string(seg_of[order[j]]) + ": cell " + std::to_string(sorted[j]) + " is listed twice (an earlier segment of the domain has it)";
			return false;
		}
	taken_after.resize(taken.size() + sorted.size());
	std::merge(taken.begin(), taken.end(), sorted.begin(), sorted.end(), taken_after.begin());
	return true;
}

// the strip's selection of cells: a strip that stores the global rows [local_lo, local_hi), ghost rows included, keeps the ring cells
// whose row is one of them (the inward neighbour of a south / north cell lies on the grid's second / last but one row, which the strip
// that stores the edge row stores too: a strip is at least three rows)
inline bool open_strip_keeps(const int64_t ring_row, const int64_t inner_row, const int64_t local_lo, const int64_t local_hi)
{
	return ring_row >= local_lo && ring_row < local_hi && inner_row >= local_lo && inner_row < local_hi;
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_math.hpp"         // State4, Scalars, Params, make_side, face_solve

namespace hp {

// a listed ring cell as the kernel reads it: flat ids of the LOCAL array (the host has checked the global indices and the strip's selection)
struct OpenDev {
	unsigned long long r, i;                      // r == OPEN_ABSENT: this strip does not store the cell
	int edge, pad;
};

// -------------------------------------------------------------------------------------------------
// bdy_open : one lane per listed ring cell of one hp_boundary_add_open call, on the iteration's source buffer.  A ring cell is in at most
//     one segment of the domain and the kernel writes ring cells only, so no two lanes touch the same entry and no lane reads what another
//     writes: no atomics, no order.  The two state entries are loaded whole and r's is stored whole (32 B / 16 B: State4 is aligned to its
//     size).  The record is this lane's alone.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void bdy_open(const Params<T> p, const Scalars<T>* __restrict__ sc, const OpenDev* __restrict__ cells,
                                               const unsigned long long count, State4<T>* __restrict__ state, const T* __restrict__ bed,
                                               hp_open_record_t* __restrict__ records)
{
	const unsigned long long k = (unsigned long long)blockIdx.x * 64u + threadIdx.x;
	if (k >= count) return;
	const OpenDev c = cells[k];
	if (c.r == OPEN_ABSENT) return;
	const double dt = (double)sc->dt, dx = (double)p.dx;
	State4<T> cr = state[c.r];
	const State4<T> ci = state[c.i];
	const T br = bed[c.r], bi = bed[c.i];
	const bool along_x = c.edge == HP_EDGE_WEST || c.edge == HP_EDGE_EAST;
	const OpenRing R = {(double)cr.zmax, (double)br};
	const OpenInner I = {(double)ci.z, (double)ci.zmax, (double)(along_x ? ci.qx : ci.qy), (double)(along_x ? ci.qy : ci.qx), (double)bi};
	const OpenImposed o = open_impose(c.edge, R, I, dt);
	hp_open_record_t rec = records[k];
	if (o.inert) {
		open_record(rec, true, c.edge, 0.0, dt, dx);
		records[k] = rec;
		return;
	}
	cr.z = (T)o.lvl;
	cr.zmax = cr.zmax > cr.z ? cr.zmax : cr.z;
	cr.qx = (T)(along_x ? o.qn : o.qs);
	cr.qy = (T)(along_x ? o.qs : o.qn);
	state[c.r] = cr;
	// the face between i and r as the flux kernel's STRICT path forms it for cell i (tracer_step's four statements)
	const Side<T> sI = make_side<true>(ci.z, ci.qx, ci.qy, bi, p.vs);
	const Side<T> sR = make_side<true>(cr.z, cr.qx, cr.qy, br, p.vs);
	T F;
	if (c.edge == HP_EDGE_EAST)       F = face_solve<AXIS_X, true, true, false>(sI, sR, p.vs).forL.f0;
	else if (c.edge == HP_EDGE_WEST)  F = face_solve<AXIS_X, true, false, true>(sR, sI, p.vs).forR.f0;
	else if (c.edge == HP_EDGE_NORTH) F = face_solve<AXIS_Y, true, true, false>(sI, sR, p.vs).forL.f0;
	else                              F = face_solve<AXIS_Y, true, false, true>(sR, sI, p.vs).forR.f0;
	open_record(rec, false, c.edge, (double)F, dt, dx);
	records[k] = rec;
}

} // namespace hp
#endif // __HIPCC__
