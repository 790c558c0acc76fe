// hp_soil.hpp -- infiltration: the boundary kind that takes water from the surface into the soil, Green-Ampt by soil class
// (hp_boundary_add_infiltration).  Every cell carries a class id (0 = impervious) and its cumulative infiltrated depth F.  No
// reference counterpart: the reference takes water out through the uniform loss rate only.
// The arithmetic of one cell and one iteration is ONE definition in plain C++ (soil_step below): the kernel uses it,
// tests/soil_probe.cpp includes this file with a host compiler, and frontend.Infiltration restates it in NumPy.  All of it is fp64
// and uses correctly rounded add, multiply, divide, square root and compare only; nothing is fused: hp_engine.hip's translation
// unit is built with -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  The contract is in include/hipims_mi.h;
// the host side (hp_boundary_add_infiltration, the pass that launches bdy_infiltration, F's part of a checkpoint) is in hp_actors.hpp.
#pragma once
#include "../../include/hipims_mi.h"
#include <cstdint>

#ifdef __HIPCC__
#define HP_SOIL_FN __host__ __device__ __forceinline__
#else
#define HP_SOIL_FN static inline
#endif

namespace hp {

constexpr unsigned SOIL_CLASS_MAX = 255;                  // ids are bytes; 0 is "impervious"

struct SoilStep {
	double dF;                                            // what the cell takes up in this iteration: >= 0; 0: nothing is stored
	double z1;                                            // the level after it, before it is rounded on store
};

// The grid's edge ring: the outermost cells of the GLOBAL grid, which the flux kernels never write and the area boundaries never
// touch (hp_kernels.hpp: bdy_in_range).  The infiltration leaves them alone too: the engine prices the ring's part of the timestep
// once per upload, and a ring cell drained in one ping-pong buffer would come back from the other.
HP_SOIL_FN bool soil_on_ring(const long x, const long gy, const long cols, const long global_rows)
{
	return x <= 0 || gy <= 0 || x >= cols - 1 || gy >= global_rows - 1;
}

// -------------------------------------------------------------------------------------------------
// soil_step : steps 1 to 6 of the contract for one cell of class `cls` (never class 0, never a ring cell: those are the caller's tests).
//     S: suction * deficit, formed once on the host; F: the cell's cumulative infiltration; z, zmax, bed: widened;
//     dt: the "Timestep" scalar widened.
// -------------------------------------------------------------------------------------------------
HP_SOIL_FN SoilStep soil_step(const hp_soil_class_t& cls, const double S, const double F, const double z, const double zmax, const double bed,
                              const double dt)
{
	SoilStep r;
	r.dF = 0.0; r.z1 = z;
	if (dt <= 0.0 || !(zmax > -9999.0 && bed <= 9999.0)) return r;            // not counted in the sense of hp_domain_stats
	const double depth = z - bed;
	if (!(depth > 0.0)) return r;
	// the closed-form Green-Ampt step of CASC2D / GSSHA: finite at F == 0
	const double kd = cls.ks * dt;
	const double two_f = 2.0 * F;
	const double b = kd - two_f;
	const double bb = b * b;
	const double kd8 = 8.0 * kd;
	const double sf = S + F;
	const double rest = kd8 * sf;
	const double disc = bb + rest;
	const double root = __builtin_sqrt(disc);
	const double sum = b + root;
	double pot = 0.5 * sum;
	if (!(pot > 0.0)) pot = 0.0;
	const double room = cls.capacity - F;
	if (!(room > 0.0)) pot = 0.0;
	else if (room < pot) pot = room;
	const double dF = depth < pot ? depth : pot;
	if (dF > 0.0) {
		r.dF = dF;
		r.z1 = z - dF;
	}
	return r;
}

} // namespace hp

#include <cmath>
#include <string>

namespace hp {

// -------------------------------------------------------------------------------------------------
// validate_infiltration : every argument error of hp_boundary_add_infiltration that needs no device, in the order the header
//     lists them.  `cells`: cols * rows of the LOCAL array.  Returns false with `why` set; where a cell is at fault `why` names
//     the first offending one.  On success `pervious` counts the cells of a class other than 0.
// -------------------------------------------------------------------------------------------------
inline bool validate_infiltration(const hp_infiltration_desc_t* desc, const uint64_t cells, uint64_t& pervious, std::string& why)
{
	const std::string who = "hp_boundary_add_infiltration";
	if (!desc) { why = who + ": desc == NULL"; return false; }
	if (desc->struct_size != sizeof(hp_infiltration_desc_t)) { why = "hp_infiltration_desc_t size mismatch (ABI)"; return false; }
	if (!desc->classes) { why = who + ": classes == NULL"; return false; }
	if (!desc->soil_of_cell) { why = who + ": soil_of_cell == NULL"; return false; }
	if (desc->class_count < 1 || desc->class_count > SOIL_CLASS_MAX) { why = who + ": class_count outside 1..255"; return false; }
	for (uint32_t k = 0; k < desc->class_count; ++k) {
		const hp_soil_class_t& c = desc->classes[k];
		const std::string which = who + ": class " + std::to_string(k + 1);
		if (!std::isfinite(c.ks) || !std::isfinite(c.suction)) { why = which + ": ks and suction must be finite"; return false; }
		if (c.ks < 0.0) { why = which + ": negative ks"; return false; }
		if (c.suction < 0.0) { why = which + ": negative suction"; return false; }
		if (!(c.deficit >= 0.0 && c.deficit <= 1.0)) { why = which + ": the moisture deficit lies in [0, 1]"; return false; }
		if (!(c.capacity >= 0.0)) { why = which + ": the capacity is >= 0 (+inf for none)"; return false; }
		if (!std::isfinite(c.ks * 1e6)) { why = which + ": ks * 1e6 must be finite"; return false; }
		if (!std::isfinite(c.suction * c.deficit)) { why = which + ": suction * deficit must be finite"; return false; }
	}
	pervious = 0;
	for (uint64_t i = 0; i < cells; ++i) {
		const unsigned id = desc->soil_of_cell[i];
		if (id > desc->class_count) { why = who + ": cell " + std::to_string(i) + " has class id " + std::to_string(id) + ", above class_count"; return false; }
		pervious += id != 0 ? 1u : 0u;
	}
	if (desc->initial)
		for (uint64_t i = 0; i < cells; ++i)
			if (!std::isfinite(desc->initial[i]) || desc->initial[i] < 0.0) { why = who + ": cell " + std::to_string(i) + ": initial must be finite and >= 0"; return false; }
	return true;
}

// the class table as the kernel reads it: indexed by the id itself (entry 0 is never read)
struct SoilTable {
	hp_soil_class_t cls[SOIL_CLASS_MAX + 1];
	double          S[SOIL_CLASS_MAX + 1];                // suction * deficit
};
inline void soil_table(const hp_infiltration_desc_t* desc, SoilTable& t)
{
	for (unsigned k = 0; k <= SOIL_CLASS_MAX; ++k) { t.cls[k] = hp_soil_class_t{0.0, 0.0, 0.0, 0.0}; t.S[k] = 0.0; }
	for (uint32_t k = 0; k < desc->class_count; ++k) {
		t.cls[k + 1] = desc->classes[k];
		t.S[k + 1] = desc->classes[k].suction * desc->classes[k].deficit;
	}
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_math.hpp"         // State4, Scalars, Params

namespace hp {

constexpr unsigned SOIL_BLOCK = 256;                      // four waves side by side along x
constexpr unsigned SOIL_GRID_MAX = 2048;                  // blocks of a launch; the rows beyond go by grid stride

// -------------------------------------------------------------------------------------------------
// bdy_infiltration : one lane per cell along x, rows by grid stride over blockIdx.y, on the iteration's source buffer.  A
//     streaming pass over the cells inside the grid's edge ring (soil_on_ring: the ring's rows and columns are skipped before
//     anything is read): every lane reads its class byte (64 consecutive bytes a wave); a wave whose 64 cells are all of class 0
//     touches nothing else (the branch is skipped with an empty lane mask).  Where the class is not 0 the lane loads the first
//     half of the State4 entry (the level, and the maximum level that the "counted" test of step 1 needs: one 16 B / 8 B load;
//     State4 is aligned to its size), the bed and F, and stores the level and F only where dF > 0.  Every cell is its lane's
//     alone: no atomics, no LDS, no order.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SOIL_BLOCK) void bdy_infiltration(const Params<T> p, const Scalars<T>* __restrict__ sc, const SoilTable* __restrict__ table,
                                                               const unsigned char* __restrict__ soil_of_cell, double* __restrict__ F,
                                                               State4<T>* __restrict__ state, const T* __restrict__ bed)
{
	const double dt = (double)sc->dt;
	if (dt <= 0.0) return;                                                    // (the same in every lane)
	const long x = (long)blockIdx.x * SOIL_BLOCK + threadIdx.x;
	if (x >= p.cols) return;
	for (long y = blockIdx.y; y < p.rows; y += gridDim.y) {
		if (soil_on_ring(x, y + p.row_offset, p.cols, p.global_rows)) continue;   // (a ring row: the same in every lane; a ring column: two lanes a row)
		const size_t i = (size_t)y * (size_t)p.cols + (size_t)x;
		const unsigned id = soil_of_cell[i];
		if (id == 0) continue;
		T* const entry = (T*)(state + i);
		const T z = entry[0], zmax = entry[1];
		const double f = F[i];
		const SoilStep s = soil_step(table->cls[id], table->S[id], f, (double)z, (double)zmax, (double)bed[i], dt);
		if (s.dF > 0.0) {
			entry[0] = (T)s.z1;
			F[i] = f + s.dF;
		}
	}
}

// the launch shape over a cols x rows array
inline dim3 soil_grid(const long cols, const long rows)
{
	const unsigned gx = (unsigned)((cols + SOIL_BLOCK - 1) / SOIL_BLOCK);
	const unsigned room = SOIL_GRID_MAX / gx > 0 ? SOIL_GRID_MAX / gx : 1;
	return dim3(gx, (unsigned)(rows < (long)room ? rows : (long)room));
}

} // namespace hp
#endif // __HIPCC__
