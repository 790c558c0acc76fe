// hp_tracer.hpp -- the passive tracer: a solute mass per unit area M (concentration x depth, fp64 whatever the domain's precision)
// carried with the water (hp_tracer_enable).  Once per iteration, behind every boundary of the list and in front of the flux launch,
// the sources add their mass (tracer_sources) and tracer_step moves M through the four faces of every cell by the mass fluxes the
// flux kernel is about to form from the same source buffer, upwinded.  No reference counterpart: the reference moves water only.
// The fp64 arithmetic behind the face fluxes is ONE definition in plain C++ (tracer_conc, tracer_update, tracer_source_add below):
// the kernels use it, tests/tracer_probe.cpp includes this file with a host compiler, and frontend.Tracer restates it in NumPy.  It
// uses correctly rounded add, multiply, divide and compare only; nothing is fused: hp_engine.hip's translation unit is built with
// -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  The face fluxes themselves are the STRICT face solve of
// hp_math.hpp in the domain's precision, whatever the domain's math mode.  The contract is in include/hipims_mi.h; the host side
// (hp_tracer_*, the launches in front of the flux kernel, M's part of a checkpoint) is in hp_actors.hpp.
#pragma once
#include "../../include/hipims_mi.h"
#include "hp_bed.hpp"          // bed_fraction: the one interpolation rule of a {time, value} series
#include <cstdint>

#ifdef __HIPCC__
#define HP_TRACER_FN __host__ __device__ __forceinline__
#else
#define HP_TRACER_FN static inline
#endif

namespace hp {

constexpr unsigned TRACER_MAX_SOURCES = 64;
constexpr unsigned TRACER_MAX_SERIES = 4096;              // entries of one source's series
constexpr uint64_t TRACER_MAX_CELLS = 1048576;            // listed cells of all sources of a domain together
constexpr double   TRACER_DEPTH_MIN = 1e-10;              // at or below this depth a cell has no concentration to give

// step 3: the concentration a cell gives to the water that leaves it.  h: the RAW depth Z - bed, widened
HP_TRACER_FN double tracer_conc(const double M, const double h) { return h > TRACER_DEPTH_MIN ? M / h : 0.0; }

// steps 4 and 5: M' of a cell from its M, the five concentrations and the four face mass fluxes (widened), in this order
HP_TRACER_FN double tracer_update(const double M, const double cC, const double cN, const double cS, const double cE, const double cW,
                                  const double FN, const double FS, const double FE, const double FW, const double dt, const double dx)
{
	const double GE = FE > 0.0 ? FE * cC : FE * cE;
	const double GW = FW > 0.0 ? FW * cW : FW * cC;
	const double GN = FN > 0.0 ? FN * cC : FN * cN;
	const double GS = FS > 0.0 ? FS * cS : FS * cC;
	const double ex = GE - GW;
	const double ey = GN - GS;
	const double sum = ex + ey;
	const double div = sum / dx;
	const double step = dt * div;
	return M - step;
}

// the source step of one listed cell: rate in units per second at the device's "Time", dt the "Timestep" scalar (> 0: the caller's test)
HP_TRACER_FN double tracer_source_add(const double M, const double rate, const double dt, const double dx)
{
	const double mass = rate * dt;
	const double area = dx * dx;
	const double add = mass / area;
	return M + add;
}

// the rate of a source at time t: the bed shapes' rule on {time, mass rate} pairs
HP_TRACER_FN double tracer_rate(const double* series, const unsigned n, const double t) { return bed_fraction(series, n, t); }

} // namespace hp

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace hp {

// The host's copies of a domain's source lists (TracerStore, hp_domain.hpp)
struct TracerHost {
	std::vector<uint64_t> listed;                     // ids of every cell of every source, sorted: the repeated-cell check
	std::vector<uint64_t> cells;                      // source after source
	std::vector<unsigned char> source_of;
	std::vector<double>   series;
	std::vector<unsigned> series_off = {0u};          // [sources + 1]
};

// -------------------------------------------------------------------------------------------------
// validate_tracer_enable : every argument error of hp_tracer_enable that needs no device.  `cells`: cols * rows of the local array.
//     Returns false with `why` set; where a cell is at fault `why` names the first offending one.
// -------------------------------------------------------------------------------------------------
inline bool validate_tracer_enable(const hp_tracer_desc_t* desc, const uint64_t cells, std::string& why)
{
	const std::string who = "hp_tracer_enable";
	if (!desc) { why = who + ": desc == NULL"; return false; }
	if (desc->struct_size != sizeof(hp_tracer_desc_t)) { why = "hp_tracer_desc_t size mismatch (ABI)"; return false; }
	if (desc->initial)
		for (uint64_t i = 0; i < cells; ++i)
			if (!std::isfinite(desc->initial[i]) || desc->initial[i] < 0.0) { why = who + ": cell " + std::to_string(i) + ": initial must be finite and >= 0"; return false; }
	return true;
}

// -------------------------------------------------------------------------------------------------
// validate_tracer_source : every argument error of hp_tracer_add_source that needs no device, in the order the header lists them.
//     `have`: the domain's lists so far.  On success `listed_after` holds have.listed merged with the new cells.
// -------------------------------------------------------------------------------------------------
inline bool validate_tracer_source(const uint64_t* cells, const uint64_t count, const double* series, const uint32_t entries, const TracerHost& have,
                                   const uint64_t cols, const uint64_t rows, std::vector<uint64_t>& listed_after, std::string& why)
{
	const std::string who = "hp_tracer_add_source";
	if (!cells || !series) { why = who + ": cells / series == NULL"; return false; }
	if (entries < 1 || entries > TRACER_MAX_SERIES) { why = who + ": entries outside 1..4096"; return false; }
	if (count < 1 || count > TRACER_MAX_CELLS) { why = who + ": count outside 1..1048576"; return false; }
	for (unsigned k = 0; k < entries; ++k) {
		const double t = series[2 * k], r = series[2 * k + 1];
		if (!std::isfinite(t) || (k > 0 && !(t > series[2 * k - 2]))) { why = who + ": series entry " + std::to_string(k) + ": times must be finite and strictly increasing"; return false; }
		if (!std::isfinite(r)) { why = who + ": series entry " + std::to_string(k) + ": the mass rate must be finite"; return false; }
	}
	for (uint64_t k = 0; k < count; ++k) {
		if (cells[k] >= cols * rows) { why = who + ": cell " + std::to_string(cells[k]) + " lies outside the grid"; return false; }
		const uint64_t y = cells[k] / cols, x = cells[k] - y * cols;
		if (x == 0 || y == 0 || x + 1 >= cols || y + 1 >= rows) { why = who + ": cell " + std::to_string(cells[k]) + " lies on the grid's edge ring"; return false; }
	}
	std::vector<uint64_t> sorted(cells, cells + count);
	std::sort(sorted.begin(), sorted.end());
	auto twice = std::adjacent_find(sorted.begin(), sorted.end());
	if (twice != sorted.end()) { why = who + ": cell " + std::to_string(*twice) + " is listed twice"; return false; }
	if (have.series_off.size() > TRACER_MAX_SOURCES) { why = who + ": more than 64 sources"; return false; }
	if (have.listed.size() + count > TRACER_MAX_CELLS) { why = who + ": more than 1048576 cells over all sources"; return false; }
	listed_after.resize(have.listed.size() + (size_t)count);
	std::merge(have.listed.begin(), have.listed.end(), sorted.begin(), sorted.end(), listed_after.begin());
	twice = std::adjacent_find(listed_after.begin(), listed_after.end());
	if (twice != listed_after.end()) { why = who + ": cell " + std::to_string(*twice) + " is listed twice (another source has it)"; return false; }
	return true;
}

// The device block of the lists of n cells, `pairs` series entries and `sources` sources (TracerLists points into it), in bytes:
// [cells: n x 8 | series: pairs x 16 | series_off: (sources + 1) x 4, to 8 | source_of: n]
struct TracerLayout { size_t cells, series, series_off, source_of, bytes; };
inline TracerLayout tracer_layout(const size_t n, const size_t pairs, const size_t sources)
{
	TracerLayout l;
	l.cells = 0;
	l.series = l.cells + n * 8;
	l.series_off = l.series + pairs * 16;
	l.source_of = l.series_off + ((sources + 1) * 4 + 7) / 8 * 8;
	l.bytes = l.source_of + std::max<size_t>(n, 1);
	return l;
}
inline std::vector<unsigned char> tracer_image(const TracerLayout& l, const TracerHost& h)
{
	std::vector<unsigned char> image(l.bytes, 0);
	if (!h.cells.empty()) {
		std::memcpy(image.data() + l.cells, h.cells.data(), h.cells.size() * 8);
		std::memcpy(image.data() + l.source_of, h.source_of.data(), h.source_of.size());
	}
	if (!h.series.empty()) std::memcpy(image.data() + l.series, h.series.data(), h.series.size() * 8);
	std::memcpy(image.data() + l.series_off, h.series_off.data(), h.series_off.size() * 4);
	return image;
}

} // namespace hp

#ifdef __HIPCC__
#include "hp_math.hpp"         // State4, Scalars, Params, make_side, face_solve

namespace hp {

// The sources' lists in device memory (one allocation, rewritten by every hp_tracer_add_source)
struct TracerLists {
	const unsigned long long* cells;              // [count] flat ids of the local array
	const unsigned char*      source_of;          // [count] the cell's source
	const double*             series;             // all sources' {time, mass rate} pairs, source after source
	const unsigned*           series_off;         // [sources + 1] entries (pairs) into `series`
	unsigned long long        count;
	unsigned                  sources;            // 1 .. TRACER_MAX_SOURCES
};

// -------------------------------------------------------------------------------------------------
// tracer_sources : one small launch over the listed cells, in front of tracer_step, in place on the M the step is about to read.
//     Per block the first `sources` threads form the sources' rates into LDS from the device's own "Time" (a binary search each),
//     one barrier, then the cells by grid stride.  Nothing happens when dt <= 0.  A cell is listed once over all sources, so no two
//     threads touch the same entry.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void tracer_sources(const Params<T> p, const Scalars<T>* __restrict__ sc, const TracerLists L, double* __restrict__ M)
{
	__shared__ double rate[TRACER_MAX_SOURCES];
	const double dt = (double)sc->dt, t = (double)sc->t;
	if (!(dt > 0.0)) return;                                                  // (the same in every lane)
	if (threadIdx.x < L.sources) {
		const unsigned lo = L.series_off[threadIdx.x], hi = L.series_off[threadIdx.x + 1];
		rate[threadIdx.x] = tracer_rate(L.series + 2ull * lo, hi - lo, t);
	}
	__syncthreads();
	const double dx = (double)p.dx;
	for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < L.count; k += (unsigned long long)gridDim.x * 256u) {
		const unsigned long long cell = L.cells[k];
		M[cell] = tracer_source_add(M[cell], rate[L.source_of[k]], dt, dx);
	}
}

// -------------------------------------------------------------------------------------------------
// tracer_step : one lane per cell, godunov_basic's dataflow (hp_kernels.hpp): 64 columns of a row per wave, four rows per block,
//     four STRICT face solves per cell of which only the mass flux is kept (every face is solved from both of its sides: the two
//     cells form the same statements the flux kernel's STRICT path forms for them).  Reads the iteration's source buffer, the bed
//     and M0; writes M1 at EVERY cell of the array -- the copy cases store M0's value -- so the two buffers never hold anything
//     stale.  Every cell is its lane's alone: no atomics, no LDS, no order.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void tracer_step(const Params<T> p, const Scalars<T>* __restrict__ sc, const T* __restrict__ bed,
                                                   const State4<T>* __restrict__ src, const double* __restrict__ M0, double* __restrict__ M1)
{
	const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
	const long y = (long)blockIdx.y * blockDim.y + threadIdx.y;
	if (x >= p.cols || y >= p.rows) return;
	const size_t id = (size_t)y * p.cols + x;
	const double m = M0[id];
	const T dt = sc->dt;
	// the copy cases, in the contract's order: the ring of godunov_cell, dt <= 0, a disabled cell, five dry cells (quirk Q3)
	if (x <= 0 || y <= 0 || x >= p.cols - 1 || y >= p.rows - 1 || dt <= T(0)) { M1[id] = m; return; }
	const State4<T> c = src[id];
	const T zb = bed[id];
	if (c.zmax <= T(-9999.0) || c.z == T(-9999.0)) { M1[id] = m; return; }

	const size_t iW = id - 1, iE = id + 1, iS = id - p.cols, iN = id + p.cols;
	const State4<T> cW = src[iW], cE = src[iE], cS = src[iS], cN = src[iN];
	const T zW = bed[iW], zE = bed[iE], zS = bed[iS], zN = bed[iN];
	if (c.z - zb < p.vs && cN.z - zN < p.vs && cE.z - zE < p.vs && cS.z - zS < p.vs && cW.z - zW < p.vs) { M1[id] = m; return; }

	const Side<T> sC = make_side<true>(c.z, c.qx, c.qy, zb, p.vs);
	const Side<T> sN = make_side<true>(cN.z, cN.qx, cN.qy, zN, p.vs);
	const Side<T> sE = make_side<true>(cE.z, cE.qx, cE.qy, zE, p.vs);
	const Side<T> sS = make_side<true>(cS.z, cS.qx, cS.qy, zS, p.vs);
	const Side<T> sW = make_side<true>(cW.z, cW.qx, cW.qy, zW, p.vs);
	const double FN = (double)face_solve<AXIS_Y, true, true, false>(sC, sN, p.vs).forL.f0;
	const double FS = (double)face_solve<AXIS_Y, true, false, true>(sS, sC, p.vs).forR.f0;
	const double FE = (double)face_solve<AXIS_X, true, true, false>(sC, sE, p.vs).forL.f0;
	const double FW = (double)face_solve<AXIS_X, true, false, true>(sW, sC, p.vs).forR.f0;

	const double cc = tracer_conc(m, (double)c.z - (double)zb);
	const double cn = tracer_conc(M0[iN], (double)cN.z - (double)zN);
	const double cs = tracer_conc(M0[iS], (double)cS.z - (double)zS);
	const double ce = tracer_conc(M0[iE], (double)cE.z - (double)zE);
	const double cw = tracer_conc(M0[iW], (double)cW.z - (double)zW);
	M1[id] = tracer_update(m, cc, cn, cs, ce, cw, FN, FS, FE, FW, (double)dt, (double)p.dx);
}

} // namespace hp
#endif // __HIPCC__
