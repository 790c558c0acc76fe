// hp_tracer.hpp -- the passive tracer: a solute mass per unit area M (concentration x depth, fp64 whatever the domain's precision)
// carried with the water (hp_tracer_enable).  Once per iteration, behind every boundary of the list and in front of the flux launch,
// the sources add their mass (tracer_sources) and tracer_step moves M through the four faces of every cell by the mass fluxes the
// flux kernel is about to form from the same source buffer, upwinded.  No reference counterpart: the reference moves water only.
// The fp64 arithmetic behind the face fluxes is ONE definition in plain C++ (tracer_conc, tracer_update, tracer_source_add below):
// the kernels use it, tests/tracer_probe.cpp includes this file with a host compiler, and frontend.Tracer restates it in NumPy.  It
// uses correctly rounded add, multiply, divide and compare only; nothing is fused: hp_engine.hip's translation unit is built with
// -ffp-contract=off -fno-fast-math (the Makefile), the probe likewise.  The face fluxes themselves are the STRICT face solve of
// hp_math.hpp in the domain's precision, whatever the domain's math mode.  A tracer SET (hp_tracer_enable_set) carries up to 8 species,
// planes of M one after the other, by one launch of tracer_step_set -- the face fluxes formed once per cell -- and lets each decay
// (tracer_decay; frontend.TracerSet).  A species of a set may also exchange mass with a deposit D on the ground (hp_tracer_set_exchange:
// tracer_exchange below, step 7, behind the decay in the same launch; its cube root is hp_crmath.h's).  The contract is in
// include/hipims_mi.h; the host side (hp_tracer_*, the launches in front of the flux kernel, M's and D's part of a checkpoint) is in hp_actors.hpp.
#pragma once
#include "../../include/hipims_mi.h"
#include "hp_bed.hpp"          // bed_fraction: the one interpolation rule of a {time, value} series
#ifdef __HIPCC__
#define HP_CR_FN __host__ __device__ __forceinline__
#endif
#include "hp_crmath.h"         // hp_cr_cbrt: the correctly rounded cube root of the bed shear stress, for host and device
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

// step 6 (tracer sets): first-order decay at the rate lambda over dt, implicit Euler; lambda == 0 divides nothing
HP_TRACER_FN double tracer_decay(const double M, const double lambda, const double dt)
{
	if (!(lambda > 0.0 && dt > 0.0)) return M;
	const double growth = lambda * dt;
	const double denom = 1.0 + growth;
	return M / denom;
}

// step 7 (tracer sets): what one species exchanges with its deposit D -- Krone's deposition below tau_deposit, Partheniades' erosion
// above tau_erode.  One definition in two halves, because the shear stress depends on the water only: a lane forms it once for all species
struct TracerExchangeParams { double settling, tau_deposit, tau_erode, erodibility; };
struct TracerPair { double M, D; };
constexpr double TRACER_RHO_G = 9810.0;                   // rho g of the Manning bed shear stress, N/m3

// the Manning bed shear stress rho g n^2 |u|^2 / h^(1/3) of a cell deeper than TRACER_DEPTH_MIN (the caller's test); NaN discharges give NaN
HP_TRACER_FN double tracer_shear(const double h, const double qx, const double qy, const double n)
{
	const double vx = qx / h;
	const double vy = qy / h;
	const double sp2 = vx * vx + vy * vy;
	const double nn = n * n;
	return ((TRACER_RHO_G * nn) * sp2) / hp_cr_cbrt(h);
}
// ... and what a species does at that shear stress: implicit Euler into D, or a clipped explicit step out of it; a NaN tau does neither
HP_TRACER_FN TracerPair tracer_exchange_at(const double M, const double D, const double tau, const double h, const double dt, const TracerExchangeParams q)
{
	TracerPair out = {M, D};
	if (q.settling > 0.0 && M > 0.0 && tau < q.tau_deposit) {
		const double pd = q.tau_deposit == __builtin_inf() ? 1.0 : 1.0 - tau / q.tau_deposit;
		const double k = (q.settling * pd) * dt;
		const double r = k / h;
		const double M3 = M / (1.0 + r);
		const double dep = M - M3;
		out.D = D + dep;
		out.M = M3;
	} else if (q.erodibility > 0.0 && D > 0.0 && tau > q.tau_erode) {
		const double ex = tau / q.tau_erode - 1.0;
		double ero = (q.erodibility * ex) * dt;
		if (ero > D) ero = D;
		out.D = D - ero;
		out.M = M + ero;
	}
	return out;
}
// step 7 of one cell that is no copy case: M the decayed M'', h the RAW depth, qx qy its discharge, n its Manning value, all widened
HP_TRACER_FN TracerPair tracer_exchange(const double M, const double D, const double h, const double qx, const double qy, const double n,
                                        const double dt, const TracerExchangeParams q)
{
	if (!(h > TRACER_DEPTH_MIN)) return TracerPair{M, D};
	return tracer_exchange_at(M, D, tracer_shear(h, qx, qy, n), h, dt, q);
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
	std::vector<uint64_t> listed;                     // species * (cols * rows) + id of every cell of every source, sorted: the repeated-cell check
	std::vector<uint64_t> cells;                      // source after source
	std::vector<unsigned char> source_of;
	std::vector<unsigned char> species_of;            // the species of each listed cell (all 0 for a single tracer)
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
// validate_tracer_set_enable : every argument error of hp_tracer_enable_set that needs no device.  `cells`: cols * rows of the local array.
//     Returns false with `why` set; a bad initial value is named by its species and its cell.
// -------------------------------------------------------------------------------------------------
inline bool validate_tracer_set_enable(const hp_tracer_set_desc_t* desc, const uint64_t cells, std::string& why)
{
	const std::string who = "hp_tracer_enable_set";
	if (!desc) { why = who + ": desc == NULL"; return false; }
	if (desc->struct_size != sizeof(hp_tracer_set_desc_t)) { why = "hp_tracer_set_desc_t size mismatch (ABI)"; return false; }
	if (desc->species < 1 || desc->species > HP_TRACER_MAX_SPECIES) { why = who + ": species outside 1..8"; return false; }
	if (desc->decay)
		for (uint32_t s = 0; s < desc->species; ++s)
			if (!std::isfinite(desc->decay[s]) || desc->decay[s] < 0.0) { why = who + ": species " + std::to_string(s) + ": the decay rate must be finite and >= 0"; return false; }
	if (desc->initial)
		for (uint32_t s = 0; s < desc->species; ++s)
			for (uint64_t i = 0; i < cells; ++i) {
				const double m = desc->initial[(uint64_t)s * cells + i];
				if (!std::isfinite(m) || m < 0.0) { why = who + ": species " + std::to_string(s) + ", cell " + std::to_string(i) + ": initial must be finite and >= 0"; return false; }
			}
	return true;
}

// -------------------------------------------------------------------------------------------------
// validate_tracer_exchange : every argument error of hp_tracer_set_exchange that needs no device, in the order the header lists them.
//     `species_count`: K of the domain's set; `cells`: cols * rows of the local array.  Returns false with `why` set.
// -------------------------------------------------------------------------------------------------
inline bool validate_tracer_exchange(const hp_tracer_exchange_desc_t* desc, const uint32_t species_count, const uint64_t cells, std::string& why)
{
	const std::string who = "hp_tracer_set_exchange";
	if (!desc) { why = who + ": desc == NULL"; return false; }
	if (desc->struct_size != sizeof(hp_tracer_exchange_desc_t)) { why = "hp_tracer_exchange_desc_t size mismatch (ABI)"; return false; }
	if (desc->species >= species_count) { why = who + ": species " + std::to_string(desc->species) + " of a tracer of " + std::to_string(species_count); return false; }
	if (!std::isfinite(desc->settling) || desc->settling < 0.0) { why = who + ": settling must be finite and >= 0"; return false; }
	if (!(desc->tau_deposit > 0.0)) { why = who + ": tau_deposit must be > 0 (+inf allowed)"; return false; }
	if (std::isnan(desc->tau_erode) || desc->tau_erode < desc->tau_deposit) { why = who + ": tau_erode must be >= tau_deposit (+inf allowed)"; return false; }
	if (!std::isfinite(desc->erodibility) || desc->erodibility < 0.0) { why = who + ": erodibility must be finite and >= 0"; return false; }
	if (desc->deposit_initial)
		for (uint64_t i = 0; i < cells; ++i)
			if (!std::isfinite(desc->deposit_initial[i]) || desc->deposit_initial[i] < 0.0) { why = who + ": cell " + std::to_string(i) + ": deposit_initial must be finite and >= 0"; return false; }
	return true;
}

// -------------------------------------------------------------------------------------------------
// validate_tracer_source : every argument error of hp_tracer_add_source (`who`; hp_tracer_add_source_to likewise) that needs no device, in
//     the order the header lists them.  `have`: the domain's lists so far; `species` of `species_count`: the species the source feeds (a
//     single tracer: 0 of 1).  A cell may be listed once per species.  On success `listed_after` holds have.listed merged with the new keys.
// -------------------------------------------------------------------------------------------------
inline bool validate_tracer_source(const uint64_t* cells, const uint64_t count, const double* series, const uint32_t entries, const TracerHost& have,
                                   const uint64_t cols, const uint64_t rows, std::vector<uint64_t>& listed_after, std::string& why,
                                   const uint32_t species = 0, const uint32_t species_count = 1, const std::string& who = "hp_tracer_add_source")
{
	if (species >= species_count) { why = who + ": species " + std::to_string(species) + " of a tracer of " + std::to_string(species_count); return false; }
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
	const uint64_t plane = cols * rows;                                       // a listed cell's key: species * plane + cell
	std::vector<uint64_t> sorted(cells, cells + count);
	for (uint64_t& key : sorted) key += (uint64_t)species * plane;
	std::sort(sorted.begin(), sorted.end());
	auto twice = std::adjacent_find(sorted.begin(), sorted.end());
	if (twice != sorted.end()) { why = who + ": cell " + std::to_string(*twice - (uint64_t)species * plane) + " is listed twice"; return false; }
	if (have.series_off.size() > TRACER_MAX_SOURCES) { why = who + ": more than 64 sources"; return false; }
	if (have.listed.size() + count > TRACER_MAX_CELLS) { why = who + ": more than 1048576 cells over all sources"; return false; }
	listed_after.resize(have.listed.size() + (size_t)count);
	std::merge(have.listed.begin(), have.listed.end(), sorted.begin(), sorted.end(), listed_after.begin());
	twice = std::adjacent_find(listed_after.begin(), listed_after.end());
	if (twice != listed_after.end()) { why = who + ": cell " + std::to_string(*twice - (uint64_t)species * plane) + " is listed twice (another source has it)"; return false; }
	return true;
}

// The device block of the lists of n cells, `pairs` series entries and `sources` sources (TracerLists points into it), in bytes:
// [cells: n x 8 | series: pairs x 16 | series_off: (sources + 1) x 4, to 8 | source_of: n | species_of: n]
struct TracerLayout { size_t cells, series, series_off, source_of, species_of, bytes; };
inline TracerLayout tracer_layout(const size_t n, const size_t pairs, const size_t sources)
{
	TracerLayout l;
	l.cells = 0;
	l.series = l.cells + n * 8;
	l.series_off = l.series + pairs * 16;
	l.source_of = l.series_off + ((sources + 1) * 4 + 7) / 8 * 8;
	l.species_of = l.source_of + std::max<size_t>(n, 1);
	l.bytes = l.species_of + std::max<size_t>(n, 1);
	return l;
}
inline std::vector<unsigned char> tracer_image(const TracerLayout& l, const TracerHost& h)
{
	std::vector<unsigned char> image(l.bytes, 0);
	if (!h.cells.empty()) {
		std::memcpy(image.data() + l.cells, h.cells.data(), h.cells.size() * 8);
		std::memcpy(image.data() + l.source_of, h.source_of.data(), h.source_of.size());
		std::memcpy(image.data() + l.species_of, h.species_of.data(), h.species_of.size());
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
	const unsigned char*      species_of;         // [count] the plane of M the entry writes (a single tracer: all 0)
	unsigned long long        plane;              // cells of one plane: cols * rows
	const double*             series;             // all sources' {time, mass rate} pairs, source after source
	const unsigned*           series_off;         // [sources + 1] entries (pairs) into `series`
	unsigned long long        count;
	unsigned                  sources;            // 1 .. TRACER_MAX_SOURCES
};

// -------------------------------------------------------------------------------------------------
// tracer_sources : one small launch over the listed cells, in front of tracer_step, in place on the M the step is about to read.
//     Per block the first `sources` threads form the sources' rates into LDS from the device's own "Time" (a binary search each),
//     one barrier, then the cells by grid stride.  Nothing happens when dt <= 0.  Each entry writes the plane of its species (M: the
//     current planes, species after species); a (species, cell) pair is listed once over all sources, so no two threads touch the same value.
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
		const unsigned long long at = (unsigned long long)L.species_of[k] * L.plane + L.cells[k];
		M[at] = tracer_source_add(M[at], rate[L.source_of[k]], dt, dx);
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

// The decay rates of a set's species, by value in the kernel's arguments
struct TracerRates { double lambda[HP_TRACER_MAX_SPECIES]; };

// What tracer_step_set<T, true> takes besides: the K planes of D, the Manning array the flux kernel reads (Params says whether it is
// uniform) and the species' parameters by value; bit s of `exchanging`: species s has settling > 0 or erodibility > 0.  The <T, false>
// kernel takes an empty one
template <typename T, bool EXCHANGE> struct TracerBedArgs {};
template <typename T> struct TracerBedArgs<T, true> {
	double*              D;
	const T*             manning;
	unsigned             exchanging;
	TracerExchangeParams of[HP_TRACER_MAX_SPECIES];
};

constexpr int TRACER_SET_ROWS = 4;                    // rows of a block of tracer_step_set: one wave each
constexpr int TRACER_SET_PITCH = 66;                  // 64 columns and the two halo columns

// -------------------------------------------------------------------------------------------------
// tracer_step_set : tracer_step for the K species of a set (hp_tracer_enable_set), planes of p.cols * p.rows doubles, species after
//     species.  Same block shape, same copy cases, same four STRICT face solves -- formed ONCE per cell: they depend on the water only.
//     Then per species: every lane forms the concentration of its own cell (one correctly rounded division), the lanes of the first
//     two waves also those of the tile's halo (its row below, its row above, its two side columns: 136 cells), all into an LDS tile
//     of (rows + 2) x 66 doubles; one barrier; the lane reads its four neighbours' from the tile and updates (steps 4 and 5), then
//     decays (step 6).  That is (256 + 136) divisions a block and species where five per lane would be 1280.  A neighbour's
//     concentration is the same statement on the same operands whichever lane forms it, so the bits are tracer_step's.  The tile is
//     double-buffered: one barrier per species.  Lanes of the copy cases and lanes outside the array reach every barrier (a flag, no
//     return); a block without a single moving cell -- still or dry ground, dt <= 0 -- skips the tile: block-uniform, by one
//     __syncthreads_or.  Writes M1 at EVERY cell of every plane.
//     EXCHANGE (a set with a species that exchanges with its deposit, hp_tracer_set_exchange): a moving lane deeper than
//     TRACER_DEPTH_MIN forms its bed shear stress once, from the cell it has loaded anyway; behind the decay, for every exchanging
//     species (a uniform branch: the flag is a kernel argument), it loads its own D, applies step 7 and stores D if it changed.  D is
//     its lane's alone and updated in place.  The block without a moving cell exchanges nothing.  <T, false> is the kernel without it.
// -------------------------------------------------------------------------------------------------
template <typename T, bool EXCHANGE>
__global__ __launch_bounds__(256) void tracer_step_set(const Params<T> p, const Scalars<T>* __restrict__ sc, const T* __restrict__ bed,
                                                       const State4<T>* __restrict__ src, const double* __restrict__ M0, double* __restrict__ M1,
                                                       const unsigned species, const TracerRates rates, const TracerBedArgs<T, EXCHANGE> X)
{
	__shared__ double tile[2][TRACER_SET_ROWS + 2][TRACER_SET_PITCH];
	const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
	const long x0 = (long)blockIdx.x * 64, y0 = (long)blockIdx.y * TRACER_SET_ROWS;
	const long x = x0 + tx, y = y0 + ty;
	const bool inside = x < p.cols && y < p.rows;
	const size_t plane = (size_t)p.cols * (size_t)p.rows;
	const size_t id = inside ? (size_t)y * p.cols + x : 0;
	const T dt = sc->dt;
	const double dt64 = (double)dt, dx64 = (double)p.dx;

	// the copy cases in the contract's order, as a flag; the cell's own raw depth is needed whatever the verdict (its neighbours read c)
	bool moves = inside && !(x <= 0 || y <= 0 || x >= p.cols - 1 || y >= p.rows - 1 || dt <= T(0));
	double hC = 0.0;
	double FN = 0.0, FS = 0.0, FE = 0.0, FW = 0.0;
	[[maybe_unused]] double tau = 0.0;                                        // (EXCHANGE) the cell's bed shear stress ...
	[[maybe_unused]] bool exchanges = false;                                  // ... if it moves and is deep enough to have one
	if (inside && dt > T(0)) {
		const State4<T> c = src[id];
		const T zb = bed[id];
		hC = (double)c.z - (double)zb;
		if (c.zmax <= T(-9999.0) || c.z == T(-9999.0)) moves = false;
		if (moves) {
			const size_t iW = id - 1, iE = id + 1, iS = id - p.cols, iN = id + p.cols;
			const State4<T> cW = src[iW], cE = src[iE], cS = src[iS], cN = src[iN];
			const T zW = bed[iW], zE = bed[iE], zS = bed[iS], zN = bed[iN];
			if (c.z - zb < p.vs && cN.z - zN < p.vs && cE.z - zE < p.vs && cS.z - zS < p.vs && cW.z - zW < p.vs) moves = false;
			else {
				const Side<T> sC = make_side<true>(c.z, c.qx, c.qy, zb, p.vs);
				const Side<T> sN = make_side<true>(cN.z, cN.qx, cN.qy, zN, p.vs);
				const Side<T> sE = make_side<true>(cE.z, cE.qx, cE.qy, zE, p.vs);
				const Side<T> sS = make_side<true>(cS.z, cS.qx, cS.qy, zS, p.vs);
				const Side<T> sW = make_side<true>(cW.z, cW.qx, cW.qy, zW, p.vs);
				FN = (double)face_solve<AXIS_Y, true, true, false>(sC, sN, p.vs).forL.f0;
				FS = (double)face_solve<AXIS_Y, true, false, true>(sS, sC, p.vs).forR.f0;
				FE = (double)face_solve<AXIS_X, true, true, false>(sC, sE, p.vs).forL.f0;
				FW = (double)face_solve<AXIS_X, true, false, true>(sW, sC, p.vs).forR.f0;
				if constexpr (EXCHANGE)
					if (X.exchanging && hC > TRACER_DEPTH_MIN) {
						exchanges = true;
						tau = tracer_shear(hC, (double)c.qx, (double)c.qy, (double)(p.manning_uniform ? p.manning_value : X.manning[id]));
					}
			}
		}
	}
	if (!__syncthreads_or(moves ? 1 : 0)) {                                    // (block-uniform) nothing moves here: copy, then decay
		if (inside)
			for (unsigned s = 0; s < species; ++s) M1[s * plane + id] = tracer_decay(M0[s * plane + id], rates.lambda[s], dt64);
		return;
	}

	// this lane's halo cell, if it has one: waves 0 and 1 share the 2 x 64 + 2 x 4 cells of the tile's rim (corners are never read)
	const int lane = ty * 64 + tx;
	int hr = -1, hc = 0;                                                      // its place in the tile
	if (lane < 64) { hr = 0; hc = lane + 1; }                                 // the row below the block
	else if (lane < 128) { hr = TRACER_SET_ROWS + 1; hc = lane - 64 + 1; }    // the row above
	else if (lane < 128 + TRACER_SET_ROWS) { hr = lane - 128 + 1; hc = 0; }   // the column to the west
	else if (lane < 128 + 2 * TRACER_SET_ROWS) { hr = lane - 128 - TRACER_SET_ROWS + 1; hc = TRACER_SET_PITCH - 1; }   // to the east
	const long hx = x0 + hc - 1, hy = y0 + hr - 1;
	const bool halo = hr >= 0 && hx >= 0 && hy >= 0 && hx < p.cols && hy < p.rows;
	const size_t hid = halo ? (size_t)hy * p.cols + hx : 0;
	double hH = 0.0;
	if (halo) hH = (double)src[hid].z - (double)bed[hid];

	for (unsigned s = 0; s < species; ++s) {
		const double* __restrict__ m0 = M0 + s * plane;
		double (*t)[TRACER_SET_PITCH] = tile[s & 1];
		const double m = inside ? m0[id] : 0.0;
		t[ty + 1][tx + 1] = inside ? tracer_conc(m, hC) : 0.0;
		if (hr >= 0) t[hr][hc] = halo ? tracer_conc(m0[hid], hH) : 0.0;
		__syncthreads();
		if (inside) {
			double next = m;
			if (moves)
				next = tracer_update(m, t[ty + 1][tx + 1], t[ty + 2][tx + 1], t[ty][tx + 1], t[ty + 1][tx + 2], t[ty + 1][tx],
				                     FN, FS, FE, FW, dt64, dx64);
			next = tracer_decay(next, rates.lambda[s], dt64);
			if constexpr (EXCHANGE)
				if ((X.exchanging >> s & 1u) && exchanges) {
					double* __restrict__ at = X.D + s * plane + id;
					const double d0 = *at;
					const TracerPair after = tracer_exchange_at(next, d0, tau, hC, dt64, X.of[s]);
					if (after.D != d0) *at = after.D;
					next = after.M;
				}
			M1[s * plane + id] = next;
		}
	}
}

} // namespace hp
#endif // __HIPCC__
