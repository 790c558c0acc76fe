// hp_engine.hip -- host side of libhipims_mi.so: the C ABI of include/hipims_mi.h over the HIP kernels.  Here: the domain's life,
// uploads and downloads, checkpoints, and stepping -- tile launches, iteration pairs and their tuner, speculative batches, strips over
// RCCL and the peer mailboxes.  What reads the state (the observers) and what changes it from outside the flux kernels (the actors:
// boundaries, link groups, bed shapes) live in hp_observers.hpp and hp_actors.hpp.
//
// Mirrors what the reference's CSchemeGodunov / CSchemeMUSCLHancock do against COCLDevice/COCLBuffer/COCLKernel
// (buffers: CSchemeGodunov.cpp:789-892; iteration graph: :1617-1666) -- one HIP stream per domain stands in for
// the reference's per-device command queue, stream order for its explicit queueBarrier() calls.
#include "hp_domain.hpp"        // fail / HIP_TRY, struct hp_domain, the map of its pinned block
#include "hp_observers.hpp"     // output stage, peak tracker, probe recorder: their entry points and what a checkpoint does for them
#include "hp_actors.hpp"        // boundaries, link groups, bed shapes: their entry points, the boundary pass, what a checkpoint does for them
#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include <unistd.h>

namespace {

constexpr size_t CFL_SLOT_BYTES = 1024;        // hp_math.hpp: SLOT_* elements, each on its own 256-B line

// RCCL entry points, resolved by hp_comm_load
struct Rccl {
	void* handle = nullptr;
	decltype(&ncclGetUniqueId)   GetUniqueId = nullptr;
	decltype(&ncclCommInitRank)  CommInitRank = nullptr;
	decltype(&ncclCommDestroy)   CommDestroy = nullptr;
	decltype(&ncclGroupStart)    GroupStart = nullptr;
	decltype(&ncclGroupEnd)      GroupEnd = nullptr;
	decltype(&ncclSend)          Send = nullptr;
	decltype(&ncclRecv)          Recv = nullptr;
	decltype(&ncclAllReduce)     AllReduce = nullptr;
	decltype(&ncclGetErrorString) GetErrorString = nullptr;
	decltype(&ncclCommCount)     CommCount = nullptr;        // optional (reporting only)
	std::string path;                                        // what the dynamic loader resolved the library to
} g_rccl;

void peer_release(hp_domain* d);      // (mailboxes of the peer-written maximum, further down)
PeerBox peer_box(hp_domain* d, bool use, long timeout_ms = 0);
PeerPush make_push(const hp_domain* d);

// The rules' switches (hp_plan.hpp) from the environment: the only place that names these variables, read once per process, at the
// first call.  (HP_MARCH2_RSEG's value is a tiling knob, below; here only whether it is set at all.)
const PlanKnobs& plan_knobs()
{
	static const PlanKnobs knobs = [] {
		auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
		auto off = [&](const char* name) { return num(name, 1) == 0; };          // NAME=0 switches off
		auto on = [&](const char* name) { return num(name, 0) != 0; };           // NAME=1 (any non-zero) switches on
		auto force = [&](const char* name) { return std::getenv(name) ? (num(name, 0) != 0 ? 1 : 0) : -1; };
		PlanKnobs k;
		k.two_step = num("HP_TWO_STEP", -1);
		k.launch_tail = !off("HP_LAUNCH_TAIL"); k.strip_reduce_always = on("HP_STRIP_REDUCE_ALWAYS");
		k.pair_bdy = !off("HP_PAIR_BDY"); k.pair_strict = !off("HP_PAIR_STRICT"); k.pair_exact = force("HP_PAIR_EXACT");
		k.pair_skip = !off("HP_PAIR_SKIP"); k.pair_wall = !off("HP_PAIR_WALL"); k.fill_after_pairs = !off("HP_FILL_AFTER_PAIRS");
		k.strict_speculate = on("HP_STRICT_SPECULATE"); k.pair_tune = !off("HP_PAIR_TUNE"); k.sweep_alternate = force("HP_SWEEP_ALTERNATE");
		k.tail_max_blocks = (unsigned)num("HP_TAIL_MAX_BLOCKS", (int)TAIL_MAX_BLOCKS);
		k.tail_max_blocks_k2k6 = (unsigned)num("HP_TAIL_MAX_BLOCKS_K2K6", (int)TAIL_MAX_BLOCKS);
		k.march2_rseg_forced = std::getenv("HP_MARCH2_RSEG") != nullptr;
		k.fuse_bdy = !off("HP_FUSE_BDY");
		return k;
	}();
	return knobs;
}
// What the rules read from the domain, as it is now: scalar copies and one walk over the boundary list.  Taken where a rule is
// evaluated -- nothing is kept, so nothing can go stale.
PlanDomain plan_domain(const hp_domain* d)
{
	PlanDomain p;
	p.scheme = d->desc.scheme; p.kernel = d->desc.kernel; p.math_mode = d->desc.math_mode; p.precision = d->desc.precision; p.dynamic_dt = d->desc.dynamic_dt;
	p.quirks = d->desc.quirks; p.rows = d->desc.rows; p.cols = d->desc.cols; p.cells = d->cells;
	p.row_offset = d->desc.row_offset; p.global_rows = d->desc.global_rows; p.ghost_rows = d->ghost_rows;
	p.has_bdy = !d->bdy.empty(); p.fusable = d->fusable; p.bdy_on_ring = d->bdy_on_ring;
	for (const Boundary& b : d->bdy)
		if ((b.kind == BDY_UNIFORM && b.definition == HP_UNIFORM_LOSS_RATE) || (b.kind == BDY_GRIDDED && b.definition == HP_GRIDDED_MASS_FLUX)) p.bdy_removes_water = true;
	p.has_comm = d->comm != nullptr; p.comm_world = d->comm_world; p.peer_direct = d->peer_direct; p.peer_mine = d->peer_mine != nullptr;
	p.has_tail_words = d->tail_words != nullptr; p.tail_allowed = d->tail_allowed; p.halo_overlap = d->halo_overlap; p.split_now = d->split_now;
	p.strip_any_bdy = d->strip_any_bdy; p.strip_first = d->strip_first; p.strip_any_full = d->strip_any_full;
	p.spec_now = d->spec_now; p.has_stamps = d->z_state != nullptr; p.march2_pays = d->tiling.march2_pays;
	p.has_links = d->links.groups != 0; p.soil_on = d->soil.on; p.tracer_on = d->tracer.on; p.open_on = d->open.segments != 0;
#ifdef HP_KEEP_SPEC_FUSED
	p.spec_fused_kept = true;                                             // (launch_march: the instantiation kept buildable for study)
#endif
	return p;
}

template <typename T> Params<T> make_params(const hp_domain* d)
{
	Params<T> p;
	p.cols = d->desc.cols; p.rows = d->desc.rows;
	p.row_offset = d->desc.row_offset; p.global_rows = d->desc.global_rows;
	p.dx = (T)d->desc.dx;
	p.inv_dx = T(1) / p.dx;
	p.vs = (T)d->desc.dry_threshold;
	p.qs = (T)d->desc.dry_threshold * T(10);             // CSchemeGodunov.cpp:57, :523
	p.courant = (T)d->desc.courant;
	p.t_end = (T)d->desc.t_end;
	p.dt_fixed = (T)d->desc.dt_fixed;
	p.friction = d->desc.friction;
	p.dynamic_dt = d->desc.dynamic_dt;
	p.manning_uniform = d->manning_uniform ? 1 : 0;
	p.manning_value = (T)d->manning_value;
	p.simplified_cfl = d->desc.scheme == HP_SCHEME_INERTIAL ? 1 : 0;       // CLSchemeInertial.clh:25
	p.muscl_nb_bed = (d->desc.quirks & HP_QUIRK_MUSCL_NEIGHBOUR_Y_IS_BED) ? 1 : 0;
	{
		// dx a power of two (in T's arithmetic): STRICT's divisions by dx become multiplications by the exact 1 / dx
		int e = 0;
		const double m = std::frexp((double)(T)d->desc.dx, &e);
		static const bool off = std::getenv("HP_STRICT_DX_POW2") && std::atoi(std::getenv("HP_STRICT_DX_POW2")) == 0;
		p.inv_dx_pow2 = (m == 0.5 && !off && e > -100 && e < 100) ? (T)(1.0 / (double)(T)d->desc.dx) : T(0);
	}
	return p;
}

inline dim3 grid2d(long cols, long rows, dim3 block)
{
	return dim3((unsigned)((cols + block.x - 1) / block.x), (unsigned)((rows + block.y - 1) / block.y));
}

template <typename T> int launch_reduce(hp_domain* d, const void* state, long row_lo, long row_hi)
{
	const Params<T> p = make_params<T>(d);
	const size_t n = (size_t)(row_hi - row_lo) * p.cols;
	unsigned blocks = (unsigned)((n + 256 * 8 - 1) / (256 * 8));
	if (blocks > 2048) blocks = 2048;
	if (blocks < 1) blocks = 1;
	// in the domain's own arithmetic: the same buffer prices to the same bits here and in the flux kernels' fused epilogue
	if (d->desc.math_mode == HP_MATH_STRICT)
		hipLaunchKernelGGL((cfl_reduce<true, T>), dim3(blocks), dim3(256), 0, d->stream, p, (const State4<T>*)state,
		                   (const T*)d->bed, row_lo, row_hi, (T*)d->cfl_slot);
	else
		hipLaunchKernelGGL((cfl_reduce<false, T>), dim3(blocks), dim3(256), 0, d->stream, p, (const State4<T>*)state,
		                   (const T*)d->bed, row_lo, row_hi, (T*)d->cfl_slot);
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

template <typename T> int price_edge_ring(hp_domain* d)
{
	const Params<T> p = make_params<T>(d);
	HIP_TRY(hipMemsetAsync((T*)d->cfl_slot + SLOT_EDGE, 0, 2 * sizeof(T), d->stream));
	const int w = (int)stencil_reach(d->desc);
	const bool at_south = d->desc.row_offset == 0;
	const bool at_north = d->desc.row_offset + d->desc.rows == d->desc.global_rows;
	const long south = at_south ? 0 : -1;
	const long north = at_north ? d->desc.rows - w : -1;
	// side columns of the owned rows, minus the rows already covered by south/north
	const long lo = d->own_lo + (at_south ? w : 0), hi = d->own_hi - (at_north ? w : 0);
	for (int b = 0; b < 2; ++b) {
		if (d->desc.math_mode == HP_MATH_STRICT)
			hipLaunchKernelGGL((cfl_edge_ring<true, T>), dim3(64), dim3(256), 0, d->stream, p, (const State4<T>*)d->state[b],
			                   (const T*)d->bed, lo, hi, south, north, w, (T*)d->cfl_slot + SLOT_EDGE + b);
		else
			hipLaunchKernelGGL((cfl_edge_ring<false, T>), dim3(64), dim3(256), 0, d->stream, p, (const State4<T>*)d->state[b],
			                   (const T*)d->bed, lo, hi, south, north, w, (T*)d->cfl_slot + SLOT_EDGE + b);
	}
	HIP_TRY(hipGetLastError());
	d->facts.edge_ring_priced();
	return HP_OK;
}

// The tiling knobs (hp_tiling.hpp) from the environment: these two readers are the only place that names the variables.  Each is
// read when it always was: at hp_domain_create HP_RSEG_REFINE and the pair kernel's look at HP_TILING_SEARCH once per process,
// the others per domain (tools/strong_probe_pair.py creates domains with the K1 / K6 search on and off); once per process, at the
// first launch, what make_tile_map takes.
TilingKnobs tiling_knobs()
{
	auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
	auto has = [](const char* name) { return std::getenv(name) != nullptr; };
	static const bool refine = num("HP_RSEG_REFINE", 1) != 0, search_pair = num("HP_TILING_SEARCH", 1) != 0;
	TilingKnobs k;
	k.rseg_refine = refine; k.search_pair = search_pair; k.search = num("HP_TILING_SEARCH", 1) != 0;
	k.search_f32 = has("HP_TILING_SEARCH_F32"); k.print_tiling = has("HP_PRINT_TILING");
	if (const char* e = std::getenv("HP_TILING_FILL")) k.tiling_fill = std::atof(e);
	if (const char* e = std::getenv("HP_MARCH2_FILL")) k.march2_fill = std::atof(e);
	k.march_rseg = num("HP_MARCH_RSEG", 0); k.muscl_rseg = num("HP_MUSCL_RSEG", 0);
	k.inertial_rseg = num("HP_INERTIAL_RSEG", 0); k.march2_rseg = num("HP_MARCH2_RSEG", 0);
	k.tail_rseg = num("HP_TAIL_RSEG", 0); k.tail_pct = num("HP_TAIL_PCT", -1);
	return k;
}
const LaunchKnobs& launch_knobs()
{
	static const LaunchKnobs k = {std::getenv("HP_HALO_ROWS") ? std::atol(std::getenv("HP_HALO_ROWS")) : 0,
	                              std::getenv("HP_NBANDS") ? std::atoi(std::getenv("HP_NBANDS")) : 0};
	return k;
}
// HP_PAIR_ORDER=0: the pair kernel's record launches raise no flags and read no table -- blocks take their tiles tile-row by tile-row
// (A/B runs; hp_order.hpp).  Once per process, like the switches above.
static bool pair_order_on()
{
	static const bool on = !(std::getenv("HP_PAIR_ORDER") && std::atoi(std::getenv("HP_PAIR_ORDER")) == 0);
	return on;
}

// Rows one flux launch updates: everything between the never-written edge ring / the outermost ghost rows.  A strip with
// two reaches of ghost rows (ghost_rows = 2g) also updates, on the iteration that follows an exchange, the g ghost rows
// next to its owned rows -- redundantly with their owner, from the same values, to the same bits -- and on the next
// iteration, which finds only those still valid, its owned rows alone.
inline void launch_rows(const hp_domain* d, long g, long& lo, long& hi)
{
	const bool south = d->desc.row_offset > 0, north = d->desc.row_offset + d->desc.rows < d->desc.global_rows;
	const long keep = d->ghost_rows - (d->facts->ghost_valid - g);      // ghost rows at each interior side NOT updated now
	lo = south ? keep : g;
	hi = d->desc.rows - (north ? keep : g);
}

// The launch's own tail block (LaunchTail, hp_kernels.hpp), and with it the rows that leave with this iteration: the tiles that
// compute the strip's first / last `ghost_rows` owned rows store them into the neighbours as well -- the neighbour's pointer
// is shifted so that this strip's cell index lands on the neighbour's copy of the cell.  `limit`: launches of more blocks keep
// the advance launch.  Returns 0 (no tail), 1 (tail block) or 2 (tail block + rows stored into the neighbours).
// how long a launch's tail block waits for ONE flux block's word before it raises SLOT_TAIL_ERR (hp_kernels.hpp: launch_tail).
// Generous: the wait only starts once the tail block runs, i.e. once its XCD has dispatched every flux block of the launch.
static long tail_timeout_ms()
{
	static const long ms = std::getenv("HP_TAIL_TIMEOUT_MS") ? std::atol(std::getenv("HP_TAIL_TIMEOUT_MS")) : 20000;
	return ms > 0 ? ms : 20000;
}
// (tests) the tail block also waits for one word that no block writes: the time-out must fire, the call sequence must fail
static unsigned tail_debug_extra_word()
{
	static const unsigned v = std::getenv("HP_DEBUG_TAIL_EXTRA_WORD") && std::atoi(std::getenv("HP_DEBUG_TAIL_EXTRA_WORD")) != 0 ? 1u : 0u;
	return v;
}
template <typename T> int make_tail(hp_domain* d, unsigned& blocks, int part, hipStream_t stream, unsigned limit, LaunchTail<T>& tail)
{
	tail = LaunchTail<T>{};
	if (part == PART_ALL) d->flux_launches++;
	const int kind = tail_kind_for(d->tail_want, part == PART_ALL, stream == d->stream, blocks, limit, d->push_now);
	if (kind == 0) return 0;
	tail.done = d->tail_words;
	tail.done1 = d->tail_words + TAIL_MAX_BLOCKS + 8;
	tail.bdy_flag = 0;
	tail.flux_blocks = blocks;
	tail.poll_blocks = blocks + tail_debug_extra_word();
	tail.timeout = (unsigned long long)tail_timeout_ms() * 100000ull;       // wall_clock64: 100 MHz
	tail.fresh = d->tail_fresh;
	tail.sc = (Scalars<T>*)d->scalars;
	tail.slot = (T*)d->cfl_slot;
	tail.box = peer_box(d, (d->tail_fresh & 4) != 0);
	tail.edge_rows[0] = tail.edge_rows[1] = tail.edge_rows[2] = tail.edge_rows[3] = 0;
	tail.peer_rows[0] = tail.peer_rows[1] = nullptr;
	if (kind == 2) {
		const long G = d->ghost_rows, rows = d->desc.rows, cols = d->desc.cols;
		const int b = d->facts->use_alt ^ 1;
		if (d->peer_state[0][b]) {
			tail.peer_rows[0] = (State4<T>*)d->peer_state[0][b] + (d->peer_rows[0] - 2 * G) * cols;     // my row G -> its row rows_s - G
			tail.edge_rows[0] = (int)G; tail.edge_rows[1] = (int)(2 * G);
		}
		if (d->peer_state[1][b]) {
			tail.peer_rows[1] = (State4<T>*)d->peer_state[1][b] - (rows - 2 * G) * cols;                // my row rows - 2G -> its row 0
			tail.edge_rows[2] = (int)(rows - 2 * G); tail.edge_rows[3] = (int)(rows - G);
		}
	}
	blocks += 1;
	d->tail_done = true;
	d->flux_launches_tailed++;
	return kind;
}

// Alternating sweep direction (hp_plan.hpp: sweep_alternates): every other whole-domain launch visits each band's tiles from the top down.
inline void sweep_direction(hp_domain* d, const int part, TileMap& tm)
{
	if (part != PART_ALL || !sweep_alternates(plan_domain(d), plan_knobs())) return;
	tm.flip = d->sweep_flip;
	d->sweep_flip ^= 1;
}

template <typename T, bool STRICT, int CFL_MODE>
int launch_muscl(hp_domain* d, const void* src, void* dst, int edge_buffer, int part, hipStream_t stream)
{
	const Params<T> p = make_params<T>(d);
	TileMap tm;
	unsigned blocks;
	long lo, hi;
	launch_rows(d, 2, lo, hi);
	const Tiling& t = d->tiling;
	if (!make_tile_map(launch_knobs(), lo, hi, 2, part, (int)((p.cols - 4 + MUSCL_COLS - 1) / MUSCL_COLS), t.muscl_rseg, t.tail_rseg < 8 ? 8 : t.tail_rseg, t.tail_pct, tm, blocks,
	                   16, d->ghost_rows, d->own_lo, d->own_hi, t.muscl_nbands))
		return HP_OK;
	sweep_direction(d, part, tm);
	LaunchTail<T> tail;
	const int tail_kind = make_tail<T>(d, blocks, part, stream, tail_limit_k2k6(plan_knobs()), tail);
#define HP_LAUNCH_K2S(UNIFORM_, TAIL_, SPEC_)                                                                                        \
	hipLaunchKernelGGL((muscl_march<STRICT, CFL_MODE, UNIFORM_, TAIL_, T, SPEC_>), dim3(blocks), dim3(256), 0, stream, p,            \
	                   (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst,                     \
	                   (const T*)d->manning, (T*)d->cfl_slot, (const T*)d->cfl_slot + SLOT_EDGE + edge_buffer, tm, tail)
#define HP_LAUNCH_K2(UNIFORM_, TAIL_) HP_LAUNCH_K2S(UNIFORM_, TAIL_, false)
	// a speculative STRICT fp64 batch (spec_begin): the shared-reciprocal instantiation; single domains only (TAIL 0 / 1)
	constexpr bool CAN_SPEC = STRICT && sizeof(T) == 8;
	if (CAN_SPEC && d->spec_now && tail_kind != 2 && part == PART_ALL) {
		if (d->manning_uniform) { if (tail_kind == 1) HP_LAUNCH_K2S(true, 1, CAN_SPEC); else HP_LAUNCH_K2S(true, 0, CAN_SPEC); }
		else                    { if (tail_kind == 1) HP_LAUNCH_K2S(false, 1, CAN_SPEC); else HP_LAUNCH_K2S(false, 0, CAN_SPEC); }
	} else
	if (d->manning_uniform) { if (tail_kind == 2) HP_LAUNCH_K2(true, 2); else if (tail_kind == 1) HP_LAUNCH_K2(true, 1); else HP_LAUNCH_K2(true, 0); }
	else                    { if (tail_kind == 2) HP_LAUNCH_K2(false, 2); else if (tail_kind == 1) HP_LAUNCH_K2(false, 1); else HP_LAUNCH_K2(false, 0); }
#undef HP_LAUNCH_K2
#undef HP_LAUNCH_K2S
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

template <typename T, bool STRICT, int CFL_MODE>
int launch_march(hp_domain* d, const void* src, void* dst, int edge_buffer, int part, hipStream_t stream)
{
	const Params<T> p = make_params<T>(d);
	TileMap tm;
	unsigned blocks;
	long lo, hi;
	launch_rows(d, 1, lo, hi);
	const Tiling& t = d->tiling;
	if (!make_tile_map(launch_knobs(), lo, hi, 1, part, (int)((p.cols - 2 + MARCH_COLS - 1) / MARCH_COLS), part == PART_ALL ? t.march_rseg : t.march_rseg_parts, t.tail_rseg, t.tail_pct, tm, blocks, t.tall_rseg,
	                   d->ghost_rows, d->own_lo, d->own_hi, t.march_nbands))
		return HP_OK;
	sweep_direction(d, part, tm);
	const int truncated = ((d->desc.quirks & HP_QUIRK_BDY_TRUNCATED) != 0 ? 1 : 0) | (d->fill_now ? 2 : 0);   // the kernel's `flags`

	LaunchTail<T> tail;
	const int tail_kind = make_tail<T>(d, blocks, part, stream, tail_limit(plan_knobs()), tail);
#define HP_LAUNCH_K1S(FUSED_, TAIL_, LIST_, NEXT_, SPEC_)                                                                                   \
	hipLaunchKernelGGL((godunov_march<STRICT, CFL_MODE, FUSED_, TAIL_, T, SPEC_>), dim3(blocks), dim3(256), 0, stream, p,                   \
	                   (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst,                     \
	                   (const T*)d->manning, (T*)d->cfl_slot, (const T*)d->cfl_slot + SLOT_EDGE + edge_buffer, tm, LIST_, NEXT_,   \
	                   truncated, tail)
#define HP_LAUNCH_K1(FUSED_, TAIL_, LIST_, NEXT_) HP_LAUNCH_K1S(FUSED_, TAIL_, LIST_, NEXT_, false)
	constexpr bool CAN_SPEC = STRICT && sizeof(T) == 8;       // a speculative STRICT fp64 batch: see launch_muscl
	if (CAN_SPEC && d->spec_now && !d->fusable && tail_kind != 2 && part == PART_ALL) {        // (never with fused boundaries: spec_wanted)
		if (tail_kind == 1) HP_LAUNCH_K1S(false, 1, (const AreaBdyList<T>*)nullptr, 0, CAN_SPEC);
		else                HP_LAUNCH_K1S(false, 0, (const AreaBdyList<T>*)nullptr, 0, CAN_SPEC);
	} else
#ifdef HP_KEEP_SPEC_FUSED
	// (the instantiation round 5 deleted -- the speculative flavour with FUSED boundaries, LAB_NOTES R5.13 -- kept buildable for the
	// study of what went wrong with it: a library built with -DHP_KEEP_SPEC_FUSED speculates on such domains too)
	if (CAN_SPEC && d->spec_now && d->fusable && tail_kind != 2 && part == PART_ALL) {
		if (tail_kind == 1) HP_LAUNCH_K1S(true, 1, (const AreaBdyList<T>*)d->fused_list, d->fuse_next, CAN_SPEC);
		else                HP_LAUNCH_K1S(true, 0, (const AreaBdyList<T>*)d->fused_list, d->fuse_next, CAN_SPEC);
	} else
#endif
	if (d->fusable) {
		if (tail_kind == 2)      HP_LAUNCH_K1(true, 2, (const AreaBdyList<T>*)d->fused_list, d->fuse_next);
		else if (tail_kind == 1) HP_LAUNCH_K1(true, 1, (const AreaBdyList<T>*)d->fused_list, d->fuse_next);
		else                     HP_LAUNCH_K1(true, 0, (const AreaBdyList<T>*)d->fused_list, d->fuse_next);
	} else {
		if (tail_kind == 2)      HP_LAUNCH_K1(false, 2, (const AreaBdyList<T>*)nullptr, 0);
		else if (tail_kind == 1) HP_LAUNCH_K1(false, 1, (const AreaBdyList<T>*)nullptr, 0);
		else                     HP_LAUNCH_K1(false, 0, (const AreaBdyList<T>*)nullptr, 0);
	}
#undef HP_LAUNCH_K1S
#undef HP_LAUNCH_K1
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

template <typename T, bool STRICT, int CFL_MODE>
int launch_inertial(hp_domain* d, const void* src, void* dst, int edge_buffer, int part, hipStream_t stream)
{
	const Params<T> p = make_params<T>(d);
	TileMap tm;
	unsigned blocks;
	long lo, hi;
	launch_rows(d, 1, lo, hi);
	const Tiling& t = d->tiling;
	if (!make_tile_map(launch_knobs(), lo, hi, 1, part, (int)((p.cols - 2 + MARCH_COLS - 1) / MARCH_COLS), part == PART_ALL ? t.inertial_rseg : t.inertial_rseg_parts, t.tail_rseg, t.tail_pct, tm, blocks, t.tall_rseg,
	                   d->ghost_rows, d->own_lo, d->own_hi, t.inertial_nbands))
		return HP_OK;
	sweep_direction(d, part, tm);
	LaunchTail<T> tail;
	const int tail_kind = make_tail<T>(d, blocks, part, stream, tail_limit_k2k6(plan_knobs()), tail);
#define HP_LAUNCH_K6(TAIL_)                                                                                                         \
	hipLaunchKernelGGL((inertial_march<STRICT, CFL_MODE, TAIL_, T>), dim3(blocks), dim3(256), 0, stream, p,                          \
	                   (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst,                     \
	                   (const T*)d->manning, (T*)d->cfl_slot, (const T*)d->cfl_slot + SLOT_EDGE + edge_buffer, tm, tail)
	if (tail_kind == 2) HP_LAUNCH_K6(2); else if (tail_kind == 1) HP_LAUNCH_K6(1); else HP_LAUNCH_K6(0);
#undef HP_LAUNCH_K6
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

template <typename T, bool STRICT>
int launch_flux(hp_domain* d, const void* src, void* dst, const SinglePlan& plan, int part, hipStream_t stream)
{
	const Params<T> p = make_params<T>(d);
	const int cfl_mode = plan.cfl_mode, ring = plan.edge_buffer;          // (ring of the buffer that is priced: plan_single)
	if (d->desc.scheme == HP_SCHEME_MUSCL_HANCOCK) {
		if (p.cols < 5 || p.rows < 5) return fail(HP_ERR_INVALID, "MUSCL-Hancock needs at least a 5x5 grid");
		return cfl_mode ? launch_muscl<T, STRICT, 1>(d, src, dst, ring, part, stream)
		                : launch_muscl<T, STRICT, 0>(d, src, dst, ring, part, stream);
	}
	if (d->desc.scheme == HP_SCHEME_INERTIAL) {
		if (p.cols < 3 || p.rows < 3) return fail(HP_ERR_INVALID, "the inertial scheme needs at least a 3x3 grid");
		switch (cfl_mode) {
		case 1:  return launch_inertial<T, STRICT, 1>(d, src, dst, ring, part, stream);
		case 2:  return launch_inertial<T, STRICT, 2>(d, src, dst, ring, part, stream);
		default: return launch_inertial<T, STRICT, 0>(d, src, dst, ring, part, stream);
		}
	}
	if (d->desc.kernel == HP_KERNEL_BASIC) {
		if (part == PART_INTERIOR) return HP_OK;                          // no split for the cross-check kernel
		long lo, hi;
		launch_rows(d, 1, lo, hi);
		const dim3 block(64, 4), grid = grid2d(p.cols, hi - lo, block);
		hipLaunchKernelGGL((godunov_basic<STRICT, T>), grid, block, 0, stream, p, (const Scalars<T>*)d->scalars,
		                   (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst, (const T*)d->manning, lo, hi);
		HIP_TRY(hipGetLastError());
		return HP_OK;
	}
	switch (cfl_mode) {
	case 1:  return launch_march<T, STRICT, 1>(d, src, dst, ring, part, stream);
	case 2:  return launch_march<T, STRICT, 2>(d, src, dst, ring, part, stream);
	default: return launch_march<T, STRICT, 0>(d, src, dst, ring, part, stream);
	}
}

// boundaries -> flux -> local CFL maximum   (CSchemeGodunov.cpp:1637-1657)
template <typename T, bool STRICT> int step_begin_impl(hp_domain* d)
{
	void* src = d->state[d->facts->use_alt];
	void* dst = d->state[d->facts->use_alt ^ 1];
	int rc;
	const PlanDomain pd = plan_domain(d);
	if (boundaries_applied(pd)) {
		d->fork_is_advance = false;
		if ((rc = apply_boundaries<T>(d, src)) != HP_OK) return rc;
	}
	// the tracer: behind every boundary, on the buffer the flux launch is about to read and the timestep its tail block is about to advance
	if (pd.tracer_on) {
		d->fork_is_advance = false;
		if ((rc = apply_tracer<T>(d, src)) != HP_OK) return rc;
	}
	// what the launch prices, whether it carries its own tail block, what follows it (hp_plan.hpp)
	const SinglePlan plan = plan_single(pd, d->facts, plan_knobs());
	if (plan.reprice_ring) { d->fork_is_advance = false; if ((rc = price_edge_ring<T>(d)) != HP_OK) return rc; }

	// flux-kernel timing: every `stride`-th launch is bracketed by a pair of events taken from a pool created by
	// hp_kernel_timing (nothing is created inside a timed region; once the pool is used up sampling stops)
	// (a domain whose batches are made of iteration pairs samples THOSE launches -- run_pair -- not the odd single iteration at a
	// batch's ends: hp_kernel_timing reports one kernel's average, the dominant one's)
	// (... while pairs really run: a domain that COULD pair but does not -- batches of one iteration, a launch too big for the tail
	// block, a maximum that stays stale -- is seen by its run of single iterations and samples them)
	d->single_streak++;
	const bool sample = d->timing_stride > 0 && d->timing_used < d->timing_events.size() && (!pairs_possible(pd, plan_knobs()) || d->single_streak > 3) &&
	                    (d->timing_counter++ % (uint64_t)d->timing_stride) == 0;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	if (sample) {
		e0 = d->timing_events[d->timing_used].first;
		e1 = d->timing_events[d->timing_used].second;
		HIP_TRY(hipEventRecord(e0, d->stream));
	}
	d->tail_want = plan.tail_want;
	d->tail_fresh = plan.tail_fresh;
	d->tail_done = false;
	if (d->halo_overlap && d->split_now) {
		// fork: everything queued so far (previous advance, boundaries, ring pricing) happens-before the halo
		// segments; they run on their own stream, next to the interior segments on the domain's stream
		// (when nothing was queued since the previous advance_time, that kernel's own completion event serves:
		// a separate marker packet in front of the interior launch costs a few microseconds on the critical path)
		if (!d->fork_is_advance) HIP_TRY(hipEventRecord(d->ev_fork, d->stream));
		d->fork_is_advance = false;
		HIP_TRY(hipStreamWaitEvent(d->stream_halo, d->ev_fork, 0));
		if ((rc = launch_flux<T, STRICT>(d, src, dst, plan, PART_HALO, d->stream_halo)) != HP_OK) return rc;
		HIP_TRY(hipEventRecord(d->ev_halo, d->stream_halo));
		if ((rc = launch_flux<T, STRICT>(d, src, dst, plan, PART_INTERIOR, d->stream)) != HP_OK) return rc;
		// join: the CFL maximum (and anything after it on the domain's stream) needs both launches
		HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_halo, 0));
	} else if ((rc = launch_flux<T, STRICT>(d, src, dst, plan, PART_ALL, d->stream)) != HP_OK) return rc;
	d->tail_want = false;
	if (sample) {
		HIP_TRY(hipEventRecord(e1, d->stream));
		d->timing_used++;
	}

	d->adv_fresh = 0;
	if (d->desc.dynamic_dt) {
		if (plan.cfl_mode != 0) {
			d->adv_fresh = 1;
			d->facts.maximum_priced();
		} else if (plan.reduce_after) {
			const void* reduce_buf = plan.reduce_buffer_is_primary ? d->state[0] : dst;
			if ((rc = launch_reduce<T>(d, reduce_buf, d->own_lo, d->own_hi)) != HP_OK) return rc;
			d->adv_fresh = 1;
			d->facts.maximum_priced();
		}
	}
	return HP_OK;
}

// the ghost rows an advance kernel (or a launch's tail block) carries to the strip neighbours: the first / last `ghost_rows`
// owned rows of the state this iteration wrote go into the neighbours' ghost rows of the same ping-pong buffer
PeerPush make_push(const hp_domain* d)
{
	const long G = d->ghost_rows, rows = d->desc.rows;
	const size_t row_bytes = (size_t)d->desc.cols * 4 * d->esize;
	const int b = d->facts->use_alt ^ 1;
	const char* mine = (const char*)d->state[b];
	PeerPush push{};
	push.count = (unsigned)((size_t)G * row_bytes / 16);
	push.arrived = d->push_arrived;
	if (d->peer_state[0][b]) {
		push.from[0] = (const uint4*)(mine + (size_t)G * row_bytes);
		push.to[0] = (uint4*)((char*)d->peer_state[0][b] + (size_t)(d->peer_rows[0] - G) * row_bytes);
	}
	if (d->peer_state[1][b]) {
		push.from[1] = (const uint4*)(mine + (size_t)(rows - 2 * G) * row_bytes);
		push.to[1] = (uint4*)d->peer_state[1][b];
	}
	return push;
}

// kernel argument of a reduction through the mailboxes (one per reduction: its parity picks the mailbox set)
static long peer_timeout_ms()
{
	static const long ms = std::getenv("HP_PEER_TIMEOUT_MS") ? std::atol(std::getenv("HP_PEER_TIMEOUT_MS")) : 10000;
	return ms > 0 ? ms : 10000;
}
PeerBox peer_box(hp_domain* d, bool use, long timeout_ms)
{
	PeerBox box{};
	if (!use) return box;
	box.mine = d->peer_mine; box.peer = d->peer_table;
	box.world = d->peer_world; box.rank = d->peer_rank;
	box.set = (int)(d->peer_rounds++ & 1);
	box.timeout = (unsigned long long)(timeout_ms > 0 ? timeout_ms : peer_timeout_ms()) * 100000ull;   // wall_clock64: 100 MHz
	return box;
}

template <typename T> int step_end_impl(hp_domain* d)
{
	const Params<T> p = make_params<T>(d);
	const PeerBox box = d->tail_done ? PeerBox{} : peer_box(d, (d->adv_fresh & 4) != 0);   // (the tail block took its own: one per round)
	if (d->tail_done) {
		// the flux launch's tail block has done it all (LaunchTail): nothing to launch
		d->tail_done = false;
		d->push_now = false;
		d->fork_is_advance = false;
	} else if (d->push_now) {
		// the ghost rows travel inside the advance kernel (PeerPush)
		const PeerPush push = make_push(d);
		static const unsigned per_block = std::getenv("HP_PUSH_PER_BLOCK") ? (unsigned)std::atoi(std::getenv("HP_PUSH_PER_BLOCK")) : 1024u;
		const unsigned blocks = (push.to[0] || push.to[1]) ? std::min(32u, (push.count + per_block - 1u) / per_block) : 1u;
		hipLaunchKernelGGL((advance_time<false, T>), dim3(blocks), dim3(256), 0, d->stream, p, (Scalars<T>*)d->scalars,
		                   (T*)d->cfl_slot, d->adv_fresh, box, push);
		d->push_now = false;
		d->fork_is_advance = false;
	} else if (d->halo_overlap && !d->peer_direct) {   // (also after an unsplit iteration: the NEXT one may be split and fork from here)
		hipExtLaunchKernelGGL((advance_time<false, T>), dim3(1), dim3(64), 0, d->stream, nullptr, d->ev_fork, 0, p,
		                      (Scalars<T>*)d->scalars, (T*)d->cfl_slot, d->adv_fresh, box, PeerPush{});
		d->fork_is_advance = true;                                        // cleared by anything else queued on the stream
	} else {
		hipLaunchKernelGGL((advance_time<false, T>), dim3(1), dim3(64), 0, d->stream, p, (Scalars<T>*)d->scalars,
		                   (T*)d->cfl_slot, d->adv_fresh, box, PeerPush{});
	}
	HIP_TRY(hipGetLastError());
	d->facts.single_ended();
	d->cells_calculated += (uint64_t)d->desc.cols * (uint64_t)d->desc.rows;   // :1299
	d->iterations += 1;
	return HP_OK;
}

// ---- two iterations per pass (hp_kernels.hpp: godunov_march2; which domains pair and when: hp_plan.hpp) ---------------------------------
// After partial uploads (rings_differ: the two buffers' edge rings MAY differ) the rings are compared once, the first time pairs are
// wanted: block-wise loads of a whole grid (hp_domain_upload_rows over all rows: how grids too big for one host array arrive) leave
// them equal to the zero-filled other buffer's wherever the ring is the usual closed wall (state 0), and such domains pair.  Blocks.
static int rings_really_differ(hp_domain* d)
{
	if (!d->facts->rings_differ || d->facts->rings_checked) return HP_OK;
	unsigned long long* word = (unsigned long long*)((char*)d->scalars + 192);     // (device scratch behind the Scalars block)
	HIP_TRY(hipMemsetAsync(word, 0, 8, d->stream));
	if (d->desc.precision == 8)
		hipLaunchKernelGGL((rings_compare<double>), dim3(32), dim3(256), 0, d->stream, (const State4<double>*)d->state[0],
		                   (const State4<double>*)d->state[1], (long)d->desc.cols, (long)d->desc.rows, word);
	else
		hipLaunchKernelGGL((rings_compare<float>), dim3(32), dim3(256), 0, d->stream, (const State4<float>*)d->state[0],
		                   (const State4<float>*)d->state[1], (long)d->desc.cols, (long)d->desc.rows, word);
	HIP_TRY(hipGetLastError());
	volatile unsigned long long* host = (volatile unsigned long long*)((char*)d->host_scalars + HOST_RINGS);
	*host = 1;
	HIP_TRY(hipMemcpyAsync((void*)host, word, 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	d->facts.rings_compared(*host == 0);
	return HP_OK;
}
// The stamps' buffers (PairAux), allocated with a domain's first exact pair.
static int pair_stamps_alloc(hp_domain* d)
{
	if (!pair_exact(plan_domain(d), plan_knobs()) || d->z_state) return HP_OK;
	const size_t rec = (size_t)4 * d->esize + 16;                         // stamp_rec<T>(): the state, then the launch's number
	HIP_TRY(hipMalloc(&d->z_state, d->cells * rec));
	HIP_TRY(hipMalloc((void**)&d->haz_words, 64));
	HIP_TRY(hipMemsetAsync(d->z_state, 0, d->cells * rec, d->stream));
	HIP_TRY(hipMemsetAsync(d->haz_words, 0, 64, d->stream));
	return HP_OK;
}
// Still records (hp_kernels.hpp: StillRec): a tile of a FAST fp64 pair launch whose stencil the launch before recorded as one still state,
// found as it was left, is skipped.  That holds only while nothing else writes either state buffer (or the bed) between the two launches:
// every such writer says so (hp_facts.hpp: buffers_written_outside), and so does every pair launch that does not write records itself
// (pair_launched).  HP_PAIR_SKIP=0: no records, nothing skipped (A/B runs; hp_plan.hpp: pair_records).
static int still_rec_alloc(hp_domain* d, const int windows)
{
	const size_t slots = (size_t)windows * (size_t)d->desc.rows;
	if (d->still_rec && d->still_rec_slots == slots) return HP_OK;
	hipFree(d->still_rec);
	d->still_rec = nullptr;
	d->facts.buffers_written_outside();
	const size_t bytes = (2 * slots + 1) * sizeof(StillRec);              // (+1: the counters of hp_pair_stats)
	HIP_TRY(hipMalloc(&d->still_rec, bytes));
	HIP_TRY(hipMemsetAsync(d->still_rec, 0xff, bytes, d->stream));       // the sentinel (rows no launch writes: the edge ring's)
	d->still_rec_slots = slots;
	return HP_OK;
}
// Block order of the same launches (hp_order.hpp; hp_kernels.hpp: OrderHook): the flags and the two table halves, sized for one tiling.
// Both halves start as the order without a hint, so a half is a permutation of every band's tiles whoever wrote it last -- also behind a
// tail block that gave up and built nothing.  Nothing about the state hangs on it: no fact of hp_facts.hpp is involved.
static int order_alloc(hp_domain* d, const TileMap& tm)
{
	const int shape[4] = {tm.nbands, tm.groups, tm.nbig, tm.ntail};
	if (d->order_buf && std::equal(shape, shape + 4, d->order_shape)) return HP_OK;
	hipFree(d->order_buf);
	d->order_buf = nullptr;
	d->order_written = d->order_read = false;
	const unsigned groups = (unsigned)tm.groups, nseg = (unsigned)(tm.nbig + tm.ntail), per_band = groups * nseg, table = (unsigned)tm.nbands * per_band;
	std::vector<unsigned> words((size_t)2 * table + (size_t)tm.nbands * groups + 1, 0u);
	for (unsigned i = 0; i < 2 * table; ++i) words[i] = order_entry(groups, nseg, 0ull, i % per_band);
	HIP_TRY(hipMalloc((void**)&d->order_buf, words.size() * sizeof(unsigned)));
	HIP_TRY(hipMemcpyAsync(d->order_buf, words.data(), words.size() * sizeof(unsigned), hipMemcpyHostToDevice, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));                            // (`words` leaves with this call; once per domain and tiling)
	std::copy(shape, shape + 4, d->order_shape);
	d->order_half = 0;
	return HP_OK;
}
// Area boundaries: the pair kernel needs the primary buffer priced WITH the first iteration's boundaries (slot[SLOT_M1]).  Every BDY
// pair leaves that figure for its successor; where there is no such predecessor -- the first pair after single iterations, an upload,
// a new target time -- the first half of iteration k is done the reference's own way: the stand-alone boundary pass on the primary
// buffer (it declines by itself if a fused store has applied them), the stand-alone reduction, and the result moved to SLOT_M1.
template <typename T> int pair_cold_start(hp_domain* d)
{
	int rc;
	d->facts.buffers_written_outside();
	if ((rc = apply_boundaries<T>(d, d->state[0])) != HP_OK) return rc;
	if ((rc = launch_reduce<T>(d, d->state[0], d->own_lo, d->own_hi)) != HP_OK) return rc;
	hipLaunchKernelGGL((pair_cold_start_words<T>), dim3(1), dim3(1), 0, d->stream, (T*)d->cfl_slot);
	HIP_TRY(hipGetLastError());
	d->facts.cold_started();
	d->pair_cold_starts++;
	return HP_OK;
}
template <typename T> int run_pair_t(hp_domain* d, const bool strip, const bool followed)
{
	const Params<T> p = make_params<T>(d);
	TileMap tm;
	unsigned blocks;
	long lo, hi;
	if (strip) {                                                          // the strip's OWNED rows: the pair consumes both reaches of ghost rows
		const bool south = d->desc.row_offset > 0, north = d->desc.row_offset + d->desc.rows < d->desc.global_rows;
		lo = south ? d->ghost_rows : 1;
		hi = d->desc.rows - (north ? d->ghost_rows : 1);
	} else launch_rows(d, 1, lo, hi);
	const PlanDomain pd = plan_domain(d);
	const PlanKnobs& knobs = plan_knobs();
	const int rseg2 = pair_tile_rows(pd, knobs, d->tiling.march2_rseg);    // (STRICT: 12-row tiles)
	if (!make_tile_map(launch_knobs(), lo, hi, 1, PART_ALL, (int)((p.cols - 2 + MARCH2_COLS - 1) / MARCH2_COLS), rseg2, rseg2, 0, tm, blocks, rseg2,
	                   0, d->own_lo, d->own_hi, d->tiling.march2_nbands))
		return HP_ERR_STATE;
	if (blocks > tail_limit(knobs)) return HP_ERR_STATE;                 // (the caller falls back to single iterations)
	d->tail_want = true; d->tail_allowed = true; d->push_now = strip;    // (strip: the final rows of the edge ranges leave with the launch)
	// single domain: the second iteration prices the primary buffer (1); a strip: ... and every rank reduces, through the mailboxes,
	// whose round is also the hand-over of the rows (7; fixed timestep: the round alone, 4) -- step_begin_impl's `fresh`
	d->tail_fresh = strip ? (d->desc.dynamic_dt ? 7 : 4) : (d->desc.dynamic_dt ? 1 : 0);
	d->tail_done = false;
	LaunchTail<T> tail;
	const int kind = make_tail<T>(d, blocks, PART_ALL, d->stream, tail_limit(knobs), tail);
	d->tail_want = false; d->tail_allowed = false; d->push_now = false;
	if (kind != (strip ? 2 : 1)) return HP_ERR_STATE;
	const bool bdy = pd.has_bdy;
	int rc;
	if ((rc = pair_stamps_alloc(d)) != HP_OK) return rc;
	bool in_place = false;
	if (bdy && !d->facts->m1_valid) {                                     // (queued in front of the pair launch: same stream)
		if ((rc = pair_cold_start<T>(d)) != HP_OK) return rc;
		in_place = true;
	} else if (bdy) in_place = d->facts->pair_fused_next;                 // the pair before stored this iteration's boundaries with its state
	tail.pair = bdy ? 2 : 1;
	tail.bdy_flag = bdy && followed ? 1 : 0;
	PairAux<T> aux{};
	const bool exact = pair_exact(pd, knobs) && d->z_state != nullptr;    // (the stamps' buffers: allocated just above, or not)
	if (exact) aux.stamps = StampBufs<T>{(char*)d->z_state, d->haz_words};
	aux.prev_gen = d->facts->other_stale ? d->pair_gen : 0u;              // `src` was written by a pair launch: its stamps apply
	aux.gen = ++d->pair_gen;
	if (aux.gen == 0) aux.gen = ++d->pair_gen;                            // (0 means "no launch")
	aux.list = (const AreaBdyList<T>*)d->fused_list; aux.fuse_next = bdy && followed ? 1 : 0; aux.in_place = in_place ? 1 : 0;
	aux.truncated = (d->desc.quirks & HP_QUIRK_BDY_TRUNCATED) != 0 ? 1 : 0;
	// still records: this launch writes the half the launch before did not, and reads that one if nothing has written a state buffer since
	const bool recs = pair_records(pd, knobs, strip, exact, rseg2);
	if (recs) {
		if ((rc = still_rec_alloc(d, tm.nstrips)) != HP_OK) return rc;
		StillRec* const base = (StillRec*)d->still_rec;
		aux.still_out = base + (size_t)(d->still_rec_half ^ 1) * d->still_rec_slots;
		aux.still_in = d->facts->still_rec_valid ? base + (size_t)d->still_rec_half * d->still_rec_slots : nullptr;
		aux.still_rows = d->desc.rows;
	}
	aux.wall = pair_wall_runs(knobs, recs) ? 1 : 0;
	// block order (hp_order.hpp): the instantiation that writes records -- with or without them -- raises its flags and leaves a table; it
	// reads the last one if that launch was the domain's flux launch just before this one, of this tiling (anything else: tile-row by tile-row)
	const bool ordered = pair_order_on() && d->desc.precision == 8 && d->desc.math_mode != HP_MATH_STRICT && !strip && !bdy && !exact &&
	                     tm.groups <= (int)ORDER_MAX_GROUPS;
	bool order_read = false;
	if (ordered) {
		if ((rc = order_alloc(d, tm)) != HP_OK) return rc;
		order_read = d->order_written && d->flux_launches == d->order_launch + 1;   // (make_tail, above, has counted this launch)
		const size_t table = (size_t)tm.nbands * tm.groups * (tm.nbig + tm.ntail);
		aux.order_in = order_read ? d->order_buf + (size_t)d->order_half * table : nullptr;
		aux.order_out = d->order_buf + (size_t)(d->order_half ^ 1) * table;
		aux.order_flags = d->order_buf + 2 * table;
	}
	const void* src = d->state[0];
	void* dst = d->state[1];
	// flux-kernel timing (hp_kernel_timing): as in step_begin_impl -- a sampled launch here covers two iterations
	const bool sample = d->timing_stride > 0 && d->timing_used < d->timing_events.size() &&
	                    (d->timing_counter++ % (uint64_t)d->timing_stride) == 0;
	if (sample) HIP_TRY(hipEventRecord(d->timing_events[d->timing_used].first, d->stream));
#define HP_LAUNCH_K1B2(CFL_, BDY_, HZ_, TAIL_)                                                                                            \
	hipLaunchKernelGGL((godunov_march2<false, CFL_, BDY_, HZ_, TAIL_, T>), dim3(blocks), dim3(256), 0, d->stream, p, (const Scalars<T>*)d->scalars, \
	                   (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst, (const T*)d->manning, (T*)d->cfl_slot,                    \
	                   (const T*)d->cfl_slot + SLOT_EDGE, tm, tail, aux)
#define HP_LAUNCH_K1B(CFL_, BDY_, TAIL_) do { if (exact) HP_LAUNCH_K1B2(CFL_, BDY_, true, TAIL_); else HP_LAUNCH_K1B2(CFL_, BDY_, false, TAIL_); } while (0)
	if (d->desc.math_mode == HP_MATH_STRICT)
		hipLaunchKernelGGL((godunov_march2<true, 1, false, true, 1, T>), dim3(blocks), dim3(256), 0, d->stream, p, (const Scalars<T>*)d->scalars,
		                   (const T*)d->bed, (const State4<T>*)src, (State4<T>*)dst, (const T*)d->manning, (T*)d->cfl_slot,
		                   (const T*)d->cfl_slot + SLOT_EDGE, tm, tail, aux);
	else
	if (strip)    { if (d->desc.dynamic_dt) HP_LAUNCH_K1B2(1, false, false, 2); else HP_LAUNCH_K1B2(0, false, false, 2); }     // (strips: no stamps -- a ghost row's would be the neighbour's to write)
	else if (bdy) HP_LAUNCH_K1B(1, true, 1);                              // (area boundaries pair with a dynamic timestep only: pairs_possible_common)
	else          { if (d->desc.dynamic_dt) HP_LAUNCH_K1B(1, false, 1); else HP_LAUNCH_K1B(0, false, 1); }
#undef HP_LAUNCH_K1B
#undef HP_LAUNCH_K1B2
	d->facts.pair_queued(bdy, followed);
	HIP_TRY(hipGetLastError());
	if (recs) d->still_rec_half ^= 1;
	d->facts.pair_launched(recs); d->still_rec_last = recs;
	if (ordered) { d->order_half ^= 1; d->order_launch = d->flux_launches; }
	d->order_written = ordered; d->order_read = order_read;
	if (sample) { HIP_TRY(hipEventRecord(d->timing_events[d->timing_used].second, d->stream)); d->timing_used++; }
	// the pass wrote state k + 2 into the other buffer: that buffer IS the primary one from here on (two single iterations would
	// have left the newest state in the primary buffer; the two buffers' edge rings are equal -- pair_eligible -- and so are their maxima)
	std::swap(d->state[0], d->state[1]);
	if (strip) {                                                          // every rank swaps: a neighbour's buffer b is the one it calls b now
		std::swap(d->peer_state[0][0], d->peer_state[0][1]);
		std::swap(d->peer_state[1][0], d->peer_state[1][1]);
	}
	d->facts.pair_ran(strip, d->ghost_rows);                              // (a strip: the exchange happened inside the launch)
	d->single_streak = 0;
	d->tail_done = false; d->fork_is_advance = false;
	d->adv_fresh = d->desc.dynamic_dt ? 1 : 0;
	d->cells_calculated += 2 * (uint64_t)d->desc.cols * (uint64_t)d->desc.rows;
	d->iterations += 2;
	d->pairs += 1;
	return HP_OK;
}
// `followed`: another iteration of the same batch comes after the pair (area boundaries: the pair stores its state with that iteration's
// boundaries applied, as K1's fused epilogue does; a batch's last launch never does -- what a download sees is the reference's buffer)
static int run_pair(hp_domain* d, const bool strip = false, const bool followed = false)
{
	return d->desc.precision == 8 ? run_pair_t<double>(d, strip, followed) : run_pair_t<float>(d, strip, followed);
}
// Before a single-iteration kernel builds on the non-current buffer again (it leaves all-dry cells of its destination untouched,
// quirk Q3): that buffer holds a state two iterations old after pairs -- bring it up to date with one device copy.
static int repair_other_buffer(hp_domain* d)
{
	if (!d->facts->other_stale) return HP_OK;
	d->facts.buffers_written_outside();
	// (the edge rings of the two buffers are equal whenever pairs have run: pair_eligible, hp_domain_upload_rows)
	HIP_TRY(hipMemcpyAsync(d->state[d->facts->use_alt ^ 1], d->state[d->facts->use_alt], d->cells * 4 * d->esize, hipMemcpyDeviceToDevice, d->stream));
	if (d->z_state) {                                                     // ... except where the last pair launch stamped a different value (PairAux)
		if (d->desc.precision == 8)
			hipLaunchKernelGGL((stamps_to_buffer<double>), dim3(1024), dim3(256), 0, d->stream, (State4<double>*)d->state[d->facts->use_alt ^ 1],
			                   StampBufs<double>{(char*)d->z_state, d->haz_words}, d->pair_gen, d->cells);
		else
			hipLaunchKernelGGL((stamps_to_buffer<float>), dim3(1024), dim3(256), 0, d->stream, (State4<float>*)d->state[d->facts->use_alt ^ 1],
			                   StampBufs<float>{(char*)d->z_state, d->haz_words}, d->pair_gen, d->cells);
		HIP_TRY(hipGetLastError());
	}
	d->facts.other_made_current();
	return HP_OK;
}
// What a checkpoint (hp_state_save) and the snapshot in front of a speculative batch (spec_begin) copy, queued on the domain's stream: both
// state buffers, state[first] in front, the scalars, and the WHOLE slot block: running maximum, last maximum used (SLOT_SAVED), ring
// maxima (SLOT_EDGE) -- round 2 kept the first four elements only, which since the slots moved 256 B apart no longer included the
// remembered maximum
static int snapshot_take(hp_domain* d, void* state, void* scalars, const int first)
{
	const size_t bytes = d->cells * 4 * d->esize;
	const size_t sc_bytes = d->desc.precision == 8 ? sizeof(Scalars<double>) : sizeof(Scalars<float>);
	HIP_TRY(hipMemcpyAsync(state, d->state[first], bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync((char*)state + bytes, d->state[first ^ 1], bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(scalars, d->scalars, sc_bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync((char*)scalars + sc_bytes, d->cfl_slot, CFL_SLOT_BYTES, hipMemcpyDeviceToDevice, d->stream));
	return HP_OK;
}

int dispatch_begin(hp_domain* d)
{
	d->facts.buffers_written_outside();                                   // (a single iteration writes the other buffer, its boundaries the current one)
	// after iteration pairs the non-current buffer is out of date: K1's FILL flag, or the device copy first
	const bool fill = fill_wanted(plan_domain(d), d->facts, plan_knobs());
	if (!fill) { const int rc0 = repair_other_buffer(d); if (rc0 != HP_OK) return rc0; }
	d->fill_now = fill;
	const bool strict = d->desc.math_mode == HP_MATH_STRICT;
	const int rc = d->desc.precision == 8 ? (strict ? step_begin_impl<double, true>(d) : step_begin_impl<double, false>(d))
	                                      : (strict ? step_begin_impl<float, true>(d) : step_begin_impl<float, false>(d));
	d->fill_now = false;
	if (fill && rc == HP_OK) d->facts.other_made_current();
	return rc;
}

int dispatch_end(hp_domain* d)
{
	return d->desc.precision == 8 ? step_end_impl<double>(d) : step_end_impl<float>(d);
}

template <typename T> int write_scalars_initial(hp_domain* d)
{
	Scalars<T> s;
	s.t = T(0); s.dt = (T)d->desc.dt_initial; s.t_hydro = T(0); s.t_sync = T(0); s.batch_dt = T(0);
	s.batch_ok = 0; s.batch_skipped = 0;                                  // CSchemeGodunov.cpp:805-867
	HIP_TRY(hipMemcpy(d->scalars, &s, sizeof s, hipMemcpyHostToDevice));
	return HP_OK;
}

// One time-control scalar rewritten in stream order, without blocking: the value travels as a kernel argument, so
// no host staging buffer has to outlive the call (the reference enqueues these writes non-blocking too,
// CSchemeGodunov.cpp:1166-1176, :1213-1232).
template <typename T> __global__ void store_scalar(T* where, const T value) { *where = value; }

template <typename T> int set_scalar_field(hp_domain* d, size_t offset, double value)
{
	hipLaunchKernelGGL(store_scalar<T>, dim3(1), dim3(1), 0, d->stream, (T*)((char*)d->scalars + offset), (T)value);
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

int spec_resolve(hp_domain* d);
int tail_failed_error()
{
	return fail(HP_ERR_STATE, "a flux launch's tail block gave up waiting for a flux block (HP_TAIL_TIMEOUT_MS): time and timestep "
	                          "are frozen from that iteration on, the domain's state is not valid; destroy the domain");
}
int check_domain(hp_domain* d)
{
	if (d) d->fork_is_advance = false;        // any entry point may queue work behind the last advance_time
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	hipError_t e = hipSetDevice(d->desc.device);
	if (e != hipSuccess) return fail(HP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
	if (d->tail_failed) return tail_failed_error();      // (hp_domain_destroy does not come through here)
	// a speculative STRICT batch is still to be looked at: whoever enters the library next does that first, so that nothing is
	// ever queued behind -- or read from -- a batch that has to be re-run
	if (d->spec_pending) return spec_resolve(d);
	return HP_OK;
}

} // namespace

// =================================================================================================
extern "C" {

int hp_abi_version(void) { return HP_ABI_VERSION; }

const char* hp_last_error(void) { return g_last_error.c_str(); }

int hp_set_log_sink(hp_log_sink_t sink, void* user)
{
	g_log_sink.store(nullptr, std::memory_order_release);
	g_log_user.store(user, std::memory_order_release);
	g_log_sink.store(sink, std::memory_order_release);
	return HP_OK;
}

int hp_device_count(int* count)
{
	if (!count) return fail(HP_ERR_INVALID, "count == NULL");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		*count = 0;
		return fail(HP_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
	}
	*count = n;
	return HP_OK;
}

int hp_device_info(int device, hp_device_info_t* info)
{
	if (!info) return fail(HP_ERR_INVALID, "info == NULL");
	int n = 0, rc = hp_device_count(&n);
	if (rc != HP_OK) return rc;
	if (device < 0 || device >= n) return fail(HP_ERR_INVALID, "device index out of range");
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	std::memset(info, 0, sizeof *info);
	std::snprintf(info->name, sizeof info->name, "%s", prop.name);
	std::snprintf(info->arch, sizeof info->arch, "%s", prop.gcnArchName);
	info->compute_units = prop.multiProcessorCount;
	info->clock_mhz = prop.clockRate / 1000;
	info->global_mem_bytes = prop.totalGlobalMem;
	info->lds_bytes_per_cu = prop.maxSharedMemoryPerMultiProcessor;
	info->wavefront = prop.warpSize;
	info->fp64 = 1;
	return HP_OK;
}

void hp_domain_desc_default(hp_domain_desc_t* desc)
{
	if (!desc) return;
	std::memset(desc, 0, sizeof *desc);
	desc->struct_size = (uint32_t)sizeof *desc;
	desc->device = 0;
	desc->dx = 1.0;
	desc->precision = 8;
	desc->scheme = HP_SCHEME_GODUNOV;
	desc->courant = 0.5;                 // CScheme.cpp:48
	desc->dry_threshold = 1e-10;         // CSchemeGodunov.cpp:56
	desc->friction = 1;                  // CScheme.cpp:51
	desc->dynamic_dt = 1;                // CScheme.cpp:50
	desc->dt_fixed = 0.001;
	desc->dt_initial = 0.001;            // CScheme.cpp:49
	desc->t_end = 1e30;
	desc->quirks = HP_QUIRKS_REFERENCE;
	desc->math_mode = HP_MATH_FAST;
	desc->kernel = HP_KERNEL_AUTO;
}

int hp_domain_create(const hp_domain_desc_t* desc, hp_domain_t** out)
{
	if (!desc || !out) return fail(HP_ERR_INVALID, "null argument");
	if (desc->struct_size != sizeof(hp_domain_desc_t)) return fail(HP_ERR_INVALID, "hp_domain_desc_t size mismatch");
	if (desc->cols < 3 || desc->rows < 3) return fail(HP_ERR_INVALID, "grid must be at least 3x3");
	if (desc->precision != 8 && desc->precision != 4) return fail(HP_ERR_INVALID, "precision must be 8 or 4");
	if (desc->scheme != HP_SCHEME_GODUNOV && desc->scheme != HP_SCHEME_MUSCL_HANCOCK &&
	    desc->scheme != HP_SCHEME_INERTIAL)
		return fail(HP_ERR_INVALID, "unknown scheme");
	if (!(desc->dx > 0)) return fail(HP_ERR_INVALID, "dx must be positive");
	int n = 0, rc = hp_device_count(&n);
	if (rc != HP_OK) return rc;
	if (desc->device < 0 || desc->device >= n) return fail(HP_ERR_INVALID, "device index out of range");
	HIP_TRY(hipSetDevice(desc->device));

	hp_domain* d = new hp_domain();
	d->desc = *desc;
	if (d->desc.global_rows <= 0) { d->desc.global_rows = d->desc.rows; d->desc.row_offset = 0; }
	if (d->desc.row_offset < 0 || d->desc.row_offset + d->desc.rows > d->desc.global_rows) {
		delete d;
		return fail(HP_ERR_INVALID, "strip does not fit the global grid");
	}
	const long g = stencil_reach(*desc);                                  // = ghost rows per exchange
	d->ghost_rows = desc->ghost_rows > 0 ? desc->ghost_rows : g;
	if (d->ghost_rows != g && d->ghost_rows != 2 * g) {
		delete d;
		return fail(HP_ERR_INVALID, "ghost_rows must be 0, the scheme's stencil reach or twice that");
	}
	d->facts.ghosts_exchanged(d->ghost_rows);
	d->split_now = true;                                                  // (hp_step_begin: every iteration is followed by an exchange)
	d->own_lo = (d->desc.row_offset > 0) ? d->ghost_rows : 0;
	d->own_hi = d->desc.rows - ((d->desc.row_offset + d->desc.rows < d->desc.global_rows) ? d->ghost_rows : 0);
	if (d->own_hi - d->own_lo < 1) { delete d; return fail(HP_ERR_INVALID, "strip has no owned rows"); }
	d->cells = (size_t)desc->cols * (size_t)desc->rows;
	d->esize = (size_t)desc->precision;
	{
		int cus = 256;
		hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, desc->device);
		const TilingKnobs knobs = tiling_knobs();
		Tiling& t = d->tiling;
		t = pick_tiling(desc->cols, desc->rows, desc->precision, cus, knobs);
		if (t.print_tiling)
			std::fprintf(stderr, "[hipims_mi] tiling %ld x %ld: K1/K6 %d rows x %d bands, K2 %d rows x %d bands\n", (long)desc->cols, (long)desc->rows,
			             t.march_rseg, t.march_nbands, t.muscl_rseg, t.muscl_nbands);
		force_heights(t, knobs);
		if (t.print_tiling)
			std::fprintf(stderr, "[hipims_mi] tiling %ld x %ld: pair kernel %d rows x %d bands, %s\n", (long)desc->cols, (long)desc->rows, t.march2_rseg,
			             t.march2_nbands, t.march2_pays ? "taken by default" : "not taken by default");
		if (!tiles_addressable(t, desc->cols, desc->precision)) {
			delete d;
			return fail(HP_ERR_UNSUPPORTED, "grid too wide for the tile addressing (cols * 32 B * (rows per tile + 4) >= 2 GiB)");
		}
	}

	auto cleanup = [&](int code) { hp_domain_destroy(d); return code; };
#define HIP_TRY_C(expr)                                                                                \
	do {                                                                                               \
		hipError_t e_ = (expr);                                                                        \
		if (e_ != hipSuccess)                                                                          \
			return cleanup(fail(HP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));       \
	} while (0)
	HIP_TRY_C(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
	HIP_TRY_C(hipMalloc(&d->state[0], d->cells * 4 * d->esize));
	HIP_TRY_C(hipMalloc(&d->state[1], d->cells * 4 * d->esize));
	HIP_TRY_C(hipMalloc(&d->bed, d->cells * d->esize));
	HIP_TRY_C(hipMalloc(&d->manning, d->cells * d->esize));
	HIP_TRY_C(hipMalloc(&d->scalars, 256));
	HIP_TRY_C(hipMalloc(&d->cfl_slot, CFL_SLOT_BYTES));
	if (std::getenv("HP_PRINT_BUFFERS"))
		std::fprintf(stderr, "[hipims_mi] buffers: state[0] %p state[1] %p bed %p manning %p\n", d->state[0], d->state[1], d->bed, d->manning);

	HIP_TRY_C(hipMalloc((void**)&d->tail_words, 2 * (TAIL_MAX_BLOCKS + 8) * sizeof(unsigned long long)));
	HIP_TRY_C(hipMemset(d->tail_words, 0xff, 2 * (TAIL_MAX_BLOCKS + 8) * sizeof(unsigned long long)));      // every word EMPTY (two arrays: LaunchTail::done, done1)
	HIP_TRY_C(hipHostMalloc(&d->host_scalars, HOST_BLOCK_BYTES, hipHostMallocDefault));
	HIP_TRY_C(hipMemset(d->state[0], 0, d->cells * 4 * d->esize));
	HIP_TRY_C(hipMemset(d->state[1], 0, d->cells * 4 * d->esize));
	HIP_TRY_C(hipMemset(d->bed, 0, d->cells * d->esize));
	HIP_TRY_C(hipMemset(d->manning, 0, d->cells * d->esize));
	HIP_TRY_C(hipMemset(d->cfl_slot, 0, CFL_SLOT_BYTES));
	HIP_TRY_C(hipMemset(d->scalars, 0, 256));
	HIP_TRY_C(hipEventCreate(&d->ev_start));
	HIP_TRY_C(hipEventCreate(&d->ev_stop));
	{
		int lo = 0, hi = 0;                                               // numerically lower = higher priority
		HIP_TRY_C(hipDeviceGetStreamPriorityRange(&lo, &hi));
		HIP_TRY_C(hipStreamCreateWithPriority(&d->stream_halo, hipStreamNonBlocking, hi));
	}
	HIP_TRY_C(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
	HIP_TRY_C(hipEventCreateWithFlags(&d->ev_halo, hipEventDisableTiming));
#undef HIP_TRY_C
	rc = (d->desc.precision == 8) ? write_scalars_initial<double>(d) : write_scalars_initial<float>(d);
	if (rc != HP_OK) return cleanup(rc);
	*out = d;
	return HP_OK;
}

int hp_domain_destroy(hp_domain_t* d)
{
	if (!d) return HP_OK;
	hipSetDevice(d->desc.device);
	if (d->stream) hipStreamSynchronize(d->stream);
	if (d->stream_halo) hipStreamSynchronize(d->stream_halo);
	peer_release(d);
	for (auto& b : d->bdy) { hipFree(b.data); hipFree(b.cells); }
	for (auto& ev : d->timing_events) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
	hipFree(d->state[0]); hipFree(d->state[1]); hipFree(d->bed); hipFree(d->manning);
	hipFree(d->scalars); hipFree(d->cfl_slot);
	hipFree(d->saved_state); hipFree(d->saved_scalars); hipFree(d->fused_list); hipFree(d->tail_words);
	hipFree(d->z_state); hipFree(d->haz_words); hipFree(d->still_rec); hipFree(d->order_buf);
	for (hipEvent_t e : d->tune_ev) if (e) hipEventDestroy(e);
	hipFree(d->spec_state); hipFree(d->spec_scalars);
	participants_destroy(d);
	if (d->host_scalars) hipHostFree(d->host_scalars);
	if (d->ev_start) hipEventDestroy(d->ev_start);
	if (d->ev_stop) hipEventDestroy(d->ev_stop);
	if (d->ev_fork) hipEventDestroy(d->ev_fork);
	if (d->ev_halo) hipEventDestroy(d->ev_halo);
	if (d->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(d->comm);
	if (d->ev_xchg) hipEventDestroy(d->ev_xchg);
	if (d->stream_halo) hipStreamDestroy(d->stream_halo);
	if (d->stream) hipStreamDestroy(d->stream);
	delete d;
	return HP_OK;
}

int hp_domain_upload(hp_domain_t* d, int which, const void* host, size_t bytes)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.boundaries_or_bed_changed();
	d->facts.buffers_written_outside();                                   // (state, bed or Manning: the records describe the old ones)
	if (!host) return fail(HP_ERR_INVALID, "host == NULL");
	if (d->in_step) return fail(HP_ERR_STATE, "upload between hp_step_begin and hp_step_end");
	switch (which) {
	case HP_ARRAY_STATE:
		if (bytes != d->cells * 4 * d->esize) return fail(HP_ERR_INVALID, "state size mismatch");
		// both ping-pong buffers get the same host array (CSchemeGodunov.cpp:1064-1065)
		HIP_TRY(hipMemcpyAsync(d->state[0], host, bytes, hipMemcpyHostToDevice, d->stream));
		HIP_TRY(hipMemcpyAsync(d->state[1], host, bytes, hipMemcpyHostToDevice, d->stream));
		return state_replaced(d);
	case HP_ARRAY_BED:
		if (bytes != d->cells * d->esize) return fail(HP_ERR_INVALID, "bed size mismatch");
		HIP_TRY(hipMemcpyAsync(d->bed, host, bytes, hipMemcpyHostToDevice, d->stream));
		d->facts.bed_uploaded();
		return HP_OK;
	case HP_ARRAY_MANNING:
		if (bytes != d->cells * d->esize) return fail(HP_ERR_INVALID, "manning size mismatch");
		HIP_TRY(hipMemcpyAsync(d->manning, host, bytes, hipMemcpyHostToDevice, d->stream));
		{
			// "constant" Manning sources are the norm (<dataSource type="constant" value="manningCoefficient">):
			// a uniform array is passed to the kernels as a scalar and its 8 B/cell are not streamed every step
			bool same = true;
			if (d->esize == 8) {
				const double* v = (const double*)host;
				for (size_t i = 1; i < d->cells && same; ++i) same = (v[i] == v[0]);
				d->manning_value = v[0];
			} else {
				const float* v = (const float*)host;
				for (size_t i = 1; i < d->cells && same; ++i) same = (v[i] == v[0]);
				d->manning_value = v[0];
			}
			d->manning_uniform = same;
		}
		return HP_OK;
	}
	return fail(HP_ERR_INVALID, "unknown array id");
}

// saveCurrentState / rollbackSimulation without the PCIe round trip: the copy stays in HBM
int hp_state_save(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_state_save between hp_step_begin and hp_step_end");
	if ((rc = repair_other_buffer(d)) != HP_OK) return rc;           // (after iteration pairs: see run_pair)
	if ((rc = participants_do(d, &Participant::reserve)) != HP_OK) return rc;    // (first: a failure leaves the checkpoint before it untouched)
	const size_t bytes = d->cells * 4 * d->esize;
	const size_t sc_bytes = d->desc.precision == 8 ? sizeof(Scalars<double>) : sizeof(Scalars<float>);
	// BOTH ping-pong buffers: the one the next iteration writes is not dead -- cells whose whole neighbourhood is dry are left
	// untouched by the flux kernel (quirk Q3) and keep what that buffer held, so a replay needs it too (a fuzz over random
	// configurations found 6 % of them replaying differently when only the next-source buffer was kept, round 3)
	if (!d->saved_state) HIP_TRY(hipMalloc(&d->saved_state, 2 * bytes));
	if (!d->saved_scalars) HIP_TRY(hipMalloc(&d->saved_scalars, sc_bytes + CFL_SLOT_BYTES));
	if ((rc = snapshot_take(d, d->saved_state, d->saved_scalars, d->facts->use_alt)) != HP_OK) return rc;
	d->facts.checkpoint_taken();
	d->saved_valid = true;
	return participants_do(d, &Participant::save);
}

int hp_state_restore(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_state_restore between hp_step_begin and hp_step_end");
	if (!d->saved_valid) return fail(HP_ERR_STATE, "hp_state_restore without a saved state");
	d->facts.buffers_written_outside();
	const size_t bytes = d->cells * 4 * d->esize;
	const size_t sc_bytes = d->desc.precision == 8 ? sizeof(Scalars<double>) : sizeof(Scalars<float>);
	// both ping-pong buffers return to what EACH of them held (rollbackSimulation writes the saved next-source state into both,
	// CSchemeGodunov.cpp:1496-1499, after which its cells with an all-dry neighbourhood no longer continue as the original run
	// did), and so do the ping-pong phase and the remembered CFL maxima: the steps that follow repeat the original ones bit for bit
	HIP_TRY(hipMemcpyAsync(d->state[d->facts.saved().use_alt], d->saved_state, bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(d->state[d->facts.saved().use_alt ^ 1], (char*)d->saved_state + bytes, bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(d->scalars, d->saved_scalars, sc_bytes, hipMemcpyDeviceToDevice, d->stream));
	// (the slot block AROUND the sticky "a tail block gave up" word: a word raised since the checkpoint, and not yet seen by the host
	// through hp_sync / hp_read_scalars, must survive the roll-back -- ADVICE r05)
	{
		const size_t lo = (size_t)SLOT_TAIL_ERR * d->esize, hi = lo + d->esize;
		const char* from = (const char*)d->saved_scalars + sc_bytes;
		HIP_TRY(hipMemcpyAsync(d->cfl_slot, from, lo, hipMemcpyDeviceToDevice, d->stream));
		HIP_TRY(hipMemcpyAsync((char*)d->cfl_slot + hi, from + hi, CFL_SLOT_BYTES - hi, hipMemcpyDeviceToDevice, d->stream));
	}
	d->facts.checkpoint_restored();
	d->tune_phase = 0;                                                    // (another state: the exact mode's pairs-or-singles choice is measured anew -- a sample
	                                                                      // still in flight measured the state that is being replaced: with samples every 128
	                                                                      // iterations bench.py's restore found one in flight nearly every time and the timed
	                                                                      // region ran on a choice made for the pre-warmed flood)
	d->fork_is_advance = false;
	return participants_do(d, &Participant::restore);
}

int hp_domain_download(hp_domain_t* d, int which, void* host, int64_t row0, int64_t nrows)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!host) return fail(HP_ERR_INVALID, "host == NULL");
	if ((rc = check_rows(d, row0, nrows)) != HP_OK) return rc;
	const size_t per_row = (size_t)d->desc.cols * d->esize * (which == HP_ARRAY_STATE ? 4 : 1);
	const void* base;
	switch (which) {
	case HP_ARRAY_STATE:   base = d->state[d->facts->use_alt]; break;     // getNextCellSourceBuffer (:1705-1715)
	case HP_ARRAY_BED:     base = d->bed; break;
	case HP_ARRAY_MANNING: base = d->manning; break;
	default: return fail(HP_ERR_INVALID, "unknown array id");
	}
	HIP_TRY(hipMemcpyAsync(host, (const char*)base + (size_t)row0 * per_row, (size_t)nrows * per_row,
	                       hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}

int hp_domain_upload_rows(hp_domain_t* d, const void* host, int64_t row0, int64_t nrows)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.time_control_changed();                                     // (not boundaries_or_bed_changed: hp_facts.hpp, ODD)
	d->facts.buffers_written_outside();
	if (!host) return fail(HP_ERR_INVALID, "host == NULL");
	if ((rc = check_rows(d, row0, nrows)) != HP_OK) return rc;
	const size_t per_row = (size_t)d->desc.cols * d->esize * 4;
	// queueWritePartial goes to the CURRENT buffer only: the other one keeps what it held -- after iteration pairs it has to be
	// brought up to date first, or the rows written now would reach it with the next single iteration's FILL
	if ((rc = repair_other_buffer(d)) != HP_OK) return rc;
	HIP_TRY(hipMemcpyAsync((char*)d->state[d->facts->use_alt] + (size_t)row0 * per_row, host, (size_t)nrows * per_row,
	                       hipMemcpyHostToDevice, d->stream));
	d->facts.rows_uploaded();
	return HP_OK;
}

int hp_set_target_time(hp_domain_t* d, double t)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.time_control_changed();
	return d->desc.precision == 8 ? set_scalar_field<double>(d, offsetof(Scalars<double>, t_sync), t)
	                              : set_scalar_field<float>(d, offsetof(Scalars<float>, t_sync), t);
}

int hp_set_time(hp_domain_t* d, double t)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.time_control_changed();
	return d->desc.precision == 8 ? set_scalar_field<double>(d, offsetof(Scalars<double>, t), t)
	                              : set_scalar_field<float>(d, offsetof(Scalars<float>, t), t);
}

int hp_force_timestep(hp_domain_t* d, double dt)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.time_control_changed();
	return d->desc.precision == 8 ? set_scalar_field<double>(d, offsetof(Scalars<double>, dt), dt)
	                              : set_scalar_field<float>(d, offsetof(Scalars<float>, dt), dt);
}

int hp_reset_counters(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	const size_t off = d->desc.precision == 8 ? offsetof(Scalars<double>, batch_dt) : offsetof(Scalars<float>, batch_dt);
	const size_t end = d->desc.precision == 8 ? sizeof(Scalars<double>) : sizeof(Scalars<float>);
	HIP_TRY(hipMemsetAsync((char*)d->scalars + off, 0, end - off, d->stream));
	return HP_OK;
}

int hp_update_timestep(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.time_control_changed();
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	if (d->desc.dynamic_dt && d->desc.global_rows != d->desc.rows)
		return fail(HP_ERR_UNSUPPORTED, "hp_update_timestep on a row strip: the maximum must be all-reduced across "
		                                "ranks not available through this call)");
	// tst_Reduce reads the primary buffer (arg wiring CSchemeGodunov.cpp:922, :927), then tst_UpdateTimestep.  MUSCL-Hancock
	// has ONE state buffer in the reference, updated in place -- its primary buffer is always the current state, which here
	// is whichever ping-pong buffer the next iteration reads (found by the fuzz's update-timestep calls between batches)
	const void* priced = d->desc.scheme == HP_SCHEME_MUSCL_HANCOCK ? d->state[d->facts->use_alt] : d->state[0];
	if (d->desc.precision == 8) {
		if (d->desc.dynamic_dt && (rc = launch_reduce<double>(d, priced, d->own_lo, d->own_hi)) != HP_OK) return rc;
		hipLaunchKernelGGL((advance_time<true, double>), dim3(1), dim3(64), 0, d->stream, make_params<double>(d),
		                   (Scalars<double>*)d->scalars, (double*)d->cfl_slot, 1, PeerBox{}, PeerPush{});
	} else {
		if (d->desc.dynamic_dt && (rc = launch_reduce<float>(d, priced, d->own_lo, d->own_hi)) != HP_OK) return rc;
		hipLaunchKernelGGL((advance_time<true, float>), dim3(1), dim3(64), 0, d->stream, make_params<float>(d),
		                   (Scalars<float>*)d->scalars, (float*)d->cfl_slot, 1, PeerBox{}, PeerPush{});
	}
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

int hp_step_begin(hp_domain_t* d)
{
	const bool fork_ready = d && d->fork_is_advance;     // nothing was queued since the last hp_step_end
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_step_begin called twice");
	if (d->ghost_rows != stencil_reach(d->desc))
		return fail(HP_ERR_UNSUPPORTED, "the split step exchanges after every iteration: it needs ghost_rows = the stencil reach "
		                                "(two reaches of ghost rows are hp_strip_step_batch's)");
	d->split_now = true;
	d->fork_is_advance = fork_ready;
	d->facts.single_begins();
	if ((rc = dispatch_begin(d)) != HP_OK) return rc;
	d->in_step = true;
	return HP_OK;
}

int hp_step_needs_reduction(hp_domain_t* d, int* needed)
{
	if (!d || !needed) return fail(HP_ERR_INVALID, "null argument");
	if (!d->in_step) return fail(HP_ERR_STATE, "hp_step_needs_reduction outside a split step");
	*needed = d->adv_fresh;
	return HP_OK;
}

int hp_step_end(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!d->in_step) return fail(HP_ERR_STATE, "hp_step_end without hp_step_begin");
	d->in_step = false;
	return dispatch_end(d);
}

} // extern "C"
namespace {
// ---- speculative STRICT fp64 batches -------------------------------------------------------------------------------------
// The STRICT flux kernels have a flavour whose quotients share refined reciprocals (hp_math.hpp: div_shared): bit-identical to
// the plain divisions except for operands at the ends of the exponent range, which it DETECTS (SLOT_SPEC) but does not handle
// -- every in-kernel fall-back cost more than the sharing gains (profiles/r04i).  A batch of at least SPEC_MIN iterations on a
// single domain therefore runs speculatively: snapshot (both state buffers, scalars, slot block: as hp_state_save), the
// shared-reciprocal kernels, the flag word copied to pinned memory behind the last launch.  The next entry into the library
// (check_domain) waits for the batch, looks at the word and, if it is raised, puts the snapshot back and runs the same
// iterations with the plain kernels.  Cost of the snapshot: two device copies of the state per batch (0.45 ms at 4096^2, i.e.
// one iteration's worth per batch); HP_STRICT_SPECULATE=1 switches it on (see hp_plan.hpp: spec_wanted for why it is off by default),
// HP_STRICT_SPEC_FORCE=k pretends every k-th batch raised the word (tests).
int spec_begin(hp_domain* d)
{
	const size_t bytes = d->cells * 4 * d->esize, sc_bytes = sizeof(Scalars<double>);
	// (after iteration pairs, as hp_state_save: the batch's first single iteration would repair the other buffer and clear other_stale, and
	// a replay would put the stale copy back with the flag down)
	{ const int rc = repair_other_buffer(d); if (rc != HP_OK) return rc; }
	if (!d->spec_state) HIP_TRY(hipMalloc(&d->spec_state, 2 * bytes));
	if (!d->spec_scalars) HIP_TRY(hipMalloc(&d->spec_scalars, sc_bytes + CFL_SLOT_BYTES));
	HIP_TRY(hipMemsetAsync((char*)d->cfl_slot + (size_t)SLOT_SPEC * d->esize, 0, d->esize, d->stream));
	{ const int rc = snapshot_take(d, d->spec_state, d->spec_scalars, 0); if (rc != HP_OK) return rc; }
	d->facts.spec_taken();
	d->spec_host.adv_fresh = d->adv_fresh;
	d->spec_host.cells_calculated = d->cells_calculated; d->spec_host.iterations = d->iterations;
	d->spec_now = true;
	return HP_OK;
}
// The exact mode's choice between pairs and single iterations (round 6).  STRICT pairs are STRICT single iterations bit for bit, so the
// choice is free -- and workload dependent: rows of still water are a copy in STRICT (K1's skip) which a pair makes at half the bytes
// (S-DAM 4096^2: 0.299 -> 0.265 ms per iteration), while water that moves everywhere is bound by instruction issue, where the pair's two
// extra first-step rows per tile and its narrower wavefronts cost 13 % (S-ROUGH: 0.60 -> 0.68 ms; profiles/r06h_strict_pairs.txt).  So the
// engine measures: every 128 iterations two pairs and four single iterations are bracketed by events on the domain's stream
// (nothing blocks: the events are looked at every sixteen iterations of the batch loop and when a batch starts -- a host that queues far
// ahead of the device sees them complete at the next batch call) and the faster flavour runs until the next sample.
// (Round 6, late: the period was 512 and the events were only looked at when a batch STARTED -- on a developing S-DAM flood the crossover
// lies near iteration 1000 and the engine ran pairs until the sample of iteration 1750, 9 % behind single iterations all the while;
// now, in batches of 250, it switches in the batch that contains the crossover: tools/strict_tuner_probe.py, profiles/r06ak_*.  A sample costs one copy of the state and six iterations in the slower flavour: 0.1-0.2 % at this period.)
// HP_PAIR_TUNE=0: always pairs where eligible; HP_PAIR_TUNE_PERIOD=n: iterations between samples.
static int tuner_poll(hp_domain* d)
{
	if (d->tune_phase == 1 && hipEventQuery(d->tune_ev[3]) == hipSuccess) {
		float pair_ms = 0.f, single_ms = 0.f;
		HIP_TRY(hipEventElapsedTime(&pair_ms, d->tune_ev[0], d->tune_ev[1]));
		HIP_TRY(hipEventElapsedTime(&single_ms, d->tune_ev[2], d->tune_ev[3]));
		const bool prefer = pair_ms < 0.98f * single_ms;
		if (prefer != d->tune_prefer_pairs) d->tune_switches++;
		d->tune_prefer_pairs = prefer;
		d->tune_pair_ms = pair_ms; d->tune_single_ms = single_ms;
		d->tune_samples++;
		d->tune_phase = 2;
		static const uint64_t period = std::getenv("HP_PAIR_TUNE_PERIOD") ? (uint64_t)std::max(12L, std::atol(std::getenv("HP_PAIR_TUNE_PERIOD"))) : 128;
		d->tune_next = d->iterations + period;
	}
	if (d->tune_phase == 2 && d->iterations >= d->tune_next) d->tune_phase = 0;
	return HP_OK;
}
int run_single(hp_domain* d, const bool followed)
{
	// (K1 FUSED) every iteration but the last carries its successor's rain / loss: between batches the buffers are
	// what the reference's are -- a download never sees rain of an iteration that has not begun
	d->fuse_next = followed;
	d->facts.single_begins();
	d->tail_allowed = true;                        // nothing is queued between the flux launch and the advance in this loop
	int rc = dispatch_begin(d);
	d->tail_allowed = false;
	if (rc != HP_OK) return rc;
	return dispatch_end(d);
}
int run_iterations(hp_domain* d, uint32_t n_iterations)
{
	int rc;
	const bool tune = tuner_on(plan_domain(d), plan_knobs());
	if (tune && (rc = tuner_poll(d)) != HP_OK) return rc;
	// (partial uploads since the last look: the rings are compared once, before the first pair_eligible -- blocks)
	if (d->facts->rings_differ && !d->facts->rings_checked && n_iterations >= 2 && pairs_possible(plan_domain(d), plan_knobs()) && (rc = rings_really_differ(d)) != HP_OK) return rc;
	for (uint32_t i = 0; i < n_iterations; ++i) {
		if (tune && d->tune_phase != 0 && (i & 15u) == 15u && (rc = tuner_poll(d)) != HP_OK) return rc;   // (two event queries: host time, behind the queue)
		// (STRICT) a sample: three pairs, then six single iterations -- the first pair and the first two single iterations warm the
		// kernel's code and are not timed, the rest are bracketed by events
		if (tune && d->tune_phase == 0 && i + 12 <= n_iterations && !d->facts->rings_differ && pair_eligible(plan_domain(d), d->facts, plan_knobs())) {
			for (hipEvent_t& e : d->tune_ev) if (!e) HIP_TRY(hipEventCreate(&e));
			if ((rc = pair_stamps_alloc(d)) != HP_OK) return rc;           // (the first pair's allocation and its memset are not the pair's price)
			rc = run_pair(d, false, true);
			if (rc == HP_OK) {
				HIP_TRY(hipEventRecord(d->tune_ev[0], d->stream));
				if ((rc = run_pair(d, false, true)) != HP_OK || (rc = run_pair(d, false, true)) != HP_OK) return rc;
				HIP_TRY(hipEventRecord(d->tune_ev[1], d->stream));
				if ((rc = repair_other_buffer(d)) != HP_OK) return rc;    // (not part of an iteration's price: a run of single iterations pays it once)
				if ((rc = run_single(d, true)) != HP_OK || (rc = run_single(d, true)) != HP_OK) return rc;
				HIP_TRY(hipEventRecord(d->tune_ev[2], d->stream));
				for (int k = 0; k < 4; ++k)
					if ((rc = run_single(d, k < 3 || i + 12 < n_iterations)) != HP_OK) return rc;
				HIP_TRY(hipEventRecord(d->tune_ev[3], d->stream));
				d->tune_phase = 1;
				i += 11;
				continue;
			}
			if (rc != HP_ERR_STATE) return rc;
		}
		if (i + 2 <= n_iterations && (!tune || d->tune_prefer_pairs) && pair_eligible(plan_domain(d), d->facts, plan_knobs())) {
			rc = run_pair(d, false, i + 2 < n_iterations);
			if (rc == HP_OK) { ++i; continue; }
			if (rc != HP_ERR_STATE) return rc;                 // (HP_ERR_STATE: not launchable as a pair -- single iterations)
		}
		if ((rc = run_single(d, i + 1 < n_iterations)) != HP_OK) return rc;
	}
	d->fuse_next = 0;
	return HP_OK;
}
int spec_resolve(hp_domain* d)
{
	const uint32_t n = d->spec_pending;
	d->spec_pending = 0;
	HIP_TRY(hipStreamSynchronize(d->stream));
	static const long force = std::getenv("HP_STRICT_SPEC_FORCE") ? std::atol(std::getenv("HP_STRICT_SPEC_FORCE")) : 0;
	const double flag = *(volatile double*)((char*)d->host_scalars + HOST_SPEC_FLAG);
	const bool raised = flag != 0.0 || (force > 0 && d->spec_batches % (uint64_t)force == 0);
	if (!raised) return HP_OK;
	// some quotient of the batch fell outside what the shared-reciprocal division covers: the batch never happened
	d->spec_replays++;
	log_line(HP_LOG_INFORMATION, "a speculative STRICT batch of " + std::to_string(n) + " iterations is re-run with the plain divisions");
	const size_t bytes = d->cells * 4 * d->esize, sc_bytes = sizeof(Scalars<double>);
	d->facts.buffers_written_outside();
	HIP_TRY(hipMemcpyAsync(d->state[0], d->spec_state, bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(d->state[1], (char*)d->spec_state + bytes, bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(d->scalars, d->spec_scalars, sc_bytes, hipMemcpyDeviceToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(d->cfl_slot, (char*)d->spec_scalars + sc_bytes, CFL_SLOT_BYTES, hipMemcpyDeviceToDevice, d->stream));
	d->facts.spec_replayed();
	d->adv_fresh = d->spec_host.adv_fresh;
	d->cells_calculated = d->spec_host.cells_calculated; d->iterations = d->spec_host.iterations;
	d->fork_is_advance = false;
	return run_iterations(d, n);
}
} // namespace
extern "C" {

int hp_step_batch(hp_domain_t* d, uint32_t n_iterations)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	const bool speculate = spec_wanted(plan_domain(d), plan_knobs(), n_iterations);
	if (speculate && (rc = spec_begin(d)) != HP_OK) return rc;
	rc = run_iterations(d, n_iterations);
	if (speculate) {
		d->spec_now = false;
		if (rc != HP_OK) return rc;
		d->spec_batches++;
		HIP_TRY(hipMemcpyAsync((char*)d->host_scalars + HOST_SPEC_FLAG, (char*)d->cfl_slot + (size_t)SLOT_SPEC * d->esize, 8,
		                       hipMemcpyDeviceToHost, d->stream));
		d->spec_pending = n_iterations;
	}
	return rc;
}

// The mailboxes' sticky error word (a strip that was not heard from within HP_PEER_TIMEOUT_MS: the tail / advance kernel then
// went on with a partial maximum and the ghost rows were not handed over).  Read wherever the host blocks on this domain's
// stream anyway -- hp_read_scalars, hp_sync (what a download or a checkpoint is followed by), the strips' batch-start
// handshake -- so that no host call sequence gets rasters of a broken exchange with HP_OK.  Blocks.
static int peer_error_check(hp_domain* d)
{
	if (!d->peer_agreed || !d->peer_mine) return HP_OK;
	uint64_t* peer_error = (uint64_t*)((char*)d->host_scalars + HOST_READBACK);
	*peer_error = 0;
	HIP_TRY(hipMemcpyAsync(peer_error, d->peer_mine + PEER_WORD_ERROR, 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (*peer_error)
		return fail(HP_ERR_HIP, "the exchange between the strips is incomplete: rank " + std::to_string((long)*peer_error - 1) +
		                        " was not heard from within the time limit (HP_PEER_TIMEOUT_MS); states and ghost rows after that point are not valid");
	return HP_OK;
}

// The sticky word of a launch's tail block that gave up waiting for a flux block (hp_kernels.hpp: launch_tail; time and timestep
// were left frozen from that launch on).  Read wherever the host blocks on the domain's stream anyway; once seen, every later call
// on the domain fails with HP_ERR_STATE (check_domain) -- its state is not a state of the model.  `queued`: the read-back has been
// queued by the caller (hp_read_scalars), only the verdict is left.
static int tail_error_queue(hp_domain* d)
{
	*(volatile double*)((char*)d->host_scalars + HOST_TAIL_ERR) = 0.0;
	HIP_TRY(hipMemcpyAsync((char*)d->host_scalars + HOST_TAIL_ERR, (char*)d->cfl_slot + (size_t)SLOT_TAIL_ERR * d->esize, d->esize,
	                       hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}
static int tail_error_verdict(hp_domain* d)
{
	const unsigned char* w = (const unsigned char*)d->host_scalars + HOST_TAIL_ERR;
	bool raised = false;
	for (size_t i = 0; i < d->esize; ++i) raised = raised || w[i] != 0;
	if (!raised) return HP_OK;
	d->tail_failed = true;
	return tail_failed_error();
}

int hp_read_scalars(hp_domain_t* d, hp_scalars_t* out)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!out) return fail(HP_ERR_INVALID, "out == NULL");
	HIP_TRY(hipMemcpyAsync(d->host_scalars, d->scalars, HOST_SCALARS_BYTES, hipMemcpyDeviceToHost, d->stream));
	if ((rc = tail_error_queue(d)) != HP_OK) return rc;
	uint64_t* peer_error = (uint64_t*)((char*)d->host_scalars + HOST_READBACK);
	*peer_error = 0;
	if (d->peer_agreed)                      // the mailboxes' sticky error word: a strip that was not heard from in time
		HIP_TRY(hipMemcpyAsync(peer_error, d->peer_mine + PEER_WORD_ERROR, 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	if ((rc = tail_error_verdict(d)) != HP_OK) return rc;
	if (*peer_error)
		return fail(HP_ERR_HIP, "the maximum over the strips is incomplete: rank " + std::to_string((long)*peer_error - 1) +
		                        " was not heard from within the time limit (HP_PEER_TIMEOUT_MS)");
	if (d->desc.precision == 8) {
		const Scalars<double>* s = (const Scalars<double>*)d->host_scalars;
		out->time = s->t; out->timestep = s->dt; out->time_hydrological = s->t_hydro; out->time_target = s->t_sync;
		out->batch_timesteps = s->batch_dt; out->batch_successful = s->batch_ok; out->batch_skipped = s->batch_skipped;
	} else {
		const Scalars<float>* s = (const Scalars<float>*)d->host_scalars;
		out->time = s->t; out->timestep = s->dt; out->time_hydrological = s->t_hydro; out->time_target = s->t_sync;
		out->batch_timesteps = s->batch_dt; out->batch_successful = s->batch_ok; out->batch_skipped = s->batch_skipped;
	}
	out->cells_calculated = d->cells_calculated;
	out->iterations = d->iterations;
	return HP_OK;
}

int hp_sync(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if ((rc = tail_error_queue(d)) != HP_OK) return rc;
	HIP_TRY(hipStreamSynchronize(d->stream));
	if ((rc = tail_error_verdict(d)) != HP_OK) return rc;                // (nor may the state of a domain whose time stands still)
	return peer_error_check(d);                                          // (a download / checkpoint of a broken exchange must not look fine)
}

int hp_is_busy(hp_domain_t* d, int* busy)
{
	if (!d || !busy) return fail(HP_ERR_INVALID, "null argument");
	hipError_t e = hipStreamQuery(d->stream);
	if (e == hipSuccess && d->stream_halo) e = hipStreamQuery(d->stream_halo);       // halo segments of a split step
	if (e == hipSuccess) {
		*busy = 0;
		// (an idle domain whose speculative batch has not been looked at yet: do that now -- the caller polls this to learn
		// whether the batch's results can be read)
		// -- and if that look re-queues the batch (the plain divisions' replay), the domain IS busy again: say so
		if (d->spec_pending) {
			hipSetDevice(d->desc.device);
			const int rc = spec_resolve(d);
			if (rc == HP_OK && hipStreamQuery(d->stream) == hipErrorNotReady) *busy = 1;
			return rc;
		}
		return HP_OK;
	}
	if (e == hipErrorNotReady) { *busy = 1; return HP_OK; }
	return fail(HP_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
}

int hp_device_ptr(hp_domain_t* d, int which, void** ptr)
{
	if (!d || !ptr) return fail(HP_ERR_INVALID, "null argument");
	d->fork_is_advance = false;          // the caller may queue work on these buffers behind the last advance_time
	if (which == HP_PTR_STATE_NEXT_SRC || which == HP_PTR_STATE_OTHER || which == HP_PTR_BED) d->facts.buffers_written_outside();  // ... or write into them
	switch (which) {
	case HP_PTR_STATE_NEXT_SRC: *ptr = d->state[d->facts->use_alt]; return HP_OK;
	case HP_PTR_STATE_OTHER:    *ptr = d->state[d->facts->use_alt ^ 1]; return HP_OK;
	case HP_PTR_BED:            *ptr = d->bed; return HP_OK;
	case HP_PTR_MANNING:        *ptr = d->manning; return HP_OK;
	case HP_PTR_CFL_MAX:        *ptr = d->cfl_slot; return HP_OK;
	case HP_PTR_SCALARS:        *ptr = d->scalars; return HP_OK;
	}
	return fail(HP_ERR_INVALID, "unknown pointer id");
}

int hp_stream(hp_domain_t* d, void** hip_stream)
{
	if (!d || !hip_stream) return fail(HP_ERR_INVALID, "null argument");
	d->fork_is_advance = false;
	*hip_stream = (void*)d->stream;
	return HP_OK;
}

int hp_set_halo_overlap(hp_domain_t* d, int on)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (d->in_step) return fail(HP_ERR_STATE, "hp_set_halo_overlap inside an iteration");
	d->halo_overlap = on != 0;
	d->halo_overlap_set = true;
	return HP_OK;
}

int hp_stream_halo(hp_domain_t* d, void** hip_stream)
{
	if (!d || !hip_stream) return fail(HP_ERR_INVALID, "null argument");
	*hip_stream = (void*)d->stream_halo;
	return HP_OK;
}

} // extern "C"

// ---- RCCL, loaded at run time: the engine has no link-time dependency on a collective library, and a process that
//      already carries one (torch bundles its own librccl, bound to its own HIP runtime) keeps using that copy ----
namespace {

int rccl_ready()
{
	return g_rccl.handle ? HP_OK : fail(HP_ERR_STATE, "no collective library loaded: call hp_comm_load first");
}
#define RCCL_TRY(expr)                                                                                 \
	do {                                                                                               \
		ncclResult_t r_ = (expr);                                                                      \
		if (r_ != ncclSuccess)                                                                         \
			return fail(HP_ERR_HIP, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "RCCL error")); \
	} while (0)


// Ghost-row exchange of the iteration in flight, queued behind the flux launches of hp_step_begin: the first / last
// `ghost_rows` owned rows of the new state go to the strip neighbours' ghost rows (CDomainLink::pullFromBuffer /
// pushToBuffer, CDomainLink.cpp:168-270; CMPIManager's block exchange, CMPIManager.cpp:555-709).
int strip_halo_exchange(hp_domain* d)
{
	const long G = d->ghost_rows, rows = d->desc.rows;
	const size_t row_elems = (size_t)d->desc.cols * 4, count = (size_t)G * row_elems;
	const ncclDataType_t type = d->desc.precision == 8 ? ncclDouble : ncclFloat;
	char* state = (char*)d->state[d->facts->use_alt ^ 1];             // the buffer the iteration in flight writes
	const size_t row_bytes = row_elems * d->esize;
	const bool south = d->comm_rank > 0, north = d->comm_rank < d->comm_world - 1;
	// the rows the neighbours need come from the halo part of the step: the transfer is ordered after that stream only
	hipStream_t xs = (d->halo_overlap && d->split_now) ? d->stream_halo : d->stream;
	if (south || north) {
		RCCL_TRY(g_rccl.GroupStart());
		if (south) {
			RCCL_TRY(g_rccl.Send(state + (size_t)G * row_bytes, count, type, d->comm_rank - 1, d->comm, xs));            // my first owned rows
			RCCL_TRY(g_rccl.Recv(state, count, type, d->comm_rank - 1, d->comm, xs));                                     // into my south ghost rows
		}
		if (north) {
			RCCL_TRY(g_rccl.Send(state + (size_t)(rows - 2 * G) * row_bytes, count, type, d->comm_rank + 1, d->comm, xs));  // my last owned rows
			RCCL_TRY(g_rccl.Recv(state + (size_t)(rows - G) * row_bytes, count, type, d->comm_rank + 1, d->comm, xs));       // into my north ghost rows
		}
		RCCL_TRY(g_rccl.GroupEnd());
		if (xs != d->stream) {
			HIP_TRY(hipEventRecord(d->ev_xchg, xs));
			HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_xchg, 0));      // hp_step_end (and the next iteration) need the rows
		}
	}
	return HP_OK;
}

template <typename T> __global__ void copy_scalar(T* to, const T* from) { *to = *from; }

// The wave-speed maximum over all strips (MPI_Allreduce(MIN dt), CMPIManager.cpp:852-861).  Whether an iteration carries a
// NEW maximum is decided from what is the same on every rank -- the scheme, quirk Q1 and the ping-pong phase, and what the
// ranks told each other at the start of the batch (does ANY of them have boundaries, or a stale maximum after an upload) --
// so either every rank enters the collective or none does, even when the host has given a boundary to one strip only.  A
// rank whose own buffer was not priced this iteration contributes the local maximum it remembers.
int strip_allreduce_max(hp_domain* d, bool first_of_batch)
{
	// (measurement knob, tools/strong_probe.py: a communicator of ONE rank normally skips the reduction; with the knob it goes
	// through it -- the library's all-reduce or its own mailbox -- so that the cost of the step can be timed on one GPU)
	if (d->comm_world <= 1 && !plan_knobs().strip_reduce_always) return HP_OK;
	if (!d->desc.dynamic_dt) {
		if (d->peer_direct) d->adv_fresh = 4;                          // fixed timestep: nothing to reduce, the round still hands the rows over
		return HP_OK;
	}
	if (!strips_reduce_everyone(plan_domain(d), d->facts, first_of_batch)) {
		if (d->adv_fresh) return fail(HP_ERR_STATE, "a strip priced a new maximum on an iteration the other ranks do not reduce "
		                                            "(boundaries or uploads changed inside a batch?)");
		if (d->peer_direct) d->adv_fresh = 4;                          // a round all the same: it is what hands the ghost rows over (PeerPush)
		return HP_OK;
	}
	const ncclDataType_t type = d->desc.precision == 8 ? ncclDouble : ncclFloat;
	if (!d->adv_fresh) {                                               // nothing new here: the remembered local maximum stands in
		if (d->desc.precision == 8) hipLaunchKernelGGL(copy_scalar<double>, dim3(1), dim3(1), 0, d->stream, (double*)d->cfl_slot, (const double*)d->cfl_slot + SLOT_LOCAL);
		else                        hipLaunchKernelGGL(copy_scalar<float>, dim3(1), dim3(1), 0, d->stream, (float*)d->cfl_slot, (const float*)d->cfl_slot + SLOT_LOCAL);
		HIP_TRY(hipGetLastError());
	}
	if (d->peer_agreed) {                                              // the advance kernel itself trades the values with the peers
		d->adv_fresh = 7;
		return HP_OK;
	}
	RCCL_TRY(g_rccl.AllReduce(d->cfl_slot, (char*)d->cfl_slot + (size_t)SLOT_GLOBAL * d->esize, 1, type, ncclMax, d->comm, d->stream));
	d->adv_fresh = 3;                                                  // advance_time: take the maximum from SLOT_GLOBAL
	return HP_OK;
}

// Start of a batch: the ranks compare notes (one 8-element all-reduce and a read-back).  Boundaries and uploads are host
// calls, which nothing forces to be the same on every rank; the ping-pong phase and the ghost-row state must be.
int strip_handshake(hp_domain* d)
{
	d->strip_any_bdy = boundaries_applied(plan_domain(d));
	d->strip_any_full = d->facts->need_full_reduce;
	d->strip_pairs = false;
	if (d->comm_world <= 1) return HP_OK;
	// (element 0 also carries the mailboxes' sticky error word of THIS rank as a value above 1: the all-reduce then tells every
	// rank that the exchange broke somewhere, and all of them fail together instead of one leaving the others in a collective)
	const bool broken = peer_error_check(d) != HP_OK;
	// (element 0: 3 = this rank's exchange is broken, 1 = it has boundary conditions, 0.5 = it has none but cannot run iteration
	// pairs, 0 = it can: the maximum over the ranks says what ALL of them may do)
	const double mine[8] = {broken ? 3.0 : (d->strip_any_bdy ? 1.0 : (strip_pairs_possible_here(plan_domain(d), d->facts, plan_knobs()) ? 0.0 : 0.5)), d->strip_any_full ? 1.0 : 0.0, (double)d->facts->use_alt, -(double)d->facts->use_alt,
	                        (double)d->facts->ghost_valid, -(double)d->facts->ghost_valid, (double)d->ghost_rows, -(double)d->ghost_rows};
	double all[8];
	char* slot = (char*)d->cfl_slot + (size_t)SLOT_HANDSHAKE * d->esize;
	const ncclDataType_t type = d->desc.precision == 8 ? ncclDouble : ncclFloat;
	// staged through the domain's pinned block (HOST_HANDSHAKE, hp_domain.hpp): an asynchronous copy
	// must not read from, or land in, this function's stack
	char* pinned = (char*)d->host_scalars + HOST_HANDSHAKE;
	HIP_TRY(hipStreamSynchronize(d->stream));                           // nothing of an earlier handshake is still in flight
	if (d->desc.precision == 8) std::memcpy(pinned, mine, sizeof mine);
	else { float* f = (float*)pinned; for (int i = 0; i < 8; ++i) f[i] = (float)mine[i]; }
	HIP_TRY(hipMemcpyAsync(slot, pinned, 8 * d->esize, hipMemcpyHostToDevice, d->stream));
	RCCL_TRY(g_rccl.AllReduce(slot, slot + 8 * d->esize, 8, type, ncclMax, d->comm, d->stream));
	HIP_TRY(hipMemcpyAsync(pinned + 128, slot + 8 * d->esize, 8 * d->esize, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (d->desc.precision == 8) std::memcpy(all, pinned + 128, sizeof all);
	else { const float* f = (const float*)(pinned + 128); for (int i = 0; i < 8; ++i) all[i] = f[i]; }
	if (all[0] > 2.0)
		return fail(HP_ERR_HIP, broken ? std::string(hp_last_error())
		                               : std::string("the exchange between the strips broke on another rank (a strip was not heard from in time)"));
	if (all[2] != -all[3]) return fail(HP_ERR_STATE, "the strips disagree on the ping-pong phase (different iteration counts?)");
	if (all[4] != -all[5] || all[6] != -all[7]) return fail(HP_ERR_STATE, "the strips disagree on their ghost rows");
	d->strip_any_bdy = all[0] >= 1.0;
	d->strip_any_full = all[1] > 0.0;
	d->strip_pairs = all[0] == 0.0;
	return HP_OK;
}

// ---- peer-written mailboxes: set-up and tear-down ----
struct PeerTicket {                     // HP_PEER_TICKET_BYTES, travels between the ranks by the host's own means
	uint64_t          magic;
	uint64_t          process;          // a number drawn once per process: same number = same address space
	uint64_t          address;          // the mailbox in its owner's address space
	int32_t           device, rank;
	hipIpcMemHandle_t handle;           // ... and for everybody else
	uint64_t          state[2];         // the two state buffers (the strip neighbours write their ghost rows), likewise
	hipIpcMemHandle_t state_handle[2];
	int64_t           rows, cols, ghost_rows, row_offset;
	int32_t           precision, state_shareable;
	unsigned char     pad[HP_PEER_TICKET_BYTES - 32 - 3 * sizeof(hipIpcMemHandle_t) - 16 - 32 - 8];
};
static_assert(sizeof(PeerTicket) == HP_PEER_TICKET_BYTES, "HP_PEER_TICKET_BYTES");
constexpr uint64_t PEER_MAGIC = 0x68702d7065657231ull;           // "hp-peer1"

uint64_t process_token()
{
	static const uint64_t token = [] {
		std::random_device rd;
		return ((uint64_t)rd() << 32) ^ (uint64_t)rd() ^ ((uint64_t)getpid() << 20);
	}();
	return token;
}

void peer_release(hp_domain* d)
{
	d->peer_agreed = false;
	if (!d->peer_mine && !d->peer_table && d->peer_mapped.empty() && !d->push_arrived) return;
	if (d->stream) hipStreamSynchronize(d->stream);
	for (void* m : d->peer_mapped) hipIpcCloseMemHandle(m);
	d->peer_mapped.clear();
	d->peer_direct = false; d->push_now = false;
	for (auto& side : d->peer_state) side[0] = side[1] = nullptr;
	if (d->push_arrived) { hipFree(d->push_arrived); d->push_arrived = nullptr; }
	if (d->peer_table) { hipFree(d->peer_table); d->peer_table = nullptr; }
	if (d->peer_mine)  { hipFree(d->peer_mine);  d->peer_mine = nullptr; }
	d->peer_world = 0; d->peer_rank = 0; d->peer_rounds = 0;
}

// one reduction of a caller-given value through the mailboxes, result and error word read back
int peer_round_now(hp_domain* d, double value, long timeout_ms, double* result, uint64_t* error)
{
	const PeerBox box = peer_box(d, true, timeout_ms);
	hipLaunchKernelGGL(peer_round, dim3(1), dim3(64), 0, d->stream, box, value);
	HIP_TRY(hipGetLastError());
	uint64_t* pinned = (uint64_t*)((char*)d->host_scalars + HOST_READBACK);
	HIP_TRY(hipMemcpyAsync(pinned, d->peer_mine + PEER_WORD_ERROR, 16, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	*error = pinned[0];
	std::memcpy(result, &pinned[1], 8);
	return HP_OK;
}
} // namespace

extern "C" {

int hp_comm_load(const char* library_path)
{
	if (g_rccl.handle) return HP_OK;
	// an explicit path is the only candidate (the caller names the copy its process already uses; silently picking
	// another one could bind a second HIP runtime); NULL = the system's
	const bool given = library_path && *library_path;
	const char* candidates[] = {given ? library_path : "librccl.so", given ? nullptr : "librccl.so.1",
	                            given ? nullptr : "/opt/rocm/lib/librccl.so"};
	void* h = nullptr;
	std::string why = "not found";
	for (const char* c : candidates) {
		if (!c || !*c) continue;
		h = dlopen(c, RTLD_NOW | RTLD_GLOBAL);
		if (h) break;
		const char* e = dlerror();           // returns the message ONCE and clears it
		if (e) why = e;
	}
	if (!h) return fail(HP_ERR_UNSUPPORTED, "cannot load the RCCL library: " + why);
	Rccl r;
	r.handle = h;
#define SYM(name) r.name = (decltype(r.name))dlsym(h, "nccl" #name); if (!r.name) { dlclose(h); return fail(HP_ERR_UNSUPPORTED, "RCCL library lacks nccl" #name); }
	SYM(GetUniqueId) SYM(CommInitRank) SYM(CommDestroy) SYM(GroupStart) SYM(GroupEnd) SYM(Send) SYM(Recv) SYM(AllReduce) SYM(GetErrorString)
#undef SYM
	r.CommCount = (decltype(r.CommCount))dlsym(h, "ncclCommCount");
	Dl_info where;
	if (dladdr((void*)r.AllReduce, &where) && where.dli_fname) r.path = where.dli_fname;
	g_rccl = r;
	return HP_OK;
}

int hp_strip_info(hp_domain_t* d, hp_strip_info_t* out)
{
	if (!out) return fail(HP_ERR_INVALID, "out == NULL");
	std::memset(out, 0, sizeof *out);
	std::snprintf(out->library, sizeof out->library, "%s", g_rccl.path.c_str());
	out->comm_ranks = -1;
	if (!d) return HP_OK;                                                // library path only
	out->comm_rank = d->comm_rank;
	out->halo_overlap = d->halo_overlap ? 1 : 0;
	out->ghost_rows = (int32_t)d->ghost_rows;
	out->peer_max = d->peer_agreed ? 1 : 0;
	out->peer_halo = d->peer_direct ? 1 : 0;
	if (d->comm && g_rccl.CommCount) {
		int n = -1;
		RCCL_TRY(g_rccl.CommCount(d->comm, &n));
		out->comm_ranks = n;                                             // what the LIBRARY says, not what the caller passed
	}
	return HP_OK;
}

int hp_comm_unique_id(void* id_out)
{
	int rc = rccl_ready();
	if (rc != HP_OK) return rc;
	if (!id_out) return fail(HP_ERR_INVALID, "id_out == NULL");
	static_assert(sizeof(ncclUniqueId) == HP_COMM_ID_BYTES, "HP_COMM_ID_BYTES");
	ncclUniqueId id;
	RCCL_TRY(g_rccl.GetUniqueId(&id));
	std::memcpy(id_out, &id, sizeof id);
	return HP_OK;
}

int hp_strip_comm_init(hp_domain_t* d, const void* id, int rank, int world)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if ((rc = rccl_ready()) != HP_OK) return rc;
	if (!id || world < 1 || rank < 0 || rank >= world) return fail(HP_ERR_INVALID, "bad communicator arguments");
	if (d->comm) return fail(HP_ERR_STATE, "the domain already has a communicator");
	// the strip's place in the global grid must agree with its rank: neighbours are rank - 1 (south) and rank + 1 (north)
	const bool has_south = d->desc.row_offset > 0, has_north = d->desc.row_offset + d->desc.rows < d->desc.global_rows;
	if (has_south != (rank > 0) || has_north != (rank < world - 1))
		return fail(HP_ERR_INVALID, "rank does not match the strip's position in the global grid");
	ncclUniqueId uid;
	std::memcpy(&uid, id, sizeof uid);
	RCCL_TRY(g_rccl.CommInitRank(&d->comm, world, uid, rank));
	d->comm_rank = rank; d->comm_world = world;
	if (!d->ev_xchg) HIP_TRY(hipEventCreateWithFlags(&d->ev_xchg, hipEventDisableTiming));
	if (!d->halo_overlap_set) d->halo_overlap = world > 1;             // default only: an explicit choice stands
	return HP_OK;
}

int hp_strip_comm_destroy(hp_domain_t* d)
{
	if (!d) return HP_OK;
	peer_release(d);
	if (d->comm) {
		hipStreamSynchronize(d->stream);
		if (d->stream_halo) hipStreamSynchronize(d->stream_halo);
		if (g_rccl.CommDestroy) g_rccl.CommDestroy(d->comm);
		d->comm = nullptr;
	}
	d->comm_world = 1; d->comm_rank = 0;
	return HP_OK;
}

// ---- the maximum over all strips without a collective: peer-written mailboxes (PeerBox, hp_kernels.hpp) ----
int hp_strip_peer_ticket(hp_domain_t* d, void* ticket_out)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!ticket_out) return fail(HP_ERR_INVALID, "ticket_out == NULL");
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	peer_release(d);
	// uncached: a peer's store must be what this device's next load sees, whichever cache it would have sat in
	void* box = nullptr;
	HIP_TRY(hipExtMallocWithFlags(&box, PEER_WORDS * sizeof(unsigned long long), hipDeviceMallocUncached));
	d->peer_mine = (unsigned long long*)box;
	HIP_TRY(hipMemsetAsync(d->peer_mine, 0xff, 2 * PEER_MAX_RANKS * sizeof(unsigned long long), d->stream));       // every word EMPTY
	HIP_TRY(hipMemsetAsync(d->peer_mine + PEER_WORD_ERROR, 0, (PEER_WORDS - PEER_WORD_ERROR) * sizeof(unsigned long long), d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));                            // ... before anybody learns where it is
	PeerTicket t;
	std::memset(&t, 0, sizeof t);
	t.magic = PEER_MAGIC; t.process = process_token(); t.address = (uint64_t)(uintptr_t)d->peer_mine;
	t.device = d->desc.device; t.rank = -1;
	if (hipIpcGetMemHandle(&t.handle, d->peer_mine) != hipSuccess) {
		(void)hipGetLastError();                                         // other processes cannot map it; ranks of THIS process still can
		std::memset(&t.handle, 0, sizeof t.handle);
	}
	t.state_shareable = 1;
	for (int b = 0; b < 2; ++b) {
		t.state[b] = (uint64_t)(uintptr_t)d->state[b];
		if (hipIpcGetMemHandle(&t.state_handle[b], d->state[b]) != hipSuccess) {
			(void)hipGetLastError();
			std::memset(&t.state_handle[b], 0, sizeof t.state_handle[b]);
			t.state_shareable = 0;
		}
	}
	t.rows = d->desc.rows; t.cols = d->desc.cols; t.ghost_rows = d->ghost_rows; t.row_offset = d->desc.row_offset;
	t.precision = d->desc.precision;
	std::memcpy(ticket_out, &t, sizeof t);
	return HP_OK;
}

int hp_strip_peer_connect(hp_domain_t* d, const void* tickets, int count, int rank, int* active)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (active) *active = 0;
	// This call is COLLECTIVE over the communicator's ranks: whatever is wrong on this rank -- arguments included -- it must
	// still reach the agreement below, or the other ranks wait in that all-reduce for ever.  A local fault
	// therefore only marks this rank's verdict as "no"; the error code is returned after the agreement.
	std::string fault;
	if (!tickets || count < 1 || count > PEER_MAX_RANKS || rank < 0 || rank >= count)
		fault = "bad mailbox arguments (1.." + std::to_string(PEER_MAX_RANKS) + " ranks)";
	else if (!d->peer_mine) fault = "hp_strip_peer_connect without hp_strip_peer_ticket";
	else if (d->comm && (count != d->comm_world || rank != d->comm_rank)) fault = "mailbox ranks do not match the communicator's";
	const PeerTicket* t = (const PeerTicket*)tickets;
	if (fault.empty() && (t[rank].magic != PEER_MAGIC || t[rank].address != (uint64_t)(uintptr_t)d->peer_mine || t[rank].process != process_token()))
		fault = "tickets[rank] is not this domain's ticket";
	if (!fault.empty() && !d->comm) return fail(HP_ERR_INVALID, fault);   // nobody to keep waiting
	if (!fault.empty()) count = 0;                                       // nothing is mapped below
	// map every peer's mailbox; a failure here is not an error of the call: the connection test below fails on every
	// rank alike (the others never hear from this one) and the run stays on the collective
	std::vector<unsigned long long*> table((size_t)(count > 0 ? count : 1), nullptr);
	bool mapped = fault.empty();
	std::string why = fault;
	for (int r = 0; r < count && mapped; ++r) {
		if (t[r].magic != PEER_MAGIC) { mapped = false; why = "ticket " + std::to_string(r) + " is not a ticket"; break; }
		if (t[r].process == process_token()) {                           // same address space (ranks as threads, or one process driving several GPUs)
			table[(size_t)r] = (unsigned long long*)(uintptr_t)t[r].address;
			if (t[r].device != d->desc.device) {
				const hipError_t e = hipDeviceEnablePeerAccess(t[r].device, 0);
				if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { mapped = false; why = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e); }
				(void)hipGetLastError();
			}
		} else {
			void* m = nullptr;
			const hipError_t e = hipIpcOpenMemHandle(&m, t[r].handle, hipIpcMemLazyEnablePeerAccess);
			if (e != hipSuccess) { (void)hipGetLastError(); mapped = false; why = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e); }
			else { d->peer_mapped.push_back(m); table[(size_t)r] = (unsigned long long*)m; }
		}
	}
	d->peer_world = count > 0 ? count : 1; d->peer_rank = fault.empty() ? rank : 0; d->peer_rounds = 0;
	// the strip neighbours' state buffers, for the ghost rows (PeerPush).  Optional on top of the mailboxes: when any rank
	// cannot have it the rows keep travelling through the collective library's send / receive
	const bool direct_wanted = !(std::getenv("HP_PEER_DIRECT") && std::atoi(std::getenv("HP_PEER_DIRECT")) == 0);
	bool direct = mapped && direct_wanted && d->comm != nullptr;
	std::string why_not_direct = direct_wanted ? "" : "switched off (HP_PEER_DIRECT=0)";
	for (int side = 0; side < 2 && direct; ++side) {
		const int r = side == 0 ? rank - 1 : rank + 1;
		if (r < 0 || r >= count) continue;
		const PeerTicket& n = t[r];
		if (n.cols != d->desc.cols || n.precision != d->desc.precision || n.ghost_rows != d->ghost_rows || d->own_hi - d->own_lo < d->ghost_rows ||
		    (side == 1 && n.row_offset != d->desc.row_offset + d->desc.rows - 2 * d->ghost_rows) ||
		    (side == 0 && n.row_offset + n.rows - 2 * d->ghost_rows != d->desc.row_offset)) {
			direct = false; why_not_direct = "rank " + std::to_string(r) + "'s strip does not adjoin this one"; break;
		}
		d->peer_rows[side] = (long)n.rows;
		for (int b = 0; b < 2 && direct; ++b) {
			if (n.process == process_token()) {
				d->peer_state[side][b] = (void*)(uintptr_t)n.state[b];
				if (n.device != d->desc.device) {
					const hipError_t e = hipDeviceEnablePeerAccess(n.device, 0);
					if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { direct = false; why_not_direct = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e); }
					(void)hipGetLastError();
				}
			} else if (!n.state_shareable) {
				direct = false; why_not_direct = "rank " + std::to_string(r) + " could not export its state buffers";
			} else {
				void* m = nullptr;
				const hipError_t e = hipIpcOpenMemHandle(&m, n.state_handle[b], hipIpcMemLazyEnablePeerAccess);
				if (e != hipSuccess) { (void)hipGetLastError(); direct = false; why_not_direct = std::string("hipIpcOpenMemHandle (state): ") + hipGetErrorString(e); }
				else { d->peer_mapped.push_back(m); d->peer_state[side][b] = m; }
			}
		}
	}
	// (from here to the agreement nothing returns early: a rank that left now would leave the others waiting in the all-reduce)
	if (direct && !d->push_arrived) {
		if (hipMalloc((void**)&d->push_arrived, 64) != hipSuccess || hipMemset(d->push_arrived, 0, 64) != hipSuccess) {
			(void)hipGetLastError();
			direct = false; why_not_direct = "no memory for the push counter";
		}
	}
	uint64_t error = 1;
	double got = 0.0;
	if (mapped && !d->peer_table && hipMalloc((void**)&d->peer_table, PEER_MAX_RANKS * sizeof(unsigned long long*)) != hipSuccess) {
		(void)hipGetLastError();
		mapped = false; why = "no memory for the mailbox table";
	}
	if (mapped && hipMemcpy(d->peer_table, table.data(), (size_t)count * sizeof(unsigned long long*), hipMemcpyHostToDevice) != hipSuccess) {
		(void)hipGetLastError();
		mapped = false; why = "mailbox table upload failed";
	}
	if (mapped) {
		// connection test: two reductions (one per mailbox set) of rank + 1 and -(rank + 1) must give `count` and -1
		const long test_ms = std::getenv("HP_PEER_TEST_MS") ? std::atol(std::getenv("HP_PEER_TEST_MS")) : 3000;
		bool ok = peer_round_now(d, (double)(rank + 1), test_ms, &got, &error) == HP_OK && error == 0 && got == (double)count;
		if (ok) ok = peer_round_now(d, -(double)(rank + 1), test_ms, &got, &error) == HP_OK && error == 0 && got == -1.0;
		if (!ok && why.empty()) why = error ? "rank " + std::to_string((long)error - 1) + " was not heard from" : "wrong maximum, or the test launch failed";
		error = ok ? 0 : 1;
	}
	if (error) log_line(HP_LOG_WARNING, "peer-written maximum not available on rank " + std::to_string(rank) + ": " + why);
	if (!error && !direct && d->comm) log_line(HP_LOG_INFORMATION, "ghost rows stay with the collective library on rank " + std::to_string(rank) + ": " + why_not_direct);
	if (d->comm) {
		// every rank must take the same road: one MAX over the ranks' verdicts through the collective library
		double verdict[2] = {error ? 1.0 : 0.0, direct ? 0.0 : 1.0};
		if (d->comm_world > 1) {
			char* slot = (char*)d->cfl_slot + (size_t)SLOT_HANDSHAKE * d->esize;
			char* pinned = (char*)d->host_scalars + HOST_HANDSHAKE;
			const ncclDataType_t type = d->desc.precision == 8 ? ncclDouble : ncclFloat;
			if (d->desc.precision == 8) std::memcpy(pinned, verdict, 16);
			else { const float v[2] = {(float)verdict[0], (float)verdict[1]}; std::memcpy(pinned, v, 8); }
			HIP_TRY(hipMemcpyAsync(slot, pinned, 2 * d->esize, hipMemcpyHostToDevice, d->stream));
			RCCL_TRY(g_rccl.AllReduce(slot, slot + 8 * d->esize, 2, type, ncclMax, d->comm, d->stream));
			HIP_TRY(hipMemcpyAsync(pinned + 128, slot + 8 * d->esize, 2 * d->esize, hipMemcpyDeviceToHost, d->stream));
			HIP_TRY(hipStreamSynchronize(d->stream));
			if (d->desc.precision == 8) std::memcpy(verdict, pinned + 128, 16);
			else { float f[2]; std::memcpy(f, pinned + 128, 8); verdict[0] = f[0]; verdict[1] = f[1]; }
		}
		d->peer_agreed = verdict[0] == 0.0;
		d->peer_direct = d->peer_agreed && verdict[1] == 0.0;
		if (active) *active = d->peer_agreed ? (d->peer_direct ? 2 : 1) : 0;
		if (!d->peer_agreed) peer_release(d);
		else if (!d->peer_direct) for (auto& side : d->peer_state) side[0] = side[1] = nullptr;
		if (!fault.empty()) return fail(HP_ERR_INVALID, fault);            // (every rank has left the agreement by now)
	} else {
		// no communicator: nothing to agree through (diagnostic use, hp_strip_peer_round); the strip loop is not touched
		if (active) *active = error ? 0 : 1;
		if (error) peer_release(d);
	}
	return HP_OK;
}

int hp_strip_peer_round(hp_domain_t* d, double value, double* max_out)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!max_out) return fail(HP_ERR_INVALID, "max_out == NULL");
	if (!d->peer_mine || !d->peer_table || d->peer_world < 1) return fail(HP_ERR_STATE, "no mailboxes connected");
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	uint64_t error = 0;
	if ((rc = peer_round_now(d, value, 0, max_out, &error)) != HP_OK) return rc;
	if (error) return fail(HP_ERR_HIP, "peer-written maximum: rank " + std::to_string((long)error - 1) + " was not heard from in time");
	return HP_OK;
}

int hp_strip_peer_disconnect(hp_domain_t* d)
{
	if (!d) return HP_OK;
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	peer_release(d);
	return HP_OK;
}

int hp_strip_step_batch(hp_domain_t* d, uint32_t n_iterations)
{
	const bool fork_ready = d && d->fork_is_advance;
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!d->comm) return fail(HP_ERR_STATE, "hp_strip_step_batch without hp_strip_comm_init");
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	if (n_iterations == 0) return HP_OK;
	const long g = stencil_reach(d->desc);
	if ((rc = strip_handshake(d)) != HP_OK) return rc;
	d->fork_is_advance = fork_ready && d->comm_world <= 1;            // (the handshake queued work behind the last advance_time)
	// (a maximum that some rank has yet to price anew -- an upload since the last batch -- keeps the ranks on single iterations
	// until the first iteration that prices on every rank has run: a decision every rank takes from the same, handshaken facts)
	bool full_pending = d->strip_any_full;
	for (uint32_t i = 0; i < n_iterations; ++i) {
		if (i + 2 <= n_iterations && d->strip_pairs && !full_pending && d->facts.strip_pair_ready(d->ghost_rows)) {
			rc = run_pair(d, true);
			if (rc != HP_OK) return rc == HP_ERR_STATE ? fail(HP_ERR_STATE, "a strip could not launch an iteration pair the ranks had agreed on") : rc;
			++i;
			d->fork_is_advance = false;
			continue;
		}
		if (d->facts->use_alt == 1) full_pending = false;  // this iteration writes the primary buffer: every rank prices it
		d->fuse_next = i + 1 < n_iterations;          // as hp_step_batch: the rows sent to the neighbours carry the rain too
		if (d->facts->ghost_valid < g) return fail(HP_ERR_STATE, "ghost rows exhausted");
		// an iteration consumes g layers of ghost rows; when fewer than g are left afterwards, the new state's rows are
		// exchanged (ghost_rows = g: every iteration; 2g: every second one, and only those iterations are split into a
		// halo and an interior launch)
		const bool exchange = d->facts->ghost_valid - g < g;
		d->split_now = exchange && !d->peer_direct;   // (rows that travel inside the advance kernel need no launch of their own)
		d->push_now = exchange && d->peer_direct;     // ... and leave with the advance kernel, or with the flux launch's tail block
		d->strip_first = i == 0;
		d->tail_allowed = true;
		rc = dispatch_begin(d);
		d->tail_allowed = false;
		if (rc != HP_OK) return rc;
		if (exchange) {
			if (!d->peer_direct && (rc = strip_halo_exchange(d)) != HP_OK) return rc;
			d->facts.ghosts_exchanged(d->ghost_rows);
		} else {
			d->facts.ghosts_consumed(g);
		}
		if ((rc = strip_allreduce_max(d, i == 0)) != HP_OK) return rc;
		if ((rc = dispatch_end(d)) != HP_OK) return rc;
		// the exchange sits between advance_time and the next flux launch on the stream graph: its event, not
		// advance_time's, is what the next halo launch may fork from only if nothing else was queued -- keep it simple
		// and let hp_step_begin record its own fork event whenever a transfer was queued on the domain's stream
		if (!d->halo_overlap || d->peer_direct) d->fork_is_advance = false;
	}
	d->fuse_next = 0;
	d->split_now = true;
	return HP_OK;
}

int hp_strip_update_timestep(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!d->comm) return fail(HP_ERR_STATE, "hp_strip_update_timestep without hp_strip_comm_init");
	if (d->in_step) return fail(HP_ERR_STATE, "inside a split step");
	// tst_Reduce over the owned rows of the primary buffer, the maximum over all strips, then tst_UpdateTimestep on every
	// rank redundantly (CSchemeGodunov.cpp:1189-1195, :1254-1260 with CMPIManager's reduction in between)
	const ncclDataType_t type = d->desc.precision == 8 ? ncclDouble : ncclFloat;
	// with the mailboxes the advance kernel WAITS for the other strips' kernels (for a bounded time): launch it only once every
	// rank's host has arrived here -- the library's all-reduce of the handshake waits without a limit, a strip still busy with
	// a long upload is no error
	if (d->peer_agreed && d->comm_world > 1 && (rc = strip_handshake(d)) != HP_OK) return rc;
	const void* priced = d->desc.scheme == HP_SCHEME_MUSCL_HANCOCK ? d->state[d->facts->use_alt] : d->state[0];  // (as hp_update_timestep)
	if (d->desc.precision == 8) {
		if (d->desc.dynamic_dt && (rc = launch_reduce<double>(d, priced, d->own_lo, d->own_hi)) != HP_OK) return rc;
	} else {
		if (d->desc.dynamic_dt && (rc = launch_reduce<float>(d, priced, d->own_lo, d->own_hi)) != HP_OK) return rc;
	}
	const bool reduced = d->desc.dynamic_dt && d->comm_world > 1, by_peers = reduced && d->peer_agreed;
	if (reduced && !by_peers)
		RCCL_TRY(g_rccl.AllReduce(d->cfl_slot, (char*)d->cfl_slot + (size_t)SLOT_GLOBAL * d->esize, 1, type, ncclMax, d->comm, d->stream));
	const int fresh = by_peers ? 7 : reduced ? 3 : 1;
	const PeerBox box = peer_box(d, by_peers);
	if (d->desc.precision == 8)
		hipLaunchKernelGGL((advance_time<true, double>), dim3(1), dim3(64), 0, d->stream, make_params<double>(d),
		                   (Scalars<double>*)d->scalars, (double*)d->cfl_slot, fresh, box, PeerPush{});
	else
		hipLaunchKernelGGL((advance_time<true, float>), dim3(1), dim3(64), 0, d->stream, make_params<float>(d),
		                   (Scalars<float>*)d->scalars, (float*)d->cfl_slot, fresh, box, PeerPush{});
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

} // extern "C"

extern "C" {

int hp_timer_start(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	HIP_TRY(hipEventRecord(d->ev_start, d->stream));
	return HP_OK;
}

int hp_timer_stop(hp_domain_t* d, float* elapsed_ms)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!elapsed_ms) return fail(HP_ERR_INVALID, "elapsed_ms == NULL");
	HIP_TRY(hipEventRecord(d->ev_stop, d->stream));
	HIP_TRY(hipEventSynchronize(d->ev_stop));
	HIP_TRY(hipEventElapsedTime(elapsed_ms, d->ev_start, d->ev_stop));
	return HP_OK;
}

int hp_kernel_timing(hp_domain_t* d, int enable_stride)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	HIP_TRY(hipStreamSynchronize(d->stream));
	constexpr size_t POOL = 16;                                          // samples per measurement: sparse on purpose
	while (enable_stride > 0 && d->timing_events.size() < POOL) {
		hipEvent_t a, b;
		HIP_TRY(hipEventCreate(&a));
		HIP_TRY(hipEventCreate(&b));
		d->timing_events.emplace_back(a, b);
	}
	// What a pair of events costs by itself (two marker packets with nothing between them): since an iteration became ONE launch
	// the step time has nothing but that launch in it, and a sample that includes the markers' own time came out ABOVE the step
	// time.  Measured here, on the idle stream, as the smallest of eight empty pairs, and taken off every sample when they are read.
	d->timing_overhead_ms = 0.0;
	if (enable_stride > 0 && !d->timing_events.empty()) {
		float best = 1e9f;
		for (int i = 0; i < 8; ++i) {
			HIP_TRY(hipEventRecord(d->timing_events[0].first, d->stream));
			HIP_TRY(hipEventRecord(d->timing_events[0].second, d->stream));
			HIP_TRY(hipEventSynchronize(d->timing_events[0].second));
			float ms = 0.f;
			HIP_TRY(hipEventElapsedTime(&ms, d->timing_events[0].first, d->timing_events[0].second));
			if (ms < best) best = ms;
		}
		d->timing_overhead_ms = best < 1e8f ? best : 0.0;
	}
	d->timing_used = 0;
	d->timing_counter = 0;
	d->timing_stride = enable_stride > 0 ? enable_stride : 0;
	return HP_OK;
}

int hp_kernel_timing_read(hp_domain_t* d, double* avg_ms, uint32_t* samples)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!avg_ms || !samples) return fail(HP_ERR_INVALID, "null argument");
	HIP_TRY(hipStreamSynchronize(d->stream));
	double total = 0.0;
	uint32_t n = 0;
	for (size_t i = 0; i < d->timing_used; ++i) {
		float ms = 0.f;
		HIP_TRY(hipEventElapsedTime(&ms, d->timing_events[i].first, d->timing_events[i].second));
		total += std::max(0.0, (double)ms - d->timing_overhead_ms);
		++n;
	}
	*avg_ms = n ? total / n : 0.0;
	*samples = n;
	return HP_OK;
}

// the last pair launch's records by tag, counted on the device (still_rec_count): window rows skipped, recorded, and the same two for the
// windows next to the edge ring alone
static int still_rec_counts(hp_domain* d, unsigned long long host_counts[4])
{
	std::fill(host_counts, host_counts + 4, 0ull);
	if (!d->still_rec || !d->still_rec_last) return HP_OK;
	const StillRec* half = (const StillRec*)d->still_rec + (size_t)d->still_rec_half * d->still_rec_slots;
	unsigned long long* counts = (unsigned long long*)((StillRec*)d->still_rec + 2 * d->still_rec_slots);
	HIP_TRY(hipMemsetAsync(counts, 0, 32, d->stream));
	hipLaunchKernelGGL(still_rec_count, dim3(256), dim3(256), 0, d->stream, half, d->still_rec_slots, counts);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(host_counts, counts, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	return HP_OK;
}

int hp_pair_wall_stats(hp_domain_t* d, uint64_t out[2])
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!out) return fail(HP_ERR_INVALID, "out == NULL");
	unsigned long long counts[4];
	if ((rc = still_rec_counts(d, counts)) != HP_OK) return rc;
	out[0] = counts[2]; out[1] = counts[3];
	return HP_OK;
}

int hp_pair_stats(hp_domain_t* d, uint64_t out[12])
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!out) return fail(HP_ERR_INVALID, "out == NULL");
	out[0] = d->pairs; out[1] = d->pair_cold_starts; out[2] = out[3] = 0;
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (tuner_on(plan_domain(d), plan_knobs()) && (rc = tuner_poll(d)) != HP_OK) return rc;
	out[4] = d->tune_samples; out[5] = d->tune_switches; out[6] = d->tune_prefer_pairs ? 1 : 0;
	out[7] = d->tune_single_ms > 0.f ? (uint64_t)(1000.0 * d->tune_pair_ms / d->tune_single_ms) : 0;
	out[8] = out[9] = out[10] = out[11] = 0;
	{                                                                     // (counted on the device, as the stamps below)
		unsigned long long host_counts[4];
		if ((rc = still_rec_counts(d, host_counts)) != HP_OK) return rc;
		out[9] = host_counts[0]; out[10] = host_counts[1];
	}
	if (d->order_buf && d->order_read) {                                  // (the half the last pair launch read: the one it did not write)
		const unsigned per_band = (unsigned)(d->order_shape[1] * (d->order_shape[2] + d->order_shape[3])), table = (unsigned)d->order_shape[0] * per_band;
		unsigned* const count = d->order_buf + 2 * (size_t)table + (size_t)d->order_shape[0] * d->order_shape[1];
		HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned), d->stream));
		hipLaunchKernelGGL(order_count, dim3(16), dim3(256), 0, d->stream, d->order_buf + (size_t)(d->order_half ^ 1) * table, (unsigned)d->order_shape[1],
		                   per_band, table, count);
		HIP_TRY(hipGetLastError());
		unsigned moved = 0;
		HIP_TRY(hipMemcpyAsync(&moved, count, sizeof moved, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(hipStreamSynchronize(d->stream));
		out[11] = moved;
	}
	if (d->haz_words) {
		unsigned long long used = 0;
		HIP_TRY(hipMemcpy(&used, d->haz_words + 2, sizeof used, hipMemcpyDeviceToHost));
		out[8] = used;
	}
	if (!d->z_state) return HP_OK;
	// (counted on the device: the records are 48 bytes a cell)
	unsigned long long* counts = d->haz_words + 4;                        // (words 4 and 5 of the 64-byte block: 0-1 the launches' words, 2 the audit)
	HIP_TRY(hipMemsetAsync(counts, 0, 16, d->stream));
	if (d->desc.precision == 8)
		hipLaunchKernelGGL((stamps_count<double>), dim3(1024), dim3(256), 0, d->stream, StampBufs<double>{(char*)d->z_state, d->haz_words}, d->pair_gen, d->cells, counts);
	else
		hipLaunchKernelGGL((stamps_count<float>), dim3(1024), dim3(256), 0, d->stream, StampBufs<float>{(char*)d->z_state, d->haz_words}, d->pair_gen, d->cells, counts);
	HIP_TRY(hipGetLastError());
	unsigned long long host_counts[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(host_counts, counts, sizeof host_counts, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	out[2] = host_counts[0]; out[3] = host_counts[1];
	return HP_OK;
}

int hp_launch_counts(hp_domain_t* d, uint64_t* flux_launches, uint64_t* with_tail)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!flux_launches || !with_tail) return fail(HP_ERR_INVALID, "null argument");
	*flux_launches = d->flux_launches;
	*with_tail = d->flux_launches_tailed;
	return HP_OK;
}

int hp_kernel_timing_overhead(hp_domain_t* d, double* overhead_ms)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!overhead_ms) return fail(HP_ERR_INVALID, "null argument");
	*overhead_ms = d->timing_overhead_ms;
	return HP_OK;
}

} // extern "C"
