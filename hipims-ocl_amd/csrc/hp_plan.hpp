// hp_plan.hpp -- what the next launch is: the host-side rules of hp_engine.hip that decide between iteration pairs and single iterations,
// which buffer a launch prices, whether it carries its own tail block, whether the strips reduce.  Each rule is a pure function of a flat
// snapshot of the domain (PlanDomain: hp_engine.hip's plan_domain fills one where a rule is evaluated), the buffer facts (hp_facts.hpp)
// and the once-per-process switches as values (PlanKnobs: hp_engine.hip's plan_knobs is the one place that names their environment
// variables).  Host logic only -- no HIP header, no getenv --, so that a plain C++17 translation unit can include it:
// tests/plan_probe.cpp answers decision requests for tests/test_plan.py without a GPU.  (Internal linkage, as all of hp_domain.hpp: the
// library exports nothing of it.)
#pragma once
#include "../../include/hipims_mi.h"
#include "hp_facts.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hp {
namespace {

constexpr unsigned TAIL_MAX_BLOCKS = 65536;    // words allocated per domain (LaunchTail::done)
constexpr uint32_t SPEC_MIN = 8;               // iterations from which a STRICT fp64 batch may run speculatively (spec_wanted)

// The once-per-process switches, as the environment leaves them when nothing is set (-1: not forced either way).
struct PlanKnobs {
	int      two_step = -1;                    // HP_TWO_STEP: 0 no pairs, 1 pairs wherever eligible, unset: where march2_pays
	bool     launch_tail = true;               // HP_LAUNCH_TAIL=0: every iteration keeps its advance launch (and nothing pairs)
	bool     strip_reduce_always = false;      // HP_STRIP_REDUCE_ALWAYS: a communicator of ONE rank goes through the reduction too
	bool     pair_bdy = true;                  // HP_PAIR_BDY=0: domains with area boundaries stay on single iterations
	bool     pair_strict = true;               // HP_PAIR_STRICT=0: the exact mode does not pair
	int      pair_exact = -1;                  // HP_PAIR_EXACT: 1 every pair keeps quirk Q3 exact, 0 none
	bool     pair_skip = true;                 // HP_PAIR_SKIP=0: no still records, nothing skipped
	bool     pair_wall = true;                 // HP_PAIR_WALL=0: still water beside the edge ring marches (pair_wall_runs)
	bool     fill_after_pairs = true;          // HP_FILL_AFTER_PAIRS=0: the device copy instead of K1's FILL flag
	bool     strict_speculate = false;         // HP_STRICT_SPECULATE=1: speculative STRICT fp64 batches
	bool     pair_tune = true;                 // HP_PAIR_TUNE=0: the exact mode always pairs where eligible
	int      sweep_alternate = -1;             // HP_SWEEP_ALTERNATE: 0 / 1 forces the alternating sweep direction
	unsigned tail_max_blocks = TAIL_MAX_BLOCKS;        // HP_TAIL_MAX_BLOCKS (a knob for A/B runs; 768 = one round of blocks)
	unsigned tail_max_blocks_k2k6 = TAIL_MAX_BLOCKS;   // HP_TAIL_MAX_BLOCKS_K2K6
	bool     march2_rseg_forced = false;       // HP_MARCH2_RSEG is set at all (pair_tile_rows: no STRICT 12-row cap then)
	bool     fuse_bdy = true;                  // HP_FUSE_BDY=0: no area boundary is carried by the flux kernel (hp_actors.hpp: refresh_fusable_t)
};

// What the rules read from a domain, as it is when the rule is evaluated.
struct PlanDomain {
	int      scheme = HP_SCHEME_GODUNOV, kernel = HP_KERNEL_AUTO, math_mode = HP_MATH_FAST, precision = 8, dynamic_dt = 1;
	unsigned quirks = HP_QUIRKS_REFERENCE;
	long     rows = 0, cols = 0;
	size_t   cells = 0;
	long     row_offset = 0, global_rows = 0, ghost_rows = 1;
	bool     has_bdy = false;                  // the boundary list is not empty
	bool     fusable = false, bdy_on_ring = false;
	bool     bdy_removes_water = false;        // an area boundary with a loss rate or a mass flux (pair_exact)
	bool     has_comm = false;
	int      comm_world = 1;
	bool     peer_direct = false, peer_mine = false;
	bool     has_tail_words = true, tail_allowed = false, halo_overlap = false, split_now = true;
	bool     strip_any_bdy = false, strip_first = false, strip_any_full = false;
	bool     spec_now = false;
	bool     has_stamps = false;               // the stamps' buffers exist (z_state)
	bool     march2_pays = false;              // hp_tiling.hpp: the pair launch is at least two rounds of blocks at 12-row tiles
	bool     has_links = false, soil_on = false, tracer_on = false, open_on = false;
	bool     spec_fused_kept = false;          // the library was built with -DHP_KEEP_SPEC_FUSED
};

inline bool reads_primary(const PlanDomain& d) { return (d.quirks & HP_QUIRK_CFL_READS_PRIMARY) != 0; }           // quirk Q1
inline bool basic_godunov(const PlanDomain& d) { return d.kernel == HP_KERNEL_BASIC && d.scheme == HP_SCHEME_GODUNOV; }
// the stand-alone boundary pass runs in front of the flux launch: MUSCL never applies them (Q8)
inline bool boundaries_applied(const PlanDomain& d) { return d.has_bdy && d.scheme != HP_SCHEME_MUSCL_HANCOCK; }

// `limit` of make_tail: launches of more blocks keep the advance launch.
inline unsigned tail_limit(const PlanKnobs& k) { return k.tail_max_blocks < TAIL_MAX_BLOCKS ? k.tail_max_blocks : TAIL_MAX_BLOCKS; }
// (K2 / K6 have their own knob for A/B runs.  A first probe had them lose 0.5 / 1.7 % at the 4608 blocks of 4096^2 and a limit of
// two rounds of blocks was set; bench.py's interleaved repeats on one box then showed the opposite -- MUSCL-Hancock 4096^2
// 0.311 -> 0.302 ms, fp32 0.215 -> 0.192, inertial 0.268 -> 0.249-0.263 -- so there is no limit of their own any more)
inline unsigned tail_limit_k2k6(const PlanKnobs& k) { return std::min(tail_limit(k), k.tail_max_blocks_k2k6); }
// The launch's own tail block (LaunchTail, hp_kernels.hpp): 0 (no tail), 1 (tail block) or 2 (tail block + rows stored into the
// strip neighbours).  `tail_want`: this iteration qualifies (plan_single, run_pair_t); `part_all`, `own_stream`: one launch over all
// rows on the domain's stream; `push_now`: this iteration's ghost rows leave with it.
inline int tail_kind_for(const bool tail_want, const bool part_all, const bool own_stream, const unsigned blocks, const unsigned limit, const bool push_now)
{
	if (!(tail_want && part_all && own_stream && blocks <= limit)) return 0;
	return push_now ? 2 : 1;
}

// Alternating sweep direction.  A launch leaves the last ~250 MiB it loaded or stored in the Infinity Cache (256 MiB, stores
// allocate: MI355X_MICROARCH.md), and what it stored last is the top of every row band -- exactly what the NEXT launch, which reads
// the state this one wrote, would reach last.  Every other whole-domain launch therefore visits each band's tiles from the top down
// (TileMap::flip: the same tiles mirrored within the band): it starts on rows whose new state and bed may still be on the die.  Pure
// scheduling: which wavefront solves a face never changes its bits.  Measured (profiles/r04zv_sweep_alternate_again.txt,
// r04zw_sweep_alternate_f64.txt; same box, interleaved): fp32, whose launch is 0.6 GB: S-DAM 4096^2 +5 %, S-RAIN +2.5 %, S-ROUGH
// +3 %, MUSCL +2.3 %, 8192^2 +0.7 %; fp64 MUSCL +2.5 % on the dam break, +0.5 % on live water; fp64 Godunov and inertial: 0 to -3 %
// (2048^2, 16384 x 1026, 16384 x 8192) and erratic at 4096^2 and 8192^2.  Box-dependent: a third box showed no difference at all
// for fp32 (0.1290 / 0.1300 / 0.1291 ms).  So: on for fp32 and for fp64 MUSCL, where it was never behind; off for fp64 Godunov /
// inertial; HP_SWEEP_ALTERNATE=0 / 1 forces it.
inline bool sweep_alternates(const PlanDomain& d, const PlanKnobs& k)
{
	if (k.sweep_alternate >= 0) return k.sweep_alternate != 0;
	return d.precision == 4 || d.scheme == HP_SCHEME_MUSCL_HANCOCK;
}

// ---- two iterations per pass (hp_kernels.hpp: godunov_march2) -------------------------------------------------------------------
// A pair is two consecutive iterations (k reads the primary buffer, k + 1 writes it) of a batch on a single domain run by ONE
// launch.  Eligible: Godunov scheme, tuned kernel, FAST arithmetic, no boundary conditions (they act between the two iterations),
// no strips, the reference's reduction quirk Q1 on (it is what makes the second timestep known in advance), the remembered maximum
// valid, the launch's own tail block available (it advances the time twice), and the next iteration reads the primary buffer.
// HP_TWO_STEP=0 switches it off, =1 forces it on wherever it is eligible; default: grids whose launch is at least two rounds of
// blocks at 12-row tiles (choose_tiling: march2_pays -- below that the extra halo rows and the shorter tiles cost more than the
// bytes save: 1024^2 and the 4096 x 514 strip lose 3-5 %, 2048^2 gains 13 %, 4096^2 22 %, profiles/r05n_two_step.txt).
// (the part of the test that does not change from one iteration to the next: this domain's batches are made of pairs wherever two
// iterations are to be had)
inline bool pairs_possible_common(const PlanDomain& d, const PlanKnobs& k)
{
	const int mode = k.two_step;
	if (mode == 0 || (mode < 0 && !d.march2_pays)) return false;
	// boundary conditions: none, or area boundaries the flux kernel can carry itself (`fusable`: uniform / coarse gridded ones; round 6) --
	// the pair kernel applies them between its two steps and prices the state it stores with and without the next iteration's
	// (godunov_march2, BDY); single domains only.  HP_PAIR_BDY=0 keeps such domains on single iterations (A/B runs).
	// (fp32: from 30 M cells on -- S-RAIN 4096^2 fp32 LOSES 3 % in pairs, 0.1436 -> 0.1478 ms, where fp64 gains 7.5 % and 8192^2 gains 8-9 %
	// in both precisions: profiles/r06w_srain_pairs_by_size.txt; with five waves per SIMD, the final binary: level at 16.8 M and 25 M cells,
	// +5 % at 37.7 M, +13 % at 67 M: profiles/r06ah_f32_bdy_pairs_by_size.txt; HP_TWO_STEP=1 overrides)
	const bool bdy_size_ok = d.precision == 8 || d.cells >= 30000000 || mode > 0;
	const bool bdy_ok = !d.has_bdy || (k.pair_bdy && bdy_size_ok && d.fusable && !d.has_comm && d.comm_world <= 1 && d.dynamic_dt);
	// STRICT (round 6): the same statements in the same order as K1's, so the pair is the same computation there too -- always with
	// the stamps (the exact mode promises the reference's bits); no boundaries, single domains, dynamic timestep.  What it is for: rows
	// of still water are a copy in STRICT (K1's skip), and a pair copies them at half the bytes.  HP_PAIR_STRICT=0 switches it off.
	const bool math_ok = d.math_mode == HP_MATH_FAST ||
	                     (k.pair_strict && !d.has_bdy && !d.has_comm && d.comm_world <= 1 && d.dynamic_dt && !d.spec_now);
	// never with a tracer: its step stands between every two iterations, as a link group's or an infiltration's does (those are entries of
	// the boundary list and so never fusable; the tracer is none, so it is named here)
	return d.scheme == HP_SCHEME_GODUNOV && d.kernel != HP_KERNEL_BASIC && math_ok && !d.tracer_on &&
	       bdy_ok && (!d.dynamic_dt || reads_primary(d)) &&
	       k.launch_tail && d.has_tail_words && d.rows >= 5 && d.cols >= 5;
}
inline bool pairs_possible(const PlanDomain& d, const PlanKnobs& k)          // a single domain
{
	return pairs_possible_common(d, k) && !d.has_comm && d.comm_world <= 1 && !d.peer_mine && d.row_offset == 0 &&
	       d.global_rows == d.rows;
}
inline bool pair_eligible(const PlanDomain& d, const BufferFacts& facts, const PlanKnobs& k)
{
	return pairs_possible(d, k) && facts.pair_ready(d.dynamic_dt != 0);
}
// A ROW STRIP runs pairs where it stores two reaches of ghost rows (one exchange per two iterations anyway) and the strips write
// their rows into each other themselves (transport level 2: the pair's tail block holds the one mailbox round, which is the
// hand-over).  What THIS rank can do goes into the batch's handshake (strip_handshake); the ranks pair up only if all of them can.
inline bool strip_pairs_possible_here(const PlanDomain& d, const BufferFacts& facts, const PlanKnobs& k)
{
	return pairs_possible_common(d, k) && d.has_comm && d.comm_world > 1 && d.peer_direct && d.ghost_rows == 2 && !facts->rings_differ;
}
// Which pairs keep quirk Q3 exact (godunov_march2's HZ instantiation: 4-9 % slower): HP_PAIR_EXACT=1 all of them, =0 none; default: the
// domains whose area boundaries can REMOVE water -- a loss rate, a mass flux -- where whole regions dry at once and sit untouched, with
// stale values in the reference's other buffer, for as long as they stay dry.
inline bool pair_exact(const PlanDomain& d, const PlanKnobs& k)
{
	if (d.math_mode == HP_MATH_STRICT) return true;
	if (k.pair_exact >= 0) return k.pair_exact != 0;
	return d.bdy_removes_water;
}
// (STRICT: 12-row tiles -- its live tiles cost 1300 instructions per row and stage, and a 24-row one is what the launch waits for at its
// end: S-DAM 4096^2 0.275 ms per iteration at 24 rows, 0.2645 at 12, 0.281 at 8; profiles/r06i_strict_pair_tile_sweep.txt)
inline int pair_tile_rows(const PlanDomain& d, const PlanKnobs& k, const int march2_rseg)
{
	return (d.math_mode == HP_MATH_STRICT && !k.march2_rseg_forced) ? std::min(march2_rseg, 12) : march2_rseg;
}
// still records: the instantiations that take still runs on a single domain (FAST fp64, no area boundaries, no stamps) -- this launch
// writes the half the launch before did not, and reads that one if nothing has written a state buffer since (still_rec_valid).
// `exact`: this launch stamps (pair_exact, and the stamps' buffers exist); `tile_rows`: pair_tile_rows.
inline bool pair_records(const PlanDomain& d, const PlanKnobs& k, const bool strip, const bool exact, const int tile_rows)
{
	return d.precision == 8 && k.pair_skip && !strip && !d.has_bdy && !exact && d.math_mode != HP_MATH_STRICT && tile_rows <= 32;
}
// ... and among those launches, whether windows next to the edge ring take their still water in runs and skip it (hp_kernels.hpp: wall_ok):
// part of the records, so HP_PAIR_SKIP=0 switches it off with them; HP_PAIR_WALL=0 switches off this part alone.
inline bool pair_wall_runs(const PlanKnobs& k, const bool records) { return records && k.pair_wall; }

// after iteration pairs the non-current buffer is out of date; K1 brings it up to date by itself (its FILL flag: every cell of the
// launch's rows is stored), any other kernel gets the device copy first
// (exact pairs: the device copy, then the stamps on top -- repair_other_buffer -- so that K1 needs no knowledge of them)
inline bool fill_wanted(const PlanDomain& d, const BufferFacts& facts, const PlanKnobs& k)
{
	return k.fill_after_pairs && facts->other_stale && d.scheme == HP_SCHEME_GODUNOV && d.kernel != HP_KERNEL_BASIC && !(pair_exact(d, k) && d.has_stamps);
}

// A batch of at least SPEC_MIN iterations on a single STRICT fp64 domain runs speculatively (hp_engine.hip: spec_begin).
inline bool spec_wanted(const PlanDomain& d, const PlanKnobs& k, const uint32_t n)
{
	// OPT-IN (HP_STRICT_SPECULATE=1).  Measured with the rigorous flag (profiles/r04j_strict_lines_*): the Godunov kernel gains 2-3 %
	// (S-DAM 4096^2 0.490 -> 0.479 ms, S-RAIN 0.716 -> 0.697), the MUSCL-Hancock kernel LOSES 9-13 % (0.580 -> 0.657, 1.069 -> 1.164):
	// the denominator-side v_div_scale + compare that make the detection exact cost most of what the shared reciprocal saves
	// (without any detection the same kernels run at 0.426 / 0.657 / 0.518 / 0.926 ms).  Not worth a snapshot per batch by default.
	// Not with FUSED area boundaries (round 5).  The speculative flavour of the fused kernel with its own tail block is the engine's
	// largest instantiation -- 168 VGPRs with 58-66 of them spilled and 103-114 spilled SGPRs -- and what the compiler made of it
	// stopped being the plain kernel's arithmetic when an unrelated flag was added to the kernel (deterministic, relative 1e-7 ...
	// 1e-4, no word raised; the same source built for two waves per SIMD, without the vector spills, is exact again:
	// profiles/r05fg_spec_fused_tail_miscompare.txt).  A 2-3 % experiment is not worth an instantiation that only holds while the
	// register allocator is lucky: such domains run the plain STRICT kernels.
	const bool fusable_ok = d.spec_fused_kept || !d.fusable;
	// Never with link groups: the batch that is queued again after a raised word would count their records twice.  Nor with an
	// infiltration: it would add to F twice.  Nor with a tracer: it would move M twice.  Nor with an open boundary: it would add to its
	// records' volume twice.
	return k.strict_speculate && n >= SPEC_MIN && d.math_mode == HP_MATH_STRICT && d.precision == 8 && !d.has_comm && fusable_ok && !d.has_links && !d.soil_on && !d.tracer_on &&
	       !d.open_on &&
	       d.kernel != HP_KERNEL_BASIC && (d.scheme == HP_SCHEME_GODUNOV || d.scheme == HP_SCHEME_MUSCL_HANCOCK);
}
// The exact mode chooses between pairs and single iterations by measurement (hp_engine.hip: run_iterations, tuner_poll).
// HP_PAIR_TUNE=0: always pairs where eligible; not where HP_TWO_STEP=1 has forced them.
inline bool tuner_on(const PlanDomain& d, const PlanKnobs& k)
{
	return k.pair_tune && d.math_mode == HP_MATH_STRICT && k.two_step != 1;
}

// The wave-speed maximum over all strips: do ALL ranks reduce on this iteration?  Decided from what is the same on every rank -- the
// scheme, quirk Q1 and the ping-pong phase, and what the ranks told each other at the start of the batch (does ANY of them have
// boundaries, or a stale maximum after an upload) -- so either every rank enters the collective or none does, even when the host has
// given a boundary to one strip only.  One copy of the rule for its two readers -- strip_allreduce_max, which enters the collective, and
// plan_single, which decides whether the launch's tail block can stand in for it: were they ever to differ, the ranks would deadlock.
inline bool strips_reduce_everyone(const PlanDomain& d, const BufferFacts& facts, const bool first_of_batch)
{
	const bool dst_is_primary = facts->use_alt == 1;
	return d.dynamic_dt && (d.scheme == HP_SCHEME_MUSCL_HANCOCK || !reads_primary(d) || dst_is_primary || basic_godunov(d) || d.strip_any_bdy ||
	                        (first_of_batch && d.strip_any_full));
}

// What a single iteration's flux launch is told, and what follows it (step_begin_impl).
struct SinglePlan {
	int  cfl_mode = 0;                      // the fused epilogue prices: 0 nothing, 1 what lands in dst, 2 the source (= primary) buffer
	bool reprice_ring = false;              // the edge ring's maxima are priced anew in front of the launch
	bool reduce_after = false;              // a stand-alone reduction follows the launch
	bool tail_want = false;                 // the launch may carry its own tail block, if it is small enough (tail_kind_for)
	int  tail_fresh = 0;                    // ... and this is what its advance would be told
	int  edge_buffer = 0;                   // ring of the buffer that is priced: mode 1 -> dst, mode 2 -> src (= primary)
	bool reduce_buffer_is_primary = false;  // the stand-alone reduction reads state[0] (Q1), not what the iteration wrote
};
inline SinglePlan plan_single(const PlanDomain& d, const BufferFacts& facts, const PlanKnobs& k)
{
	SinglePlan s;
	const bool has_bdy = boundaries_applied(d);
	// Which buffer does the CFL reduction price?  Q1: always the primary one (CSchemeGodunov.cpp:1629/:1634);
	// otherwise what this iteration writes.
	const bool q1 = reads_primary(d);
	const bool muscl = d.scheme == HP_SCHEME_MUSCL_HANCOCK;
	const bool basic = basic_godunov(d);
	const bool dst_is_primary = facts->use_alt == 1;
	if (d.dynamic_dt && !basic) {
		// MUSCL-Hancock has ONE state buffer in the reference (updated in place), so its reduction always sees
		// the new state: here that is dst, whichever physical buffer it is
		if (muscl || !q1 || dst_is_primary) s.cfl_mode = 1; // price what lands in dst
		else if (has_bdy)          s.cfl_mode = 2;         // primary = source, changed in place by the boundaries
		else                       s.cfl_mode = 0;         // primary untouched: last maximum still holds
		// the ring maxima are cached from the last upload -- unless a cell boundary rewrites ring cells in place
		// (bdy_cell accepts any cell; tst_Reduce re-reads every cell each iteration, CLDynamicTimestep.clc:166-249)
		s.reprice_ring = s.cfl_mode != 0 && (facts->edge_dirty || (has_bdy && d.bdy_on_ring));
	}
	s.edge_buffer = s.cfl_mode == 1 ? (facts->use_alt ^ 1) : s.cfl_mode == 2 ? facts->use_alt : 0;
	// The launch's own tail block instead of a separate advance launch (LaunchTail): inside a batch call, the tuned Godunov
	// kernel, one launch over all rows, nothing between the flux launch and the advance (no stand-alone reduction), and
	// either no reduction over strips at all or the strips' own transport in its plain shape (no rank with boundaries or a
	// stale maximum: those iterations pass remembered maxima around, which stays with the advance launch).
	s.reduce_after = d.dynamic_dt && s.cfl_mode == 0 && (basic || facts->need_full_reduce);
	s.reduce_buffer_is_primary = q1;
	const int priced = (d.dynamic_dt && s.cfl_mode != 0) ? 1 : 0;
	// strips: the ranks reduce on the iterations strip_allreduce_max says (strips_reduce_everyone); the tail block serves the two plain
	// shapes -- this rank priced and everyone reduces, or nobody does -- and leaves the rest (a rank that passes its
	// REMEMBERED maximum around: boundaries or a stale maximum somewhere else) to the advance launch
	bool strips_ok = d.comm_world <= 1 ? !(d.has_comm && k.strip_reduce_always) : d.peer_direct;
	int fresh = priced;
	if (d.comm_world > 1 && d.peer_direct) {
		const bool everyone = strips_reduce_everyone(d, facts, d.strip_first);
		strips_ok = (priced != 0) == everyone;
		fresh = everyone ? 7 : 4;
	}
	s.tail_want = k.launch_tail && d.tail_allowed && !basic && !s.reduce_after && strips_ok &&
	              !(d.halo_overlap && d.split_now) && d.has_tail_words;
	s.tail_fresh = fresh;
	return s;
}

} // namespace
} // namespace hp
