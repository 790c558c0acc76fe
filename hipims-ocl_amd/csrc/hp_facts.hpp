// hp_facts.hpp -- what the host knows, between launches, about the two state buffers and the CFL slot block of a domain: ten facts,
// the copy a checkpoint keeps of them and the copy in front of a speculative batch.  hp_engine.hip reads the facts through
// `d->facts->name` and changes them only by saying what happened to the device: one event per kind of happening, each with the
// reason for what it does.  Host logic only -- no HIP header, no getenv --, so that a plain C++17 translation unit can include it:
// tests/facts_probe.cpp replays event sequences for tests/test_facts.py without a GPU.  (Internal linkage, as all of hp_domain.hpp:
// the library exports nothing of it.)
#pragma once
#include <cassert>

namespace hp {
namespace {

struct Facts {
	int  use_alt = 0;                 // the buffer the next iteration reads (bUseAlternateKernel): state[use_alt]
	bool need_full_reduce = true;     // the remembered maximum is stale (upload / link import)
	bool edge_dirty = true;           // edge-ring maxima must be re-priced
	bool rings_differ = false;        // a partial state upload went into ONE buffer: the edge rings of the two may differ -- no iteration
	                                  // pairs until the next full upload (pair_ready)
	bool rings_checked = false;       // ... and have been compared since (rings_really_differ): the flag is a fact, not a maybe
	bool other_stale = false;         // pairs (godunov_march2) ran since the non-current state buffer last held a state the single-iteration
	                                  // kernels can build on
	bool m1_valid = false;            // area boundaries: cfl_slot[SLOT_M1] prices the primary buffer with the next iteration's boundaries
	                                  // (left by the last pair)
	bool pair_fused_next = false;     // the last pair stored its state with the next iteration's boundaries applied (SLOT_BDY = 1)
	bool still_rec_valid = false;     // no writer of either state buffer (or the bed) has run since the last pair launch that wrote still records
	long ghost_valid = 0;             // ghost rows per interior side that currently hold their owners' values
};

class BufferFacts {
	Facts f, at_save, at_spec;
public:
	const Facts* operator->() const { return &f; }        // read-only: `d->facts->use_alt = 1` does not compile
	const Facts& saved() const { return at_save; }        // (hp_state_restore needs the checkpoint's buffer order before it restores)

	// ---- what the host calls do --------------------------------------------------------------------------------------------------
	// slot[SLOT_M1] prices the primary buffer under the boundary set and the bed of its time: a change of either voids the figure a
	// checkpoint holds as well -- a restore brings the slot block back, but neither the boundary list nor the bed.  (Every upload
	// counts, Manning's too; the calls say so before they look at their arguments: one that fails has still forgotten.)
	void boundaries_or_bed_changed() { f.m1_valid = false; at_save.m1_valid = false; }
	// a new time, target time or timestep: the next pair with area boundaries starts cold (pair_cold_start).  The checkpoint's figure
	// stays -- it comes back together with the time it was priced for.  ODD: hp_domain_upload_rows says this, not the event above,
	// so a checkpoint keeps its figure across a partial upload where a full upload voids it.
	void time_control_changed() { f.m1_valid = false; }
	// something other than a recording pair launch writes, or may write, a state buffer or the bed (or Manning's n): uploads, restore,
	// a replay, single iterations and their FILL, the stand-alone boundary passes, the repair copy, a device pointer handed out, and
	// the records' own reallocation -- the still records describe what is no longer there
	void buffers_written_outside() { f.still_rec_valid = false; }
	// both buffers hold the host's array (`ghost_rows`: strips are uploaded with all their ghost rows).  ODD: rings_checked stays
	// as it is -- it is read only while rings_differ holds, and rows_uploaded clears it
	void full_state_uploaded(const long ghost_rows)
	{
		f.other_stale = false; f.rings_differ = false; f.use_alt = 0;
		f.need_full_reduce = f.edge_dirty = true;
		f.ghost_valid = ghost_rows;
	}
	void bed_uploaded() { f.need_full_reduce = f.edge_dirty = true; }
	// queueWritePartial goes to the CURRENT buffer only: the two buffers' edge rings may differ from here on
	void rows_uploaded() { f.need_full_reduce = f.edge_dirty = true; f.rings_differ = true; f.rings_checked = false; }
	// rings_really_differ has looked, once per run of partial uploads: block-wise loads of a whole grid leave the rings equal
	void rings_compared(const bool equal) { f.rings_checked = true; if (equal) f.rings_differ = false; }

	// ---- what the iterations do --------------------------------------------------------------------------------------------------
	void edge_ring_priced() { f.edge_dirty = false; }
	void maximum_priced() { f.need_full_reduce = false; }
	// a single iteration prices one maximum, not the pair kernel's two: the next pair starts cold (run_single, hp_step_begin; a strip's
	// loop does not say it -- strips carry no area boundaries in pairs).  Its writes are dispatch_begin's buffers_written_outside.
	void single_begins() { f.m1_valid = false; }
	// the non-current buffer is up to date again: K1's FILL launch stored every cell, or repair_other_buffer copied
	void other_made_current() { f.other_stale = false; }
	void single_ended() { f.use_alt ^= 1; }               // Threaded_runBatch :1300
	// the stand-alone boundary pass and reduction have left the figure a pair with area boundaries needs from its predecessor
	void cold_started() { f.m1_valid = true; }
	// One pair launch says three things, at three points of run_pair_t, and they stay apart: between them lie the two early returns of
	// a failing hipGetLastError and a failing hipEventRecord, behind which the flags were always left exactly so.
	// The launch is queued: with area boundaries it leaves SLOT_M1 for its successor, and when `followed` by another iteration of
	// the batch its state with that iteration's boundaries applied ...
	void pair_queued(const bool bdy, const bool followed) { f.pair_fused_next = bdy && followed; f.m1_valid = bdy; }
	// ... and went out without an error: it wrote still records, or voided them ...
	void pair_launched(const bool recs) { f.still_rec_valid = recs; }
	// ... and the engine has swapped the buffers (use_alt stays 0): the one the pair read is two iterations old; a strip's launch
	// held the exchange
	void pair_ran(const bool strip, const long ghost_rows) { f.other_stale = true; if (strip) f.ghost_valid = ghost_rows; }
	void ghosts_consumed(const long g) { f.ghost_valid -= g; }                    // a strip's iteration without an exchange behind it
	void ghosts_exchanged(const long ghost_rows) { f.ghost_valid = ghost_rows; }  // ... with one; a new domain's start

	// ---- checkpoint and speculative batch ----------------------------------------------------------------------------------------
	// Both are taken with the other buffer repaired, between batches (asserted: both callers run repair_other_buffer first).  A
	// checkpoint keeps use_alt, need_full_reduce, edge_dirty, rings_differ, m1_valid and ghost_valid; the snapshot of a speculative
	// batch use_alt, need_full_reduce, edge_dirty and ghost_valid.  The other fields of the two copies are never written or read.
	void checkpoint_taken()
	{
		assert(!f.other_stale);
		at_save.use_alt = f.use_alt; at_save.need_full_reduce = f.need_full_reduce; at_save.edge_dirty = f.edge_dirty;
		at_save.rings_differ = f.rings_differ; at_save.m1_valid = f.m1_valid; at_save.ghost_valid = f.ghost_valid;
	}
	// the buffers, their phase and the slot block are the checkpoint's again; a bed or state upload since the save has left its own
	// marks, and they stay.  The rings are compared anew, nothing fused is in the buffer.  (The still records went when the first copy
	// was queued -- buffers_written_outside --, here and in a replay: a copy that fails has still written.)
	void checkpoint_restored()
	{
		f.use_alt = at_save.use_alt; f.rings_differ = at_save.rings_differ; f.m1_valid = at_save.m1_valid; f.ghost_valid = at_save.ghost_valid;
		f.other_stale = false; f.rings_checked = false; f.pair_fused_next = false;
		f.need_full_reduce = f.need_full_reduce || at_save.need_full_reduce;
		f.edge_dirty = f.edge_dirty || at_save.edge_dirty;
	}
	void spec_taken()
	{
		assert(!f.other_stale);
		at_spec.use_alt = f.use_alt; at_spec.need_full_reduce = f.need_full_reduce; at_spec.edge_dirty = f.edge_dirty;
		at_spec.ghost_valid = f.ghost_valid;
	}
	// ODD: fewer fields than a restore brings back.  The batch in between ran single iterations only and took no upload: the rings'
	// facts, other_stale and pair_fused_next are what they were, and m1_valid is down either way
	void spec_replayed()
	{
		f.use_alt = at_spec.use_alt; f.need_full_reduce = at_spec.need_full_reduce; f.edge_dirty = at_spec.edge_dirty;
		f.ghost_valid = at_spec.ghost_valid;
	}

	// ---- what the facts allow ----------------------------------------------------------------------------------------------------
	// (not after a PARTIAL upload -- rings_differ, until the next full one: single iterations read the OTHER buffer's ring on every
	// second iteration while a pair carries the primary buffer's through both steps: next to ring cells that matter hydraulically --
	// an edge without walls -- the two part.)  A pair reads the primary buffer, and with a dynamic timestep the remembered maxima hold.
	bool pair_ready(const bool dynamic_dt) const
	{
		return f.use_alt == 0 && !f.rings_differ && (!dynamic_dt || (!f.need_full_reduce && !f.edge_dirty));
	}
	// a strip's pair consumes both reaches of ghost rows
	bool strip_pair_ready(const long ghost_rows) const { return f.use_alt == 0 && f.ghost_valid == ghost_rows; }
};

} // namespace
} // namespace hp
