// hp_checkpoint.hpp -- what a store of a domain keeps about its share of a checkpoint (hp_state_save / hp_state_restore): the peak
// tracker, the two record logs, the moving bed, the links' records, the infiltration's F, the open boundary's records and the tracer's M
// each have one SaveMark, and all but the logs a device copy next to it (SaveSlot, hp_domain.hpp).  Every store counts in an epoch of its
// own the calls that make an older checkpoint none of its (added, cleared, enabled, disabled, reset).  What a stale store does is
// its own affair (hp_observers.hpp, hp_actors.hpp).  Host logic only -- no HIP header --, as hp_facts.hpp: tests/checkpoint_probe.cpp
// replays event sequences for tests/test_checkpoint.py without a GPU.
#pragma once
#include <cstdint>

namespace hp {
namespace {

enum class Verdict { NOTHING, BRING_BACK, STALE };       // no checkpoint; the store's own; taken before the store's last change of epoch

struct SaveMark {
	bool     taken = false;           // a checkpoint exists (of a store that was on, or off or empty: then nothing was copied) ...
	uint64_t epoch = 0;               // ... of this epoch of the store
	uint64_t count = 0;               // what comes back with the copy: the peaks' and the logs' samples, the tracer's iterations
	uint64_t room = 0;                // units the device copy holds (0: there is none)

	// hp_state_save, before it touches anything: must the copy be allocated?  One rule for the copies of a fixed size (the same request
	// every time: allocated once) and for those that grow with their store; a store that is off or empty asks for 0 units
	bool needs_room(const uint64_t units) const { return units > room; }
	void got_room(const uint64_t units) { room = units; }
	void lost_room() { room = 0; }                        // the copy is freed; what the mark says of the checkpoint stays
	void take(const uint64_t store_epoch, const uint64_t store_count = 0) { taken = true; epoch = store_epoch; count = store_count; }
	void drop() { taken = false; }                        // the peaks and the logs while off: they keep no mark
	Verdict verdict(const uint64_t store_epoch) const { return !taken ? Verdict::NOTHING : epoch == store_epoch ? Verdict::BRING_BACK : Verdict::STALE; }
	// the store's struct is reset and its copy freed (hp_bed_shapes_clear): that there was a checkpoint, and of which epoch, survives
	SaveMark carried() const { SaveMark m; m.taken = taken; m.epoch = epoch; return m; }
};

} // namespace
} // namespace hp
