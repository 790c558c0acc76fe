// Probe of hp_facts.hpp for tests/test_facts.py: plain C++17, no HIP.  Reads one line per event from stdin -- the event's name as in
// BufferFacts, then its arguments as integers; `new` starts over with a fresh BufferFacts and prints nothing -- and prints the facts,
// the six a checkpoint keeps, and the two predicates after each event, as name=value pairs on one line.
#include "hp_facts.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace hp;

int main()
{
	BufferFacts facts;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string ev;
		long a[3] = {0, 0, 0};
		if (!(in >> ev)) continue;
		for (long& v : a) in >> v;
		if (ev == "new") { facts = BufferFacts(); continue; }
		else if (ev == "boundaries_or_bed_changed") facts.boundaries_or_bed_changed();
		else if (ev == "time_control_changed") facts.time_control_changed();
		else if (ev == "buffers_written_outside") facts.buffers_written_outside();
		else if (ev == "full_state_uploaded") facts.full_state_uploaded(a[0]);
		else if (ev == "bed_uploaded") facts.bed_uploaded();
		else if (ev == "rows_uploaded") facts.rows_uploaded();
		else if (ev == "rings_compared") facts.rings_compared(a[0] != 0);
		else if (ev == "edge_ring_priced") facts.edge_ring_priced();
		else if (ev == "maximum_priced") facts.maximum_priced();
		else if (ev == "single_begins") facts.single_begins();
		else if (ev == "other_made_current") facts.other_made_current();
		else if (ev == "single_ended") facts.single_ended();
		else if (ev == "cold_started") facts.cold_started();
		else if (ev == "pair_queued") facts.pair_queued(a[0] != 0, a[1] != 0);
		else if (ev == "pair_launched") facts.pair_launched(a[0] != 0);
		else if (ev == "pair_ran") facts.pair_ran(a[0] != 0, a[1]);
		else if (ev == "ghosts_consumed") facts.ghosts_consumed(a[0]);
		else if (ev == "ghosts_exchanged") facts.ghosts_exchanged(a[0]);
		else if (ev == "checkpoint_taken") facts.checkpoint_taken();
		else if (ev == "checkpoint_restored") facts.checkpoint_restored();
		else if (ev == "spec_taken") facts.spec_taken();
		else if (ev == "spec_replayed") facts.spec_replayed();
		else {
			std::fprintf(stderr, "facts_probe: unknown event %s\n", ev.c_str());
			return 2;
		}
		const Facts& s = facts.saved();
		std::printf("use_alt=%d need_full_reduce=%d edge_dirty=%d rings_differ=%d rings_checked=%d other_stale=%d m1_valid=%d pair_fused_next=%d "
		            "still_rec_valid=%d ghost_valid=%ld saved.use_alt=%d saved.need_full_reduce=%d saved.edge_dirty=%d saved.rings_differ=%d "
		            "saved.m1_valid=%d saved.ghost_valid=%ld pair_ready.fixed=%d pair_ready.dynamic=%d strip_pair_ready.2=%d\n",
		            facts->use_alt, (int)facts->need_full_reduce, (int)facts->edge_dirty, (int)facts->rings_differ, (int)facts->rings_checked,
		            (int)facts->other_stale, (int)facts->m1_valid, (int)facts->pair_fused_next, (int)facts->still_rec_valid, facts->ghost_valid,
		            s.use_alt, (int)s.need_full_reduce, (int)s.edge_dirty, (int)s.rings_differ, (int)s.m1_valid, s.ghost_valid,
		            (int)facts.pair_ready(false), (int)facts.pair_ready(true), (int)facts.strip_pair_ready(2));
		std::fflush(stdout);
	}
	return 0;
}
