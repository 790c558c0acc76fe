// Probe of hp_plan.hpp for tests/test_plan.py: plain C++17, no HIP.  Reads one decision request per line from stdin -- name=value
// fields, integers: the knobs as k.<name>, the facts as f.<name>, a rule's own arguments as a.<name>, everything else a PlanDomain
// field; what is not named is a created domain's (96 x 64 cells, a single domain, nothing uploaded yet) under an empty environment --
// and prints every rule's answer to it as name=value pairs on one line.
#include "hp_plan.hpp"

#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <type_traits>

using namespace hp;

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::map<std::string, long long> in;
		std::istringstream words(line);
		std::string w;
		while (words >> w) {
			const size_t eq = w.find('=');
			if (eq == std::string::npos) { std::fprintf(stderr, "plan_probe: not name=value: %s\n", w.c_str()); return 2; }
			in[w.substr(0, eq)] = std::stoll(w.substr(eq + 1));
		}
		auto take = [&](const char* name, auto& field) {
			auto it = in.find(name);
			if (it == in.end()) return false;
			field = (std::decay_t<decltype(field)>)it->second;
			in.erase(it);
			return true;
		};
		PlanKnobs k;
		take("k.two_step", k.two_step); take("k.launch_tail", k.launch_tail); take("k.strip_reduce_always", k.strip_reduce_always);
		take("k.pair_bdy", k.pair_bdy); take("k.pair_strict", k.pair_strict); take("k.pair_exact", k.pair_exact); take("k.pair_skip", k.pair_skip);
		take("k.fill_after_pairs", k.fill_after_pairs); take("k.strict_speculate", k.strict_speculate); take("k.pair_tune", k.pair_tune);
		take("k.sweep_alternate", k.sweep_alternate); take("k.tail_max_blocks", k.tail_max_blocks); take("k.tail_max_blocks_k2k6", k.tail_max_blocks_k2k6);
		take("k.march2_rseg_forced", k.march2_rseg_forced); take("k.fuse_bdy", k.fuse_bdy);
		PlanDomain d;
		d.rows = 64; d.cols = 96;
		take("scheme", d.scheme); take("kernel", d.kernel); take("math_mode", d.math_mode); take("precision", d.precision); take("dynamic_dt", d.dynamic_dt);
		take("quirks", d.quirks); take("rows", d.rows); take("cols", d.cols);
		if (!take("cells", d.cells)) d.cells = (size_t)d.rows * (size_t)d.cols;
		take("row_offset", d.row_offset);
		if (!take("global_rows", d.global_rows)) d.global_rows = d.rows;
		take("ghost_rows", d.ghost_rows);
		take("has_bdy", d.has_bdy); take("fusable", d.fusable); take("bdy_on_ring", d.bdy_on_ring); take("bdy_removes_water", d.bdy_removes_water);
		take("has_comm", d.has_comm); take("comm_world", d.comm_world); take("peer_direct", d.peer_direct); take("peer_mine", d.peer_mine);
		take("has_tail_words", d.has_tail_words); take("tail_allowed", d.tail_allowed); take("halo_overlap", d.halo_overlap); take("split_now", d.split_now);
		take("strip_any_bdy", d.strip_any_bdy); take("strip_first", d.strip_first); take("strip_any_full", d.strip_any_full);
		take("spec_now", d.spec_now); take("has_stamps", d.has_stamps); take("march2_pays", d.march2_pays);
		take("has_links", d.has_links); take("soil_on", d.soil_on); take("spec_fused_kept", d.spec_fused_kept);
		// the facts, reached the only way there is: by the events that leave them so
		int use_alt = 0;
		bool need_full_reduce = true, edge_dirty = true, rings_differ = false, other_stale = false;
		take("f.use_alt", use_alt); take("f.need_full_reduce", need_full_reduce); take("f.edge_dirty", edge_dirty);
		take("f.rings_differ", rings_differ); take("f.other_stale", other_stale);
		BufferFacts facts;
		if (rings_differ) facts.rows_uploaded();
		if (!need_full_reduce) facts.maximum_priced();
		if (!edge_dirty) facts.edge_ring_priced();
		if (use_alt) facts.single_ended();
		if (other_stale) facts.pair_ran(false, 0);
		if (facts->use_alt != use_alt || facts->need_full_reduce != need_full_reduce || facts->edge_dirty != edge_dirty ||
		    facts->rings_differ != rings_differ || facts->other_stale != other_stale) {
			std::fprintf(stderr, "plan_probe: the facts asked for were not reached\n");
			return 2;
		}
		long n = 8, march2_rseg = 24, tile_rows = 24, blocks = 100;
		bool first_of_batch = false, strip = false, exact = false, tail_want = true, part_all = true, own_stream = true, push_now = false;
		take("a.n", n); take("a.march2_rseg", march2_rseg); take("a.tile_rows", tile_rows); take("a.blocks", blocks);
		take("a.first_of_batch", first_of_batch); take("a.strip", strip); take("a.exact", exact); take("a.tail_want", tail_want);
		take("a.part_all", part_all); take("a.own_stream", own_stream); take("a.push_now", push_now);
		if (!in.empty()) { std::fprintf(stderr, "plan_probe: unknown field %s\n", in.begin()->first.c_str()); return 2; }

		const SinglePlan s = plan_single(d, facts, k);
		std::printf("pairs_possible_common=%d pairs_possible=%d strip_pairs_possible_here=%d pair_eligible=%d pair_exact=%d pair_records=%d "
		            "pair_tile_rows=%d fill_wanted=%d spec_wanted=%d tuner_on=%d sweep_alternates=%d strips_reduce_everyone=%d boundaries_applied=%d "
		            "cfl_mode=%d reprice_ring=%d reduce_after=%d tail_want=%d tail_fresh=%d edge_buffer=%d reduce_buffer_is_primary=%d "
		            "tail_kind=%d tail_kind_k2k6=%d tail_limit=%u tail_limit_k2k6=%u\n",
		            (int)pairs_possible_common(d, k), (int)pairs_possible(d, k), (int)strip_pairs_possible_here(d, facts, k), (int)pair_eligible(d, facts, k),
		            (int)pair_exact(d, k), (int)pair_records(d, k, strip, exact, (int)tile_rows), pair_tile_rows(d, k, (int)march2_rseg),
		            (int)fill_wanted(d, facts, k), (int)spec_wanted(d, k, (uint32_t)n), (int)tuner_on(d, k), (int)sweep_alternates(d, k),
		            (int)strips_reduce_everyone(d, facts, first_of_batch), (int)boundaries_applied(d),
		            s.cfl_mode, (int)s.reprice_ring, (int)s.reduce_after, (int)s.tail_want, s.tail_fresh, s.edge_buffer, (int)s.reduce_buffer_is_primary,
		            tail_kind_for(tail_want, part_all, own_stream, (unsigned)blocks, tail_limit(k), push_now),
		            tail_kind_for(tail_want, part_all, own_stream, (unsigned)blocks, tail_limit_k2k6(k), push_now), tail_limit(k), tail_limit_k2k6(k));
	}
	std::fflush(stdout);
	return 0;
}
