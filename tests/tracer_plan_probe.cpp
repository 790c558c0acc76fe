// The launch rules (csrc/hp_plan.hpp) for a domain with a tracer, without a GPU: over every combination of the fields and switches
// that decide between iteration pairs, single iterations and speculative batches, a PlanDomain with tracer_on never pairs and never
// speculates -- and the same domain without it does both somewhere, so the clause is what holds them off.
// Prints: checked <n> traced_pairs <n> traced_spec <n> plain_pairs <n> plain_spec <n>
#include "hp_plan.hpp"

#include <cstdio>

int main()
{
	using namespace hp;
	unsigned long checked = 0, traced_pairs = 0, traced_spec = 0, plain_pairs = 0, plain_spec = 0;
	for (int traced = 0; traced < 2; ++traced)
	for (int math = 0; math < 2; ++math)
	for (int precision = 4; precision <= 8; precision += 4)
	for (int kernel = 0; kernel < 2; ++kernel)
	for (int bdy = 0; bdy < 3; ++bdy)                      // none, fusable area boundaries, a list that is not fusable
	for (int two_step = -1; two_step <= 1; ++two_step)
	for (int pays = 0; pays < 2; ++pays)
	for (int speculate = 0; speculate < 2; ++speculate)
	for (uint32_t n = 1; n <= 64; n *= 8) {
		PlanDomain d;
		d.scheme = HP_SCHEME_GODUNOV;
		d.kernel = kernel ? HP_KERNEL_BASIC : HP_KERNEL_AUTO;
		d.math_mode = math ? HP_MATH_STRICT : HP_MATH_FAST;
		d.precision = precision;
		d.rows = d.cols = d.global_rows = 4096;
		d.cells = (size_t)d.rows * (size_t)d.cols;
		d.has_bdy = bdy != 0;
		d.fusable = bdy == 1 && !traced;                   // (refresh_fusable: a traced domain is never fusable)
		d.tail_allowed = true;
		d.march2_pays = pays != 0;
		d.tracer_on = traced != 0;
		PlanKnobs k;
		k.two_step = two_step;
		k.strict_speculate = speculate != 0;
		BufferFacts facts;                                 // (the facts as ready for a pair as they get)
		facts.maximum_priced();
		facts.edge_ring_priced();
		const bool pairs = pairs_possible_common(d, k) || pairs_possible(d, k) || strip_pairs_possible_here(d, facts, k) || pair_eligible(d, facts, k);
		const bool spec = spec_wanted(d, k, n);
		++checked;
		if (traced) { traced_pairs += pairs; traced_spec += spec; }
		else { plain_pairs += pairs; plain_spec += spec; }
	}
	std::printf("checked %lu traced_pairs %lu traced_spec %lu plain_pairs %lu plain_spec %lu\n", checked, traced_pairs, traced_spec, plain_pairs, plain_spec);
	return 0;
}
