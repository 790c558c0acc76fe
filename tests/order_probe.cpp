// order_probe.cpp -- hp_order.hpp under a host compiler (tests/test_order.py).
//   order_probe sweep           every groups 1..20, nseg 1..23 and flag mask (all masks up to 10 groups, 200 seeded ones above), and one
//                               64-group case: checks each table against the order's definition and prints {"cases": n, "bad": [...]}
//   order_probe tables < lines  "groups nseg mask" per line: prints that table, one line of "g:seg" words each
#include "hp_order.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace hp;

// What the table must be, built the long way round: the flagged groups' tiles tile-row by tile-row, then the others'.
static std::vector<unsigned> expected(const unsigned groups, const unsigned nseg, const unsigned long long mask)
{
	std::vector<unsigned> flagged, others;
	for (unsigned g = 0; g < groups; ++g) ((mask >> g) & 1ull ? flagged : others).push_back(g);
	if (flagged.empty() || others.empty()) { flagged.clear(); others.clear(); for (unsigned g = 0; g < groups; ++g) flagged.push_back(g); }
	std::vector<unsigned> t;
	for (const std::vector<unsigned>* cls : {&flagged, &others})
		for (unsigned seg = 0; seg < nseg; ++seg)
			for (const unsigned g : *cls) t.push_back(order_pack(g, seg));
	return t;
}

static const char* check(const unsigned groups, const unsigned nseg, const unsigned long long mask)
{
	const unsigned n = groups * nseg;
	const unsigned long long all = groups >= 64 ? ~0ull : ((1ull << groups) - 1ull);
	const std::vector<unsigned> want = expected(groups, nseg, mask);
	std::vector<char> seen(n, 0);
	bool left_flagged = false;
	std::vector<unsigned> by_columns(n + 2, 0xdeadbeefu);                          // (a word in front and one behind: nothing is written there)
	for (unsigned k = 0; k < groups; ++k) order_fill_group(groups, nseg, mask, k, by_columns.data() + 1);
	if (by_columns[0] != 0xdeadbeefu || by_columns[n + 1] != 0xdeadbeefu) return "order_fill_group wrote outside the table";
	for (unsigned i = 0; i < n; ++i) if (by_columns[i + 1] != want[i]) return "order_fill_group: not the defined order";
	for (unsigned i = 0; i < n; ++i) {
		const unsigned e = order_entry(groups, nseg, mask, i), g = order_g(e), seg = order_seg(e);
		if (g >= groups || seg >= nseg) return "a word that is no tile";
		if (seen[g * nseg + seg]++) return "a tile twice";                      // n positions, n tiles, none twice: a bijection
		const bool f = ((mask >> g) & 1ull) != 0;
		if (!f) left_flagged = true;
		else if (left_flagged && (mask & all) != all) return "a flagged tile behind an unflagged one";
		if (e != want[i]) return "not the defined order";
		if (((mask & all) == 0 || (mask & all) == all) && !order_is_identity(groups, i, e)) return "no hint, yet not tile-row by tile-row";
		if (order_is_identity(groups, i, e) != (g == i % groups && seg == i / groups)) return "order_is_identity";
	}
	return nullptr;
}

int main(int argc, char** argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "tables")) {
		unsigned groups, nseg;
		unsigned long long mask;
		while (std::scanf("%u %u %llu", &groups, &nseg, &mask) == 3) {
			for (unsigned i = 0; i < groups * nseg; ++i) {
				const unsigned e = order_entry(groups, nseg, mask, i);
				std::printf("%s%u:%u", i ? " " : "", order_g(e), order_seg(e));
			}
			std::printf("\n");
		}
		return 0;
	}
	unsigned long long cases = 0, seed = 0x9e3779b97f4a7c15ull;
	std::string bad;
	auto run = [&](const unsigned groups, const unsigned nseg, const unsigned long long mask) {
		++cases;
		if (const char* why = check(groups, nseg, mask)) {
			char line[160];
			std::snprintf(line, sizeof line, "%s\"groups %u nseg %u mask %llu: %s\"", bad.empty() ? "" : ", ", groups, nseg, mask, why);
			if (bad.size() < 2000) bad += line;
		}
	};
	auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed ^ (seed >> 29); };
	for (unsigned groups = 1; groups <= 20; ++groups)
		for (unsigned nseg = 1; nseg <= 23; ++nseg) {
			if (groups <= 10) for (unsigned long long m = 0; m < (1ull << groups); ++m) run(groups, nseg, m);
			else {
				run(groups, nseg, 0); run(groups, nseg, (1ull << groups) - 1ull);
				for (int k = 0; k < 200; ++k) run(groups, nseg, next());            // (bits beyond the groups are to be ignored)
			}
		}
	for (const unsigned long long m : {0ull, ~0ull, 1ull << 63, ~(1ull << 63), 0x00000000ffff0000ull, next(), next()}) run(64, 7, m);
	std::printf("{\"cases\": %llu, \"bad\": [%s]}\n", cases, bad.c_str());
	return 0;
}
