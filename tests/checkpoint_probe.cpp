// Probe of hp_checkpoint.hpp for tests/test_checkpoint.py: plain C++17, no HIP.  Reads one line per event from stdin -- `needs_room N`
// (the answer; where it is yes the copy is had, as slot_reserve does: got_room N), `lost_room`, `take EPOCH COUNT`, `drop`,
// `verdict EPOCH`, `carry` (the mark becomes its carried() self); `new` starts over with a fresh mark and prints nothing -- and prints
// the mark and the event's answer (-1: it has none; verdicts: 0 nothing, 1 bring back, 2 stale) after each, as name=value pairs on one line.
#include "hp_checkpoint.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace hp;

int main()
{
	SaveMark mark;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string ev;
		unsigned long long a[2] = {0, 0};
		if (!(in >> ev)) continue;
		for (unsigned long long& v : a) in >> v;
		int answer = -1;
		if (ev == "new") { mark = SaveMark(); continue; }
		else if (ev == "needs_room") { answer = mark.needs_room(a[0]) ? 1 : 0; if (answer) mark.got_room(a[0]); }
		else if (ev == "lost_room") mark.lost_room();
		else if (ev == "take") mark.take(a[0], a[1]);
		else if (ev == "drop") mark.drop();
		else if (ev == "verdict") answer = mark.verdict(a[0]) == Verdict::NOTHING ? 0 : mark.verdict(a[0]) == Verdict::BRING_BACK ? 1 : 2;
		else if (ev == "carry") mark = mark.carried();
		else {
			std::fprintf(stderr, "checkpoint_probe: unknown event %s\n", ev.c_str());
			return 2;
		}
		std::printf("taken=%d epoch=%llu count=%llu room=%llu answer=%d\n", (int)mark.taken, (unsigned long long)mark.epoch, (unsigned long long)mark.count,
		            (unsigned long long)mark.room, answer);
		std::fflush(stdout);
	}
	return 0;
}
