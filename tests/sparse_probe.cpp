// The run planner of hp_domain_sparse (csrc/hp_sparse.hpp: sparse_plan_runs) without a GPU: the header's HIP-free part under a plain
// host compiler.  Reads cases from standard input, one a line: bytes_per_entry budget nrows row_ptr[0] ... row_ptr[nrows]; prints
// one line per case: the runs as row_lo:row_hi:first:count, separated by blanks (an empty line: no run).
// tests/test_sparse.py holds the lines to the rule; the program may also be built with -fsanitize=address,undefined.
#include "hp_sparse.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		unsigned long long bytes_per_entry, budget;
		long long nrows;
		if (!(in >> bytes_per_entry >> budget >> nrows) || nrows < 0) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
		std::vector<uint64_t> row_ptr((size_t)nrows + 1);
		for (auto& v : row_ptr) {
			unsigned long long w;
			if (!(in >> w)) { std::fprintf(stderr, "short row_ptr: %s\n", line.c_str()); return 2; }
			v = w;
		}
		const std::vector<hp::SparseRun> runs = hp::sparse_plan_runs(row_ptr.data(), nrows, bytes_per_entry, budget);
		for (size_t k = 0; k < runs.size(); ++k)
			std::printf("%s%lld:%lld:%llu:%llu", k ? " " : "", (long long)runs[k].row_lo, (long long)runs[k].row_hi,
			            (unsigned long long)runs[k].first, (unsigned long long)runs[k].count);
		std::printf("\n");
	}
	return 0;
}
