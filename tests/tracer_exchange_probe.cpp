// A tracer species' exchange with the bed (csrc/hp_tracer.hpp: tracer_exchange, validate_tracer_exchange; csrc/hp_crmath.h: hp_cr_cbrt)
// without a GPU: the header under a plain host compiler, the very definitions the kernel tracer_step_set<T, true> and
// hp_tracer_set_exchange use.
// Reads cases from standard input, one a line, every double as the 16 hexadecimal digits of its bit pattern:
//     C x                                                       -> hp_cr_cbrt(x)
//     X M D h qx qy n dt settling tau_deposit tau_erode erodibility
//                                                              -> "M D" after step 7
//     V struct_size species species_count settling tau_deposit tau_erode erodibility  cells n_deposit deposit...
//                                                              -> "ok" or "bad <message>"  (struct_size 0 stands for the right one,
//                                                                  "null" for the whole line for a NULL descriptor)
// tests/test_tracer_exchange.py holds the results to frontend.cbrt_exact and frontend.Tracer(exchange=...) bit for bit.
#include "hp_tracer.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static double from_bits(const std::string& s)
{
	const unsigned long long u = std::stoull(s, nullptr, 16);
	double v;
	std::memcpy(&v, &u, 8);
	return v;
}
static unsigned long long bits(const double v)
{
	unsigned long long u;
	std::memcpy(&u, &v, 8);
	return u;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string what, w;
		if (!(in >> what)) continue;
		if (what == "C") {
			in >> w;
			if (!in) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			std::printf("%016llx\n", bits(hp_cr_cbrt(from_bits(w))));
		} else if (what == "X") {
			double v[11];
			for (double& x : v) { in >> w; x = from_bits(w); }
			if (!in) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			const hp::TracerPair out = hp::tracer_exchange(v[0], v[1], v[2], v[3], v[4], v[5], v[6], hp::TracerExchangeParams{v[7], v[8], v[9], v[10]});
			std::printf("%016llx %016llx\n", bits(out.M), bits(out.D));
		} else if (what == "V") {
			std::string first, why;
			in >> first;
			if (first == "null") {
				const bool ok = hp::validate_tracer_exchange(nullptr, 1, 0, why);
				std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
				continue;
			}
			hp_tracer_exchange_desc_t desc;
			unsigned species_count;
			unsigned long long cells, n_deposit;
			desc.struct_size = (uint32_t)std::stoul(first);
			if (desc.struct_size == 0) desc.struct_size = sizeof desc;
			in >> desc.species >> species_count;
			double q[4];
			for (double& x : q) { in >> w; x = from_bits(w); }
			desc.settling = q[0]; desc.tau_deposit = q[1]; desc.tau_erode = q[2]; desc.erodibility = q[3];
			in >> cells >> n_deposit;
			std::vector<double> deposit(n_deposit);
			for (double& x : deposit) { in >> w; x = from_bits(w); }
			if (!in || (n_deposit && n_deposit != cells)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
			desc.deposit_initial = deposit.empty() ? nullptr : deposit.data();
			const bool ok = hp::validate_tracer_exchange(&desc, species_count, cells, why);
			std::printf("%s\n", ok ? "ok" : ("bad " + why).c_str());
		} else { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
	}
	return 0;
}
