// test_heis_spin_plan.cpp -- the host planner of the one-site observables of the spin-S Heisenberg digit basis (csrc/lpp_obs_heis_spin_plan.h) in a
// stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_heis_spin_observables_host.py does).  For
// sz, splus and sminus at every site of small, odd, long and limiting sectors the plan is expanded through obs_heis_spin_source as the kernel walks
// it: every source stays inside the source sector, none is used twice, the touched count equals the closed form, and -- where the sector is small
// enough to list -- the source and the value equal those of a brute-force list of the digit words.  Prints `ok`.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "lpp_obs_heis_spin_plan.h"

using namespace lpp;
using namespace lpp::obs_host;

#define CHECK(c)                                                           \
	do {                                                                   \
		if (!(c)) {                                                        \
			std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
			std::exit(1);                                                  \
		}                                                                  \
	} while (0)

// the words of L digits 0 .. twiceS with digit sum m, ascending, by counting through all digit strings (small L only)
static std::vector<uint64_t> brute_words(int L, int twiceS, int bits, int m)
{
	std::vector<uint64_t> out;
	std::vector<int> d((size_t)L, 0);
	for (;;) {
		int s = 0;
		uint64_t w = 0;
		for (int p = 0; p < L; p++) {
			s += d[(size_t)p];
			w |= (uint64_t)d[(size_t)p] << (p * bits);
		}
		if (s == m) out.push_back(w);
		int p = 0;
		while (p < L && ++d[(size_t)p] > twiceS) d[(size_t)p++] = 0;
		if (p == L) break;
	}
	std::sort(out.begin(), out.end());
	return out;
}

static void check_sector(int L, int twiceS, int m, bool brute)
{
	const int ops[3] = { LPP_OP_SZ, LPP_OP_SPLUS, LPP_OP_SMINUS };
	for (const int op : ops) {
		for (int site = 0; site < L; site++) {
			ObsHeisSpinPlan P;
			const char* why = nullptr;
			const bool ok = obs_plan_heis_spin(op, site, LPP_SPIN_UP, L, twiceS, m, P, &why);
			if ((op == LPP_OP_SPLUS && m == L * twiceS) || (op == LPP_OP_SMINUS && m == 0)) {
				CHECK(!ok && why);
				continue;
			}
			CHECK(ok);
			CHECK(P.n_src == heis_spin_sector_size(L, twiceS, m) && P.n_dst == heis_spin_sector_size(L, twiceS, P.m2));
			CHECK(P.runs.size() >= 2 && P.runs.back().dst0 == P.n_dst && (int)P.val.size() == twiceS + 1);
			std::vector<int64_t> action((size_t)P.n_dst, -1);
			std::vector<double> coef((size_t)P.n_dst, -1.0);
			int64_t touched = -1;
			heis_spin_expand(P, action.data(), coef.data(), &touched);
			CHECK(touched == heis_spin_touched(op, L, twiceS, P.m2));
			std::vector<char> used((size_t)P.n_src, 0);
			for (int64_t i = 0; i < P.n_dst; i++) {
				const int64_t s = action[(size_t)i];
				CHECK(s >= 0 && s <= P.n_src);
				if (s == 0) continue;
				CHECK(!used[(size_t)(s - 1)]);
				used[(size_t)(s - 1)] = 1;
			}
			if (!brute) continue;
			const std::vector<uint64_t> src = brute_words(L, twiceS, P.bits, m), dst = brute_words(L, twiceS, P.bits, P.m2);
			CHECK((int64_t)src.size() == P.n_src && (int64_t)dst.size() == P.n_dst);
			std::map<uint64_t, int64_t> find;
			for (size_t i = 0; i < src.size(); i++) find[src[i]] = (int64_t)i;
			const uint64_t one = 1ull << (site * P.bits), mask = (1ull << P.bits) - 1;
			for (size_t i = 0; i < dst.size(); i++) {
				const int d = (int)((dst[i] >> (site * P.bits)) & mask);
				int64_t want = 0;
				int sd = d; // the source's digit
				if (op == LPP_OP_SPLUS && d >= 1) want = find.at(dst[i] - one) + 1, sd = d - 1;
				if (op == LPP_OP_SMINUS && d < twiceS) want = find.at(dst[i] + one) + 1, sd = d + 1;
				if (op == LPP_OP_SZ && 2 * d != twiceS) want = (int64_t)i + 1;
				CHECK(action[i] == want);
				CHECK(coef[i] == (want ? P.val[(size_t)sd] : 0.0));
			}
		}
	}
}

int main()
{
	// the sectors of tests/test_heis_spin_observables_host.py
	check_sector(5, 2, 4, true);
	check_sector(9, 2, 8, true);
	check_sector(8, 3, 12, true);
	check_sector(7, 4, 13, true);
	check_sector(5, 7, 17, true);
	check_sector(24, 2, 3, false);
	check_sector(6, 2, 0, true);
	check_sector(6, 2, 12, true);
	// one digit, one-bit digits on both sides of the cut, the widest digit the planner admits
	check_sector(1, 2, 1, true);
	check_sector(14, 1, 6, true);
	check_sector(2, 4095, 4000, false);
	// refusals: spins the assembler refuses, n / c / cdagger, a site or a sector out of range, a run table past its limit
	ObsHeisSpinPlan P;
	const char* why = nullptr;
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 0, 4, 5, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 0, 32, 2, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 0, 4, 4096, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_N, 0, 0, 6, 2, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_C, 0, 0, 6, 2, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 6, 0, 6, 2, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 2, 6, 2, 3, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 0, 6, 2, 13, P, &why));
	CHECK(!obs_plan_heis_spin(LPP_OP_SZ, 0, 0, 31, 2, 31, P, &why));
	CHECK(heis_spin_sector_size(16, 2, 16) == 5196627 && heis_spin_sector_size(18, 2, 18) == 44152809 && heis_spin_sector_size(4, 5, 3) < 0);
	std::puts("ok");
	return 0;
}
