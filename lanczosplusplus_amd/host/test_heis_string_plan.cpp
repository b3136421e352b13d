// test_heis_string_plan.cpp -- the host planner of the operator strings in the S = 1/2 Heisenberg basis (csrc/lpp_obs_heis_string_plan.h) in a
// stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_heis_many_point_host.py does).  It checks:
//   - that the composed plan of a string, expanded as the kernels walk it, IS the composition of the one-operator plans (csrc/lpp_obs_heis_plan.h)
//     through the sectors, destination by destination, on the sectors of the tests and at (40;3), where the cut of the word is at 14 bits;
//   - the invariants: every entry a source of the first sector, no source used twice, the count of heis_string_touched;
//   - what a launch uploads (heis_string_pack): one string in apply's one slot and batches of 1, 8 and 5 in the bracket kernel's 8, every slot and low
//     descriptor against its plan; a dead plan or more plans than slots is refused, nothing written;
//   - the refusals, and the planning alone of a 16-operator string at 32 sites (2^20 runs).
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lpp_obs_heis_string_plan.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

struct Op {
	int op, site, spin;
};

int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			failures++;                                                    \
		}                                                                  \
	} while (0)

const int N = LPP_OP_N, Z = LPP_OP_SZ, P_ = LPP_OP_SPLUS, M = LPP_OP_SMINUS, U = LPP_SPIN_UP, W = LPP_SPIN_DOWN;

bool plan(const std::vector<Op>& s, int L, int m, HeisStringPlan& P, const char** why)
{
	std::vector<int32_t> ops, sites, spins;
	for (const Op& o : s) {
		ops.push_back(o.op);
		sites.push_back(o.site);
		spins.push_back(o.spin);
	}
	return plan_heis_string((int)s.size(), ops.data(), sites.data(), spins.data(), L, m, P, why);
}

// the plan expanded through the run entries and the lookup function; false: the run table's limit
bool expand(const HeisStringPlan& P, int L, int m, std::vector<int64_t>& action)
{
	std::vector<ObsHeisRun> runs;
	std::vector<uint64_t> highs;
	std::vector<uint16_t> word, rank;
	std::vector<int64_t> src;
	if (!heis_string_runs(L, P.m2, true, runs, highs, word, rank)) return false;
	CHECK(runs.size() == highs.size() + 1 && runs.back().dst0 == P.n_dst);
	heis_string_sources(P, L, m, highs, src);
	for (int64_t v : src) CHECK((v < 0 ? -v : v) <= P.n_src);
	action.assign((size_t)P.n_dst, 0);
	heis_string_expand(P, runs, src, word, rank, action.data());
	return true;
}

std::vector<std::vector<Op>> strings(int L)
{
	const int lo = (L < 12 ? L : 12) - 1, hi = (12 < L - 1 ? 12 : L - 1), e = L - 1;
	std::vector<Op> twice;
	for (int k = 0; k < 8; k++) {
		twice.push_back({ P_, 0, U });
		twice.push_back({ M, 0, U });
	}
	return {
		{ { Z, 0, U }, { Z, e, U } },
		{ { P_, 0, U }, { M, hi, U } },
		{ { M, lo, U }, { P_, hi, U } },
		{ { P_, 0, U }, { M, 3, U }, { P_, hi, U }, { M, e, U } },
		{ { Z, 0, U }, { Z, 3, U }, { Z, lo, U }, { Z, e, U } },
		{ { N, 0, U }, { N, 3, W }, { N, hi, U } },
		{ { M, 3, U }, { Z, 3, U }, { P_, 3, U } },
		{ { P_, 0, U }, { P_, 0, U } }, // dead
		{ { P_, 0, U }, { Z, hi, U } }, // ends in another sector
		{ { N, 0, U }, { N, 0, W } }, // dead
		{ { P_, 0, U }, { M, 3, U }, { Z, hi, U } },
		twice, // 16 operators
		{ { M, e, U }, { N, e, W }, { Z, e, U }, { P_, e, U }, { Z, 1, U } },
	};
}

// the composed plan against the one-operator plans chained backwards from every destination; returns whether any destination is reached
bool check_string(const std::vector<Op>& s, int L, int m)
{
	HeisStringPlan P;
	const char* why = nullptr;
	CHECK(plan(s, L, m, P, &why));
	std::vector<int64_t> action;
	CHECK(expand(P, L, m, action));
	std::vector<std::vector<int64_t>> one(s.size());
	int cur = m;
	for (size_t k = 0; k < s.size(); k++) {
		ObsHeisPlan Q;
		CHECK(obs_plan_heis(s[k].op, s[k].site, s[k].spin, L, cur, Q, &why));
		one[k].assign((size_t)Q.n_dst, 0);
		heis_expand(Q, one[k].data(), nullptr);
		cur = Q.m2;
	}
	CHECK(cur == P.m2 && P.n_dst == binom(L, cur) && P.n_src == binom(L, m) && P.lb == heis_low_bits(L));
	std::vector<char> used((size_t)P.n_src, 0);
	int64_t reached = 0;
	for (int64_t d = 0; d < P.n_dst; d++) {
		int64_t at = d;
		int coef = 1;
		for (size_t k = s.size(); k-- > 0 && coef != 0;) {
			const int64_t a = one[k][(size_t)at];
			coef = a == 0 ? 0 : (a < 0 ? -coef : coef);
			at = (a < 0 ? -a : a) - 1;
		}
		const int64_t want = coef == 0 ? 0 : coef * (at + 1);
		CHECK(action[(size_t)d] == want);
		if (want != 0) {
			reached++;
			CHECK(at >= 0 && at < P.n_src && !used[(size_t)at]);
			if (at >= 0 && at < P.n_src) used[(size_t)at] = 1;
		}
	}
	CHECK(reached == heis_string_touched(P, L, m));
	CHECK(!P.dead || reached == 0);
	return reached > 0;
}

// What a launch uploads (heis_string_pack) on sector (L; m): every live string alone into the one slot apply has, on the runs of the sector it ends in,
// and 1, 8 and 5 of the strings that stay in the sector into the 8 slots of the bracket kernel -- each slot and low descriptor against the plan it came
// from, the slot expanded against the plan's own expansion; then the refusals.  Returns the number of strings that stay.
int check_pack(int L, int m)
{
	const char* why = nullptr;
	std::vector<HeisStringPlan> stay;
	HeisStringPlan dead;
	for (const auto& s : strings(L)) {
		HeisStringPlan P;
		CHECK(plan(s, L, m, P, &why));
		if (P.dead) {
			dead = P;
			continue;
		}
		std::vector<ObsHeisRun> runs;
		std::vector<uint64_t> highs;
		std::vector<uint16_t> word, rank;
		CHECK(heis_string_runs(L, P.m2, true, runs, highs, word, rank));
		std::vector<int64_t> entries(highs.size(), 77), src, got((size_t)P.n_dst, 0), want;
		ObsHeisStringLow low {};
		bool low_work = false;
		CHECK(heis_string_pack(&P, 1, L, m, highs, entries, &low, &low_work, &why));
		heis_string_sources(P, L, m, highs, src);
		CHECK(entries == src && low_work == obs_heis_string_low_work(P.low()));
		CHECK(low.flip == P.low().flip && low.need == P.low().need && low.want == P.low().want && low.zmask == P.low().zmask);
		heis_string_expand(P, runs, entries, word, rank, got.data());
		CHECK(expand(P, L, m, want) && got == want);
		if (P.m2 == m) stay.push_back(P);
	}
	CHECK(dead.dead);
	std::vector<ObsHeisRun> runs;
	std::vector<uint64_t> highs;
	std::vector<uint16_t> word, rank;
	CHECK(heis_string_runs(L, m, true, runs, highs, word, rank));
	const size_t nr = highs.size();
	std::vector<int64_t> entries(8 * nr, 77), src;
	for (int ns : { 1, 8, 5 }) {
		const std::vector<int64_t> before = entries;
		std::vector<HeisStringPlan> batch;
		for (int s = 0; s < ns; s++) batch.push_back(stay[(size_t)(s + ns) % stay.size()]);
		ObsHeisStringLow low[8] = {};
		bool low_work = false, any = false;
		CHECK(heis_string_pack(batch.data(), ns, L, m, highs, entries, low, &low_work, &why));
		for (int s = 0; s < ns; s++) {
			heis_string_sources(batch[(size_t)s], L, m, highs, src);
			CHECK(std::vector<int64_t>(entries.begin() + (std::ptrdiff_t)(s * nr), entries.begin() + (std::ptrdiff_t)((s + 1) * nr)) == src);
			CHECK(low[s].flip == batch[(size_t)s].low().flip && low[s].need == batch[(size_t)s].low().need && low[s].want == batch[(size_t)s].low().want &&
			      low[s].zmask == batch[(size_t)s].low().zmask);
			any = any || obs_heis_string_low_work(low[s]);
		}
		CHECK(low_work == any);
		CHECK(std::equal(entries.begin() + (std::ptrdiff_t)(ns * nr), entries.end(), before.begin() + (std::ptrdiff_t)(ns * nr))); // the later slots stay
	}
	// refusals: a dead plan in the batch, more plans than slots -- nothing is written
	const std::vector<int64_t> before = entries;
	ObsHeisStringLow low[9] = {};
	bool low_work = false;
	const std::vector<HeisStringPlan> with_dead { stay[0], dead }, nine(9, stay[0]);
	why = nullptr;
	CHECK(!heis_string_pack(with_dead.data(), 2, L, m, highs, entries, low, &low_work, &why) && why && entries == before);
	CHECK(!heis_string_pack(nine.data(), 9, L, m, highs, entries, low, &low_work, &why) && entries == before);
	std::vector<int64_t> one_slot(nr, 0);
	CHECK(!heis_string_pack(nine.data(), 2, L, m, highs, one_slot, low, &low_work, &why));
	return (int)stay.size();
}

} // namespace

int main()
{
	const int sectors[6][2] = { { 7, 2 }, { 7, 3 }, { 14, 7 }, { 16, 7 }, { 16, 8 }, { 18, 9 } };
	for (const auto& sec : sectors) CHECK(check_pack(sec[0], sec[1]) == 10);
	for (const auto& sec : sectors) {
		int nonzero = 0, k = 0;
		for (const auto& s : strings(sec[0])) {
			const bool any = check_string(s, sec[0], sec[1]);
			CHECK(any == (k != 7 && k != 9));
			nonzero += any && k != 8;
			k++;
		}
		CHECK(nonzero == 10);
	}
	// every single operator on a small sector, and pairs on one site: all four conditions against all four
	for (int a : { N, Z, P_, M })
		for (int sa : { U, W }) {
			check_string({ { a, 2, sa } }, 7, 3);
			for (int b : { N, Z, P_, M })
				for (int sb : { U, W }) {
					check_string({ { a, 2, sa }, { b, 2, sb } }, 7, 3);
					check_string({ { a, 13, sa }, { b, 13, sb }, { Z, 2, U } }, 14, 7);
				}
		}
	// the cut of the word at 14 bits: sites 13 | 14 straddle it
	CHECK(heis_low_bits(40) == 14);
	CHECK(check_string({ { M, 0, U }, { P_, 39, U } }, 40, 3));
	CHECK(check_string({ { Z, 13, U }, { Z, 14, U } }, 40, 3));
	CHECK(check_string({ { M, 13, U }, { P_, 14, U } }, 40, 3));
	CHECK(check_string({ { M, 13, U }, { N, 14, W }, { Z, 39, U }, { Z, 13, U } }, 40, 3));

	// 32 sites, 16 operators: planning only (6.0e8 states are not expanded)
	{
		HeisStringPlan P;
		const char* why = nullptr;
		const std::vector<Op> s { { P_, 0, U }, { M, 31, U }, { Z, 0, U }, { Z, 31, U }, { N, 12, U }, { N, 11, W }, { P_, 13, U }, { M, 20, U },
			                      { Z, 5, U }, { M, 13, U }, { P_, 20, U }, { Z, 13, U }, { M, 0, U }, { P_, 31, U }, { N, 30, W }, { Z, 30, U } };
		CHECK(s.size() == 16 && plan(s, 32, 16, P, &why) && !P.dead && P.m2 == 16 && P.lb == 12 && P.flip == 0);
		std::vector<ObsHeisRun> runs;
		std::vector<uint64_t> highs;
		std::vector<uint16_t> word, rank;
		std::vector<int64_t> src;
		CHECK(heis_string_runs(32, 16, true, runs, highs, word, rank) && highs.size() == ((size_t)1 << 20) - (size_t)(binom(20, 0) + binom(20, 1) + binom(20, 2) + binom(20, 3)) - (size_t)(binom(20, 17) + binom(20, 18) + binom(20, 19) + binom(20, 20)));
		heis_string_sources(P, 32, 16, highs, src);
		int64_t live = 0;
		for (size_t k = 0; k < src.size(); k++) {
			const int64_t a = src[k] < 0 ? -src[k] : src[k];
			CHECK(a <= P.n_src);
			if (a) {
				CHECK(a - 1 == runs[k].dst0); // no flip: the source run is the destination run
				live++;
			}
		}
		CHECK(live > 0 && heis_string_touched(P, 32, 16) == binom(32 - 7, 16 - 3));
	}

	// refusals
	{
		HeisStringPlan P;
		const char* why = nullptr;
		CHECK(!plan({ { LPP_OP_C, 0, U } }, 7, 3, P, &why) && why);
		CHECK(!plan({ { Z, 0, U }, { LPP_OP_CDAGGER, 1, U } }, 7, 3, P, &why));
		CHECK(!plan({ { LPP_OP_IDENTITY, 0, U } }, 7, 3, P, &why));
		CHECK(!plan({ { Z, 7, U } }, 7, 3, P, &why));
		CHECK(!plan({ { Z, -1, U } }, 7, 3, P, &why));
		CHECK(!plan({ { Z, 0, 2 } }, 7, 3, P, &why));
		CHECK(!plan({ { Z, 0, U } }, 7, 8, P, &why));
		CHECK(!plan({ { Z, 0, U } }, 63, 3, P, &why));
		CHECK(!plan({}, 7, 3, P, &why));
		CHECK(!plan(std::vector<Op>(17, Op { Z, 0, U }), 7, 3, P, &why));
		CHECK(!plan({ { P_, 0, U } }, 4, 4, P, &why));
		CHECK(!plan({ { M, 0, U } }, 4, 0, P, &why));
		CHECK(plan({ { M, 0, U } }, 4, 1, P, &why) && P.m2 == 0);
		CHECK(!plan({ { M, 0, U }, { M, 1, U } }, 4, 1, P, &why)); // at the second step
		CHECK(!plan({ { P_, 0, U }, { P_, 0, U } }, 4, 3, P, &why)); // a dead string still walks the sectors
		CHECK(plan({ { P_, 0, U }, { P_, 0, U } }, 4, 2, P, &why) && P.dead && P.m2 == 4);
	}
	if (failures) return 1;
	std::printf("ok\n");
	return 0;
}
