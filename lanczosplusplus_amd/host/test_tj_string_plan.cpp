// test_tj_string_plan.cpp -- the host planner of the operator strings in the one-orbital t-J basis (csrc/lpp_obs_tj_string_plan.h) in a stand-alone
// program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_tj_many_point_host.py does).  It checks:
//   - that the composed plan of a string, expanded as the kernels walk it, IS the composition of the one-operator plans (csrc/lpp_obs_tj_plan.h:
//     obs_plan_tj + tj_expand) through the sectors, destination by destination;
//   - the invariants: every entry a source of the first sector, no source used twice, the closed-form count of tj_string_touched;
//   - what a launch uploads (TjStringImage): one string in apply's one slot and batches of 1, 8 and 5 in the bracket kernel's 8, every slot against its
//     plan; a plan of another sector, a dead plan or an over-full batch is refused, nothing copied;
//   - the refusals, and the planning alone of a 16-operator string at 30 sites.
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lpp_obs_tj_string_plan.h"

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

const int C_ = LPP_OP_C, D_ = LPP_OP_CDAGGER, N = LPP_OP_N, Z = LPP_OP_SZ, P_ = LPP_OP_SPLUS, M = LPP_OP_SMINUS, U = LPP_SPIN_UP, W = LPP_SPIN_DOWN;

bool plan(const std::vector<Op>& s, int L, int nup, int ndn, TjStringPlan& P, const char** why)
{
	std::vector<int32_t> ops, sites, spins;
	for (const Op& o : s) {
		ops.push_back(o.op);
		sites.push_back(o.site);
		spins.push_back(o.spin);
	}
	return obs_string_plan_tj((int)s.size(), ops.data(), sites.data(), spins.data(), L, nup, ndn, P, why);
}

// the 15 strings of the tests on L sites
std::vector<std::vector<Op>> strings(int L)
{
	const int e = L - 1, h = L / 2;
	std::vector<Op> twice;
	for (int k = 0; k < 8; k++) {
		twice.push_back({ C_, 1, U });
		twice.push_back({ D_, 1, U });
	}
	return {
		{ { N, 0, U }, { N, e, W } },
		{ { Z, 1, U }, { Z, 1, U } },
		{ { C_, 0, U }, { D_, h, U } },
		{ { C_, e, W }, { D_, 1, W } },
		{ { C_, 0, U }, { C_, 1, W }, { D_, e, W }, { D_, h, U } },
		{ { P_, 0, U }, { M, e, U } },
		{ { M, h, U }, { P_, 1, U } },
		{ { M, 2, U }, { N, 2, W }, { P_, 2, U } },
		{ { C_, 3, U }, { D_, 3, W }, { Z, 3, W }, { P_, 3, U }, { N, 3, U }, { C_, 3, U }, { D_, 3, U } },
		{ { C_, 0, U }, { C_, 0, U } }, // dead, or no sector
		{ { N, 0, U }, { N, 0, W } }, // dead
		{ { C_, 0, U }, { N, h, W } }, // ends elsewhere
		{ { C_, 2, W }, { D_, 2, U } }, // ends elsewhere
		twice, // 16 operators
		{ { P_, 1, U }, { M, h, U }, { C_, 0, U }, { D_, 0, U } },
	};
}

// The composed plan against the one-operator plans chained backwards from every destination.  Returns 0: no sector (the chain agrees), 1: a sector
// and no destination reached, 2: destinations reached
int check_string(const std::vector<Op>& s, int L, int nup, int ndn)
{
	TjStringPlan P;
	const char* why = nullptr;
	CHECK(plan(s, L, nup, ndn, P, &why));
	std::vector<std::vector<int64_t>> one(s.size());
	int cu = nup, cd = ndn;
	bool has = true;
	for (size_t k = 0; k < s.size() && has; k++) {
		ObsTjPlan Q;
		CHECK(obs_plan_tj(s[k].op, s[k].site, s[k].spin, L, cu, cd, &has, Q, &why));
		if (!has) break;
		one[k].assign((size_t)(Q.n_up_dst * Q.n_dn_dst), 0);
		tj_expand(Q, one[k].data(), nullptr);
		cu = Q.nup2;
		cd = Q.ndn2;
	}
	CHECK(P.has == has);
	if (!has || !P.has) return 0;
	CHECK(cu == P.nup2 && cd == P.ndn2 && P.n_up_dst * P.n_dn_dst == tj_sector_size(L, cu, cd) && P.n_up_src * P.n_dn_src == tj_sector_size(L, nup, ndn));
	const int64_t n_src = P.n_up_src * P.n_dn_src, n_dst = P.n_up_dst * P.n_dn_dst;
	std::vector<int64_t> action((size_t)n_dst, 77);
	int64_t touched = -1;
	CHECK(tj_string_expand(P, action.data(), &touched, &why));
	std::vector<char> used((size_t)n_src, 0);
	int64_t reached = 0;
	for (int64_t d = 0; d < n_dst; d++) {
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
			CHECK(at >= 0 && at < n_src && !used[(size_t)at]);
			if (at >= 0 && at < n_src) used[(size_t)at] = 1;
		}
	}
	CHECK(reached == touched && reached == tj_string_touched(P));
	CHECK(!P.dead || reached == 0);
	return reached > 0 ? 2 : 1;
}

// What a launch uploads on sector (L; nup, ndn): 1, 8 and 5 of the strings that stay into the 8 slots of the bracket kernel, each slot expanded against
// the plan's own expansion and the later slots untouched; then the refusals.  Returns the number of live strings that stay.
int check_pack(int L, int nup, int ndn)
{
	const char* why = nullptr;
	std::vector<TjStringPlan> stay;
	TjStringPlan dead, leaves;
	for (const auto& s : strings(L)) {
		TjStringPlan P;
		CHECK(plan(s, L, nup, ndn, P, &why));
		if (!P.has) continue;
		if (P.dead) dead = P;
		else if (P.nup2 != nup || P.ndn2 != ndn) leaves = P;
		else stay.push_back(P);
	}
	CHECK(dead.dead && leaves.has && !stay.empty());
	if (stay.empty()) return 0;
	const int64_t n = tj_sector_size(L, nup, ndn);
	TjStringImage G;
	std::vector<int32_t> img;
	CHECK(tj_string_image_begin(G, L, nup, ndn, nup, ndn, 8, img, &why));
	CHECK(G.n_up * G.n_dn == n && img.size() == G.size());
	for (int s = 0; s < 8; s++) std::fill(img.begin() + (std::ptrdiff_t)G.entries(s), img.begin() + (std::ptrdiff_t)G.entries(s + 1), 77);
	for (int ns : { 1, 8, 5 }) {
		const std::vector<int32_t> before = img;
		std::vector<TjStringPlan> batch;
		for (int s = 0; s < ns; s++) batch.push_back(stay[(size_t)(s + ns) % stay.size()]);
		CHECK(tj_string_image_entries(G, batch.data(), ns, img, &why));
		for (int s = 0; s < ns; s++) {
			std::vector<int64_t> got((size_t)n, 77), want((size_t)n, 78);
			tj_string_expand_slot(G, img, s, batch[(size_t)s].up, got.data(), nullptr);
			CHECK(tj_string_expand(batch[(size_t)s], want.data(), nullptr, &why) && got == want);
		}
		CHECK(std::equal(img.begin() + (std::ptrdiff_t)G.entries(ns), img.end(), before.begin() + (std::ptrdiff_t)G.entries(ns))); // the later slots stay
		CHECK(std::equal(img.begin(), img.begin() + (std::ptrdiff_t)G.fixed(), before.begin())); // and so do the word lists and the rank tables
	}
	// refusals: a dead plan in the batch, a plan that ends in another sector, a plan of another source sector, more plans than slots -- nothing is written
	const std::vector<int32_t> before = img;
	const std::vector<TjStringPlan> with_dead { stay[0], dead }, with_leaving { stay[0], leaves }, nine(9, stay[0]);
	why = nullptr;
	CHECK(!tj_string_image_entries(G, with_dead.data(), 2, img, &why) && why && img == before);
	CHECK(!tj_string_image_entries(G, with_leaving.data(), 2, img, &why) && img == before);
	CHECK(!tj_string_image_entries(G, nine.data(), 9, img, &why) && img == before);
	TjStringPlan other;
	CHECK(plan({ { N, 0, U } }, L + 1, nup, ndn, other, &why) && other.has);
	CHECK(!tj_string_image_entries(G, &other, 1, img, &why) && img == before);
	TjStringImage G1;
	std::vector<int32_t> one_slot;
	CHECK(tj_string_image_begin(G1, L, nup, ndn, nup, ndn, 1, one_slot, &why));
	CHECK(!tj_string_image_entries(G1, nine.data(), 2, one_slot, &why));
	CHECK(tj_string_image_entries(G1, nine.data(), 1, one_slot, &why));
	CHECK(!tj_string_image_begin(G1, L, nup, L, nup, ndn, 1, one_slot, &why));
	return (int)stay.size();
}

} // namespace

int main()
{
	// (L; nup, ndn): 105 states; (7;2,2); three tiles; (9;1,3); one block; blocks of one element; full: cdagger finds no sector
	const int sectors[7][3] = { { 7, 1, 2 }, { 7, 2, 2 }, { 10, 3, 3 }, { 9, 1, 3 }, { 8, 3, 0 }, { 9, 0, 3 }, { 6, 3, 3 } };
	const int stays[4] = { 10, 11, 11, 11 };
	for (int q = 0; q < 7; q++) {
		const int L = sectors[q][0], nup = sectors[q][1], ndn = sectors[q][2];
		int nonzero = 0;
		for (const auto& s : strings(L)) {
			TjStringPlan P;
			const char* why = nullptr;
			CHECK(plan(s, L, nup, ndn, P, &why));
			nonzero += check_string(s, L, nup, ndn) == 2 && P.nup2 == nup && P.ndn2 == ndn;
		}
		if (q < 3) CHECK(nonzero == stays[q]);
		if (q < 4) CHECK(check_pack(L, nup, ndn) >= nonzero);
	}
	// every operator alone, and every pair and some triples on one site: all nine site histories against each other
	for (int a : { C_, D_, N, Z, P_, M })
		for (int sa : { U, W }) {
			if ((a == P_ || a == M) && sa == W) continue;
			check_string({ { a, 2, sa } }, 7, 2, 2);
			check_string({ { a, 0, sa } }, 6, 3, 3);
			for (int b : { C_, D_, N, Z, P_, M })
				for (int sb : { U, W }) {
					if ((b == P_ || b == M) && sb == W) continue;
					check_string({ { a, 2, sa }, { b, 2, sb } }, 7, 2, 2);
					check_string({ { a, 2, sa }, { b, 4, sb }, { C_, 3, U } }, 7, 2, 2);
					check_string({ { a, 3, sa }, { C_, 1, W }, { b, 3, sb }, { D_, 5, W }, { a, 3, sa } }, 8, 2, 3);
				}
		}
	// the (0,0) walk: c then cdagger of the only electron
	CHECK(check_string({ { C_, 0, U }, { D_, 0, U } }, 5, 1, 0) == 0);

	// 30 sites, 16 operators: planning only
	{
		TjStringPlan P;
		const char* why = nullptr;
		const std::vector<Op> s { { C_, 0, U }, { C_, 29, W }, { D_, 29, W }, { D_, 0, U }, { N, 12, U }, { N, 11, W }, { P_, 13, U }, { M, 13, U },
			                      { Z, 5, U }, { M, 20, U }, { P_, 20, U }, { Z, 13, W }, { C_, 7, U }, { D_, 7, U }, { N, 28, W }, { Z, 28, W } };
		CHECK(s.size() == 16 && plan(s, 30, 8, 8, P, &why) && P.has && !P.dead && P.nup2 == 8 && P.ndn2 == 8 && P.flip_up == 0 && P.flip_dn == 0 && !P.up.changes);
		CHECK(__builtin_popcount(P.touched) == 9 && tj_string_touched(P) == binom(21, 8 - 4) * binom(21 - 4, 8 - 5));
		CHECK(P.want_up == P.dst_up && P.want_dn == P.dst_dn && (P.want_up & P.want_dn) == 0);
	}

	// refusals
	{
		TjStringPlan P;
		const char* why = nullptr;
		CHECK(!plan({ { LPP_OP_IDENTITY, 0, U } }, 7, 2, 2, P, &why) && why);
		CHECK(!plan({ { N, 7, U } }, 7, 2, 2, P, &why));
		CHECK(!plan({ { N, -1, U } }, 7, 2, 2, P, &why));
		CHECK(!plan({ { N, 0, 2 } }, 7, 2, 2, P, &why));
		CHECK(!plan({ { N, 0, U } }, 7, 4, 4, P, &why));
		CHECK(!plan({ { N, 0, U } }, 31, 2, 2, P, &why));
		CHECK(!plan({}, 7, 2, 2, P, &why));
		CHECK(!plan(std::vector<Op>(17, Op { N, 0, U }), 7, 2, 2, P, &why));
		CHECK(!plan({ { P_, 0, W } }, 7, 2, 2, P, &why));
		CHECK(!plan({ { N, 0, U }, { M, 0, W } }, 7, 2, 2, P, &why));
		// (26;1,1): 25 sites free of down electrons -- a string that changes the pattern is refused, one that does not is planned
		CHECK(!plan({ { C_, 0, U }, { D_, 1, U } }, 26, 1, 1, P, &why));
		CHECK(plan({ { N, 0, W } }, 26, 1, 1, P, &why) && P.has && !P.up.changes && tj_string_touched(P) == 25);
		CHECK(plan({ { C_, 0, U }, { D_, 0, U } }, 26, 1, 1, P, &why) && P.has && !P.up.changes); // (net: a test)
		CHECK(plan({ { C_, 0, U }, { C_, 0, U } }, 7, 1, 2, P, &why) && !P.has); // no sector at the second step
		CHECK(plan({ { C_, 0, U }, { C_, 0, U } }, 7, 2, 2, P, &why) && P.has && P.dead && P.nup2 == 0);
	}
	if (failures) return 1;
	std::printf("ok\n");
	return 0;
}
