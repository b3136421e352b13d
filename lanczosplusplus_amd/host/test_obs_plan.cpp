// test_obs_plan.cpp -- the host planners of the one-site observables (csrc/lpp_obs_plan.h, lpp_obs_tj_plan.h, lpp_obs_heis_plan.h) in a stand-alone
// program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_observables_host.py does).  For every operator, spin and
// site of a list of sectors it expands the plan as the kernels walk it and checks
//   - every non-zero action k has |k| - 1 < n_src, and no source index is used twice;
//   - the number of touched destinations against a closed form (Hubbard: the species' counts; Heisenberg: heis_touched, the byte model's C(L - 1, .)),
//     or against a direct count over the sorted word list built by brute force (t-J, and with it the byte model's tj_touched);
//   - t-J and Heisenberg: that the source index IS the position of the source word in the brute-force list of the source sector;
// and the exact binomial against the long double product, the run counts of the long Heisenberg chains, and the refusals.
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lpp_obs_heis_plan.h"
#include "lpp_obs_plan.h"
#include "lpp_obs_tj_plan.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond) && failures++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
	} while (0)

const int kOps[] = { LPP_OP_C, LPP_OP_CDAGGER, LPP_OP_N, LPP_OP_SZ, LPP_OP_SPLUS, LPP_OP_SMINUS };
const int kSpins[] = { LPP_SPIN_UP, LPP_SPIN_DOWN };

// the first two invariants over an expanded plan; returns the number of touched destinations
int64_t check_action(const std::vector<int64_t>& action, int64_t n_src)
{
	std::vector<uint8_t> used((size_t)n_src, 0);
	int64_t touched = 0;
	for (const int64_t k : action) {
		if (k == 0) continue;
		touched++;
		const int64_t s = (k < 0 ? -k : k) - 1;
		CHECK(s < n_src);
		if (s >= n_src) continue;
		CHECK(!used[(size_t)s]);
		used[(size_t)s] = 1;
	}
	return touched;
}

// the ascending words of n set bits among L
std::vector<uint64_t> words(int L, int n)
{
	std::vector<uint64_t> out;
	uint64_t w = first_word(n);
	for (int64_t i = 0, cnt = binom(L, n); i < cnt; i++) {
		out.push_back(w);
		if (i + 1 < cnt) w = next_word(w);
	}
	return out;
}

int64_t position(const std::vector<uint64_t>& sorted, uint64_t w)
{
	const auto it = std::lower_bound(sorted.begin(), sorted.end(), w);
	return (it != sorted.end() && *it == w) ? (int64_t)(it - sorted.begin()) : -1;
}

void check_binomials()
{
	for (int n = 0; n <= 30; n++)
		for (int k = 0; k <= n; k++) {
			long double r = 1;
			for (int i = 1; i <= k; i++) r = r * (n - k + i) / i;
			CHECK(binom(n, k) == (int64_t)(r + 0.5L));
		}
	CHECK(binom(62, 31) == 465428353255261088ll && binom(5, 6) == 0 && binom(5, -1) == 0 && binom(63, 1) == 0);
}

// ---- Hubbard: k_obs_apply's lookup (obs_contrib) restated ---------------------------------------------------------------------------------
void check_hubbard(int L, int nup, int ndn)
{
	for (const int op : kOps)
		for (const int spin : kSpins)
			for (int site = 0; site < L; site++) {
				ObsPlan P;
				bool has = false;
				const char* why = nullptr;
				CHECK(obs_plan(op, site, spin, L, nup, ndn, &has, P, &why));
				int n1 = nup, n2 = ndn;
				CHECK(has == (!needs_new_basis(op) || new_parts(op, spin, L, nup, ndn, &n1, &n2)));
				if (!has) continue;
				CHECK(P.nup2 == n1 && P.ndn2 == n2 && P.n_up_dst == binom(L, n1) && P.n_dn_dst == binom(L, n2));
				CHECK((P.tu.empty() || (int64_t)P.tu.size() == P.n_up_dst) && (P.td.empty() || (int64_t)P.td.size() == P.n_dn_dst));
				std::vector<int64_t> action((size_t)(P.n_up_dst * P.n_dn_dst), 0);
				for (int64_t dd = 0; dd < P.n_dn_dst; dd++)
					for (int64_t du = 0; du < P.n_up_dst; du++) {
						const int64_t tu = P.tu.empty() ? du + 1 : P.tu[(size_t)du], td = P.td.empty() ? dd + 1 : P.td[(size_t)dd];
						int64_t k = 0;
						if (P.sz) k = ((tu != 0) - (td != 0)) * (du + dd * P.n_up_src + 1);
						else if (tu != 0 && td != 0) k = (((tu < 0) != (td < 0)) ? -1 : 1) * ((std::abs(tu) - 1) + (std::abs(td) - 1) * P.n_up_src + 1);
						action[(size_t)(du + dd * P.n_up_dst)] = k;
					}
				const int64_t touched = check_action(action, P.n_up_src * P.n_dn_src);
				// the species' counts: a destination word with the site's bit set (cdagger, n) or clear (c), the other L - 1 bits free; untouched: all
				const int64_t up_set = binom(L - 1, n1 - 1), up_clear = binom(L - 1, n1), dn_set = binom(L - 1, n2 - 1), dn_clear = binom(L - 1, n2);
				int64_t want = 0;
				switch (op) {
				case LPP_OP_C: want = (spin == LPP_SPIN_UP) ? up_clear * P.n_dn_dst : P.n_up_dst * dn_clear; break;
				case LPP_OP_CDAGGER:
				case LPP_OP_N: want = (spin == LPP_SPIN_UP) ? up_set * P.n_dn_dst : P.n_up_dst * dn_set; break;
				case LPP_OP_SPLUS: want = up_set * dn_clear; break;
				case LPP_OP_SMINUS: want = up_clear * dn_set; break;
				default: want = up_set * dn_clear + up_clear * dn_set; break; // sz: up only or down only -- a difference of the two tables, not a product
				}
				CHECK(touched == want);
				if (op != LPP_OP_SZ) CHECK(obs_touched(P) == touched); // (for sz the byte model counts the doubly occupied sites instead)
			}
}

// ---- t-J: the sorted words (down << L) | up without double occupancy ----------------------------------------------------------------------
std::vector<uint64_t> tj_words(int L, int nup, int ndn)
{
	std::vector<uint64_t> out;
	for (const uint64_t d : words(L, ndn))
		for (const uint64_t u : words(L, nup))
			if (!(u & d)) out.push_back((d << L) | u);
	std::sort(out.begin(), out.end());
	return out;
}

void check_tj(int L, int nup, int ndn)
{
	const std::vector<uint64_t> src = tj_words(L, nup, ndn);
	CHECK((int64_t)src.size() == tj_sector_size(L, nup, ndn));
	for (const int op : kOps)
		for (const int spin : kSpins)
			for (int site = 0; site < L; site++) {
				ObsTjPlan P;
				bool has = false;
				const char* why = nullptr;
				const bool ok = obs_plan_tj(op, site, spin, L, nup, ndn, &has, P, &why);
				CHECK(ok == !((op == LPP_OP_SPLUS || op == LPP_OP_SMINUS) && spin == LPP_SPIN_DOWN));
				if (!ok) CHECK(why && std::strstr(why, "spin DOWN"));
				if (!ok || !has) continue;
				const std::vector<uint64_t> dst = tj_words(L, P.nup2, P.ndn2);
				CHECK((int64_t)dst.size() == P.n_up_dst * P.n_dn_dst && (int64_t)src.size() == P.n_up_src * P.n_dn_src);
				std::vector<int64_t> action(dst.size(), 0);
				int64_t touched = 0;
				tj_expand(P, action.data(), &touched);
				CHECK(check_action(action, (int64_t)src.size()) == touched);
				// the direct count: the ket word the operator makes each destination (bra) word from
				const uint64_t ub = 1ull << site, db = ub << L;
				int64_t want = 0;
				for (size_t i = 0; i < dst.size(); i++) {
					const uint64_t w = dst[i];
					const bool up = (w & ub) != 0, dn = (w & db) != 0;
					bool hit = false;
					uint64_t ket = w;
					switch (op) {
					case LPP_OP_C: hit = !up && !dn, ket = w | (spin == LPP_SPIN_UP ? ub : db); break;
					case LPP_OP_CDAGGER: hit = (spin == LPP_SPIN_UP) ? up : dn, ket = w ^ (spin == LPP_SPIN_UP ? ub : db); break;
					case LPP_OP_SPLUS: hit = up, ket = (w ^ ub) | db; break;
					case LPP_OP_SMINUS: hit = dn, ket = (w ^ db) | ub; break;
					default: hit = (spin == LPP_SPIN_UP) ? up : dn; break; // n, sz: the occupancy of `spin`
					}
					want += hit;
					CHECK(hit == (action[i] != 0));
					if (hit && action[i] != 0) CHECK(std::abs(action[i]) - 1 == position(src, ket));
				}
				CHECK(touched == want && tj_touched(op, spin, L, P.nup2, P.ndn2) == want); // (the byte model's closed form)
			}
}

// ---- Heisenberg: the ascending L-bit words of m set bits -----------------------------------------------------------------------------------
void check_heis(int L, int m, int lb_want)
{
	CHECK(heis_low_bits(L) == lb_want);
	const std::vector<uint64_t> src = words(L, m);
	for (const int op : { LPP_OP_N, LPP_OP_SZ, LPP_OP_SPLUS, LPP_OP_SMINUS })
		for (const int spin : kSpins)
			for (int site = 0; site < L; site++) {
				ObsHeisPlan P;
				const char* why = nullptr;
				const bool ok = obs_plan_heis(op, site, spin, L, m, P, &why);
				CHECK(ok == !((op == LPP_OP_SPLUS && m == L) || (op == LPP_OP_SMINUS && m == 0)));
				if (!ok) CHECK(why && std::strstr(why, "S+ to all ups or S- to all downs"));
				if (!ok) continue;
				CHECK(P.lb == lb_want && P.n_src == (int64_t)src.size() && P.n_dst == binom(L, P.m2) && P.runs.back().dst0 == P.n_dst);
				const std::vector<uint64_t> dst = words(L, P.m2);
				std::vector<int64_t> action(dst.size(), 0);
				int64_t touched = 0;
				heis_expand(P, action.data(), &touched);
				CHECK(check_action(action, P.n_src) == touched);
				CHECK(touched == heis_touched(op, spin, L, P.m2));
				const uint64_t bit = 1ull << site;
				for (size_t i = 0; i < dst.size(); i++) {
					const bool set = (dst[i] & bit) != 0;
					int64_t want = 0; // +-(position of the ket word + 1)
					if (op == LPP_OP_SZ) want = set ? -((int64_t)i + 1) : (int64_t)i + 1;
					else if (op == LPP_OP_N) want = (set == (spin == LPP_SPIN_UP)) ? (int64_t)i + 1 : 0;
					else if (set == (op == LPP_OP_SPLUS)) want = position(src, dst[i] ^ bit) + 1;
					CHECK(action[i] == want);
				}
			}
	ObsHeisPlan P;
	const char* why = nullptr;
	CHECK(!obs_plan_heis(LPP_OP_C, 0, LPP_SPIN_UP, L, m, P, &why) && !obs_plan_heis(LPP_OP_CDAGGER, 0, LPP_SPIN_UP, L, m, P, &why));
}

int64_t heis_runs(int op, int L, int m)
{
	ObsHeisPlan P;
	const char* why = nullptr;
	return obs_plan_heis(op, 0, LPP_SPIN_UP, L, m, P, &why) ? (int64_t)P.runs.size() - 1 : -1;
}

} // namespace

int main()
{
	check_binomials();

	check_hubbard(1, 1, 0);
	check_hubbard(4, 0, 2);
	check_hubbard(4, 4, 4);
	check_hubbard(6, 3, 3);
	check_hubbard(12, 6, 5);

	check_tj(4, 1, 1);
	check_tj(6, 0, 3);
	check_tj(6, 3, 0);
	check_tj(6, 2, 4);
	check_tj(8, 3, 2);
	check_tj(24, 1, 0); // the pattern width is exactly 2 * kObsTjMaxHalf
	{ // 25 free sites: only what leaves the patterns alone is planned
		ObsTjPlan P;
		bool has = false;
		const char* why = nullptr;
		for (const int op : { LPP_OP_C, LPP_OP_CDAGGER, LPP_OP_N, LPP_OP_SZ }) {
			why = nullptr;
			CHECK(!obs_plan_tj(op, 3, LPP_SPIN_UP, 26, 1, 1, &has, P, &why) && why && std::strstr(why, "more than 24 sites"));
		}
		CHECK(obs_plan_tj(LPP_OP_N, 3, LPP_SPIN_DOWN, 26, 1, 1, &has, P, &why) && has && P.up == TJ_UP_SAME);
		int64_t touched = 0;
		tj_expand(P, nullptr, &touched);
		CHECK(touched == 25 && tj_touched(LPP_OP_N, LPP_SPIN_DOWN, 26, 1, 1) == 25); // the down electron at the site, the up electron on any other
	}

	check_heis(1, 0, 1);
	check_heis(7, 2, 7);
	check_heis(12, 6, 12);
	check_heis(13, 6, 12); // one high bit
	check_heis(16, 7, 12);
	check_heis(40, 2, 14); // 26 high bits: the class-by-class path
	CHECK(heis_runs(LPP_OP_SZ, 40, 2) == 352 && heis_runs(LPP_OP_SPLUS, 40, 2) == 2952);
	check_heis(62, 1, 14); // the largest word
	CHECK(heis_runs(LPP_OP_SZ, 62, 1) == 49);
	check_heis(7, 7, 7); // S+ refused
	check_heis(7, 0, 7); // S- refused

	if (failures) return 1;
	std::printf("ok\n");
	return 0;
}
