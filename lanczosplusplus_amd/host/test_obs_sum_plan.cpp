// test_obs_sum_plan.cpp -- the host planner of the site-weighted operator sums (csrc/lpp_obs_sum_plan.h) in a stand-alone program, meant to be built
// with -fsanitize=address,undefined and run on the CPU (tests/test_operator_sum_host.py does).  For every sector with L <= 7, every operator and spin:
//   - the planner refuses, or reports "no sector", exactly where obs_plan does (splus / sminus: always refused, they have no fused plan);
//   - c / cdagger: the width is L - n or n, every destination word has exactly W non-zero entries with sources inside the source species, no source
//     twice, sites ascending with k, and entry (k, d) IS obs_plan's table of that site at d;
//   - n / sz: the word lists are the species' ascending words, and the expansion's factor is the closed form under random weights;
//   - the expansion stays inside the source sector.
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lpp_obs_plan.h"
#include "lpp_obs_sum_plan.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond) && failures++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
	} while (0)

const int kOps[] = { LPP_OP_C, LPP_OP_CDAGGER, LPP_OP_N, LPP_OP_SZ, LPP_OP_SPLUS, LPP_OP_SMINUS };

void check_sector(int L, int nup, int ndn)
{
	std::vector<double> wr((size_t)(L > 0 ? L : 1)), wi(wr.size());
	for (size_t r = 0; r < wr.size(); r++) {
		wr[r] = 0.25 + 0.5 * (double)r;
		wi[r] = 1.0 - 0.125 * (double)(r * r);
	}
	for (const int op : kOps)
		for (int spin = 0; spin < 2; spin++) {
			ObsPlan S;
			ObsSumPlan P;
			bool has1 = false, has = false;
			const char *why1 = nullptr, *why = nullptr;
			const bool ok1 = obs_plan(op, 0, spin, L, nup, ndn, &has1, S, &why1);
			const bool ok = obs_sum_plan(op, spin, L, nup, ndn, &has, P, &why);
			if (!ok1 || !obs_sum_fused_op(op)) {
				CHECK(!ok && why != nullptr && !has);
				continue;
			}
			CHECK(ok);
			CHECK(has == has1);
			if (!ok || !has) continue;
			CHECK(P.nup2 == S.nup2 && P.ndn2 == S.ndn2 && P.n_up_dst == S.n_up_dst && P.n_dn_dst == S.n_dn_dst && P.n_up_src == S.n_up_src && P.n_dn_src == S.n_dn_src);
			const int64_t n_src = P.n_up_src * P.n_dn_src, n_dst = P.n_up_dst * P.n_dn_dst;
			const int width = obs_sum_width(P);
			std::vector<int64_t> src((size_t)(n_dst * width));
			std::vector<int32_t> site(src.size());
			std::vector<double> fr(src.size()), fi(src.size());
			obs_sum_expand(P, wr.data(), wi.data(), src.data(), site.data(), fr.data(), fi.data());
			for (const int64_t s : src) CHECK(s >= 0 && s < n_src);
			if (P.diag) {
				CHECK(width == 1 && P.src.empty() && (int64_t)P.words_up.size() == P.n_up_dst && (int64_t)P.words_dn.size() == P.n_dn_dst);
				for (int64_t el = 0; el < n_dst; el++) {
					const uint32_t wu = P.words_up[(size_t)(el % P.n_up_dst)], wd = P.words_dn[(size_t)(el / P.n_up_dst)];
					CHECK(__builtin_popcount(wu) == nup && __builtin_popcount(wd) == ndn);
					double er = 0, ei = 0; // sum_r f_r (value of the operator at site r)
					for (int r = 0; r < L; r++) {
						const double u = (double)((wu >> r) & 1), d = (double)((wd >> r) & 1);
						const double v = (op == LPP_OP_SZ) ? 0.5 * (u - d) : (spin == LPP_SPIN_UP ? u : d);
						er += wr[(size_t)r] * v;
						ei += wi[(size_t)r] * v;
					}
					CHECK(src[(size_t)el] == el && site[(size_t)el] == -1);
					CHECK(std::abs(fr[(size_t)el] - er) < 1e-12 && std::abs(fi[(size_t)el] - ei) < 1e-12);
				}
				continue;
			}
			const int n_moved = P.down ? P.ndn2 : P.nup2;
			const int64_t n_src_species = P.down ? P.n_dn_src : P.n_up_src;
			CHECK(P.down == (spin == LPP_SPIN_DOWN));
			CHECK(P.W == (op == LPP_OP_C ? L - n_moved : n_moved) && P.W >= 1);
			CHECK(P.n == (P.down ? P.n_dn_dst : P.n_up_dst));
			CHECK((int64_t)P.src.size() == (int64_t)P.W * P.n && P.site.size() == P.src.size());
			// against the per-site tables, site by site
			std::vector<std::vector<int32_t>> tabs((size_t)L);
			for (int r = 0; r < L; r++) {
				bool h = false;
				ObsPlan Q;
				CHECK(obs_plan(op, r, spin, L, nup, ndn, &h, Q, &why1) && h);
				tabs[(size_t)r] = P.down ? Q.td : Q.tu;
			}
			for (int64_t d = 0; d < P.n; d++) {
				std::vector<uint8_t> used((size_t)n_src_species, 0);
				int last = -1, per_site = 0;
				for (int k = 0; k < P.W; k++) {
					const int32_t t = P.src[(size_t)k * (size_t)P.n + (size_t)d];
					const int r = P.site[(size_t)k * (size_t)P.n + (size_t)d];
					CHECK(t != 0);
					const int64_t s = (int64_t)(t < 0 ? -t : t) - 1;
					CHECK(s >= 0 && s < n_src_species);
					if (s >= 0 && s < n_src_species) {
						CHECK(!used[(size_t)s]);
						used[(size_t)s] = 1;
					}
					CHECK(r > last && r < L);
					last = r;
					if (r >= 0 && r < L) CHECK(tabs[(size_t)r][(size_t)d] == t);
				}
				for (int r = 0; r < L; r++) per_site += (tabs[(size_t)r][(size_t)d] != 0);
				CHECK(per_site == P.W); // no entry of any site is left out
			}
		}
}

} // namespace

int main()
{
	for (int L = 1; L <= 7; L++)
		for (int nup = 0; nup <= L; nup++)
			for (int ndn = 0; ndn <= L; ndn++) check_sector(L, nup, ndn);
	// refusals as obs_plan: sites, sector, spin, operator
	ObsSumPlan P;
	bool has = true;
	const char* why = nullptr;
	CHECK(!obs_sum_plan(LPP_OP_C, LPP_SPIN_UP, 0, 0, 0, &has, P, &why) && why && !has);
	CHECK(!obs_sum_plan(LPP_OP_C, LPP_SPIN_UP, 31, 3, 3, &has, P, &why));
	CHECK(!obs_sum_plan(LPP_OP_C, LPP_SPIN_UP, 6, 7, 3, &has, P, &why));
	CHECK(!obs_sum_plan(LPP_OP_C, LPP_SPIN_UP, 6, 3, -1, &has, P, &why));
	CHECK(!obs_sum_plan(LPP_OP_C, 2, 6, 3, 3, &has, P, &why));
	CHECK(!obs_sum_plan(0, LPP_SPIN_UP, 6, 3, 3, &has, P, &why));
	CHECK(!obs_sum_plan(LPP_OP_SPLUS, LPP_SPIN_UP, 6, 3, 3, &has, P, &why));
	// "no sector" as obs_plan: cdagger on a full species, c on an empty one, the (0,0) sector
	CHECK(obs_sum_plan(LPP_OP_CDAGGER, LPP_SPIN_UP, 6, 6, 3, &has, P, &why) && !has);
	CHECK(obs_sum_plan(LPP_OP_C, LPP_SPIN_DOWN, 6, 3, 0, &has, P, &why) && !has);
	CHECK(obs_sum_plan(LPP_OP_C, LPP_SPIN_UP, 6, 1, 0, &has, P, &why) && !has);
	// the coefficient of a word adds the weights in ascending site
	std::vector<uint32_t> words { 0u, 0x5u, 0x2au };
	const double wr[6] = { 1, 2, 4, 8, 16, 32 }, wi[6] = { -1, -2, -4, -8, -16, -32 };
	std::vector<double> cr, ci;
	obs_sum_coef(words, wr, wi, cr, ci);
	CHECK(cr[0] == 0 && cr[1] == 5 && cr[2] == 42 && ci[1] == -5 && ci[2] == -42);
	obs_sum_coef(words, wr, nullptr, cr, ci);
	CHECK(cr[2] == 42 && ci[2] == 0);
	if (failures) {
		std::printf("%d check(s) failed\n", failures);
		return 1;
	}
	std::printf("ok\n");
	return 0;
}
