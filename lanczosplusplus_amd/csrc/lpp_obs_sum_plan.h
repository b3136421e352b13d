// lpp_obs_sum_plan.h -- host-only planning of a site-weighted operator sum  sum_r f_r O_r  in the Hubbard product basis (the kernels that read its
// tables: lpp_obs_sum_kernels.h).  Plain C++, no HIP: host/test_obs_sum_plan.cpp compiles the plan headers alone under the sanitizers.
//
// The tables are those of the per-site planner (lpp_obs_plan.h: species_table through obs_plan) for every site, transposed: signs and ranks are the
// existing ones by construction, and nothing here depends on the weights -- one plan serves every momentum.
//   c, cdagger (one species moves): every destination word of the moved species has exactly W sources (W = L - n for c, n for cdagger, n = the
//       destination word's popcount), one per site that c may have emptied / cdagger may have filled.  Uniform width, k-major:
//       src[k * n + d] = +-(source rank + 1), site[k * n + d] = the site whose weight applies; k ascends with the site.
//   n (given spin), sz: the operator stays in the sector and is diagonal; the plan is the two species' word lists, and per call a coefficient per
//       species word, c[word] = sum_{r in word} f_r (obs_sum_coef, added in ascending site from 0).  The element factor is alpha cu[du] + beta cd[dd]
//       with (alpha, beta) = (1, 0) for n up, (0, 1) for n down, (1/2, -1/2) for sz -- Engine::accModifiedState's meanings (Engine.h:535-599).
// splus / sminus have no fused plan: the driver chains the one-site launches for them.
#pragma once
#include <stdint.h>

#include <vector>

#include "lpp_obs_plan.h"
#include "lpp_switch.h"

namespace lpp {
namespace obs_host {

constexpr int kObsSumMaxSites = 30; // the weights travel in the kernel arguments

// the LPP_OBS_* switches, read once per engine (lpp_obs.hip: where the engine's plan cache is made)
struct ObsSwitches {
	EnvSwitch sum_chain; // LPP_OBS_SUM_CHAIN=1: operator sums go through the chain of one-site launches (tests and the benchmark)
};
inline ObsSwitches obs_switches_from_env()
{
	ObsSwitches sw;
	sw.sum_chain = env_switch("LPP_OBS_SUM_CHAIN");
	return sw;
}

inline bool obs_sum_fused_op(int op) { return op == LPP_OP_C || op == LPP_OP_CDAGGER || op == LPP_OP_N || op == LPP_OP_SZ; }

struct ObsSumPlan {
	int nup2 = 0, ndn2 = 0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	bool diag = false; // n, sz
	bool down = false; // the moved species (c, cdagger)
	int W = 0; // sources per destination word of the moved species
	int64_t n = 0; // destination words of the moved species
	std::vector<int32_t> src; // W * n, k-major
	std::vector<uint8_t> site; // W * n
	double alpha = 0.0, beta = 0.0; // diag: the factors on the up and the down coefficient
	std::vector<uint32_t> words_up, words_dn; // diag: the words of the two species, ascending
};

// false: refused, *why says why (exactly where obs_plan refuses, and for an operator without a fused plan).  *has == false: no sector
inline bool obs_sum_plan(int op, int spin, int L, int nup, int ndn, bool* has, ObsSumPlan& P, const char** why)
{
	*has = false;
	P = ObsSumPlan();
	ObsPlan S;
	if (!obs_plan(op, 0, spin, L, nup, ndn, has, S, why)) return false; // (site 0 is a site of every admissible L)
	if (!obs_sum_fused_op(op)) {
		*has = false;
		*why = "operator sum: splus / sminus have no fused plan";
		return false;
	}
	if (!*has) return true;
	P.nup2 = S.nup2, P.ndn2 = S.ndn2;
	P.n_up_src = S.n_up_src, P.n_dn_src = S.n_dn_src, P.n_up_dst = S.n_up_dst, P.n_dn_dst = S.n_dn_dst;
	if (op == LPP_OP_N || op == LPP_OP_SZ) {
		P.diag = true;
		P.alpha = (op == LPP_OP_SZ) ? 0.5 : (spin == LPP_SPIN_UP ? 1.0 : 0.0);
		P.beta = (op == LPP_OP_SZ) ? -0.5 : (spin == LPP_SPIN_UP ? 0.0 : 1.0);
		species_words(L, nup, P.words_up);
		species_words(L, ndn, P.words_dn);
		return true;
	}
	P.down = (spin == LPP_SPIN_DOWN);
	const int n_moved = P.down ? P.ndn2 : P.nup2;
	P.W = (op == LPP_OP_C) ? L - n_moved : n_moved;
	P.n = P.down ? P.n_dn_dst : P.n_up_dst;
	P.src.assign((size_t)P.W * (size_t)P.n, 0);
	P.site.assign((size_t)P.W * (size_t)P.n, 0);
	std::vector<int> fill((size_t)P.n, 0);
	for (int r = 0; r < L; r++) { // ascending site: k ascends with the site
		bool h = false;
		if (r > 0 && !obs_plan(op, r, spin, L, nup, ndn, &h, S, why)) return false;
		const std::vector<int32_t>& t = P.down ? S.td : S.tu;
		for (int64_t d = 0; d < P.n; d++) {
			if (t[(size_t)d] == 0) continue;
			const int k = fill[(size_t)d]++;
			if (k >= P.W) {
				*why = "operator sum: a destination word with more sources than its width (internal)";
				return false;
			}
			P.src[(size_t)k * (size_t)P.n + (size_t)d] = t[(size_t)d];
			P.site[(size_t)k * (size_t)P.n + (size_t)d] = (uint8_t)r;
		}
	}
	for (int64_t d = 0; d < P.n; d++)
		if (fill[(size_t)d] != P.W) {
			*why = "operator sum: a destination word with fewer sources than its width (internal)";
			return false;
		}
	return true;
}

// c[word] = sum_{r in word} f_r, added in ascending site starting from 0: what k_obs_sum_coef computes, term by term
inline void obs_sum_coef(const std::vector<uint32_t>& words, const double* w_re, const double* w_im, std::vector<double>& c_re, std::vector<double>& c_im)
{
	c_re.assign(words.size(), 0.0);
	c_im.assign(words.size(), 0.0);
	for (size_t i = 0; i < words.size(); i++) {
		double re = 0.0, im = 0.0;
		for (uint32_t w = words[i]; w; w &= w - 1) {
			const int r = __builtin_ctz(w);
			re += w_re[r];
			if (w_im) im += w_im[r];
		}
		c_re[i] = re;
		c_im[i] = im;
	}
}

// The plan expanded for the host tests: coef[dst * n_src + src] would be dense, so the expansion is a list per destination in kernel order --
// term t of destination dst: src_index[dst * width + t] (or -1), with the weight's site and the sign.  For diag plans width == 1, the source is the
// destination itself, site = -1 and (fac_re, fac_im) carry the element factor of the given weights.
inline int obs_sum_width(const ObsSumPlan& P) { return P.diag ? 1 : P.W; }
inline void obs_sum_expand(const ObsSumPlan& P, const double* w_re, const double* w_im, int64_t* src_index, int32_t* site, double* fac_re, double* fac_im)
{
	const int64_t nd = P.n_up_dst * P.n_dn_dst;
	if (P.diag) {
		std::vector<double> ur, ui, dr, di;
		obs_sum_coef(P.words_up, w_re, w_im, ur, ui);
		obs_sum_coef(P.words_dn, w_re, w_im, dr, di);
		for (int64_t el = 0; el < nd; el++) {
			const int64_t dd = el / P.n_up_dst, du = el - dd * P.n_up_dst;
			src_index[el] = el;
			site[el] = -1;
			fac_re[el] = P.alpha * ur[(size_t)du] + P.beta * dr[(size_t)dd];
			fac_im[el] = P.alpha * ui[(size_t)du] + P.beta * di[(size_t)dd];
		}
		return;
	}
	for (int64_t el = 0; el < nd; el++) {
		const int64_t dd = el / P.n_up_dst, du = el - dd * P.n_up_dst;
		const int64_t d = P.down ? dd : du;
		for (int k = 0; k < P.W; k++) {
			const int32_t t = P.src[(size_t)k * (size_t)P.n + (size_t)d];
			const int r = P.site[(size_t)k * (size_t)P.n + (size_t)d];
			const int64_t s = (int64_t)(t < 0 ? -t : t) - 1;
			const double sg = t < 0 ? -1.0 : 1.0;
			src_index[el * P.W + k] = P.down ? du + s * P.n_up_src : s + dd * P.n_up_src;
			site[el * P.W + k] = r;
			fac_re[el * P.W + k] = sg * w_re[r];
			fac_im[el * P.W + k] = w_im ? sg * w_im[r] : 0.0;
		}
	}
}

} // namespace obs_host
} // namespace lpp
