// lpp_obs_plan.h -- host-only planning of the one-site observables: the sector arithmetic every basis shares (binomials, species ranks, the next word
// of a popcount, HubbardOneOrbital::hasNewParts) and the planner of ONE operator in the Hubbard product basis (the kernel that reads its two tables:
// lpp_obs_kernels.h).  Plain C++, no HIP: the sanitizer test of the planners (host/test_obs_plan.cpp) compiles the plan headers alone.
// A planner refuses by returning false with *why set; the entry points turn that into LPP_ERR_INVALID (lpp_obs.hip).
#pragma once
#include <stdint.h>

#include <vector>

#include "lpp_engine.h"

// the one lookup of a family (obs_tj_source, obs_heis_source): the kernel calls it per element, the host expands the plan with it
#ifdef __HIPCC__
#define LPP_OBS_LOOKUP __host__ __device__ __forceinline__
#else
#define LPP_OBS_LOOKUP inline
#endif

namespace lpp {
namespace obs_host {

inline bool needs_new_basis(int op) { return op == LPP_OP_C || op == LPP_OP_CDAGGER || op == LPP_OP_SPLUS || op == LPP_OP_SMINUS; } // LabeledOperator.h:83-90
inline bool valid_op(int op) { return op == LPP_OP_C || op == LPP_OP_SZ || op == LPP_OP_CDAGGER || op == LPP_OP_N || op == LPP_OP_SPLUS || op == LPP_OP_SMINUS; }

constexpr int kBinomMax = 62; // the longest word any basis here has (Heisenberg)

// C(n, k) in integers, exact for n <= 62; 0 outside the triangle
inline int64_t binom(int n, int k)
{
	static const std::vector<int64_t> tab = [] {
		std::vector<int64_t> t((size_t)(kBinomMax + 1) * (kBinomMax + 1), 0);
		for (int i = 0; i <= kBinomMax; i++) {
			t[(size_t)i * (kBinomMax + 1)] = 1;
			for (int j = 1; j <= i; j++) t[(size_t)i * (kBinomMax + 1) + j] = t[(size_t)(i - 1) * (kBinomMax + 1) + j - 1] + (j <= i - 1 ? t[(size_t)(i - 1) * (kBinomMax + 1) + j] : 0);
		}
		return t;
	}();
	return (n < 0 || n > kBinomMax || k < 0 || k > n) ? 0 : tab[(size_t)n * (kBinomMax + 1) + k];
}

// a species (or a sector's count of patterns) the 32-bit table entries +-(rank + 1) cannot index
inline bool too_many_states(int64_t n) { return n >= (int64_t)INT32_MAX - 4096; }
template <typename Plan> bool too_many_states(const Plan& P) { return too_many_states(P.n_up_src) || too_many_states(P.n_dn_src) || too_many_states(P.n_up_dst) || too_many_states(P.n_dn_dst); }

// HubbardOneOrbital::hasNewParts for c / cdagger / splus / sminus
inline bool new_parts(int op, int spin, int L, int nup, int ndn, int* n1, int* n2)
{
	int p1 = nup, p2 = ndn;
	if (op == LPP_OP_C || op == LPP_OP_CDAGGER) { // hasNewPartsCorCdagger :212-230
		const int c = (op == LPP_OP_C) ? -1 : 1;
		if (spin == LPP_SPIN_UP) p1 += c;
		else p2 += c;
		if (p1 < 0 || p2 < 0) return false;
		if (p1 > L || p2 > L) return false;
		if (p1 == 0 && p2 == 0) return false;
	} else { // hasNewPartsSplusOrSminus :232-253
		const int c = (op == LPP_OP_SPLUS) ? 1 : -1;
		p1 += c;
		p2 -= c;
		if (p1 < 0 || p2 < 0) return false;
		if (p1 > L || p2 > L) return false;
	}
	*n1 = p1;
	*n2 = p2;
	return true;
}

inline int64_t hubbard_sector_size(int L, int nup, int ndn) { return (L < 1 || L > 30 || nup < 0 || ndn < 0 || nup > L || ndn > L) ? -1 : binom(L, nup) * binom(L, ndn); }

// BasisOneSpin::perfectIndex (BasisOneSpin.h:73-81): the rank of a word among the ascending words of its popcount
struct Ranker {
	int L;
	std::vector<int64_t> comb; // comb[b * (L + 2) + c]
	explicit Ranker(int L_) : L(L_), comb((size_t)(L_ + 1) * (L_ + 2))
	{
		for (int b = 0; b <= L; b++)
			for (int c = 0; c <= L + 1; c++) comb[(size_t)b * (L + 2) + c] = binom(b, c);
	}
	int64_t rank(uint64_t w) const
	{
		int64_t n = 0;
		int c = 1;
		for (int b = 0; w; b++, w >>= 1)
			if (w & 1) n += comb[(size_t)b * (L + 2) + c++];
		return n;
	}
};

// the lowest word of n set bits, and the next word of the same popcount (BasisOneSpin.h:53-61; not for w == 0, and not past the last word)
inline uint64_t first_word(int n) { return (n == 0) ? 0 : ((1ull << n) - 1); }
inline uint64_t next_word(uint64_t w)
{
	const uint64_t c = w & (~w + 1), r = w + c;
	return (((r ^ w) >> 2) / c) | r;
}

// the ascending words of one species by rank (at most 32 sites)
inline void species_words(int L, int n, std::vector<uint32_t>& out)
{
	const int64_t cnt = binom(L, n);
	out.resize((size_t)cnt);
	uint64_t w = first_word(n);
	for (int64_t i = 0; i < cnt; i++) {
		out[(size_t)i] = (uint32_t)w;
		if (i + 1 < cnt) w = next_word(w);
	}
}

// ---- one operator in the Hubbard product basis ------------------------------------------------------------------------------------------

enum { SP_C, SP_CDAGGER, SP_N };

// one species: destination rank -> +-(source rank + 1) or 0.  kind: what the operator does to the KET word (BasisOneSpin::getBra :121-149);
// with_sign: the parity of the ket's bits below `site` (doSignGf :112-136 for ind > 0 and both species; ProgramGlobals::doSign :109-114)
inline void species_table(const Ranker& R, int L, int n_dst, int kind, int site, bool with_sign, int global_sign, std::vector<int32_t>& tab)
{
	const int64_t cnt = binom(L, n_dst);
	tab.assign((size_t)cnt, 0);
	if (cnt == 0) return;
	const uint64_t bit = 1ull << site;
	uint64_t w = first_word(n_dst);
	for (int64_t i = 0; i < cnt; i++) {
		uint64_t ket = 0;
		bool ok = false;
		if (kind == SP_C) { // the bra lacks the bit the ket had
			ok = !(w & bit);
			ket = w | bit;
		} else if (kind == SP_CDAGGER) {
			ok = (w & bit) != 0;
			ket = w ^ bit;
		} else {
			ok = (w & bit) != 0;
			ket = w;
		}
		if (ok) {
			int s = global_sign;
			if (with_sign && (__builtin_popcountll(ket & (bit - 1)) & 1)) s = -s;
			tab[(size_t)i] = (int32_t)(s * (R.rank(ket) + 1));
		}
		if (i + 1 < cnt) w = next_word(w);
	}
}

struct ObsPlan {
	int nup2 = 0, ndn2 = 0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	bool sz = false;
	std::vector<int32_t> tu, td; // empty: the species is untouched
};

// false: refused, *why says why.  *has == false: the operator leads to no sector (hasNewParts refused)
inline bool obs_plan(int op, int site, int spin, int L, int nup, int ndn, bool* has, ObsPlan& P, const char** why)
{
	*has = false;
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	if (!valid_op(op)) return refuse("observables: unknown operator (LPP_OP_*)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return refuse("observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (L < 1 || L > 30 || site < 0 || site >= L || nup < 0 || ndn < 0 || nup > L || ndn > L) return refuse("observables: bad sites / site / sector");
	P = ObsPlan();
	P.nup2 = nup;
	P.ndn2 = ndn;
	if (needs_new_basis(op) && !new_parts(op, spin, L, nup, ndn, &P.nup2, &P.ndn2)) return true;
	P.n_up_src = binom(L, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(L, P.nup2);
	P.n_dn_dst = binom(L, P.ndn2);
	if (too_many_states(P)) return refuse("observables: a species with 2^31 states or more");
	const Ranker R(L);
	const int kind = (op == LPP_OP_C) ? SP_C : SP_CDAGGER;
	switch (op) {
	case LPP_OP_C:
	case LPP_OP_CDAGGER:
		if (spin == LPP_SPIN_UP) {
			species_table(R, L, P.nup2, kind, site, true, 1, P.tu);
		} else {
			// doSignGf, SPIN_DOWN: for ind > 0 the up parity computed first is overwritten by the parity of the down bits below ind;
			// for ind == 0 the up parity is the whole sign (BasisHubbardLanczos.h:125-136) -- a constant of the source sector
			const int up_parity = (site == 0 && (nup & 1)) ? -1 : 1;
			species_table(R, L, P.ndn2, kind, site, site > 0, up_parity, P.td);
		}
		break;
	case LPP_OP_N:
		if (spin == LPP_SPIN_UP) species_table(R, L, nup, SP_N, site, false, 1, P.tu);
		else species_table(R, L, ndn, SP_N, site, false, 1, P.td);
		break;
	case LPP_OP_SZ: // getBraIndexSz :210-223: +1 up only, -1 down only
		species_table(R, L, nup, SP_N, site, false, 1, P.tu);
		species_table(R, L, ndn, SP_N, site, false, 1, P.td);
		P.sz = true;
		break;
	case LPP_OP_SPLUS: // getBraIndexSplusSminus :225-246: cdagger on the up word, c on the down word; sign doSignSpSm :151-160
		species_table(R, L, P.nup2, SP_CDAGGER, site, true, 1, P.tu);
		species_table(R, L, P.ndn2, SP_C, site, true, 1, P.td);
		break;
	case LPP_OP_SMINUS:
		species_table(R, L, P.nup2, SP_C, site, true, 1, P.tu);
		species_table(R, L, P.ndn2, SP_CDAGGER, site, true, 1, P.td);
		break;
	}
	*has = true;
	return true;
}

// the byte model's count of the destinations that have a source: the product of the species' counts (an untouched species counts whole)
inline int64_t obs_touched(const ObsPlan& P)
{
	auto count = [](const std::vector<int32_t>& t, int64_t whole) {
		int64_t c = 0;
		for (const int32_t v : t) c += (v != 0);
		return t.empty() ? whole : c;
	};
	return count(P.tu, P.n_up_dst) * count(P.td, P.n_dn_dst);
}

} // namespace obs_host
} // namespace lpp
