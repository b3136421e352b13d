// lpp_obs_tj_plan.h -- host-only planning of ONE operator in the one-orbital t-J basis (BasisTjMultiOrbLanczos): the sector arithmetic, the down table
// and the split pattern rank tables k_obs_apply_tj reads (lpp_obs_tj_kernels.h, where the layout is described), and obs_tj_source, the ONE lookup the
// kernel calls per element and the host expands a plan with.  Plain C++, no HIP (host/test_obs_plan.cpp).
#pragma once
#include "lpp_obs_plan.h"

namespace lpp {

// what the operator does to the destination's pattern at position p to give the source's pattern
enum {
	TJ_UP_SAME = 0, // nothing, no condition: the source has the same pattern rank (n of the down species)
	TJ_UP_TEST, // bit p set, the same pattern (n of the up species)
	TJ_UP_SET, // bit p clear -> set (c up); sign: the parity of the bits below p
	TJ_UP_CLEAR, // bit p set -> cleared (cdagger up); the same sign
	TJ_UP_DEL0, // bit p clear -> deleted (c down: the source holds a down electron there, the site leaves the free sites)
	TJ_UP_DEL1, // bit p set -> deleted (splus)
	TJ_UP_INS0, // a 0 inserted at p (cdagger down: the site is free in the source, and empty)
	TJ_UP_INS1 // a 1 inserted at p (sminus)
};

constexpr int kObsTjMaxHalf = 12; // bits of a half pattern: the rank tables take 4096 x (4 + 2) bytes of LDS at most
struct ObsTjDown { // 8 bytes per destination down word
	int32_t src; // +-(rank of the source down word + 1), 0: the destination is not touched
	int32_t p; // position of the site among the sites the destination's down word leaves free
};

// destination (du, dd) -> +-(source index + 1), 0 = the reference does not touch it.  d = dn[dd]; hi_base / lo_rank wherever the caller keeps them.
LPP_OBS_LOOKUP int64_t obs_tj_source(int up, ObsTjDown d, uint32_t du, const uint32_t* __restrict__ pat, const int32_t* hi_base, const uint16_t* lo_rank, int lb,
                                     int64_t n_up_src)
{
	if (d.src == 0) return 0;
	bool neg = d.src < 0;
	const int64_t sd = (int64_t)(neg ? -d.src : d.src) - 1;
	int64_t su = du;
	if (up != TJ_UP_SAME) {
		const uint32_t cu = pat[du], bit = 1u << d.p, low = bit - 1u;
		const bool set = (cu & bit) != 0;
		uint32_t s = cu;
		switch (up) {
		case TJ_UP_TEST:
			if (!set) return 0;
			break;
		case TJ_UP_SET:
		case TJ_UP_CLEAR:
			if (set != (up == TJ_UP_CLEAR)) return 0;
			s = cu ^ bit;
			if (__builtin_popcount(cu & low) & 1) neg = !neg;
			break;
		case TJ_UP_DEL0:
		case TJ_UP_DEL1:
			if (set != (up == TJ_UP_DEL1)) return 0;
			s = (cu & low) | ((cu >> (d.p + 1)) << d.p);
			break;
		default: // TJ_UP_INS0, TJ_UP_INS1
			s = (cu & low) | ((cu >> d.p) << (d.p + 1)) | (up == TJ_UP_INS1 ? bit : 0u);
			break;
		}
		su = (int64_t)hi_base[s >> lb] + (int64_t)lo_rank[s & ((1u << lb) - 1u)];
	}
	const int64_t k = su + sd * n_up_src + 1;
	return neg ? -k : k;
}

namespace obs_host {

// TjMultiOrb::hasNewParts (TjMultiOrb.h:140-159, :538-584) for c / cdagger / splus / sminus: the Hubbard rules, the spin read by splus / sminus as well,
// no (0,0) sector for either pair, and no sector with more electrons than sites
inline bool new_parts_tj(int op, int spin, int L, int nup, int ndn, int* n1, int* n2)
{
	int p1 = nup, p2 = ndn;
	if (op == LPP_OP_C || op == LPP_OP_CDAGGER) {
		const int c = (op == LPP_OP_CDAGGER) ? 1 : -1;
		if (spin == LPP_SPIN_UP) p1 += c;
		else p2 += c;
	} else {
		const int c = (op == LPP_OP_SPLUS) ? 1 : -1;
		if (spin == LPP_SPIN_UP) {
			p1 += c;
			p2 -= c;
		} else {
			p2 += c;
			p1 -= c;
		}
	}
	if (p1 < 0 || p2 < 0) return false;
	if (p1 > L || p2 > L) return false;
	if (p1 == 0 && p2 == 0) return false;
	if (p1 + p2 > L) return false; // no double occupancy
	*n1 = p1;
	*n2 = p2;
	return true;
}

inline int64_t tj_sector_size(int L, int nup, int ndn) { return (L < 1 || L > 30 || nup < 0 || ndn < 0 || nup + ndn > L) ? -1 : binom(L, ndn) * binom(L - ndn, nup); }

struct ObsTjPlan {
	int nup2 = 0, ndn2 = 0, up = TJ_UP_SAME, lb = 0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	std::vector<ObsTjDown> dn;
	std::vector<uint32_t> pat;
	std::vector<int32_t> hi_base;
	std::vector<uint16_t> lo_rank;
};

// rank(s) among the W-bit words of n set bits, ascending = by the high half, then by the low half: hi_base (2^(W - lb) entries) and lo_rank (2^lb);
// returns lb = W / 2.  W <= 2 * kObsTjMaxHalf
inline int tj_rank_tables(int W, int n, std::vector<int32_t>& hi_base, std::vector<uint16_t>& lo_rank)
{
	const int lb = W / 2, hb = W - lb;
	std::vector<int> seen((size_t)lb + 1, 0);
	lo_rank.resize((size_t)1 << lb);
	for (uint32_t lo = 0; lo < (1u << lb); lo++) lo_rank[lo] = (uint16_t)seen[(size_t)__builtin_popcount(lo)]++;
	hi_base.resize((size_t)1 << hb);
	int64_t acc = 0;
	for (uint32_t hi = 0; hi < (1u << hb); hi++) {
		hi_base[hi] = (int32_t)acc;
		acc += binom(lb, n - __builtin_popcount(hi));
	}
	return lb;
}

// the cnt ascending words of n set bits: the patterns of a sector by rank
inline void tj_patterns(int n, int64_t cnt, std::vector<uint32_t>& pat)
{
	pat.clear();
	pat.reserve((size_t)cnt);
	uint64_t w = first_word(n);
	for (int64_t i = 0; i < cnt; i++) {
		pat.push_back((uint32_t)w);
		if (i + 1 < cnt) w = next_word(w);
	}
}

// what the operator asks of the destination's down word d' and what the source's down word is
enum { DN_KEEP_OUT, DN_KEEP_IN, DN_ADD, DN_REMOVE }; // site not in d', source d' | site in d', source d' | not in d', source d' + site | in d', source d' - site

// false: refused, *why says why.  *has == false: the operator leads to no sector
inline bool obs_plan_tj(int op, int site, int spin, int L, int nup, int ndn, bool* has, ObsTjPlan& P, const char** why)
{
	*has = false;
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	if (!valid_op(op)) return refuse("t-J observables: unknown operator (LPP_OP_*)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return refuse("t-J observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (site < 0 || site >= L || tj_sector_size(L, nup, ndn) < 0) return refuse("t-J observables: bad sites / site / sector (nup + ndown <= sites <= 30)");
	if ((op == LPP_OP_SPLUS || op == LPP_OP_SMINUS) && spin != LPP_SPIN_UP)
		return refuse("t-J observables: splus / sminus with spin DOWN: the reference's hasNewParts names the sector (nup -+ 1, ndown +- 1) while its getBraIndex "
		              "ignores the spin and makes states of (nup +- 1, ndown -+ 1), so it ranks words that are not in the basis; pass LPP_SPIN_UP");
	P = ObsTjPlan();
	P.nup2 = nup;
	P.ndn2 = ndn;
	if (needs_new_basis(op) && !new_parts_tj(op, spin, L, nup, ndn, &P.nup2, &P.ndn2)) return true;
	const int Ws = L - ndn, Wd = L - P.ndn2; // pattern widths: the sites free of down electrons
	P.n_up_src = binom(Ws, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(Wd, P.nup2);
	P.n_dn_dst = binom(L, P.ndn2);
	if (too_many_states(P)) return refuse("t-J observables: a species with 2^31 states or more");
	int dkind = DN_KEEP_OUT;
	bool down_sign = false;
	switch (op) {
	case LPP_OP_C:
	case LPP_OP_CDAGGER:
		if (spin == LPP_SPIN_UP) {
			P.up = (op == LPP_OP_C) ? TJ_UP_SET : TJ_UP_CLEAR;
		} else {
			P.up = (op == LPP_OP_C) ? TJ_UP_DEL0 : TJ_UP_INS0;
			dkind = (op == LPP_OP_C) ? DN_ADD : DN_REMOVE;
			down_sign = true;
		}
		break;
	case LPP_OP_N:
	case LPP_OP_SZ: // getBraSzOrN (:456-469): the occupancy of `spin` for both
		P.up = (spin == LPP_SPIN_UP) ? TJ_UP_TEST : TJ_UP_SAME;
		dkind = (spin == LPP_SPIN_UP) ? DN_KEEP_OUT : DN_KEEP_IN;
		break;
	case LPP_OP_SPLUS:
		P.up = TJ_UP_DEL1;
		dkind = DN_ADD;
		break;
	case LPP_OP_SMINUS:
		P.up = TJ_UP_INS1;
		dkind = DN_REMOVE;
		break;
	}
	if (P.up != TJ_UP_SAME) {
		if (Ws > 2 * kObsTjMaxHalf) return refuse("t-J observables: more than 24 sites free of down electrons (the pattern rank tables are kept in LDS)");
		P.lb = tj_rank_tables(Ws, nup, P.hi_base, P.lo_rank);
		tj_patterns(P.nup2, P.n_up_dst, P.pat); // the destination's patterns, ascending
	}
	const Ranker R(L);
	P.dn.assign((size_t)P.n_dn_dst, ObsTjDown { 0, 0 });
	const uint64_t bit = 1ull << site;
	uint64_t d = first_word(P.ndn2);
	for (int64_t i = 0; i < P.n_dn_dst; i++) {
		const bool in = (d & bit) != 0;
		const bool ok = (dkind == DN_KEEP_IN || dkind == DN_REMOVE) ? in : !in;
		ObsTjDown& e = P.dn[(size_t)i];
		e.p = __builtin_popcountll(~d & (bit - 1));
		if (ok) {
			const uint64_t sd = (dkind == DN_ADD || dkind == DN_REMOVE) ? (d ^ bit) : d;
			int s = 1; // doSignGf, SPIN_DOWN (:180-191): the parity of the up electrons at EVERY site, times the parity of the down bits below the site
			if (down_sign && ((nup + __builtin_popcountll(d & (bit - 1))) & 1)) s = -1;
			e.src = (int32_t)(s * (R.rank(sd) + 1));
		}
		if (i + 1 < P.n_dn_dst) d = next_word(d);
	}
	*has = true;
	return true;
}

// the plan expanded as the kernel walks it: action[dst] = +-(src + 1) or 0 (action may be null); *touched = destinations with a source
inline void tj_expand(const ObsTjPlan& P, int64_t* action, int64_t* touched)
{
	int64_t cnt = 0;
	for (int64_t dd = 0; dd < P.n_dn_dst; dd++)
		for (int64_t du = 0; du < P.n_up_dst; du++) {
			const int64_t k = obs_tj_source(P.up, P.dn[(size_t)dd], (uint32_t)du, P.pat.data(), P.hi_base.data(), P.lo_rank.data(), P.lb, P.n_up_src);
			if (action) action[du + dd * P.n_up_dst] = k;
			cnt += (k != 0);
		}
	if (touched) *touched = cnt;
}

// the same count in closed form: the destination words with the site as the operator leaves it -- empty (c), holding an up electron (cdagger, n, sz
// of the up species, splus) or a down electron (cdagger, n, sz of the down species, sminus) -- are a sector of the other L - 1 sites
inline int64_t tj_touched(int op, int spin, int L, int nup2, int ndn2)
{
	const bool up = op == LPP_OP_SPLUS || (op != LPP_OP_SMINUS && spin == LPP_SPIN_UP);
	const int a = nup2 - (op != LPP_OP_C && up), b = ndn2 - (op != LPP_OP_C && !up);
	return binom(L - 1, b) * binom(L - 1 - b, a);
}

} // namespace obs_host
} // namespace lpp
