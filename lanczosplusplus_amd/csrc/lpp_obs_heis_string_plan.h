// lpp_obs_heis_string_plan.h -- host-only planning of operator strings in the S = 1/2 Heisenberg basis (BasisHeisenberg, twiceS = 1): a PRODUCT of n,
// sz, splus, sminus composed into five bit masks and a sign (no tables at all), the per-run source entries the kernels read
// (lpp_obs_heis_string_kernels.h), their packing into the slots of one upload (heis_string_pack) and obs_heis_string_source, the ONE lookup the
// kernels call per element and the host expands a plan with.
// Plain C++, no HIP (host/test_heis_string_plan.cpp).  The run structure, the low tables and the sector arithmetic are lpp_obs_heis_plan.h's.
//
// Engine::manyPoint (reference src/Engine/Engine.h:341-389) chains accModifiedState_ with factor 1; for this basis every step either flips the site's
// bit where it is clear (splus) or set (sminus) with value 1, or keeps the word with value bit / 1 - bit (n) or 1 - 2 bit (sz); there is no sign
// (BasisHeisenberg.h:123-139, :230-280).  Walking the string once with f = the sites flipped so far, the bit an operator meets is b ^ f with b the
// SOURCE word's bit, so the whole string is
//     result[d] = sign * (-1)^popcount((d ^ flip) & zmask) * src[rank(d ^ flip)]   where ((d ^ flip) & need) == want,   0 elsewhere.
// DEVIATIONS from the reference, both where it is ill-defined: n and sz act in the sector the string has reached (getNeededBasis :397-400 hands them
// the original sector's basis), and S- is refused when the CURRENT sector is the all-down one (Heisenberg.h:233 tests the original szPlusConst and
// otherwise wraps an unsigned number).
#pragma once
#include <algorithm>

#include "lpp_obs_heis_plan.h"
#include "lpp_obs_string_plan.h"

namespace lpp {

// the low lb bits of a string's masks: what the kernel evaluates per element; all zero: the run's entry alone decides (no tables are staged)
struct ObsHeisStringLow {
	uint32_t flip, need, want, zmask;
};
LPP_OBS_LOOKUP bool obs_heis_string_low_work(const ObsHeisStringLow& S) { return (S.flip | S.need | S.zmask) != 0; }

// destination = element r of a run whose low words are w (the DESTINATION's low word; not read without low work) -> +-(source index + 1), 0 = the
// string does not reach it.  src: the run's entry, +-(first index of the source run + 1) or 0; rank wherever the caller keeps it.
LPP_OBS_LOOKUP int64_t obs_heis_string_source(const ObsHeisStringLow& S, int64_t src, int64_t r, uint32_t w, const uint16_t* rank)
{
	if (src == 0) return 0;
	bool neg = src < 0;
	int64_t pos = r;
	if (obs_heis_string_low_work(S)) {
		w ^= S.flip; // the source's low word
		if ((w & S.need) != S.want) return 0;
		if (S.flip) pos = (int64_t)rank[w];
		if (__builtin_popcount(w & S.zmask) & 1) neg = !neg;
	}
	const int64_t a = (src < 0 ? -src : src) + pos;
	return neg ? -a : a;
}

namespace obs_host {

struct HeisStringPlan {
	int m2 = 0, lb = 0, sign = 1;
	bool dead = false; // two conditions on one site contradict each other: identically zero
	uint64_t flip = 0, need = 0, want = 0, zmask = 0;
	int64_t n_src = 0, n_dst = 0;
	ObsHeisStringLow low() const
	{
		const uint32_t lm = (uint32_t)((1ull << lb) - 1);
		return ObsHeisStringLow { (uint32_t)flip & lm, (uint32_t)need & lm, (uint32_t)want & lm, (uint32_t)zmask & lm };
	}
};

// the masks of ops[0 .. nops), ops[0] acting first, on sector (L; m).  false: refused, *why says why (where the reference throws: c / cdagger, S+ met in
// the all-up sector, S- met in the all-down one)
inline bool plan_heis_string(int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, int L, int m, HeisStringPlan& P, const char** why)
{
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	P = HeisStringPlan();
	if (nops < 1 || nops > kObsStringMaxOps) return refuse("Heisenberg operator string: 1 to 16 operators per string");
	if (!ops || !sites || !spins) return refuse("Heisenberg operator string: null argument");
	if (heis_sector_size(L, m, 0) < 0) return refuse("Heisenberg operator string: bad sites / sector (szPlusConst <= sites <= 62)");
	for (int i = 0; i < nops; i++) {
		if (!valid_op(ops[i])) return refuse("Heisenberg operator string: unknown operator (LPP_OP_*)");
		if (ops[i] == LPP_OP_C || ops[i] == LPP_OP_CDAGGER) return refuse("Heisenberg operator string: c / cdagger are no operators of this model (the reference throws)");
		if (spins[i] != LPP_SPIN_UP && spins[i] != LPP_SPIN_DOWN) return refuse("Heisenberg operator string: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
		if (sites[i] < 0 || sites[i] >= L) return refuse("Heisenberg operator string: site out of range");
	}
	int cur = m;
	uint64_t f = 0; // sites flipped an odd number of times so far
	for (int i = 0; i < nops; i++) {
		const int op = ops[i];
		const uint64_t bit = 1ull << sites[i];
		const bool flipped = (f & bit) != 0;
		if (op == LPP_OP_SZ) { // (-1)^(b ^ f)
			P.zmask ^= bit;
			if (flipped) P.sign = -P.sign;
			continue;
		}
		// the bit the operator meets, b ^ f, must be: splus 0, sminus 1, n UP 1, n DOWN 0
		const bool meets = (op == LPP_OP_SMINUS) || (op == LPP_OP_N && spins[i] == LPP_SPIN_UP);
		const bool b = meets != flipped; // ... so the source's bit must be
		if (P.need & bit) {
			if (((P.want & bit) != 0) != b) P.dead = true; // the first condition stays
		} else {
			P.need |= bit;
			if (b) P.want |= bit;
		}
		if (op == LPP_OP_N) continue;
		int dummy = 0;
		if (!new_parts_heis(op, LPP_SPIN_UP, L, cur, 0, &cur, &dummy)) return refuse("Heisenberg operator string: S+ met in the all-up sector or S- in the all-down one (the reference throws)");
		f ^= bit;
	}
	P.m2 = cur;
	P.flip = f;
	P.lb = heis_low_bits(L);
	P.n_src = binom(L, m);
	P.n_dst = binom(L, cur);
	return true;
}

// the shared geometry of the destination sector m2: one entry per non-empty run { first destination index, 0, popcount of the low part, word base }
// and a closing entry, the high parts of the runs, and (tables) the two low tables.  false: the run table's limit
inline bool heis_string_runs(int L, int m2, bool tables, std::vector<ObsHeisRun>& runs, std::vector<uint64_t>& highs, std::vector<uint16_t>& word, std::vector<uint16_t>& rank)
{
	const int lb = heis_low_bits(L), hb = L - lb;
	if (!heis_highs(hb, lb, m2, highs)) return false;
	std::vector<int32_t> base;
	heis_low_base(lb, base);
	runs.clear();
	runs.reserve(highs.size() + 1);
	int64_t acc = 0;
	for (const uint64_t h : highs) {
		const int pl = m2 - __builtin_popcountll(h);
		runs.push_back(ObsHeisRun { acc, 0, pl, base[(size_t)pl] });
		acc += binom(lb, pl);
	}
	runs.push_back(ObsHeisRun { acc, 0, 0, 0 }); // acc = C(L, m2)
	if (tables) heis_low_tables(lb, base, word, rank);
	return true;
}

// per destination run (high part highs[k]) of a string that is not dead: +-(first index of the source run of h ^ flip_hi in sector m + 1), the sign
// carrying P.sign and the parity of the source's high part under zmask_hi; 0 where the high conditions fail
inline void heis_string_sources(const HeisStringPlan& P, int L, int m, const std::vector<uint64_t>& highs, int64_t* src)
{
	const int lb = P.lb, hb = L - lb;
	const uint64_t fh = P.flip >> lb, nh = P.need >> lb, wh = P.want >> lb, zh = P.zmask >> lb;
	std::fill(src, src + highs.size(), (int64_t)0);
	if (P.dead) return;
	const bool same = fh == 0 && P.m2 == m; // the source run is the destination run: its start is the running sum of the run lengths
	int64_t acc = 0;
	for (size_t k = 0; k < highs.size(); k++) {
		const uint64_t hs = highs[k] ^ fh;
		const int pl = m - __builtin_popcountll(hs); // set bits the source's low part has
		const int64_t here = acc;
		if (same) acc += binom(lb, pl);
		if ((hs & nh) != wh || pl < 0 || pl > lb) continue;
		const int64_t first = (same ? here : heis_run_start(hs, hb, lb, m)) + 1;
		src[k] = ((P.sign < 0) != ((__builtin_popcountll(hs & zh) & 1) != 0)) ? -first : first;
	}
}

inline void heis_string_sources(const HeisStringPlan& P, int L, int m, const std::vector<uint64_t>& highs, std::vector<int64_t>& src)
{
	src.resize(highs.size());
	heis_string_sources(P, L, m, highs, src.data());
}

// What a launch of plans[0 .. ns) of source sector m uploads, packed on the host: slot s of `entries` (highs.size() entries each) takes the source
// entries of plans[s], low[s] its low descriptor; *low_work: whether any of them has low-part work (none: the kernels stage no tables).
// false, and nothing written: more plans than `entries` has slots, or a dead plan (nothing is launched for those)
inline bool heis_string_pack(const HeisStringPlan* plans, int ns, int L, int m, const std::vector<uint64_t>& highs, std::vector<int64_t>& entries, ObsHeisStringLow* low,
                             bool* low_work, const char** why)
{
	bool fits = ns >= 0 && (size_t)ns * highs.size() <= entries.size();
	for (int s = 0; s < ns && fits; s++) fits = !plans[s].dead;
	if (!fits) {
		*why = "Heisenberg operator string: more plans than the upload has slots, or a dead plan among them";
		return false;
	}
	*low_work = false;
	for (int s = 0; s < ns; s++) {
		heis_string_sources(plans[s], L, m, highs, entries.data() + (size_t)s * highs.size());
		low[s] = plans[s].low();
		*low_work = *low_work || obs_heis_string_low_work(low[s]);
	}
	return true;
}

// the plan expanded as the kernels walk it; word / rank may be empty without low work
inline void heis_string_expand(const HeisStringPlan& P, const std::vector<ObsHeisRun>& runs, const std::vector<int64_t>& src, const std::vector<uint16_t>& word,
                               const std::vector<uint16_t>& rank, int64_t* action)
{
	const ObsHeisStringLow S = P.low();
	const bool low = obs_heis_string_low_work(S);
	for (size_t k = 0; k + 1 < runs.size(); k++)
		for (int64_t r = 0, len = runs[k + 1].dst0 - runs[k].dst0; r < len; r++)
			action[runs[k].dst0 + r] = obs_heis_string_source(S, src[k], r, low ? word[(size_t)(runs[k].wbase + r)] : 0u, rank.data());
}

// destinations the string reaches: the conditioned bits are fixed in the source word, the others are free
inline int64_t heis_string_touched(const HeisStringPlan& P, int L, int m)
{
	return P.dead ? 0 : binom(L - __builtin_popcountll(P.need), m - __builtin_popcountll(P.want));
}

} // namespace obs_host
} // namespace lpp
