// lpp_obs_heis_plan.h -- host-only planning of ONE operator in the S = 1/2 Heisenberg basis (BasisHeisenberg, twiceS = 1): the sector arithmetic, the
// run table and the low-word tables k_obs_apply_heis reads (lpp_obs_heis_kernels.h, where the layout is described), and obs_heis_source, the ONE
// lookup the kernel calls per element and the host expands a plan with.  Plain C++, no HIP (host/test_obs_plan.cpp).
#pragma once
#include <algorithm>

#include "lpp_obs_plan.h"

namespace lpp {

// what decides the source of a destination element inside its run
enum {
	HEIS_RUN = 0, // the run's entry alone: source = first source + position (a site in the high part; the entry's sign is the value's)
	HEIS_FLIP_SET, // site in the low part, the destination's bit must be set, the source has it cleared (splus)
	HEIS_FLIP_CLEAR, // ... must be clear, the source has it set (sminus)
	HEIS_TEST_SET, // same index where the bit is set (n, SPIN_UP)
	HEIS_TEST_CLEAR, // same index where the bit is clear (n, SPIN_DOWN)
	HEIS_SZ // same index, value 1 - 2 bit (the raw sz)
};

constexpr int kObsHeisMaxLow = 14; // lb at most: two 16-bit tables of 2^lb entries in LDS (64 KiB), ranks below C(14, 7)
struct ObsHeisRun { // 24 bytes per non-empty destination run, ascending; one closing entry with dst0 = N_dst
	int64_t dst0; // index of the run's first element
	int64_t src; // +-(index of the source run's first element + 1), 0: no element of the run is touched
	int32_t pl, wbase; // popcount p of the low part of the run's words; word[wbase + r] is the low word of popcount p and rank r
};

// destination = element r of run R -> +-(source index + 1), 0 = the reference does not touch it.  word / rank wherever the caller keeps them.
LPP_OBS_LOOKUP int64_t obs_heis_source(int mode, const ObsHeisRun& R, int64_t r, uint32_t bit, const uint16_t* word, const uint16_t* rank)
{
	if (R.src == 0) return 0;
	if (mode == HEIS_RUN) return R.src < 0 ? R.src - r : R.src + r;
	const uint32_t w = word[R.wbase + (int32_t)r];
	const bool set = (w & bit) != 0;
	switch (mode) {
	case HEIS_FLIP_SET:
	case HEIS_FLIP_CLEAR:
		if (set != (mode == HEIS_FLIP_SET)) return 0;
		return R.src + (int64_t)rank[w ^ bit];
	case HEIS_TEST_SET:
		return set ? R.src + r : 0;
	case HEIS_TEST_CLEAR:
		return set ? 0 : R.src + r;
	default: // HEIS_SZ
		return set ? -(R.src + r) : R.src + r;
	}
}

namespace obs_host {

constexpr int kHeisMaxSites = kBinomMax; // as lpp_engine_assemble_heisenberg admits
constexpr int64_t kHeisMaxRuns = (int64_t)1 << 22; // entries of the run table (24 bytes each)

inline int64_t heis_sector_size(int L, int m, int) { return (L < 1 || L > kHeisMaxSites || m < 0 || m > L) ? -1 : binom(L, m); }

// Heisenberg::hasNewPartsSplusOrMinus (Heisenberg.h:218-240): szPlusConst +- 1, reported as (szPlusConst', 0).  false: S+ on all ups, S- on all downs --
// the reference THROWS there (:239), and so it does for every other operator but sz (:129-133); the callers turn false into LPP_ERR_INVALID.
inline bool new_parts_heis(int op, int, int L, int m, int, int* n1, int* n2)
{
	if (op != LPP_OP_SPLUS && op != LPP_OP_SMINUS) return false;
	const int m2 = m + (op == LPP_OP_SPLUS ? 1 : -1);
	if (m2 < 0 || m2 > L) return false;
	*n1 = m2;
	*n2 = 0;
	return true;
}

// the low part of the word: 12 bits (two 16-bit tables of 4096 entries = 16 KiB of LDS, several workgroups per CU), more for long chains so that the
// run table stays small
inline int heis_low_bits(int L) { return std::min(L, std::max(12, std::min(kObsHeisMaxLow, L - 20))); }

// index of the first word with high part h among the L-bit words of k set bits: the words below h << lb
inline int64_t heis_run_start(uint64_t h, int hb, int lb, int k)
{
	int64_t n = 0;
	int c = 0;
	for (int b = hb - 1; b >= 0; b--)
		if ((h >> b) & 1) n += binom(b + lb, k - c++);
	return n;
}

// the high parts of the non-empty runs of sector m2, ascending: those whose popcount leaves 0 .. lb set bits to the low part.  false: more than kHeisMaxRuns
inline bool heis_highs(int hb, int lb, int m2, std::vector<uint64_t>& highs)
{
	const int p_lo = std::max(0, m2 - lb), p_hi = std::min(hb, m2);
	int64_t nruns = 0;
	for (int p = p_lo; p <= p_hi && nruns <= kHeisMaxRuns; p++) nruns += binom(hb, p);
	if (nruns > kHeisMaxRuns) return false;
	highs.clear();
	highs.reserve((size_t)nruns);
	if (hb <= 22) {
		for (uint64_t h = 0; h < (1ull << hb); h++) {
			const int p = __builtin_popcountll(h);
			if (p >= p_lo && p <= p_hi) highs.push_back(h);
		}
	} else { // few of very many: class by class, then sorted
		for (int p = p_lo; p <= p_hi; p++) {
			uint64_t h = first_word(p);
			for (int64_t i = 0, cnt = binom(hb, p); i < cnt; i++) {
				highs.push_back(h);
				if (i + 1 < cnt) h = next_word(h);
			}
		}
		std::sort(highs.begin(), highs.end());
	}
	return true;
}

// word[base[p] + r]: the lb-bit word of popcount p and rank r; base has lb + 2 entries
inline void heis_low_base(int lb, std::vector<int32_t>& base)
{
	base.assign((size_t)lb + 2, 0);
	for (int p = 0; p <= lb; p++) base[(size_t)p + 1] = base[(size_t)p] + (int32_t)binom(lb, p);
}

// the two low tables: the lb-bit words ordered by (popcount, rank), and the rank of every lb-bit word among the words of its popcount
inline void heis_low_tables(int lb, const std::vector<int32_t>& base, std::vector<uint16_t>& word, std::vector<uint16_t>& rank)
{
	word.resize((size_t)1 << lb);
	rank.resize((size_t)1 << lb);
	std::vector<int32_t> seen((size_t)lb + 1, 0);
	for (uint32_t w = 0; w < (1u << lb); w++) {
		const int p = __builtin_popcount(w);
		rank[w] = (uint16_t)seen[(size_t)p];
		word[(size_t)(base[(size_t)p] + seen[(size_t)p]++)] = (uint16_t)w;
	}
}

struct ObsHeisPlan {
	int m2 = 0, mode = HEIS_RUN, lb = 0;
	uint32_t bit = 0;
	int64_t n_src = 0, n_dst = 0;
	std::vector<ObsHeisRun> runs; // one closing entry at the end
	std::vector<uint16_t> word, rank; // empty for HEIS_RUN
};

// false: refused, *why says why (this basis has no "no sector": the plan refuses where the reference throws)
inline bool obs_plan_heis(int op, int site, int spin, int L, int m, ObsHeisPlan& P, const char** why)
{
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	if (!valid_op(op)) return refuse("Heisenberg observables: unknown operator (LPP_OP_*)");
	if (op == LPP_OP_C || op == LPP_OP_CDAGGER) return refuse("Heisenberg observables: c / cdagger are no operators of this model (the reference throws)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return refuse("Heisenberg observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (site < 0 || site >= L || heis_sector_size(L, m, 0) < 0) return refuse("Heisenberg observables: bad sites / site / sector (szPlusConst <= sites <= 62)");
	P = ObsHeisPlan();
	P.m2 = m;
	int dummy = 0;
	if (needs_new_basis(op) && !new_parts_heis(op, spin, L, m, 0, &P.m2, &dummy)) return refuse("Heisenberg observables: S+ to all ups or S- to all downs (the reference throws)");
	P.n_src = binom(L, m);
	P.n_dst = binom(L, P.m2);
	const int lb = P.lb = heis_low_bits(L), hb = L - lb;
	const bool high = site >= lb, flip = needs_new_basis(op);
	const uint64_t hbit = high ? 1ull << (site - lb) : 0;
	if (!high) {
		P.bit = 1u << site;
		P.mode = (op == LPP_OP_SPLUS) ? HEIS_FLIP_SET : (op == LPP_OP_SMINUS) ? HEIS_FLIP_CLEAR : (op == LPP_OP_SZ) ? HEIS_SZ : (spin == LPP_SPIN_UP) ? HEIS_TEST_SET : HEIS_TEST_CLEAR;
	}
	// the non-empty runs: high parts whose popcount leaves 0 .. lb set bits to the low part, ascending
	std::vector<uint64_t> highs;
	if (!heis_highs(hb, lb, P.m2, highs)) return refuse("Heisenberg observables: the sector has more than 2^22 runs of equal high part (the run table's limit)");
	std::vector<int32_t> base;
	heis_low_base(lb, base);
	P.runs.reserve(highs.size() + 1);
	int64_t acc = 0;
	for (const uint64_t h : highs) {
		const int ph = __builtin_popcountll(h), pl = P.m2 - ph;
		ObsHeisRun R { acc, 0, pl, base[(size_t)pl] };
		const bool set = (h & hbit) != 0;
		if (flip) { // the destination (bra) has the bit set for splus and clear for sminus; the source is the word with the bit flipped, in sector m
			const bool want = op == LPP_OP_SPLUS;
			if (high) {
				if (set == want) R.src = heis_run_start(h ^ hbit, hb, lb, m) + 1;
			} else if (want ? pl >= 1 : pl <= lb - 1) { // (otherwise no low word of the run has the bit as asked)
				R.src = heis_run_start(h, hb, lb, m) + 1;
			}
		} else if (!high) {
			R.src = acc + 1;
		} else if (op == LPP_OP_SZ) {
			R.src = set ? -(acc + 1) : acc + 1;
		} else if (set == (spin == LPP_SPIN_UP)) {
			R.src = acc + 1;
		}
		P.runs.push_back(R);
		acc += binom(lb, pl);
	}
	if (acc != P.n_dst) return refuse("Heisenberg observables: internal error, the runs do not add up to the sector");
	P.runs.push_back(ObsHeisRun { P.n_dst, 0, 0, 0 });
	if (P.mode != HEIS_RUN) heis_low_tables(lb, base, P.word, P.rank);
	return true;
}

// the plan expanded as the kernel walks it (action may be null); *touched = destinations with a source
inline void heis_expand(const ObsHeisPlan& P, int64_t* action, int64_t* touched)
{
	int64_t cnt = 0;
	for (size_t k = 0; k + 1 < P.runs.size(); k++) {
		const ObsHeisRun& R = P.runs[k];
		for (int64_t r = 0, len = P.runs[k + 1].dst0 - R.dst0; r < len; r++) {
			const int64_t s = obs_heis_source(P.mode, R, r, P.bit, P.word.data(), P.rank.data());
			if (action) action[R.dst0 + r] = s;
			cnt += (s != 0);
		}
	}
	if (touched) *touched = cnt;
}

// the same count in closed form: sz touches every destination; splus / sminus / n those with the site's bit as asked, the other L - 1 bits are free
inline int64_t heis_touched(int op, int spin, int L, int m2)
{
	const bool bit_set = op == LPP_OP_SPLUS || (op == LPP_OP_N && spin == LPP_SPIN_UP);
	return (op == LPP_OP_SZ) ? binom(L, m2) : binom(L - 1, bit_set ? m2 - 1 : m2);
}

} // namespace obs_host
} // namespace lpp
