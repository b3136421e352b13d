// lpp_obs_heis_spin_plan.h -- host-only planning of ONE operator in the digit basis of a spin-S Heisenberg model (BasisHeisenberg.h:24-47 with any
// twiceS the assembler admits): the sector arithmetic, the run table and the low tables k_obs_apply_heis_spin reads (lpp_obs_heis_spin_kernels.h),
// the operator's value table, and obs_heis_spin_source, the ONE lookup the kernel calls per element and the host expands a plan with.
// The digit-basis counterpart of lpp_obs_heis_plan.h.  Plain C++, no HIP (host/test_heis_spin_plan.cpp).
//
// The reference throws for these spins (BasisHeisenberg.h:130,263, Heisenberg.h:223), so the operators are the project's own definition.  A word
// holds L digits of `bits` bits, site p at bit offset p * bits, digit d = m + S in [0, twiceS]; the basis is the words of digit sum szPlusConst,
// ascending.  With m = d - S of the SOURCE state:
//   splus   digit d -> d + 1, value sqrt(S(S+1) - m(m+1)); nothing leaves d = twiceS
//   sminus  digit d -> d - 1, value sqrt(S(S+1) - m(m-1)); nothing leaves d = 0
//   sz      index kept, value m (the true S^z); a value of 0 leaves the destination untouched
// n, c and cdagger are refused.
//
// Cut the word at lb low digits: the words of one high part are consecutive and ordered by their low part, so a RUN holds the lb-digit strings of
// digit sum szPlusConst - sum(high), and the position inside a run is the rank of the low string among the lb-digit strings of that sum.
#pragma once
#include <algorithm>
#include <cmath>

#include "lpp_obs_plan.h"

namespace lpp {

// what decides the source of a destination element inside its run
enum {
	HSPIN_RUN = 0, // the run's entry alone: source = first source + position, value index from the entry (a site in the high part)
	HSPIN_RAISE, // site in the low part, splus: source low code = destination code - (1 << shift), in the run of the same high part one sector down
	HSPIN_LOWER, // ... sminus: + (1 << shift), one sector up
	HSPIN_SZ // same index, the value by the site's digit
};

constexpr int kObsHeisSpinMaxLowBits = 14; // lb * bits at most: two 16-bit tables of at most 2^14 entries in LDS (64 KiB)
struct ObsHeisSpinRun { // 24 bytes per non-empty destination run, ascending; one closing entry with dst0 = N_dst
	int64_t dst0; // index of the run's first element
	int64_t src; // index of the source run's first element + 1, 0: no element of the run is touched
	int32_t wbase; // word[wbase + r] is the low string of digit sum pl and rank r
	int16_t pl; // digit sum of the low part of the run's words
	int16_t dig; // HSPIN_RUN: the SOURCE's digit at the site = the index into the value table
};

// destination = element r of run R -> source index + 1 and *vi = index into the value table, 0 = untouched.  word / rank wherever the caller
// keeps them; shift / mask: the site's digit inside the low part; top = twiceS.
LPP_OBS_LOOKUP int64_t obs_heis_spin_source(int mode, const ObsHeisSpinRun& R, int64_t r, int shift, uint32_t mask, int top, const uint16_t* word, const uint16_t* rank,
                                            int* vi)
{
	if (R.src == 0) return 0;
	if (mode == HSPIN_RUN) {
		*vi = R.dig;
		return R.src + r;
	}
	const uint32_t w = word[R.wbase + (int32_t)r];
	const int d = (int)((w >> shift) & mask);
	switch (mode) {
	case HSPIN_RAISE:
		if (d == 0) return 0;
		*vi = d - 1;
		return R.src + (int64_t)rank[w - (1u << shift)];
	case HSPIN_LOWER:
		if (d == top) return 0;
		*vi = d + 1;
		return R.src + (int64_t)rank[w + (1u << shift)];
	default: // HSPIN_SZ
		if (2 * d == top) return 0;
		*vi = d;
		return R.src + r;
	}
}

namespace obs_host {

constexpr int kHeisSpinMaxTwiceS = 4095; // digits of at most 12 bits: at least one digit below the cut, a value table of at most 4096 doubles
constexpr int64_t kHeisSpinMaxRuns = (int64_t)1 << 22; // entries of the run table (24 bytes each), the limit of lpp_obs_heis_plan.h

// the digit width the assembler uses (lpp_engine_assemble_heisenberg_spin; BasisHeisenberg.h:28-46): 1 + floor(log2(twiceS + 1)), one less for odd
// twiceS.  0: a spin the assembler refuses (odd twiceS with twiceS + 1 no power of two, bits * L > 62) or one past kHeisSpinMaxTwiceS
inline int heis_spin_bits(int L, int twiceS)
{
	if (L < 1 || twiceS < 1 || twiceS > kHeisSpinMaxTwiceS) return 0;
	int bits = 1;
	while ((2 << (bits - 1)) <= twiceS + 1) bits++;
	if (twiceS & 1) bits--;
	if ((twiceS & 1) && (1 << bits) - 1 < twiceS) return 0;
	if ((int64_t)bits * L > 62) return 0;
	return bits;
}

// cnt(l, s): the l-digit strings of digit sum s, digits 0 .. twiceS
struct HeisSpinCounts {
	int L = 0, twiceS = 0, bits = 0, sdim = 0;
	std::vector<int64_t> tab;
	bool init(int L_, int twiceS_)
	{
		bits = heis_spin_bits(L_, twiceS_);
		if (!bits) return false;
		L = L_;
		twiceS = twiceS_;
		sdim = twiceS * L + 1;
		tab.assign((size_t)(L + 1) * sdim, 0);
		tab[0] = 1;
		for (int l = 1; l <= L; l++) {
			int64_t window = 0; // sum of tab[l - 1][s - twiceS .. s]
			for (int s = 0; s < sdim; s++) {
				window += tab[(size_t)(l - 1) * sdim + s];
				if (s - twiceS - 1 >= 0) window -= tab[(size_t)(l - 1) * sdim + s - twiceS - 1];
				tab[(size_t)l * sdim + s] = window;
			}
		}
		return true;
	}
	int64_t cnt(int l, int s) const { return (l < 0 || l > L || s < 0 || s >= sdim) ? 0 : tab[(size_t)l * sdim + s]; }
};

// < 0: not a sector (a spin the assembler refuses, or a digit sum outside 0 .. L * twiceS)
inline int64_t heis_spin_sector_size(int L, int twiceS, int m)
{
	HeisSpinCounts C;
	if (!C.init(L, twiceS) || m < 0 || m > L * twiceS) return -1;
	return C.cnt(L, m);
}

// szPlusConst +- 1, reported as (twiceS, szPlusConst'); false: S+ on the top sector, S- on szPlusConst = 0, or another operator
inline bool new_parts_heis_spin(int op, int, int L, int twiceS, int m, int* t2, int* m2)
{
	if (op != LPP_OP_SPLUS && op != LPP_OP_SMINUS) return false;
	const int mm = m + (op == LPP_OP_SPLUS ? 1 : -1);
	if (mm < 0 || mm > L * twiceS) return false;
	*t2 = twiceS;
	*m2 = mm;
	return true;
}

// the operator's value by the digit of the SOURCE state, in double on the host: the kernel multiplies table entries and calls no sqrt
inline void heis_spin_values(int op, int twiceS, std::vector<double>& val)
{
	const double spin = twiceS * 0.5;
	val.assign((size_t)twiceS + 1, 0.0);
	for (int d = 0; d <= twiceS; d++) {
		const double m = d - spin;
		if (op == LPP_OP_SPLUS) val[(size_t)d] = d < twiceS ? std::sqrt(spin * (spin + 1.0) - m * (m + 1.0)) : 0.0;
		else if (op == LPP_OP_SMINUS) val[(size_t)d] = d > 0 ? std::sqrt(spin * (spin + 1.0) - m * (m - 1.0)) : 0.0;
		else val[(size_t)d] = m;
	}
}

// the non-empty runs of sector m2 when the word is cut at lb low digits: the high strings whose digit sum leaves 0 .. lb * twiceS to the low part
inline int64_t heis_spin_run_count(const HeisSpinCounts& C, int lb, int m2)
{
	int64_t n = 0;
	for (int pl = 0; pl <= lb * C.twiceS && pl <= m2; pl++) n += C.cnt(C.L - lb, m2 - pl);
	return n;
}

// the cut: lb * bits = 12 by default, more (up to 14) where the run table at 12 would pass kHeisSpinMaxRuns; 0: it passes it at 14 as well
inline int heis_spin_low_digits(const HeisSpinCounts& C, int m2)
{
	int lb = std::min(C.L, std::max(1, 12 / C.bits));
	while (heis_spin_run_count(C, lb, m2) > kHeisSpinMaxRuns) {
		if (lb >= C.L || (lb + 1) * C.bits > kObsHeisSpinMaxLowBits) return 0;
		lb++;
	}
	return lb;
}

// index of the first word with high part h among the words of digit sum m: the words below h << (lb * bits)
inline int64_t heis_spin_run_start(const HeisSpinCounts& C, uint64_t h, int hb, int lb, int m)
{
	int64_t n = 0;
	const uint64_t mask = (1ull << C.bits) - 1;
	for (int b = hb - 1; b >= 0; b--) {
		const int d = (int)((h >> (C.bits * b)) & mask);
		for (int c = 0; c < d; c++) n += C.cnt(b + lb, m - c);
		m -= d;
	}
	return n;
}

// base[s]: offset of the lb-digit strings of digit sum s in the word table; lb * twiceS + 2 entries
inline void heis_spin_low_base(const HeisSpinCounts& C, int lb, std::vector<int32_t>& base)
{
	base.assign((size_t)lb * C.twiceS + 2, 0);
	for (int s = 0; s <= lb * C.twiceS; s++) base[(size_t)s + 1] = base[(size_t)s] + (int32_t)C.cnt(lb, s);
}

// the two low tables: the lb-digit strings ordered by (digit sum, rank), and the rank of every raw low code among the strings of its digit sum (a
// code with a digit above twiceS never occurs; its entry is 0)
inline void heis_spin_low_tables(const HeisSpinCounts& C, int lb, const std::vector<int32_t>& base, std::vector<uint16_t>& word, std::vector<uint16_t>& rank)
{
	const uint32_t mask = (1u << C.bits) - 1;
	word.assign((size_t)base.back(), 0);
	rank.assign((size_t)1 << (lb * C.bits), 0);
	std::vector<int32_t> seen((size_t)lb * C.twiceS + 1, 0);
	for (uint32_t w = 0; w < (1u << (lb * C.bits)); w++) {
		int s = 0;
		bool ok = true;
		for (int p = 0; p < lb; p++) {
			const int d = (int)((w >> (p * C.bits)) & mask);
			ok = ok && d <= C.twiceS;
			s += d;
		}
		if (!ok) continue;
		rank[w] = (uint16_t)seen[(size_t)s];
		word[(size_t)(base[(size_t)s] + seen[(size_t)s]++)] = (uint16_t)w;
	}
}

struct ObsHeisSpinPlan {
	int twiceS = 0, bits = 0, m2 = 0, mode = HSPIN_RUN, lb = 0, shift = 0;
	uint32_t mask = 0;
	int64_t n_src = 0, n_dst = 0;
	std::vector<ObsHeisSpinRun> runs; // one closing entry at the end
	std::vector<uint16_t> word, rank; // empty for HSPIN_RUN; rank is empty for HSPIN_SZ as well
	std::vector<double> val; // twiceS + 1 values by the source's digit
};

// false: refused, *why says why (this basis has no "no sector": S+ on the top sector and S- on szPlusConst = 0 are refused)
inline bool obs_plan_heis_spin(int op, int site, int spin, int L, int twiceS, int m, ObsHeisSpinPlan& P, const char** why)
{
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	if (!valid_op(op)) return refuse("spin-S Heisenberg observables: unknown operator (LPP_OP_*)");
	if (op == LPP_OP_C || op == LPP_OP_CDAGGER || op == LPP_OP_N) return refuse("spin-S Heisenberg observables: the operators of this basis are sz, splus and sminus");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return refuse("spin-S Heisenberg observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	HeisSpinCounts C;
	if (!C.init(L, twiceS))
		return refuse("spin-S Heisenberg observables: bad sites / twiceS (odd twiceS needs twiceS + 1 a power of two, bits * sites <= 62, twiceS <= 4095)");
	if (site < 0 || site >= L || m < 0 || m > L * twiceS) return refuse("spin-S Heisenberg observables: bad site / sector (0 <= szPlusConst <= sites * twiceS)");
	P = ObsHeisSpinPlan();
	P.twiceS = twiceS;
	P.bits = C.bits;
	P.m2 = m;
	int t2 = 0;
	if (needs_new_basis(op) && !new_parts_heis_spin(op, spin, L, twiceS, m, &t2, &P.m2))
		return refuse("spin-S Heisenberg observables: S+ on the top sector or S- on szPlusConst = 0");
	P.n_src = C.cnt(L, m);
	P.n_dst = C.cnt(L, P.m2);
	const int lb = P.lb = heis_spin_low_digits(C, P.m2);
	if (lb == 0) return refuse("spin-S Heisenberg observables: the sector has more than 2^22 runs of equal high part (the run table's limit)");
	const int hb = L - lb, bits = C.bits;
	const bool high = site >= lb;
	const uint64_t dmask = (1ull << bits) - 1;
	P.mask = (uint32_t)dmask;
	if (!high) {
		P.shift = site * bits;
		P.mode = (op == LPP_OP_SPLUS) ? HSPIN_RAISE : (op == LPP_OP_SMINUS) ? HSPIN_LOWER : HSPIN_SZ;
	}
	heis_spin_values(op, twiceS, P.val);
	std::vector<int32_t> base;
	heis_spin_low_base(C, lb, base);
	const int hshift = high ? (site - lb) * bits : 0;
	const int low_max = lb * twiceS;
	P.runs.reserve((size_t)heis_spin_run_count(C, lb, P.m2) + 1);
	int64_t acc = 0;
	// the feasible high strings, ascending: digit by digit from the most significant one, by the digit sum that remains
	auto emit = [&](uint64_t h, int pl) {
		ObsHeisSpinRun R { acc, 0, base[(size_t)pl], (int16_t)pl, 0 };
		const int d = high ? (int)((h >> hshift) & dmask) : 0; // the destination's digit at a site in the high part
		switch (op) {
		case LPP_OP_SPLUS:
			if (high) {
				if (d >= 1) {
					R.src = heis_spin_run_start(C, h - (1ull << hshift), hb, lb, m) + 1;
					R.dig = (int16_t)(d - 1);
				}
			} else if (pl >= 1) { // (otherwise no low string of the run has a digit to come from)
				R.src = heis_spin_run_start(C, h, hb, lb, m) + 1;
			}
			break;
		case LPP_OP_SMINUS:
			if (high) {
				if (d < twiceS) {
					R.src = heis_spin_run_start(C, h + (1ull << hshift), hb, lb, m) + 1;
					R.dig = (int16_t)(d + 1);
				}
			} else if (pl + 1 <= low_max) {
				R.src = heis_spin_run_start(C, h, hb, lb, m) + 1;
			}
			break;
		default: // sz
			if (!high || 2 * d != twiceS) R.src = acc + 1;
			R.dig = (int16_t)d;
			break;
		}
		P.runs.push_back(R);
		acc += C.cnt(lb, pl);
	};
	auto walk = [&](auto&& self, int b, uint64_t h, int left) -> void { // left: the digit sum that remains for high positions b .. 0 and the low part
		if (b < 0) return emit(h, left);
		for (int d = 0; d <= twiceS && d <= left; d++)
			if (left - d <= b * twiceS + low_max) self(self, b - 1, h | ((uint64_t)d << (bits * b)), left - d); // (otherwise the rest cannot hold what remains)
	};
	walk(walk, hb - 1, 0, P.m2);
	if (acc != P.n_dst) return refuse("spin-S Heisenberg observables: internal error, the runs do not add up to the sector");
	P.runs.push_back(ObsHeisSpinRun { P.n_dst, 0, 0, 0, 0 });
	if (P.mode != HSPIN_RUN) {
		heis_spin_low_tables(C, lb, base, P.word, P.rank);
		if (P.mode == HSPIN_SZ) std::vector<uint16_t>().swap(P.rank);
	}
	return true;
}

// the plan expanded as the kernel walks it (action: source + 1 or 0, coef: the value; either may be null); *touched = destinations with a source
inline void heis_spin_expand(const ObsHeisSpinPlan& P, int64_t* action, double* coef, int64_t* touched)
{
	int64_t cnt = 0;
	for (size_t k = 0; k + 1 < P.runs.size(); k++) {
		const ObsHeisSpinRun& R = P.runs[k];
		for (int64_t r = 0, len = P.runs[k + 1].dst0 - R.dst0; r < len; r++) {
			int vi = 0;
			const int64_t s = obs_heis_spin_source(P.mode, R, r, P.shift, P.mask, P.twiceS, P.word.data(), P.rank.data(), &vi);
			if (action) action[R.dst0 + r] = s;
			if (coef) coef[R.dst0 + r] = s ? P.val[(size_t)vi] : 0.0;
			cnt += (s != 0);
		}
	}
	if (touched) *touched = cnt;
}

// the same count in closed form: the destinations whose digit at the site is not the one nothing arrives at (0 for splus, twiceS for sminus, the
// m = 0 digit for sz); the other L - 1 digits hold the rest of the sum
inline int64_t heis_spin_touched(int op, int L, int twiceS, int m2)
{
	HeisSpinCounts C;
	if (!C.init(L, twiceS)) return 0;
	const int64_t all = C.cnt(L, m2);
	if (op == LPP_OP_SPLUS) return all - C.cnt(L - 1, m2);
	if (op == LPP_OP_SMINUS) return all - C.cnt(L - 1, m2 - twiceS);
	return (twiceS & 1) ? all : all - C.cnt(L - 1, m2 - twiceS / 2);
}

} // namespace obs_host
} // namespace lpp
