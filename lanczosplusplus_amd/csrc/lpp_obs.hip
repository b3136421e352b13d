// lpp_obs.hip -- ground-state observables of the Hubbard product basis, of the one-orbital t-J basis and of the S = 1/2 Heisenberg basis (one body per entry point, ObsBasis) on one GPU: one-site operators applied to device vectors
// (Engine::accModifiedState_, reference src/Engine/Engine.h:416-458), the two-point matrix (Engine::twoPoint :266-338) and the modified
// state + decomposition of one spectral-function type (Engine::spectralFunction :134-206, getModifiedState :494-533, calcSpectral :460-490).
//
// Host part (no GPU): sector arithmetic (HubbardOneOrbital::hasNewParts, HubbardOneOrbital.h:87-109,212-253), the per-species tables the
// kernel of lpp_obs_kernels.h reads, and the continued-fraction evaluator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "lpp_engine_impl.h"
#include "lpp_obs_kernels.h"
#include "lpp_obs_string_plan.h"
#include "lpp_obs_string_kernels.h"
#include "lpp_obs_tj_kernels.h"
#include "lpp_obs_heis_kernels.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

// needs_new_basis, valid_op, binom, new_parts (HubbardOneOrbital::hasNewParts), Ranker (BasisOneSpin::perfectIndex): lpp_obs_string_plan.h

enum { SP_C, SP_CDAGGER, SP_N };

// one species: destination rank -> +-(source rank + 1) or 0.  kind: what the operator does to the KET word (BasisOneSpin::getBra :121-149);
// with_sign: the parity of the ket's bits below `site` (doSignGf :112-136 for ind > 0 and both species; ProgramGlobals::doSign :109-114)
void species_table(const Ranker& R, int L, int n_dst, int kind, int site, bool with_sign, int global_sign, std::vector<int32_t>& tab)
{
	const int64_t cnt = binom(L, n_dst);
	tab.assign((size_t)cnt, 0);
	if (cnt == 0) return;
	const uint64_t bit = 1ull << site;
	uint64_t w = (n_dst == 0) ? 0 : ((1ull << n_dst) - 1);
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
		if (n_dst > 0 && i + 1 < cnt) { // next word of the same popcount (BasisOneSpin.h:53-61)
			const uint64_t c = w & (~w + 1), r = w + c;
			w = (((r ^ w) >> 2) / c) | r;
		}
	}
}

struct ObsPlan {
	int nup2 = 0, ndn2 = 0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	bool sz = false;
	std::vector<int32_t> tu, td; // empty: the species is untouched
};

// has == false: the operator leads to no sector (hasNewParts refused)
lpp_status obs_plan(int op, int site, int spin, int L, int nup, int ndn, bool* has, ObsPlan& P)
{
	*has = false;
	if (!valid_op(op)) return fail(LPP_ERR_INVALID, "observables: unknown operator (LPP_OP_*)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (L < 1 || L > 30 || site < 0 || site >= L || nup < 0 || ndn < 0 || nup > L || ndn > L) return fail(LPP_ERR_INVALID, "observables: bad sites / site / sector");
	P = ObsPlan();
	P.nup2 = nup;
	P.ndn2 = ndn;
	if (needs_new_basis(op) && !new_parts(op, spin, L, nup, ndn, &P.nup2, &P.ndn2)) return LPP_OK;
	P.n_up_src = binom(L, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(L, P.nup2);
	P.n_dn_dst = binom(L, P.ndn2);
	if (P.n_up_src >= (int64_t)INT32_MAX - 4096 || P.n_dn_src >= (int64_t)INT32_MAX - 4096 || P.n_up_dst >= (int64_t)INT32_MAX - 4096 || P.n_dn_dst >= (int64_t)INT32_MAX - 4096)
		return fail(LPP_ERR_INVALID, "observables: a species with 2^31 states or more");
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
	return LPP_OK;
}

// ---- a product of one-site operators composed into ONE pair of tables (planner: lpp_obs_string_plan.h, kernels: lpp_obs_string_kernels.h) ----
lpp_status string_plan(int conv, int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int L, int nup, int ndn, StringPlan& P)
{
	const char* why = nullptr;
	if (!plan_string(conv, nops, ops, sites, spins, flags, L, nup, ndn, P, &why)) return fail(LPP_ERR_INVALID, why);
	return LPP_OK;
}

// ---- the one-orbital t-J basis (BasisTjMultiOrbLanczos; kernel and lookup: lpp_obs_tj_kernels.h) ---------------------------------------

// TjMultiOrb::hasNewParts (TjMultiOrb.h:140-159, :538-584) for c / cdagger / splus / sminus: the Hubbard rules, the spin read by splus / sminus as well,
// no (0,0) sector for either pair, and no sector with more electrons than sites
bool new_parts_tj(int op, int spin, int L, int nup, int ndn, int* n1, int* n2)
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

int64_t tj_sector_size(int L, int nup, int ndn) { return (L < 1 || L > 30 || nup < 0 || ndn < 0 || nup + ndn > L) ? -1 : binom(L, ndn) * binom(L - ndn, nup); }
int64_t hubbard_sector_size(int L, int nup, int ndn) { return (L < 1 || L > 30 || nup < 0 || ndn < 0 || nup > L || ndn > L) ? -1 : binom(L, nup) * binom(L, ndn); }

struct ObsTjPlan {
	int nup2 = 0, ndn2 = 0, up = TJ_UP_SAME, lb = 0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	std::vector<ObsTjDown> dn;
	std::vector<uint32_t> pat;
	std::vector<int32_t> hi_base;
	std::vector<uint16_t> lo_rank;
};

// what the operator asks of the destination's down word d' and what the source's down word is
enum { DN_KEEP_OUT, DN_KEEP_IN, DN_ADD, DN_REMOVE }; // site not in d', source d' | site in d', source d' | not in d', source d' + site | in d', source d' - site

lpp_status obs_plan_tj(int op, int site, int spin, int L, int nup, int ndn, bool* has, ObsTjPlan& P)
{
	*has = false;
	if (!valid_op(op)) return fail(LPP_ERR_INVALID, "t-J observables: unknown operator (LPP_OP_*)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "t-J observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (site < 0 || site >= L || tj_sector_size(L, nup, ndn) < 0) return fail(LPP_ERR_INVALID, "t-J observables: bad sites / site / sector (nup + ndown <= sites <= 30)");
	if ((op == LPP_OP_SPLUS || op == LPP_OP_SMINUS) && spin != LPP_SPIN_UP)
		return fail(LPP_ERR_INVALID, "t-J observables: splus / sminus with spin DOWN: the reference's hasNewParts names the sector (nup -+ 1, ndown +- 1) while its getBraIndex "
		                             "ignores the spin and makes states of (nup +- 1, ndown -+ 1), so it ranks words that are not in the basis; pass LPP_SPIN_UP");
	P = ObsTjPlan();
	P.nup2 = nup;
	P.ndn2 = ndn;
	if (needs_new_basis(op) && !new_parts_tj(op, spin, L, nup, ndn, &P.nup2, &P.ndn2)) return LPP_OK;
	const int Ws = L - ndn, Wd = L - P.ndn2; // pattern widths: the sites free of down electrons
	P.n_up_src = binom(Ws, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(Wd, P.nup2);
	P.n_dn_dst = binom(L, P.ndn2);
	if (P.n_up_src >= (int64_t)INT32_MAX - 4096 || P.n_dn_src >= (int64_t)INT32_MAX - 4096 || P.n_up_dst >= (int64_t)INT32_MAX - 4096 || P.n_dn_dst >= (int64_t)INT32_MAX - 4096)
		return fail(LPP_ERR_INVALID, "t-J observables: a species with 2^31 states or more");
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
		if (Ws > 2 * kObsTjMaxHalf) return fail(LPP_ERR_INVALID, "t-J observables: more than 24 sites free of down electrons (the pattern rank tables are kept in LDS)");
		// rank(s) among the Ws-bit words of nup set bits, ascending = by the high half, then by the low half
		P.lb = Ws / 2;
		const int hb = Ws - P.lb;
		std::vector<int> seen((size_t)P.lb + 1, 0);
		P.lo_rank.resize((size_t)1 << P.lb);
		for (uint32_t lo = 0; lo < (1u << P.lb); lo++) P.lo_rank[lo] = (uint16_t)seen[(size_t)__builtin_popcount(lo)]++;
		P.hi_base.resize((size_t)1 << hb);
		int64_t acc = 0;
		for (uint32_t hi = 0; hi < (1u << hb); hi++) {
			P.hi_base[hi] = (int32_t)acc;
			acc += binom(P.lb, nup - __builtin_popcount(hi));
		}
		// the destination's patterns, ascending
		P.pat.reserve((size_t)P.n_up_dst);
		uint32_t w = (P.nup2 == 0) ? 0 : ((1u << P.nup2) - 1);
		for (int64_t i = 0; i < P.n_up_dst; i++) {
			P.pat.push_back(w);
			if (P.nup2 > 0 && i + 1 < P.n_up_dst) {
				const uint32_t c = w & (~w + 1), r = w + c;
				w = (((r ^ w) >> 2) / c) | r;
			}
		}
	}
	const Ranker R(L);
	P.dn.assign((size_t)P.n_dn_dst, ObsTjDown { 0, 0 });
	const uint64_t bit = 1ull << site;
	uint64_t d = (P.ndn2 == 0) ? 0 : ((1ull << P.ndn2) - 1);
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
		if (P.ndn2 > 0 && i + 1 < P.n_dn_dst) {
			const uint64_t c = d & (~d + 1), r = d + c;
			d = (((r ^ d) >> 2) / c) | r;
		}
	}
	*has = true;
	return LPP_OK;
}

// the plan expanded as the kernel walks it: action[dst] = +-(src + 1) or 0 (action may be null); *touched = destinations with a source
void tj_expand(const ObsTjPlan& P, int64_t* action, int64_t* touched)
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

// ---- the S = 1/2 Heisenberg basis (BasisHeisenberg, twiceS = 1; kernel and lookup: lpp_obs_heis_kernels.h) --------------------------------

constexpr int kHeisMaxSites = 62; // as lpp_engine_assemble_heisenberg admits
constexpr int64_t kHeisMaxRuns = (int64_t)1 << 22; // entries of the run table (24 bytes each)

// C(n, k) in integers for n <= 62 (binom above goes through long double, which is not exact that far)
int64_t heis_binom(int n, int k)
{
	static const std::vector<int64_t> tab = [] {
		std::vector<int64_t> t((size_t)(kHeisMaxSites + 1) * (kHeisMaxSites + 1), 0);
		for (int i = 0; i <= kHeisMaxSites; i++) {
			t[(size_t)i * (kHeisMaxSites + 1)] = 1;
			for (int j = 1; j <= i; j++) t[(size_t)i * (kHeisMaxSites + 1) + j] = t[(size_t)(i - 1) * (kHeisMaxSites + 1) + j - 1] + (j <= i - 1 ? t[(size_t)(i - 1) * (kHeisMaxSites + 1) + j] : 0);
		}
		return t;
	}();
	return (n < 0 || n > kHeisMaxSites || k < 0 || k > n) ? 0 : tab[(size_t)n * (kHeisMaxSites + 1) + k];
}

int64_t heis_sector_size(int L, int m, int) { return (L < 1 || L > kHeisMaxSites || m < 0 || m > L) ? -1 : heis_binom(L, m); }

// Heisenberg::hasNewPartsSplusOrMinus (Heisenberg.h:218-240): szPlusConst +- 1, reported as (szPlusConst', 0).  false: S+ on all ups, S- on all downs --
// the reference THROWS there (:239), and so it does for every other operator but sz (:129-133); the callers turn false into LPP_ERR_INVALID.
bool new_parts_heis(int op, int, int L, int m, int, int* n1, int* n2)
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
int heis_low_bits(int L) { return std::min(L, std::max(12, std::min(kObsHeisMaxLow, L - 20))); }

// index of the first word with high part h among the L-bit words of k set bits: the words below h << lb
int64_t heis_run_start(uint64_t h, int hb, int lb, int k)
{
	int64_t n = 0;
	int c = 0;
	for (int b = hb - 1; b >= 0; b--)
		if ((h >> b) & 1) n += heis_binom(b + lb, k - c++);
	return n;
}

struct ObsHeisPlan {
	int m2 = 0, mode = HEIS_RUN, lb = 0;
	uint32_t bit = 0;
	int64_t n_src = 0, n_dst = 0;
	std::vector<ObsHeisRun> runs; // one closing entry at the end
	std::vector<uint16_t> word, rank; // empty for HEIS_RUN
};

lpp_status obs_plan_heis(int op, int site, int spin, int L, int m, ObsHeisPlan& P)
{
	if (!valid_op(op)) return fail(LPP_ERR_INVALID, "Heisenberg observables: unknown operator (LPP_OP_*)");
	if (op == LPP_OP_C || op == LPP_OP_CDAGGER) return fail(LPP_ERR_INVALID, "Heisenberg observables: c / cdagger are no operators of this model (the reference throws)");
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "Heisenberg observables: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
	if (site < 0 || site >= L || heis_sector_size(L, m, 0) < 0) return fail(LPP_ERR_INVALID, "Heisenberg observables: bad sites / site / sector (szPlusConst <= sites <= 62)");
	P = ObsHeisPlan();
	P.m2 = m;
	int dummy = 0;
	if (needs_new_basis(op) && !new_parts_heis(op, spin, L, m, 0, &P.m2, &dummy))
		return fail(LPP_ERR_INVALID, "Heisenberg observables: S+ to all ups or S- to all downs (the reference throws)");
	P.n_src = heis_binom(L, m);
	P.n_dst = heis_binom(L, P.m2);
	const int lb = P.lb = heis_low_bits(L), hb = L - lb;
	const bool high = site >= lb, flip = needs_new_basis(op);
	const uint64_t hbit = high ? 1ull << (site - lb) : 0;
	if (!high) {
		P.bit = 1u << site;
		P.mode = (op == LPP_OP_SPLUS) ? HEIS_FLIP_SET : (op == LPP_OP_SMINUS) ? HEIS_FLIP_CLEAR : (op == LPP_OP_SZ) ? HEIS_SZ : (spin == LPP_SPIN_UP) ? HEIS_TEST_SET : HEIS_TEST_CLEAR;
	}
	// the non-empty runs: high parts whose popcount leaves 0 .. lb set bits to the low part, ascending
	const int p_lo = std::max(0, P.m2 - lb), p_hi = std::min(hb, P.m2);
	int64_t nruns = 0;
	for (int p = p_lo; p <= p_hi && nruns <= kHeisMaxRuns; p++) nruns += heis_binom(hb, p);
	if (nruns > kHeisMaxRuns) return fail(LPP_ERR_INVALID, "Heisenberg observables: the sector has more than 2^22 runs of equal high part (the run table's limit)");
	std::vector<uint64_t> highs;
	highs.reserve((size_t)nruns);
	if (hb <= 22) {
		for (uint64_t h = 0; h < (1ull << hb); h++) {
			const int p = __builtin_popcountll(h);
			if (p >= p_lo && p <= p_hi) highs.push_back(h);
		}
	} else { // few of very many: class by class (the next word of the same popcount, BasisOneSpin.h:53-61), then sorted
		for (int p = p_lo; p <= p_hi; p++) {
			uint64_t h = (p == 0) ? 0 : ((1ull << p) - 1);
			for (int64_t i = 0, cnt = heis_binom(hb, p); i < cnt; i++) {
				highs.push_back(h);
				if (p > 0 && i + 1 < cnt) {
					const uint64_t c = h & (~h + 1), r = h + c;
					h = (((r ^ h) >> 2) / c) | r;
				}
			}
		}
		std::sort(highs.begin(), highs.end());
	}
	std::vector<int32_t> base((size_t)lb + 2, 0); // word[base[p] + r]
	for (int p = 0; p <= lb; p++) base[(size_t)p + 1] = base[(size_t)p] + (int32_t)heis_binom(lb, p);
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
		acc += heis_binom(lb, pl);
	}
	if (acc != P.n_dst) return fail(LPP_ERR_INVALID, "Heisenberg observables: internal error, the runs do not add up to the sector");
	P.runs.push_back(ObsHeisRun { P.n_dst, 0, 0, 0 });
	if (P.mode != HEIS_RUN) {
		P.word.resize((size_t)1 << lb);
		P.rank.resize((size_t)1 << lb);
		std::vector<int32_t> seen((size_t)lb + 1, 0);
		for (uint32_t w = 0; w < (1u << lb); w++) {
			const int p = __builtin_popcount(w);
			P.rank[w] = (uint16_t)seen[(size_t)p];
			P.word[(size_t)(base[(size_t)p] + seen[(size_t)p]++)] = (uint16_t)w;
		}
	}
	return LPP_OK;
}

// the plan expanded as the kernel walks it (action may be null); *touched = destinations with a source
void heis_expand(const ObsHeisPlan& P, int64_t* action, int64_t* touched)
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

// ---- device side ---------------------------------------------------------------------------------------------------------------------

struct DevPlan {
	ObsPlan host; // tables dropped after the upload
	bool has = false;
	int32_t *tu = nullptr, *td = nullptr;
	// the t-J basis: the plan (tables dropped after the upload likewise) and its four device tables
	ObsTjPlan tj;
	ObsTjDown* tj_dn = nullptr;
	uint32_t* tj_pat = nullptr;
	int32_t* tj_hi = nullptr;
	uint16_t* tj_lo = nullptr;
	int tj_nhi = 0, tj_nlo = 0;
	// the Heisenberg basis: the plan (the run table and the low-word tables dropped after the upload) and its three device tables
	ObsHeisPlan heis;
	ObsHeisRun* hs_runs = nullptr;
	uint16_t *hs_word = nullptr, *hs_rank = nullptr;
	int64_t hs_nruns = 0;
	int hs_nlo = 0;
};

enum { BASIS_HUBBARD = 0, BASIS_TJ = 1, BASIS_HEIS = 2 };
typedef std::tuple<int, int, int, int, int, int, int> PlanKey; // basis, operator, site, spin, sites, nup, ndown
struct ObsCache {
	std::map<PlanKey, DevPlan> plans;
	size_t heis_bytes = 0; // device bytes of the Heisenberg run tables held (24 MB each at 32 sites)
};

inline bool multi(const lpp_engine* e) { return e->has_comm && e->comm.nranks > 1; }

lpp_status refuse(const lpp_engine* e, const char* who, bool hole_major_ok = false)
{
	if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
	if (e->tj.active && !hole_major_ok) return fail(LPP_ERR_STATE, std::string(who) + ": not on a hole-major t-J engine");
	return LPP_OK;
}

void free_plan(DevPlan& D)
{
	for (void* p : { (void*)D.tu, (void*)D.td, (void*)D.tj_dn, (void*)D.tj_pat, (void*)D.tj_hi, (void*)D.tj_lo, (void*)D.hs_runs, (void*)D.hs_word, (void*)D.hs_rank })
		if (p) (void)hipFree(p);
	D.tu = D.td = nullptr;
	D.tj_dn = nullptr;
	D.tj_pat = nullptr;
	D.tj_hi = nullptr;
	D.tj_lo = nullptr;
	D.hs_runs = nullptr;
	D.hs_word = D.hs_rank = nullptr;
}

// one table to the device (at least one element is allocated); the host copy is dropped
template <typename V> hipError_t upload(V** dst, std::vector<V>& src)
{
	hipError_t err = hipMalloc((void**)dst, sizeof(V) * std::max<size_t>(src.size(), 1));
	if (err == hipSuccess && !src.empty()) err = hipMemcpy(*dst, src.data(), sizeof(V) * src.size(), hipMemcpyHostToDevice);
	if (err == hipSuccess) std::vector<V>().swap(src);
	return err;
}

// The tables of one (operator, site, spin, sites, sector), uploaded once and kept with the engine.  The key is what the caller passes -- the engine
// needs no model for lpp_engine_apply_operator -- so the cache is bounded: a density of states or a two-point matrix uses at most 2 * sites entries
// per operator; past kMaxPlans entries everything is dropped and rebuilt on demand.  The returned pointer is valid until the next get_plan.
constexpr size_t kMaxPlans = 256;
constexpr size_t kMaxHeisBytes = (size_t)1 << 30; // ... or past 1 GiB of Heisenberg run tables: a two-point sweep over 32 sites holds 0.8 GB of them

lpp_status get_plan(lpp_engine* e, int basis, int op, int site, int spin, int L, int nup, int ndn, const DevPlan** out)
{
	if (!e->obs) e->obs = new ObsCache();
	ObsCache* C = (ObsCache*)e->obs;
	if (basis == BASIS_HEIS) ndn = 0; // not read: one entry per sector
	const PlanKey key(basis, op, site, spin, L, nup, ndn);
	auto it = C->plans.find(key);
	if (it == C->plans.end()) {
		DevPlan D;
		bool has = basis == BASIS_HEIS; // (this basis has no "no sector": the plan refuses where the reference throws)
		lpp_status st = (basis == BASIS_HEIS) ? obs_plan_heis(op, site, spin, L, nup, D.heis)
		                : (basis == BASIS_TJ) ? obs_plan_tj(op, site, spin, L, nup, ndn, &has, D.tj)
		                                      : obs_plan(op, site, spin, L, nup, ndn, &has, D.host);
		if (st != LPP_OK) return st;
		D.has = has;
		if (has) {
			hipError_t err = hipSuccess;
			if (basis == BASIS_HEIS) {
				D.hs_nruns = (int64_t)D.heis.runs.size() - 1;
				D.hs_nlo = (int)D.heis.word.size();
				err = upload(&D.hs_runs, D.heis.runs);
				if (err == hipSuccess) err = upload(&D.hs_word, D.heis.word);
				if (err == hipSuccess) err = upload(&D.hs_rank, D.heis.rank);
			} else if (basis == BASIS_TJ) {
				D.tj_nhi = (int)D.tj.hi_base.size();
				D.tj_nlo = (int)D.tj.lo_rank.size();
				err = upload(&D.tj_dn, D.tj.dn);
				if (err == hipSuccess) err = upload(&D.tj_pat, D.tj.pat);
				if (err == hipSuccess) err = upload(&D.tj_hi, D.tj.hi_base);
				if (err == hipSuccess) err = upload(&D.tj_lo, D.tj.lo_rank);
			} else { // an empty table stays null: the species is untouched
				if (!D.host.tu.empty()) err = upload(&D.tu, D.host.tu);
				if (err == hipSuccess && !D.host.td.empty()) err = upload(&D.td, D.host.td);
			}
			if (err != hipSuccess) {
				free_plan(D); // the tables uploaded so far
				if (err == hipErrorOutOfMemory) {
					(void)hipGetLastError();
					return fail(LPP_ERR_NOMEM, "observables: no device memory for the operator tables");
				}
				HIP_TRY(err);
			}
		}
		const size_t run_bytes = (basis == BASIS_HEIS) ? sizeof(ObsHeisRun) * (size_t)(D.hs_nruns + 1) : 0;
		if (C->plans.size() >= kMaxPlans || C->heis_bytes + run_bytes > kMaxHeisBytes) {
			HIP_TRY(hipStreamSynchronize(e->stream)); // launches that still read the old tables
			for (auto& kv : C->plans) free_plan(kv.second);
			C->plans.clear();
			C->heis_bytes = 0;
		}
		C->heis_bytes += run_bytes;
		it = C->plans.emplace(key, D).first;
	}
	*out = &it->second;
	return LPP_OK;
}

int obs_grid(const lpp_engine* e, int64_t units)
{
	const int64_t tiles = (units + kObsTile - 1) / kObsTile;
	return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)e->num_cus * 32));
}

lpp_status check_vectors(const lpp_engine* e, double fi, const void* d_src, const void* d_dst)
{
	if (!d_src || !d_dst) return fail(LPP_ERR_INVALID, "observables: null vector");
	// the destination is written in 16-byte units; a c128 source element is read as one double2, an f64 source element as one double
	if (((uintptr_t)d_dst & 15) != 0) return fail(LPP_ERR_INVALID, "observables: the destination must be 16-byte aligned");
	if (((uintptr_t)d_src & (e->is_complex ? 15 : 7)) != 0) return fail(LPP_ERR_INVALID, "observables: the source must be aligned to its element size (8 bytes f64, 16 bytes c128)");
	if (!e->is_complex && fi != 0.0) return fail(LPP_ERR_INVALID, "observables: complex factor on a real engine");
	return LPP_OK;
}

// z (+)= factor * A src on device vectors in the basis order; *has == false: no such sector, nothing was launched
lpp_status apply_dev(lpp_engine* e, int op, int site, int spin, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc, bool* has,
                     int64_t* n_dst)
{
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, BASIS_HUBBARD, op, site, spin, L, nup, ndn, &D);
	if (st != LPP_OK) return st;
	*has = D->has;
	if (!D->has) return LPP_OK;
	const ObsPlan& P = D->host;
	if (n_dst) *n_dst = P.n_up_dst * P.n_dn_dst;
	if ((st = check_vectors(e, fi, d_src, d_dst)) != LPP_OK) return st;
	const int64_t nd = P.n_up_dst * P.n_dn_dst;
	if (nd == 0) return LPP_OK;
	ObsArgs A { D->tu, D->td, P.n_up_dst, P.n_dn_dst, P.n_up_src, P.sz ? 1 : 0, fr, fi };
	const int64_t units = e->is_complex ? nd : (nd + 1) / 2;
	const int g = obs_grid(e, units);
	if (e->is_complex) {
		if (acc) k_obs_apply<true, true><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply<true, false><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	} else {
		if (acc) k_obs_apply<false, true><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply<false, false><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	}
	HIP_TRY(hipGetLastError());
	return LPP_OK;
}

// the same in the t-J basis (k_obs_apply_tj)
lpp_status apply_dev_tj(lpp_engine* e, int op, int site, int spin, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc, bool* has,
                        int64_t* n_dst)
{
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, BASIS_TJ, op, site, spin, L, nup, ndn, &D);
	if (st != LPP_OK) return st;
	*has = D->has;
	if (!D->has) return LPP_OK;
	const ObsTjPlan& P = D->tj;
	const int64_t nd = P.n_up_dst * P.n_dn_dst;
	if (n_dst) *n_dst = nd;
	if ((st = check_vectors(e, fi, d_src, d_dst)) != LPP_OK) return st;
	if (nd == 0) return LPP_OK;
	ObsTjArgs A { D->tj_dn, D->tj_pat, D->tj_hi, D->tj_lo, P.up, P.lb, D->tj_nhi, D->tj_nlo, P.n_up_dst, P.n_dn_dst, P.n_up_src, fr, fi };
	const int64_t units = e->is_complex ? nd : (nd + 1) / 2;
	const int g = obs_grid(e, units);
	const size_t lds = obs_tj_lds_bytes(A.nhi, A.nlo);
	if (e->is_complex) {
		if (acc) k_obs_apply_tj<true, true><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply_tj<true, false><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	} else {
		if (acc) k_obs_apply_tj<false, true><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply_tj<false, false><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	}
	HIP_TRY(hipGetLastError());
	return LPP_OK;
}

// the same in the S = 1/2 Heisenberg basis (k_obs_apply_heis); nup = szPlusConst, ndown is not read
lpp_status apply_dev_heis(lpp_engine* e, int op, int site, int spin, int L, int nup, int, double fr, double fi, const void* d_src, void* d_dst, bool acc, bool* has,
                          int64_t* n_dst)
{
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, BASIS_HEIS, op, site, spin, L, nup, 0, &D);
	if (st != LPP_OK) return st;
	*has = true;
	const ObsHeisPlan& P = D->heis;
	const int64_t nd = P.n_dst;
	if (n_dst) *n_dst = nd;
	if ((st = check_vectors(e, fi, d_src, d_dst)) != LPP_OK) return st;
	ObsHeisArgs A { D->hs_runs, D->hs_word, D->hs_rank, P.mode, D->hs_nlo, P.bit, D->hs_nruns, nd, fr, fi };
	const int64_t units = e->is_complex ? nd : (nd + 1) / 2;
	const int g = obs_grid(e, units);
	const size_t lds = obs_heis_lds_bytes(A.mode, A.nlo);
	if (e->is_complex) {
		if (acc) k_obs_apply_heis<true, true><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply_heis<true, false><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	} else {
		if (acc) k_obs_apply_heis<false, true><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_apply_heis<false, false><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	}
	HIP_TRY(hipGetLastError());
	return LPP_OK;
}

// Everything the entry points below need to know about a basis: they are written once and run for every family.
struct ObsBasis {
	int id;
	bool hole_major_ok; // a hole-major t-J engine is admitted (its resident states and start vectors pass through S.perm)
	int64_t (*sector_size)(int L, int nup, int ndn); // < 0: not a sector
	bool (*new_parts)(int op, int spin, int L, int nup, int ndn, int* n1, int* n2);
	lpp_status (*apply)(lpp_engine* e, int op, int site, int spin, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc, bool* has,
	                    int64_t* n_dst);
	bool no_sector_throws; // new_parts == false is where the reference throws: LPP_ERR_INVALID instead of "no such sector"
};
const ObsBasis kHubbard { BASIS_HUBBARD, false, hubbard_sector_size, new_parts, apply_dev, false };
const ObsBasis kTj { BASIS_TJ, true, tj_sector_size, new_parts_tj, apply_dev_tj, false };
const ObsBasis kHeis { BASIS_HEIS, false, heis_sector_size, new_parts_heis, apply_dev_heis, true };

// sizes of the plan's two sectors, and (touched != null) the destinations that have a source
lpp_status plan_sizes(lpp_engine* e, const ObsBasis& B, int op, int site, int spin, int L, int nup, int ndn, bool* has, int64_t* ns, int64_t* nd, int64_t* touched)
{
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, B.id, op, site, spin, L, nup, ndn, &D);
	if (st != LPP_OK) return st;
	*has = D->has;
	if (!D->has) return LPP_OK;
	if (B.id == BASIS_HEIS) {
		*ns = D->heis.n_src;
		*nd = D->heis.n_dst;
	} else if (B.id == BASIS_TJ) {
		*ns = D->tj.n_up_src * D->tj.n_dn_src;
		*nd = D->tj.n_up_dst * D->tj.n_dn_dst;
	} else {
		*ns = D->host.n_up_src * D->host.n_dn_src;
		*nd = D->host.n_up_dst * D->host.n_dn_dst;
	}
	if (!touched) return LPP_OK;
	bool hh = false;
	if (B.id == BASIS_HEIS) { // sz touches every destination; splus / sminus / n those with the site's bit as asked: the other L - 1 bits are free
		const int m2 = D->heis.m2;
		const bool bit_set = op == LPP_OP_SPLUS || (op == LPP_OP_N && spin == LPP_SPIN_UP);
		*touched = (op == LPP_OP_SZ) ? D->heis.n_dst : heis_binom(L - 1, bit_set ? m2 - 1 : m2);
	} else if (B.id == BASIS_TJ) {
		ObsTjPlan P;
		if ((st = obs_plan_tj(op, site, spin, L, nup, ndn, &hh, P)) != LPP_OK) return st;
		tj_expand(P, nullptr, touched);
	} else {
		ObsPlan P;
		if ((st = obs_plan(op, site, spin, L, nup, ndn, &hh, P)) != LPP_OK) return st;
		int64_t cu = P.n_up_dst, cd = P.n_dn_dst;
		if (!P.tu.empty()) cu = (int64_t)std::count_if(P.tu.begin(), P.tu.end(), [](int32_t v) { return v != 0; });
		if (!P.td.empty()) cd = (int64_t)std::count_if(P.td.begin(), P.td.end(), [](int32_t v) { return v != 0; });
		*touched = cu * cd;
	}
	return LPP_OK;
}

// the operator Engine::accModifiedState applies (Engine.h:535-599): n directly, sz as n_up/2 - n_down/2, the others as given
lpp_status acc_modified_dev(lpp_engine* e, const ObsBasis& B, int op, int site, int spin, int L, int nup, int ndn, double isign, const void* d_src, void* d_dst, bool acc, bool* has)
{
	if (op == LPP_OP_SZ) {
		lpp_status st = B.apply(e, LPP_OP_N, site, LPP_SPIN_UP, L, nup, ndn, isign * 0.5, 0.0, d_src, d_dst, acc, has, nullptr);
		if (st != LPP_OK) return st;
		return B.apply(e, LPP_OP_N, site, LPP_SPIN_DOWN, L, nup, ndn, -isign * 0.5, 0.0, d_src, d_dst, true, has, nullptr);
	}
	return B.apply(e, op, site, spin, L, nup, ndn, isign, 0.0, d_src, d_dst, acc, has, nullptr);
}

int blas_blocks(int64_t n2)
{
	const int64_t b = (n2 + kBlock - 1) / kBlock;
	return (int)std::max<int64_t>(1, std::min<int64_t>(b, 2048));
}

lpp_status state_ptr(lpp_engine* e, int k, const char* who, double** p)
{
	if (k < 0 || k >= e->resident_n || !e->resident) return fail(LPP_ERR_STATE, std::string(who) + ": no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)");
	*p = e->resident + (int64_t)k * e->resident_stride;
	return LPP_OK;
}

lpp_status apply_operator_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                               double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has)
{
	if (!e || !has) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool h = false;
	st = B.apply(e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate != 0, &h, nullptr);
	*has = h ? 1 : 0;
	return st;
}

lpp_status apply_operator_host_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                                    double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has)
{
	if (!e || !has || !src || !dst) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool planned = false;
	int64_t es = 0, ed = 0;
	st = plan_sizes(e, B, op, site, spin, nsites, nup, ndown, &planned, &es, &ed, nullptr);
	if (st != LPP_OK) return st;
	*has = planned ? 1 : 0;
	if (!planned) return LPP_OK;
	const size_t ns = e->esz * (size_t)es, nd = e->esz * (size_t)ed;
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(nd, 16) + 16));
	HIP_TRY(hipMemcpyAsync(ds.p, src, ns, hipMemcpyHostToDevice, e->stream));
	if (accumulate) HIP_TRY(hipMemcpyAsync(dd.p, dst, nd, hipMemcpyHostToDevice, e->stream));
	bool h = false;
	st = B.apply(e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, ds.p, dd.p, accumulate != 0, &h, nullptr);
	if (st != LPP_OK) return st;
	HIP_TRY(hipMemcpyAsync(dst, dd.p, nd, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status bench_operator_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                               int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes)
{
	if (!e || !ms_per_launch || iters < 1 || warmup < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool planned = false;
	int64_t ns = 0, nd = 0, touched = 0;
	st = plan_sizes(e, B, op, site, spin, nsites, nup, ndown, &planned, &ns, &nd, &touched); // touched: the byte model below
	if (st != LPP_OK) return st;
	if (!planned) return fail(LPP_ERR_INVALID, std::string(who) + ": the operator leads to no sector");
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(e->esz * (size_t)ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(e->esz * (size_t)nd, 16) + 16));
	HIP_TRY(hipMemsetAsync(ds.p, 0, e->esz * (size_t)ns, e->stream));
	HIP_TRY(hipMemsetAsync(dd.p, 0, e->esz * (size_t)nd, e->stream));
	hipEvent_t t0 = nullptr, t1 = nullptr;
	HIP_TRY(hipEventCreate(&t0));
	HIP_TRY(hipEventCreate(&t1));
	bool h = false;
	for (int i = 0; i < warmup + iters && st == LPP_OK; i++) {
		if (i == warmup) (void)hipEventRecord(t0, e->stream);
		st = B.apply(e, op, site, spin, nsites, nup, ndown, 1.0, 0.0, ds.p, dd.p, true, &h, nullptr);
	}
	(void)hipEventRecord(t1, e->stream);
	hipError_t err = hipEventSynchronize(t1);
	float ms = 0;
	if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
	(void)hipEventDestroy(t0);
	(void)hipEventDestroy(t1);
	if (st != LPP_OK) return st;
	HIP_TRY(err);
	*ms_per_launch = ms / iters;
	// the issue's byte model of z += A src: destination read + write, source entries read once
	if (model_bytes) *model_bytes = (double)e->esz * (2.0 * (double)nd + (double)touched);
	return LPP_OK;
}

lpp_status two_point_body(const ObsBasis& Bs, const std::string& who, lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown,
                          int32_t bra_state, int32_t ket_state, void* result, void* trace)
{
	if (!e || !result) return fail(LPP_ERR_INVALID, who + ": null argument");
	lpp_status st = refuse(e, who.c_str(), Bs.hole_major_ok);
	if (st != LPP_OK) return st;
	if (!valid_op(op)) return fail(LPP_ERR_INVALID, who + ": unknown operator");
	if ((spin1 != 0 && spin1 != 1) || (spin2 != 0 && spin2 != 1)) return fail(LPP_ERR_INVALID, who + ": bad spin");
	const int L = nsites;
	if (Bs.sector_size(L, nup, ndown) < 0) return fail(LPP_ERR_INVALID, who + ": bad sites / sector");
	double *bra = nullptr, *ket = nullptr;
	if ((st = state_ptr(e, bra_state, who.c_str(), &bra)) != LPP_OK) return st;
	if ((st = state_ptr(e, ket_state, who.c_str(), &ket)) != LPP_OK) return st;
	if (e->resident_len != Bs.sector_size(L, nup, ndown)) return fail(LPP_ERR_INVALID, who + ": (sites, nup, ndown) is not the sector of the resident states");
	HIP_TRY(hipSetDevice(e->cfg.device));
	const int w = e->is_complex ? 2 : 1;
	double* res = (double*)result;
	for (int64_t i = 0; i < (int64_t)L * L; i++) { // Engine.h:303-305
		res[w * i] = -100.0;
		if (w == 2) res[w * i + 1] = 0.0;
	}
	if (trace) {
		((double*)trace)[0] = 0.0;
		if (w == 2) ((double*)trace)[1] = 0.0;
	}
	int nup2 = nup, ndn2 = ndown;
	if (needs_new_basis(op)) {
		if (spin1 != spin2) return fail(LPP_ERR_INVALID, "twoPoint: no support yet for off-diagonal spin when needs new basis"); // Engine.h:276-282
		if (!Bs.new_parts(op, spin1, L, nup, ndown, &nup2, &ndn2)) // no such sector: the matrix keeps its fill
			return Bs.no_sector_throws ? fail(LPP_ERR_INVALID, who + ": the operator leads to no sector, and the reference throws for this model") : LPP_OK;
	}
	const int64_t ndst = Bs.sector_size(L, nup2, ndn2);
	if (ndst <= 0) return LPP_OK;
	const int64_t stride = ((ndst * w + 1) & ~(int64_t)1) + 0; // doubles per modified vector, 16-byte aligned columns
	const int64_t ld2 = stride / 2, n2 = stride / 2;
	const bool same = (bra == ket) && (spin1 == spin2);
	// panels of bra vectors sized to the free memory; the ket vectors are one scratch vector each unless they ARE the bra vectors
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	const size_t vec_bytes = sizeof(double) * (size_t)stride;
	int64_t fit = (int64_t)((double)free_b * 0.8 / (double)vec_bytes) - 1;
	if (fit < 1) return fail(LPP_ERR_NOMEM, who + ": no room for two modified vectors");
	const int panel = (int)std::min<int64_t>(L, fit);
	DevBuf B, K, part, out;
	HIP_TRY_MEM(hipMalloc(&B.p, vec_bytes * (size_t)panel));
	HIP_TRY_MEM(hipMalloc(&K.p, vec_bytes));
	const int nb = blas_blocks(n2);
	HIP_TRY_MEM(hipMalloc(&part.p, sizeof(double) * (size_t)nb * 2 * kPanel));
	HIP_TRY_MEM(hipMalloc(&out.p, sizeof(double) * 2 * (size_t)L * (size_t)L));
	HIP_TRY(hipMemsetAsync(out.p, 0, sizeof(double) * 2 * (size_t)L * (size_t)L, e->stream));
	HIP_TRY(hipMemsetAsync(B.p, 0, vec_bytes * (size_t)panel, e->stream)); // the padding element of an odd length stays 0
	HIP_TRY(hipMemsetAsync(K.p, 0, vec_bytes, e->stream));
	bool has = false;
	for (int j0 = 0; j0 < L; j0 += panel) {
		const int nj = std::min(panel, L - j0);
		for (int j = 0; j < nj; j++) {
			st = acc_modified_dev(e, Bs, op, j0 + j, spin2, L, nup, ndown, 1.0, bra, (double*)B.p + (int64_t)j * stride, false, &has);
			if (st != LPP_OK) return st;
		}
		for (int i = 0; i < L; i++) {
			const double* xi = nullptr;
			if (same && i >= j0 && i < j0 + nj) {
				xi = (const double*)B.p + (int64_t)(i - j0) * stride;
			} else {
				st = acc_modified_dev(e, Bs, op, i, spin1, L, nup, ndown, 1.0, ket, K.p, false, &has);
				if (st != LPP_OK) return st;
				xi = (const double*)K.p;
			}
			for (int p0 = 0; p0 < nj; p0 += kPanel) {
				const int np = std::min(kPanel, nj - p0);
				const double2* v0 = (const double2*)((double*)B.p + (int64_t)p0 * stride);
				// coef_p = sum conj(v_p) x: the bra side (the left factor of modifVector2 * modifVector1) is conjugated
				if (e->is_complex) k_multi_dot<true><<<nb, kBlock, 0, e->stream>>>((const double2*)xi, v0, ld2, np, n2, (double*)part.p);
				else k_multi_dot<false><<<nb, kBlock, 0, e->stream>>>((const double2*)xi, v0, ld2, np, n2, (double*)part.p);
				k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)part.p, nb, 2 * kPanel, 2 * np, (double*)out.p + 2 * ((int64_t)i * L + j0 + p0));
			}
		}
	}
	HIP_TRY(hipGetLastError());
	std::vector<double> h(2 * (size_t)L * (size_t)L);
	HIP_TRY(hipMemcpyAsync(h.data(), out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	double tr = 0, ti = 0;
	for (int i = 0; i < L; i++)
		for (int j = 0; j < L; j++) {
			const size_t q = (size_t)i * L + j;
			res[w * q] = h[2 * q];
			if (w == 2) res[w * q + 1] = h[2 * q + 1];
			if (i == j) {
				tr += h[2 * q];
				ti += h[2 * q + 1];
			}
		}
	if (trace) {
		((double*)trace)[0] = tr;
		if (w == 2) ((double*)trace)[1] = ti;
	}
	return LPP_OK;
}

lpp_status spectral_body(const ObsBasis& B, const std::string& who, lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin,
                         double isign, int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats)
{
	if (!e || !sector || !weight || !nsteps || !a || !b) return fail(LPP_ERR_INVALID, who + ": null argument");
	lpp_status st = refuse(e, who.c_str(), B.hole_major_ok);
	if (st != LPP_OK) return st;
	if ((st = refuse(sector, (who + " (sector engine)").c_str(), B.hole_major_ok)) != LPP_OK) return st;
	if (e->cfg.device != sector->cfg.device || e->is_complex != sector->is_complex) return fail(LPP_ERR_INVALID, who + ": the sector engine must share device and dtype");
	if (!sector->has_matrix()) return fail(LPP_ERR_STATE, who + ": the sector engine has no matrix");
	double* gs = nullptr;
	if ((st = state_ptr(e, state, who.c_str(), &gs)) != LPP_OK) return st;
	const int L = nsites;
	if (B.sector_size(L, nup, ndown) < 0 || e->resident_len != B.sector_size(L, nup, ndown))
		return fail(LPP_ERR_INVALID, who + ": (sites, nup, ndown) is not the sector of the resident state");
	int nup2 = nup, ndn2 = ndown;
	if (needs_new_basis(op) && !B.new_parts(op, spin, L, nup, ndown, &nup2, &ndn2)) return fail(LPP_ERR_INVALID, who + ": the operator leads to no sector (lpp_obs_new_parts)");
	const int64_t ndst = B.sector_size(L, nup2, ndn2);
	if (ndst != sector->n_global) return fail(LPP_ERR_INVALID, who + ": the sector engine does not hold the operator's sector");
	HIP_TRY(hipSetDevice(e->cfg.device));
	const int w = e->is_complex ? 2 : 1;
	const int64_t stride = (ndst * w + 1) & ~(int64_t)1;
	DevBuf M, part;
	HIP_TRY_MEM(hipMalloc(&M.p, sizeof(double) * (size_t)stride + 16));
	const int nb = blas_blocks(stride / 2);
	HIP_TRY_MEM(hipMalloc(&part.p, sizeof(double) * (size_t)(nb + 1)));
	HIP_TRY(hipMemsetAsync(M.p, 0, sizeof(double) * (size_t)stride, e->stream));
	bool has = false;
	// getModifiedState (Engine.h:494-533): A_i gs, then isign A_j gs on top -- for i == j the state is accumulated twice
	st = B.apply(e, op, isite, spin, L, nup, ndown, 1.0, 0.0, gs, M.p, true, &has, nullptr);
	if (st != LPP_OK) return st;
	st = B.apply(e, op, jsite, spin, L, nup, ndown, isign, 0.0, gs, M.p, true, &has, nullptr);
	if (st != LPP_OK) return st;
	k_dot<<<nb, kBlock, 0, e->stream>>>((const double2*)M.p, (const double2*)M.p, stride / 2, (double*)part.p);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)part.p, nb, 1, 1, (double*)part.p + nb);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(weight, (double*)part.p + nb, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream)); // the sector engine runs on a stream of its own
	return decomposition_device_any(sector, M.p, nsteps, a, b, stats); // (a hole-major sector engine takes the vector through its permutation)
}

// ---- operator strings on the device (Hubbard product basis) -----------------------------------------------------------------------------

// t-J and Heisenberg engines set up through the Python layer or the C++ shim are refused there, by the model's name; here what the engine itself knows
lpp_status refuse_string(const lpp_engine* e, const char* who)
{
	if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
	if (e->tj.active) return fail(LPP_ERR_INVALID, std::string(who) + ": the t-J model (TjMultiOrb) is not supported, operator strings are built for the Hubbard product basis");
	return LPP_OK;
}

inline ObsString dev_string(const StringPlan& P, const int32_t* tu, const int32_t* td)
{
	ObsString S { tu, td, 0, 0, P.nsz, 0 };
	for (int k = 0; k < P.nsz; k++) ((k < 8) ? S.sz_lo : S.sz_hi) |= (uint64_t)P.sz[k] << (8 * (k & 7));
	return S;
}

// z (+)= factor * scale * string src on device vectors in the basis order.  One launch; the tables are this call's own, so it ends with a stream sync.
lpp_status apply_string_dev(lpp_engine* e, const StringPlan& P, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc)
{
	lpp_status st = check_vectors(e, fi, d_src, d_dst);
	if (st != LPP_OK) return st;
	const int64_t nd = P.n_up_dst * P.n_dn_dst;
	std::vector<uint32_t> wu, wd;
	if (P.nsz > 0) {
		species_words(L, nup, wu);
		species_words(L, ndn, wd);
	}
	const size_t ntu = P.tu.size(), ntd = P.td.size();
	std::vector<int32_t> img(ntu + ntd + wu.size() + wd.size() + 4);
	std::memcpy(img.data(), P.tu.data(), 4 * ntu);
	std::memcpy(img.data() + ntu, P.td.data(), 4 * ntd);
	if (!wu.empty()) std::memcpy(img.data() + ntu + ntd, wu.data(), 4 * wu.size());
	if (!wd.empty()) std::memcpy(img.data() + ntu + ntd + wu.size(), wd.data(), 4 * wd.size());
	DevBuf T;
	HIP_TRY_MEM(hipMalloc(&T.p, 4 * img.size()));
	HIP_TRY(hipMemcpyAsync(T.p, img.data(), 4 * img.size(), hipMemcpyHostToDevice, e->stream));
	const int32_t* d = (const int32_t*)T.p;
	ObsStringApplyArgs A { dev_string(P, d, d + ntu), (const uint32_t*)(d + ntu + ntd), (const uint32_t*)(d + ntu + ntd + wu.size()), P.n_up_dst, P.n_dn_dst, P.n_up_src,
		                   fr * P.scale, fi * P.scale };
	const int64_t units = e->is_complex ? nd : (nd + 1) / 2;
	const int g = obs_grid(e, units);
	if (e->is_complex) {
		if (acc) k_obs_string_apply<true, true><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_string_apply<true, false><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	} else {
		if (acc) k_obs_string_apply<false, true><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
		else k_obs_string_apply<false, false><<<g, kObsBlock, 0, e->stream>>>((double*)d_dst, (const double*)d_src, A);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

// strings as offsets into flat arrays: string s is entries offsets[s] .. offsets[s+1]-1
struct StringList {
	int32_t n;
	const int64_t* off;
	const int32_t *ops, *sites, *spins, *flags;
};

lpp_status check_list(const StringList& S, const char* who)
{
	if (S.n < 0 || !S.off || !S.ops || !S.sites || !S.spins) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	for (int s = 0; s < S.n; s++)
		if (S.off[s] < 0 || S.off[s + 1] - S.off[s] < 1 || S.off[s + 1] - S.off[s] > kObsStringMaxOps) return fail(LPP_ERR_INVALID, std::string(who) + ": 1 to 16 operators per string");
	return LPP_OK;
}

// The brackets of strings [first, first + count) that stay in the sector, kObsStringBatch per launch: device workspace for one batch, reused after a sync.
struct DotWork {
	DevBuf tabs, part, out;
	std::vector<int32_t> img;
	int64_t nu = 0, nd = 0;
	int grid = 1;
};

lpp_status dot_work(lpp_engine* e, int L, int nup, int ndn, int64_t nstrings, DotWork& W)
{
	W.nu = binom(L, nup);
	W.nd = binom(L, ndn);
	const int64_t n = W.nu * W.nd, units = e->is_complex ? n : (n + 1) / 2;
	W.grid = obs_grid(e, units);
	const size_t per = (size_t)(W.nu + W.nd);
	W.img.assign(per * (kObsStringBatch + 1), 0); // kObsStringBatch pairs of tables, then the two word lists
	HIP_TRY_MEM(hipMalloc(&W.tabs.p, 4 * W.img.size()));
	HIP_TRY_MEM(hipMalloc(&W.part.p, sizeof(double) * 2 * kObsStringBatch * (size_t)W.grid));
	HIP_TRY_MEM(hipMalloc(&W.out.p, sizeof(double) * 2 * (size_t)std::max<int64_t>(nstrings, 1)));
	std::vector<uint32_t> wu, wd;
	species_words(L, nup, wu);
	species_words(L, ndn, wd);
	std::memcpy(W.img.data() + per * kObsStringBatch, wu.data(), 4 * wu.size());
	std::memcpy(W.img.data() + per * kObsStringBatch + W.nu, wd.data(), 4 * wd.size());
	return LPP_OK;
}

// plans[0 .. ns) into the image and the kernel's arguments (the image is uploaded by the caller)
ObsStringDotArgs dot_args(DotWork& W, const StringPlan* plans, int ns)
{
	const size_t per = (size_t)(W.nu + W.nd);
	const int32_t* d = (const int32_t*)W.tabs.p;
	ObsStringDotArgs A {};
	for (int s = 0; s < ns; s++) {
		std::memcpy(W.img.data() + per * s, plans[s].tu.data(), 4 * (size_t)W.nu);
		std::memcpy(W.img.data() + per * s + W.nu, plans[s].td.data(), 4 * (size_t)W.nd);
		A.s[s] = dev_string(plans[s], d + per * s, d + per * s + W.nu);
	}
	A.words_up = (const uint32_t*)(d + per * kObsStringBatch);
	A.words_dn = A.words_up + W.nu;
	A.n_up = W.nu;
	A.n_dn = W.nd;
	A.partial = (double*)W.part.p;
	A.ns = ns;
	return A;
}

void launch_dot(lpp_engine* e, const DotWork& W, const ObsStringDotArgs& A, const double* bra, const double* ket, double* d_out)
{
	if (e->is_complex) k_obs_string_dot<true><<<W.grid, kObsBlock, 0, e->stream>>>(bra, ket, A);
	else k_obs_string_dot<false><<<W.grid, kObsBlock, 0, e->stream>>>(bra, ket, A);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)W.part.p, W.grid, 2 * kObsStringBatch, 2 * A.ns, d_out);
}

// result[2 s], result[2 s + 1] = re, im of conj(bra) . (string_s ket); 0 where the string leads to no sector or ends in another one (nothing launched for it)
lpp_status many_point_dev(lpp_engine* e, int conv, const StringList& S, int L, int nup, int ndn, const double* bra, const double* ket, double* result)
{
	std::vector<StringPlan> plans;
	std::vector<int> slot; // the string of each plan
	DotWork W;
	bool ready = false;
	std::vector<double> scale((size_t)S.n, 0.0);
	int launched = 0;
	auto flush = [&]() -> lpp_status {
		if (plans.empty()) return LPP_OK;
		if (!ready) {
			lpp_status st = dot_work(e, L, nup, ndn, S.n, W);
			if (st != LPP_OK) return st;
			ready = true;
		} else {
			HIP_TRY(hipStreamSynchronize(e->stream)); // the launch that still reads the tables of the batch before
		}
		const ObsStringDotArgs A = dot_args(W, plans.data(), (int)plans.size());
		HIP_TRY(hipMemcpyAsync(W.tabs.p, W.img.data(), 4 * W.img.size(), hipMemcpyHostToDevice, e->stream));
		launch_dot(e, W, A, bra, ket, (double*)W.out.p + 2 * launched);
		HIP_TRY(hipGetLastError());
		launched += (int)plans.size();
		plans.clear();
		return LPP_OK;
	};
	for (int s = 0; s < S.n; s++) {
		StringPlan P;
		const int64_t o = S.off[s];
		lpp_status st = string_plan(conv, (int)(S.off[s + 1] - o), S.ops + o, S.sites + o, S.spins + o, S.flags ? S.flags + o : nullptr, L, nup, ndn, P);
		if (st != LPP_OK) return st;
		result[2 * s] = result[2 * s + 1] = 0.0;
		if (!P.has || P.nup2 != nup || P.ndn2 != ndn) continue; // Engine.h:364, :382-383
		scale[(size_t)slot.size()] = P.scale;
		slot.push_back(s);
		plans.push_back(std::move(P));
		if ((int)plans.size() == kObsStringBatch && (st = flush()) != LPP_OK) return st;
	}
	lpp_status st = flush();
	if (st != LPP_OK) return st;
	if (launched == 0) return LPP_OK;
	std::vector<double> h(2 * (size_t)launched);
	HIP_TRY(hipMemcpyAsync(h.data(), W.out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	for (int k = 0; k < launched; k++) {
		result[2 * slot[(size_t)k]] = scale[(size_t)k] * h[2 * (size_t)k];
		result[2 * slot[(size_t)k] + 1] = scale[(size_t)k] * h[2 * (size_t)k + 1];
	}
	return LPP_OK;
}

} // namespace

namespace lpp {
void free_obs(lpp_engine* e)
{
	if (e->obs) {
		ObsCache* C = (ObsCache*)e->obs;
		for (auto& kv : C->plans) free_plan(kv.second);
		delete C;
		e->obs = nullptr;
	}
	if (e->resident) (void)hipFree(e->resident);
	e->resident = nullptr;
	e->resident_n = e->resident_cap = 0;
}
} // namespace lpp

extern "C" {

lpp_status lpp_obs_new_parts(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts: null argument");
	*has = 0;
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts: bad spin");
	if (nsites < 1 || nup < 0 || ndown < 0 || nup > nsites || ndown > nsites) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts: bad sector");
	if (op == LPP_OP_SZ) return LPP_OK; // HubbardOneOrbital.h:101-102
	if (!needs_new_basis(op)) return fail(LPP_ERR_INVALID, "hasNewParts: unsupported operator"); // the reference throws (:104-108)
	int n1 = 0, n2 = 0;
	if (!new_parts(op, spin, nsites, nup, ndown, &n1, &n2)) return LPP_OK;
	*has = 1;
	if (nup_new) *nup_new = n1;
	if (ndown_new) *ndown_new = n2;
	return LPP_OK;
}

lpp_status lpp_obs_plan(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                        int64_t* n_up_dst, int64_t* n_down_dst, int32_t* table_up, int32_t* table_down)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan: null argument");
	ObsPlan P;
	bool h = false;
	lpp_status st = obs_plan(op, site, spin, nsites, nup, ndown, &h, P);
	if (st != LPP_OK) return st;
	*has = h ? 1 : 0;
	if (!h) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (n_up_dst) *n_up_dst = P.n_up_dst;
	if (n_down_dst) *n_down_dst = P.n_dn_dst;
	for (int s = 0; s < 2; s++) {
		int32_t* out = s ? table_down : table_up;
		if (!out) continue;
		const std::vector<int32_t>& t = s ? P.td : P.tu;
		const int64_t n = s ? P.n_dn_dst : P.n_up_dst;
		for (int64_t i = 0; i < n; i++) out[i] = t.empty() ? (int32_t)(i + 1) : t[(size_t)i];
	}
	return LPP_OK;
}

lpp_status lpp_obs_string_plan(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                               int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new, double* scale, int64_t* n_up_dst, int64_t* n_down_dst,
                               int32_t* table_up, int32_t* table_down, int32_t* nsz, int32_t* sz)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_string_plan: null argument");
	*has = 0;
	StringPlan P;
	lpp_status st = string_plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P);
	if (st != LPP_OK) return st;
	*has = P.has ? 1 : 0;
	if (!P.has) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (scale) *scale = P.scale;
	if (n_up_dst) *n_up_dst = P.n_up_dst;
	if (n_down_dst) *n_down_dst = P.n_dn_dst;
	if (table_up) std::memcpy(table_up, P.tu.data(), 4 * P.tu.size());
	if (table_down) std::memcpy(table_down, P.td.data(), 4 * P.td.size());
	if (nsz) *nsz = P.nsz;
	if (sz)
		for (int k = 0; k < P.nsz; k++) {
			sz[3 * k] = P.sz[k] & 31;
			sz[3 * k + 1] = (P.sz[k] >> 5) & 1;
			sz[3 * k + 2] = (P.sz[k] >> 6) & 1;
		}
	return LPP_OK;
}

lpp_status lpp_engine_apply_string(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                   int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate,
                                   int32_t* has, int32_t* nup_new, int32_t* ndown_new)
{
	if (!e || !has) return fail(LPP_ERR_INVALID, "lpp_engine_apply_string: null argument");
	*has = 0;
	lpp_status st = refuse_string(e, "lpp_engine_apply_string");
	if (st != LPP_OK) return st;
	StringPlan P;
	if ((st = string_plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P)) != LPP_OK) return st;
	if (!P.has) return LPP_OK;
	*has = 1;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	HIP_TRY(hipSetDevice(e->cfg.device));
	return apply_string_dev(e, P, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate != 0);
}

lpp_status lpp_engine_apply_string_host(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                        int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate,
                                        int32_t* has, int32_t* nup_new, int32_t* ndown_new)
{
	if (!e || !has || !src || !dst) return fail(LPP_ERR_INVALID, "lpp_engine_apply_string_host: null argument");
	*has = 0;
	lpp_status st = refuse_string(e, "lpp_engine_apply_string_host");
	if (st != LPP_OK) return st;
	StringPlan P;
	if ((st = string_plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P)) != LPP_OK) return st;
	if (!P.has) return LPP_OK;
	*has = 1;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	HIP_TRY(hipSetDevice(e->cfg.device));
	const size_t ns = e->esz * (size_t)(P.n_up_src * P.n_dn_src), nd = e->esz * (size_t)(P.n_up_dst * P.n_dn_dst);
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(nd, 16) + 16));
	HIP_TRY(hipMemcpyAsync(ds.p, src, ns, hipMemcpyHostToDevice, e->stream));
	if (accumulate) HIP_TRY(hipMemcpyAsync(dd.p, dst, nd, hipMemcpyHostToDevice, e->stream));
	if ((st = apply_string_dev(e, P, nsites, nup, ndown, factor_re, factor_im, ds.p, dd.p, accumulate != 0)) != LPP_OK) return st;
	HIP_TRY(hipMemcpyAsync(dst, dd.p, nd, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status lpp_engine_many_point(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                 const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, double* result)
{
	const char* who = "lpp_engine_many_point";
	if (!e || !result) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse_string(e, who);
	if (st != LPP_OK) return st;
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	if ((st = check_list(S, who)) != LPP_OK) return st;
	if (hubbard_sector_size(nsites, nup, ndown) < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad sites / sector");
	double *bra = nullptr, *ket = nullptr;
	if ((st = state_ptr(e, bra_state, who, &bra)) != LPP_OK) return st;
	if ((st = state_ptr(e, ket_state, who, &ket)) != LPP_OK) return st;
	if (e->resident_len != hubbard_sector_size(nsites, nup, ndown)) return fail(LPP_ERR_INVALID, std::string(who) + ": (sites, nup, ndown) is not the sector of the resident states");
	HIP_TRY(hipSetDevice(e->cfg.device));
	return many_point_dev(e, convention, S, nsites, nup, ndown, bra, ket, result);
}

lpp_status lpp_engine_many_point_host(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                      const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, const void* bra, const void* ket, double* result)
{
	const char* who = "lpp_engine_many_point_host";
	if (!e || !result || !bra || !ket) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse_string(e, who);
	if (st != LPP_OK) return st;
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	if ((st = check_list(S, who)) != LPP_OK) return st;
	const int64_t n = hubbard_sector_size(nsites, nup, ndown);
	if (n < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad sites / sector");
	HIP_TRY(hipSetDevice(e->cfg.device));
	const size_t bytes = e->esz * (size_t)n;
	DevBuf db, dk;
	HIP_TRY_MEM(hipMalloc(&db.p, bytes + 16));
	HIP_TRY_MEM(hipMalloc(&dk.p, bytes + 16));
	HIP_TRY(hipMemcpyAsync(db.p, bra, bytes, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(dk.p, ket, bytes, hipMemcpyHostToDevice, e->stream));
	st = many_point_dev(e, convention, S, nsites, nup, ndown, (const double*)db.p, (const double*)dk.p, result);
	HIP_TRY(hipStreamSynchronize(e->stream));
	return st;
}

lpp_status lpp_engine_bench_string_dot(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                       const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes)
{
	const char* who = "lpp_engine_bench_string_dot";
	if (!e || !ms_per_launch || iters < 1 || warmup < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad argument");
	lpp_status st = refuse_string(e, who);
	if (st != LPP_OK) return st;
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	if ((st = check_list(S, who)) != LPP_OK) return st;
	if (nstrings < 1 || nstrings > kObsStringBatch) return fail(LPP_ERR_INVALID, std::string(who) + ": 1 to 8 strings (one launch)");
	const int64_t n = hubbard_sector_size(nsites, nup, ndown);
	if (n < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad sites / sector");
	std::vector<StringPlan> plans((size_t)nstrings);
	double reached = 0;
	for (int s = 0; s < nstrings; s++) {
		StringPlan& P = plans[(size_t)s];
		const int64_t o = offsets[s];
		if ((st = string_plan(convention, (int)(offsets[s + 1] - o), ops + o, sites + o, spins + o, flags ? flags + o : nullptr, nsites, nup, ndown, P)) != LPP_OK) return st;
		if (!P.has || P.nup2 != nup || P.ndn2 != ndown) return fail(LPP_ERR_INVALID, std::string(who) + ": a string that leaves the sector launches nothing");
		reached += (double)std::count_if(P.tu.begin(), P.tu.end(), [](int32_t v) { return v != 0; }) * (double)std::count_if(P.td.begin(), P.td.end(), [](int32_t v) { return v != 0; });
	}
	HIP_TRY(hipSetDevice(e->cfg.device));
	const size_t bytes = e->esz * (size_t)n;
	DevBuf db, dk;
	HIP_TRY_MEM(hipMalloc(&db.p, bytes + 16));
	HIP_TRY_MEM(hipMalloc(&dk.p, bytes + 16));
	HIP_TRY(hipMemsetAsync(db.p, 0, bytes + 16, e->stream));
	HIP_TRY(hipMemsetAsync(dk.p, 0, bytes + 16, e->stream));
	DotWork W;
	if ((st = dot_work(e, nsites, nup, ndown, nstrings, W)) != LPP_OK) return st;
	const ObsStringDotArgs A = dot_args(W, plans.data(), nstrings);
	HIP_TRY(hipMemcpyAsync(W.tabs.p, W.img.data(), 4 * W.img.size(), hipMemcpyHostToDevice, e->stream));
	hipEvent_t t0 = nullptr, t1 = nullptr;
	HIP_TRY(hipEventCreate(&t0));
	HIP_TRY(hipEventCreate(&t1));
	for (int i = 0; i < warmup + iters; i++) {
		if (i == warmup) (void)hipEventRecord(t0, e->stream);
		launch_dot(e, W, A, (const double*)db.p, (const double*)dk.p, (double*)W.out.p);
	}
	(void)hipEventRecord(t1, e->stream);
	hipError_t err = hipEventSynchronize(t1);
	float ms = 0;
	if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
	if (err == hipSuccess) err = hipGetLastError();
	(void)hipEventDestroy(t0);
	(void)hipEventDestroy(t1);
	HIP_TRY(err);
	*ms_per_launch = ms / iters;
	// bra read once, one ket element per string and destination it reaches (the tables stay in L2)
	if (model_bytes) *model_bytes = (double)e->esz * ((double)n + reached);
	return LPP_OK;
}

lpp_status lpp_obs_new_parts_tj(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_tj: null argument");
	*has = 0;
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_tj: bad spin");
	if (nsites < 1 || nup < 0 || ndown < 0 || nup + ndown > nsites) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_tj: bad sector");
	if (!needs_new_basis(op)) return fail(LPP_ERR_INVALID, "hasNewParts: unsupported operator"); // the reference throws for n and sz (TjMultiOrb.h:154-158)
	int n1 = 0, n2 = 0;
	if (!new_parts_tj(op, spin, nsites, nup, ndown, &n1, &n2)) return LPP_OK;
	*has = 1;
	if (nup_new) *nup_new = n1;
	if (ndown_new) *ndown_new = n2;
	return LPP_OK;
}

lpp_status lpp_obs_plan_tj(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                           int64_t* n_dst, int64_t* action)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan_tj: null argument");
	ObsTjPlan P;
	bool h = false;
	lpp_status st = obs_plan_tj(op, site, spin, nsites, nup, ndown, &h, P);
	if (st != LPP_OK) return st;
	*has = h ? 1 : 0;
	if (!h) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (n_dst) *n_dst = P.n_up_dst * P.n_dn_dst;
	if (action) tj_expand(P, action, nullptr);
	return LPP_OK;
}

lpp_status lpp_obs_new_parts_heis(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new)
{
	(void)ndown;
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_heis: null argument");
	*has = 0;
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_heis: bad spin");
	if (heis_sector_size(nsites, nup, 0) < 0) return fail(LPP_ERR_INVALID, "lpp_obs_new_parts_heis: bad sector");
	if (op == LPP_OP_SZ) return LPP_OK; // Heisenberg.h:122-123
	if (op != LPP_OP_SPLUS && op != LPP_OP_SMINUS) return fail(LPP_ERR_INVALID, "hasNewParts: unsupported operator"); // the reference throws (:129-133)
	int n1 = 0, n2 = 0;
	if (!new_parts_heis(op, spin, nsites, nup, 0, &n1, &n2)) return fail(LPP_ERR_INVALID, "hasNewParts: S+ to all ups or S- to all downs"); // the reference throws (:239)
	*has = 1;
	if (nup_new) *nup_new = n1;
	if (ndown_new) *ndown_new = n2;
	return LPP_OK;
}

lpp_status lpp_obs_plan_heis(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                             int64_t* n_dst, int32_t* low_bits, int64_t* action)
{
	(void)ndown;
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan_heis: null argument");
	*has = 0;
	ObsHeisPlan P;
	lpp_status st = obs_plan_heis(op, site, spin, nsites, nup, P);
	if (st != LPP_OK) return st;
	*has = 1;
	if (nup_new) *nup_new = P.m2;
	if (ndown_new) *ndown_new = 0;
	if (n_dst) *n_dst = P.n_dst;
	if (low_bits) *low_bits = P.lb;
	if (action) heis_expand(P, action, nullptr);
	return LPP_OK;
}

lpp_status lpp_continued_fraction(int32_t n, const double* a, const double* b, double eg, double weight, double sigma, double z_re, double z_im, double* out)
{
	if (n < 1 || !a || !b || !out) return fail(LPP_ERR_INVALID, "lpp_continued_fraction: bad argument");
	const std::complex<double> z(z_re, z_im);
	std::complex<double> t = z + sigma * (a[n - 1] - eg);
	for (int k = n - 2; k >= 0; k--) t = z + sigma * (a[k] - eg) - b[k] * b[k] / t; // b[k] couples levels k and k+1
	const std::complex<double> g = weight / t;
	out[0] = g.real();
	out[1] = g.imag();
	return LPP_OK;
}

lpp_status lpp_engine_apply_operator(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                     double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_body(kHubbard, "lpp_engine_apply_operator", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate, has);
}
lpp_status lpp_engine_apply_operator_tj(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                        double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_body(kTj, "lpp_engine_apply_operator_tj", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate, has);
}

lpp_status lpp_engine_apply_operator_heis(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                          double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_body(kHeis, "lpp_engine_apply_operator_heis", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate, has);
}

lpp_status lpp_engine_apply_operator_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                          double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_host_body(kHubbard, "lpp_engine_apply_operator_host", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, src, dst, accumulate, has);
}
lpp_status lpp_engine_apply_operator_tj_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                             double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_host_body(kTj, "lpp_engine_apply_operator_tj_host", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, src, dst, accumulate, has);
}

lpp_status lpp_engine_apply_operator_heis_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                               double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has)
{
	return apply_operator_host_body(kHeis, "lpp_engine_apply_operator_heis_host", e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, src, dst, accumulate, has);
}

lpp_status lpp_engine_bench_operator(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                     double* ms_per_launch, double* model_bytes)
{
	return bench_operator_body(kHubbard, "lpp_engine_bench_operator", e, op, site, spin, nsites, nup, ndown, warmup, iters, ms_per_launch, model_bytes);
}
lpp_status lpp_engine_bench_operator_tj(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                        double* ms_per_launch, double* model_bytes)
{
	return bench_operator_body(kTj, "lpp_engine_bench_operator_tj", e, op, site, spin, nsites, nup, ndown, warmup, iters, ms_per_launch, model_bytes);
}

lpp_status lpp_engine_bench_operator_heis(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                          double* ms_per_launch, double* model_bytes)
{
	return bench_operator_body(kHeis, "lpp_engine_bench_operator_heis", e, op, site, spin, nsites, nup, ndown, warmup, iters, ms_per_launch, model_bytes);
}

lpp_status lpp_engine_keep_states(lpp_engine* e, int32_t k)
{
	if (!e || k < 0) return fail(LPP_ERR_INVALID, "lpp_engine_keep_states: bad argument");
	if (e->active) return fail(LPP_ERR_STATE, "lpp_engine_keep_states: a Lanczos run is active");
	if (k > 0) {
		lpp_status st = refuse(e, "lpp_engine_keep_states");
		if (st != LPP_OK) return st;
	}
	e->keep_k = k;
	e->keep_tj = false;
	return LPP_OK;
}

lpp_status lpp_engine_keep_states_tj(lpp_engine* e, int32_t k)
{
	if (!e || k < 0) return fail(LPP_ERR_INVALID, "lpp_engine_keep_states_tj: bad argument");
	if (e->active) return fail(LPP_ERR_STATE, "lpp_engine_keep_states_tj: a Lanczos run is active");
	if (k > 0) {
		lpp_status st = refuse(e, "lpp_engine_keep_states_tj", true);
		if (st != LPP_OK) return st;
	}
	e->keep_k = k;
	e->keep_tj = true; // the solve lets a hole-major engine through (lanczos_impl)
	return LPP_OK;
}

lpp_status lpp_engine_state_device(lpp_engine* e, int32_t k, void** d_ptr, int64_t* len)
{
	if (!e || !d_ptr) return fail(LPP_ERR_INVALID, "lpp_engine_state_device: null argument");
	double* p = nullptr;
	lpp_status st = state_ptr(e, k, "lpp_engine_state_device", &p);
	if (st != LPP_OK) return st;
	*d_ptr = p;
	if (len) *len = e->resident_len;
	return LPP_OK;
}

lpp_status lpp_engine_state_to_host(lpp_engine* e, int32_t k, void* host)
{
	if (!e || !host) return fail(LPP_ERR_INVALID, "lpp_engine_state_to_host: null argument");
	double* p = nullptr;
	lpp_status st = state_ptr(e, k, "lpp_engine_state_to_host", &p);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	HIP_TRY(hipMemcpyAsync(host, p, e->esz * (size_t)e->resident_len, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status lpp_engine_two_point(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                int32_t ket_state, void* result, void* trace)
{
	return two_point_body(kHubbard, "lpp_engine_two_point", e, op, spin1, spin2, nsites, nup, ndown, bra_state, ket_state, result, trace);
}
lpp_status lpp_engine_two_point_tj(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                   int32_t ket_state, void* result, void* trace)
{
	return two_point_body(kTj, "lpp_engine_two_point_tj", e, op, spin1, spin2, nsites, nup, ndown, bra_state, ket_state, result, trace);
}

lpp_status lpp_engine_two_point_heis(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                     int32_t ket_state, void* result, void* trace)
{
	return two_point_body(kHeis, "lpp_engine_two_point_heis", e, op, spin1, spin2, nsites, nup, ndown, bra_state, ket_state, result, trace);
}

lpp_status lpp_engine_spectral_decomposition(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                             int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats)
{
	return spectral_body(kHubbard, "lpp_engine_spectral_decomposition", e, state, sector, op, isite, jsite, spin, isign, nsites, nup, ndown, weight, nsteps, a, b, stats);
}
lpp_status lpp_engine_spectral_decomposition_tj(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                                int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats)
{
	return spectral_body(kTj, "lpp_engine_spectral_decomposition_tj", e, state, sector, op, isite, jsite, spin, isign, nsites, nup, ndown, weight, nsteps, a, b, stats);
}

lpp_status lpp_engine_spectral_decomposition_heis(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                                  int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats)
{
	return spectral_body(kHeis, "lpp_engine_spectral_decomposition_heis", e, state, sector, op, isite, jsite, spin, isign, nsites, nup, ndown, weight, nsteps, a, b, stats);
}

} // extern "C"
