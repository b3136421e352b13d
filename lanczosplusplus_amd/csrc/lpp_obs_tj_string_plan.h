// lpp_obs_tj_string_plan.h -- host-only planning of operator strings in the one-orbital t-J basis (BasisTjMultiOrbLanczos): a PRODUCT of c, cdagger,
// n, sz, splus, sminus composed into a handful of words and one short program on the up pattern, the per-down-word entries the kernels read
// (lpp_obs_tj_string_kernels.h), the packing of a launch's upload image (TjStringImage) and obs_tj_string_source, the ONE lookup the kernels call per
// element and the host expands a plan with.  Plain C++, no HIP (host/test_tj_string_plan.cpp).  Sector arithmetic, rank tables and the pattern
// primitives are lpp_obs_tj_plan.h's.
//
// Engine::manyPoint (reference src/Engine/Engine.h:341-389) chains accModifiedState_ with factor 1 through the sectors of TjMultiOrb::hasNewParts.  In
// this basis a site is empty, up or down, and every operator fully determines the state of the site it meets and the state it leaves:
//     c up: up -> empty     cdagger up: empty -> up     c down: down -> empty     cdagger down: empty -> down
//     n / sz of a spin: that spin, kept                 splus: down -> up          sminus: up -> down
// so a whole string fixes a SOURCE state and a DESTINATION state for every site it touches (a step that meets another state than the one the steps
// before left makes the string identically zero: "dead").  The signs are doSignGf's: for spin UP the parity of the up bits below the site, for spin
// DOWN the parity of all up electrons times the parity of the down bits below the site -- of the word the operator meets, which is the source word
// with the flips made so far, so each folds into a parity mask on the source word and a constant:
//     result[(u, d)] = sign * (-1)^popcount(us & par_up) * (-1)^popcount(ds & par_down) * src[index(us, ds)]
//         with us = u ^ flip_up, ds = d ^ flip_down, where (us & touched) == want_up and (ds & touched) == want_down, else 0.
// The index is rank(up compressed onto the sites free of down electrons) + rank(down) * C(L - ndown, nup), so
//   the down half  is one 32-bit entry per destination down word: +-(source down rank + 1) or 0, with the down conditions, the down parity and every
//                  constant in it (tj_string_down);
//   the up half    is a fixed sequence of pattern primitives over the touched sites in DESCENDING site order (ObsTjStringUp): at position
//                  p = popcount(~d & below(site)) of the destination's pattern test / set / clear / delete / insert a bit, which turns the
//                  destination's pattern into the source's; descending, because an insertion or deletion moves only the bits above it.  The up
//                  parity needs no word of its own: compressed onto the destination's free sites below(site) is the low p bits, so the mask is the
//                  XOR of (1 << p) - 1 over the sites with an odd number of fermionic up steps, applied to the destination's pattern; the parity of
//                  flip_up & par_up that separates it from the source's is a constant of the down entry.
// n and sz act in the sector the string has reached (the deviation of the other two families from Engine.h:397-400).
#pragma once
#include <algorithm>

#include "lpp_obs_string_plan.h"
#include "lpp_obs_tj_plan.h"

namespace lpp {

enum { TJ_UP_TEST0 = TJ_UP_INS1 + 1 }; // bit p clear, the same pattern (the site is empty in source and destination)

// the up half of a string as the kernels take it: step k = site | primitive << 5 | parity << 9, sites descending
struct ObsTjStringUp {
	int32_t n; // steps; 0: the pattern is not read
	int32_t changes; // a step other than a test: the source pattern is ranked through hi_base / lo_rank
	uint16_t step[kObsStringMaxOps];
};
constexpr int kTjStepPrim = 5, kTjStepParity = 9;

// destination (pattern word cu of rank du, down word d) -> +-(source index + 1), 0 = the string does not reach it.  dsrc: the down entry of d;
// hi_base / lo_rank (of the SOURCE sector, not read without U.changes) wherever the caller keeps them.
LPP_OBS_LOOKUP int64_t obs_tj_string_source(const ObsTjStringUp& U, int32_t dsrc, uint32_t d, uint32_t du, uint32_t cu, const int32_t* hi_base, const uint16_t* lo_rank, int lb,
                                            int64_t n_up_src)
{
	if (dsrc == 0) return 0;
	bool neg = dsrc < 0;
	const int64_t sd = (int64_t)(neg ? -dsrc : dsrc) - 1;
	int64_t su = du;
	if (U.n > 0) {
		uint32_t s = cu, par = 0;
		for (int k = 0; k < U.n; k++) {
			const uint32_t st = U.step[k], site = st & 31u, prim = (st >> kTjStepPrim) & 15u;
			const int p = __builtin_popcount(~d & ((1u << site) - 1u));
			const uint32_t bit = 1u << p, low = bit - 1u;
			if ((st >> kTjStepParity) & 1u) par ^= low;
			const bool set = (s & bit) != 0;
			switch (prim) {
			case TJ_UP_SAME:
				break;
			case TJ_UP_TEST:
			case TJ_UP_TEST0:
				if (set != (prim == TJ_UP_TEST)) return 0;
				break;
			case TJ_UP_SET:
			case TJ_UP_CLEAR:
				if (set != (prim == TJ_UP_CLEAR)) return 0;
				s ^= bit;
				break;
			case TJ_UP_DEL0:
			case TJ_UP_DEL1:
				if (set != (prim == TJ_UP_DEL1)) return 0;
				s = (s & low) | ((s >> (p + 1)) << p);
				break;
			default: // TJ_UP_INS0, TJ_UP_INS1
				s = (s & low) | ((s >> p) << (p + 1)) | (prim == TJ_UP_INS1 ? bit : 0u);
				break;
			}
		}
		if (__builtin_popcount(cu & par) & 1) neg = !neg;
		if (U.changes) su = (int64_t)hi_base[s >> lb] + (int64_t)lo_rank[s & ((1u << lb) - 1u)];
	}
	const int64_t k = su + sd * n_up_src + 1;
	return neg ? -k : k;
}

namespace obs_host {

struct TjStringPlan {
	bool has = false; // false: a step leads to no sector
	bool dead = false; // two steps contradict each other on a site: identically zero
	int L = 0, nup = 0, ndn = 0, nup2 = 0, ndn2 = 0; // the source sector, the sector the string ends in
	int sign = 1, lb = 0;
	uint32_t flip_up = 0, flip_dn = 0, touched = 0, want_up = 0, want_dn = 0, par_up = 0, par_dn = 0;
	uint32_t dst_up = 0, dst_dn = 0; // the touched sites that end up / down
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	ObsTjStringUp up = {};
};

// the words of ops[0 .. nops), ops[0] acting first, on sector (L; nup, ndn).  false: refused, *why says why.  P.has == false: no sector
inline bool obs_string_plan_tj(int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, int L, int nup, int ndn, TjStringPlan& P, const char** why)
{
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	P = TjStringPlan();
	if (nops < 1 || nops > kObsStringMaxOps) return refuse("t-J operator string: 1 to 16 operators per string");
	if (!ops || !sites || !spins) return refuse("t-J operator string: null argument");
	if (tj_sector_size(L, nup, ndn) < 0) return refuse("t-J operator string: bad sites / sector (nup + ndown <= sites <= 30)");
	for (int i = 0; i < nops; i++) {
		if (!valid_op(ops[i])) return refuse("t-J operator string: unknown operator (LPP_OP_*)");
		if (spins[i] != LPP_SPIN_UP && spins[i] != LPP_SPIN_DOWN) return refuse("t-J operator string: spin must be LPP_SPIN_UP or LPP_SPIN_DOWN");
		if (sites[i] < 0 || sites[i] >= L) return refuse("t-J operator string: site out of range");
		if ((ops[i] == LPP_OP_SPLUS || ops[i] == LPP_OP_SMINUS) && spins[i] != LPP_SPIN_UP)
			return refuse("t-J operator string: splus / sminus with spin DOWN: the reference's hasNewParts names the sector (nup -+ 1, ndown +- 1) while its getBraIndex "
			              "ignores the spin and makes states of (nup +- 1, ndown -+ 1), so it ranks words that are not in the basis; pass LPP_SPIN_UP");
	}
	if (too_many_states(binom(L, L / 2))) return refuse("t-J operator string: a species with 2^31 states or more");
	enum { EMPTY, UP, DOWN };
	int src[32] = {}, cur[32] = {};
	uint32_t fu = 0, fd = 0, odd_up = 0; // flips so far; sites with an odd number of fermionic up steps
	bool neg = false;
	int pu = nup, pd = ndn;
	for (int i = 0; i < nops; i++) {
		const int op = ops[i], site = sites[i], mine = (spins[i] == LPP_SPIN_UP) ? UP : DOWN;
		int n1 = pu, n2 = pd;
		if (needs_new_basis(op) && !new_parts_tj(op, spins[i], L, pu, pd, &n1, &n2)) return true; // no sector: has stays false
		const uint32_t bit = 1u << site, below = bit - 1u;
		int need = mine, make = mine; // n, sz: getBraSzOrN, the occupancy of the spin for both
		const bool fermion = op == LPP_OP_C || op == LPP_OP_CDAGGER;
		if (op == LPP_OP_C) make = EMPTY;
		else if (op == LPP_OP_CDAGGER) need = EMPTY; // getBraC: its own bit clear and the other species absent
		else if (op == LPP_OP_SPLUS) need = DOWN, make = UP;
		else if (op == LPP_OP_SMINUS) need = UP, make = DOWN;
		if (!(P.touched & bit)) {
			P.touched |= bit;
			src[site] = cur[site] = need;
		}
		if (cur[site] != need) P.dead = true; // (the sectors are walked to the end all the same)
		if (fermion) { // doSignGf of the word the operator meets = the source word ^ the flips so far
			if (mine == UP) {
				P.par_up ^= below;
				odd_up ^= bit;
				neg ^= (__builtin_popcount(fu & below) & 1) != 0;
			} else {
				P.par_dn ^= below;
				neg ^= ((pu + __builtin_popcount(fd & below)) & 1) != 0;
			}
		}
		cur[site] = make;
		fu = (fu & ~bit) | (((make == UP) != (src[site] == UP)) ? bit : 0u);
		fd = (fd & ~bit) | (((make == DOWN) != (src[site] == DOWN)) ? bit : 0u);
		pu = n1;
		pd = n2;
	}
	P.has = true;
	P.L = L;
	P.nup = nup;
	P.ndn = ndn;
	P.nup2 = pu;
	P.ndn2 = pd;
	P.sign = neg ? -1 : 1;
	P.flip_up = fu;
	P.flip_dn = fd;
	P.n_up_src = binom(L - ndn, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(L - pd, pu);
	P.n_dn_dst = binom(L, pd);
	for (int site = L - 1; site >= 0; site--) { // descending
		const uint32_t bit = 1u << site;
		if (!(P.touched & bit)) continue;
		const int a = src[site], b = cur[site];
		if (a == UP) P.want_up |= bit;
		if (a == DOWN) P.want_dn |= bit;
		if (b == UP) P.dst_up |= bit;
		if (b == DOWN) P.dst_dn |= bit;
		// destination state b, source state a -> what turns the destination's pattern into the source's
		static const int prim[3][3] = { /* b = EMPTY */ { TJ_UP_TEST0, TJ_UP_SET, TJ_UP_DEL0 }, /* UP */ { TJ_UP_CLEAR, TJ_UP_TEST, TJ_UP_DEL1 },
			                            /* DOWN */ { TJ_UP_INS0, TJ_UP_INS1, TJ_UP_SAME } };
		const int pr = prim[b][a];
		const bool parity = (odd_up & bit) != 0;
		if (pr == TJ_UP_SAME && !parity) continue;
		if (pr != TJ_UP_SAME && pr != TJ_UP_TEST && pr != TJ_UP_TEST0) P.up.changes = 1;
		P.up.step[P.up.n++] = (uint16_t)(site | (pr << kTjStepPrim) | ((parity ? 1 : 0) << kTjStepParity));
	}
	if (P.dead) {
		P.up = ObsTjStringUp {};
		return true;
	}
	if (P.up.changes) {
		if (L - ndn > 2 * kObsTjMaxHalf) return refuse("t-J operator string: the string changes the up pattern with more than 24 sites free of down electrons (the pattern rank tables are kept in LDS)");
		P.lb = (L - ndn) / 2;
	}
	return true;
}

// per destination down word dnw[i] (the ascending words of ndn2 set bits) of a plan with a sector: +-(rank of the source down word + 1), the sign
// carrying P.sign, the parity of the source down word under par_dn and the constant that separates the up parity of the source's up word from the
// destination's; 0 where the down conditions fail, everywhere for a dead plan
inline void tj_string_down(const TjStringPlan& P, const Ranker& R, const uint32_t* dnw, int32_t* out)
{
	std::fill(out, out + P.n_dn_dst, (int32_t)0);
	if (P.dead) return;
	const bool neg0 = (P.sign < 0) != ((__builtin_popcount(P.flip_up & P.par_up) & 1) != 0);
	for (int64_t i = 0; i < P.n_dn_dst; i++) {
		const uint32_t d = dnw[i];
		if ((d & P.touched) != P.dst_dn) continue;
		const uint32_t ds = d ^ P.flip_dn;
		const int32_t k = (int32_t)(R.rank(ds) + 1);
		out[i] = (neg0 != ((__builtin_popcount(ds & P.par_dn) & 1) != 0)) ? -k : k;
	}
}

// ---- what is uploaded for a launch, packed on the host -----------------------------------------------------------------------------------

// One upload image of 32-bit words for strings from source sector (L; nup, ndn) to destination sector (nup2, ndn2): the destination's down words by
// rank (n_dn), its patterns by rank (n_up), the SOURCE sector's rank tables hi_base (nhi) and lo_rank (nlo 16-bit entries; none where the source
// sector has more than 24 free sites: no plan that changes the pattern exists there), then `slots` tables of n_dn down entries.  Offsets in words.
struct TjStringImage {
	int L = 0, nup = 0, ndn = 0, nup2 = 0, ndn2 = 0, slots = 0, lb = 0, nhi = 0, nlo = 0;
	int64_t n_dn = 0, n_up = 0, n_up_src = 0;
	size_t down_words() const { return 0; }
	size_t patterns() const { return (size_t)n_dn; }
	size_t hi_base() const { return patterns() + (size_t)n_up; }
	size_t lo_rank() const { return hi_base() + (size_t)nhi; }
	size_t entries(int s) const { return lo_rank() + (size_t)(nlo + 1) / 2 + (size_t)n_dn * (size_t)s; }
	size_t fixed() const { return entries(0); } // the words a sector uploads once
	size_t size() const { return entries(slots) + 4; }
};

// a fresh image: the geometry, the word lists and the rank tables; every slot zero.  false: not a pair of sectors
inline bool tj_string_image_begin(TjStringImage& G, int L, int nup, int ndn, int nup2, int ndn2, int slots, std::vector<int32_t>& img, const char** why)
{
	if (tj_sector_size(L, nup, ndn) < 0 || tj_sector_size(L, nup2, ndn2) < 0 || slots < 1) {
		*why = "t-J operator string: the upload image needs two sectors (nup + ndown <= sites <= 30) and a slot";
		return false;
	}
	G = TjStringImage();
	G.L = L, G.nup = nup, G.ndn = ndn, G.nup2 = nup2, G.ndn2 = ndn2, G.slots = slots;
	G.n_dn = binom(L, ndn2);
	G.n_up = binom(L - ndn2, nup2);
	G.n_up_src = binom(L - ndn, nup);
	std::vector<int32_t> hi;
	std::vector<uint16_t> lo;
	if (L - ndn <= 2 * kObsTjMaxHalf) G.lb = tj_rank_tables(L - ndn, nup, hi, lo);
	G.nhi = (int)hi.size();
	G.nlo = (int)lo.size();
	img.assign(G.size(), 0);
	std::vector<uint32_t> w;
	tj_patterns(ndn2, G.n_dn, w);
	std::copy(w.begin(), w.end(), img.begin() + (std::ptrdiff_t)G.down_words());
	tj_patterns(nup2, G.n_up, w);
	std::copy(w.begin(), w.end(), img.begin() + (std::ptrdiff_t)G.patterns());
	std::copy(hi.begin(), hi.end(), img.begin() + (std::ptrdiff_t)G.hi_base());
	for (size_t i = 0; i < lo.size(); i++) img[G.lo_rank() + i / 2] |= (int32_t)((uint32_t)lo[i] << (16 * (i & 1))); // 16-bit entries, little endian
	return true;
}

// the down entries of plans[0 .. ns) into slots 0 .. ns-1.  false, and nothing copied: more plans than slots, a plan without a sector or of other
// sectors than the image's (its entries would not be n_dn long and the kernel would rank in the wrong tables), or a dead plan (nothing is launched
// for those)
inline bool tj_string_image_entries(const TjStringImage& G, const TjStringPlan* plans, int ns, std::vector<int32_t>& img, const char** why)
{
	bool fits = ns >= 0 && ns <= G.slots && img.size() == G.size();
	for (int s = 0; s < ns && fits; s++) {
		const TjStringPlan& P = plans[s];
		fits = P.has && !P.dead && P.L == G.L && P.nup == G.nup && P.ndn == G.ndn && P.nup2 == G.nup2 && P.ndn2 == G.ndn2 && (!P.up.changes || G.nhi > 0);
	}
	if (!fits) {
		*why = "t-J operator string: more plans than the upload image has slots, or a plan that is dead or not of the image's sectors";
		return false;
	}
	const Ranker R(G.L);
	for (int s = 0; s < ns; s++) tj_string_down(plans[s], R, (const uint32_t*)(img.data() + G.down_words()), img.data() + G.entries(s));
	return true;
}

// slot s of an image expanded as the kernels walk it: action[dst] = +-(src + 1) or 0 (action may be null); *touched = destinations with a source
inline void tj_string_expand_slot(const TjStringImage& G, const std::vector<int32_t>& img, int s, const ObsTjStringUp& U, int64_t* action, int64_t* touched)
{
	const uint32_t* const dnw = (const uint32_t*)(img.data() + G.down_words());
	const uint32_t* const pat = (const uint32_t*)(img.data() + G.patterns());
	const int32_t* const ent = img.data() + G.entries(s);
	const int32_t* const hi = img.data() + G.hi_base();
	std::vector<uint16_t> lo16((size_t)G.nlo);
	for (size_t i = 0; i < lo16.size(); i++) lo16[i] = (uint16_t)((uint32_t)img[G.lo_rank() + i / 2] >> (16 * (i & 1)));
	const uint16_t* const lo = lo16.data();
	int64_t cnt = 0;
	for (int64_t dd = 0; dd < G.n_dn; dd++)
		for (int64_t du = 0; du < G.n_up; du++) {
			const int64_t k = obs_tj_string_source(U, ent[dd], dnw[dd], (uint32_t)du, pat[du], hi, lo, G.lb, G.n_up_src);
			if (action) action[du + dd * G.n_up] = k;
			cnt += (k != 0);
		}
	if (touched) *touched = cnt;
}

// a plan with a sector expanded through an image of its own; a dead plan gives zeros
inline bool tj_string_expand(const TjStringPlan& P, int64_t* action, int64_t* touched, const char** why)
{
	if (P.dead) {
		if (action) std::fill(action, action + P.n_up_dst * P.n_dn_dst, (int64_t)0);
		if (touched) *touched = 0;
		return true;
	}
	TjStringImage G;
	std::vector<int32_t> img;
	if (!tj_string_image_begin(G, P.L, P.nup, P.ndn, P.nup2, P.ndn2, 1, img, why) || !tj_string_image_entries(G, &P, 1, img, why)) return false;
	tj_string_expand_slot(G, img, 0, P.up, action, touched);
	return true;
}

// the same count in closed form: the destination words with the k touched sites in their destination states are a sector of the other L - k sites
inline int64_t tj_string_touched(const TjStringPlan& P)
{
	if (!P.has || P.dead) return 0;
	const int k = __builtin_popcount(P.touched), a = __builtin_popcount(P.dst_up), b = __builtin_popcount(P.dst_dn);
	return binom(P.L - k, P.ndn2 - b) * binom(P.L - k - (P.ndn2 - b), P.nup2 - a);
}

} // namespace obs_host
} // namespace lpp
