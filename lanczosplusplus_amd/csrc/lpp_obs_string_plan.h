// lpp_obs_string_plan.h -- host-only planning of operator strings in the Hubbard product basis: the composition of a PRODUCT of one-site operators
// into one pair of per-species tables (the kernels that read them: lpp_obs_string_kernels.h; sector arithmetic and species ranks: lpp_obs_plan.h),
// and the packing of a launch's tables and word lists into one upload image (StringImage).  Plain C++, no HIP: the sanitizer test of the planner (host/test_string_plan.cpp) compiles this header alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "lpp_engine.h"
#include "lpp_obs_plan.h"

namespace lpp {

constexpr int kObsStringMaxOps = 16; // operators per string (so at most 16 sz entries)

namespace obs_host {

// what one operator does to a word of one species, walking FORWARD from the ket
enum { FW_REMOVE, FW_ADD, FW_KEEP_SET, FW_SIGN_SET }; // needs the bit, clears it | needs it clear, sets it | needs the bit | -1 where the bit is set
struct FwStep {
	int kind, site;
	bool parity; // times the parity of the word's bits below the site
	int gsign; // times a constant of the sector the operator meets
};

struct StringPlan {
	bool has = false;
	int nup2 = 0, ndn2 = 0;
	double scale = 1.0;
	int64_t n_up_src = 0, n_dn_src = 0, n_up_dst = 0, n_dn_dst = 0;
	std::vector<int32_t> tu, td; // never empty when has
	int nsz = 0;
	uint8_t sz[kObsStringMaxOps] = {}; // site | flip_up << 5 | flip_down << 6
};

// one species: every word of the source sector pushed through the steps; table[rank of the word it ends as] = +-(its rank + 1).  Each step is
// injective on words, so no destination is written twice.
inline void compose_table(const Ranker& R, int L, int n_src, int n_dst, const std::vector<FwStep>& steps, bool dead, std::vector<int32_t>& tab)
{
	tab.assign((size_t)binom(L, n_dst), 0);
	if (dead) return;
	const int64_t cnt = binom(L, n_src);
	uint64_t w = first_word(n_src);
	for (int64_t i = 0; i < cnt; i++) {
		uint64_t x = w;
		int s = 1;
		bool ok = true;
		for (const FwStep& f : steps) {
			const uint64_t bit = 1ull << f.site;
			const bool set = (x & bit) != 0;
			if (f.kind == FW_SIGN_SET) {
				if (set) s = -s;
				continue;
			}
			if ((f.kind == FW_ADD) ? set : !set) {
				ok = false;
				break;
			}
			if (f.parity && (__builtin_popcountll(x & (bit - 1)) & 1)) s = -s;
			s *= f.gsign;
			if (f.kind != FW_KEEP_SET) x ^= bit;
		}
		if (ok) tab[(size_t)R.rank(x)] = (int32_t)(s * (i + 1));
		if (i + 1 < cnt) w = next_word(w);
	}
}

// LPP_STRING_MANY_POINT: Engine::manyPoint (Engine.h:341-389), ops[0] acts first, each step accModifiedState_ with factor 1 and the sector walk of
// hasNewParts; n and sz act in the CURRENT sector (the reference's getNeededBasis :397-400 hands them the original sector's basis even after the
// string has left it, which ranks words of another particle number: ill-defined there, defined here).
// LPP_STRING_MEASURE: ModelBase::rahulMethod (ModelBase.h:89-141) with RahulOperator.h, ops[nops-1] acts first, spins[] = dof, flags[] bit 0 = transpose.
// false: refused, *why says why.  P.has == false: a step leads to no sector.
inline bool plan_string(int conv, int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int L, int nup, int ndn, StringPlan& P,
                        const char** why)
{
	P = StringPlan();
	auto refuse = [&](const char* msg) {
		*why = msg;
		return false;
	};
	if (conv != LPP_STRING_MANY_POINT && conv != LPP_STRING_MEASURE) return refuse("operator string: unknown convention (LPP_STRING_*)");
	if (nops < 1 || nops > kObsStringMaxOps) return refuse("operator string: 1 to 16 operators per string");
	if (!ops || !sites || !spins) return refuse("operator string: null argument");
	if (L < 1 || L > 30 || nup < 0 || ndn < 0 || nup > L || ndn > L) return refuse("operator string: bad sites / sector");
	if (too_many_states(binom(L, L / 2))) return refuse("operator string: a species with 2^31 states or more");
	const bool meas = conv == LPP_STRING_MEASURE;
	for (int i = 0; i < nops; i++) {
		const bool known = meas ? (ops[i] == LPP_OP_C || ops[i] == LPP_OP_N || ops[i] == LPP_OP_SZ || ops[i] == LPP_OP_IDENTITY) : valid_op(ops[i]);
		if (!known) return refuse(meas ? "measure: unknown label (c, n, sz, identity)" : "many-point: unknown operator (LPP_OP_*)");
		if (spins[i] != LPP_SPIN_UP && spins[i] != LPP_SPIN_DOWN) return refuse("operator string: spin / dof must be 0 (up) or 1 (down)");
		if (sites[i] < 0 || sites[i] >= L) return refuse("operator string: site out of range");
	}
	std::vector<FwStep> up, dn;
	int pu = nup, pd = ndn;
	bool dead = false; // measure only: a count left [0, L], no word survives
	uint32_t flip_up = 0, flip_dn = 0; // sites flipped an odd number of times so far
	for (int q = 0; q < nops; q++) {
		const int i = meas ? nops - 1 - q : q;
		const int op = ops[i], site = sites[i], spin = spins[i];
		if (meas) {
			std::vector<FwStep>& sp = (spin == LPP_SPIN_UP) ? up : dn;
			if (op == LPP_OP_C) { // the sign: doSign(word after the flip, site), times the parity of the up electrons for dof = down (ModelBase.h:120-131)
				const bool add = flags && (flags[i] & 1);
				int& cnt = (spin == LPP_SPIN_UP) ? pu : pd;
				cnt += add ? 1 : -1;
				if (cnt < 0 || cnt > L) dead = true;
				sp.push_back(FwStep { add ? FW_ADD : FW_REMOVE, site, true, (spin == LPP_SPIN_DOWN && (pu & 1)) ? -1 : 1 });
			} else if (op == LPP_OP_N) {
				sp.push_back(FwStep { FW_KEEP_SET, site, false, 1 });
			} else if (op == LPP_OP_SZ) { // -1/2 on an occupied bit, +1/2 on an empty one (RahulOperator.h:38-40)
				sp.push_back(FwStep { FW_SIGN_SET, site, false, 1 });
				P.scale *= 0.5;
			}
			continue;
		}
		int n1 = pu, n2 = pd;
		if (needs_new_basis(op) && !new_parts(op, spin, L, pu, pd, &n1, &n2)) return true; // no sector: has stays false
		const uint32_t bit = 1u << site;
		switch (op) {
		case LPP_OP_C:
		case LPP_OP_CDAGGER: {
			const int kind = (op == LPP_OP_C) ? FW_REMOVE : FW_ADD;
			if (spin == LPP_SPIN_UP) {
				up.push_back(FwStep { kind, site, true, 1 });
				flip_up ^= bit;
			} else { // doSignGf, SPIN_DOWN: the down bits below the site; at site 0 the parity of the up electrons of the sector the operator meets
				dn.push_back(FwStep { kind, site, site > 0, (site == 0 && (pu & 1)) ? -1 : 1 });
				flip_dn ^= bit;
			}
			break;
		}
		case LPP_OP_N:
			((spin == LPP_SPIN_UP) ? up : dn).push_back(FwStep { FW_KEEP_SET, site, false, 1 });
			break;
		case LPP_OP_SZ: // +1 up only, -1 down only, absent otherwise: of the word the operator meets = the source word with the flips so far
			P.sz[P.nsz++] = (uint8_t)(site | (((flip_up >> site) & 1u) << 5) | (((flip_dn >> site) & 1u) << 6));
			break;
		default: // splus / sminus: cdagger on one word, c on the other, sign doSignSpSm
			up.push_back(FwStep { op == LPP_OP_SPLUS ? FW_ADD : FW_REMOVE, site, true, 1 });
			dn.push_back(FwStep { op == LPP_OP_SPLUS ? FW_REMOVE : FW_ADD, site, true, 1 });
			flip_up ^= bit;
			flip_dn ^= bit;
			break;
		}
		pu = n1;
		pd = n2;
	}
	if (meas && (pu != nup || pd != ndn))
		return refuse("measure: the string does not conserve the number of up and of down electrons (the reference would index outside the sector)");
	P.nup2 = pu;
	P.ndn2 = pd;
	P.n_up_src = binom(L, nup);
	P.n_dn_src = binom(L, ndn);
	P.n_up_dst = binom(L, pu);
	P.n_dn_dst = binom(L, pd);
	const Ranker R(L);
	compose_table(R, L, nup, pu, up, dead, P.tu);
	compose_table(R, L, ndn, pd, dn, dead, P.td);
	P.has = true;
	return true;
}

// ---- what is uploaded for a launch, packed on the host -----------------------------------------------------------------------------------

// the sz entries of a plan as the kernels read them: entry k is 8 bits of lo (k < 8) or of hi
struct StringSzWords {
	uint64_t lo = 0, hi = 0;
	uint8_t entry(int k) const { return (uint8_t)(((k < 8) ? lo : hi) >> (8 * (k & 7))); }
};
inline StringSzWords pack_sz(const StringPlan& P)
{
	StringSzWords W;
	for (int k = 0; k < P.nsz; k++) ((k < 8) ? W.lo : W.hi) |= (uint64_t)P.sz[k] << (8 * (k & 7));
	return W;
}

// One upload image of 32-bit words: `slots` pairs of tables (up: ntu entries, down: ntd, the DESTINATION sector's species counts), then the SOURCE
// sector's species words by rank, up (nwu) then down (nwd); 0, 0: no word lists (a string without sz reads none).  The offsets are in words.
struct StringImage {
	int64_t ntu = 0, ntd = 0;
	int slots = 0;
	int64_t nwu = 0, nwd = 0;
	size_t tab_up(int s) const { return (size_t)(ntu + ntd) * (size_t)s; }
	size_t tab_dn(int s) const { return tab_up(s) + (size_t)ntu; }
	size_t words_up() const { return tab_up(slots); }
	size_t words_dn() const { return words_up() + (size_t)nwu; }
	size_t size() const { return words_dn() + (size_t)nwd + 4; } // (4 spare words: the word pointers of an image without lists stay inside it)
};

// a fresh image: zeros, and the word lists of source sector (L; nup, ndn) where the image has them.  false: the lists are not of the image's lengths
inline bool string_image_begin(const StringImage& G, int L, int nup, int ndn, std::vector<int32_t>& img, const char** why)
{
	img.assign(G.size(), 0);
	std::vector<uint32_t> w;
	for (int sp = 0; sp < 2; sp++) {
		const int64_t len = sp ? G.nwd : G.nwu;
		if (len == 0) continue;
		species_words(L, sp ? ndn : nup, w);
		if ((int64_t)w.size() != len) {
			*why = "operator string: the word lists are not of the upload image's sector";
			return false;
		}
		std::copy(w.begin(), w.end(), img.begin() + (std::ptrdiff_t)(sp ? G.words_dn() : G.words_up()));
	}
	return true;
}

// the tables of plans[0 .. ns) into slots 0 .. ns-1 of the image.  false, and nothing copied: more plans than slots, or a table whose length is not
// the image's species count -- copying it would write, and the kernel would read, outside its slot
inline bool string_image_tables(const StringImage& G, const StringPlan* plans, int ns, std::vector<int32_t>& img, const char** why)
{
	bool fits = ns >= 0 && ns <= G.slots && img.size() == G.size();
	for (int s = 0; s < ns && fits; s++) fits = (int64_t)plans[s].tu.size() == G.ntu && (int64_t)plans[s].td.size() == G.ntd;
	if (!fits) {
		*why = "operator string: a plan's tables are not of the upload image's sector";
		return false;
	}
	for (int s = 0; s < ns; s++) {
		std::copy(plans[s].tu.begin(), plans[s].tu.end(), img.begin() + (std::ptrdiff_t)G.tab_up(s));
		std::copy(plans[s].td.begin(), plans[s].td.end(), img.begin() + (std::ptrdiff_t)G.tab_dn(s));
	}
	return true;
}

} // namespace obs_host
} // namespace lpp
