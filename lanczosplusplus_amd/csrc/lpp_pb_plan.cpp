// lpp_pb_plan.cpp -- the product-basis build's decisions and host data (lpp_pb_plan.h); pb_build (lpp_pb.hip) uploads the result.
#include "lpp_pb_plan.h"

#include "lpp_pb_instances.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lpp {

PbSwitches pb_switches_from_env()
{
	auto rd = env_switch;
	PbSwitches sw;
	sw.big2 = rd("LPP_PB_BIG2"), sw.big2_four = rd("LPP_PB_BIG2_FOUR"), sw.piece_rows = rd("LPP_PB_PIECE_ROWS"), sw.parts = rd("LPP_PB_PARTS");
	sw.wide = rd("LPP_PB_WIDE"), sw.bank_ways = rd("LPP_PB_BANK_WAYS"), sw.perm = rd("LPP_PB_PERM"), sw.seg = rd("LPP_PB_SEG"), sw.pre0 = rd("LPP_PB_PRE0");
	sw.down_rounds = rd("LPP_PB_DOWN_ROUNDS"), sw.order_window = rd("LPP_PB_ORDER_WINDOW"), sw.down_image = rd("LPP_PB_DOWN_IMAGE"), sw.pace = rd("LPP_PB_PACE");
	sw.chain = rd("LPP_PB_CHAIN"), sw.down_tasks = rd("LPP_PB_DOWN_TASKS"), sw.down_pf = rd("LPP_PB_DOWN_PF"), sw.chain_pace = rd("LPP_PB_CHAIN_PACE");
	sw.lazy_tx = rd("LPP_PB_LAZY_TX"), sw.down_grid = rd("LPP_PB_DOWN_GRID");
	sw.verbose = rd("LPP_VERBOSE").set;
	return sw;
}

// the realified in-block matrix: complex entry (i, c, t) -> row 2i: (2c, Re t), (2c+1, -Im t); row 2i+1: (2c, Im t), (2c+1, Re t); zero parts
// are dropped (a real hop costs two entries, not four); columns stay ascending
void pb_realify(int64_t n, const int64_t* rp, const int32_t* ci, const double* va, std::vector<int64_t>& rrp, std::vector<int32_t>& rci, std::vector<double>& rva)
{
	rrp.assign((size_t)(2 * n) + 1, 0);
	rci.clear();
	rva.clear();
	for (int64_t i = 0; i < n; i++)
		for (int half = 0; half < 2; half++) {
			for (int64_t p = rp[i]; p < rp[i + 1]; p++) {
				const int64_t c = ci[p];
				if (c == i) continue; // the diagonal lives in D
				const double re = va[2 * p], im = va[2 * p + 1];
				const double v0 = half == 0 ? re : im, v1 = half == 0 ? -im : re; // coefficients of (Re y_c, Im y_c)
				if (v0 != 0.0) {
					rci.push_back((int32_t)(2 * c));
					rva.push_back(v0);
				}
				if (v1 != 0.0) {
					rci.push_back((int32_t)(2 * c + 1));
					rva.push_back(v1);
				}
			}
			rrp[(size_t)(2 * i + half) + 1] = (int64_t)rci.size();
		}
}

// rows by the chunk counts of their lists (plan_form: want_perm); pt_* = P T P^T.  Leaves `perm` empty where T has no or too many values
void pb_list_length_order(const PbBuildInput& in, std::vector<int32_t>& perm, std::vector<int32_t>& inv, std::vector<int64_t>& p_rp, std::vector<int32_t>& p_ci,
                            std::vector<double>& p_va)
{
	const int64_t n_up = in.n_up;
	const int64_t* const t_rp = in.t_rp;
	const int32_t* const t_ci = in.t_ci;
	const double* const t_va = in.t_va;
	std::vector<unsigned long long> vals; // distinct values, ascending bit pattern (the order pb_pack_template numbers its groups in does not matter here)
	for (int64_t i = 0; i < n_up && vals.size() <= (size_t)kPbMaxGroups; i++)
		for (int64_t q = t_rp[i]; q < t_rp[i + 1] && vals.size() <= (size_t)kPbMaxGroups; q++) {
			if (t_ci[q] == i) continue; // the diagonal is not part of the template (it lives in D)
			unsigned long long k;
			std::memcpy(&k, &t_va[q], 8);
			if (std::find(vals.begin(), vals.end(), k) == vals.end()) vals.push_back(k);
		}
	if (vals.size() > (size_t)kPbMaxGroups || vals.empty()) return;
	const int G = (int)vals.size();
	std::vector<uint8_t> key((size_t)n_up * (size_t)G, 0); // chunks of 4 per group
	for (int64_t i = 0; i < n_up; i++) {
		int cnt[kPbMaxGroups] = { 0 };
		for (int64_t q = t_rp[i]; q < t_rp[i + 1]; q++) {
			if (t_ci[q] == i) continue;
			unsigned long long k;
			std::memcpy(&k, &t_va[q], 8);
			cnt[std::find(vals.begin(), vals.end(), k) - vals.begin()]++;
		}
		for (int g = 0; g < G; g++) key[(size_t)i * G + g] = (uint8_t)std::min(255, (cnt[g] + 3) / 4);
	}
	perm.resize((size_t)n_up);
	for (int64_t i = 0; i < n_up; i++) perm[(size_t)i] = (int32_t)i;
	std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return std::lexicographical_compare(&key[(size_t)x * G], &key[(size_t)x * G] + G, &key[(size_t)y * G], &key[(size_t)y * G] + G); });
	inv.resize((size_t)n_up);
	for (int64_t q = 0; q < n_up; q++) inv[(size_t)perm[(size_t)q]] = (int32_t)q;
	// T' = P T P^T, columns ascending inside a row
	p_rp.assign((size_t)n_up + 1, 0);
	p_ci.resize((size_t)t_rp[n_up]);
	p_va.resize((size_t)t_rp[n_up]);
	std::vector<std::pair<int32_t, double>> row;
	for (int64_t q = 0; q < n_up; q++) {
		const int64_t i = perm[(size_t)q];
		row.clear();
		for (int64_t k = t_rp[i]; k < t_rp[i + 1]; k++) row.emplace_back(inv[(size_t)t_ci[k]], t_va[k]);
		std::sort(row.begin(), row.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
		int64_t o = p_rp[(size_t)q];
		for (const auto& en : row) {
			p_ci[(size_t)o] = en.first;
			p_va[(size_t)o] = en.second;
			o++;
		}
		p_rp[(size_t)q + 1] = o;
	}
}

namespace {
// what the form step decides beyond the fields of PbForm
struct Choice {
	int64_t wmax = 0, nblk_padded = 0;
	size_t vec_bytes = 0;
	bool big2 = true, big2_four = true, want_perm = false, try_seg = false;
	int ways = 2;
};

uint8_t code_of(const double* dict, int ndict, double v)
{
	// same order as the device's dict_code: bit patterns compared as unsigned integers
	uint64_t key;
	std::memcpy(&key, &v, 8);
	int lo = 0, hi = ndict - 1;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		uint64_t k;
		std::memcpy(&k, &dict[mid], 8);
		if (k < key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return (uint8_t)lo;
}

// The counter-scheduled form of k_pb_down (PF) keeps its task sums in LDS behind the image: it runs only where both fit 150 KB; the
// fixed-share form, whose sums follow a fixed order by construction, takes the rest
bool pb_down_pf_fits(const PbForm& B) { return B.down_lds_pf <= kPbDownLdsMax; }
// a panel (16 positions = 128 bytes of every block) fits an XCD's 4 MB L2 with room to spare
bool pb_panel_fits_l2(int64_t n_blk) { return (size_t)n_blk * 128 <= (size_t)3 << 20; }

// ---- the form, from sizes and switches alone ---------------------------------------------------------------------------------------
lpp_status plan_form(const PbBuildInput& in, const PbSwitches& sw, PbForm& B, Choice& c)
{
	const int64_t n_up = in.n_up, n_blk = in.n_blk;
	B.n_up = n_up;
	B.n_blk = n_blk;
	B.pitch = pb_pitch_for(n_up);
	B.tx = in.pitch_dn > 0; // several GPUs: own blocks for the in-block part, the transposed slice for the couplings
	B.blk0 = in.blk0;
	B.nblk_loc = in.nblk_loc < 0 ? n_blk : in.nblk_loc;
	B.pitch_dn = B.tx ? in.pitch_dn : B.pitch;
	c.nblk_padded = B.tx ? in.nblk_padded : n_blk;
	if (B.blk0 < 0 || B.blk0 + B.nblk_loc > n_blk || (B.pitch_dn & 15) || c.nblk_padded < n_blk) return fail(LPP_ERR_INVALID, "pb_build: bad block range / coupling pitch");
	// Rows beyond one LDS window are cut into pieces (k_pb_up_big): two 512-thread workgroups of <= 80 KB per CU.  LPP_PB_PIECE_ROWS
	// forces pieces of (at most) that many positions on any matrix (tests run the small cases of the suite through them).
	// pieces of <= 8128 positions: two blocks' windows share a workgroup (k_pb_up_big2) and the second one stays within the 64 KB an
	// LDS instruction's offset reaches; LPP_PB_BIG2=0: one block per workgroup, two 512-thread workgroups per CU (k_pb_up_big, <= 8768)
	c.big2 = !sw.big2.off();
	// four value groups (complex hoppings realified) two blocks at a time too -- half the template words per output row: 4.74 against
	// 5.48 ms (k_pb_up_big<.., 4, 3>) at 1.47e8 complex states; LPP_PB_BIG2_FOUR=0: the one-block kernel
	c.big2_four = !sw.big2_four.off();
	// one window needs the row, its diagonal codes and the template's list heads in LDS (pb_up_lds_bytes; two value groups assumed here):
	// rows of 17,400-19,500 positions pass a test of the row alone and then failed pb_build -- the 3x6 lattice's 6-electron species (18,564)
	if ((size_t)(B.pitch + kPbZeroSlots) * sizeof(double) > (size_t)156 * 1024 || pb_up_lds_bytes(B.pitch, (int)((n_up + 63) / 64), 2) > kPbUpLdsMax)
		c.wmax = c.big2 ? 8128 : 8768;
	if (sw.piece_rows.set) c.wmax = std::max<int64_t>(64, std::min<int64_t>(sw.piece_rows.v, c.big2 ? 8128 : 16384)) & ~(int64_t)63;
	int64_t W = 0;
	if (c.wmax > 0) {
		const int64_t np = (n_up + c.wmax - 1) / c.wmax;
		W = (((n_up + np - 1) / np) + 63) & ~(int64_t)63;
		if (n_up >= ((int64_t)1 << 24) && !in.pre) return fail(LPP_ERR_INVALID, "pb_build: more than 2^24 positions per block"); // (24-bit positions of the per-position template)
	}
	B.big = W > 0;
	B.W = (int)W;
	// Couplings: the panel of 16 positions of all blocks has to stay in one XCD's L2 (4 MiB) while it is gathered from.  Beyond
	// ~1.6 MB the source blocks are walked in parts (k_pb_down_parts, which also forms 64-bit addresses: vectors beyond 4 GiB).
	c.vec_bytes = (size_t)c.nblk_padded * (size_t)B.pitch_dn * sizeof(double);
	// (the pacing of k_pb_down_parts keeps the workgroups of a group within two consecutive parts: two parts of <= 1.7 MB live)
	// Measured at N_dn = 38760 (panel 4.96 MB, 3.0e9 states, scripts/experiments/r03_parts_ab.sh): whole panel 46.6 ms per product
	// (the misses of an over-full L2 are Infinity-Cache hits), 2 parts 51.4, 3 parts 56.7, 4 parts 63.4, 6 parts 84.3 -- the part
	// phases cost more (a wait per part, lists padded per part) than the L2 hits return.  So parts are kept for panels beyond
	// 6 MB only; up to there the whole-panel kernel runs, with 64-bit addresses where the vector needs them (k_pb_down<WIDE>).
	B.nparts = (size_t)c.nblk_padded * 128 <= (size_t)6 << 20 || n_blk > 65535 ? 1 : 2; // (the parts form keeps 16-bit places and all of a workgroup's sums in registers: below 65536 blocks)
	if (sw.parts.set) B.nparts = std::max(1, std::min(sw.parts.v, kPbMaxParts));
	B.parts = B.nparts > 1 || sw.parts.set;
	B.wide = c.vec_bytes >= ((size_t)1 << 32) || sw.wide.set;
	c.ways = std::max(1, std::min(sw.bank_ways.value_or(2), 4));
	// complex hoppings: the realified in-block matrix is an ordinary real template (4-8 value groups: k_pb_up / k_pb_up_big with any number
	// of groups), in one window or in pieces; the couplings' kernel multiplies complex values (k_pb_down<CPLX>, with 64-bit addresses too)
	if (in.cx && (B.tx || B.parts)) return fail(LPP_ERR_INVALID, "pb_build: complex hoppings are held in the single-GPU forms with whole-panel couplings only");
	if (B.parts && n_blk > 65535) return fail(LPP_ERR_INVALID, "pb_build: the parts form holds 16-bit block numbers");
	if (n_blk >= ((int64_t)1 << 24)) return fail(LPP_ERR_INVALID, "pb_build: more than 2^24 - 1 blocks");
	if ((size_t)c.nblk_padded * (size_t)(B.pitch_dn >> 4) >= ((size_t)1 << 32)) return fail(LPP_ERR_INVALID, "pb_build: vector beyond 32-bit line numbers");
	// Row order inside a block.  A slice of 64 rows walks as many template chunks per value group as its LONGEST list needs, and in
	// the basis order neighbouring rows have lists of very different lengths: at config 2 17.1 entries per row occupy 28.9 slots.
	// Stored in the order of their chunk counts (stable, so neighbours stay neighbours among equals) they occupy 20.2: 30 % fewer
	// template words through L1, LDS gathers and adds.  One-window, single-GPU form only: the pieces form lives on the locality of
	// the basis order and the exchange kernels address positions by their basis index.  LPP_PB_PERM=0 switches it off.
	c.want_perm = !in.cx && W == 0 && !B.tx && B.nblk_loc == n_blk && n_up >= 128 && !sw.perm.off();
	// The segmented in-block form (plan_segments) is taken by itself from 65536 positions per row on: below that the per-position template
	// (80 bytes per position: 3.1 MB at the 38760 positions of the 4x5 lattice's 6-electron species) still shares an XCD's L2 with the rows,
	// and k_pb_up_big2 -- compact far lists, fewer lines through L1 -- is faster (the (6,6) sector: 36.8 against 42.7 ms per step; the (7,6)
	// sector, 77520 positions: 91.9 against 90.0).  LPP_PB_SEG=0 / 1: never / wherever it applies.
	c.try_seg = !in.pre && W > 0 && !in.cx && c.big2 && (sw.seg.set ? sw.seg.v != 0 : n_up >= 65536);
	B.lazy_tx = B.tx && sw.lazy_tx.value_or(1) != 0;
	return LPP_OK;
}

// ---- in-block part ---------------------------------------------------------------------------------------------------------------------
// Rows beyond one LDS window: T decomposed by the high sites of the species' basis word (lpp_pbseg.h) when T is the hopping matrix of
// one species in the ascending-word basis -- read off T itself and verified against it entry by entry (pb_seg_plan); otherwise the
// per-position template of lpp_pbig_kernels.h.  One GPU or the transposition exchange alike: every kernel of a step is position-blind.
lpp_status plan_segments(const PbBuildInput& in, const Choice& c, PbPlan& P)
{
	PbForm& B = P.form;
	SegPlan& SP = P.seg;
	bool seg = false;
	if (in.pre) { // the caller made the plan from the model's parameters (pb_chain): there is no host copy of T
		if (!B.big || in.cx || B.tx || in.n_blk != 1 || in.c_rp[1] != 0) return fail(LPP_ERR_INVALID, "pb_build: a ready-made plan is for one block beyond the LDS window");
		SP = std::move(*in.pre);
		seg = pb_seg_lds_bytes(SP.ws, SP.wmax, 1) <= kPbUpLdsMax;
		if (!seg) return fail(LPP_ERR_INVALID, "pb_build: the plan exceeds LDS");
	} else if (c.try_seg) {
		int wcap = (int)std::min<int64_t>(c.wmax, 8128);
		lpp_status rs = pb_seg_plan(in.n_up, in.t_rp, in.t_ci, in.t_va, wcap, SP, &seg);
		if (rs != LPP_OK) return rs;
		// One more high site when the two windows of the longest item do not fit beside the tables, or when the cut runs through a ring of
		// the lattice and a segment has more hops than the (5 pairs, 4) kernel instance carries -- the (6, 8) one spills: the (6,6) sector of the
		// 4x5 lattice cut at 4 high sites ran 71 ms per step against 37 with the per-position template
		for (int more = 0; more < 2 && seg && (pb_seg_lds_bytes(SP.ws, SP.wmax, 2) > kPbUpLdsMax || SP.nc_pad > 5); more++) {
			SegPlan SP2;
			bool seg2 = false;
			wcap = std::max(64, SP.wmax - 1);
			rs = pb_seg_plan(in.n_up, in.t_rp, in.t_ci, in.t_va, wcap, SP2, &seg2);
			if (rs != LPP_OK) return rs;
			if (!seg2 || SP2.s <= SP.s) break;
			SP = std::move(SP2);
		}
		if (seg && pb_seg_lds_bytes(SP.ws, SP.wmax, 2) > kPbUpLdsMax) seg = false;
		P.seg_tried = true;
	}
	if (!seg) return LPP_OK;
	B.seg = true;
	B.seg_nitems = (int)SP.items.size();
	B.seg_nsegs = (int)SP.segs.size();
	B.seg_ws = SP.ws;
	B.seg_wmax = SP.wmax;
	B.seg_nc = SP.nc_pad;
	B.seg_nh = SP.nh_pad;
	B.seg_pre0 = SP.pre0;
	B.seg_one = in.pre != nullptr; // one block per workgroup
	B.seg_bytes = (int64_t)(SP.words.size() * 4 + SP.xwords.size() * 4 + SP.slices.size() * 16 + SP.cross.size() * 32 + SP.hh.size() * 16 + SP.segs.size() * 32 + SP.items.size() * 32);
	P.perm = SP.perm; // (the stored order is the segments by length)
	P.inv = SP.inv;
	PbTemplate& T = P.T; // the per-position template is not built at all
	T.G = SP.G;
	for (int g = 0; g < kPbMaxGroups; g++) T.gval[g] = SP.gval[g];
	T.spb = (int)((in.n_up + 63) / 64);
	T.entries = SP.entries_lo;
	T.slots = SP.slots_lo;
	T.W = B.W;
	return LPP_OK;
}

// chunk pairs: lane l's two words of chunk 2q and of chunk 2q+1 side by side (one 16-byte load); a list of an odd number of chunks ends
// with half a pair of zero-slot indices; offsets count pairs (k_pb_up)
void repack_chunk_pairs(PbTemplate& T)
{
	std::vector<uint32_t> pw;
	pw.reserve(T.words.size() + T.words.size() / 4);
	const uint32_t zw = T.words.empty() ? 0u : T.words.back(); // the slack behind the lists: (zero slot, zero slot)
	for (size_t i = 0; i < T.off.size(); i++) {
		const size_t src = (size_t)T.off[i] * 128;
		const int nc = T.len[i];
		T.off[i] = (int32_t)(pw.size() / 256);
		for (int q = 0; q < (nc + 1) / 2; q++)
			for (int l = 0; l < 64; l++)
				for (int h = 0; h < 2; h++)
					for (int k = 0; k < 2; k++) pw.push_back(2 * q + h < nc ? T.words[src + (size_t)(2 * q + h) * 128 + (size_t)l * 2 + k] : zw);
	}
	pw.resize(pw.size() + 256 * 4, zw); // slack for the look-ahead loads
	T.words.swap(pw);
}

// the template (in the stored order of the rows), its chunk-pair repack and look-ahead split, and which in-block kernel reads it
lpp_status plan_template(const PbBuildInput& in, const PbSwitches& sw, const Choice& c, PbPlan& P)
{
	PbForm& B = P.form;
	PbTemplate& T = P.T;
	const int64_t n_up = in.n_up;
	if (!B.seg) {
		std::vector<int64_t> p_rp;
		std::vector<int32_t> p_ci;
		std::vector<double> p_va;
		if (c.want_perm) pb_list_length_order(in, P.perm, P.inv, p_rp, p_ci, p_va);
		const lpp_status rc = !P.perm.empty() ? pb_pack_template(n_up, B.pitch, p_rp.data(), p_ci.data(), p_va.data(), T, c.ways, B.W)
		                                      : pb_pack_template(n_up, B.pitch, in.t_rp, in.t_ci, in.t_va, T, c.ways, B.W);
		if (rc != LPP_OK) return rc;
	}
	B.G = T.G;
	for (int g = 0; g < kPbMaxGroups; g++) B.gval[g] = T.gval[g];
	B.spb = T.spb;
	B.t_entries = T.entries;
	B.t_slots = T.slots;
	B.pre0 = kPbPre;
	const bool pairs = kPbPairs && !B.big; // one-window form: chunk pairs, even look-ahead depths (2,6), (4,4) or (6,4)
	if (T.G == 2 && !B.seg) {
		// look-ahead split of the in-block kernels: the depth pair (3,5), (4,4) or (5,3) that leaves the fewest chunks beyond it, among the
		// depths the kernel is instantiated for (lpp_pb_instances.h)
		int64_t best = -1;
		pb_for_each_pre0(B.big, [&](int p0) {
			int64_t beyond = 0;
			const int p1 = pairs ? pb_depth(2, 1, p0) : 2 * kPbPre - p0;
			for (int j = 0; j < T.spb; j++) beyond += std::max(0, (int)T.len[(size_t)j * 2] - p0) + std::max(0, (int)T.len[(size_t)j * 2 + 1] - p1);
			if (best < 0 || beyond < best || (beyond == best && p0 == kPbPre)) {
				best = beyond;
				B.pre0 = p0;
			}
		});
		if (sw.pre0.set) B.pre0 = pb_listed_pre0(B.big, sw.pre0.v);
	}
	if (pairs && !B.seg) repack_chunk_pairs(T);
	B.tw_words = (int64_t)T.words.size();
	B.big2 = B.big && c.big2 && (T.G == 1 || T.G == 2 || (T.G == 4 && c.big2_four)) && pb_big2_lds_bytes(B.W) <= kPbUpLdsMax && (B.W + kPbZeroSlots) * 8 < 65536;
	B.npieces = B.seg ? B.seg_nitems : B.big ? (int)((n_up + B.W - 1) / B.W) : 1;
	if (B.big && !B.seg) {
		B.f_words = (int64_t)T.fwords.size();
		B.f_entries = T.far_entries;
		if (pb_big_lds_bytes(B.W) > kPbUpLdsMax) return fail(LPP_ERR_INVALID, "pb_build: piece exceeds LDS");
	}
	if (!B.big && pb_up_lds_bytes(B.pitch, T.spb, T.G) > kPbUpLdsMax) return fail(LPP_ERR_INVALID, "pb_build: window + template metadata exceed LDS");
	return LPP_OK;
}

// ---- couplings: plain off-diagonal copies of T and C, coupling codes, dictionaries, block bases; *longest: the longest coupling list ----
lpp_status plan_couplings(const PbBuildInput& in, PbPlan& P, int64_t* longest)
{
	PbForm& B = P.form;
	const int64_t n_blk = in.n_blk;
	const PbCplxInput* const cx = in.cx;
	const int64_t n_rows_t = cx ? cx->n_c : in.n_up; // rows of the matrix lpp_engine_get_csr walks
	const int64_t* const rp = cx ? cx->t_rp : in.t_rp;
	const int32_t* const ci = cx ? cx->t_ci : in.t_ci;
	const double* const va = cx ? cx->t_va : in.t_va;
	// (a ready-made plan (pb_chain) has no host T, and lpp_engine_get_csr re-runs the assembler: nothing to keep)
	P.tp.assign(rp ? (size_t)n_rows_t + 1 : 1, 0);
	for (int64_t r = 0; r < n_rows_t && rp; r++) {
		for (int64_t p = rp[r]; p < rp[r + 1]; p++) {
			if (ci[p] == r) continue;
			if (!P.tc.empty() && (int64_t)P.tc.size() > P.tp[(size_t)r] && P.tc.back() >= ci[p]) return fail(LPP_ERR_INVALID, "pb_build: in-block rows must be sorted by column");
			P.tc.push_back(ci[p]);
			if (cx) {
				P.tv.push_back(va[2 * p]);
				P.tv.push_back(va[2 * p + 1]);
			} else
				P.tv.push_back(va[p]);
		}
		P.tp[(size_t)r + 1] = (int64_t)P.tc.size();
	}
	std::vector<double>& cdict = P.cdict; // complex hoppings: the couplings' own dictionary; code 0 = 0 (the padding places of k_pb_down)
	if (cx) cdict.assign(2, 0.0);
	P.cp.assign((size_t)n_blk + 1, 0);
	*longest = 1;
	for (int64_t b = 0; b < n_blk; b++) {
		for (int64_t p = in.c_rp[b]; p < in.c_rp[b + 1]; p++) {
			if (in.c_ci[p] == b) continue;
			if (in.c_ci[p] < 0 || in.c_ci[p] >= n_blk) return fail(LPP_ERR_INVALID, "pb_build: block coupling out of range");
			if ((int64_t)P.cc.size() > P.cp[(size_t)b] && P.cc.back() >= in.c_ci[p]) return fail(LPP_ERR_INVALID, "pb_build: block couplings must be sorted");
			uint8_t code = 0;
			if (cx) {
				size_t k = 0;
				for (; k < cdict.size() / 2; k++)
					if (std::memcmp(&cdict[2 * k], &cx->c_va[2 * p], 16) == 0) break;
				if (k == cdict.size() / 2) {
					if (k >= 256) return fail(LPP_ERR_INVALID, "pb_build: more than 256 distinct complex coupling values");
					cdict.push_back(cx->c_va[2 * p]);
					cdict.push_back(cx->c_va[2 * p + 1]);
				}
				code = (uint8_t)k;
			} else {
				code = code_of(in.dict256, in.ndict, in.c_va[p]);
				if (std::memcmp(&in.dict256[code], &in.c_va[p], 8) != 0) return fail(LPP_ERR_INVALID, "pb_build: coupling value missing from the dictionary");
			}
			P.cc.push_back(in.c_ci[p]);
			P.ccode.push_back(code);
		}
		P.cp[(size_t)b + 1] = (int64_t)P.cc.size();
		*longest = std::max(*longest, P.cp[(size_t)b + 1] - P.cp[(size_t)b]);
	}
	B.c_nnz = (int64_t)P.cc.size();
	P.dict.assign(in.dict256, in.dict256 + 256);
	B.ndict = in.ndict;
	if (cx) {
		cdict.resize(512, 0.0);
		B.cplx = true;
		B.n_c = cx->n_c;
	}
	// first CSR entry of every block: a block holds Z_T + n_up*(1 + couplings of the block) entries
	P.base.assign((size_t)n_blk + 1, 0);
	const int64_t zt = P.tp.back();
	for (int64_t b = 0; b < n_blk; b++) P.base[(size_t)b + 1] = P.base[(size_t)b] + zt + n_rows_t * (1 + P.cp[(size_t)b + 1] - P.cp[(size_t)b]);
	B.nnz = P.base[(size_t)n_blk];
	B.nnz_loc = P.base[(size_t)(B.blk0 + B.nblk_loc)] - P.base[(size_t)B.blk0];
	if (in.pre) B.nnz = B.nnz_loc = in.pre_nnz;
	return LPP_OK;
}

// ---- coupling-kernel geometry ------------------------------------------------------------------------------------------------------------
// The LDS image of a workgroup's coupling lists (150 KB at most): when its blocks' lists do not fit, the workgroup walks its range in
// rounds of ids_per_round blocks inside every panel (k_pb_down, whole-panel form only); LPP_PB_DOWN_ROUNDS=n forces n rounds (tests)
void plan_rounds(const PbSwitches& sw, const Choice& c, PbForm& B)
{
	const int unit = B.ids_per_wg >= 512 ? 64 : 8; // whole sorting windows of `order` (small ranges: whole tasks)
	auto per_round = [&](int r) { return r == 1 ? B.ids_per_wg : (int)((((int64_t)B.ids_per_wg + r - 1) / r + unit - 1) / unit * unit); };
	// Pieces of ~320 blocks also run FASTER than one long range where a workgroup owns 800 blocks and more (measured on the 4x5 lattice,
	// scripts/experiments/README.md "Round 5": 38760 blocks, 1212 per workgroup: 33.2 ms in one round, 28.5 in four; 77520 blocks, 2423 per
	// workgroup: 82.6 ms in the two rounds LDS asks for, 76.8 in eight), and slower below (config 2, 403 per workgroup: 1.30 / 1.50 / 1.69 ms
	// in 1 / 2 / 3 rounds) -- and slower on the same 38760 blocks when the vector is 12 instead of 24 GB (the (6,6) sector: 12.1 ms in one round,
	// 13.5 in four): what the rounds cure grows with the span of addresses a panel touches (one line every 620 KB over 24 GB at the (7,6)
	// sector, whose coupling kernel takes 36 % longer per element than the (6,6) sector's in one round, 17 % in four).  So: vectors from 16 GB on
	int r = 1;
	if (sw.down_rounds.set) r = std::max(1, std::min(sw.down_rounds.v, 64));
	else if (B.ids_per_wg >= 800 && c.vec_bytes >= ((size_t)16 << 30)) r = std::min(64, (B.ids_per_wg + 160) / 320);
	while (r < 64 && pb_down_lds_bytes(per_round(r), B.rowcap) > kPbDownLdsMax) r++;
	while (r > 1 && (int64_t)per_round(r) * (r - 1) >= B.ids_per_wg) r--; // (a last round without blocks: one round less covers the range)
	B.down_rounds = r;
	B.ids_per_round = per_round(r);
}

// the parts form: per block and part, where the part's entries start in the (ascending) list; per part: the longest list, in whole chunks of 4
lpp_status plan_parts(PbPlan& P)
{
	PbForm& B = P.form;
	const int64_t n_blk = B.n_blk;
	const int nparts = B.nparts;
	B.part_blocks = (n_blk + nparts - 1) / nparts;
	P.pstart.assign((size_t)n_blk * (size_t)(nparts + 1), 0);
	for (int64_t b = 0; b < n_blk; b++) {
		int32_t* ps = P.pstart.data() + (size_t)b * (size_t)(nparts + 1);
		const int64_t len = P.cp[(size_t)b + 1] - P.cp[(size_t)b];
		if (len > 1020) return fail(LPP_ERR_INVALID, "pb_build: coupling list too long");
		int h = 0;
		for (int64_t k = 0; k < len; k++) {
			const int hk = (int)std::min<int64_t>(P.cc[(size_t)(P.cp[(size_t)b] + k)] / B.part_blocks, nparts - 1);
			while (h < hk) ps[++h] = (int32_t)k;
		}
		while (h < nparts) ps[++h] = (int32_t)len;
	}
	// list entries per workgroup (contiguous ranges of ids_per_wg blocks): the largest sizes the LDS image
	int64_t ent_cap = 0;
	for (int64_t lo = 0; lo < n_blk; lo += B.ids_per_wg) ent_cap = std::max(ent_cap, P.cp[(size_t)std::min<int64_t>(lo + B.ids_per_wg, n_blk)] - P.cp[(size_t)lo]);
	if (ent_cap > 65000) return fail(LPP_ERR_INVALID, "pb_build: block couplings of a workgroup exceed the 16-bit places of the LDS image");
	B.ent_cap = (int)ent_cap;
	B.down_lds = pb_parts_lds_bytes(B.ids_per_wg, B.ent_cap, nparts);
	constexpr int nw = kPbPartsThreads / 64;
	const int rounds = (((B.ids_per_wg + 7) / 8) + nw - 1) / nw; // tasks of 8 blocks over the waves of a workgroup
	B.maxr = (rounds + 3) / 4 * 4;
	if (rounds > 24) return fail(LPP_ERR_INVALID, "pb_build: too many blocks per workgroup for the register accumulators");
	const int64_t npanels = std::max(B.pitch, B.pitch_dn) / 16;
	B.pace_stride = (int)(((npanels + 7) / 8 + 1) * nparts);
	if (B.down_grid < 8) B.pace_stride = (int)((npanels + 1) * nparts);
	return LPP_OK;
}

// every workgroup takes its blocks in the order of decreasing list length (tasks of 8 blocks with equal trip counts)
void plan_order(const PbSwitches& sw, PbPlan& P)
{
	const PbForm& B = P.form;
	const int64_t n_blk = B.n_blk;
	const std::vector<int64_t>& cp = P.cp;
	std::vector<int32_t>& order = P.order;
	order.resize((size_t)n_blk);
	for (int64_t b = 0; b < n_blk; b++) order[(size_t)b] = (int32_t)b;
	// ... inside windows of 64 consecutive blocks: neighbouring blocks gather many of the same lines (hops among the low sites
	// keep the high part of the word -- a run of <= 70 consecutive blocks at config 2), so the tasks that are in flight together
	// share them in L1.  Measured at config 2 (scripts/experiments/r03_order_ab.sh): k_pb_down<RMW> 1.711 ms sorted over the
	// whole range of ~400 blocks, 1.655-1.662 ms with windows of 48-64, 1.73 ms with windows of 32 (tasks of unequal lists)
	const int64_t order_window = sw.order_window.set ? std::max(0, sw.order_window.v) / 16 * 16 : 64;
	for (int sl = 0; sl < P.slots; sl++) {
		const int64_t lo = std::min<int64_t>((int64_t)sl * B.ids_per_wg, n_blk), hi = std::min<int64_t>(lo + B.ids_per_wg, n_blk);
		if (B.parts) {
			// tasks of 8 consecutive blocks run as long as their longest list IN EVERY PART: blocks with the same profile of
			// part lengths belong together (measured on N_dn = 38760 in 3 parts: 1.11 instead of 1.19 gathers issued per entry)
			const int nparts = B.nparts;
			const int64_t pbk = B.part_blocks;
			auto profile = [&](int32_t b, int* out) {
				for (int q = 0; q < nparts; q++) out[q] = 0;
				for (int64_t p = cp[(size_t)b]; p < cp[(size_t)b + 1]; p++) out[std::min<int64_t>(P.cc[(size_t)p] / pbk, nparts - 1)]++;
			};
			std::stable_sort(order.begin() + lo, order.begin() + hi, [&](int32_t x, int32_t y) {
				int px[kPbMaxParts], py[kPbMaxParts];
				profile(x, px);
				profile(y, py);
				for (int q = 0; q < nparts; q++)
					if (px[q] != py[q]) return px[q] > py[q];
				return false;
			});
		} else {
			// sorted inside windows of `ow` consecutive blocks (a multiple of 16; 0: the whole range at once)
			const int64_t ow = order_window > 0 ? order_window : hi - lo;
			for (int64_t w0 = lo; w0 < hi; w0 += ow)
				std::stable_sort(order.begin() + w0, order.begin() + std::min(w0 + ow, hi), [&](int32_t x, int32_t y) { return cp[(size_t)x + 1] - cp[(size_t)x] > cp[(size_t)y + 1] - cp[(size_t)y]; });
		}
	}
}

// k_pb_down geometry: one workgroup per CU, 8 groups; the couplings of a workgroup's blocks must fit LDS
lpp_status plan_down_geometry(const PbSwitches& sw, const Choice& c, int num_cus, int64_t longest_list, PbPlan& P)
{
	PbForm& B = P.form;
	int grid = num_cus & ~7;
	// LPP_PB_DOWN_GRID=n (diagnostic): n workgroups instead of one per CU, a multiple of 8 from 8 up to that -- the ranges of hundreds of blocks
	// per workgroup that only the largest sectors have (the 64-block unit of plan_rounds, more than 64 tasks per step) on a matrix of test size
	if (sw.down_grid.set && grid >= 8) grid = std::max(8, std::min(sw.down_grid.v, grid)) & ~7;
	if (grid < 8) grid = num_cus; // fewer than 8 CUs: one group
	P.slots = grid >= 8 ? grid / 8 : grid;
	B.rowcap = (int)std::max<int64_t>(4, (longest_list + 3) & ~(int64_t)3);
	B.ids_per_wg = (int)((B.n_blk + P.slots - 1) / P.slots);
	B.down_grid = grid;
	B.down_rounds = 1;
	B.ids_per_round = B.ids_per_wg;
	if (!B.parts) plan_rounds(sw, c, B); // (the parts form has an image of its own)
	B.down_lds = pb_down_lds_bytes(B.ids_per_round, B.rowcap);
	B.down_lds_pf = B.down_lds + pb_down_task_sum_bytes(B.ids_per_round); // the counter-scheduled form where that fits the same bound (pb_down_pf_fits)
	if (B.parts) {
		const lpp_status rc = plan_parts(P);
		if (rc != LPP_OK) return rc;
	}
	if (B.down_lds > kPbDownLdsMax) return fail(LPP_ERR_INVALID, "pb_build: block couplings of a workgroup exceed LDS");
	plan_order(sw, P);
	// the LDS images of all (workgroup, round) pairs, made once: a round then starts with a copy instead of a walk through the lists
	// ((7,6) sector of the 4x5 lattice forced into two rounds: coupling kernel 33.2 ms in one round, 43.0 ms rebuilding)
	if (B.down_rounds > 1 && !sw.down_image.off()) P.image_bytes = pb_down_lds_bytes(B.ids_per_round, B.rowcap) * (size_t)P.slots * (size_t)B.down_rounds;
	if (!sw.pace.off()) P.pace_counters = 8 * (B.parts ? (size_t)B.pace_stride : (size_t)(std::max(B.pitch, B.pitch_dn) / 16));
	return LPP_OK;
}

// the launch forms, decided here once: a launch reads these fields, never the environment
void plan_launch_forms(const PbSwitches& sw, PbForm& B)
{
	const bool pf_fits = pb_down_pf_fits(B), l2 = pb_panel_fits_l2(B.n_blk);
	// (more than two value groups -- complex hoppings realified, t-t' models -- take the any-number-of-groups path of k_pb_up)
	B.chain_ok = sw.chain.value_or(1) != 0 && !B.tx && !B.big && !B.parts && !B.wide && B.down_rounds == 1 && B.c_nnz > 0 && B.G >= 1 && B.G <= kPbMaxGroups;
	B.down_tasks = pf_fits && sw.down_tasks.value_or(l2 ? 1 : 0) != 0;
	B.down_pf = pf_fits && sw.down_pf.value_or(1) != 0;
	B.chain_drop_pace = B.down_pf && l2 && sw.chain_pace.value_or(0) == 0;
}
} // namespace

lpp_status pb_plan(const PbBuildInput& in, const PbSwitches& sw, int num_cus, PbPlan& P)
{
	P = PbPlan();
	Choice c;
	int64_t longest = 1;
	lpp_status rc;
	if ((rc = plan_form(in, sw, P.form, c)) != LPP_OK) return rc;
	if ((rc = plan_segments(in, c, P)) != LPP_OK) return rc;
	if ((rc = plan_template(in, sw, c, P)) != LPP_OK) return rc;
	if ((rc = plan_couplings(in, P, &longest)) != LPP_OK) return rc;
	if ((rc = plan_down_geometry(sw, c, num_cus, longest, P)) != LPP_OK) return rc;
	plan_launch_forms(sw, P.form);
	return pb_check_instances(P.form);
}

lpp_status pb_check_instances(const PbForm& B)
{
	const char* missing = nullptr;
	auto need = [&](int index, const char* kernel) {
		if (index < 0 && !missing) missing = kernel;
	};
	for (const bool dot : { false, true }) {
		if (B.seg) need(inst_index(kPbSegInsts, pb_seg_inst(B, dot)), "k_pb_up_seg");
		else if (B.big2) need(inst_index(kPbBig2Insts, pb_big2_inst(B, dot)), "k_pb_up_big2");
		else if (B.big) need(inst_index(kPbBigInsts, pb_big_inst(B, dot)), "k_pb_up_big");
		else need(inst_index(kPbUpInsts, pb_up_inst(B, dot, false)), "k_pb_up");
	}
	if (B.parts) need(inst_index(kPbPartsInsts, pb_parts_inst(B)), "k_pb_down_parts");
	else need(inst_index(kPbDownInsts, pb_down_inst(B, false)), "k_pb_down");
	if (B.chain_ok) {
		need(inst_index(kPbUpInsts, pb_up_inst(B, false, true)), "k_pb_up (chained)");
		need(inst_index(kPbDownInsts, pb_down_inst(B, true)), "k_pb_down (chained)");
	}
	if (missing) return fail(LPP_ERR_INVALID, std::string("pb_build: no kernel instance for ") + missing + " of this form");
	return LPP_OK;
}

void pb_plan_print(const PbPlan& P)
{
	const PbForm& B = P.form;
	const SegPlan& SP = P.seg;
	const PbTemplate& T = P.T;
	if (P.seg_tried)
		fprintf(stderr, "lpp: segmented in-block form %s (L = %d, n = %d, %d high sites, %zu segments, %zu items of <= %d positions, %d types, %.2f MB)\n", B.seg ? "taken" : "does not apply",
		        SP.L, SP.n, SP.s, SP.segs.size(), SP.items.size(), SP.wmax, SP.ntypes, (SP.words.size() * 4 + SP.xwords.size() * 4) / 1048576.0);
	fprintf(stderr, "lpp: product-basis rows %s (pieces %d, exchange %d, blocks %lld of %lld, %lld positions)\n", !B.seg && !P.perm.empty() ? "stored by list length" : "in basis order", B.big ? 1 : 0, B.tx ? 1 : 0, (long long)B.nblk_loc, (long long)B.n_blk, (long long)B.n_up);
	if (!B.seg) { // list lengths of the packed template: chunks of 4 slots per (slice, group), far slots per slice
		int hist[kPbMaxGroups][9] = { { 0 } }, fh[9] = { 0 };
		for (int j = 0; j < T.spb; j++) {
			for (int g = 0; g < T.G; g++) hist[g][std::min<int>(T.len[(size_t)j * T.G + g], 8)]++;
			if (!T.flen.empty()) fh[std::min<int>((T.flen[(size_t)j] + 3) / 4, 8)]++;
		}
		for (int g = 0; g < T.G; g++) fprintf(stderr, "lpp: template group %d: slices with 0..8+ chunks: %d %d %d %d %d %d %d %d %d\n", g, hist[g][0], hist[g][1], hist[g][2], hist[g][3], hist[g][4], hist[g][5], hist[g][6], hist[g][7], hist[g][8]);
		if (!T.flen.empty()) fprintf(stderr, "lpp: template far slots / 4 per slice 0..8+: %d %d %d %d %d %d %d %d %d; %lld entries in pieces, %lld far\n", fh[0], fh[1], fh[2], fh[3], fh[4], fh[5], fh[6], fh[7], fh[8], (long long)T.entries, (long long)T.far_entries);
	}
	fprintf(stderr, "lpp: coupling kernel grid %d (%d workgroups per group, %d blocks each in %d rounds of %d)\n", B.down_grid, P.slots, B.ids_per_wg, B.down_rounds, B.ids_per_round);
	fprintf(stderr, "lpp: product-basis launch forms: chain %d, down tasks %d, chained counter form %d, pacing dropped %d, lazy exchange %d\n", B.chain_ok ? 1 : 0,
	        B.down_tasks ? 1 : 0, B.down_pf ? 1 : 0, B.chain_drop_pace ? 1 : 0, B.lazy_tx ? 1 : 0);
}

} // namespace lpp
