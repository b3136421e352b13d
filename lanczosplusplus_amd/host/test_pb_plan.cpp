// test_pb_plan.cpp -- the planner of the product-basis layout (csrc/lpp_pb_plan.h) in a stand-alone program, meant to be built together with
// lpp_host.cpp, lpp_pbseg_host.cpp and lpp_pb_plan.cpp under -fsanitize=address,undefined and run on the CPU (tests/test_host_logic.py does).
// Inputs are made here: the hopping matrix of one species on a ring or open chain, enumerated from bit words, as T, and that of another species
// as the block couplings C.  Over small species, block counts, CU counts, the exchange on and off and the forced forms it checks what every plan
// must satisfy (permutations, P T P^T, the chunk-pair repack, coupling codes, block bases, block order, rounds, part starts, LDS bounds), the
// launch forms at the sizes of the suite's 2x6 ladder, the coupling kernel's geometry at 256 CUs for the cases of tests/test_gpu_pb_down_edges.py
// (the forced grid and forced rounds included), the text of every refusal these sizes reach, and the kernel instance lists (csrc/lpp_pb_instances.h):
// their sizes, that every plan made here finds its kernels in them, and that a form without an instance is refused.
// Prints `ok` and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lpp_pb_instances.h"
#include "lpp_pb_plan.h"

using namespace lpp;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond) && failures++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
	} while (0)

struct Csr {
	int64_t n = 0;
	std::vector<int64_t> rp;
	std::vector<int32_t> ci;
	std::vector<double> va; // one double per entry, or (re, im) pairs
};

// hopping matrix of n particles on L sites (nearest neighbours, ring or open) in the basis of the ascending L-bit words: entry = t x (-1)^(particles
// strictly between the two sites); phase != 0: complex hoppings t e^{+-i phase}, values as (re, im) pairs
Csr species(int L, int n, bool ring, double t, double phase = 0.0)
{
	std::vector<uint32_t> words;
	for (uint32_t w = 0; w < (1u << L); w++)
		if (__builtin_popcount(w) == n) words.push_back(w);
	Csr A;
	A.n = (int64_t)words.size();
	A.rp.assign(1, 0);
	std::vector<std::pair<int32_t, std::pair<double, double>>> row;
	for (const uint32_t w : words) {
		row.clear();
		for (int b = 0; b < (ring && L > 2 ? L : L - 1); b++)
			for (int dir = 0; dir < 2; dir++) {
				const int from = dir ? b : (b + 1) % L, to = dir ? (b + 1) % L : b;
				if (!((w >> from) & 1) || ((w >> to) & 1)) continue;
				const uint32_t w2 = w ^ (1u << from) ^ (1u << to);
				const int lo = std::min(from, to), hi = std::max(from, to);
				const uint32_t between = w & ((1u << hi) - 1) & ~((1u << (lo + 1)) - 1);
				const double s = (__builtin_popcount(between) & 1) ? -t : t;
				const int32_t col = (int32_t)(std::lower_bound(words.begin(), words.end(), w2) - words.begin());
				row.push_back({ col, { s * std::cos(phase), (dir ? s : -s) * std::sin(phase) } });
			}
		std::sort(row.begin(), row.end());
		for (const auto& en : row) {
			A.ci.push_back(en.first);
			A.va.push_back(en.second.first);
			if (phase != 0.0) A.va.push_back(en.second.second);
		}
		A.rp.push_back((int64_t)A.ci.size());
	}
	return A;
}

bool same_bits(const double* a, const double* b, int n = 1) { return std::memcmp(a, b, 8 * (size_t)n) == 0; }

// the sorted dictionary pb_build is given: +0.0 first, keys ascending by bit pattern, the last one repeated
std::vector<double> dict_of(const std::vector<double>& values, int* ndict)
{
	std::vector<uint64_t> keys(1, 0);
	for (const double v : values) {
		uint64_t k;
		std::memcpy(&k, &v, 8);
		if (std::find(keys.begin(), keys.end(), k) == keys.end()) keys.push_back(k);
	}
	std::sort(keys.begin(), keys.end());
	std::vector<double> d(256);
	for (size_t i = 0; i < 256; i++) std::memcpy(&d[i], &keys[std::min(i, keys.size() - 1)], 8);
	*ndict = (int)keys.size();
	return d;
}

// one problem: T, C and what points at them
struct Problem {
	Csr T, C, Tc, Cc; // Tc / Cc: the complex matrices (T is then the realified one)
	std::vector<double> dict;
	PbCplxInput cx;
	PbBuildInput in;
};
void make_problem(Problem& p, const Csr& T, const Csr& C, bool tx)
{
	p.T = T;
	p.C = C;
	int ndict = 0;
	p.dict = dict_of(C.va, &ndict);
	PbBuildInput& in = p.in;
	in = PbBuildInput();
	in.n_up = p.T.n;
	in.n_blk = p.C.n;
	in.t_rp = p.T.rp.data();
	in.t_ci = p.T.ci.data();
	in.t_va = p.T.va.data();
	in.c_rp = p.C.rp.data();
	in.c_ci = p.C.ci.data();
	in.c_va = p.C.va.data();
	in.dict256 = p.dict.data();
	in.ndict = ndict;
	if (tx) { // the first of two ranks
		in.blk0 = 0;
		in.nblk_loc = (p.C.n + 1) / 2;
		in.pitch_dn = pb_pitch_for((p.T.n + 1) / 2);
		in.nblk_padded = (p.C.n + 1) / 2 * 2;
	}
}
void make_complex_problem(Problem& p, const Csr& Tc, const Csr& Cc)
{
	p.Tc = Tc;
	p.Cc = Cc;
	pb_realify(Tc.n, p.Tc.rp.data(), p.Tc.ci.data(), p.Tc.va.data(), p.T.rp, p.T.ci, p.T.va);
	p.T.n = 2 * Tc.n;
	p.dict.assign(256, 0.0);
	p.cx = PbCplxInput { Tc.n, p.Tc.rp.data(), p.Tc.ci.data(), p.Tc.va.data(), p.Cc.va.data() };
	PbBuildInput& in = p.in;
	in = PbBuildInput();
	in.n_up = p.T.n;
	in.n_blk = Cc.n;
	in.t_rp = p.T.rp.data();
	in.t_ci = p.T.ci.data();
	in.t_va = p.T.va.data();
	in.c_rp = p.Cc.rp.data();
	in.c_ci = p.Cc.ci.data();
	in.dict256 = p.dict.data();
	in.ndict = 1;
	in.cx = &p.cx;
}

bool is_permutation_of(std::vector<int32_t> v, int64_t lo, int64_t hi)
{
	std::sort(v.begin(), v.end());
	if ((int64_t)v.size() != hi - lo) return false;
	for (int64_t k = lo; k < hi; k++)
		if (v[(size_t)(k - lo)] != k) return false;
	return true;
}

// the in-block part of a plan that is not segmented: the row order, P T P^T and the repack against a template packed here
void check_rows(const PbBuildInput& in, const PbSwitches& sw, const PbPlan& P)
{
	const PbForm& B = P.form;
	const int64_t n = in.n_up;
	std::vector<int32_t> perm, inv;
	std::vector<int64_t> p_rp;
	std::vector<int32_t> p_ci;
	std::vector<double> p_va;
	if (!P.perm.empty()) {
		pb_list_length_order(in, perm, inv, p_rp, p_ci, p_va);
		CHECK(perm == P.perm && inv == P.inv);
		CHECK(n >= 128 && !B.big && !B.tx && !in.cx);
		if (perm.empty()) return;
		CHECK(p_rp.back() == in.t_rp[n]);
		for (int64_t q = 0; q < n; q++) { // row q of P T P^T is row perm[q] of T with columns mapped through inv, ascending
			const int64_t i = perm[(size_t)q];
			CHECK(p_rp[(size_t)q + 1] - p_rp[(size_t)q] == in.t_rp[i + 1] - in.t_rp[i]);
			for (int64_t k = p_rp[(size_t)q]; k < p_rp[(size_t)q + 1]; k++) {
				CHECK(k == p_rp[(size_t)q] || p_ci[(size_t)k - 1] < p_ci[(size_t)k]);
				bool found = false;
				for (int64_t m = in.t_rp[i]; m < in.t_rp[i + 1]; m++) found = found || (inv[(size_t)in.t_ci[m]] == p_ci[(size_t)k] && same_bits(&in.t_va[m], &p_va[(size_t)k]));
				CHECK(found);
			}
		}
	} else
		CHECK(n < 128 || B.big || B.tx || in.cx || sw.perm.off() || B.nblk_loc != B.n_blk);
	PbTemplate T0;
	const int ways = std::max(1, std::min(sw.bank_ways.value_or(2), 4));
	const lpp_status rc = perm.empty() ? pb_pack_template(n, B.pitch, in.t_rp, in.t_ci, in.t_va, T0, ways, B.W) : pb_pack_template(n, B.pitch, p_rp.data(), p_ci.data(), p_va.data(), T0, ways, B.W);
	CHECK(rc == LPP_OK);
	CHECK(T0.len == P.T.len && T0.G == B.G && T0.spb == B.spb && T0.entries == B.t_entries);
	CHECK((int64_t)P.T.words.size() == B.tw_words);
	if (B.big || !kPbPairs) {
		CHECK(T0.words == P.T.words && T0.off == P.T.off && T0.fwords == P.T.fwords && T0.foff == P.T.foff && T0.flen == P.T.flen);
		return;
	}
	// undoing the chunk pairs gives back the packed words: pair q of list i holds chunks 2q and 2q + 1, lane by lane
	for (size_t i = 0; i < T0.off.size(); i++)
		for (int ch = 0; ch < T0.len[i]; ch++)
			for (int l = 0; l < 64; l++)
				for (int k = 0; k < 2; k++) {
					const size_t at = ((size_t)P.T.off[i] + (size_t)(ch / 2)) * 256 + (size_t)l * 4 + (size_t)(ch & 1) * 2 + (size_t)k;
					CHECK(at < P.T.words.size() && P.T.words[at] == T0.words[((size_t)T0.off[i] + (size_t)ch) * 128 + (size_t)l * 2 + (size_t)k]);
				}
}

void check_plan(const PbBuildInput& in, const PbSwitches& sw, int num_cus, const PbPlan& P)
{
	const PbForm& B = P.form;
	const int64_t n_blk = in.n_blk;
	CHECK(B.n_up == in.n_up && B.n_blk == n_blk && B.pitch == pb_pitch_for(in.n_up) && B.tx == (in.pitch_dn > 0));
	// the stored order of the rows
	CHECK(P.perm.size() == P.inv.size());
	if (!P.perm.empty()) {
		CHECK(is_permutation_of(P.perm, 0, in.n_up));
		for (int64_t q = 0; q < in.n_up; q++) CHECK(P.perm[(size_t)q] >= 0 && P.perm[(size_t)q] < in.n_up && P.inv[(size_t)P.perm[(size_t)q]] == q);
	}
	if (!B.seg) check_rows(in, sw, P);
	CHECK(B.big == (B.W > 0) && (!B.seg || B.big) && (!B.big2 || B.big));
	// couplings: every code decodes to its value bit for bit; the block bases end at nnz
	size_t at = 0;
	for (int64_t b = 0; b < n_blk; b++) {
		for (int64_t p = in.c_rp[b]; p < in.c_rp[b + 1]; p++) {
			if (in.c_ci[p] == b) continue;
			CHECK(at < P.cc.size() && P.cc[at] == in.c_ci[p]);
			if (at >= P.cc.size()) return;
			if (in.cx) CHECK(same_bits(&P.cdict[2 * (size_t)P.ccode[at]], &in.cx->c_va[2 * p], 2));
			else CHECK(P.ccode[at] < in.ndict && same_bits(&P.dict[P.ccode[at]], &in.c_va[p]));
			at++;
		}
		CHECK(P.cp[(size_t)b + 1] == (int64_t)at);
	}
	CHECK(B.c_nnz == (int64_t)at && P.ccode.size() == at);
	CHECK(P.base.size() == (size_t)n_blk + 1 && P.base.back() == B.nnz && P.base[0] == 0);
	CHECK(B.nnz_loc == P.base[(size_t)(B.blk0 + B.nblk_loc)] - P.base[(size_t)B.blk0]);
	CHECK(in.cx ? P.cdict.size() == 512 : P.cdict.empty());
	// the coupling kernel's geometry
	int want_grid = num_cus >= 8 ? (num_cus & ~7) : num_cus;
	if (sw.down_grid.set && num_cus >= 8) want_grid = std::max(8, std::min(sw.down_grid.v, want_grid)) & ~7; // LPP_PB_DOWN_GRID: a multiple of 8 from 8 to the CUs'
	CHECK(B.down_grid == want_grid && B.down_grid <= std::max(num_cus, 1) && P.slots == (num_cus >= 8 ? B.down_grid / 8 : num_cus));
	CHECK((int64_t)B.ids_per_wg * P.slots >= n_blk && (int64_t)(B.ids_per_wg - 1) * P.slots < n_blk);
	CHECK(B.rowcap % 4 == 0 && B.rowcap >= 4);
	for (int64_t b = 0; b < n_blk; b++) CHECK(P.cp[(size_t)b + 1] - P.cp[(size_t)b] <= B.rowcap);
	CHECK((int64_t)B.ids_per_round * B.down_rounds >= B.ids_per_wg && B.ids_per_wg > (int64_t)B.ids_per_round * (B.down_rounds - 1));
	CHECK(B.down_lds <= kPbDownLdsMax);
	if (!B.parts) {
		CHECK(B.down_lds == pb_down_lds_bytes(B.ids_per_round, B.rowcap));
		CHECK(sw.down_rounds.set || B.down_rounds == 1); // (these sizes need no rounds by themselves)
		CHECK((P.image_bytes > 0) == (B.down_rounds > 1 && !sw.down_image.off()));
		CHECK(P.image_bytes == 0 || P.image_bytes == B.down_lds * (size_t)P.slots * (size_t)B.down_rounds);
	} else
		CHECK(B.down_rounds == 1 && P.image_bytes == 0 && B.down_lds == pb_parts_lds_bytes(B.ids_per_wg, B.ent_cap, B.nparts));
	CHECK(sw.pace.off() ? P.pace_counters == 0 : P.pace_counters >= 8);
	// the block order: a permutation of every workgroup's range; outside the parts form list lengths do not increase inside a sorting window
	CHECK(P.order.size() == (size_t)n_blk);
	auto len = [&](int32_t b) { return P.cp[(size_t)b + 1] - P.cp[(size_t)b]; };
	for (int sl = 0; sl < P.slots; sl++) {
		const int64_t lo = std::min<int64_t>((int64_t)sl * B.ids_per_wg, n_blk), hi = std::min<int64_t>(lo + B.ids_per_wg, n_blk);
		CHECK(is_permutation_of(std::vector<int32_t>(P.order.begin() + lo, P.order.begin() + hi), lo, hi));
		const int64_t ow = sw.order_window.set ? sw.order_window.v / 16 * 16 : 64;
		for (int64_t k = lo + 1; k < hi && !B.parts; k++)
			if (ow <= 0 || (k - lo) % ow != 0) CHECK(len(P.order[(size_t)k - 1]) >= len(P.order[(size_t)k]));
	}
	// the parts form: rows of pstart from 0 to the list length, monotone, every entry of part q with its source block in part q
	CHECK(B.parts == (B.nparts > 1 || sw.parts.set));
	if (B.parts) {
		CHECK(B.part_blocks == (n_blk + B.nparts - 1) / B.nparts && P.pstart.size() == (size_t)n_blk * (size_t)(B.nparts + 1));
		for (int64_t b = 0; b < n_blk; b++) {
			const int32_t* ps = P.pstart.data() + (size_t)b * (size_t)(B.nparts + 1);
			CHECK(ps[0] == 0 && ps[B.nparts] == len((int32_t)b));
			for (int q = 0; q < B.nparts; q++) {
				CHECK(ps[q] <= ps[q + 1]);
				for (int32_t k = ps[q]; k < ps[q + 1]; k++) CHECK(std::min<int64_t>(P.cc[(size_t)(P.cp[(size_t)b] + k)] / B.part_blocks, B.nparts - 1) == q);
			}
		}
		CHECK(B.maxr % 4 == 0 && B.maxr * 8 * (kPbPartsThreads / 64) >= B.ids_per_wg && B.pace_stride > 0);
	} else
		CHECK(P.pstart.empty());
	// LDS of the in-block kernel the form takes
	if (B.seg) CHECK(pb_seg_lds_bytes(B.seg_ws, B.seg_wmax, B.seg_one ? 1 : 2) <= kPbUpLdsMax && B.npieces == B.seg_nitems);
	else if (B.big) CHECK(pb_big_lds_bytes(B.W) <= kPbUpLdsMax && (int64_t)B.npieces * B.W >= in.n_up && (!B.big2 || pb_big2_lds_bytes(B.W) <= kPbUpLdsMax));
	else CHECK(pb_up_lds_bytes(B.pitch, B.spb, B.G) <= kPbUpLdsMax && B.npieces == 1);
	// launch forms never outrun what was planned
	CHECK(!B.chain_ok || (!B.tx && !B.big && !B.parts && !B.wide && B.down_rounds == 1 && B.c_nnz > 0));
	CHECK((!B.down_tasks && !B.down_pf) || B.down_lds_pf <= kPbDownLdsMax);
	CHECK(B.lazy_tx == (B.tx && sw.lazy_tx.value_or(1) != 0));
}

EnvSwitch on(int v)
{
	EnvSwitch s;
	s.set = true;
	s.v = v;
	return s;
}

struct Forced {
	const char* name;
	PbSwitches sw;
};
std::vector<Forced> forced_forms()
{
	std::vector<Forced> f;
	f.push_back({ "default", PbSwitches() });
	for (const int w : { 64, 128 }) {
		f.push_back({ "pieces", PbSwitches() });
		f.back().sw.piece_rows = on(w);
		f.push_back({ "pieces, one block", f.back().sw });
		f.back().sw.big2 = on(0);
		f.push_back({ "segments", PbSwitches() });
		f.back().sw.piece_rows = on(w);
		f.back().sw.seg = on(1);
	}
	for (const int q : { 1, 2, 3 }) {
		f.push_back({ "parts", PbSwitches() });
		f.back().sw.parts = on(q);
	}
	for (const int r : { 2, 3 }) {
		f.push_back({ "rounds", PbSwitches() });
		f.back().sw.down_rounds = on(r);
		f.push_back({ "rounds, no image, no pacing, whole-range order", f.back().sw });
		f.back().sw.down_image = on(0);
		f.back().sw.pace = on(0);
		f.back().sw.order_window = on(0);
	}
	for (const int g : { 8, 20, 4096, -3 }) { // the forced grid: as given, rounded down to a multiple of 8, clamped from above and from below
		f.push_back({ "grid", PbSwitches() });
		f.back().sw.down_grid = on(g);
	}
	f.push_back({ "grid 8, rounds", PbSwitches() });
	f.back().sw.down_grid = on(8);
	f.back().sw.down_rounds = on(2);
	f.push_back({ "basis order, wide", PbSwitches() });
	f.back().sw.perm = on(0);
	f.back().sw.wide = on(1);
	f.back().sw.pre0 = on(6);
	return f;
}

void check_keys(const PbForm& B); // (kernel instances: below)
void note_shape(const PbForm& B);

int plans = 0, refused = 0, seen_perm = 0, seen_seg = 0, seen_big2 = 0, seen_rounds3 = 0, seen_parts3 = 0, seen_two_groups = 0;
void run(const Problem& p, const PbSwitches& sw, int num_cus)
{
	PbPlan P;
	const lpp_status rc = pb_plan(p.in, sw, num_cus, P);
	if (rc != LPP_OK) { // a combination the layout does not hold: a refusal in the build's words, nothing else
		CHECK(rc == LPP_ERR_INVALID && std::strncmp(lpp_last_error(), "pb_build: ", 10) == 0);
		refused++;
		return;
	}
	plans++;
	check_plan(p.in, sw, num_cus, P);
	check_keys(P.form);
	note_shape(P.form);
	seen_perm += !P.form.seg && !P.perm.empty();
	seen_seg += P.form.seg;
	seen_big2 += P.form.big2 && !P.form.seg;
	seen_rounds3 += P.form.down_rounds == 3;
	seen_parts3 += P.form.nparts == 3;
	seen_two_groups += P.form.G == 2;
}

void expect_refusal(const PbBuildInput& in, const PbSwitches& sw, const char* text)
{
	PbPlan P;
	const lpp_status rc = pb_plan(in, sw, 256, P);
	if (rc != LPP_ERR_INVALID || std::string(lpp_last_error()) != text) {
		if (failures++ < 20) std::printf("FAILED refusal: wanted \"%s\", got status %d \"%s\"\n", text, (int)rc, lpp_last_error());
	}
}

void check_refusals()
{
	const Csr T5 = species(5, 1, true, -1.0), C15 = species(6, 2, false, -1.0);
	Problem p;
	make_problem(p, T5, C15, false);
	{
		Problem q;
		make_problem(q, T5, C15, false);
		std::swap(q.T.ci[0], q.T.ci[1]); // (row 0 of the ring has two entries)
		expect_refusal(q.in, PbSwitches(), "pb_build: in-block rows must be sorted by column");
	}
	{
		Problem q;
		make_problem(q, T5, C15, false);
		int64_t b = 0;
		while (q.C.rp[(size_t)b + 1] - q.C.rp[(size_t)b] < 2) b++;
		std::swap(q.C.ci[(size_t)q.C.rp[(size_t)b]], q.C.ci[(size_t)q.C.rp[(size_t)b] + 1]);
		expect_refusal(q.in, PbSwitches(), "pb_build: block couplings must be sorted");
		make_problem(q, T5, C15, false);
		q.C.ci.back() = 15;
		expect_refusal(q.in, PbSwitches(), "pb_build: block coupling out of range");
		make_problem(q, T5, C15, false);
		q.C.va[0] = 0.5;
		expect_refusal(q.in, PbSwitches(), "pb_build: coupling value missing from the dictionary");
	}
	{ // 300 blocks in a line, every coupling with a value of its own: the 257th is one too many
		Csr Tc = species(5, 1, true, -1.0, 0.3), Cc;
		Cc.n = 300;
		Cc.rp.assign(1, 0);
		for (int64_t b = 0; b < Cc.n; b++) {
			if (b + 1 < Cc.n) {
				Cc.ci.push_back((int32_t)(b + 1));
				Cc.va.push_back(1.0 + (double)b);
				Cc.va.push_back(0.25);
			}
			Cc.rp.push_back((int64_t)Cc.ci.size());
		}
		Problem q;
		make_complex_problem(q, Tc, Cc);
		expect_refusal(q.in, PbSwitches(), "pb_build: more than 256 distinct complex coupling values");
		PbSwitches sw;
		sw.parts = on(2);
		expect_refusal(q.in, sw, "pb_build: complex hoppings are held in the single-GPU forms with whole-panel couplings only");
	}
	{ // block 0 coupled to 1021 others, parts form
		Csr C;
		C.n = 1100;
		C.rp.assign(1, 0);
		for (int32_t k = 1; k <= 1021; k++) {
			C.ci.push_back(k);
			C.va.push_back(-1.0);
		}
		C.rp.resize((size_t)C.n + 1, 1021);
		Problem q;
		make_problem(q, T5, C, false);
		PbSwitches sw;
		sw.parts = on(2);
		expect_refusal(q.in, sw, "pb_build: coupling list too long");
	}
	{ // item 6: 16-bit block numbers of the parts form; empty coupling lists
		Csr C;
		C.n = 65536;
		C.rp.assign((size_t)C.n + 1, 0);
		Problem q;
		make_problem(q, T5, C, false);
		PbSwitches sw;
		sw.parts = on(2);
		expect_refusal(q.in, sw, "pb_build: the parts form holds 16-bit block numbers");
		PbPlan P; // the default path never takes parts there: it plans
		CHECK(pb_plan(q.in, PbSwitches(), 256, P) == LPP_OK && !P.form.parts);
	}
	{
		SegPlan ready;
		PbBuildInput in = p.in;
		in.pre = &ready;
		in.n_blk = 2;
		PbSwitches sw;
		sw.piece_rows = on(64);
		expect_refusal(in, sw, "pb_build: a ready-made plan is for one block beyond the LDS window");
	}
	{
		PbBuildInput in = p.in;
		in.blk0 = -1;
		expect_refusal(in, PbSwitches(), "pb_build: bad block range / coupling pitch");
		in = p.in;
		in.nblk_loc = 16;
		expect_refusal(in, PbSwitches(), "pb_build: bad block range / coupling pitch");
		in = p.in;
		in.pitch_dn = 8;
		in.nblk_padded = in.n_blk;
		expect_refusal(in, PbSwitches(), "pb_build: bad block range / coupling pitch");
		in.pitch_dn = 16;
		in.nblk_padded = in.n_blk - 1;
		expect_refusal(in, PbSwitches(), "pb_build: bad block range / coupling pitch");
	}
}

// tests/test_gpu_parity.py LAUNCH_FORMS at ladder_2x6's sizes: 924 blocks of 924 positions, 256 CUs
void check_launch_forms()
{
	const Csr S = species(12, 6, true, -1.0);
	CHECK(S.n == 924);
	Problem p;
	make_problem(p, S, S, false);
	struct Row {
		const char* name;
		EnvSwitch PbSwitches::*sw;
		int v;
		bool chain, down_tasks, down_pf, drop_pace, lazy;
	};
	const Row table[] = {
		{ "none", nullptr, 0, true, true, true, true, false },
		{ "chain0", &PbSwitches::chain, 0, false, true, true, true, false },
		{ "down_tasks0", &PbSwitches::down_tasks, 0, true, false, true, true, false },
		{ "down_pf0", &PbSwitches::down_pf, 0, true, true, false, false, false },
		{ "chain_pace1", &PbSwitches::chain_pace, 1, true, true, true, false, false },
	};
	for (const Row& r : table) {
		PbSwitches sw;
		if (r.sw) sw.*(r.sw) = on(r.v);
		PbPlan P;
		CHECK(pb_plan(p.in, sw, 256, P) == LPP_OK);
		const PbForm& B = P.form;
		if (B.chain_ok != r.chain || B.down_tasks != r.down_tasks || B.down_pf != r.down_pf || B.chain_drop_pace != r.drop_pace || B.lazy_tx != r.lazy) {
			if (failures++ < 20) std::printf("FAILED launch forms of %s: %d %d %d %d %d\n", r.name, B.chain_ok, B.down_tasks, B.down_pf, B.chain_drop_pace, B.lazy_tx);
		}
		CHECK(B.ids_per_wg == 29 && !B.big && !B.parts && B.down_rounds == 1);
		check_plan(p.in, sw, 256, P);
	}
}

// hopping matrix of n particles on L sites for any symmetric real hop[L * L] (zero: no bond), same basis and sign rule as species()
Csr species_of(int L, int n, const std::vector<double>& hop)
{
	std::vector<uint32_t> words;
	for (uint32_t w = 0; w < (1u << L); w++)
		if (__builtin_popcount(w) == n) words.push_back(w);
	Csr A;
	A.n = (int64_t)words.size();
	A.rp.assign(1, 0);
	std::vector<std::pair<int32_t, double>> row;
	for (const uint32_t w : words) {
		row.clear();
		for (int from = 0; from < L; from++)
			for (int to = 0; to < L; to++) {
				const double t = hop[(size_t)from * L + to];
				if (from == to || t == 0.0 || !((w >> from) & 1) || ((w >> to) & 1)) continue;
				const int lo = std::min(from, to), hi = std::max(from, to);
				const uint32_t between = w & ((1u << hi) - 1) & ~((1u << (lo + 1)) - 1);
				row.push_back({ (int32_t)(std::lower_bound(words.begin(), words.end(), w ^ (1u << from) ^ (1u << to)) - words.begin()), (__builtin_popcount(between) & 1) ? -t : t });
			}
		std::sort(row.begin(), row.end());
		for (const auto& en : row) {
			A.ci.push_back(en.first);
			A.va.push_back(en.second);
		}
		A.rp.push_back((int64_t)A.ci.size());
	}
	return A;
}
std::vector<double> hop_all_to_all(int L) // every pair of sites, +-1 (the signs do not enter the geometry: the suite's matrices draw them from a seed)
{
	std::vector<double> h((size_t)L * L, 0.0);
	for (int i = 0; i < L; i++)
		for (int j = 0; j < L; j++)
			if (i != j) h[(size_t)i * L + j] = ((i + j) & 1) ? -1.0 : 1.0;
	return h;
}
std::vector<double> hop_ring(int L, double t1, double t2) // nearest neighbours t1 on the ring, second neighbours t2 on the open chain
{
	std::vector<double> h((size_t)L * L, 0.0);
	for (int i = 0; i < L; i++) {
		h[(size_t)i * L + (i + 1) % L] = h[(size_t)((i + 1) % L) * L + i] = t1;
		if (i + 2 < L) h[(size_t)i * L + i + 2] = h[(size_t)(i + 2) * L + i] = t2;
	}
	return h;
}

// tests/test_gpu_pb_down_edges.py: the coupling kernel's geometry at 256 CUs for every case of that file, under the forced grid and the forced rounds
void check_down_edge_cases()
{
	struct Want {
		int slots, ids_per_wg, rounds, ids_per_round, rowcap;
	};
	auto pin = [&](const char* name, const PbBuildInput& in, const PbSwitches& sw, const Want& w) {
		PbPlan P;
		if (pb_plan(in, sw, 256, P) != LPP_OK) {
			if (failures++ < 20) std::printf("FAILED down edges %s: refused \"%s\"\n", name, lpp_last_error());
			return PbPlan();
		}
		const PbForm& B = P.form;
		if (P.slots != w.slots || B.down_grid != 8 * w.slots || B.ids_per_wg != w.ids_per_wg || B.down_rounds != w.rounds || B.ids_per_round != w.ids_per_round || B.rowcap != w.rowcap) {
			if (failures++ < 20)
				std::printf("FAILED down edges %s: slots %d, grid %d, ids_per_wg %d, rounds %d, ids_per_round %d, rowcap %d\n", name, P.slots, B.down_grid, B.ids_per_wg, B.down_rounds, B.ids_per_round, B.rowcap);
		}
		check_plan(in, sw, 256, P);
		return P;
	};
	PbSwitches none, rounds2, grid8, grid8_rounds2, rounds2_rebuilt;
	rounds2.down_rounds = on(2);
	rounds2_rebuilt.down_rounds = on(2);
	rounds2_rebuilt.down_image = on(0);
	grid8.down_grid = on(8);
	grid8_rounds2.down_grid = on(8);
	grid8_rounds2.down_rounds = on(2);
	const std::vector<double> a8 = hop_all_to_all(8), a10 = hop_all_to_all(10), a12 = hop_all_to_all(12);
	Problem p;
	make_problem(p, species_of(8, 4, a8), species_of(8, 1, a8), false); // 8 blocks: 24 of the 32 workgroups of a group own nothing; lists of 7
	CHECK(p.in.n_up == 70 && p.in.n_blk == 8);
	pin("(8,4,1)", p.in, none, { 32, 1, 1, 1, 8 });
	make_problem(p, species_of(8, 4, a8), species_of(8, 3, a8), false); // lists of 15
	CHECK(p.in.n_blk == 56);
	pin("(8,4,3)", p.in, none, { 32, 2, 1, 2, 16 });
	make_problem(p, species_of(10, 3, a10), species_of(10, 5, a10), false); // lists of 25: 28 places, a stride of 28
	CHECK(p.in.n_blk == 252 && pb_down_stride(28) == 28);
	pin("(10,3,5)", p.in, none, { 32, 8, 1, 8, 28 });
	make_problem(p, species_of(12, 2, a12), species_of(12, 6, a12), false); // lists of 36
	CHECK(p.in.n_blk == 924 && p.in.n_up == 66);
	pin("(12,2,6)", p.in, none, { 32, 29, 1, 29, 36 });
	pin("(12,2,6) rounds 2", p.in, rounds2, { 32, 29, 2, 16, 36 }); // units of 8: 16 + 13
	{ // one workgroup per group owns all 924 blocks: 116 tasks, image and task sums inside 150 KB, so the counter forms and the chained step stay
		const PbPlan P = pin("(12,2,6) grid 8", p.in, grid8, { 1, 924, 1, 924, 36 });
		CHECK(P.form.down_lds == 140464 && P.form.down_lds_pf == 140464 + 116 * 32 && P.form.down_lds_pf <= kPbDownLdsMax);
		CHECK(P.form.chain_ok && P.form.down_pf && P.form.down_tasks && P.form.chain_drop_pace && P.image_bytes == 0);
		const PbPlan Q = pin("(12,2,6) grid 8 rounds 2", p.in, grid8_rounds2, { 1, 924, 2, 512, 36 }); // 512 blocks and more per workgroup: units of 64, 512 + 412
		CHECK(!Q.form.chain_ok && Q.image_bytes == 2 * pb_down_lds_bytes(512, 36));
	}
	{
		const std::vector<double> h = hop_ring(11, -1.0, 0.5);
		make_problem(p, species_of(11, 5, h), species_of(11, 4, h), false); // lists of 4 to 14, four coupling values, 29 panels
		CHECK(p.in.n_blk == 330 && p.in.ndict == 5 && pb_pitch_for(p.in.n_up) / 16 == 29);
		const PbPlan P = pin("t-t' (11,5,4)", p.in, none, { 32, 11, 1, 11, 16 });
		int64_t lo = 1 << 30;
		for (int64_t b = 0; b < 330; b++) lo = std::min(lo, P.cp[(size_t)b + 1] - P.cp[(size_t)b]);
		CHECK(lo == 4 && P.pace_counters == 8 * 29);
	}
	make_problem(p, species(14, 2, true, -1.0), species(14, 4, true, -1.0), false);
	CHECK(p.in.n_blk == 1001);
	pin("(14,2,4)", p.in, none, { 32, 32, 1, 32, 8 });
	pin("(14,2,4) rounds 2", p.in, rounds2, { 32, 32, 2, 16, 8 }); // the last workgroup owns 1001 - 31 * 32 = 9 blocks: its second round is empty
	pin("(14,2,4) rounds 2, rebuilt", p.in, rounds2_rebuilt, { 32, 32, 2, 16, 8 });
	{ // a last round that would be empty for EVERY workgroup is trimmed: 3 rounds of 16 blocks asked for 32 per workgroup
		PbSwitches rounds3;
		rounds3.down_rounds = on(3);
		pin("(14,2,4) rounds 3", p.in, rounds3, { 32, 32, 2, 16, 8 });
	}
	make_problem(p, species(15, 2, true, -1.0), species(15, 6, true, -1.0), false); // 20 tasks per workgroup against 16 waves
	CHECK(p.in.n_blk == 5005);
	pin("(15,2,6)", p.in, none, { 32, 157, 1, 157, 12 });
	{
		Problem q;
		make_complex_problem(q, species(11, 5, true, -1.0, 0.37), species(11, 4, true, -1.0, 0.37));
		CHECK(q.in.n_blk == 330 && q.in.n_up == 924);
		const PbPlan P = pin("Peierls (11,5,4)", q.in, none, { 32, 11, 1, 11, 8 });
		CHECK(P.form.cplx && P.form.chain_ok && P.pace_counters == 8 * 58);
		PbSwitches pf0;
		pf0.down_pf = on(0);
		const PbPlan Q = pin("Peierls (11,5,4), fixed shares", q.in, pf0, { 32, 11, 1, 11, 8 });
		CHECK(Q.form.cplx && Q.form.chain_ok && !Q.form.down_pf && !Q.form.chain_drop_pace); // k_pb_down<1024, true, false, true, false>
	}
}

// ---- kernel instances (csrc/lpp_pb_instances.h) -------------------------------------------------------------------------------------------
template <typename K, size_t N> bool no_duplicates(const std::array<K, N>& list)
{
	for (size_t i = 0; i < N; i++)
		for (size_t j = i + 1; j < N; j++)
			if (list[i] == list[j]) return false;
	return true;
}

// every kernel the launches of a planned form ask for, looked up key by key (what pb_plan's last step checks in one go)
void check_keys(const PbForm& B)
{
	CHECK(pb_check_instances(B) == LPP_OK);
	for (const bool dot : { false, true }) {
		if (B.seg) CHECK(inst_index(kPbSegInsts, pb_seg_inst(B, dot)) >= 0);
		else if (B.big2) CHECK(inst_index(kPbBig2Insts, pb_big2_inst(B, dot)) >= 0);
		else if (B.big) CHECK(inst_index(kPbBigInsts, pb_big_inst(B, dot)) >= 0);
		else CHECK(inst_index(kPbUpInsts, pb_up_inst(B, dot, false)) >= 0);
	}
	if (B.parts) CHECK(inst_index(kPbPartsInsts, pb_parts_inst(B)) >= 0 && pb_parts_inst(B).r == B.maxr);
	else CHECK(inst_index(kPbDownInsts, pb_down_inst(B, false)) >= 0);
	if (B.chain_ok) CHECK(inst_index(kPbUpInsts, pb_up_inst(B, false, true)) >= 0 && inst_index(kPbDownInsts, pb_down_inst(B, true)) >= 0);
}

// the up spins of a Heisenberg chain as ONE block of the segmented form, planned from the model and handed to pb_plan ready-made (pb_chain)
bool plan_chain(int L, int n, bool ring, PbPlan& P)
{
	std::vector<double> hv((size_t)L * L, 0.0);
	std::vector<int64_t> cnt((size_t)L * L, 0);
	for (int i = 0; i < (ring ? L : L - 1); i++) {
		const int j = (i + 1) % L;
		hv[(size_t)i * L + j] = hv[(size_t)j * L + i] = 0.5;
		cnt[(size_t)i * L + j] = cnt[(size_t)j * L + i] = 1;
	}
	SegPlan SP;
	bool ok = false;
	if (pb_seg_plan_model(L, n, hv, cnt, 64, SP, &ok, true) != LPP_OK || !ok) return false;
	const int64_t c_rp[2] = { 0, 0 };
	const std::vector<double> dict(256, 0.0);
	PbBuildInput in;
	in.n_up = SP.n_up;
	in.n_blk = 1;
	in.c_rp = c_rp;
	in.dict256 = dict.data();
	in.ndict = 1;
	in.pre = &SP;
	in.pre_nnz = 1;
	PbSwitches sw;
	sw.piece_rows = on(64);
	return pb_plan(in, sw, 256, P) == LPP_OK;
}

int seen_shape[kPbSegShapes.size()] = { 0 };
void note_shape(const PbForm& B)
{
	if (!B.seg) return;
	const int at = inst_index(kPbSegShapes, PbSegShape { B.seg_nc, B.seg_nh, B.seg_one ? 1 : 2 });
	CHECK(at >= 0);
	if (at >= 0) seen_shape[at]++;
}

void check_instances()
{
	CHECK(kPbUpInsts.size() == 15 && kPbBigInsts.size() == 8 && kPbBig2Insts.size() == 10 && kPbSegInsts.size() == 48 && kPbDownInsts.size() == 12 && kPbPartsInsts.size() == 6);
	CHECK(no_duplicates(kPbUpInsts) && no_duplicates(kPbBigInsts) && no_duplicates(kPbBig2Insts) && no_duplicates(kPbSegInsts) && no_duplicates(kPbDownInsts) && no_duplicates(kPbPartsInsts));
	CHECK(no_duplicates(kPbSegShapes) && no_duplicates(kPbSegDepths) && no_duplicates(kPbUpDepths) && no_duplicates(kPbBigDepths) && no_duplicates(kPbBig2Depths));
	CHECK(inst_index(kPbPartsInsts, PbPartsInst { 28 }) == -1 && inst_index(kPbPartsInsts, PbPartsInst { 24 }) == 5 && inst_index(kPbUpInsts, kPbUpInsts[7]) == 7);
	// LPP_PB_PRE0 = 0 .. 8 lands on a listed depth in the one-window form (216 blocks of 924 positions) and by pieces (k_pb_up_big2)
	const Csr S = species(12, 6, true, -1.0);
	Problem p;
	make_problem(p, S, species(9, 4, true, -1.0), false);
	for (int v = 0; v <= 8; v++)
		for (const bool pieces : { false, true }) {
			PbSwitches sw;
			sw.pre0 = on(v);
			if (pieces) sw.piece_rows = on(128);
			PbPlan P;
			CHECK(pb_plan(p.in, sw, 256, P) == LPP_OK && P.form.G == 2 && P.form.big2 == pieces && !P.form.seg);
			check_keys(P.form);
			const int want = pieces ? std::max(3, std::min(v, 5)) : kPbPairs ? std::max(2, std::min(v, 6)) & ~1 : std::max(3, std::min(v, 5));
			CHECK(P.form.pre0 == want);
		}
	// the shapes of the segmented kernel: two blocks per workgroup on rings and lattices, one block on chains
	struct Lattice {
		int L, n;
		std::vector<double> hop;
	};
	std::vector<Lattice> lattices;
	lattices.push_back({ 10, 4, hop_ring(10, -1.0, 0.0) });
	lattices.push_back({ 12, 6, hop_ring(12, -1.0, 0.0) });
	{ // a 4 x 3 lattice, periodic in both directions
		std::vector<double> h(144, 0.0);
		for (int x = 0; x < 4; x++)
			for (int y = 0; y < 3; y++) {
				const int i = x + 4 * y, r = (x + 1) % 4 + 4 * y, u = x + 4 * ((y + 1) % 3);
				h[(size_t)i * 12 + r] = h[(size_t)r * 12 + i] = -1.0;
				h[(size_t)i * 12 + u] = h[(size_t)u * 12 + i] = -1.0;
			}
		lattices.push_back({ 12, 6, h });
	}
	for (const Lattice& l : lattices) {
		make_problem(p, species_of(l.L, l.n, l.hop), species(6, 2, false, -1.0), false);
		PbSwitches sw;
		sw.piece_rows = on(64);
		sw.seg = on(1);
		PbPlan P;
		CHECK(pb_plan(p.in, sw, 256, P) == LPP_OK);
		CHECK(P.form.seg && !P.form.seg_one);
		check_keys(P.form);
		note_shape(P.form);
	}
	// (open: one bond between the low and the high sites; 10 sites: 2 high-high hops per segment, 16: 8, 21: 13)
	for (const int L : { 10, 16, 21 })
		for (const bool ring : { false, true }) {
			PbPlan P;
			CHECK(plan_chain(L, L / 2, ring, P) && P.form.seg && P.form.seg_one);
			check_keys(P.form);
			note_shape(P.form);
		}
	for (size_t k = 0; k < kPbSegShapes.size(); k++) // every (NC, NH, blocks per workgroup) of the list was planned by some fixture above or in main
		if (seen_shape[k] == 0 && failures++ < 20) std::printf("FAILED no plan reached the shape (%d, %d, %d)\n", kPbSegShapes[k].nc, kPbSegShapes[k].nh, kPbSegShapes[k].rows);
	{ // a form whose lists were padded to a width no instance has is refused by the planner's last step, in the build's words
		PbPlan P;
		CHECK(plan_chain(10, 5, false, P));
		PbForm B = P.form;
		B.seg_nc = 3;
		CHECK(pb_check_instances(B) == LPP_ERR_INVALID && std::strncmp(lpp_last_error(), "pb_build: no kernel instance for k_pb_up_seg", 44) == 0);
		B = P.form;
		B.seg = false; // (pieces of one block: k_pb_up_big2 with three value groups has no instance either)
		B.big2 = true;
		B.G = 3;
		CHECK(pb_check_instances(B) == LPP_ERR_INVALID && std::strncmp(lpp_last_error(), "pb_build: no kernel instance for k_pb_up_big2", 45) == 0);
	}
}

} // namespace

int main()
{
	// 210 and 252 positions: above the 128 from which rows are reordered, no multiples of 64; 5 positions: basis order
	const Csr Ts[] = { species(10, 4, true, -1.0), species(10, 5, false, -1.0), species(5, 1, true, -1.0) };
	// 1 block without couplings, an odd number of blocks, and enough blocks for several rounds and parts
	const Csr Cs[] = { species(4, 0, true, -1.0), species(6, 2, false, -1.0), species(9, 4, true, -1.0) };
	CHECK(Ts[0].n == 210 && Ts[1].n == 252 && Ts[2].n == 5 && Cs[0].n == 1 && Cs[0].ci.empty() && Cs[1].n == 15 && Cs[2].n == 126);
	const std::vector<Forced> forms = forced_forms();
	for (const Csr& T : Ts)
		for (const Csr& C : Cs)
			for (const bool tx : { false, true }) {
				Problem p;
				make_problem(p, T, C, tx);
				for (const int num_cus : { 256, 8, 5 })
					for (const Forced& f : forms) run(p, f.sw, num_cus);
			}
	{ // complex hoppings, 3 distinct coupling values: the two directions of an open chain's hops conjugate, and one entry gets a value of its own
		const Csr Tc = species(8, 3, true, -1.0, 0.4);
		Csr Cc = species(6, 2, false, -0.5, 0.7);
		Cc.va[0] = 0.125;
		Problem p;
		make_complex_problem(p, Tc, Cc);
		for (const int num_cus : { 256, 8, 5 })
			for (const Forced& f : forms) run(p, f.sw, num_cus);
		PbPlan P;
		CHECK(pb_plan(p.in, PbSwitches(), 256, P) == LPP_OK && P.form.cplx && P.form.n_c == Tc.n);
		int distinct = 0;
		for (size_t k = 1; k < 256; k++) distinct += P.cdict[2 * k] != 0.0 || P.cdict[2 * k + 1] != 0.0;
		CHECK(distinct == 3);
	}
	CHECK(plans > 500 && refused > 0);
	CHECK(seen_perm > 0 && seen_seg > 0 && seen_big2 > 0 && seen_rounds3 > 0 && seen_parts3 > 0 && seen_two_groups > 0);
	check_refusals();
	check_launch_forms();
	check_down_edge_cases();
	check_instances();
	if (failures) {
		std::printf("%d checks failed (%d plans, %d refusals)\n", failures, plans, refused);
		return 1;
	}
	std::printf("%d plans, %d refusals\nok\n", plans, refused);
	return 0;
}
