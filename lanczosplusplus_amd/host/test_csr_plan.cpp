// test_csr_plan.cpp -- the decisions of the general CSR layout (csrc/lpp_csr_plan.h) without a GPU: a stand-alone program, built with the
// address and undefined-behaviour sanitizers by tests/test_host_logic.py.  Prints `ok`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lpp_csr_plan.h"

using namespace lpp;

#define CHECK(cond)                                                                                                    \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);                                   \
			exit(1);                                                                                                   \
		}                                                                                                              \
	} while (0)

namespace {

EnvSwitch on(int v)
{
	EnvSwitch s;
	s.set = true;
	s.v = v;
	return s;
}

void test_pick_group()
{
	const EnvSwitch none;
	// g = the largest power of two <= avg / 2, in [4, 64]: both sides of avg = 16, 32, 64, 128
	const struct {
		int64_t nnz;
		int g;
	} rows[] = { { 1000, 4 }, { 15999, 4 }, { 16000, 8 }, { 31999, 8 }, { 32000, 16 }, { 63999, 16 }, { 64000, 32 }, { 127999, 32 }, { 128000, 64 }, { 100000000, 64 } };
	for (const auto& r : rows) CHECK(pick_group(1000, r.nnz, none) == r.g);
	CHECK(pick_group(0, 0, none) == 4);
	for (int g : { 4, 8, 16, 32, 64 }) CHECK(pick_group(1000, 1000, on(g)) == g);
	CHECK(pick_group(1000, 64000, on(5)) == 32 && pick_group(1000, 64000, on(0)) == 32 && pick_group(1000, 64000, on(128)) == 32); // not a group: by itself
}

void test_geometry()
{
	SliceGeom g = slice_geom(10, 1);
	CHECK(g.nrows == 10 && g.B == 1 && g.spb == 1 && g.nblocks == 10 && g.nslices == 10);
	g = slice_geom(100, 100);
	CHECK(g.B == 100 && g.spb == 2 && g.nblocks == 1 && g.nslices == 2);
	g = slice_geom(100, 500); // B > nrows: one block of all rows
	CHECK(g.B == 100 && g.spb == 2 && g.nblocks == 1 && g.nslices == 2);
	g = slice_geom(1000, 300); // the last block is partial
	CHECK(g.B == 300 && g.spb == 5 && g.nblocks == 4 && g.nslices == 20);
	g = slice_geom(128, 64);
	CHECK(g.spb == 1 && g.nblocks == 2 && g.nslices == 2);
	g = slice_geom(0, 0);
	CHECK(g.B == 1 && g.nblocks == 0 && g.nslices == 0);
}

void test_window_rows()
{
	for (size_t esz : { (size_t)8, (size_t)16 }) {
		const int64_t cap = lds_cap_elems(esz);
		CHECK(cap == (esz == 8 ? 19968 : 9984)); // 156 KiB / element size
		CHECK(window_rows_of_block(0, cap) == 0);
		CHECK(window_rows_of_block(1, cap) == 1024); // small blocks grouped: up to ceil(1024 / block) of them
		CHECK(window_rows_of_block(63, cap) == 63 * 17);
		CHECK(window_rows_of_block(511, cap) == 511 * 3);
		CHECK(window_rows_of_block(512, cap) == 512); // one block per window from 512 rows on
		CHECK(window_rows_of_block(cap, cap) == cap);
		CHECK(window_rows_of_block(cap + 1, cap) == 0);
		CHECK(generic_window_rows(cap) == (esz == 8 ? 16384 : 9984));
	}
	CHECK(window_rows_of_block(2, 100) == 100); // the grouping stops at the cap
}

void test_mode_table()
{
	const int cus = 4; // a window pays from 2 * cus = 8 blocks on
	const CsrSwitches none;
	for (int req : { LPP_SPMV_AUTO, LPP_SPMV_ROWGROUP, LPP_SPMV_SLICED, LPP_SPMV_WINDOW })
		for (int cplx = 0; cplx < 2; cplx++)
			for (int fits = 0; fits < 2; fits++)
				for (int known = 0; known < 2; known++)
					for (int enough = 0; enough < 2; enough++)
						for (int share = 0; share < 2; share++) {
							CsrFacts f;
							f.esz = cplx ? 16 : 8;
							f.is_complex = cplx != 0;
							f.num_cus = cus;
							f.has_plain = true;
							f.nnz = 1000;
							f.hint_block = known ? 1000 : 0;
							const int64_t gw = cplx ? 9984 : 16384, w = known ? 1000 : gw;
							f.nrows = enough ? 7 * w + 1 : 7 * w; // 8 blocks / 7 blocks
							f.src_elems = fits ? 0 : (int64_t)(((size_t)1 << 32) / f.esz);
							f.mode = csr_requested_mode(LPP_SPMV_AUTO, none, req);
							f.forced = req != 0;
							CHECK(f.mode == req && f.fits32() == (fits != 0));
							const unsigned long long counted = share ? 350 : 349; // of 1000 entries
							const int64_t cw = csr_count_window(f);
							const bool counts = req == LPP_SPMV_AUTO && !known && !cplx && fits && enough;
							CHECK(cw == (counts ? gw : 0));
							const CsrMode m = csr_mode(f, none, cw, counted);
							int want = req;
							if (req == LPP_SPMV_AUTO) want = ((known && !cplx && enough) || (counts && share)) ? LPP_SPMV_WINDOW : LPP_SPMV_SLICED;
							int64_t rows = known ? 1000 : (want == LPP_SPMV_WINDOW ? gw : 0);
							if (!fits && want != LPP_SPMV_ROWGROUP) want = LPP_SPMV_ROWGROUP;
							CHECK(m.mode == want && m.win_rows == rows);
							CHECK(m.sliced() == (want == LPP_SPMV_SLICED || want == LPP_SPMV_WINDOW) && m.window() == (want == LPP_SPMV_WINDOW));
							if (m.sliced()) CHECK(m.block(f.nrows, 0) == (m.window() ? rows : f.nrows) && m.block(f.nrows, 77) == 77);
						}
	// the requested mode: the caller's, else the switch, else the configuration
	CsrSwitches sw;
	CHECK(csr_requested_mode(2, sw, 0) == 2 && csr_requested_mode(2, sw, 3) == 3);
	sw.spmv_kernel = on(1);
	CHECK(csr_requested_mode(2, sw, 0) == 1 && csr_requested_mode(2, sw, 3) == 3);
	// LPP_WINDOW_ROWS: clamped to [64, cap], ignored when the caller forces a mode
	CsrFacts f;
	f.nrows = 100000, f.nnz = 1000, f.hint_block = 1000, f.num_cus = 4, f.has_plain = true;
	sw = CsrSwitches();
	for (const auto& r : { std::pair<int, int64_t> { 4096, 4096 }, { 1, 64 }, { -5, 64 }, { 1 << 30, 19968 } }) {
		sw.window_rows = on(r.first);
		f.mode = LPP_SPMV_AUTO, f.forced = false;
		CHECK(csr_mode(f, sw, 0, 0).mode == LPP_SPMV_WINDOW && csr_mode(f, sw, 0, 0).win_rows == r.second);
		f.mode = LPP_SPMV_WINDOW, f.forced = true;
		CHECK(csr_mode(f, sw, 0, 0).win_rows == 1000);
	}
	// detection: only for a real matrix nobody described, chosen by itself, whose columns index its own rows
	f = CsrFacts();
	f.nrows = 100000, f.nnz = 1000;
	sw = CsrSwitches();
	CHECK(csr_detection_wanted(f, sw));
	sw.detect_block = on(0);
	CHECK(!csr_detection_wanted(f, sw));
	sw.detect_block = on(1);
	CHECK(csr_detection_wanted(f, sw));
	CsrFacts h = f;
	h.hint_block = 70;
	CHECK(!csr_detection_wanted(h, sw));
	h = f, h.mode = LPP_SPMV_SLICED;
	CHECK(!csr_detection_wanted(h, sw));
	h = f, h.is_complex = true, h.esz = 16;
	CHECK(!csr_detection_wanted(h, sw));
	h = f, h.src_elems = 200000;
	CHECK(!csr_detection_wanted(h, sw));
	h = f, h.nrows = (int64_t)1 << 29; // 4 GiB of doubles
	CHECK(!csr_detection_wanted(h, sw));
	// no count without the plain columns or without entries
	f.num_cus = 1;
	CHECK(csr_count_window(f) == 0);
	f.has_plain = true;
	CHECK(csr_count_window(f) == 16384);
	f.nnz = 0;
	CHECK(csr_count_window(f) == 0);
}

void test_pitch_pad()
{
	CsrSwitches sw;
	// BASELINE config 2: 12870 blocks of 12870 rows (= 6 mod 16), 1.3 GB per vector
	CHECK(pitch_pad(slice_geom((int64_t)12870 * 12870, 12870), 8, true, sw) == 10);
	CHECK(pitch_pad(slice_geom((int64_t)12870 * 12870, 12870), 8, false, sw) == 0); // not eligible
	// 924 rows (= 12 mod 16): by the switch on a small matrix, by itself on a large one
	CHECK(pitch_pad(slice_geom(924 * 792, 924), 8, true, sw) == 0);
	CHECK(pitch_pad(slice_geom((int64_t)924 * 40000, 924), 8, true, sw) == 4);
	sw.pitch_rows = on(1);
	CHECK(pitch_pad(slice_geom(924 * 792, 924), 8, true, sw) == 4);
	CHECK(pitch_pad(slice_geom(924 * 792 - 1, 924), 8, true, sw) == 0); // a partial last block
	CHECK(pitch_pad(slice_geom((int64_t)11440 * 11440, 11440), 8, true, sw) == 0); // 11440 = 16 x 715: lines already
	sw.pitch_rows = on(0);
	CHECK(pitch_pad(slice_geom((int64_t)12870 * 12870, 12870), 8, true, sw) == 0);
	// by itself from 256 MB per vector on: 2^25 doubles
	sw = CsrSwitches();
	CHECK(pitch_pad(slice_geom((int64_t)1000 * 33555, 1000), 8, true, sw) == 8);
	CHECK(pitch_pad(slice_geom((int64_t)1000 * 33554, 1000), 8, true, sw) == 0);
	// the pitched vector stays below 4 GiB (2^29 doubles: 1008 * 532610 < 2^29 <= 1008 * 532611) ...
	CHECK(pitch_pad(slice_geom((int64_t)1000 * 532610, 1000), 8, true, sw) == 8);
	CHECK(pitch_pad(slice_geom((int64_t)1000 * 532611, 1000), 8, true, sw) == 0);
	// ... and below 2^31 positions (which only elements of one byte could reach first: the arithmetic alone)
	CHECK(pitch_pad(slice_geom((int64_t)100 * (((int64_t)1 << 24) - 1), 100), 1, true, sw) == 28);
	CHECK(pitch_pad(slice_geom((int64_t)100 * ((int64_t)1 << 24), 100), 1, true, sw) == 0);
}

void test_split_panel_gate()
{
	CsrSwitches sw;
	CsrFacts f;
	f.hint_block = 11440, f.nrows = (int64_t)11440 * 3000, f.nnz = 1; // 275 MB per vector
	CsrMode win;
	win.mode = LPP_SPMV_WINDOW, win.win_rows = 11440;
	CHECK(split_panel_wanted(f, win, 11440, false, false, sw)); // on by size
	CHECK(!split_panel_wanted(f, win, 11440, true, false, sw)); // shared offsets take the leaving entries their own way
	CHECK(!split_panel_wanted(f, win, 11440, false, true, sw)); // split already
	CHECK(!split_panel_wanted(f, win, 22880, false, false, sw)); // the window is not the basis block
	CsrMode sl = win;
	sl.mode = LPP_SPMV_SLICED;
	CHECK(!split_panel_wanted(f, sl, 11440, false, false, sw));
	CsrFacts h = f;
	h.forced = true;
	CHECK(!split_panel_wanted(h, win, 11440, false, false, sw));
	h = f, h.src_elems = 2 * f.nrows;
	CHECK(!split_panel_wanted(h, win, 11440, false, false, sw));
	h = f, h.is_complex = true, h.esz = 16;
	CHECK(!split_panel_wanted(h, win, 11440, false, false, sw));
	h = f, h.nrows = (int64_t)11440 * 2934; // the first whole number of blocks from 2^25 rows (256 MB of doubles) on
	CHECK(split_panel_wanted(h, win, 11440, false, false, sw));
	h.nrows = (int64_t)11440 * 2933;
	CHECK(!split_panel_wanted(h, win, 11440, false, false, sw));
	// the 256 MB threshold with blocks of 16 rows: 2^25 rows / one block less
	h = f, h.hint_block = 16, h.nrows = (int64_t)1 << 25;
	CHECK(split_panel_wanted(h, win, 16, false, false, sw));
	h.nrows -= 16;
	CHECK(!split_panel_wanted(h, win, 16, false, false, sw));
	// BASELINE config 2: 12870 = 6 mod 16, not taken by itself
	CsrFacts c2 = f;
	c2.hint_block = 12870, c2.nrows = (int64_t)12870 * 12870;
	CHECK(!split_panel_wanted(c2, win, 12870, false, false, sw));
	// LPP_SPLIT_PANEL=1: wherever a basis block is known (complex too); =0: never
	sw.split_panel = on(1);
	CHECK(split_panel_wanted(c2, win, 12870, false, false, sw));
	h = f, h.nrows = 11440 * 64;
	CHECK(split_panel_wanted(h, win, 11440, false, false, sw));
	h.is_complex = true, h.esz = 16;
	CHECK(split_panel_wanted(h, win, 11440, false, false, sw));
	h = f, h.hint_block = 0;
	CHECK(!split_panel_wanted(h, win, 0, false, false, sw));
	CHECK(!split_panel_wanted(f, win, 11440, true, false, sw));
	sw.split_panel = on(0);
	CHECK(!split_panel_wanted(f, win, 11440, false, false, sw));
	// parts
	sw = CsrSwitches();
	CHECK(split_panel_parts(sw, 4) == 1);
	for (const auto& r : { std::pair<int, int> { 3, 3 }, { 0, 1 }, { -2, 1 }, { 9, 4 } }) {
		sw.split_parts = on(r.first);
		CHECK(split_panel_parts(sw, 4) == r.second);
	}
}

void test_form_rules()
{
	CsrSwitches sw;
	const SliceGeom g = slice_geom(924 * 8, 924), one = slice_geom(924, 924), ragged = slice_geom(924 * 8 - 1, 924), wide = slice_geom(1 << 20, 65537);
	CHECK(value_dictionary_wanted(-1, sw) && value_dictionary_wanted(1, sw) && !value_dictionary_wanted(0, sw));
	CHECK(shared_offsets_wanted(false, sw) && !shared_offsets_wanted(true, sw));
	CHECK(diag_codes_wanted(true, true, sw) && !diag_codes_wanted(false, true, sw) && !diag_codes_wanted(true, false, sw));
	CHECK(local16_check_wanted(true, g, 10, sw) && !local16_check_wanted(false, g, 10, sw) && !local16_check_wanted(true, g, 0, sw) && !local16_check_wanted(true, wide, 10, sw));
	CHECK(local16_check_wanted(true, slice_geom(1 << 20, 65536), 10, sw));
	CHECK(outs_first_eligible(true, false, false, g, 10, sw) && !outs_first_eligible(false, false, false, g, 10, sw) && !outs_first_eligible(true, true, false, g, 10, sw)
	      && !outs_first_eligible(true, false, true, g, 10, sw) && !outs_first_eligible(true, false, false, one, 10, sw) && !outs_first_eligible(true, false, false, g, 0, sw));
	CHECK(block_template_check_wanted(true, true, g, sw) && !block_template_check_wanted(false, true, g, sw) && !block_template_check_wanted(true, false, g, sw)
	      && !block_template_check_wanted(true, true, one, sw) && !block_template_check_wanted(true, true, ragged, sw));
	CHECK(template_pack_wanted(2, sw) && !template_pack_wanted(1, sw) && !template_pack_wanted(0, sw));
	CHECK(release_plain_wanted(true, true, sw) && !release_plain_wanted(false, true, sw) && !release_plain_wanted(true, false, sw));
	// every switch override
	sw.compress_values = on(0);
	CHECK(!value_dictionary_wanted(-1, sw));
	sw.compress_values = on(1);
	CHECK(value_dictionary_wanted(0, sw));
	sw.shared_offsets = on(0);
	CHECK(!shared_offsets_wanted(false, sw));
	sw.shared_offsets = on(1);
	CHECK(shared_offsets_wanted(false, sw) && !shared_offsets_wanted(true, sw));
	sw.diag_codes = on(0), sw.local16 = on(0), sw.outs_first = on(0), sw.block_template = on(0), sw.template_pack = on(0);
	CHECK(!diag_codes_wanted(true, true, sw) && !local16_check_wanted(true, g, 10, sw) && !outs_first_eligible(true, false, false, g, 10, sw)
	      && !block_template_check_wanted(true, true, g, sw) && !template_pack_wanted(2, sw));
	sw.diag_codes = on(1), sw.local16 = on(1), sw.outs_first = on(1), sw.block_template = on(1), sw.template_pack = on(1);
	CHECK(diag_codes_wanted(true, true, sw) && local16_check_wanted(true, g, 10, sw) && outs_first_eligible(true, false, false, g, 10, sw)
	      && block_template_check_wanted(true, true, g, sw) && template_pack_wanted(2, sw));
	sw.keep_plain_csr = on(0); // set, whatever its value
	CHECK(!release_plain_wanted(true, true, sw));
}

// H = 1 (x) T + C (x) 1 + D over two species of n states: T a chain inside the block (value t), C a chain between neighbouring blocks (value c)
struct Csr {
	std::vector<int64_t> rp { 0 };
	std::vector<int32_t> ci;
	std::vector<double> va;
};
Csr product_matrix(int n, double t, double c)
{
	Csr A;
	for (int b = 0; b < n; b++)
		for (int l = 0; l < n; l++) {
			const int r = b * n + l;
			auto put = [&](int col, double v) {
				A.ci.push_back(col);
				A.va.push_back(v);
			};
			if (b > 0) put(r - n, c);
			if (l > 0) put(r - 1, t);
			put(r, 0.25 * (double)(r % 7));
			if (l < n - 1) put(r + 1, t);
			if (b < n - 1) put(r + n, c);
			A.rp.push_back((int64_t)A.ci.size());
		}
	return A;
}
int64_t detect(const Csr& A, int64_t cap)
{
	RowBlockDetector det;
	for (int64_t row0 : detect_sample_rows((int64_t)A.rp.size() - 1)) {
		const int64_t p0 = A.rp[(size_t)row0], n = A.rp[(size_t)row0 + 64] - p0;
		if (!detect_sample_usable(n)) continue;
		det.add(row0, &A.rp[(size_t)row0], &A.ci[(size_t)p0], &A.va[(size_t)p0], sizeof(double));
	}
	return det.block(cap);
}
void test_detection()
{
	const int64_t cap = lds_cap_elems(8);
	// the samples: 48 slices spread over the rows, none below 64 slices
	CHECK(detect_sample_rows(64 * 64 - 1).empty() && detect_sample_rows(0).empty());
	const std::vector<int64_t> rows = detect_sample_rows(4900);
	CHECK((int)rows.size() == kDetectSamples && rows.front() == 0 && rows.back() == 75 * 64);
	for (size_t i = 0; i < rows.size(); i++) CHECK(rows[i] % 64 == 0 && rows[i] + 64 <= 4900 && (i == 0 || rows[i] > rows[i - 1]));
	CHECK(!detect_sample_usable(0) && detect_sample_usable(1) && detect_sample_usable(1 << 20) && !detect_sample_usable((1 << 20) + 1));
	// a two-species product of a 70-state species
	Csr A = product_matrix(70, -0.5, -1.0);
	CHECK(A.rp.size() == 4901);
	CHECK(detect(A, cap) == 70);
	CHECK(detect(A, (int64_t)1 << 23) == 70 && detect(A, 70) == 70);
	CHECK(detect(A, 69) == 0); // a block above the cap
	// One coupling value changed in one sampled row: that slice no longer shares the shift with one value and names no block; the
	// other samples still do, and the structure is that of 70-row blocks everywhere -- the detector looks at values only to find the
	// shift, so the answer stays 70 (the product-basis builder behind it verifies the matrix row by row and refuses this one).
	Csr V = A;
	const int64_t row = rows[10] + 5;
	for (int64_t p = V.rp[(size_t)row]; p < V.rp[(size_t)row + 1]; p++)
		if (std::llabs((int64_t)V.ci[(size_t)p] - row) == 70) V.va[(size_t)p] = -1.5;
	CHECK(detect(V, cap) == 70);
	// ... changed in a row of every sampled slice: no slice shares a shift, no block
	V = A;
	for (int64_t r0 : rows)
		for (int64_t p = V.rp[(size_t)r0 + 5]; p < V.rp[(size_t)r0 + 6]; p++)
			if (std::llabs((int64_t)V.ci[(size_t)p] - (r0 + 5)) == 70) V.va[(size_t)p] = -1.5;
	CHECK(detect(V, cap) == 0);
	// a coupling that is not a whole number of blocks away, in one sampled row: refused by the structure check
	V = A;
	{
		const int64_t p = V.rp[(size_t)rows[20] + 7];
		V.ci[(size_t)p] = V.ci[(size_t)p] == 0 ? 1 : V.ci[(size_t)p] - 1; // the row's first entry, one column to the left
	}
	CHECK(detect(V, cap) == 0);
	// a banded matrix: no shared far offset
	Csr T3;
	for (int r = 0; r < 4900; r++) {
		for (int c = r - 1; c <= r + 1; c++)
			if (c >= 0 && c < 4900) {
				T3.ci.push_back(c);
				T3.va.push_back(c == r ? 2.0 : -1.0);
			}
		T3.rp.push_back((int64_t)T3.ci.size());
	}
	CHECK(detect(T3, cap) == 0);
	// no samples at all
	CHECK(RowBlockDetector().block(cap) == 0);
	// complex elements: the value comparison covers both halves
	std::vector<double> cv(A.va.size() * 2, 0.0);
	for (size_t i = 0; i < A.va.size(); i++) cv[2 * i] = A.va[i], cv[2 * i + 1] = 0.125;
	RowBlockDetector dc, dbad;
	for (int64_t row0 : rows) {
		const int64_t p0 = A.rp[(size_t)row0];
		dc.add(row0, &A.rp[(size_t)row0], &A.ci[(size_t)p0], &cv[2 * (size_t)p0], 16);
	}
	CHECK(dc.block(lds_cap_elems(16)) == 70);
	for (size_t i = 0; i < A.va.size(); i++) cv[2 * i + 1] = 0.001 * (double)i; // every imaginary part differs
	for (int64_t row0 : rows) {
		const int64_t p0 = A.rp[(size_t)row0];
		dbad.add(row0, &A.rp[(size_t)row0], &A.ci[(size_t)p0], &cv[2 * (size_t)p0], 16);
	}
	CHECK(dbad.block(lds_cap_elems(16)) == 0);
}

void test_sizes()
{
	// 8 blocks of 924 rows: 15 slices per block, 120 in all; 40000 per-row entries (5000 per block); 3000 code words, 400 of them block 0's
	const SliceGeom g = slice_geom(924 * 8, 924);
	CHECK(g.spb == 15 && g.nslices == 120);
	for (size_t esz : { (size_t)8, (size_t)16 })
		for (int l16 = 0; l16 < 2; l16++)
			for (int coded = 0; coded < 2; coded++)
				for (int tmpl = 0; tmpl < 3; tmpl++)
					for (int stride : { 0, 8 })
						for (int split = 0; split < 2; split++)
							for (int dcode = 0; dcode < 2; dcode++) {
								if (tmpl && !(l16 && coded)) continue; // a template needs 16-bit columns and codes
								if (stride && !split) continue;
								SlicedShape s;
								s.g = g, s.esz = esz, s.entries = 40000, s.local16 = l16, s.coded = coded, s.code_words = tmpl == 2 ? 400 : 3000, s.tmpl = tmpl;
								s.split = split, s.dia_stride = stride, s.dcode = dcode;
								const SlicedSizes z = sliced_sizes(s);
								// DevCsr's arrays, from its comments:
								const size_t slices = tmpl ? 15 : 120, rows = tmpl ? 924 : 7392, nz = tmpl ? 5000 : 40000; // tmpl: slice_ptr / row_len / scol describe block 0 only
								CHECK(z.slice_ptr == 8 * (slices + 1)); // int64 per slice + the end
								CHECK(z.row_len == 4 * rows);
								CHECK(z.scol == (l16 ? 2u : 4u) * (nz + 64)); // 16-bit window-local or 32-bit columns, 64 entries of slack
								CHECK(z.sval == (coded ? 0 : esz * (40000 + 64))); // coded layout: sval == nullptr
								CHECK(z.code_ptr == (coded ? 8 * ((tmpl == 2 ? 15u : 120u) + 1) : 0)); // tmpl 2: codes / code_ptr describe block 0 too
								CHECK(z.codes == (coded ? 4 * ((size_t)(tmpl == 2 ? 400 : 3000) + 64 * 16) : 0)); // 32-bit words + slack
								CHECK(z.dict == (coded ? 256u * 8u : 0u));
								CHECK(z.rrowptr == (split ? 8u * 7393u : 0u)); // row pointers of the rest CSR
								CHECK(z.dia_off == (size_t)(split ? 4 * 120 * stride : 0) && z.dia_val == (split ? esz * 120 * (size_t)stride : 0)); // places per slice
								CHECK(z.dcode == (dcode ? 7392 * (esz / 8) : 0)); // one code per real component and row
								// what lpp_layout reports: everything but the code words' slack; a product does not read the rest CSR's row pointers
								const size_t all = z.slice_ptr + z.row_len + z.scol + z.sval + z.code_ptr + z.codes + z.dict + z.rrowptr + z.dia_off + z.dia_val + z.dcode;
								const size_t slack = coded ? 4 * 64 * 16 : 0;
								CHECK(z.resident_bytes() == all - slack && z.stream_bytes() == all - slack - z.rrowptr);
								CHECK(z.structure() == z.slice_ptr + z.row_len + z.scol && z.values() == z.sval + z.code_ptr + z.codes + z.dict - slack);
							}
}

void test_dictionary()
{
	auto key = [](double v) {
		unsigned long long k;
		std::memcpy(&k, &v, 8);
		return k;
	};
	std::vector<double> dict;
	// one key: code 0 = +0.0 is added, the tail repeats the last key
	CHECK(dict256_from_keys({ key(1.5) }, dict) == 2 && dict.size() == 256 && key(dict[0]) == 0 && dict[1] == 1.5 && dict[255] == 1.5);
	// -0.0 and +0.0 are different keys; repeats are dropped; ascending by bit pattern (negative doubles last)
	CHECK(dict256_from_keys({ key(-0.0), key(0.0), key(2.0), key(-1.0), key(2.0), key(0.5) }, dict) == 5);
	CHECK(key(dict[0]) == 0 && dict[1] == 0.5 && dict[2] == 2.0 && key(dict[3]) == key(-0.0) && dict[4] == -1.0 && dict[255] == -1.0);
	CHECK(dict256_from_keys({}, dict) == 1 && key(dict[0]) == 0 && key(dict[255]) == 0);
	for (int n : { 255, 256, 257 }) {
		std::vector<unsigned long long> keys; // n distinct keys, +0.0 among them
		for (int i = 0; i < n; i++) keys.push_back(key((double)i));
		std::vector<double> d(3, 7.0);
		const int nd = dict256_from_keys(keys, d);
		if (n > 256) {
			CHECK(nd == 0 && d.size() == 3 && d[0] == 7.0); // more than 256: not coded, dict left alone
			continue;
		}
		CHECK(nd == n && d.size() == 256);
		for (int i = 0; i < 256; i++) CHECK(d[(size_t)i] == (double)std::min(i, n - 1));
	}
	{
		std::vector<unsigned long long> keys; // 256 distinct keys without +0.0: 257 with it
		for (int i = 1; i <= 256; i++) keys.push_back(key((double)i));
		CHECK(dict256_from_keys(keys, dict) == 0);
	}
}

void test_switches_from_env()
{
	for (const char* k : { "LPP_SPMV_G", "LPP_SPMV_KERNEL", "LPP_COMPRESS_VALUES", "LPP_SHARED_OFFSETS", "LPP_DIAG_CODES", "LPP_LOCAL16", "LPP_OUTS_FIRST", "LPP_PITCH_ROWS",
	                       "LPP_BLOCK_TEMPLATE", "LPP_TEMPLATE_PACK", "LPP_SPLIT_PARTS", "LPP_SPLIT_PANEL", "LPP_DETECT_BLOCK", "LPP_WINDOW_ROWS", "LPP_KEEP_PLAIN_CSR", "LPP_VERBOSE" })
		unsetenv(k);
	CsrSwitches sw = csr_switches_from_env();
	EnvSwitch CsrSwitches::*all[] = { &CsrSwitches::spmv_g, &CsrSwitches::spmv_kernel, &CsrSwitches::compress_values, &CsrSwitches::shared_offsets, &CsrSwitches::diag_codes,
		                              &CsrSwitches::local16, &CsrSwitches::outs_first, &CsrSwitches::pitch_rows, &CsrSwitches::block_template, &CsrSwitches::template_pack,
		                              &CsrSwitches::split_parts, &CsrSwitches::split_panel, &CsrSwitches::detect_block, &CsrSwitches::window_rows, &CsrSwitches::keep_plain_csr };
	for (auto m : all) CHECK(!(sw.*m).set && !(sw.*m).off() && (sw.*m).value_or(7) == 7);
	CHECK(!sw.verbose);
	setenv("LPP_WINDOW_ROWS", "4096", 1);
	setenv("LPP_LOCAL16", "0", 1);
	setenv("LPP_KEEP_PLAIN_CSR", "", 1);
	setenv("LPP_VERBOSE", "1", 1);
	sw = csr_switches_from_env(); // read again at every call
	CHECK(sw.window_rows.set && sw.window_rows.v == 4096 && sw.local16.off() && sw.keep_plain_csr.set && sw.keep_plain_csr.v == 0 && sw.verbose && !sw.spmv_g.set);
	unsetenv("LPP_LOCAL16");
	CHECK(!csr_switches_from_env().local16.set);
}

} // namespace

int main()
{
	test_pick_group();
	test_geometry();
	test_window_rows();
	test_mode_table();
	test_pitch_pad();
	test_split_panel_gate();
	test_form_rules();
	test_detection();
	test_sizes();
	test_dictionary();
	test_switches_from_env();
	printf("ok\n");
	return 0;
}
