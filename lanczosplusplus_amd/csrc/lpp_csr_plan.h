// lpp_csr_plan.h -- the decisions of the general CSR layout (sliced / LDS-window kernels, lpp_spmv_kernels.h) in plain C++: the LPP_*
// switches of its build as values, the geometry, the kernel mode, every "is this form taken" rule, the basis-block detection over sampled
// slices, the byte size of every array and the 256-entry value dictionary.  lpp_csr_layout.hip runs the device work between these decisions.
// No HIP, and no environment outside csr_switches_from_env: lanczosplusplus_amd/host/test_csr_plan.cpp runs it under the sanitizers
// without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "lpp_engine.h"
#include "lpp_switch.h"

namespace lpp {

// ---- switches -------------------------------------------------------------------------------------------------------------------------
struct CsrSwitches { // LPP_<NAME>
	EnvSwitch spmv_g, spmv_kernel, compress_values, shared_offsets, diag_codes, local16, outs_first, pitch_rows, block_template, template_pack, split_parts,
	    split_panel, detect_block, window_rows, keep_plain_csr;
	bool verbose = false; // LPP_VERBOSE
};
// The only getenv of the general layout's build.  Called once per top-level build (finalize_csr, try_product_layout, layout_gate) and the
// result passed down; never kept across builds: a process may change its environment between two engines.
inline CsrSwitches csr_switches_from_env()
{
	CsrSwitches sw;
	sw.spmv_g = env_switch("LPP_SPMV_G"), sw.spmv_kernel = env_switch("LPP_SPMV_KERNEL"), sw.compress_values = env_switch("LPP_COMPRESS_VALUES");
	sw.shared_offsets = env_switch("LPP_SHARED_OFFSETS"), sw.diag_codes = env_switch("LPP_DIAG_CODES"), sw.local16 = env_switch("LPP_LOCAL16");
	sw.outs_first = env_switch("LPP_OUTS_FIRST"), sw.pitch_rows = env_switch("LPP_PITCH_ROWS"), sw.block_template = env_switch("LPP_BLOCK_TEMPLATE");
	sw.template_pack = env_switch("LPP_TEMPLATE_PACK"), sw.split_parts = env_switch("LPP_SPLIT_PARTS"), sw.split_panel = env_switch("LPP_SPLIT_PANEL");
	sw.detect_block = env_switch("LPP_DETECT_BLOCK"), sw.window_rows = env_switch("LPP_WINDOW_ROWS"), sw.keep_plain_csr = env_switch("LPP_KEEP_PLAIN_CSR");
	sw.verbose = env_switch("LPP_VERBOSE").set;
	return sw;
}

// ---- geometry -------------------------------------------------------------------------------------------------------------------------
// rows in row blocks of B rows, every block in slices of 64 rows (lpp_spmv_kernels.h)
struct SliceGeom {
	int64_t nrows;
	int64_t B; // rows per block
	int32_t spb; // slices per block = ceil(B/64)
	int64_t nblocks;
	int64_t nslices; // nblocks * spb
};
inline SliceGeom slice_geom(int64_t nrows, int64_t B)
{
	SliceGeom g;
	g.nrows = nrows;
	g.B = std::max<int64_t>(1, std::min<int64_t>(B, std::max<int64_t>(nrows, 1)));
	g.spb = (int32_t)((g.B + 63) / 64);
	g.nblocks = (nrows + g.B - 1) / g.B;
	g.nslices = g.nblocks * g.spb;
	return g;
}

// lanes per row of the row-group kernel: LPP_SPMV_G when it names one, otherwise the largest power of two <= avg/2, in [4,64]
inline int pick_group(int64_t nrows, int64_t nnz, const EnvSwitch& spmv_g)
{
	if (spmv_g.set) {
		const int g = spmv_g.v;
		if (g == 4 || g == 8 || g == 16 || g == 32 || g == 64) return g;
	}
	const double avg = nrows > 0 ? (double)nnz / (double)nrows : 1.0;
	int g = 4;
	while (g < 64 && g * 2 <= avg / 2.0 + 1e-9) g *= 2;
	return g;
}

// elements of the source vector one LDS window holds (<= 156 KB of the CU's 160 KB)
inline int64_t lds_cap_elems(size_t esz) { return (int64_t)((156 * 1024) / esz); }
// the generic diagonal window of a matrix without a natural block
inline int64_t generic_window_rows(int64_t cap) { return std::min<int64_t>(cap, 16384); }

// Window rows from the basis' natural block (N_up for the Hubbard product basis): one basis block per window whenever it gives the 16 waves
// of a workgroup something to do: only then do all row blocks repeat the same in-block structure (block template); tiny basis blocks are
// grouped.  0: no block, or one beyond the window.
inline int64_t window_rows_of_block(int64_t hint_block, int64_t cap)
{
	if (hint_block <= 0 || hint_block > cap) return 0;
	const int64_t k = hint_block >= 512 ? 1 : std::max<int64_t>(1, std::min<int64_t>(cap / hint_block, (1024 + hint_block - 1) / hint_block));
	return hint_block * k;
}

// ---- the kernel mode ------------------------------------------------------------------------------------------------------------------
// what finalize_csr knows about the matrix before any device work
struct CsrFacts {
	int64_t nrows = 0, nnz = 0;
	int64_t src_elems = 0; // length of the vector the columns index (0 = nrows)
	int64_t hint_block = 0; // the basis' natural block, 0 = unknown
	bool has_plain = false; // the plain column array is resident
	bool is_complex = false;
	size_t esz = 8;
	int num_cus = 256;
	int mode = LPP_SPMV_AUTO; // the request: csr_requested_mode
	bool forced = false; // ... came from the caller (force_mode), not from the configuration
	int64_t cap() const { return lds_cap_elems(esz); }
	// the sliced kernels address the source vector with 32-bit byte offsets
	bool fits32() const { return (size_t)std::max<int64_t>(src_elems, nrows) * esz < ((size_t)1 << 32); }
};
// the caller's mode, else LPP_SPMV_KERNEL, else the configuration's
inline int csr_requested_mode(int cfg_kernel, const CsrSwitches& sw, int force_mode) { return force_mode ? force_mode : sw.spmv_kernel.value_or(cfg_kernel); }

// a matrix nobody described is searched for a basis block (detect_row_block)
inline bool csr_detection_wanted(const CsrFacts& f, const CsrSwitches& sw)
{
	return f.hint_block == 0 && f.mode == LPP_SPMV_AUTO && !f.is_complex && f.fits32() && f.src_elems == 0 && !sw.detect_block.off();
}

// The mode is decided in two steps because a device count sits in the middle.  Step 1: is a locality count needed, and over which window
// (0: none).  No natural block: a plain diagonal window of 16384 rows pays when enough gathers land inside it (bases in ascending word
// order couple mostly nearby ranks: Heisenberg L=28 0.95 vs 1.22 ms); measured on the matrix itself (k_count_local).
inline int64_t csr_count_window(const CsrFacts& f)
{
	if (f.mode != LPP_SPMV_AUTO || window_rows_of_block(f.hint_block, f.cap()) != 0) return 0;
	if (f.is_complex || !f.fits32() || !f.has_plain || f.nnz <= 0) return 0;
	const int64_t gw = generic_window_rows(f.cap());
	return (f.nrows + gw - 1) / gw >= 2 * (int64_t)f.num_cus ? gw : 0;
}
struct CsrMode {
	int mode = LPP_SPMV_ROWGROUP;
	int64_t win_rows = 0;
	bool sliced() const { return mode == LPP_SPMV_SLICED || mode == LPP_SPMV_WINDOW; }
	bool window() const { return mode == LPP_SPMV_WINDOW; }
	// rows per block of the sliced layout: the caller's, the window, or one block of all rows
	int64_t block(int64_t nrows, int64_t force_block) const { return force_block > 0 ? force_block : (window() ? win_rows : nrows); }
};
// Step 2: the mode, given the entries counted inside the window of step 1 (`counted`; unused when count_window == 0).
// The LDS window pays when in-block gathers dominate (Hubbard up-hops), the matrix is large enough to give every CU several blocks, and a
// window element is 8 bytes (measured: complex t-J windows lose).  With the block template and 16-bit local columns it also wins when the
// whole vector fits the Infinity Cache (Hubbard chains L=12: 31.6 vs 33.1 us, L=14: 0.306 vs 0.372 ms).
inline CsrMode csr_mode(const CsrFacts& f, const CsrSwitches& sw, int64_t count_window, unsigned long long counted)
{
	CsrMode m;
	m.mode = f.mode;
	m.win_rows = window_rows_of_block(f.hint_block, f.cap());
	if (m.mode == LPP_SPMV_AUTO) {
		bool window_ok = m.win_rows > 0 && !f.is_complex && (f.nrows + m.win_rows - 1) / m.win_rows >= 2 * (int64_t)f.num_cus;
		if (count_window > 0 && (double)counted >= 0.35 * (double)f.nnz) {
			window_ok = true;
			m.win_rows = count_window;
		}
		m.mode = window_ok ? LPP_SPMV_WINDOW : LPP_SPMV_SLICED;
	}
	// no natural block: a generic diagonal window (captures near-diagonal columns)
	if (m.mode == LPP_SPMV_WINDOW && m.win_rows == 0) m.win_rows = generic_window_rows(f.cap());
	// (LPP_WINDOW_ROWS is ignored when the caller forces a mode)
	if (!f.forced && sw.window_rows.set) m.win_rows = std::max<int64_t>(64, std::min<int64_t>(sw.window_rows.v, f.cap()));
	if (!f.fits32() && (m.mode == LPP_SPMV_AUTO || m.sliced())) m.mode = LPP_SPMV_ROWGROUP;
	return m;
}

// ---- which forms are taken ------------------------------------------------------------------------------------------------------------
inline bool value_dictionary_wanted(int cfg_compress_values, const CsrSwitches& sw) { return sw.compress_values.value_or(cfg_compress_values) != 0; }
// the shared-offset split (k_dia_split); no_dia: the matrix is an out part of the split-panel layout
inline bool shared_offsets_wanted(bool no_dia, const CsrSwitches& sw) { return !no_dia && sw.shared_offsets.value_or(1) != 0; }
// the diagonal as dictionary codes apart from the per-row entries (needs the value dictionary)
inline bool diag_codes_wanted(bool for_window, bool coded, const CsrSwitches& sw) { return for_window && coded && !sw.diag_codes.off(); }
// window kernel: 16-bit window-local columns are worth a check (k_cols_local) of whether every per-row entry stays inside its row block
inline bool local16_check_wanted(bool for_window, const SliceGeom& g, int64_t entries, const CsrSwitches& sw)
{
	return for_window && g.B <= 65536 && entries > 0 && !sw.local16.off();
}
// Plain values, window kernel, no shared-offset split: the entries that leave a row's block go into the row's first slots, so that every
// 512-byte run of the source vector is gathered by one load (k_slice_fill).  Eligibility before the check that rows are sorted by column.
inline bool outs_first_eligible(bool for_window, bool local16, bool split_taken, const SliceGeom& g, int64_t entries, const CsrSwitches& sw)
{
	return for_window && !local16 && !split_taken && g.nblocks >= 2 && entries > 0 && !sw.outs_first.off();
}
// ... and the vectors pitched to 128-byte lines per row block (whole matrix on one GPU, real, blocks not line-aligned by themselves, from
// 256 MB per vector on): the runs gathered from other blocks then start on a line -- 4 lines per run instead of 4.9 at config 2
// (N_up = 12870 = 6 mod 16).  LPP_PITCH_ROWS=0/1: never / wherever it applies.
// eligible: outs-first taken, the engine's own whole real matrix (no communicator, no out parts, columns index its own rows).
// Returns the elements added to every row block (0: not pitched).
inline int pitch_pad(const SliceGeom& g, size_t esz, bool eligible, const CsrSwitches& sw)
{
	const int64_t line = 128 / (int64_t)esz;
	const bool want = sw.pitch_rows.set ? sw.pitch_rows.v != 0 : (size_t)g.nrows * esz >= ((size_t)256 << 20);
	const int64_t pitched = (g.B + line - 1) / line * line;
	if (eligible && want && g.nrows == g.nblocks * g.B && g.B % line != 0 && pitched * g.nblocks < ((int64_t)1 << 31)
	    && (size_t)(pitched * g.nblocks) * esz < ((size_t)1 << 32))
		return (int)(pitched - g.B);
	return 0;
}
// Block-periodic structure: when every row block repeats block 0's row lengths and local columns (the in-block part of a product basis
// is the same one-species matrix in every block) only block 0's copy is kept; it stays in L2 instead of streaming 2 bytes per entry + 4
// per row from HBM.  Values (codes) remain per block.  Worth a check (k_tmpl_check) when:
inline bool block_template_check_wanted(bool local16, bool coded, const SliceGeom& g, const CsrSwitches& sw)
{
	return local16 && coded && g.nblocks >= 2 && g.nrows == g.nblocks * g.B && !sw.block_template.off();
}
// packed padded copy of a level-2 template for the inner loop (the compact copy stays for get_csr)
inline bool template_pack_wanted(int tmpl, const CsrSwitches& sw) { return tmpl == 2 && !sw.template_pack.off(); }
// the sliced copy is the resident one; release the plain arrays (frees ~12 B/nnz)
inline bool release_plain_wanted(bool allow_drop_plain, bool owned, const CsrSwitches& sw) { return allow_drop_plain && !sw.keep_plain_csr.set && owned; }

// Split-panel layout (split_panel_t): plain-format matrix with a basis block, the entries that leave the row blocks go panel-major.
// Taken by itself where a panel of 16 positions is ONE 128-byte line of every source block -- basis blocks of a multiple of 16
// rows (vectors are not pitched in the general layout) -- from 256 MB per vector on.  Measured on the 4x4 cluster with
// 7 + 7 electrons (N_up = 11440 = 16 x 715, 1.3e8 rows, 58.6 GB algorithmic): 6.2 + 7.0 = 13.2 ms and 72 GB of fabric reads in two
// launches against 13.9 ms / 85.6 GB in one kernel (4.45 against 4.2 TB/s algorithmic = 0.56 of 8 TB/s; both launches stream at
// 5.2-5.75 TB/s: the 12-byte format's ceiling on this matrix).  At BASELINE config 2 (N_up = 12870 = 6 mod 16: two lines per
// source block and panel, which no longer fit the L2 beside the entry streams) it loses, 8.1 + 9.9 ms against 18.3-18.7 ms in
// one kernel, and is not taken.  LPP_SPLIT_PANEL=0 / 1: never / wherever a basis block is known.
// (real matrices only: 16 complex positions are two lines, and no complex shape has been measured)
// B: the rows per block chosen; has_out_part: the matrix is split already
inline bool split_panel_wanted(const CsrFacts& f, const CsrMode& m, int64_t B, bool want_dia, bool has_out_part, const CsrSwitches& sw)
{
	const bool off = sw.split_panel.set ? sw.split_panel.v == 0 : (f.is_complex || (f.hint_block & 15) != 0 || (size_t)f.nrows * f.esz < ((size_t)256 << 20));
	return m.window() && !f.forced && !want_dia && !off && f.hint_block > 0 && B == f.hint_block && !has_out_part && f.src_elems == 0;
}
// Parts of the leaving entries by source block range.
// measured: parts do not raise the L2 hit rate here (2 parts: 6.0 + 6.2 ms and 32 + 34 GB against 9.9 ms and 61 GB in one)
inline int split_panel_parts(const CsrSwitches& sw, int max_parts) { return sw.split_parts.set ? std::max(1, std::min(sw.split_parts.v, max_parts)) : 1; }

// ---- basis-block detection ------------------------------------------------------------------------------------------------------------
// Basis block of an uploaded matrix nobody described (lpp_engine_set_row_block not called): product bases show up as couplings at offsets
// k*B that are identical for 64 consecutive rows.  A sample of 64-row slices is looked at; per slice the largest offset shared by all its
// rows (same value in every row) is a block shift, B = the gcd of those over the sample.  Accepted only when every sampled entry is then
// either inside its row's block or a whole number of blocks away, and B is at most the caller's cap.
constexpr int kDetectSamples = 48;
// first rows of the sampled slices; none for fewer than 64 slices
inline std::vector<int64_t> detect_sample_rows(int64_t nrows)
{
	std::vector<int64_t> rows;
	const int64_t nsl = nrows / 64;
	if (nsl < 64) return rows;
	for (int sidx = 0; sidx < kDetectSamples; sidx++) rows.push_back(((nsl * (2 * sidx + 1)) / (2 * kDetectSamples)) * 64);
	return rows;
}
// entries of a sampled slice worth looking at (others are skipped, not refused)
inline bool detect_sample_usable(int64_t entries) { return entries > 0 && entries <= (int64_t)1 << 20; }
class RowBlockDetector {
	struct Slice {
		int64_t row0;
		std::vector<int64_t> rp;
		std::vector<int32_t> ci;
	};
	std::vector<Slice> kept;
	int64_t G = 0;

public:
	// one sampled slice: rows row0 .. row0+63, rp[0..64] as in the matrix, ci / va its rp[64] - rp[0] entries (elements of esz bytes)
	void add(int64_t row0, const int64_t* rp, const int32_t* ci, const void* va, size_t esz)
	{
		const int64_t p0 = rp[0], n = rp[64] - rp[0];
		const char* v = (const char*)va;
		int64_t best = 0; // largest |offset| shared by all 64 rows with the same value
		for (int64_t q = rp[0]; q < rp[1]; q++) {
			const int64_t off = (int64_t)ci[(size_t)(q - p0)] - row0;
			if (std::llabs(off) < 64 || std::llabs(off) <= best) continue;
			bool all = true;
			for (int r = 1; r < 64 && all; r++) {
				bool found = false;
				for (int64_t t = rp[r]; t < rp[r + 1]; t++)
					if ((int64_t)ci[(size_t)(t - p0)] - (row0 + r) == off) {
						found = std::memcmp(v + (size_t)(t - p0) * esz, v + (size_t)(q - p0) * esz, esz) == 0;
						break;
					}
				all = found;
			}
			if (all) best = std::llabs(off);
		}
		if (best > 0) G = G == 0 ? best : std::gcd(G, best);
		Slice sl;
		sl.row0 = row0;
		sl.rp.assign(rp, rp + 65);
		sl.ci.assign(ci, ci + n);
		kept.push_back(std::move(sl));
	}
	// the block, or 0 when no such structure is found
	int64_t block(int64_t cap_elems) const
	{
		if (G < 64 || G > cap_elems || kept.empty()) return 0;
		for (const Slice& sl : kept) {
			const int64_t p0 = sl.rp[0];
			for (int r = 0; r < 64; r++) {
				const int64_t row = sl.row0 + r, b0 = (row / G) * G;
				for (int64_t t = sl.rp[r]; t < sl.rp[r + 1]; t++) {
					const int64_t c = sl.ci[(size_t)(t - p0)];
					if (!((c >= b0 && c < b0 + G) || (c - row) % G == 0)) return 0;
				}
			}
		}
		return G;
	}
};

// ---- array sizes ----------------------------------------------------------------------------------------------------------------------
// what the sizes of the sliced layout's arrays depend on
struct SlicedShape {
	SliceGeom g {};
	size_t esz = 8;
	int64_t entries = 0; // per-row entries of the whole matrix (the rest CSR when shared offsets were split off)
	bool local16 = false, coded = false;
	int64_t code_words = 0; // 32-bit code words held (block 0's at template level 2)
	int tmpl = 0; // block template level: 1 = structure of block 0 only, 2 = code words too
	bool split = false; // shared-offset split taken (rest CSR + per-slice lists)
	int dia_stride = 0; // places per slice in the lists
	bool dcode = false; // diagonal codes
};
constexpr size_t kSliceSlack = 64; // entries: the pipelined kernel reads (and discards) the entry after a slice's last one
constexpr size_t kCodeSlack = 64 * 16; // code words, for the same reason
// bytes of every array of DevCsr's sliced layout, as allocated (0: not held)
struct SlicedSizes {
	size_t slice_ptr = 0, row_len = 0, scol = 0; // structure (block 0 only under a template)
	size_t sval = 0; // plain values ...
	size_t code_ptr = 0, codes = 0, dict = 0; // ... or the value dictionary's
	size_t rrowptr = 0, dia_off = 0, dia_val = 0; // shared-offset split
	size_t dcode = 0;
	size_t structure() const { return slice_ptr + row_len + scol; }
	// lpp_layout's figures have never counted the slack of the code words (nor the packed template copy, whose size only k_tmpl_pack knows)
	size_t values() const { return codes ? code_ptr + dict + codes - sizeof(uint32_t) * kCodeSlack : sval; }
	// what one product must read (a template is counted once: it stays in L2 after the first block); the rest CSR's row pointers are not read
	size_t stream_bytes() const { return structure() + values() + dia_off + dia_val + dcode; }
	size_t resident_bytes() const { return stream_bytes() + rrowptr; }
};
inline SlicedSizes sliced_sizes(const SlicedShape& s)
{
	SlicedSizes z;
	const size_t struct_slices = s.tmpl ? (size_t)s.g.spb : (size_t)s.g.nslices; // block-periodic: block 0 only
	const size_t struct_rows = s.tmpl ? (size_t)s.g.B : (size_t)s.g.nrows;
	const size_t struct_nz = s.tmpl ? (size_t)s.entries / (size_t)s.g.nblocks : (size_t)s.entries;
	z.slice_ptr = sizeof(int64_t) * (struct_slices + 1);
	z.row_len = sizeof(int32_t) * struct_rows;
	z.scol = (s.local16 ? sizeof(uint16_t) : sizeof(int32_t)) * (struct_nz + kSliceSlack);
	if (s.coded) {
		z.code_ptr = sizeof(int64_t) * ((s.tmpl == 2 ? (size_t)s.g.spb : (size_t)s.g.nslices) + 1);
		z.codes = sizeof(uint32_t) * ((size_t)s.code_words + kCodeSlack);
		z.dict = 256 * sizeof(double);
	} else {
		z.sval = s.esz * ((size_t)s.entries + kSliceSlack);
	}
	if (s.split) {
		const size_t places = (size_t)s.g.nslices * (size_t)s.dia_stride;
		z.rrowptr = sizeof(int64_t) * (size_t)(s.g.nrows + 1);
		z.dia_off = sizeof(int32_t) * places;
		z.dia_val = s.esz * places;
	}
	if (s.dcode) z.dcode = (size_t)s.g.nrows * (s.esz / 8);
	return z;
}

// ---- the value dictionary -------------------------------------------------------------------------------------------------------------
// Distinct 64-bit patterns of doubles -> the 256-entry dictionary the coded layouts read: keys ascending by bit pattern, code 0 = +0.0
// (padded / inactive slots decode to an exact zero; added when `keys` lacks it, repeats in `keys` are dropped), the tail padded with the
// last key.  Returns the number of codes in use, or 0 when there are more than 256 (dict is then left alone).
inline int dict256_from_keys(std::vector<unsigned long long> keys, std::vector<double>& dict)
{
	keys.push_back(0ull);
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	if (keys.size() > 256) return 0;
	dict.resize(256);
	for (size_t i = 0; i < 256; i++) std::memcpy(&dict[i], &keys[std::min(i, keys.size() - 1)], sizeof(double));
	return (int)keys.size();
}

} // namespace lpp
