// lpp_csr_layout.hip -- the device side of the general CSR layout's build (kernels: lpp_layout_kernels.h, lpp_spmv_kernels.h): the value
// dictionary, the shared-offset split, the sliced arrays, the block template, the split-panel layout, and rebuild_csr, which undoes all of
// it for lpp_engine_get_csr.  What is built is decided in plain C++ (lpp_csr_plan.h; the switches are read there, once per build, by
// csr_switches_from_env); the functions here run the device work between those decisions.  Every temporary device allocation is held by a
// DevBuf or a DevFlags until its pointer is handed to the DevCsr: no early return leaks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lpp_assemble_kernels.h"
#include "lpp_engine_impl.h"

using namespace lpp;

namespace lpp {

void free_csr(DevCsr& A)
{
	if (A.owned) {
		if (A.rowptr) (void)hipFree(A.rowptr);
		if (A.col) (void)hipFree(A.col);
		if (A.val) (void)hipFree(A.val);
	}
	if (A.slice_ptr) (void)hipFree(A.slice_ptr);
	if (A.row_len) (void)hipFree(A.row_len);
	if (A.scol) (void)hipFree(A.scol);
	if (A.sval) (void)hipFree(A.sval);
	if (A.codes) (void)hipFree(A.codes);
	if (A.code_ptr) (void)hipFree(A.code_ptr);
	if (A.dict) (void)hipFree(A.dict);
	if (A.rrowptr) (void)hipFree(A.rrowptr);
	if (A.dia_off) (void)hipFree(A.dia_off);
	if (A.dia_val) (void)hipFree(A.dia_val);
	if (A.dcode) (void)hipFree(A.dcode);
	if (A.tw) (void)hipFree(A.tw);
	if (A.tw_off) (void)hipFree(A.tw_off);
	if (A.tw_len) (void)hipFree(A.tw_len);
	if (A.out_part) {
		for (int q = 0; q < A.split_parts; q++) free_csr(A.out_part[q]);
		delete[] A.out_part;
	}
	if (A.out_rowmap) (void)hipFree(A.out_rowmap);
	A = DevCsr();
}

SlicedShape sliced_shape(const DevCsr& A, size_t esz)
{
	SlicedShape s;
	s.g = A.geom;
	s.esz = esz;
	s.entries = A.rrowptr ? A.rnnz : A.nnz;
	s.local16 = A.local16;
	s.coded = A.coded;
	s.code_words = A.code_words;
	s.tmpl = A.tmpl;
	s.split = A.rrowptr != nullptr;
	s.dia_stride = A.dia_stride;
	s.dcode = A.dcode != nullptr;
	return s;
}

namespace {

// N zeroed device words for a checking kernel to raise, and their host copy after one stream synchronisation
template <typename W, int N> struct DevFlags {
	DevBuf buf;
	hipStream_t st = nullptr;
	hipError_t init(hipStream_t stream)
	{
		st = stream;
		const hipError_t err = buf.alloc(sizeof(W) * N);
		return err != hipSuccess ? err : hipMemsetAsync(buf.p, 0, sizeof(W) * N, st);
	}
	W* dev() const { return (W*)buf.p; }
	hipError_t clear(int first, int count) { return hipMemsetAsync(dev() + first, 0, sizeof(W) * count, st); }
	hipError_t fetch(W* host)
	{
		const hipError_t e1 = hipMemcpyAsync(host, buf.p, sizeof(W) * N, hipMemcpyDeviceToHost, st);
		const hipError_t e2 = hipStreamSynchronize(st);
		return e1 != hipSuccess ? e1 : e2;
	}
};

// a finished temporary becomes an array of the DevCsr (whatever the field held is released)
template <typename P> void adopt(P*& field, DevBuf& b)
{
	if (field) (void)hipFree(field);
	field = (P*)b.p;
	b.p = nullptr;
}

// rows strictly sorted by column?  *unsorted: some row is not
lpp_status rows_unsorted(lpp_engine* e, const DevCsr& A, const char* what, bool* unsorted)
{
	DevFlags<int, 1> flag;
	HIP_TRY_MEM(flag.init(e->stream));
	k_rows_sorted<<<(int)((A.nrows + 255) / 256), 256, 0, e->stream>>>(A.nrows, A.rowptr, A.col, flag.dev());
	int h = 1;
	if (flag.fetch(&h) != hipSuccess) return fail(LPP_ERR_HIP, what);
	*unsorted = h != 0;
	return LPP_OK;
}

// distinct values of vals -> sorted dictionary on the device (A.dict, A.ndict); *ok == false when there are more than 256
template <typename T> lpp_status try_build_dict(lpp_engine* e, DevCsr& A, const T* vals, int64_t nvals, bool* ok)
{
	*ok = false;
	if (nvals == 0) return LPP_OK;
	DictTable t;
	lpp_status st = t.init(e->stream);
	if (st != LPP_OK) return st;
	const int64_t nd = nvals * (int64_t)(sizeof(T) / sizeof(double));
	k_dict_collect<<<2048, kBlock, 0, e->stream>>>((const double*)vals, nd, t.dev(), t.dev_overflow());
	if (t.fetch(e->stream) != LPP_OK || hipStreamSynchronize(e->stream) != hipSuccess) return fail(LPP_ERR_HIP, "dictionary collection failed");
	std::vector<unsigned long long> keys;
	for (unsigned long long k : t.host)
		if (k != kDictEmpty) keys.push_back(k);
	std::vector<double> dict;
	const int ndict = t.ov ? 0 : dict256_from_keys(std::move(keys), dict);
	if (ndict == 0) return LPP_OK;
	HIP_TRY_MEM(hipMalloc(&A.dict, sizeof(double) * 256));
	HIP_TRY(hipMemcpyAsync(A.dict, dict.data(), sizeof(double) * 256, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	A.ndict = ndict;
	*ok = true;
	return LPP_OK;
}

void drop_dia(DevCsr& A)
{
	for (void* p : { (void*)A.rrowptr, (void*)A.dia_off, A.dia_val, (void*)A.dcode })
		if (p) (void)hipFree(p);
	A.rrowptr = nullptr;
	A.dcode = nullptr;
	A.dia_off = nullptr;
	A.dia_val = nullptr;
	A.rnnz = A.ndia = 0;
	A.dia_stride = 0;
}

// Split the shared-offset entries off the plain CSR of A (see k_dia_split).  On success with A.rrowptr != nullptr the
// rest CSR is (A.rrowptr, rcol, rval) and A.dia_* hold the shared lists.
// Leaves A untouched (rrowptr == nullptr) when rows are unsorted or fewer than 10 % of the entries are shared.
// xdiag: also split the diagonal off (needs the value dictionary: its codes go to A.dcode, one per real component and row)
template <typename T>
lpp_status split_dia_t(lpp_engine* e, DevCsr& A, const SliceGeom& g, bool for_window, bool xdiag, bool verbose, DevBuf& rcol, DevBuf& rval)
{
	if (!A.known_sorted) {
		bool unsorted = true;
		lpp_status st = rows_unsorted(e, A, "shared-offset split: sortedness check failed", &unsorted);
		if (st != LPP_OK) return st;
		if (unsorted) return LPP_OK;
	}
	DevFlags<unsigned long long, 4> flags; // [0] unused, [1] max shared per slice, [2] total shared, [3] rows without a diagonal
	HIP_TRY_MEM(flags.init(e->stream));
	unsigned long long h[4] = { 0, 0, 0, 0 };
	HIP_TRY_MEM(hipMalloc(&A.rrowptr, sizeof(int64_t) * (size_t)(A.nrows + 1)));
	HIP_TRY(hipMemsetAsync(A.rrowptr, 0, sizeof(int64_t) * (size_t)(A.nrows + 1), e->stream));
	const int nbw = (int)std::max<int64_t>(1, std::min<int64_t>((g.nslices + 3) / 4, 16384));
	const int win = for_window ? 1 : 0;
	int xd = xdiag ? 1 : 0;
	{
		StageTimer t_count("  split: count pass", verbose);
		for (;;) {
			k_dia_split<T, false><<<nbw, kBlock, 0, e->stream>>>(g, A.rowptr, A.col, (const T*)A.val, win, 0, A.rrowptr, flags.dev() + 1, nullptr, nullptr,
			                                                    nullptr, nullptr, nullptr, xd, nullptr, 0, nullptr);
			HIP_TRY(hipGetLastError());
			HIP_TRY(flags.fetch(h));
			if (!xd || h[3] == 0) break;
			// some row has no diagonal entry: count again with the diagonal left where it is
			xd = 0;
			HIP_TRY(hipMemsetAsync(A.rrowptr, 0, sizeof(int64_t) * (size_t)(A.nrows + 1), e->stream));
			HIP_TRY(flags.clear(1, 3));
		}
	}
	lpp_status st = scan_exclusive(e, A.rrowptr, A.nrows + 1, &A.rnnz);
	if (st != LPP_OK) return st;
	A.ndia = (int64_t)h[2];
	A.dia_stride = (int)((h[1] + 3) & ~3ull);
	if (verbose)
		fprintf(stderr, "lpp: shared-offset split: nnz %lld -> per-row %lld + %lld per-slice entries (%lld slices, <= %d per slice)%s\n",
		        (long long)A.nnz, (long long)A.rnnz, (long long)A.ndia, (long long)g.nslices, (int)h[1], xd ? " + diagonal codes" : "");
	if ((double)(A.nnz - A.rnnz) < 0.10 * (double)A.nnz || (A.dia_stride == 0 && !xd)) {
		drop_dia(A);
		return LPP_OK;
	}
	if (xd) {
		HIP_TRY_MEM(hipMalloc(&A.dcode, (size_t)A.nrows * (sizeof(T) / sizeof(double))));
		HIP_TRY(hipMemsetAsync(A.dcode, 0, (size_t)A.nrows * (sizeof(T) / sizeof(double)), e->stream));
	}
	{
		StageTimer t_alloc("  split: allocations", verbose);
		const size_t places = std::max<size_t>((size_t)g.nslices * (size_t)A.dia_stride, 1);
		HIP_TRY_MEM(rcol.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(A.rnnz, 1)));
		HIP_TRY_MEM(rval.alloc(sizeof(T) * (size_t)std::max<int64_t>(A.rnnz, 1)));
		HIP_TRY_MEM(hipMalloc(&A.dia_off, sizeof(int32_t) * places));
		HIP_TRY_MEM(hipMalloc(&A.dia_val, sizeof(T) * places));
		HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.dia_off, (int)kDiaNone, places, e->stream));
		HIP_TRY(hipMemsetAsync(A.dia_val, 0, sizeof(T) * places, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	StageTimer t_fill("  split: fill pass", verbose);
	k_dia_split<T, true><<<nbw, kBlock, 0, e->stream>>>(g, A.rowptr, A.col, (const T*)A.val, win, A.dia_stride, nullptr, nullptr, A.rrowptr,
	                                                   (int32_t*)rcol.p, (T*)rval.p, A.dia_off, (T*)A.dia_val, xd, A.dict, A.ndict, A.dcode);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

// ---- build_sliced: the sliced layout of A for row blocks of B rows, as a sequence of steps over this state ----------------------------
template <typename T> struct SlicedBuild {
	lpp_engine* e;
	DevCsr& A;
	const CsrSwitches& sw;
	bool for_window;
	SliceGeom g;
	// the CSR the sliced arrays hold: the plain one, or the rest after the shared-offset split (then rcol / rval own its arrays)
	const int64_t* rp;
	const int32_t* cc;
	const T* vv;
	int64_t nz;
	DevBuf rcol, rval;
	bool coded = false;
	SlicedShape shape() const
	{
		SlicedShape s = sliced_shape(A, sizeof(T));
		s.entries = nz;
		s.coded = coded;
		return s;
	}
	int fill_blocks() const { return (int)std::max<int64_t>(1, std::min<int64_t>((g.nslices + 3) / 4, 8192)); }
};

// the value dictionary is built from the whole matrix first: the diagonal codes need it
template <typename T> lpp_status step_value_dictionary(SlicedBuild<T>& b)
{
	if (!value_dictionary_wanted(b.e->cfg.compress_values, b.sw)) return LPP_OK;
	StageTimer tm("value dictionary", b.sw.verbose);
	return try_build_dict<T>(b.e, b.A, b.vv, b.nz, &b.coded);
}

// entries shared by all rows of a slice are split off; the sliced arrays then hold the rest
template <typename T> lpp_status step_shared_offsets(SlicedBuild<T>& b)
{
	DevCsr& A = b.A;
	if (!shared_offsets_wanted(A.no_dia, b.sw) || A.nnz <= 0) return LPP_OK;
	StageTimer tm("shared-offset split", b.sw.verbose);
	lpp_status st = split_dia_t<T>(b.e, A, b.g, b.for_window, diag_codes_wanted(b.for_window, b.coded, b.sw), b.sw.verbose, b.rcol, b.rval);
	if (st != LPP_OK) return st;
	if (A.rrowptr) {
		b.rp = A.rrowptr;
		b.cc = (const int32_t*)b.rcol.p;
		b.vv = (const T*)b.rval.p;
		b.nz = A.rnnz;
	}
	return LPP_OK;
}

// window kernel: 16-bit window-local columns when every per-row entry stays inside its row block
template <typename T> lpp_status step_local16(SlicedBuild<T>& b)
{
	b.A.local16 = false;
	if (!local16_check_wanted(b.for_window, b.g, b.nz, b.sw)) return LPP_OK;
	DevFlags<int, 1> outside;
	HIP_TRY_MEM(outside.init(b.e->stream));
	k_cols_local<<<(int)((b.A.nrows + 255) / 256), 256, 0, b.e->stream>>>(b.g, b.rp, b.cc, outside.dev());
	int bad = 0;
	if (outside.fetch(&bad) != hipSuccess) return fail(LPP_ERR_HIP, "column locality check failed");
	b.A.local16 = !bad;
	return LPP_OK;
}

// slice pointers, row lengths and the column array; with the dictionary, the per-slice word counts scanned into code_ptr and the code array
template <typename T> lpp_status step_slice_arrays(SlicedBuild<T>& b)
{
	DevCsr& A = b.A;
	const SliceGeom& g = b.g;
	hipStream_t st = b.e->stream;
	SlicedSizes z = sliced_sizes(b.shape());
	HIP_TRY_MEM(hipMalloc(&A.slice_ptr, z.slice_ptr));
	HIP_TRY_MEM(hipMalloc(&A.row_len, std::max<size_t>(z.row_len, sizeof(int32_t))));
	const size_t colsz = A.local16 ? sizeof(uint16_t) : sizeof(int32_t);
	HIP_TRY_MEM(hipMalloc(&A.scol, z.scol));
	HIP_TRY(hipMemsetAsync((char*)A.scol + colsz * (size_t)b.nz, 0, colsz * kSliceSlack, st));
	if (b.coded) HIP_TRY_MEM(hipMalloc(&A.code_ptr, z.code_ptr));
	const int64_t nthreads = std::max<int64_t>(A.nrows, g.nslices + 1);
	k_slice_meta<<<(int)((nthreads + 255) / 256), 256, 0, st>>>(g, b.rp, A.slice_ptr, A.row_len, A.code_ptr, CodeTraits<T>::kSlotsPerWord);
	if (!b.coded) return LPP_OK;
	// exclusive scan of the per-slice word counts -> code_ptr; the grand total sizes the code array
	lpp_status rc = scan_exclusive(b.e, A.code_ptr, g.nslices + 1, &A.code_words);
	if (rc != LPP_OK) return rc;
	z = sliced_sizes(b.shape());
	HIP_TRY_MEM(hipMalloc(&A.codes, z.codes));
	HIP_TRY(hipMemsetAsync(A.codes + A.code_words, 0, sizeof(uint32_t) * kCodeSlack, st));
	return LPP_OK;
}

// slot-major columns and value codes
template <typename T> lpp_status step_fill_coded(SlicedBuild<T>& b)
{
	DevCsr& A = b.A;
	hipStream_t st = b.e->stream;
	const int nb2 = b.fill_blocks();
	if (A.local16)
		k_slice_fill<T, false, true><<<nb2, kBlock, 0, st>>>(b.g, b.rp, b.cc, (const T*)nullptr, A.scol, (T*)nullptr);
	else
		k_slice_fill<T, false><<<nb2, kBlock, 0, st>>>(b.g, b.rp, b.cc, (const T*)nullptr, A.scol, (T*)nullptr);
	k_slice_codes<T><<<nb2, kBlock, 0, st>>>(b.g, b.rp, b.vv, A.code_ptr, A.dict, A.ndict, A.codes);
	A.coded = true;
	return LPP_OK;
}

// slot-major columns and plain values; window kernel: the leaving entries first, the vectors pitched (lpp_csr_plan.h)
template <typename T> lpp_status step_fill_plain(SlicedBuild<T>& b)
{
	lpp_engine* e = b.e;
	DevCsr& A = b.A;
	const SliceGeom& g = b.g;
	hipStream_t st = e->stream;
	HIP_TRY_MEM(hipMalloc(&A.sval, sliced_sizes(b.shape()).sval));
	HIP_TRY(hipMemsetAsync((T*)A.sval + b.nz, 0, sizeof(T) * kSliceSlack, st));
	bool outs = outs_first_eligible(b.for_window, A.local16, b.rp != A.rowptr, g, b.nz, b.sw);
	if (outs && !A.known_sorted) { // needs rows sorted by column
		bool unsorted = true;
		lpp_status rc = rows_unsorted(e, A, "row order check failed", &unsorted);
		if (rc != LPP_OK) return rc;
		outs = !unsorted;
	}
	A.outs_first = outs;
	const bool whole_matrix = &A == &e->A_loc && !A.out_part && !e->has_comm && !e->is_complex && A.src_elems == 0;
	const int pad = pitch_pad(g, sizeof(T), outs && whole_matrix, b.sw);
	A.pad = pad;
	if (pad) {
		e->pitch = g.B + pad;
		e->pitch_rows = g.B;
		e->pitch_blocks = g.nblocks;
	}
	const int nb2 = b.fill_blocks();
	if (A.local16)
		k_slice_fill<T, false, true><<<nb2, kBlock, 0, st>>>(g, b.rp, b.cc, b.vv, A.scol, (T*)A.sval);
	else
		k_slice_fill<T, false><<<nb2, kBlock, 0, st>>>(g, b.rp, b.cc, b.vv, A.scol, (T*)A.sval, 0, outs ? 1 : 0, pad);
	return LPP_OK;
}

// Block template (block_template_check_wanted): when every row block repeats block 0, only block 0's copy of the structure is kept
// (level 1), and of the code words as well when they repeat too (level 2: the diagonal travels apart)
template <typename T> lpp_status step_block_template(SlicedBuild<T>& b)
{
	DevCsr& A = b.A;
	const SliceGeom& g = b.g;
	hipStream_t st = b.e->stream;
	if (!block_template_check_wanted(A.local16, b.coded, g, b.sw)) return LPP_OK;
	DevFlags<int, 2> differs; // [0] the structure, [1] the value codes
	HIP_TRY_MEM(differs.init(st));
	k_tmpl_check<<<b.fill_blocks(), kBlock, 0, st>>>(g, A.slice_ptr, A.row_len, (const uint16_t*)A.scol, A.code_ptr, A.codes, differs.dev());
	int hd[2] = { 1, 1 };
	if (differs.fetch(hd) != hipSuccess) return fail(LPP_ERR_HIP, "block-template check failed");
	if (hd[0]) return LPP_OK;
	SlicedShape s = b.shape();
	s.tmpl = hd[1] ? 1 : 2;
	int64_t w0 = 0, n0 = 0; // code words and entries of block 0
	HIP_TRY(hipMemcpy(&w0, A.code_ptr + g.spb, sizeof(int64_t), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(&n0, A.slice_ptr + g.spb, sizeof(int64_t), hipMemcpyDeviceToHost));
	if (n0 * g.nblocks != b.nz) return fail(LPP_ERR_HIP, "block-template check failed"); // the sizes below take every block to hold block 0's entries
	if (s.tmpl == 2) s.code_words = w0;
	const SlicedSizes z = sliced_sizes(s);
	DevBuf cp, cw, sp, rl, sc;
	if (s.tmpl == 2) {
		// the value codes repeat as well: keep block 0's code words only
		HIP_TRY_MEM(cp.alloc(z.code_ptr));
		HIP_TRY_MEM(cw.alloc(z.codes));
		HIP_TRY(hipMemcpyAsync(cp.p, A.code_ptr, z.code_ptr, hipMemcpyDeviceToDevice, st));
		HIP_TRY(hipMemcpyAsync(cw.p, A.codes, sizeof(uint32_t) * (size_t)w0, hipMemcpyDeviceToDevice, st));
		HIP_TRY(hipMemsetAsync((uint32_t*)cw.p + w0, 0, sizeof(uint32_t) * kCodeSlack, st));
	}
	HIP_TRY_MEM(sp.alloc(z.slice_ptr));
	HIP_TRY_MEM(rl.alloc(z.row_len));
	HIP_TRY_MEM(sc.alloc(z.scol));
	HIP_TRY(hipMemcpyAsync(sp.p, A.slice_ptr, z.slice_ptr, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipMemcpyAsync(rl.p, A.row_len, z.row_len, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipMemcpyAsync(sc.p, A.scol, sizeof(uint16_t) * (size_t)n0, hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipMemsetAsync((char*)sc.p + sizeof(uint16_t) * (size_t)n0, 0, sizeof(uint16_t) * kSliceSlack, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (s.tmpl == 2) {
		adopt(A.code_ptr, cp);
		adopt(A.codes, cw);
		A.code_words = w0;
	}
	adopt(A.slice_ptr, sp);
	adopt(A.row_len, rl);
	adopt(A.scol, sc);
	A.tmpl = s.tmpl;
	return LPP_OK;
}

// packed padded copy of a level-2 template for the inner loop (the compact copy stays for get_csr)
template <typename T> lpp_status step_template_pack(SlicedBuild<T>& b)
{
	DevCsr& A = b.A;
	const SliceGeom& g = b.g;
	hipStream_t st = b.e->stream;
	if (!template_pack_wanted(A.tmpl, b.sw)) return LPP_OK;
	HIP_TRY_MEM(hipMalloc(&A.tw_len, sizeof(int32_t) * (size_t)g.spb));
	HIP_TRY_MEM(hipMalloc(&A.tw_off, sizeof(int32_t) * (size_t)g.spb));
	const int nbp = (int)std::max<int64_t>(1, (g.spb + 3) / 4);
	k_tmpl_pack<T, 0><<<nbp, kBlock, 0, st>>>(g, A.slice_ptr, A.row_len, (const uint16_t*)A.scol, A.code_ptr, A.codes, A.tw_len, nullptr, nullptr);
	std::vector<int32_t> hl((size_t)g.spb), ho((size_t)g.spb);
	HIP_TRY(hipMemcpyAsync(hl.data(), A.tw_len, sizeof(int32_t) * (size_t)g.spb, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	int64_t tot = 0;
	for (int32_t j2 = 0; j2 < g.spb; j2++) {
		ho[(size_t)j2] = (int32_t)tot;
		tot += (int64_t)hl[(size_t)j2] * 64;
	}
	if (tot >= ((int64_t)1 << 30)) return LPP_OK;
	HIP_TRY_MEM(hipMalloc(&A.tw, sizeof(uint32_t) * (size_t)std::max<int64_t>(tot, 1)));
	HIP_TRY(hipMemcpyAsync(A.tw_off, ho.data(), sizeof(int32_t) * (size_t)g.spb, hipMemcpyHostToDevice, st));
	k_tmpl_pack<T, 1><<<nbp, kBlock, 0, st>>>(g, A.slice_ptr, A.row_len, (const uint16_t*)A.scol, A.code_ptr, A.codes, A.tw_len, A.tw_off, A.tw);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	return LPP_OK;
}

template <typename T> lpp_status build_sliced_t(lpp_engine* e, DevCsr& A, const CsrSwitches& sw, int64_t B, bool for_window)
{
	A.geom = slice_geom(A.nrows, B);
	SlicedBuild<T> b { e, A, sw, for_window, A.geom, A.rowptr, A.col, (const T*)A.val, A.nnz, {}, {} };
	lpp_status st;
	if ((st = step_value_dictionary(b)) != LPP_OK) return st;
	if ((st = step_shared_offsets(b)) != LPP_OK) return st;
	if ((st = step_local16(b)) != LPP_OK) return st;
	if ((st = step_slice_arrays(b)) != LPP_OK) return st;
	if ((st = b.coded ? step_fill_coded(b) : step_fill_plain(b)) != LPP_OK) return st;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->stream));
	A.sliced = true;
	if ((st = step_block_template(b)) != LPP_OK) return st;
	return step_template_pack(b);
}

// the out parts of a split-panel build until they are handed to the matrix
struct OutParts {
	DevCsr* o;
	int n;
	~OutParts()
	{
		if (!o) return;
		for (int q = 0; q < n; q++) free_csr(o[q]);
		delete[] o;
	}
};

// Split-panel layout (k_split_count): A keeps the entries inside its row blocks, *A.out_part takes the others in panel-major row
// order.  Only for plain-format matrices (shared offsets off: they take the leaving entries out of the rows in their own way),
// rows sorted by column, whole blocks, and a leaving part worth a second launch (>= 20 % of the entries).
template <typename T> lpp_status split_panel_t(lpp_engine* e, DevCsr& A, const CsrSwitches& sw, int64_t B, bool* did)
{
	*did = false;
	const int64_t nb = A.nrows / B;
	if (nb < 64 || nb * B != A.nrows || !A.col || !A.val || A.nnz == 0) return LPP_OK;
	hipStream_t st = e->stream;
	if (!A.known_sorted) {
		bool unsorted = true;
		lpp_status rc = rows_unsorted(e, A, "split-panel layout: sortedness check failed", &unsorted);
		if (rc != LPP_OK) return rc;
		if (unsorted) return LPP_OK;
	}
	StageTimer tm("split-panel layout", sw.verbose);
	SplitParams P;
	P.nrows = A.nrows;
	P.B = B;
	P.nb = nb;
	P.nparts = split_panel_parts(sw, kSplitMaxParts);
	P.pblk = (nb + P.nparts - 1) / P.nparts;
	const int nbk = (int)((A.nrows + 255) / 256);
	OutParts parts { new DevCsr[P.nparts], P.nparts };
	DevCsr* O = parts.o;
	DevBuf rpi, ci, vi, map, ptrs; // the in-block CSR, the row map, the parts' row pointers as the kernel reads them
	HIP_TRY_MEM(rpi.alloc(sizeof(int64_t) * (size_t)(A.nrows + 1)));
	HIP_TRY_MEM(map.alloc(sizeof(int32_t) * (size_t)A.nrows));
	HIP_TRY(hipMemsetAsync(rpi.p, 0, sizeof(int64_t) * (size_t)(A.nrows + 1), st));
	int64_t* lens[kSplitMaxParts] = { nullptr, nullptr, nullptr, nullptr };
	for (int q = 0; q < P.nparts; q++) {
		O[q].nrows = A.nrows;
		O[q].owned = true;
		O[q].known_sorted = true;
		O[q].no_dia = true;
		HIP_TRY_MEM(hipMalloc(&O[q].rowptr, sizeof(int64_t) * (size_t)(A.nrows + 1)));
		HIP_TRY(hipMemsetAsync(O[q].rowptr, 0, sizeof(int64_t) * (size_t)(A.nrows + 1), st));
		lens[q] = O[q].rowptr;
	}
	HIP_TRY_MEM(ptrs.alloc(sizeof(lens)));
	HIP_TRY(hipMemcpyAsync(ptrs.p, lens, sizeof(lens), hipMemcpyHostToDevice, st));
	k_split_count<<<nbk, 256, 0, st>>>(P, A.rowptr, A.col, (int64_t*)rpi.p, (int64_t* const*)ptrs.p, (int32_t*)map.p);
	int64_t nin = 0, nout = 0;
	lpp_status rc = scan_exclusive(e, (int64_t*)rpi.p, A.nrows + 1, &nin);
	if (rc != LPP_OK) return rc;
	for (int q = 0; q < P.nparts; q++) {
		rc = scan_exclusive(e, O[q].rowptr, A.nrows + 1, &O[q].nnz);
		if (rc != LPP_OK) return rc;
		nout += O[q].nnz;
	}
	if (nin + nout != A.nnz) return fail(LPP_ERR_HIP, "split-panel layout: entry count mismatch");
	if ((double)nout < 0.20 * (double)A.nnz) return LPP_OK; // not worth the extra launches
	HIP_TRY_MEM(ci.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(nin, 1)));
	HIP_TRY_MEM(vi.alloc(sizeof(T) * (size_t)std::max<int64_t>(nin, 1)));
	SplitOut SO {};
	for (int q = 0; q < P.nparts; q++) {
		HIP_TRY_MEM(hipMalloc(&O[q].col, sizeof(int32_t) * (size_t)std::max<int64_t>(O[q].nnz, 1)));
		HIP_TRY_MEM(hipMalloc(&O[q].val, sizeof(T) * (size_t)std::max<int64_t>(O[q].nnz, 1)));
		SO.rp[q] = O[q].rowptr;
		SO.col[q] = O[q].col;
		SO.val[q] = O[q].val;
	}
	k_split_fill<T><<<nbk, 256, 0, st>>>(P, A.rowptr, A.col, (const T*)A.val, (const int64_t*)rpi.p, (int32_t*)ci.p, (T*)vi.p, SO);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	// the in-block part replaces the matrix in A
	adopt(A.rowptr, rpi);
	adopt(A.col, ci);
	adopt(A.val, vi);
	A.nnz = nin;
	A.known_sorted = true;
	// the leaving parts: sliced layout over ALL rows in panel-major order (one "block" = the whole matrix)
	for (int q = 0; q < P.nparts; q++) {
		rc = finalize_csr(e, O[q], sw, true, LPP_SPMV_SLICED, 0);
		if (rc != LPP_OK) return rc;
	}
	A.out_part = O;
	A.split_parts = P.nparts;
	parts.o = nullptr;
	adopt(A.out_rowmap, map);
	A.split_B = B;
	A.split_nb = nb;
	A.split_pblk = P.pblk;
	*did = true;
	return LPP_OK;
}

// entries of A inside the diagonal window of gw rows around their row (k_count_local)
lpp_status count_window_entries(lpp_engine* e, const DevCsr& A, int64_t gw, unsigned long long* counted)
{
	DevFlags<unsigned long long, 1> inside;
	HIP_TRY_MEM(inside.init(e->stream));
	k_count_local<<<(int)((A.nrows + 255) / 256), 256, 0, e->stream>>>(A.nrows, gw, A.rowptr, A.col, inside.dev());
	if (inside.fetch(counted) != hipSuccess) return fail(LPP_ERR_HIP, "window locality count failed");
	return LPP_OK;
}

} // namespace

StageTimer::~StageTimer()
{
	if (on) fprintf(stderr, "lpp: %-28s %8.1f ms\n", what, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

// in-place exclusive scan of arr[0..n) (arr[n-1] must be 0 on entry and receives the total, also returned)
lpp_status scan_exclusive(lpp_engine* e, int64_t* arr, int64_t n, int64_t* total_out)
{
	const int64_t nblk = (n + kScanChunk - 1) / kScanChunk;
	DevBuf sums, total;
	if (sums.alloc(sizeof(int64_t) * (size_t)nblk) != hipSuccess || total.alloc(sizeof(int64_t)) != hipSuccess)
		return fail(LPP_ERR_NOMEM, "scan scratch allocation failed");
	k_scan_block_sums<<<(int)nblk, kBlock, 0, e->stream>>>(arr, n, (int64_t*)sums.p);
	k_scan_sums<<<1, kBlock, 0, e->stream>>>((int64_t*)sums.p, nblk, (int64_t*)total.p);
	k_scan_apply<<<(int)nblk, kBlock, 0, e->stream>>>(arr, n, (int64_t*)sums.p, arr);
	hipError_t e1 = hipMemcpyAsync(total_out, total.p, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream);
	hipError_t e2 = hipStreamSynchronize(e->stream);
	if (e1 != hipSuccess || e2 != hipSuccess) return fail(LPP_ERR_HIP, "device scan failed");
	return LPP_OK;
}

// The sampling half of the basis-block detection (RowBlockDetector, lpp_csr_plan.h): which 64-row slices, and the three copies per sample
int64_t detect_row_block(lpp_engine* e, const DevCsr& A, size_t esz, int64_t cap_elems)
{
	if (!A.col || !A.val || A.nnz == 0) return 0;
	RowBlockDetector det;
	std::vector<int64_t> rp(65);
	std::vector<int32_t> ci;
	std::vector<char> va;
	for (int64_t row0 : detect_sample_rows(A.nrows)) {
		if (hipMemcpy(rp.data(), A.rowptr + row0, sizeof(int64_t) * 65, hipMemcpyDeviceToHost) != hipSuccess) return 0;
		const int64_t p0 = rp[0], n = rp[64] - rp[0];
		if (!detect_sample_usable(n)) continue;
		ci.resize((size_t)n);
		va.resize((size_t)n * esz);
		if (hipMemcpy(ci.data(), A.col + p0, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return 0;
		if (hipMemcpy(va.data(), (const char*)A.val + (size_t)p0 * esz, esz * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return 0;
		det.add(row0, rp.data(), ci.data(), va.data(), esz);
	}
	return det.block(cap_elems);
}

// Choose the SpMV kernel and build its layout: switches, group, optional detection, mode (two steps, the count between), optional
// split-panel, build, optional release.  A.hint_block (rows) is the basis' natural block (N_up for the Hubbard product basis): when a
// whole number of such blocks fits the LDS window, the window kernel serves every in-block gather (diagonal + up-hops) from LDS.
lpp_status finalize_csr(lpp_engine* e, DevCsr& A, bool allow_drop_plain, int force_mode, int64_t force_block)
{
	return finalize_csr(e, A, csr_switches_from_env(), allow_drop_plain, force_mode, force_block);
}

lpp_status finalize_csr(lpp_engine* e, DevCsr& A, const CsrSwitches& sw, bool allow_drop_plain, int force_mode, int64_t force_block)
{
	A.G = pick_group(A.nrows, A.nnz, sw.spmv_g);
	CsrFacts f;
	f.nrows = A.nrows, f.nnz = A.nnz, f.src_elems = A.src_elems, f.hint_block = A.hint_block;
	f.has_plain = A.col != nullptr;
	f.is_complex = e->is_complex, f.esz = e->esz, f.num_cus = e->num_cus;
	f.mode = csr_requested_mode(e->cfg.spmv_kernel, sw, force_mode);
	f.forced = force_mode != 0;
	if (csr_detection_wanted(f, sw)) {
		StageTimer tm("basis block detection", sw.verbose);
		f.hint_block = A.hint_block = detect_row_block(e, A, sizeof(double), f.cap());
		if (A.hint_block && sw.verbose) fprintf(stderr, "lpp: detected a basis block of %lld rows\n", (long long)A.hint_block);
	}
	const int64_t count_window = csr_count_window(f);
	unsigned long long counted = 0;
	if (count_window > 0) {
		lpp_status st = count_window_entries(e, A, count_window, &counted);
		if (st != LPP_OK) return st;
	}
	const CsrMode m = csr_mode(f, sw, count_window, counted);
	if (!m.sliced() || A.nrows <= 0) return LPP_OK;
	const int64_t B = m.block(A.nrows, force_block);
	if (split_panel_wanted(f, m, B, shared_offsets_wanted(A.no_dia, sw), A.out_part != nullptr, sw)) {
		bool did = false;
		lpp_status st = e->is_complex ? split_panel_t<cplx>(e, A, sw, B, &did) : split_panel_t<double>(e, A, sw, B, &did);
		if (st != LPP_OK) return st;
	}
	StageTimer tm("sliced layout (total)", sw.verbose);
	lpp_status st = e->is_complex ? build_sliced_t<cplx>(e, A, sw, B, m.window()) : build_sliced_t<double>(e, A, sw, B, m.window());
	if (st != LPP_OK) return st;
	A.window = m.window();
	if (release_plain_wanted(allow_drop_plain, A.owned, sw)) {
		StageTimer tm2("release plain CSR", sw.verbose);
		(void)hipFree(A.col);
		(void)hipFree(A.val);
		A.col = nullptr;
		A.val = nullptr;
	}
	return LPP_OK;
}

// Plain CSR order (columns, values) of a matrix whose only resident form is the sliced layout: undo the slot-major
// order (template-aware), decode the value codes, then merge the per-slice shared entries and the diagonal codes back.
template <typename T> static lpp_status rebuild_csr_t(lpp_engine* e, const DevCsr& A, DevBuf& col_out, DevBuf& val_out)
{
	const int64_t* rp = A.rrowptr ? A.rrowptr : A.rowptr; // the sliced arrays hold the rest CSR when entries were split off
	const int64_t nz = A.rrowptr ? A.rnnz : A.nnz;
	DevBuf tcol, tval;
	if (tcol.alloc(sizeof(int32_t) * (size_t)nz) != hipSuccess || tval.alloc(sizeof(T) * (size_t)nz) != hipSuccess)
		return fail(LPP_ERR_NOMEM, "lpp_engine_get_csr: scratch allocation failed");
	const int nb2 = (int)std::max<int64_t>(1, std::min<int64_t>((A.geom.nslices + 3) / 4, 8192));
	T* plain_vals = A.coded ? nullptr : (T*)tval.p;
	if (A.local16)
		k_slice_fill<T, true, true><<<nb2, kBlock, 0, e->stream>>>(A.geom, rp, A.scol, (const T*)A.sval, (int32_t*)tcol.p, plain_vals, A.tmpl ? 1 : 0);
	else
		k_slice_fill<T, true><<<nb2, kBlock, 0, e->stream>>>(A.geom, rp, A.scol, (const T*)A.sval, (int32_t*)tcol.p, plain_vals, 0, A.outs_first ? 1 : 0, A.pad);
	if (A.coded) k_slice_decode<T><<<nb2, kBlock, 0, e->stream>>>(A.geom, rp, A.codes, A.code_ptr, A.dict, (T*)tval.p, A.tmpl == 2 ? 1 : 0);
	if (A.rrowptr) {
		DevBuf fcol, fval;
		if (fcol.alloc(sizeof(int32_t) * (size_t)A.nnz) != hipSuccess || fval.alloc(sizeof(T) * (size_t)A.nnz) != hipSuccess)
			return fail(LPP_ERR_NOMEM, "lpp_engine_get_csr: scratch allocation failed");
		k_dia_merge<T><<<(int)((A.nrows + 255) / 256), 256, 0, e->stream>>>(A.geom, A.rowptr, rp, (const int32_t*)tcol.p, (const T*)tval.p, A.dia_stride,
		                                                                   A.dia_off, (const T*)A.dia_val, (int32_t*)fcol.p, (T*)fval.p, A.dcode, A.dict);
		HIP_TRY(hipStreamSynchronize(e->stream)); // the merge reads tcol / tval, which are released next
		tcol.take(fcol);
		tval.take(fval);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->stream));
	col_out.take(tcol);
	val_out.take(tval);
	return LPP_OK;
}

lpp_status rebuild_csr(lpp_engine* e, const DevCsr& A, DevBuf& col_out, DevBuf& val_out)
{
	return e->is_complex ? rebuild_csr_t<cplx>(e, A, col_out, val_out) : rebuild_csr_t<double>(e, A, col_out, val_out);
}

} // namespace lpp
