// lpp_engine.hip -- the MI355X-native Lanczos inner engine behind include/lpp_engine.h.
//
// Device boundary: the CSR is made resident once, the whole
// computeAllStatesBelow loop (reference src/Engine/Engine.h:601-657 -> LanczosSolver
// [PsimagLite]) runs on the GPU, only the tridiagonal coefficients (and requested Ritz
// vectors) come back.  The host keeps the tiny tridiagonal eigenproblem and tests convergence
// `check_lag` steps behind the GPU so the stream never drains.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "lpp_assemble_kernels.h"
#include "lpp_engine_impl.h"
#include "lpp_launch.h"

using namespace lpp;

namespace lpp {

template <typename T, bool DOT>
static void launch_rowgroup(const DevCsr& A, const T* src, T* x, const T* ydot, double* partial, int nblocks,
                            hipStream_t st, const EpiScale& sc)
{
	const int64_t* rp = A.rowptr;
	const int32_t* col = A.col;
	const T* val = (const T*)A.val;
	switch (A.G) {
	case 4: k_spmv_rowgroup<T, 4, DOT><<<nblocks, kBlock, 0, st>>>(A.nrows, rp, col, val, src, x, ydot, partial, sc); break;
	case 8: k_spmv_rowgroup<T, 8, DOT><<<nblocks, kBlock, 0, st>>>(A.nrows, rp, col, val, src, x, ydot, partial, sc); break;
	case 16: k_spmv_rowgroup<T, 16, DOT><<<nblocks, kBlock, 0, st>>>(A.nrows, rp, col, val, src, x, ydot, partial, sc); break;
	case 32: k_spmv_rowgroup<T, 32, DOT><<<nblocks, kBlock, 0, st>>>(A.nrows, rp, col, val, src, x, ydot, partial, sc); break;
	default: k_spmv_rowgroup<T, 64, DOT><<<nblocks, kBlock, 0, st>>>(A.nrows, rp, col, val, src, x, ydot, partial, sc); break;
	}
}

// the kernel arguments of a sliced matrix; rowmap: the rows of an out part of the split-panel layout (null: rows in place)
template <typename T>
static SlicedArgs<T> sliced_args(const DevCsr& A, const void* src, void* x, const void* ydot, double* partial, const EpiScale& sc, int xcd_map, const int32_t* rowmap)
{
	SlicedArgs<T> a {};
	a.g = A.geom;
	a.slice_ptr = A.slice_ptr;
	a.row_len = A.row_len;
	a.col = A.scol;
	a.val = (const T*)A.sval;
	a.codes = A.codes;
	a.code_ptr = A.code_ptr;
	a.dict = A.dict;
	a.src = (const T*)src;
	a.x = (T*)x;
	a.ydot = (const T*)ydot;
	a.partial = partial;
	a.xcd_map = xcd_map;
	a.sc = sc;
	a.dia_stride = A.dia_stride;
	a.dia_off = A.dia_off;
	a.dia_val = (const T*)A.dia_val;
	a.tmpl = A.tmpl;
	a.dcode = A.dcode;
	a.tw = A.tw;
	a.tw_off = A.tw_off;
	a.tw_len = A.tw_len;
	a.rowmap = rowmap;
	a.pad = A.pad;
	return a;
}

// x += A * src ; if partial != nullptr also partial[b] = block sums of Re<ydot|x>.
// Returns the number of partials written (0 when partial == nullptr).
template <typename T> static int spmv_launch_t(lpp_engine* e, const DevCsr& A, const void* src, void* x, const void* ydot, double* partial, const EpiScale& sc)
{
	hipStream_t st = e->stream;
	if (A.nrows == 0) return 0;
	if (A.sliced) {
		const SlicedArgs<T> a = sliced_args<T>(A, src, x, ydot, partial, sc, (e->k2_variant >> 1) & 1, nullptr);
		const bool u8 = (e->k2_variant & 4) != 0;
		int nb;
		if (A.window) {
			const size_t lds_bytes = sizeof(T) * (size_t)std::max<int64_t>(A.geom.B, 64);
			const int per_cu = std::max(1, std::min(2, (int)((160 * 1024 - 4096) / (lds_bytes + 1))));
			nb = launch_grid(A.geom.nblocks, e->num_cus, per_cu);
			with_flags(
			    [&](auto dot, auto coded, auto u8, auto l16) {
				    launch_lds(k_spmv_window<T, decltype(dot)::value, decltype(coded)::value, decltype(u8)::value ? 8 : 4, decltype(l16)::value>, nb, kWinThreads, lds_bytes, st, a);
			    },
			    partial != nullptr, A.coded, u8, A.local16);
		} else {
			const int64_t need = (A.geom.nslices + (kBlock / 64) - 1) / (kBlock / 64);
			nb = (int)std::max<int64_t>(1, std::min<int64_t>(need, e->spmv_max_blocks));
			if (nb >= 8) nb &= ~7; // multiple of 8 so the XCD-contiguous mapping applies
			with_flags([&](auto dot, auto coded, auto u8) { k_spmv_sliced<T, decltype(dot)::value, decltype(coded)::value, decltype(u8)::value ? 8 : 4><<<nb, kBlock, 0, st>>>(a); },
			           partial != nullptr, A.coded, u8);
		}
		return partial ? nb : 0;
	}
	const int rows_per_block = kBlock / A.G;
	const int64_t need = (A.nrows + rows_per_block - 1) / rows_per_block;
	const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(need, e->spmv_max_blocks));
	if (partial)
		launch_rowgroup<T, true>(A, (const T*)src, (T*)x, (const T*)ydot, partial, nb, st, sc);
	else
		launch_rowgroup<T, false>(A, (const T*)src, (T*)x, nullptr, nullptr, nb, st, sc);
	return partial ? nb : 0;
}

// the part of a split-panel matrix that leaves the row blocks: k_spmv_sliced over the panel-major rows, one contiguous eighth
// of the panels per XCD (so every panel is gathered from ONE L2), x and ydot through the row map
template <typename T> static int spmv_launch_out_t(lpp_engine* e, const DevCsr& A, const int32_t* rowmap, const void* src, void* x, const void* ydot, double* partial, const EpiScale& sc)
{
	if (A.nrows == 0) return 0;
	const SlicedArgs<T> a = sliced_args<T>(A, src, x, ydot, partial, sc, 1, rowmap);
	// two resident workgroups per CU walk the panels together (measured at BASELINE config 2, scripts/experiments/r03_generic_ab.sh:
	// 512 workgroups 9.85 ms and 60.7 GB of fabric reads, 2048 11.1 ms / 66.1 GB, 4096 11.3 ms / 66.2 GB)
	const int64_t need = (A.geom.nslices + (kBlock / 64) - 1) / (kBlock / 64);
	int nb = (int)std::max<int64_t>(1, std::min<int64_t>(need, std::min<int64_t>(e->spmv_max_blocks, 2 * (int64_t)e->num_cus)));
	if (nb >= 8) nb &= ~7;
	hipStream_t st = e->stream;
	with_flags([&](auto dot, auto coded) { k_spmv_sliced<T, decltype(dot)::value, decltype(coded)::value, 8><<<nb, kBlock, 0, st>>>(a); }, partial != nullptr, A.coded);
	return partial ? nb : 0;
}

int spmv_launch(lpp_engine* e, const DevCsr& A, const void* src, void* x, const void* ydot, double* partial, const EpiScale& sc)
{
	if (e->tj.active && &A == &e->A_loc) return tj_launch(e, src, x, ydot, partial, sc); // t-J without a stored matrix (lpp_tj_kernels.h)
	if (A.out_part) { // split-panel layout: the in-block entries first (x = beta x + alpha A_in src), then the leaving ones on top
		if (e->is_complex) spmv_launch_t<cplx>(e, A, src, x, nullptr, nullptr, sc);
		else spmv_launch_t<double>(e, A, src, x, nullptr, nullptr, sc);
		EpiScale sc2 = sc;
		sc2.beta_one = 1;
		int np = 0;
		for (int q = 0; q < A.split_parts; q++) { // the dot rides in the last launch: x is complete there
			const bool last = q == A.split_parts - 1;
			np = e->is_complex ? spmv_launch_out_t<cplx>(e, A.out_part[q], A.out_rowmap, src, x, last ? ydot : nullptr, last ? partial : nullptr, sc2)
			                   : spmv_launch_out_t<double>(e, A.out_part[q], A.out_rowmap, src, x, last ? ydot : nullptr, last ? partial : nullptr, sc2);
		}
		return np;
	}
	return e->is_complex ? spmv_launch_t<cplx>(e, A, src, x, ydot, partial, sc) : spmv_launch_t<double>(e, A, src, x, ydot, partial, sc);
}

void set_spmv_bytes(lpp_engine* e)
{
	const double s = (double)e->esz;
	const double N = (double)e->n_local;
	if (e->pb.active) {
		// the CSR this layout stands for (several GPUs: this rank's share of the rows)
		e->spmv_bytes = (double)e->pb.nnz_loc * (s + 4.0) + (N + 1.0) * 8.0 + 3.0 * N * s;
		return;
	}
	if (e->tj.active) { // the CSR the hole-major t-J form stands for
		e->spmv_bytes = (double)e->tj.nnz * (s + 4.0) + (N + 1.0) * 8.0 + 3.0 * N * s;
		return;
	}
	if (e->kron.active) {
		// matrix-free product: no matrix stream.  Vector-streaming model: x in/out and y once (3 N s) plus one
		// coalesced pass over the source block of every connected down-configuration (H_down off-diagonals).
		const KronState& K = e->kron;
		if (K.terms) { // term-list product: the CSR it stands for, as the SURVEY 8(d) figure
			e->spmv_bytes = K.equiv_nnz * (s + 4.0) + (N + 1.0) * 8.0 + 3.0 * N * s;
			return;
		}
		const double avg_down = K.n_dn > 0 ? ((double)K.dn.nnz - (double)K.n_dn) / (double)K.n_dn : 0.0;
		e->spmv_bytes = N * s * (3.0 + avg_down);
		return;
	}
	const double Z = (double)(e->A_loc.nnz + e->A_loc.out_nnz() + e->A_rem.nnz);
	e->spmv_bytes = Z * (s + 4.0) + (N + 1.0) * 8.0 + 3.0 * N * s;
}

lpp_status alloc_work(lpp_engine* e)
{
	// vectors are padded to an even number of doubles so BLAS-1 kernels can move double2
	// product-basis matrices keep their vectors pitched (block b at element b*pitch, padding zero)
	const int64_t nd = (e->pitch > 0 ? e->pitch * e->pitch_blocks : e->n_local) * (e->is_complex ? 2 : 1);
	e->nd = nd;
	e->nd_pad = (nd + 1) & ~(int64_t)1;
	e->n2 = e->nd_pad / 2;
	for (double** p : { &e->x, &e->y }) {
		if (*p) (void)hipFree(*p);
		*p = nullptr;
		HIP_TRY_MEM(hipMalloc(p, sizeof(double) * (size_t)std::max<int64_t>(e->nd_pad, 2)));
		HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * (size_t)std::max<int64_t>(e->nd_pad, 2), e->stream));
	}
	return LPP_OK;
}

// The skeleton of a matrix set-up entry point: begin, build, finish.  The opening step of the single-GPU ones: no communicator,
// the engine's own scalars, no remote part, no product state.  A_loc is the caller's to free, before or after its builder.
void begin_single_gpu(lpp_engine* e)
{
	e->has_comm = false;
	e->bind_scalars(e->scal_own);
	free_csr(e->A_rem);
	drop_product(e);
}

// ... and the closing step of every one: the only place that sets the rows of a new matrix and ends a Lanczos run in flight
lpp_status finish_setup(lpp_engine* e, int64_t n_local, int64_t n_global, int64_t row_start)
{
	e->n_local = n_local;
	e->n_global = n_global;
	e->row_start = row_start;
	e->active = false;
	set_spmv_bytes(e);
	return alloc_work(e);
}

} // namespace lpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

lpp_status lpp_engine_create(lpp_engine** out, const lpp_config* cfg)
{
	if (!out || !cfg) return fail(LPP_ERR_INVALID, "lpp_engine_create: null argument");
	if (cfg->abi_version != LPP_ABI_VERSION) return fail(LPP_ERR_INVALID, "lpp_engine_create: ABI version mismatch");
	if (cfg->dtype != LPP_F64 && cfg->dtype != LPP_C128) return fail(LPP_ERR_INVALID, "lpp_engine_create: bad dtype");
	if (cfg->max_steps < 1) return fail(LPP_ERR_INVALID, "lpp_engine_create: max_steps < 1");
	int ndev = 0;
	hipError_t err = hipGetDeviceCount(&ndev);
	if (err != hipSuccess || ndev <= 0)
		return fail(LPP_ERR_HIP, std::string("lpp_engine_create: no HIP device (there is no CPU fallback): ") + hipGetErrorString(err));
	if (cfg->device < 0 || cfg->device >= ndev) return fail(LPP_ERR_INVALID, "lpp_engine_create: device ordinal out of range");
	HIP_TRY(hipSetDevice(cfg->device));
	lpp_engine* e = new lpp_engine();
	e->cfg = *cfg;
	if (e->cfg.check_lag < 0) e->cfg.check_lag = 0;
	if (e->cfg.check_lag > 16) e->cfg.check_lag = 16;
	e->is_complex = (cfg->dtype == LPP_C128);
	e->esz = e->is_complex ? 16 : 8;
	if (cfg->stream) {
		e->stream = (hipStream_t)cfg->stream;
		e->own_stream = false;
	} else {
		err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
		if (err != hipSuccess) {
			delete e;
			return fail(LPP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(err));
		}
		e->own_stream = true;
	}
	e->spmv_max_blocks = 256 * 16;
	// bit1: XCD-contiguous slice/block map, bit2: 8 slots per batch.  Measured (profiles/README.md): the plain
	// round-robin map is faster for every real-valued workload (4x4 Hubbard 10.8 vs 11.6 ms, matrix-free 4.47 vs
	// 4.70, Heisenberg L=28 1.29 vs 1.36), the XCD-contiguous map for the complex t-J matrix (0.62 vs 0.68).
	e->k2_variant = e->is_complex ? 6 : 4;
	if (const char* s = getenv("LPP_K2_VARIANT")) e->k2_variant = atoi(s);
	{
		int ncu = 0;
		if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0) e->num_cus = ncu;
	}
	if (const char* s = getenv("LPP_SPMV_BLOCKS")) e->spmv_max_blocks = std::max(1, std::min(atoi(s), kMaxPartials));
	const int M = cfg->max_steps + 2;
	e->M = M;
	err = hipMalloc(&e->partial, sizeof(double) * (size_t)kMaxPartials * 2 * kPanel);
	if (err == hipSuccess) err = hipMalloc(&e->scal_own, sizeof(double) * (size_t)(6 * M + 8));
	if (err == hipSuccess) err = hipHostMalloc(&e->h_scal, sizeof(double) * (size_t)(2 * M + 2), hipHostMallocDefault);
	if (err != hipSuccess) {
		lpp_engine_destroy(e);
		return fail(LPP_ERR_NOMEM, std::string("lpp_engine_create: allocation failed: ") + hipGetErrorString(err));
	}
	e->bind_scalars(e->scal_own);
	(void)hipEventCreate(&e->ev_t0);
	(void)hipEventCreate(&e->ev_t1);
	*out = e;
	return LPP_OK;
}

void* lpp_engine_stream(lpp_engine* e) { return e ? (void*)e->stream : nullptr; }

lpp_status lpp_engine_destroy(lpp_engine* e)
{
	if (!e) return LPP_OK;
	(void)hipSetDevice(e->cfg.device);
	if (e->stream) (void)hipStreamSynchronize(e->stream);
	free_csr(e->A_loc);
	free_csr(e->A_rem);
	drop_product(e);
	free_pb(e);
	free_obs(e);
	free_rdm(e);
	for (double* p : { e->x, e->y, e->V, e->partial, e->scal_own, e->zwork })
		if (p) (void)hipFree(p);
	if (e->h_scal) (void)hipHostFree(e->h_scal);
	for (auto& ev : e->step_events)
		if (ev) (void)hipEventDestroy(ev);
	for (auto& pr : e->spmv_events) {
		(void)hipEventDestroy(pr.first);
		(void)hipEventDestroy(pr.second);
	}
	if (e->ev_t0) (void)hipEventDestroy(e->ev_t0);
	if (e->ev_t1) (void)hipEventDestroy(e->ev_t1);
	if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
	delete e;
	return LPP_OK;
}

// A whole matrix (real, or complex Hermitian with a real diagonal) on one GPU that turns out to be of product-basis form (basis block = the caller's hint or the detected one)
// is taken into the product-basis layout (pb_from_csr: T, C, D extracted and the CSR verified against them row by row) and the
// CSR is dropped; *as_product says so.  Everything else goes on to finalize_csr.
static lpp_status try_product_layout(lpp_engine* e, DevCsr& A, bool* as_product)
{
	*as_product = false;
	if (A.nrows == 0 || A.nnz == 0) return LPP_OK;
	const CsrSwitches sw = csr_switches_from_env();
	if (e->hint.kind) { // the caller described the model behind this matrix (lpp_engine_set_model_*): its structured form, if the description is this CSR
		StageTimer tm("structured form from the model description", sw.verbose);
		bool done = false;
		lpp_status st = model_layout_from_hint(e, A, &done);
		e->hint = ModelHint(); // one matrix per description
		if (st != LPP_OK) return st;
		if (done) {
			*as_product = true;
			free_csr(A);
			return LPP_OK;
		}
	}
	int64_t hb = A.hint_block;
	if (hb == 0 && !sw.detect_block.off() && (size_t)A.nrows * e->esz < ((size_t)1 << 32)) {
		StageTimer tm("basis block detection", sw.verbose);
		hb = detect_row_block(e, A, e->esz, (int64_t)1 << 23); // (the product-basis layout holds blocks beyond the LDS window)
		if (hb && sw.verbose) fprintf(stderr, "lpp: detected a basis block of %lld rows\n", (long long)hb);
		if (hb > 0 && hb <= lds_cap_elems(e->esz)) A.hint_block = hb; // finalize_csr need not look again
	}
	if (hb <= 0) return LPP_OK;
	StageTimer tm("product-basis layout from the CSR", sw.verbose);
	lpp_status st = pb_from_csr(e, A, hb, as_product);
	if (st != LPP_OK) return st;
	if (*as_product) free_csr(A);
	return LPP_OK;
}

// rowptr / colind / values: host or device memory, as `kind` says
static lpp_status upload_csr(lpp_engine* e, DevCsr& A, int64_t nrows, int64_t nnz, const int64_t* rowptr, const int32_t* colind, const void* values,
                             hipMemcpyKind kind, int64_t hint_block = 0, bool try_product = false)
{
	const int64_t keep_src = A.src_elems; // (A_rem: set by the caller before the call; A_loc never has one)
	free_csr(A);
	A.src_elems = keep_src;
	A.hint_block = hint_block;
	A.nrows = nrows;
	A.nnz = nnz;
	A.owned = true;
	HIP_TRY_MEM(hipMalloc(&A.rowptr, sizeof(int64_t) * (size_t)(nrows + 1)));
	HIP_TRY_MEM(hipMalloc(&A.col, sizeof(int32_t) * (size_t)std::max<int64_t>(A.nnz, 1)));
	HIP_TRY_MEM(hipMalloc(&A.val, e->esz * (size_t)std::max<int64_t>(A.nnz, 1)));
	HIP_TRY(hipMemcpyAsync(A.rowptr, rowptr, sizeof(int64_t) * (size_t)(nrows + 1), kind, e->stream));
	if (A.nnz > 0) {
		HIP_TRY(hipMemcpyAsync(A.col, colind, sizeof(int32_t) * (size_t)A.nnz, kind, e->stream));
		HIP_TRY(hipMemcpyAsync(A.val, values, e->esz * (size_t)A.nnz, kind, e->stream));
	}
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (try_product) {
		bool as_product = false;
		lpp_status st = try_product_layout(e, A, &as_product);
		if (st != LPP_OK || as_product) return st;
	}
	return finalize_csr(e, A, true);
}

static lpp_status check_csr_host(int64_t nrows, int64_t ncols, const int64_t* rowptr, const int32_t* colind)
{
	if (rowptr[0] != 0) return fail(LPP_ERR_INVALID, "CSR: rowptr[0] != 0");
	for (int64_t i = 0; i < nrows; i++)
		if (rowptr[i + 1] < rowptr[i]) return fail(LPP_ERR_INVALID, "CSR: rowptr not monotone");
	const int64_t nnz = rowptr[nrows];
	for (int64_t p = 0; p < nnz; p++)
		if (colind[p] < 0 || (int64_t)colind[p] >= ncols) return fail(LPP_ERR_INVALID, "CSR: column index out of range");
	return LPP_OK;
}

lpp_status lpp_engine_set_row_block(lpp_engine* e, int64_t rows_per_block)
{
	if (!e || rows_per_block < 0) return fail(LPP_ERR_INVALID, "lpp_engine_set_row_block: bad argument");
	e->row_block_hint = rows_per_block;
	return LPP_OK;
}

lpp_status lpp_engine_set_model_tj(lpp_engine* e, int32_t L, int32_t nup, int32_t ndown, const double* hop_re, const double* hop_im, const double* jpm,
                                   const double* jzz, const double* w, const double* potentialV, int32_t npot)
{
	if (!e) return fail(LPP_ERR_INVALID, "lpp_engine_set_model_tj: null engine");
	e->hint = ModelHint();
	if (L == 0) return LPP_OK; // forget the description
	if (!hop_re || !jpm || !jzz || !w || L < 1 || L > 31 || nup < 0 || ndown < 0 || nup + ndown > L || (potentialV && npot > 0 && npot < 2 * L))
		return fail(LPP_ERR_INVALID, "lpp_engine_set_model_tj: bad argument");
	e->hint.tj = tj_model_from_args(L, nup, ndown, hop_re, hop_im, jpm, jzz, w, potentialV, npot);
	e->hint.kind = 1;
	return LPP_OK;
}

lpp_status lpp_engine_set_model_heisenberg(lpp_engine* e, int32_t L, int32_t szPlusConst, const double* jpm, const double* jzz, const double* field, int32_t nfield)
{
	if (!e) return fail(LPP_ERR_INVALID, "lpp_engine_set_model_heisenberg: null engine");
	e->hint = ModelHint();
	if (L == 0) return LPP_OK;
	if (!jpm || !jzz || L < 1 || L > 62 || szPlusConst < 0 || szPlusConst > L || (nfield > 0 && !field)) return fail(LPP_ERR_INVALID, "lpp_engine_set_model_heisenberg: bad argument");
	ModelHint& H = e->hint;
	H.L = L;
	H.m = szPlusConst;
	H.nfield = std::max(nfield, 0);
	H.jpm.assign(jpm, jpm + (size_t)L * L);
	H.jzz.assign(jzz, jzz + (size_t)L * L);
	if (nfield > 0) H.field.assign(field, field + nfield);
	H.kind = 2;
	return LPP_OK;
}

lpp_status lpp_engine_set_csr(lpp_engine* e, int64_t nrows, const int64_t* rowptr, const int32_t* colind, const void* values)
{
	if (!e || nrows < 0 || !rowptr) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr: bad argument");
	if (nrows > (int64_t)INT32_MAX) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr: nrows exceeds 32-bit column range");
	if (rowptr[nrows] > 0 && (!colind || !values)) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr: null colind/values");
	lpp_status st = check_csr_host(nrows, nrows, rowptr, colind);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	begin_single_gpu(e);
	st = upload_csr(e, e->A_loc, nrows, rowptr[nrows], rowptr, colind, values, hipMemcpyHostToDevice, e->row_block_hint, true);
	if (st != LPP_OK) return st;
	return finish_setup(e, nrows, nrows, 0);
}

lpp_status lpp_engine_set_csr_device(lpp_engine* e, int64_t nrows, const int64_t* d_rowptr, const int32_t* d_colind, const void* d_values)
{
	if (!e || nrows < 0 || !d_rowptr) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr_device: bad argument");
	if (nrows > (int64_t)INT32_MAX) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr_device: nrows exceeds 32-bit column range");
	HIP_TRY(hipSetDevice(e->cfg.device));
	int64_t nnz = 0;
	HIP_TRY(hipMemcpy(&nnz, d_rowptr + nrows, sizeof(int64_t), hipMemcpyDeviceToHost));
	if (nnz < 0) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr_device: negative rowptr[nrows]");
	if (nnz > 0 && (!d_colind || !d_values)) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr_device: null colind/values");
	// the same structural checks as the host entry point, on the device
	int* bad = nullptr;
	HIP_TRY_MEM(hipMalloc(&bad, sizeof(int)));
	(void)hipMemsetAsync(bad, 0, sizeof(int), e->stream);
	k_check_csr<<<(int)((std::max<int64_t>(nrows, 1) + 255) / 256), 256, 0, e->stream>>>(nrows, nrows, d_rowptr, d_colind, bad);
	int hbad = 0;
	hipError_t e1 = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, e->stream);
	hipError_t e2 = hipStreamSynchronize(e->stream);
	(void)hipFree(bad);
	if (e1 != hipSuccess || e2 != hipSuccess) return fail(LPP_ERR_HIP, "lpp_engine_set_csr_device: validation failed to run");
	if (hbad) return fail(LPP_ERR_INVALID, "CSR: rowptr not monotone from 0 or column index out of range");
	begin_single_gpu(e);
	lpp_status st = upload_csr(e, e->A_loc, nrows, nnz, d_rowptr, d_colind, d_values, hipMemcpyDeviceToDevice, e->row_block_hint, true);
	if (st != LPP_OK) return st;
	return finish_setup(e, nrows, nrows, 0);
}

lpp_status lpp_engine_set_csr_partition(lpp_engine* e, const lpp_comm* comm, int64_t global_rows, const int64_t* shard_starts,
                                        const int64_t* rowptr, const int32_t* colind, const void* values)
{
	if (!e || !comm || !shard_starts || !rowptr) return fail(LPP_ERR_INVALID, "lpp_engine_set_csr_partition: bad argument");
	lpp_status st = e->adopt_comm(comm);
	if (st != LPP_OK) return st;
	const int32_t r = comm->rank, P = comm->nranks;
	if (shard_starts[0] != 0 || shard_starts[P] != global_rows) return fail(LPP_ERR_INVALID, "set_csr_partition: shard_starts must span [0, global_rows]");
	const int64_t local = shard_starts[r + 1] - shard_starts[r];
	st = check_csr_host(local, global_rows, rowptr, colind);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	int64_t nl = 0, nr = 0;
	st = lpp_split_csr(r, P, shard_starts, comm->shard_stride, local, rowptr, colind, values, (int32_t)e->esz, &nl, &nr, nullptr,
	                   nullptr, nullptr, nullptr, nullptr, nullptr);
	if (st != LPP_OK) return st;
	std::vector<int64_t> rpl(local + 1), rpr(local + 1);
	std::vector<int32_t> cl(std::max<int64_t>(nl, 1)), cr(std::max<int64_t>(nr, 1));
	std::vector<char> vl((size_t)std::max<int64_t>(nl, 1) * e->esz), vr((size_t)std::max<int64_t>(nr, 1) * e->esz);
	st = lpp_split_csr(r, P, shard_starts, comm->shard_stride, local, rowptr, colind, values, (int32_t)e->esz, &nl, &nr, rpl.data(),
	                   cl.data(), vl.data(), rpr.data(), cr.data(), vr.data());
	if (st != LPP_OK) return st;
	drop_product(e);
	// the hint survives the partition when this rank's rows start on a block boundary (columns of A_loc are local)
	const int64_t hint = (e->row_block_hint > 0 && shard_starts[r] % e->row_block_hint == 0) ? e->row_block_hint : 0;
	st = upload_csr(e, e->A_loc, local, rpl[local], rpl.data(), cl.data(), vl.data(), hipMemcpyHostToDevice, hint);
	if (st != LPP_OK) return st;
	e->A_rem.src_elems = (int64_t)comm->nranks * comm->shard_stride;
	st = upload_csr(e, e->A_rem, local, rpr[local], rpr.data(), cr.data(), vr.data(), hipMemcpyHostToDevice);
	if (st != LPP_OK) return st;
	return finish_setup(e, local, global_rows, shard_starts[r]);
}

lpp_status lpp_engine_get_csr(lpp_engine* e, int32_t which, int64_t* nrows, int64_t* nnz, int64_t* rowptr, int32_t* colind, void* values)
{
	if (!e) return fail(LPP_ERR_INVALID, "lpp_engine_get_csr: null engine");
	DevCsr& A = which == 0 ? e->A_loc : e->A_rem;
	if (e->tj.active || (e->pb.active && e->pb.chain_model)) {
		// t-J without a stored matrix / a spin chain planned from its couplings: the device assembler runs again, in the reference's order
		const int64_t have = e->tj.active ? e->tj.nnz : e->pb.nnz;
		if (nrows) *nrows = which == 0 ? e->n_local : 0;
		if (nnz) *nnz = which == 0 ? have : 0;
		if (!rowptr && !colind && !values) return LPP_OK;
		if (which != 0) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: no remote part");
		HIP_TRY(hipSetDevice(e->cfg.device));
		DevCsr T;
		const PbState& B = e->pb;
		lpp_status st = e->tj.active ? assemble_tj_raw(e, e->tj.model, T)
		                             : assemble_heisenberg_raw(e, B.chain_L, B.chain_m, B.chain_jpm.data(), B.chain_jzz.data(),
		                                                       B.chain_field.empty() ? nullptr : B.chain_field.data(), B.chain_nfield, T);
		if (st == LPP_OK && T.nnz != have) st = fail(LPP_ERR_HIP, "lpp_engine_get_csr: the regenerated matrix has a different number of entries");
		hipError_t he = hipSuccess;
		if (st == LPP_OK && rowptr) he = hipMemcpy(rowptr, T.rowptr, sizeof(int64_t) * (size_t)(T.nrows + 1), hipMemcpyDeviceToHost);
		if (st == LPP_OK && he == hipSuccess && colind) he = hipMemcpy(colind, T.col, sizeof(int32_t) * (size_t)T.nnz, hipMemcpyDeviceToHost);
		if (st == LPP_OK && he == hipSuccess && values) he = hipMemcpy(values, T.val, e->esz * (size_t)T.nnz, hipMemcpyDeviceToHost);
		free_csr(T);
		if (st != LPP_OK) return st;
		if (he != hipSuccess) return fail(LPP_ERR_HIP, std::string("lpp_engine_get_csr: ") + hipGetErrorString(he));
		return LPP_OK;
	}
	if (e->pb.active) { // product-basis layout: the CSR is regenerated from T, C and the diagonal codes
		if (e->pb.tx) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: not available for the product-basis layout on several GPUs");
		if (nrows) *nrows = which == 0 ? e->n_local : 0;
		if (nnz) *nnz = which == 0 ? e->pb.nnz : 0;
		if (!rowptr && !colind && !values) return LPP_OK;
		if (which != 0) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: no remote part");
		HIP_TRY(hipSetDevice(e->cfg.device));
		return pb_get_csr(e, rowptr, colind, values);
	}
	const int64_t nnz_all = A.nnz + A.out_nnz();
	if (nrows) *nrows = A.nrows;
	if (nnz) *nnz = nnz_all;
	if (!rowptr && !colind && !values) return LPP_OK;
	if (e->kron.active) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: the matrix-free engine stores no CSR");
	if (!A.rowptr) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: no matrix");
	HIP_TRY(hipSetDevice(e->cfg.device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	// plain (col, val) arrays of one stored CSR on the device: the resident ones, or rebuilt from the sliced layout
	auto plain_of = [&](const DevCsr& X, DevBuf& scol, DevBuf& sval, const int32_t*& dcol, const void*& dval) -> lpp_status {
		dcol = X.col;
		dval = X.val;
		if (X.nnz == 0 || (dcol && dval)) return LPP_OK;
		if (!X.sliced) return fail(LPP_ERR_STATE, "lpp_engine_get_csr: matrix arrays missing");
		lpp_status st = rebuild_csr(e, X, scol, sval);
		if (st != LPP_OK) return st;
		dcol = (const int32_t*)scol.p;
		dval = sval.p;
		return LPP_OK;
	};
	if (A.out_part) {
		// split-panel layout: the in-block CSR and the panel-major CSRs of the leaving entries, merged back row by row
		SplitParams P;
		P.nrows = A.nrows;
		P.B = A.split_B;
		P.nb = A.split_nb;
		P.nparts = A.split_parts;
		P.pblk = A.split_pblk;
		DevBuf ic, iv, oc[kSplitMaxParts], ov[kSplitMaxParts], mrp, mc, mv;
		const int32_t* dic = nullptr;
		const void* div = nullptr;
		lpp_status st = plain_of(A, ic, iv, dic, div);
		if (st != LPP_OK) return st;
		SplitOut SO {};
		for (int q = 0; q < A.split_parts; q++) {
			const int32_t* dc = nullptr;
			const void* dv = nullptr;
			if ((st = plain_of(A.out_part[q], oc[q], ov[q], dc, dv)) != LPP_OK) return st;
			SO.rp[q] = A.out_part[q].rowptr;
			SO.col[q] = (int32_t*)dc;
			SO.val[q] = (void*)dv;
		}
		if (mrp.alloc(sizeof(int64_t) * (size_t)(A.nrows + 1)) != hipSuccess || mc.alloc(sizeof(int32_t) * (size_t)nnz_all) != hipSuccess
		    || mv.alloc(e->esz * (size_t)nnz_all) != hipSuccess)
			return fail(LPP_ERR_NOMEM, "lpp_engine_get_csr: scratch allocation failed");
		HIP_TRY(hipMemsetAsync(mrp.p, 0, sizeof(int64_t) * (size_t)(A.nrows + 1), e->stream));
		const int nbk = (int)((A.nrows + 255) / 256);
		k_split_lengths<<<nbk, 256, 0, e->stream>>>(P, A.rowptr, SO, (int64_t*)mrp.p);
		int64_t tot = 0;
		if ((st = scan_exclusive(e, (int64_t*)mrp.p, A.nrows + 1, &tot)) != LPP_OK) return st;
		if (tot != nnz_all) return fail(LPP_ERR_HIP, "lpp_engine_get_csr: split-panel merge lost entries");
		if (e->is_complex)
			k_split_merge<cplx><<<nbk, 256, 0, e->stream>>>(P, A.rowptr, dic, (const cplx*)div, SO, (const int64_t*)mrp.p, (int32_t*)mc.p, (cplx*)mv.p);
		else
			k_split_merge<double><<<nbk, 256, 0, e->stream>>>(P, A.rowptr, dic, (const double*)div, SO, (const int64_t*)mrp.p, (int32_t*)mc.p, (double*)mv.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(e->stream));
		if (rowptr) HIP_TRY(hipMemcpy(rowptr, mrp.p, sizeof(int64_t) * (size_t)(A.nrows + 1), hipMemcpyDeviceToHost));
		if (colind) HIP_TRY(hipMemcpy(colind, mc.p, sizeof(int32_t) * (size_t)nnz_all, hipMemcpyDeviceToHost));
		if (values) HIP_TRY(hipMemcpy(values, mv.p, e->esz * (size_t)nnz_all, hipMemcpyDeviceToHost));
		return LPP_OK;
	}
	if (rowptr) HIP_TRY(hipMemcpy(rowptr, A.rowptr, sizeof(int64_t) * (size_t)(A.nrows + 1), hipMemcpyDeviceToHost));
	if ((colind || values) && A.nnz) {
		DevBuf scol, sval;
		const int32_t* dcol = nullptr;
		const void* dval = nullptr;
		lpp_status st = plain_of(A, scol, sval, dcol, dval);
		if (st != LPP_OK) return st;
		if (colind) HIP_TRY(hipMemcpy(colind, dcol, sizeof(int32_t) * (size_t)A.nnz, hipMemcpyDeviceToHost));
		if (values) HIP_TRY(hipMemcpy(values, dval, e->esz * (size_t)A.nnz, hipMemcpyDeviceToHost));
	}
	return LPP_OK;
}

lpp_status lpp_engine_spmv_acc(lpp_engine* e, void* x_inout, const void* y)
{
	if (!e || !x_inout || !y) return fail(LPP_ERR_INVALID, "lpp_engine_spmv_acc: null argument");
	if (!e->has_matrix()) return fail(LPP_ERR_STATE, "lpp_engine_spmv_acc: no matrix (call lpp_engine_set_csr first)");
	if (e->has_comm && e->comm.nranks > 1) return fail(LPP_ERR_STATE, "lpp_engine_spmv_acc: not available on a partitioned matrix");
	if (e->active) return fail(LPP_ERR_STATE, "lpp_engine_spmv_acc: a Lanczos run is active");
	if (e->pb.active && e->pb.tx) return fail(LPP_ERR_STATE, "lpp_engine_spmv_acc: a row slice alone has no product (several GPUs: use the Lanczos entry points)");
	HIP_TRY(hipSetDevice(e->cfg.device));
	lpp_status st = vec_from_host(e, e->x, x_inout);
	if (st != LPP_OK) return st;
	if ((st = vec_from_host(e, e->y, y)) != LPP_OK) return st;
	if (e->pb.active)
		pb_launch(e, e->y, e->x, nullptr);
	else if (e->kron.active)
		kron_launch(e, e->y, e->y, e->x, nullptr);
	else
		spmv_launch(e, e->A_loc, e->y, e->x, nullptr, nullptr);
	HIP_TRY(hipGetLastError());
	if ((st = vec_to_host(e, x_inout, e->x)) != LPP_OK) return st;
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status lpp_engine_bench_spmv(lpp_engine* e, int32_t warmup, int32_t iters, double* ms_per_launch)
{
	if (!e || iters <= 0 || !ms_per_launch) return fail(LPP_ERR_INVALID, "lpp_engine_bench_spmv: bad argument");
	if (!e->has_matrix()) return fail(LPP_ERR_STATE, "lpp_engine_bench_spmv: no matrix");
	if (e->active) return fail(LPP_ERR_STATE, "lpp_engine_bench_spmv: a Lanczos run is active");
	if (e->has_comm && e->comm.nranks > 1 && e->tx) return fail(LPP_ERR_STATE, "lpp_engine_bench_spmv: not available with the transposition exchange");
	HIP_TRY(hipSetDevice(e->cfg.device));
	vec_fill_random(e, e->y, 99);
	HIP_TRY(hipMemsetAsync(e->x, 0, sizeof(double) * (size_t)e->nd_pad, e->stream));
	const void* src = e->y;
	if (e->has_comm && e->comm.nranks > 1) {
		// bench the two local kernels against a synthetic gathered vector (no collective in the loop)
		k_fill_random<<<1024, 256, 0, e->stream>>>((double*)e->comm.gath_buf, e->comm.shard_stride * e->comm.nranks * (e->is_complex ? 2 : 1), 0, 98);
	}
	for (int i = 0; i < warmup + iters; i++) {
		if (i == warmup) HIP_TRY(hipEventRecord(e->ev_t0, e->stream));
		if (e->pb.active) {
			pb_launch(e, e->y, e->x, e->partial);
			continue;
		}
		if (e->kron.active) {
			kron_launch(e, e->y, (e->has_comm && e->comm.nranks > 1) ? e->comm.gath_buf : e->y, e->x, e->partial);
			continue;
		}
		spmv_launch(e, e->A_loc, src, e->x, e->y, e->A_rem.nnz ? nullptr : e->partial);
		if (e->A_rem.nnz) spmv_launch(e, e->A_rem, e->comm.gath_buf, e->x, e->y, e->partial);
	}
	HIP_TRY(hipEventRecord(e->ev_t1, e->stream));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventSynchronize(e->ev_t1));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e->ev_t0, e->ev_t1));
	*ms_per_launch = (double)ms / iters;
	HIP_TRY(hipMemsetAsync(e->x, 0, sizeof(double) * (size_t)e->nd_pad, e->stream));
	HIP_TRY(hipMemsetAsync(e->y, 0, sizeof(double) * (size_t)e->nd_pad, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status lpp_engine_sync(lpp_engine* e)
{
	if (!e) return fail(LPP_ERR_INVALID, "lpp_engine_sync: null engine");
	HIP_TRY(hipSetDevice(e->cfg.device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status lpp_engine_get_layout(lpp_engine* e, int32_t which, lpp_layout* out)
{
	if (!e || !out || which < 0 || which > 1) return fail(LPP_ERR_INVALID, "lpp_engine_get_layout: bad argument");
	if (e->kron.active) return fail(LPP_ERR_STATE, "lpp_engine_get_layout: the matrix-free engine stores no CSR");
	const DevCsr& A = which == 0 ? e->A_loc : e->A_rem;
	const size_t s = e->esz;
	lpp_layout L {};
	if (e->tj.active && which == 0) {
		const TjState& S = e->tj;
		L.kernel = LPP_SPMV_HOLE_MAJOR;
		L.nnz = S.nnz;
		L.rows_per_block = S.ns;
		L.pieces = 1;
		L.diagonal_plain = 1;
		// the tables (L2 / LDS resident during a product), one f64 of diagonal per stored position, the boundary's permutation
		L.resident_bytes = S.table_bytes + (int64_t)sizeof(double) * S.nblk * S.pitch + (int64_t)sizeof(int32_t) * S.nblk * S.ns;
		L.stream_bytes = (int64_t)sizeof(double) * S.nblk * S.pitch;
		*out = L;
		return LPP_OK;
	}
	if (e->pb.active && which == 0) {
		const PbState& B = e->pb;
		L.kernel = LPP_SPMV_PRODUCT;
		L.coded = 1;
		L.local16 = 1;
		L.block_template = 2;
		L.diagonal_codes = B.dval ? 0 : 1;
		L.shared_stride = B.rowcap;
		L.nnz = B.nnz;
		L.per_row_entries = B.t_entries * B.n_blk; // in-block entries, stored once (the template)
		L.shared_entries = B.c_nnz; // block couplings, stored once per block
		L.rows_per_block = B.n_up;
		L.pieces = B.npieces;
		L.coupling_parts = B.parts ? B.nparts : 1;
		L.chained_step = pb_chain_ok(e) ? 1 : 0;
		L.rows_by_list_length = e->pb.perm && !B.seg ? 1 : 0;
		L.segments = B.seg ? B.seg_nsegs : 0;
		L.coupling_rounds = B.c_nnz > 0 && !B.parts ? B.down_rounds : 1;
		L.diagonal_plain = B.dval ? 1 : 0;
		const size_t small = sizeof(uint32_t) * (size_t)B.f_words + sizeof(uint32_t) * (size_t)B.tw_words + (sizeof(int32_t) + sizeof(uint16_t)) * (size_t)B.spb * (size_t)B.G
		    + (size_t)B.seg_bytes + (size_t)B.t_entries * 12 + (B.chain_model ? 0 : sizeof(int64_t) * (size_t)(B.n_up + 1)) + (size_t)B.c_nnz * 5 + sizeof(int64_t) * 2 * (size_t)(B.n_blk + 1) + 256 * sizeof(double);
		// one diagonal code per row this rank holds, or one plain double when the diagonal has more than 256 distinct values
		const size_t codes = (size_t)(B.tx ? B.nblk_loc : B.n_blk) * (size_t)B.pitch * (B.dval ? 9 : 1);
		L.resident_bytes = (int64_t)(small + codes);
		// per product: one diagonal code per row; the template words and the couplings are re-read from L2 / LDS
		L.stream_bytes = (int64_t)(codes + sizeof(uint32_t) * (size_t)(B.tw_words + B.f_words) + (size_t)B.seg_bytes + (size_t)B.c_nnz * 5);
		*out = L;
		return LPP_OK;
	}
	L.kernel = A.sliced ? (A.window ? LPP_SPMV_WINDOW : LPP_SPMV_SLICED) : LPP_SPMV_ROWGROUP;
	L.coded = A.coded ? 1 : 0;
	L.local16 = A.local16 ? 1 : 0;
	L.block_template = A.tmpl;
	L.diagonal_codes = A.dcode ? 1 : 0;
	L.shared_stride = A.dia_stride;
	L.nnz = A.nnz;
	L.per_row_entries = A.rrowptr ? A.rnnz : A.nnz;
	L.shared_entries = A.ndia;
	L.rows_per_block = A.sliced ? A.geom.B : 0;
	size_t bytes = A.rowptr ? sizeof(int64_t) * (size_t)(A.nrows + 1) : 0;
	size_t stream = 0; // what one product must read of the matrix (see lpp_layout::stream_bytes)
	if (A.col) bytes += sizeof(int32_t) * (size_t)A.nnz;
	if (A.val) bytes += s * (size_t)A.nnz;
	if (A.sliced) { // the arrays build_sliced allocated (lpp_csr_plan.h)
		const SlicedSizes z = sliced_sizes(sliced_shape(A, s));
		bytes += z.resident_bytes();
		stream += z.stream_bytes();
	} else {
		stream = bytes; // row-group kernel: row pointers, columns and values are all read
	}
	if (A.out_part) { // split-panel layout: the leaving entries as further (sliced, panel-major) matrices + the row map
		for (int q = 0; q < A.split_parts; q++) {
			const DevCsr& O = A.out_part[q];
			const SlicedSizes z = sliced_sizes(sliced_shape(O, s));
			const size_t b = z.structure() + z.values() + sizeof(int32_t) * (size_t)O.nrows; // + its share of the row map
			stream += b;
			bytes += b + sizeof(int64_t) * (size_t)(O.nrows + 1);
			L.nnz += O.nnz;
			L.per_row_entries += O.nnz;
		}
		L.split_panel = A.split_parts;
	}
	L.stream_bytes = (int64_t)stream;
	L.resident_bytes = (int64_t)bytes;
	*out = L;
	return LPP_OK;
}

lpp_status lpp_engine_get_stats(lpp_engine* e, lpp_stats* s)
{
	if (!e || !s) return fail(LPP_ERR_INVALID, "lpp_engine_get_stats: null argument");
	e->collect_spmv_times();
	*s = e->stats;
	s->nrows = e->n_local;
	s->nnz = e->tj.active ? e->tj.nnz : e->pb.active ? e->pb.nnz_loc : (e->kron.active ? (int64_t)e->kron.equiv_nnz : e->A_loc.nnz + e->A_loc.out_nnz() + e->A_rem.nnz);
	s->spmv_bytes = e->spmv_bytes;
	return LPP_OK;
}

} // extern "C"
