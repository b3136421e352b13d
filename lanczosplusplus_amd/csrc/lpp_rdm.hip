// lpp_rdm.hip -- the reduced density matrix of the lattice cut at a site (reference src/Engine/ReducedDensityMatrix.h, called from
// LanczosDriver1.h:201-206 for `-r siteForSplit`) on one GPU, for the two bases the reference supports there: BasisHubbardLanczos and the
// S = 1/2 words of BasisHeisenberg (:78-88).
//
// Host part (no GPU): the plan -- the classes (k_up, k_down) of particle numbers in the low `split` sites, the packed layout of the block
// diagonal result, the alpha word of every row, the run-start ranks of every environment configuration -- and the cut of the work into
// tiles and K ranges.  Device part: the launches of lpp_rdm_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "lpp_engine_impl.h"
#include "lpp_rdm_kernels.h"

using namespace lpp;

namespace {

int64_t binom(int n, int k)
{
	if (k < 0 || k > n) return 0;
	long double r = 1;
	for (int i = 1; i <= k; i++) r = r * (n - k + i) / i;
	return (int64_t)(r + 0.5L);
}

// the next word of the same popcount (BasisOneSpin.h:53-61); w != 0
inline uint64_t next_word(uint64_t w)
{
	const uint64_t c = w & (~w + 1), r = w + c;
	return (((r ^ w) >> 2) / c) | r;
}

// the words of `bits` bits with `n` set, ascending
void words_of(int bits, int n, std::vector<uint64_t>& out)
{
	const int64_t cnt = binom(bits, n);
	out.resize((size_t)cnt);
	uint64_t w = (n == 0) ? 0 : ((1ull << n) - 1);
	for (int64_t i = 0; i < cnt; i++) {
		out[(size_t)i] = w;
		if (n > 0 && i + 1 < cnt) w = next_word(w);
	}
}

// BasisOneSpin::perfectIndex (BasisOneSpin.h:73-81)
int64_t rank_of(uint64_t w)
{
	int64_t n = 0;
	int c = 1;
	for (int b = 0; w; b++, w >>= 1)
		if (w & 1) n += binom(b, c++);
	return n;
}

struct Species {
	int n = 0, kmin = 0, kmax = -1; // particles, classes
	int64_t size = 1; // states of the species
	std::vector<int64_t> start_off; // per class, offset into starts
	std::vector<int32_t> starts; // per class, per environment configuration t ascending: the rank of (t << split | lowest low word)
};

struct RdmBlock {
	int k_up = 0, k_dn = 0;
	int64_t du = 0, dd = 0, eu = 0, ed = 0, off = 0;
};

struct RdmPlan {
	int basis = 0, L = 0, nup = 0, ndn = 0, split = 0;
	Species up, dn;
	std::vector<RdmBlock> blocks;
	int64_t total = 0, rows = 0, states = 0; // packed elements, sum of d, N
	double total_f = 0; // the packed element count in floating point: it may exceed 2^63
};

void plan_species(int L, int split, int n, Species& S, bool with_starts)
{
	S.n = n;
	S.size = binom(L, n);
	S.kmin = std::max(0, n - (L - split));
	S.kmax = std::min(split, n);
	S.start_off.clear();
	S.starts.clear();
	int64_t off = 0;
	for (int k = S.kmin; k <= S.kmax; k++) {
		S.start_off.push_back(off);
		off += binom(L - split, n - k);
	}
	if (!with_starts) return;
	S.starts.reserve((size_t)off);
	std::vector<uint64_t> t;
	for (int k = S.kmin; k <= S.kmax; k++) {
		words_of(L - split, n - k, t);
		const uint64_t low = (k == 0) ? 0 : ((1ull << k) - 1);
		for (uint64_t hi : t) S.starts.push_back((int32_t)rank_of((hi << split) | low));
	}
}

lpp_status rdm_plan(int basis, int L, int nup, int ndn, int split, bool with_starts, RdmPlan& P)
{
	if (basis != LPP_BASIS_HUBBARD && basis != LPP_BASIS_SPIN_HALF) return fail(LPP_ERR_INVALID, "reduced density matrix: basis must be LPP_BASIS_HUBBARD or LPP_BASIS_SPIN_HALF");
	if (L < 1 || L > 40) return fail(LPP_ERR_INVALID, "reduced density matrix: 1 to 40 sites");
	if (split < 0 || split > L) return fail(LPP_ERR_INVALID, "reduced density matrix: the split site must lie in 0 .. sites");
	if (basis == LPP_BASIS_SPIN_HALF) ndn = 0; // one species: the down word is empty
	if (nup < 0 || nup > L || ndn < 0 || ndn > L) return fail(LPP_ERR_INVALID, "reduced density matrix: impossible sector");
	if (binom(L, nup) >= (int64_t)INT32_MAX - 4096 || binom(L, ndn) >= (int64_t)INT32_MAX - 4096)
		return fail(LPP_ERR_INVALID, "reduced density matrix: a species with 2^31 states or more");
	P = RdmPlan();
	P.basis = basis;
	P.L = L;
	P.nup = nup;
	P.ndn = ndn;
	P.split = split;
	plan_species(L, split, nup, P.up, with_starts);
	plan_species(L, split, ndn, P.dn, with_starts);
	P.states = P.up.size * P.dn.size;
	for (int kd = P.dn.kmin; kd <= P.dn.kmax; kd++)
		for (int ku = P.up.kmin; ku <= P.up.kmax; ku++) {
			RdmBlock B;
			B.k_up = ku;
			B.k_dn = kd;
			B.du = binom(split, ku);
			B.dd = binom(split, kd);
			B.eu = binom(L - split, nup - ku);
			B.ed = binom(L - split, ndn - kd);
			B.off = P.total;
			const int64_t d = B.du * B.dd;
			P.total_f += (double)d * (double)d;
			P.total = (P.total_f < 4e18) ? P.total + d * d : INT64_MAX;
			P.rows += d;
			P.blocks.push_back(B);
		}
	return LPP_OK;
}

// ---- the cut into work items ---------------------------------------------------------------------------------------------------------------
// A block of T x T tiles has T (T + 1) / 2 stored tiles.  Where those are fewer than kFillTiles the K range is cut into S ranges of equal
// length (a multiple of the panel, at least kMinRange columns) so that the block has about kFillTiles work items; the partial tiles of all such
// blocks together are held to kMaxPartials by scaling every S down.  All of it is a function of the sector: the sums have one fixed order.
constexpr int64_t kFillTiles = 256, kMinRange = 64, kMaxPartials = 8192;

struct Cut {
	std::vector<RdmItem> items, reds;
	int64_t partials = 0; // 64 x 64 partial tiles in the workspace
};

int64_t tiles_of(int64_t d)
{
	const int64_t T = (d + kRdmTile - 1) / kRdmTile;
	return T * (T + 1) / 2;
}

void splits_of(const RdmPlan& P, std::vector<int64_t>& S, std::vector<int64_t>& len)
{
	const size_t nb = P.blocks.size();
	S.assign(nb, 1);
	len.assign(nb, 0);
	int64_t partials = 0;
	for (size_t b = 0; b < nb; b++) {
		const RdmBlock& B = P.blocks[b];
		const int64_t K = B.eu * B.ed, nt = tiles_of(B.du * B.dd);
		if (nt < kFillTiles) S[b] = std::max<int64_t>(1, std::min((K + kMinRange - 1) / kMinRange, (kFillTiles + nt - 1) / nt));
		if (S[b] > 1) partials += S[b] * nt;
	}
	for (size_t b = 0; b < nb; b++) {
		const RdmBlock& B = P.blocks[b];
		const int64_t K = B.eu * B.ed;
		if (S[b] > 1 && partials > kMaxPartials) S[b] = std::max<int64_t>(1, S[b] * kMaxPartials / partials);
		int64_t l = (K + S[b] - 1) / S[b];
		l = (l + kRdmPanel - 1) / kRdmPanel * kRdmPanel;
		len[b] = l;
		S[b] = (K + l - 1) / l;
	}
}

// the number of work items and partial tiles, without building them
void cut_sizes(const RdmPlan& P, int64_t* nitems, int64_t* partials)
{
	std::vector<int64_t> S, len;
	splits_of(P, S, len);
	*nitems = *partials = 0;
	for (size_t b = 0; b < P.blocks.size(); b++) {
		const int64_t nt = tiles_of(P.blocks[b].du * P.blocks[b].dd);
		*nitems += nt * S[b];
		if (S[b] > 1) *partials += nt * S[b];
	}
}

void cut_work(const RdmPlan& P, Cut& C)
{
	std::vector<int64_t> S, len;
	splits_of(P, S, len);
	C = Cut();
	for (size_t b = 0; b < P.blocks.size(); b++) {
		const RdmBlock& B = P.blocks[b];
		const int64_t K = B.eu * B.ed, T = (B.du * B.dd + kRdmTile - 1) / kRdmTile;
		for (int64_t ti = 0; ti < T; ti++)
			for (int64_t tj = 0; tj <= ti; tj++) {
				if (S[b] > 1) C.reds.push_back(RdmItem { (int32_t)b, (int32_t)ti, (int32_t)tj, (int32_t)S[b], 0, K, C.partials });
				for (int64_t s = 0; s < S[b]; s++) {
					RdmItem it { (int32_t)b, (int32_t)ti, (int32_t)tj, (int32_t)S[b], s * len[b], std::min(K, (s + 1) * len[b]), -1 };
					if (S[b] > 1) it.ws = C.partials++;
					C.items.push_back(it);
				}
			}
	}
}

// ---- device side -----------------------------------------------------------------------------------------------------------------------------
struct RdmDev {
	RdmPlan plan;
	int64_t nitems = 0, nreds = 0, partials = 0;
	RdmBlockDev* blocks = nullptr;
	RdmItem *items = nullptr, *reds = nullptr;
	int32_t *su = nullptr, *sd = nullptr;
	double* ws = nullptr;
	void release()
	{
		for (void* p : { (void*)blocks, (void*)items, (void*)reds, (void*)su, (void*)sd, (void*)ws })
			if (p) (void)hipFree(p);
		blocks = nullptr;
		items = reds = nullptr;
		su = sd = nullptr;
		ws = nullptr;
		nitems = nreds = partials = 0;
		plan = RdmPlan();
	}
};

inline bool multi(const lpp_engine* e) { return e->has_comm && e->comm.nranks > 1; }

lpp_status refuse(const lpp_engine* e, const char* who)
{
	if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
	if (e->tj.active) return fail(LPP_ERR_STATE, std::string(who) + ": not on a hole-major t-J engine");
	return LPP_OK;
}

template <typename T> hipError_t upload(T** dst, const std::vector<T>& src)
{
	hipError_t err = hipMalloc((void**)dst, std::max<size_t>(sizeof(T) * src.size(), 16));
	if (err == hipSuccess && !src.empty()) err = hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
	return err;
}

// Everything a launch needs, checked and uploaded; kept with the engine for the next call on the same (basis, sites, sector, split).
// result_allocated: the caller holds the packed result already, so only the workspace has to fit.  Nothing is launched.
lpp_status get_rdm(lpp_engine* e, int basis, int L, int nup, int ndn, int split, bool result_allocated, const char* who, RdmDev** out)
{
	RdmPlan P;
	lpp_status st = rdm_plan(basis, L, nup, ndn, split, false, P);
	if (st != LPP_OK) return st;
	RdmDev* D = (RdmDev*)e->rdm;
	const bool cached = D && D->blocks && D->plan.basis == P.basis && D->plan.L == L && D->plan.nup == P.nup && D->plan.ndn == P.ndn && D->plan.split == split;
	int64_t nitems = 0, partials = 0;
	cut_sizes(P, &nitems, &partials);
	const double W = e->is_complex ? 2.0 : 1.0;
	const double out_bytes = 8.0 * W * P.total_f, ws_bytes = 8.0 * W * (double)partials * kRdmTileElems;
	const double tab_bytes = (double)nitems * sizeof(RdmItem) * 1.5 + 4.0 * ((double)P.up.start_off.size() + (double)P.dn.start_off.size()) + 4.0 * (double)(1ll << std::min(L - split, 30)) * 2;
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	const double need = (result_allocated ? 0.0 : out_bytes) + (cached ? 0.0 : ws_bytes + tab_bytes);
	if (need > 0.95 * (double)free_b || nitems >= (int64_t)INT32_MAX || P.total == INT64_MAX) {
		char msg[320];
		snprintf(msg, sizeof msg, "%s: the packed result (%.0f bytes, %.0f elements in %zu blocks) plus workspace (%.0f bytes) does not fit in the free device memory (%zu bytes)", who,
		         out_bytes, P.total_f, P.blocks.size(), ws_bytes + tab_bytes, free_b);
		return fail(LPP_ERR_NOMEM, msg);
	}
	if (cached) {
		*out = D;
		return LPP_OK;
	}
	if (!D) e->rdm = D = new RdmDev();
	HIP_TRY(hipStreamSynchronize(e->stream)); // launches that still read the previous plan
	D->release();
	st = rdm_plan(basis, L, nup, ndn, split, true, P);
	if (st != LPP_OK) return st;
	Cut C;
	cut_work(P, C);
	std::vector<RdmBlockDev> bd(P.blocks.size());
	for (size_t b = 0; b < bd.size(); b++) {
		const RdmBlock& B = P.blocks[b];
		bd[b] = RdmBlockDev { B.off, (int32_t)(B.du * B.dd), (int32_t)B.du, (int32_t)B.eu, (int32_t)P.up.start_off[(size_t)(B.k_up - P.up.kmin)],
			                  (int32_t)P.dn.start_off[(size_t)(B.k_dn - P.dn.kmin)], 0 };
	}
	hipError_t err = upload(&D->blocks, bd);
	if (err == hipSuccess) err = upload(&D->items, C.items);
	if (err == hipSuccess) err = upload(&D->reds, C.reds);
	if (err == hipSuccess) err = upload(&D->su, P.up.starts);
	if (err == hipSuccess) err = upload(&D->sd, P.dn.starts);
	if (err == hipSuccess) err = hipMalloc((void**)&D->ws, std::max<size_t>((size_t)ws_bytes, 16));
	if (err != hipSuccess) {
		D->release();
		if (err == hipErrorOutOfMemory) {
			(void)hipGetLastError();
			return fail(LPP_ERR_NOMEM, std::string(who) + ": no device memory for the plan and the workspace");
		}
		HIP_TRY(err);
	}
	D->nitems = (int64_t)C.items.size();
	D->nreds = (int64_t)C.reds.size();
	D->partials = C.partials;
	P.up.starts = std::vector<int32_t>();
	P.dn.starts = std::vector<int32_t>();
	D->plan = P;
	*out = D;
	return LPP_OK;
}

lpp_status launch_rdm(lpp_engine* e, const RdmDev* D, const void* d_psi, void* d_out)
{
	RdmArgs A { (const double*)d_psi, D->plan.up.size, D->blocks, D->items, D->su, D->sd, (double*)d_out, D->ws };
	if (D->nitems > 0) {
		if (e->is_complex) k_rdm_tiles<true><<<(int)D->nitems, kRdmBlock, 0, e->stream>>>(A);
		else k_rdm_tiles<false><<<(int)D->nitems, kRdmBlock, 0, e->stream>>>(A);
	}
	if (D->nreds > 0) {
		if (e->is_complex) k_rdm_reduce<true><<<(int)D->nreds, kRdmBlock, 0, e->stream>>>(A, D->reds);
		else k_rdm_reduce<false><<<(int)D->nreds, kRdmBlock, 0, e->stream>>>(A, D->reds);
	}
	HIP_TRY(hipGetLastError());
	return LPP_OK;
}

// device vector -> host result through a result buffer of this call; out == nullptr: every check, no launch
lpp_status rdm_to_host(lpp_engine* e, int basis, int L, int nup, int ndn, int split, const void* d_psi, void* out, const char* who)
{
	RdmDev* D = nullptr;
	lpp_status st = get_rdm(e, basis, L, nup, ndn, split, false, who, &D);
	if (st != LPP_OK || !out) return st;
	const size_t bytes = e->esz * (size_t)D->plan.total;
	DevBuf r;
	HIP_TRY_MEM(hipMalloc(&r.p, std::max<size_t>(bytes, 16)));
	if ((st = launch_rdm(e, D, d_psi, r.p)) != LPP_OK) return st;
	HIP_TRY(hipMemcpyAsync(out, r.p, bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

} // namespace

namespace lpp {
void free_rdm(lpp_engine* e)
{
	if (!e->rdm) return;
	RdmDev* D = (RdmDev*)e->rdm;
	D->release();
	delete D;
	e->rdm = nullptr;
}
} // namespace lpp

extern "C" {

lpp_status lpp_rdm_plan(int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, int32_t* nblocks, int64_t* total, int64_t* nrows, int64_t* nstarts_up,
                        int64_t* nstarts_down, lpp_rdm_block* blocks, int64_t* alpha, int64_t* starts_up, int64_t* starts_down)
{
	RdmPlan P;
	const bool tables = starts_up || starts_down;
	lpp_status st = rdm_plan(basis, nsites, nup, ndown, split, tables, P);
	if (st != LPP_OK) return st;
	if (P.total == INT64_MAX) return fail(LPP_ERR_INVALID, "lpp_rdm_plan: the packed result has 2^62 elements or more");
	if (nblocks) *nblocks = (int32_t)P.blocks.size();
	if (total) *total = P.total;
	if (nrows) *nrows = P.rows;
	if (nstarts_up) *nstarts_up = P.up.start_off.back() + binom(nsites - split, P.nup - P.up.kmax);
	if (nstarts_down) *nstarts_down = P.dn.start_off.back() + binom(nsites - split, P.ndn - P.dn.kmax);
	if (blocks)
		for (size_t b = 0; b < P.blocks.size(); b++) {
			const RdmBlock& B = P.blocks[b];
			blocks[b] = lpp_rdm_block { B.k_up, B.k_dn, B.du, B.dd, B.eu, B.ed, B.off };
		}
	if (alpha) {
		std::vector<uint64_t> wu, wd;
		int64_t r = 0;
		for (const RdmBlock& B : P.blocks) {
			words_of(split, B.k_up, wu);
			words_of(split, B.k_dn, wd);
			for (uint64_t d : wd)
				for (uint64_t u : wu) alpha[r++] = (int64_t)(u + (d << split));
		}
	}
	if (starts_up) std::copy(P.up.starts.begin(), P.up.starts.end(), starts_up);
	if (starts_down) std::copy(P.dn.starts.begin(), P.dn.starts.end(), starts_down);
	return LPP_OK;
}

lpp_status lpp_engine_reduced_density_matrix(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, const void* d_psi, void* d_out)
{
	if (!e || !d_psi || !d_out) return fail(LPP_ERR_INVALID, "lpp_engine_reduced_density_matrix: null argument");
	lpp_status st = refuse(e, "lpp_engine_reduced_density_matrix");
	if (st != LPP_OK) return st;
	if (((uintptr_t)d_psi & 15) != 0 || ((uintptr_t)d_out & 15) != 0) return fail(LPP_ERR_INVALID, "lpp_engine_reduced_density_matrix: the vector and the result must be 16-byte aligned");
	HIP_TRY(hipSetDevice(e->cfg.device));
	RdmDev* D = nullptr;
	if ((st = get_rdm(e, basis, nsites, nup, ndown, split, true, "lpp_engine_reduced_density_matrix", &D)) != LPP_OK) return st;
	return launch_rdm(e, D, d_psi, d_out);
}

lpp_status lpp_engine_reduced_density_matrix_host(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, const void* psi, void* out)
{
	if (!e || (out && !psi)) return fail(LPP_ERR_INVALID, "lpp_engine_reduced_density_matrix_host: null argument");
	lpp_status st = refuse(e, "lpp_engine_reduced_density_matrix_host");
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	if (!out) return rdm_to_host(e, basis, nsites, nup, ndown, split, nullptr, nullptr, "lpp_engine_reduced_density_matrix_host");
	RdmPlan P;
	if ((st = rdm_plan(basis, nsites, nup, ndown, split, false, P)) != LPP_OK) return st;
	const size_t bytes = e->esz * (size_t)P.states;
	DevBuf v;
	HIP_TRY_MEM(hipMalloc(&v.p, std::max<size_t>(bytes, 16)));
	HIP_TRY(hipMemcpyAsync(v.p, psi, bytes, hipMemcpyHostToDevice, e->stream));
	return rdm_to_host(e, basis, nsites, nup, ndown, split, v.p, out, "lpp_engine_reduced_density_matrix_host");
}

lpp_status lpp_engine_state_reduced_density_matrix(lpp_engine* e, int32_t state, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, void* out_host)
{
	if (!e) return fail(LPP_ERR_INVALID, "lpp_engine_state_reduced_density_matrix: null argument");
	lpp_status st = refuse(e, "lpp_engine_state_reduced_density_matrix");
	if (st != LPP_OK) return st;
	if (state < 0 || state >= e->resident_n || !e->resident)
		return fail(LPP_ERR_STATE, "lpp_engine_state_reduced_density_matrix: no such resident state (lpp_engine_keep_states before lpp_engine_lanczos)");
	RdmPlan P;
	if ((st = rdm_plan(basis, nsites, nup, ndown, split, false, P)) != LPP_OK) return st;
	if (e->resident_len != P.states) return fail(LPP_ERR_INVALID, "lpp_engine_state_reduced_density_matrix: (basis, sites, nup, ndown) is not the sector of the resident states");
	HIP_TRY(hipSetDevice(e->cfg.device));
	return rdm_to_host(e, basis, nsites, nup, ndown, split, e->resident + (int64_t)state * e->resident_stride, out_host, "lpp_engine_state_reduced_density_matrix");
}

lpp_status lpp_engine_bench_rdm(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, int32_t warmup, int32_t iters, double* ms_per_call,
                                double* macs)
{
	if (!e || !ms_per_call || iters < 1 || warmup < 0) return fail(LPP_ERR_INVALID, "lpp_engine_bench_rdm: bad argument");
	lpp_status st = refuse(e, "lpp_engine_bench_rdm");
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	RdmDev* D = nullptr;
	if ((st = get_rdm(e, basis, nsites, nup, ndown, split, false, "lpp_engine_bench_rdm", &D)) != LPP_OK) return st;
	const int64_t n = D->plan.states, nd = n * (e->is_complex ? 2 : 1);
	DevBuf v, r;
	HIP_TRY_MEM(hipMalloc(&v.p, std::max<size_t>(sizeof(double) * (size_t)nd, 16)));
	HIP_TRY_MEM(hipMalloc(&r.p, std::max<size_t>(e->esz * (size_t)D->plan.total, 16)));
	{
		// pseudo-random entries in (-0.5, 0.5) / sqrt(N): a vector of norm about 0.29 (splitmix64 of the index)
		std::vector<double> h((size_t)nd);
		const double scale = 1.0 / std::sqrt((double)std::max<int64_t>(n, 1));
		for (int64_t i = 0; i < nd; i++) {
			uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x1234;
			z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
			z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
			z ^= z >> 31;
			h[(size_t)i] = ((double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5) * scale;
		}
		HIP_TRY(hipMemcpy(v.p, h.data(), sizeof(double) * (size_t)nd, hipMemcpyHostToDevice));
	}
	hipEvent_t t0 = nullptr, t1 = nullptr;
	HIP_TRY(hipEventCreate(&t0));
	HIP_TRY(hipEventCreate(&t1));
	for (int i = 0; i < warmup + iters && st == LPP_OK; i++) {
		if (i == warmup) (void)hipEventRecord(t0, e->stream);
		st = launch_rdm(e, D, v.p, r.p);
	}
	(void)hipEventRecord(t1, e->stream);
	hipError_t err = hipEventSynchronize(t1);
	float ms = 0;
	if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
	(void)hipEventDestroy(t0);
	(void)hipEventDestroy(t1);
	if (st != LPP_OK) return st;
	HIP_TRY(err);
	*ms_per_call = ms / iters;
	if (macs) {
		double m = 0;
		for (const RdmBlock& B : D->plan.blocks) m += (double)(B.du * B.dd) * (double)(B.du * B.dd) * (double)(B.eu * B.ed);
		*macs = m * (e->is_complex ? 4.0 : 1.0);
	}
	return LPP_OK;
}

} // extern "C"
