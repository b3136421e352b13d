// lpp_obs.hip -- ground-state observables of the Hubbard product basis, of the one-orbital t-J basis, of the S = 1/2 Heisenberg basis and of the spin-S
// Heisenberg digit basis on one GPU:
// one-site operators applied to device vectors (Engine::accModifiedState_, reference src/Engine/Engine.h:416-458), the two-point matrix
// (Engine::twoPoint :266-338), the modified state + decomposition of one spectral-function type (Engine::spectralFunction :134-206, getModifiedState
// :494-533, calcSpectral :460-490), operator strings (Engine::manyPoint :341-389) and the continued-fraction evaluator.
//
// The device side only.  Each family is one ObsBasis: how its plan is built and uploaded (a DevPlan of its own in the engine's cache) and how it is
// launched; every entry point is one body over an ObsBasis, and every destination-driven kernel (one-site, fused sum, string apply) goes through one
// launch (obs_launch), which like the other kernels here names its instance through lpp_launch.h's with_flags.
// Operator strings have three families (HubbardStrings, HeisStrings, TjStrings) under one driver and one set of entry-point bodies (STRING_ENTRY).
// The host planners (no GPU, plain C++) are lpp_obs_plan.h (shared sector arithmetic, Hubbard), lpp_obs_tj_plan.h, lpp_obs_heis_plan.h and
// lpp_obs_string_plan.h, for strings in the Heisenberg basis lpp_obs_heis_string_plan.h, in the t-J basis lpp_obs_tj_string_plan.h; the kernels are
// lpp_obs_kernels.h, lpp_obs_tj_kernels.h, lpp_obs_heis_kernels.h, lpp_obs_string_kernels.h, lpp_obs_heis_string_kernels.h and
// lpp_obs_tj_string_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "lpp_engine_impl.h"
#include "lpp_obs_kernels.h"
#include "lpp_obs_sum_plan.h"
#include "lpp_obs_sum_kernels.h"
#include "lpp_obs_string_plan.h"
#include "lpp_obs_string_kernels.h"
#include "lpp_obs_tj_kernels.h"
#include "lpp_obs_heis_kernels.h"
#include "lpp_obs_heis_spin_kernels.h"
#include "lpp_launch.h"
#include "lpp_obs_heis_string_kernels.h"
#include "lpp_obs_tj_string_kernels.h"

using namespace lpp;
using namespace lpp::obs_host;

namespace {

// a planner's refusal (lpp_obs_plan.h, lpp_obs_tj_plan.h, lpp_obs_heis_plan.h, lpp_obs_string_plan.h) as a status
inline lpp_status plan_status(bool ok, const char* why) { return ok ? LPP_OK : fail(LPP_ERR_INVALID, why); }

// ---- device side ---------------------------------------------------------------------------------------------------------------------

// What the cache keeps of one planned operator: the sizes, and in the family's own struct (below) its host plan without the uploaded tables and the
// device tables, freed by the destructor.
struct DevPlan {
	bool has = false; // false: the operator leads to no sector
	int64_t n_src = 0, n_dst = 0;
	int64_t touched = 0; // destinations that have a source, for the byte model
	size_t bytes = 0; // device bytes that count toward kMaxPlanBytes
	virtual ~DevPlan() {}
};
typedef std::unique_ptr<DevPlan> DevPlanPtr;

inline void free_tables(std::initializer_list<void*> tables)
{
	for (void* p : tables)
		if (p) (void)hipFree(p);
}

// one table to the device (at least one element is allocated); the host copy is dropped
template <typename V> hipError_t upload(V** dst, std::vector<V>& src)
{
	hipError_t err = hipMalloc((void**)dst, sizeof(V) * std::max<size_t>(src.size(), 1));
	if (err == hipSuccess && !src.empty()) err = hipMemcpy(*dst, src.data(), sizeof(V) * src.size(), hipMemcpyHostToDevice);
	if (err == hipSuccess) std::vector<V>().swap(src);
	return err;
}

inline bool multi(const lpp_engine* e) { return e->has_comm && e->comm.nranks > 1; }

lpp_status refuse(const lpp_engine* e, const char* who, bool hole_major_ok = false)
{
	if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
	if (e->tj.active && !hole_major_ok) return fail(LPP_ERR_STATE, std::string(who) + ": not on a hole-major t-J engine");
	return LPP_OK;
}

int obs_grid(const lpp_engine* e, int64_t units)
{
	const int64_t tiles = (units + kObsTile - 1) / kObsTile;
	return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)e->num_cus * 32));
}

// The one launch of a destination-driven kernel template <CPLX, ACC>(dst, src, args) over n destination elements: 16-byte units in tiles of kObsTile,
// at most 32 blocks per CU.  launch(grid, lds, cplx, acc) names the instance with the two std::bool_constants and enqueues it on the engine's stream.
template <typename Launch> lpp_status obs_launch(const lpp_engine* e, bool acc, int64_t n, size_t lds, Launch&& launch)
{
	const int grid = obs_grid(e, e->is_complex ? n : (n + 1) / 2);
	with_flags([&](auto cplx, auto accumulate) { launch(grid, lds, cplx, accumulate); }, e->is_complex, acc);
	HIP_TRY(hipGetLastError());
	return LPP_OK;
}

// Everything the entry points below need to know about a basis: they are written once and run for every family.
struct ObsBasis {
	int id;
	bool hole_major_ok; // a hole-major t-J engine is admitted (its resident states and start vectors pass through S.perm)
	bool reads_ndown; // false: one count names the sector, ndown is not read (one cache entry per sector)
	bool fermions; // c / cdagger are operators of the model
	bool no_sector_throws; // new_parts == false is where the reference throws: LPP_ERR_INVALID instead of "no such sector"
	bool sz_has_no_parts; // lpp_obs_new_parts*: sz answers "no new sector" (otherwise it is unsupported like n)
	bool (*counts_ok)(int L, int nup, int ndn); // lpp_obs_new_parts*: the sector check
	int64_t (*sector_size)(int L, int nup, int ndn); // < 0: not a sector
	bool (*new_parts)(int op, int spin, int L, int nup, int ndn, int* n1, int* n2);
	// the plan of one operator, sizes and touched count filled in, its tables uploaded; *err: what the upload met (the caller frees the partial plan)
	lpp_status (*build)(int op, int site, int spin, int L, int nup, int ndn, DevPlanPtr& out, hipError_t* err);
	// z (+)= factor * A src through a plan with has and n_dst > 0
	lpp_status (*launch)(lpp_engine* e, const DevPlan& D, double fr, double fi, const void* d_src, void* d_dst, bool acc);
	// optional, the fused form of z (+)= sum_r f_r A_r src (site = -1 names its plan in the cache); null: sum_dev chains `launch` over the sites
	bool (*sum_fused)(int op);
	lpp_status (*build_sum)(int op, int site, int spin, int L, int nup, int ndn, DevPlanPtr& out, hipError_t* err);
	lpp_status (*launch_sum)(lpp_engine* e, const DevPlan& D, const double* w_re, const double* w_im, const void* d_src, void* d_dst, bool acc);
	// the spin-S digit basis: the two counts are (twiceS, szPlusConst), sz is ONE operator of the basis (no n to split it into), and lpp_obs_new_parts*
	// reports the new sector as (szPlusConst', 0)
	bool spin_args;
};

// ---- the Hubbard product basis (plan: lpp_obs_plan.h, kernel: lpp_obs_kernels.h) ---------------------------------------------------------------
struct HubbardDev : DevPlan {
	ObsPlan host; // tables dropped after the upload
	int32_t *tu = nullptr, *td = nullptr; // null: the species is untouched
	~HubbardDev() override { free_tables({ tu, td }); }
};

lpp_status build_hubbard(int op, int site, int spin, int L, int nup, int ndn, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<HubbardDev> D(new HubbardDev());
	ObsPlan& P = D->host;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan(op, site, spin, L, nup, ndn, &D->has, P, &why), why);
	if (st != LPP_OK) return st;
	D->n_src = P.n_up_src * P.n_dn_src;
	D->n_dst = P.n_up_dst * P.n_dn_dst;
	if (D->has) {
		D->touched = obs_touched(P);
		if (!P.tu.empty()) *err = upload(&D->tu, P.tu);
		if (*err == hipSuccess && !P.td.empty()) *err = upload(&D->td, P.td);
	}
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_hubbard(lpp_engine* e, const DevPlan& D0, double fr, double fi, const void* d_src, void* d_dst, bool acc)
{
	const HubbardDev& D = static_cast<const HubbardDev&>(D0);
	const ObsPlan& P = D.host;
	ObsArgs A { D.tu, D.td, P.n_up_dst, P.n_dn_dst, P.n_up_src, P.sz ? 1 : 0, fr, fi };
	return obs_launch(e, acc, D.n_dst, 0, [&](int g, size_t lds, auto c, auto a) { k_obs_apply<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

// the fused operator sum of this basis (plan: lpp_obs_sum_plan.h, kernels: lpp_obs_sum_kernels.h)
struct HubbardSumDev : DevPlan {
	ObsSumPlan host; // tables and word lists dropped after the upload
	int32_t* tab = nullptr;
	uint8_t* site = nullptr;
	uint32_t *wu = nullptr, *wd = nullptr; // diag: the species' words
	double *cu = nullptr, *cd = nullptr; // diag: the coefficients of the call in flight (rewritten per call, in stream order)
	~HubbardSumDev() override { free_tables({ tab, site, wu, wd, cu, cd }); }
};

lpp_status build_hubbard_sum(int op, int, int spin, int L, int nup, int ndn, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<HubbardSumDev> D(new HubbardSumDev());
	ObsSumPlan& P = D->host;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_sum_plan(op, spin, L, nup, ndn, &D->has, P, &why), why);
	if (st != LPP_OK) return st;
	D->n_src = P.n_up_src * P.n_dn_src;
	D->n_dst = P.n_up_dst * P.n_dn_dst;
	D->touched = D->n_src; // every source state holds a particle c may remove / a hole cdagger may fill, or is read by the diagonal stream
	if (D->has && P.diag) {
		D->bytes = (4 + 16) * (P.words_up.size() + P.words_dn.size()); // the word lists and the coefficients
		*err = upload(&D->wu, P.words_up);
		if (*err == hipSuccess) *err = upload(&D->wd, P.words_dn);
		if (*err == hipSuccess) *err = hipMalloc((void**)&D->cu, 16 * (size_t)std::max<int64_t>(P.n_up_dst, 1));
		if (*err == hipSuccess) *err = hipMalloc((void**)&D->cd, 16 * (size_t)std::max<int64_t>(P.n_dn_dst, 1));
	} else if (D->has) {
		D->bytes = 5 * P.src.size(); // 1.0 MB per unit of W at 16 sites
		*err = upload(&D->tab, P.src);
		if (*err == hipSuccess) *err = upload(&D->site, P.site);
	}
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_hubbard_sum(lpp_engine* e, const DevPlan& D0, const double* w_re, const double* w_im, const void* d_src, void* d_dst, bool acc)
{
	const HubbardSumDev& D = static_cast<const HubbardSumDev&>(D0);
	const ObsSumPlan& P = D.host;
	ObsSumWeights w {};
	for (int r = 0; r < kObsSumSites; r++) { // (sum_dev pads the weights with zeros past the sites)
		w.re[r] = w_re[r];
		w.im[r] = w_im[r];
	}
	if (P.diag) {
		for (int s = 0; s < 2; s++) {
			const int64_t n = s ? P.n_dn_dst : P.n_up_dst;
			const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + kObsBlock - 1) / kObsBlock, 1024));
			with_flags([&](auto c) { k_obs_sum_coef<c><<<g, kObsBlock, 0, e->stream>>>(s ? D.wd : D.wu, n, s ? D.cd : D.cu, w); }, e->is_complex);
		}
		HIP_TRY(hipGetLastError());
		ObsSumDiagArgs A { D.cu, D.cd, P.n_up_dst, P.n_dn_dst, P.alpha, P.beta };
		return obs_launch(e, acc, D.n_dst, 0, [&](int g, size_t lds, auto c, auto a) { k_obs_sum_diag<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
	}
	ObsSumMoveArgs A { D.tab, D.site, P.n, P.W, P.n_up_dst, P.n_dn_dst, P.n_up_src, w };
	if (P.down) return obs_launch(e, acc, D.n_dst, 0, [&](int g, size_t lds, auto c, auto a) { k_obs_sum_move_down<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
	return obs_launch(e, acc, D.n_dst, 0, [&](int g, size_t lds, auto c, auto a) { k_obs_sum_move_up<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

// ---- the one-orbital t-J basis (plan: lpp_obs_tj_plan.h, kernel: lpp_obs_tj_kernels.h) -------------------------------------------------------
struct TjDev : DevPlan {
	ObsTjPlan host; // tables dropped after the upload
	ObsTjDown* dn = nullptr;
	uint32_t* pat = nullptr;
	int32_t* hi = nullptr;
	uint16_t* lo = nullptr;
	int nhi = 0, nlo = 0;
	~TjDev() override { free_tables({ dn, pat, hi, lo }); }
};

lpp_status build_tj(int op, int site, int spin, int L, int nup, int ndn, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<TjDev> D(new TjDev());
	ObsTjPlan& P = D->host;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_tj(op, site, spin, L, nup, ndn, &D->has, P, &why), why);
	if (st != LPP_OK) return st;
	D->n_src = P.n_up_src * P.n_dn_src;
	D->n_dst = P.n_up_dst * P.n_dn_dst;
	if (D->has) {
		D->touched = tj_touched(op, spin, L, P.nup2, P.ndn2);
		D->nhi = (int)P.hi_base.size();
		D->nlo = (int)P.lo_rank.size();
		*err = upload(&D->dn, P.dn);
		if (*err == hipSuccess) *err = upload(&D->pat, P.pat);
		if (*err == hipSuccess) *err = upload(&D->hi, P.hi_base);
		if (*err == hipSuccess) *err = upload(&D->lo, P.lo_rank);
	}
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_tj(lpp_engine* e, const DevPlan& D0, double fr, double fi, const void* d_src, void* d_dst, bool acc)
{
	const TjDev& D = static_cast<const TjDev&>(D0);
	const ObsTjPlan& P = D.host;
	ObsTjArgs A { D.dn, D.pat, D.hi, D.lo, P.up, P.lb, D.nhi, D.nlo, P.n_up_dst, P.n_dn_dst, P.n_up_src, fr, fi };
	return obs_launch(e, acc, D.n_dst, obs_tj_lds_bytes(A.nhi, A.nlo),
	                  [&](int g, size_t lds, auto c, auto a) { k_obs_apply_tj<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

// ---- the S = 1/2 Heisenberg basis (plan: lpp_obs_heis_plan.h, kernel: lpp_obs_heis_kernels.h); nup = szPlusConst -----------------------------
struct HeisDev : DevPlan {
	ObsHeisPlan host; // the run table and the low-word tables dropped after the upload
	ObsHeisRun* runs = nullptr;
	uint16_t *word = nullptr, *rank = nullptr;
	int64_t nruns = 0;
	int nlo = 0;
	~HeisDev() override { free_tables({ runs, word, rank }); }
};

lpp_status build_heis(int op, int site, int spin, int L, int nup, int, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<HeisDev> D(new HeisDev());
	ObsHeisPlan& P = D->host;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_heis(op, site, spin, L, nup, P, &why), why);
	if (st != LPP_OK) return st;
	D->has = true; // (this basis has no "no sector": the plan refuses where the reference throws)
	D->n_src = P.n_src;
	D->n_dst = P.n_dst;
	D->touched = heis_touched(op, spin, L, P.m2);
	D->nruns = (int64_t)P.runs.size() - 1;
	D->nlo = (int)P.word.size();
	D->bytes = sizeof(ObsHeisRun) * P.runs.size(); // 24 MB at 32 sites
	*err = upload(&D->runs, P.runs);
	if (*err == hipSuccess) *err = upload(&D->word, P.word);
	if (*err == hipSuccess) *err = upload(&D->rank, P.rank);
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_heis(lpp_engine* e, const DevPlan& D0, double fr, double fi, const void* d_src, void* d_dst, bool acc)
{
	const HeisDev& D = static_cast<const HeisDev&>(D0);
	const ObsHeisPlan& P = D.host;
	ObsHeisArgs A { D.runs, D.word, D.rank, P.mode, D.nlo, P.bit, D.nruns, D.n_dst, fr, fi };
	return obs_launch(e, acc, D.n_dst, obs_heis_lds_bytes(A.mode, A.nlo),
	                  [&](int g, size_t lds, auto c, auto a) { k_obs_apply_heis<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

// the fused sum_r f_r sz_r of this basis (k_obs_sum_sz_heis): the run table and the low words of the one-site sz plan, and the runs' high parts
struct HeisSumDev : DevPlan {
	ObsHeisRun* runs = nullptr;
	uint16_t* word = nullptr;
	uint64_t* highs = nullptr;
	double* hi = nullptr; // the coefficients of the call in flight (rewritten per call, in stream order)
	int64_t nruns = 0;
	int nlo = 0, lb = 0;
	~HeisSumDev() override { free_tables({ runs, word, highs, hi }); }
};

bool heis_sum_fused_op(int op) { return op == LPP_OP_SZ; }

lpp_status build_heis_sum(int op, int, int spin, int L, int nup, int, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<HeisSumDev> D(new HeisSumDev());
	ObsHeisPlan P;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_heis(op, 0, spin, L, nup, P, &why), why); // (site 0 is in the low part: the plan has the low words)
	if (st != LPP_OK) return st;
	if (op != LPP_OP_SZ) return fail(LPP_ERR_INVALID, "operator sum: the Heisenberg basis has a fused plan for sz only");
	std::vector<uint64_t> highs;
	if (!heis_highs(L - P.lb, P.lb, P.m2, highs) || highs.size() + 1 != P.runs.size())
		return fail(LPP_ERR_INVALID, "operator sum: the sector has more than 2^22 runs of equal high part (the run table's limit)");
	D->has = true;
	D->n_src = P.n_src;
	D->n_dst = P.n_dst;
	D->touched = P.n_dst;
	D->nruns = (int64_t)highs.size();
	D->nlo = (int)P.word.size();
	D->lb = P.lb;
	D->bytes = (sizeof(ObsHeisRun) + 8 + 16) * P.runs.size();
	*err = upload(&D->runs, P.runs);
	if (*err == hipSuccess) *err = upload(&D->word, P.word);
	if (*err == hipSuccess) *err = upload(&D->highs, highs);
	if (*err == hipSuccess) *err = hipMalloc((void**)&D->hi, 16 * (size_t)std::max<int64_t>(D->nruns, 1));
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_heis_sum(lpp_engine* e, const DevPlan& D0, const double* w_re, const double* w_im, const void* d_src, void* d_dst, bool acc)
{
	const HeisSumDev& D = static_cast<const HeisSumDev&>(D0);
	ObsSumHeisArgs A { D.runs, D.word, D.hi, D.nlo, D.nruns, D.n_dst, 0.0, 0.0, {} };
	for (int r = 0; r < kObsSumSites; r++) { // F in ascending site, as every sum of weights here
		A.w.re[r] = w_re[r];
		A.w.im[r] = w_im[r];
		A.F_re += w_re[r];
		A.F_im += w_im[r];
	}
	const int g = (int)std::max<int64_t>(1, std::min<int64_t>((D.nruns + kObsBlock - 1) / kObsBlock, 1024));
	with_flags([&](auto c) { k_obs_sum_hi_heis<c><<<g, kObsBlock, 0, e->stream>>>(D.highs, D.nruns, D.lb, D.hi, A.w); }, e->is_complex);
	HIP_TRY(hipGetLastError());
	return obs_launch(e, acc, D.n_dst, obs_sum_heis_lds_bytes(A.nlo),
	                  [&](int g, size_t lds, auto c, auto a) { k_obs_sum_sz_heis<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

// ---- the spin-S Heisenberg digit basis (plan: lpp_obs_heis_spin_plan.h, kernel: lpp_obs_heis_spin_kernels.h); nup = twiceS, ndn = szPlusConst --------
struct HeisSpinDev : DevPlan {
	ObsHeisSpinPlan host; // the tables dropped after the upload
	ObsHeisSpinRun* runs = nullptr;
	uint16_t *word = nullptr, *rank = nullptr;
	double* val = nullptr;
	int64_t nruns = 0;
	int nword = 0, nrank = 0;
	~HeisSpinDev() override { free_tables({ runs, word, rank, val }); }
};

lpp_status build_heis_spin(int op, int site, int spin, int L, int twiceS, int m, DevPlanPtr& out, hipError_t* err)
{
	std::unique_ptr<HeisSpinDev> D(new HeisSpinDev());
	ObsHeisSpinPlan& P = D->host;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_heis_spin(op, site, spin, L, twiceS, m, P, &why), why);
	if (st != LPP_OK) return st;
	D->has = true; // (this basis has no "no sector": the plan refuses S+ on the top sector and S- on szPlusConst = 0)
	D->n_src = P.n_src;
	D->n_dst = P.n_dst;
	D->touched = heis_spin_touched(op, L, twiceS, P.m2);
	D->nruns = (int64_t)P.runs.size() - 1;
	D->nword = (int)P.word.size();
	D->nrank = (int)P.rank.size();
	D->bytes = sizeof(ObsHeisSpinRun) * P.runs.size();
	*err = upload(&D->runs, P.runs);
	if (*err == hipSuccess) *err = upload(&D->word, P.word);
	if (*err == hipSuccess) *err = upload(&D->rank, P.rank);
	if (*err == hipSuccess) *err = upload(&D->val, P.val);
	out = std::move(D);
	return LPP_OK;
}

lpp_status launch_heis_spin(lpp_engine* e, const DevPlan& D0, double fr, double fi, const void* d_src, void* d_dst, bool acc)
{
	const HeisSpinDev& D = static_cast<const HeisSpinDev&>(D0);
	const ObsHeisSpinPlan& P = D.host;
	const ObsHeisSpinArgs A { D.runs, D.word, D.rank, D.val, P.mode, D.nword, D.nrank, P.shift, P.mask, P.twiceS, D.nruns, D.n_dst, fr, fi };
	return obs_launch(e, acc, D.n_dst, obs_heis_spin_lds_bytes(A.mode, A.nword, A.nrank),
	                  [&](int g, size_t lds, auto c, auto a) { k_obs_apply_heis_spin<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
}

enum { BASIS_HUBBARD = 0, BASIS_TJ = 1, BASIS_HEIS = 2, BASIS_HEIS_SPIN = 3 };
const ObsBasis kHubbard {
	.id = BASIS_HUBBARD, .hole_major_ok = false, .reads_ndown = true, .fermions = true, .no_sector_throws = false, .sz_has_no_parts = true,
	.counts_ok = [](int L, int nup, int ndn) { return L >= 1 && nup >= 0 && ndn >= 0 && nup <= L && ndn <= L; },
	.sector_size = hubbard_sector_size, .new_parts = new_parts, .build = build_hubbard, .launch = launch_hubbard,
	.sum_fused = obs_sum_fused_op, .build_sum = build_hubbard_sum, .launch_sum = launch_hubbard_sum, .spin_args = false };
const ObsBasis kTj {
	.id = BASIS_TJ, .hole_major_ok = true, .reads_ndown = true, .fermions = true, .no_sector_throws = false, .sz_has_no_parts = false,
	.counts_ok = [](int L, int nup, int ndn) { return L >= 1 && nup >= 0 && ndn >= 0 && nup + ndn <= L; },
	.sector_size = tj_sector_size, .new_parts = new_parts_tj, .build = build_tj, .launch = launch_tj,
	.sum_fused = nullptr, .build_sum = nullptr, .launch_sum = nullptr, .spin_args = false };
const ObsBasis kHeis {
	.id = BASIS_HEIS, .hole_major_ok = false, .reads_ndown = false, .fermions = false, .no_sector_throws = true, .sz_has_no_parts = true,
	.counts_ok = [](int L, int nup, int) { return heis_sector_size(L, nup, 0) >= 0; },
	.sector_size = heis_sector_size, .new_parts = new_parts_heis, .build = build_heis, .launch = launch_heis,
	.sum_fused = heis_sum_fused_op, .build_sum = build_heis_sum, .launch_sum = launch_heis_sum, .spin_args = false };
// (reads_ndown: the cache key holds both counts, so it tells twiceS apart; the operator sums chain the one-site launches)
const ObsBasis kHeisSpin {
	.id = BASIS_HEIS_SPIN, .hole_major_ok = false, .reads_ndown = true, .fermions = false, .no_sector_throws = true, .sz_has_no_parts = true,
	.counts_ok = [](int L, int twiceS, int m) { return heis_spin_sector_size(L, twiceS, m) >= 0; },
	.sector_size = heis_spin_sector_size, .new_parts = new_parts_heis_spin, .build = build_heis_spin, .launch = launch_heis_spin,
	.sum_fused = nullptr, .build_sum = nullptr, .launch_sum = nullptr, .spin_args = true };

// The tables of one (operator, site, spin, sites, sector), uploaded once and kept with the engine.  The key is what the caller passes -- the engine
// needs no model for lpp_engine_apply_operator -- so the cache is bounded: a density of states or a two-point matrix uses at most 2 * sites entries
// per operator; past kMaxPlans entries everything is dropped and rebuilt on demand.  The returned pointer is valid until the next get_plan.
constexpr size_t kMaxPlans = 256;
// ... or past 1 GiB of DevPlan::bytes, which counts the Heisenberg run tables alone: a two-point sweep over 32 sites holds 0.8 GB of them, every
// other table is a species' or a half word's size
constexpr size_t kMaxPlanBytes = (size_t)1 << 30;
typedef std::tuple<int, int, int, int, int, int, int> PlanKey; // basis, operator, site, spin, sites, nup, ndown
struct ObsCache {
	std::map<PlanKey, DevPlanPtr> plans;
	size_t bytes = 0; // DevPlan::bytes summed over the plans
	ObsSwitches sw = obs_switches_from_env(); // resolved once, when the engine first plans an operator
};

// sum: the fused plan of an operator sum (B.build_sum), kept under site = -1 -- a key no one-site plan has, the planners refuse such a site
lpp_status get_plan(lpp_engine* e, const ObsBasis& B, int op, int site, int spin, int L, int nup, int ndn, const DevPlan** out, bool sum = false)
{
	if (!e->obs) e->obs = new ObsCache();
	ObsCache* C = (ObsCache*)e->obs;
	if (!B.reads_ndown) ndn = 0;
	if (sum) site = -1;
	else if (site < 0) { // the planner's own refusal, past the cache
		DevPlanPtr D;
		hipError_t err = hipSuccess;
		const lpp_status st = B.build(op, site, spin, L, nup, ndn, D, &err);
		return st != LPP_OK ? st : fail(LPP_ERR_INVALID, "observables: bad sites / site / sector");
	}
	const PlanKey key(B.id, op, site, spin, L, nup, ndn);
	auto it = C->plans.find(key);
	if (it == C->plans.end()) {
		DevPlanPtr D;
		hipError_t err = hipSuccess;
		lpp_status st = (sum ? B.build_sum : B.build)(op, site, spin, L, nup, ndn, D, &err);
		if (st != LPP_OK) return st;
		if (err != hipSuccess) {
			D.reset(); // the tables uploaded so far
			if (err == hipErrorOutOfMemory) {
				(void)hipGetLastError();
				return fail(LPP_ERR_NOMEM, "observables: no device memory for the operator tables");
			}
			HIP_TRY(err);
		}
		if (C->plans.size() >= kMaxPlans || C->bytes + D->bytes > kMaxPlanBytes) {
			HIP_TRY(hipStreamSynchronize(e->stream)); // launches that still read the old tables
			C->plans.clear();
			C->bytes = 0;
		}
		C->bytes += D->bytes;
		it = C->plans.emplace(key, std::move(D)).first;
	}
	*out = it->second.get();
	return LPP_OK;
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
lpp_status apply_dev(lpp_engine* e, const ObsBasis& B, int op, int site, int spin, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc,
                     bool* has)
{
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, B, op, site, spin, L, nup, ndn, &D);
	if (st != LPP_OK) return st;
	*has = D->has;
	if (!D->has) return LPP_OK;
	if ((st = check_vectors(e, fi, d_src, d_dst)) != LPP_OK) return st;
	if (D->n_dst == 0) return LPP_OK;
	return B.launch(e, *D, fr, fi, d_src, d_dst, acc);
}

// the operator Engine::accModifiedState applies (Engine.h:535-599): n directly, sz as n_up/2 - n_down/2 (the spin-S digit basis: its own sz), the
// others as given
lpp_status acc_modified_dev(lpp_engine* e, const ObsBasis& B, int op, int site, int spin, int L, int nup, int ndn, double isign, const void* d_src, void* d_dst, bool acc, bool* has)
{
	if (op == LPP_OP_SZ && !B.spin_args) {
		lpp_status st = apply_dev(e, B, LPP_OP_N, site, LPP_SPIN_UP, L, nup, ndn, isign * 0.5, 0.0, d_src, d_dst, acc, has);
		if (st != LPP_OK) return st;
		return apply_dev(e, B, LPP_OP_N, site, LPP_SPIN_DOWN, L, nup, ndn, -isign * 0.5, 0.0, d_src, d_dst, true, has);
	}
	return apply_dev(e, B, op, site, spin, L, nup, ndn, isign, 0.0, d_src, d_dst, acc, has);
}

// the site weights of an operator sum, checked and padded with zeros to the kernels' fixed count
struct SumWeights {
	double re[kObsSumSites] = {}, im[kObsSumSites] = {};
};
lpp_status sum_weights(const lpp_engine* e, const char* who, int L, int nweights, const double* w_re, const double* w_im, SumWeights& w)
{
	if (!w_re) return fail(LPP_ERR_INVALID, std::string(who) + ": null weights");
	if (L < 1 || L > kObsSumMaxSites) return fail(LPP_ERR_INVALID, std::string(who) + ": bad sites / sector");
	if (nweights != L) return fail(LPP_ERR_INVALID, std::string(who) + ": one weight per site");
	for (int r = 0; r < L; r++) {
		w.re[r] = w_re[r];
		w.im[r] = w_im ? w_im[r] : 0.0;
		if (!e->is_complex && w.im[r] != 0.0) return fail(LPP_ERR_INVALID, std::string(who) + ": complex weight on a real engine");
	}
	return LPP_OK;
}

// z (+)= sum_r f_r A_r src on device vectors in the basis order, A_r as Engine::accModifiedState has them (sz of the two fermion bases is
// n_up/2 - n_down/2; the Heisenberg basis applies its raw sz, as its spectral functions do).  One fused launch where the basis has one for the
// operator (B.launch_sum), otherwise -- and under LPP_OBS_SUM_CHAIN=1 -- the chain of B.launch over the sites with a non-zero weight, which is
// also the yardstick of the fused kernels.  *has == false: no such sector, nothing was launched.  The sizes are reported for the callers that stage.
lpp_status sum_dev(lpp_engine* e, const ObsBasis& B, int op, int spin, int L, int nup, int ndn, const SumWeights& w, const void* d_src, void* d_dst, bool acc, bool* has,
                   int64_t* n_src = nullptr, int64_t* n_dst = nullptr)
{
	const bool split_sz = (op == LPP_OP_SZ) && B.fermions;
	const int op1 = split_sz ? LPP_OP_N : op; // the one-site operator whose plan names the sector and carries the basis' refusals
	const DevPlan* D = nullptr;
	lpp_status st = get_plan(e, B, op1, 0, spin, L, nup, ndn, &D);
	if (st != LPP_OK) return st;
	*has = D->has;
	if (n_src) *n_src = D->n_src;
	if (n_dst) *n_dst = D->n_dst;
	if (!D->has) return LPP_OK;
	const int64_t nd = D->n_dst;
	if (!d_src && !d_dst) return LPP_OK; // sizes only
	if ((st = check_vectors(e, 0.0, d_src, d_dst)) != LPP_OK) return st;
	if (nd == 0) return LPP_OK;
	if (B.launch_sum && B.sum_fused(op) && ((ObsCache*)e->obs)->sw.sum_chain.value_or(0) == 0) {
		if ((st = get_plan(e, B, op, -1, spin, L, nup, ndn, &D, true)) != LPP_OK) return st;
		return B.launch_sum(e, *D, w.re, w.im, d_src, d_dst, acc);
	}
	bool h = false, first = !acc;
	for (int r = 0; r < L; r++) {
		if (w.re[r] == 0.0 && w.im[r] == 0.0) continue;
		if (split_sz) {
			if ((st = apply_dev(e, B, LPP_OP_N, r, LPP_SPIN_UP, L, nup, ndn, 0.5 * w.re[r], 0.5 * w.im[r], d_src, d_dst, !first, &h)) != LPP_OK) return st;
			st = apply_dev(e, B, LPP_OP_N, r, LPP_SPIN_DOWN, L, nup, ndn, -0.5 * w.re[r], -0.5 * w.im[r], d_src, d_dst, true, &h);
		} else {
			st = apply_dev(e, B, op, r, spin, L, nup, ndn, w.re[r], w.im[r], d_src, d_dst, !first, &h);
		}
		if (st != LPP_OK) return st;
		first = false;
	}
	if (first) HIP_TRY(hipMemsetAsync(d_dst, 0, e->esz * (size_t)nd, e->stream)); // no weight: z = 0
	return LPP_OK;
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
	st = apply_dev(e, B, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate != 0, &h);
	*has = h ? 1 : 0;
	return st;
}

// host vectors of ns / nd bytes staged on the device around run(d_src, d_dst): the source up, the destination up where it is accumulated into, and back
template <typename Run> lpp_status staged(lpp_engine* e, size_t ns, size_t nd, const void* src, void* dst, int32_t accumulate, Run&& run)
{
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(nd, 16) + 16));
	HIP_TRY(hipMemcpyAsync(ds.p, src, ns, hipMemcpyHostToDevice, e->stream));
	if (accumulate) HIP_TRY(hipMemcpyAsync(dd.p, dst, nd, hipMemcpyHostToDevice, e->stream));
	lpp_status st = run(ds.p, dd.p);
	if (st != LPP_OK) return st;
	HIP_TRY(hipMemcpyAsync(dst, dd.p, nd, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status apply_operator_host_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                                    double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has)
{
	if (!e || !has || !src || !dst) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	const DevPlan* D = nullptr;
	if ((st = get_plan(e, B, op, site, spin, nsites, nup, ndown, &D)) != LPP_OK) return st;
	*has = D->has ? 1 : 0;
	if (!D->has) return LPP_OK;
	return staged(e, e->esz * (size_t)D->n_src, e->esz * (size_t)D->n_dst, src, dst, accumulate, [&](const void* d_src, void* d_dst) {
		bool h = false;
		return apply_dev(e, B, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate != 0, &h);
	});
}

// milliseconds per step over `iters` steps after `warmup` untimed ones, between two events on the engine's stream; a failing step ends the loop
struct EventPair {
	hipEvent_t a = nullptr, b = nullptr;
	~EventPair()
	{
		if (a) (void)hipEventDestroy(a);
		if (b) (void)hipEventDestroy(b);
	}
};
template <typename Step> lpp_status timed_steps(lpp_engine* e, int warmup, int iters, double* ms_per_step, Step&& step)
{
	EventPair ev;
	hipEvent_t &t0 = ev.a, &t1 = ev.b;
	HIP_TRY(hipEventCreate(&t0));
	HIP_TRY(hipEventCreate(&t1));
	lpp_status st = LPP_OK;
	for (int i = 0; i < warmup + iters && st == LPP_OK; i++) {
		if (i == warmup) (void)hipEventRecord(t0, e->stream);
		st = step();
	}
	(void)hipEventRecord(t1, e->stream);
	hipError_t err = hipEventSynchronize(t1);
	float ms = 0;
	if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
	if (err == hipSuccess) err = hipGetLastError();
	if (st != LPP_OK) return st;
	HIP_TRY(err);
	*ms_per_step = ms / iters;
	return LPP_OK;
}

lpp_status bench_operator_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                               int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes)
{
	if (!e || !ms_per_launch || iters < 1 || warmup < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	const DevPlan* D = nullptr;
	if ((st = get_plan(e, B, op, site, spin, nsites, nup, ndown, &D)) != LPP_OK) return st;
	if (!D->has) return fail(LPP_ERR_INVALID, std::string(who) + ": the operator leads to no sector");
	const int64_t ns = D->n_src, nd = D->n_dst, touched = D->touched; // (the plan is valid until the next get_plan; touched: the byte model below)
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(e->esz * (size_t)ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(e->esz * (size_t)nd, 16) + 16));
	HIP_TRY(hipMemsetAsync(ds.p, 0, e->esz * (size_t)ns, e->stream));
	HIP_TRY(hipMemsetAsync(dd.p, 0, e->esz * (size_t)nd, e->stream));
	bool h = false;
	st = timed_steps(e, warmup, iters, ms_per_launch, [&] { return apply_dev(e, B, op, site, spin, nsites, nup, ndown, 1.0, 0.0, ds.p, dd.p, true, &h); });
	if (st != LPP_OK) return st;
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
				with_flags([&](auto c) { k_multi_dot<c><<<nb, kBlock, 0, e->stream>>>((const double2*)xi, v0, ld2, np, n2, (double*)part.p); }, e->is_complex);
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
	st = apply_dev(e, B, op, isite, spin, L, nup, ndown, 1.0, 0.0, gs, M.p, true, &has);
	if (st != LPP_OK) return st;
	st = apply_dev(e, B, op, jsite, spin, L, nup, ndown, isign, 0.0, gs, M.p, true, &has);
	if (st != LPP_OK) return st;
	k_dot<<<nb, kBlock, 0, e->stream>>>((const double2*)M.p, (const double2*)M.p, stride / 2, (double*)part.p);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)part.p, nb, 1, 1, (double*)part.p + nb);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(weight, (double*)part.p + nb, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream)); // the sector engine runs on a stream of its own
	return decomposition_device_any(sector, M.p, nsteps, a, b, stats); // (a hole-major sector engine takes the vector through its permutation)
}

// ---- site-weighted operator sums: z (+)= sum_r f_r A_r src, the modified state of the momentum-resolved quantities --------------------------------

lpp_status apply_sum_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights,
                          const double* w_re, const double* w_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has)
{
	if (!e || !has || !d_src || !d_dst) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	SumWeights w;
	if ((st = sum_weights(e, who, nsites, nweights, w_re, w_im, w)) != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool h = false;
	st = sum_dev(e, B, op, spin, nsites, nup, ndown, w, d_src, d_dst, accumulate != 0, &h);
	*has = h ? 1 : 0;
	return st;
}

lpp_status apply_sum_host_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights,
                               const double* w_re, const double* w_im, const void* src, void* dst, int32_t accumulate, int32_t* has, int64_t* n_dst)
{
	if (!e || !has) return fail(LPP_ERR_INVALID, std::string(who) + ": null argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	SumWeights w;
	if ((st = sum_weights(e, who, nsites, nweights, w_re, w_im, w)) != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool h = false;
	int64_t ns = 0, nd = 0;
	if ((st = sum_dev(e, B, op, spin, nsites, nup, ndown, w, nullptr, nullptr, false, &h, &ns, &nd)) != LPP_OK) return st; // sizes and refusals
	*has = h ? 1 : 0;
	if (n_dst) *n_dst = nd;
	if (!h || (!src && !dst)) return LPP_OK; // both null: the sector's size only
	if (!src || !dst) return fail(LPP_ERR_INVALID, std::string(who) + ": null vector");
	return staged(e, e->esz * (size_t)ns, e->esz * (size_t)nd, src, dst, accumulate, [&](const void* d_src, void* d_dst) {
		return sum_dev(e, B, op, spin, nsites, nup, ndown, w, d_src, d_dst, accumulate != 0, &h);
	});
}

lpp_status bench_sum_body(const ObsBasis& B, const char* who, lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights,
                          const double* w_re, const double* w_im, int32_t accumulate, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes)
{
	if (!e || !ms_per_launch || iters < 1 || warmup < 0) return fail(LPP_ERR_INVALID, std::string(who) + ": bad argument");
	lpp_status st = refuse(e, who, B.hole_major_ok);
	if (st != LPP_OK) return st;
	SumWeights w;
	if ((st = sum_weights(e, who, nsites, nweights, w_re, w_im, w)) != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	bool h = false;
	int64_t ns = 0, nd = 0;
	if ((st = sum_dev(e, B, op, spin, nsites, nup, ndown, w, nullptr, nullptr, false, &h, &ns, &nd)) != LPP_OK) return st;
	if (!h) return fail(LPP_ERR_INVALID, std::string(who) + ": the operator leads to no sector");
	DevBuf ds, dd;
	HIP_TRY_MEM(hipMalloc(&ds.p, std::max<size_t>(e->esz * (size_t)ns, 16)));
	HIP_TRY_MEM(hipMalloc(&dd.p, std::max<size_t>(e->esz * (size_t)nd, 16) + 16));
	HIP_TRY(hipMemsetAsync(ds.p, 0, e->esz * (size_t)ns, e->stream));
	HIP_TRY(hipMemsetAsync(dd.p, 0, e->esz * (size_t)nd, e->stream));
	st = timed_steps(e, warmup, iters, ms_per_launch, [&] { return sum_dev(e, B, op, spin, nsites, nup, ndown, w, ds.p, dd.p, accumulate != 0, &h); });
	if (st != LPP_OK) return st;
	// the byte model of the sum, whichever way it is launched: destination written (and read when accumulating), source elements touched once
	if (model_bytes) *model_bytes = (double)e->esz * ((accumulate ? 2.0 : 1.0) * (double)nd + (double)ns);
	return LPP_OK;
}

// |phi> = sum_r f_r A_r |resident state> in M (zero padded to a whole 16-byte unit) and <phi|phi>, read back after a stream sync.  sector: the engine
// that will decompose |phi> (null: none); it must hold the operator's sector, which is checked after the sizes-only pass, before anything is launched
lpp_status sum_state(const ObsBasis& B, const std::string& who, lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                     int32_t nweights, const double* w_re, const double* w_im, DevBuf& M, int64_t* ndst, double* norm2, bool* has, const lpp_engine* sector = nullptr)
{
	lpp_status st = refuse(e, who.c_str(), B.hole_major_ok);
	if (st != LPP_OK) return st;
	SumWeights w;
	if ((st = sum_weights(e, who.c_str(), nsites, nweights, w_re, w_im, w)) != LPP_OK) return st;
	double* gs = nullptr;
	if ((st = state_ptr(e, state, who.c_str(), &gs)) != LPP_OK) return st;
	if (B.sector_size(nsites, nup, ndown) < 0 || e->resident_len != B.sector_size(nsites, nup, ndown))
		return fail(LPP_ERR_INVALID, who + ": (sites, nup, ndown) is not the sector of the resident state");
	HIP_TRY(hipSetDevice(e->cfg.device));
	int64_t ns = 0;
	if ((st = sum_dev(e, B, op, spin, nsites, nup, ndown, w, nullptr, nullptr, false, has, &ns, ndst)) != LPP_OK) return st;
	if (!*has) return sector ? fail(LPP_ERR_INVALID, who + ": the operator leads to no sector (lpp_obs_new_parts)") : LPP_OK;
	if (sector && *ndst != sector->n_global) return fail(LPP_ERR_INVALID, who + ": the sector engine does not hold the operator's sector");
	const int wd = e->is_complex ? 2 : 1;
	const int64_t stride = (*ndst * wd + 1) & ~(int64_t)1;
	DevBuf part;
	HIP_TRY_MEM(hipMalloc(&M.p, sizeof(double) * (size_t)stride + 16));
	const int nb = blas_blocks(stride / 2);
	HIP_TRY_MEM(hipMalloc(&part.p, sizeof(double) * (size_t)(nb + 1)));
	HIP_TRY(hipMemsetAsync(M.p, 0, sizeof(double) * (size_t)stride + 16, e->stream)); // the padding element of an odd length stays 0
	if ((st = sum_dev(e, B, op, spin, nsites, nup, ndown, w, gs, M.p, false, has)) != LPP_OK) return st;
	k_dot<<<nb, kBlock, 0, e->stream>>>((const double2*)M.p, (const double2*)M.p, stride / 2, (double*)part.p);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)part.p, nb, 1, 1, (double*)part.p + nb);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(norm2, (double*)part.p + nb, sizeof(double), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return LPP_OK;
}

lpp_status sum_norm2_body(const ObsBasis& B, const std::string& who, lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                          int32_t nweights, const double* w_re, const double* w_im, double* norm2, int32_t* has)
{
	if (!e || !norm2 || !has) return fail(LPP_ERR_INVALID, who + ": null argument");
	DevBuf M;
	int64_t ndst = 0;
	bool h = false;
	*norm2 = 0.0;
	lpp_status st = sum_state(B, who, e, state, op, spin, nsites, nup, ndown, nweights, w_re, w_im, M, &ndst, norm2, &h);
	*has = h ? 1 : 0;
	return st;
}

// spectral_body with the modified state from one sum_dev call; an operator that stays in the sector takes a sector engine of the same sector
lpp_status spectral_sum_body(const ObsBasis& B, const std::string& who, lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t nup,
                             int32_t ndown, int32_t nweights, const double* w_re, const double* w_im, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats)
{
	if (!e || !sector || !weight || !nsteps || !a || !b) return fail(LPP_ERR_INVALID, who + ": null argument");
	lpp_status st = refuse(sector, (who + " (sector engine)").c_str(), B.hole_major_ok);
	if (st != LPP_OK) return st;
	if (e->cfg.device != sector->cfg.device || e->is_complex != sector->is_complex) return fail(LPP_ERR_INVALID, who + ": the sector engine must share device and dtype");
	if (!sector->has_matrix()) return fail(LPP_ERR_STATE, who + ": the sector engine has no matrix");
	DevBuf M;
	int64_t ndst = 0;
	bool h = false;
	if ((st = sum_state(B, who, e, state, op, spin, nsites, nup, ndown, nweights, w_re, w_im, M, &ndst, weight, &h, sector)) != LPP_OK) return st;
	if (*weight == 0.0) { // |phi> = 0 (S^z_q=0 of a singlet, all weights zero): nothing to decompose, the fraction is identically 0
		*nsteps = 0;
		return LPP_OK;
	}
	return decomposition_device_any(sector, M.p, nsteps, a, b, stats); // (the stream of e is synchronised: the sector engine runs on a stream of its own)
}

// ---- operator strings on the device: three families, one driver -----------------------------------------------------------------------------------
//
// A family of strings is a struct (HubbardStrings, HeisStrings and TjStrings below) with
//   Plan                                  the host plan of one string
//   kBadSector, kNotResident, kLeaves     its wording of three refusals
//   refuse(e, who, conv)                  what the engine or the convention rules out
//   plan(conv, nops, ops, sites, spins, flags, L, nup, ndn, P)    its planner, the refusal as a status
//   sector_size(L, nup, ndn)              < 0: not a sector
//   has_sector(P)                         false: the string leads to no sector; apply reports that and launches nothing
//   new_sector(P, &nup, &ndn), n_src(P), n_dst(P)    the sector apply reports, the lengths of its vectors
//   apply(e, P, L, nup, ndn, fr, fi, d_src, d_dst, acc)    z (+)= factor * string src: the tables are the call's own, so it ends with a stream sync
//   stays(P, nup, ndn)                    the bracket kernel launches for it: it is not identically zero and ends in (nup, ndn)
//   scale(P), reached(P, L, nup)          the factor on its bracket; the destinations it reaches, for the byte model
//   Work                                  the bracket kernel's device workspace for kObsStringBatch strings, a DotOut with
//                                         prepare(e, L, nup, ndn, nstrings), load(e, plans, ns, L, nup, ndn) and launch(e, bra, ket, d_out)
// Everything after the three structs is written once over F.  A further family is one more struct and one more name per STRING_ENTRY.

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

// what a bracket workspace of either family ends in: the partial sums of one launch over a sector of n states and the brackets of all the call's strings
struct DotOut {
	DevBuf part, out;
	int grid = 1;
	lpp_status alloc_out(const lpp_engine* e, int64_t n, int64_t nstrings)
	{
		grid = obs_grid(e, e->is_complex ? n : (n + 1) / 2);
		HIP_TRY_MEM(part.alloc(sizeof(double) * 2 * kObsStringBatch * (size_t)grid));
		HIP_TRY_MEM(out.alloc(sizeof(double) * 2 * (size_t)std::max<int64_t>(nstrings, 1)));
		return LPP_OK;
	}
	// the tail of every launch: the fixed-order sum of the partials of ns strings into d_out[0 .. 2 ns)
	void reduce(lpp_engine* e, int ns, double* d_out) const
	{
		k_reduce_final<<<1, kBlock, 0, e->stream>>>((const double*)part.p, grid, 2 * kObsStringBatch, 2 * ns, d_out);
	}
};

// the Hubbard product basis: a string is ONE pair of tables and up to 16 sz entries (plan and upload image: lpp_obs_string_plan.h, kernels:
// lpp_obs_string_kernels.h)
struct HubbardStrings {
	typedef StringPlan Plan;
	static constexpr const char* kBadSector = ": bad sites / sector";
	static constexpr const char* kNotResident = ": (sites, nup, ndown) is not the sector of the resident states";
	static constexpr const char* kLeaves = ": a string that leaves the sector launches nothing";

	// t-J and Heisenberg engines set up through the Python layer or the C++ shim are refused there, by the model's name; here what the engine itself knows
	static lpp_status refuse(const lpp_engine* e, const char* who, int)
	{
		if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
		if (e->tj.active) return fail(LPP_ERR_INVALID, std::string(who) + ": the t-J model (TjMultiOrb) is not supported, operator strings are built for the Hubbard product basis");
		return LPP_OK;
	}
	static lpp_status plan(int conv, int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int L, int nup, int ndn, Plan& P)
	{
		const char* why = nullptr;
		return plan_status(plan_string(conv, nops, ops, sites, spins, flags, L, nup, ndn, P, &why), why);
	}
	static int64_t sector_size(int L, int nup, int ndn) { return hubbard_sector_size(L, nup, ndn); }
	static bool has_sector(const Plan& P) { return P.has; }
	static void new_sector(const Plan& P, int32_t* nup, int32_t* ndn) { *nup = P.nup2, *ndn = P.ndn2; }
	static int64_t n_src(const Plan& P) { return P.n_up_src * P.n_dn_src; }
	static int64_t n_dst(const Plan& P) { return P.n_up_dst * P.n_dn_dst; }
	static bool stays(const Plan& P, int nup, int ndn) { return P.has && P.nup2 == nup && P.ndn2 == ndn; } // Engine.h:364, :382-383
	static double scale(const Plan& P) { return P.scale; }
	static double reached(const Plan& P, int, int)
	{
		const auto live = [](int32_t v) { return v != 0; };
		return (double)std::count_if(P.tu.begin(), P.tu.end(), live) * (double)std::count_if(P.td.begin(), P.td.end(), live);
	}

	// slot s of an uploaded image at d as the kernels take a string
	static ObsString dev_string(const Plan& P, const StringImage& G, const int32_t* d, int s)
	{
		const StringSzWords sz = pack_sz(P);
		return ObsString { d + G.tab_up(s), d + G.tab_dn(s), sz.lo, sz.hi, P.nsz, 0 };
	}

	// one launch, the scale folded into the factor; the word lists are uploaded only for a string with sz entries
	static lpp_status apply(lpp_engine* e, const Plan& P, int L, int nup, int ndn, double fr, double fi, const void* d_src, void* d_dst, bool acc)
	{
		lpp_status st = check_vectors(e, fi, d_src, d_dst);
		if (st != LPP_OK) return st;
		const bool words = P.nsz > 0;
		const StringImage G { P.n_up_dst, P.n_dn_dst, 1, words ? P.n_up_src : 0, words ? P.n_dn_src : 0 };
		std::vector<int32_t> img;
		const char* why = nullptr;
		if (!string_image_begin(G, L, nup, ndn, img, &why) || !string_image_tables(G, &P, 1, img, &why)) return fail(LPP_ERR_INVALID, why);
		DevBuf T;
		HIP_TRY_MEM(T.alloc(4 * img.size()));
		HIP_TRY(hipMemcpyAsync(T.p, img.data(), 4 * img.size(), hipMemcpyHostToDevice, e->stream));
		const int32_t* d = (const int32_t*)T.p;
		ObsStringApplyArgs A { dev_string(P, G, d, 0), (const uint32_t*)(d + G.words_up()), (const uint32_t*)(d + G.words_dn()), P.n_up_dst, P.n_dn_dst, P.n_up_src,
			                   fr * P.scale, fi * P.scale };
		st = obs_launch(e, acc, n_dst(P), 0, [&](int g, size_t lds, auto c, auto a) { k_obs_string_apply<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
		if (st != LPP_OK) return st;
		HIP_TRY(hipStreamSynchronize(e->stream));
		return LPP_OK;
	}

	// kObsStringBatch pairs of tables and the sector's two word lists in one image, uploaded whole per batch
	struct Work : DotOut {
		DevBuf tabs;
		std::vector<int32_t> img;
		StringImage G;
		ObsStringDotArgs A;
		lpp_status prepare(lpp_engine* e, int L, int nup, int ndn, int64_t nstrings)
		{
			const int64_t nu = binom(L, nup), nd = binom(L, ndn);
			G = StringImage { nu, nd, kObsStringBatch, nu, nd };
			const char* why = nullptr;
			if (!string_image_begin(G, L, nup, ndn, img, &why)) return fail(LPP_ERR_INVALID, why);
			HIP_TRY_MEM(tabs.alloc(4 * img.size()));
			return alloc_out(e, nu * nd, nstrings);
		}
		lpp_status load(lpp_engine* e, const Plan* plans, int ns, int, int, int)
		{
			const char* why = nullptr;
			if (!string_image_tables(G, plans, ns, img, &why)) return fail(LPP_ERR_INVALID, why);
			const int32_t* d = (const int32_t*)tabs.p;
			A = ObsStringDotArgs {};
			for (int s = 0; s < ns; s++) A.s[s] = dev_string(plans[s], G, d, s);
			A.words_up = (const uint32_t*)(d + G.words_up());
			A.words_dn = (const uint32_t*)(d + G.words_dn());
			A.n_up = G.ntu;
			A.n_dn = G.ntd;
			A.partial = (double*)part.p;
			A.ns = ns;
			HIP_TRY(hipMemcpyAsync(tabs.p, img.data(), 4 * img.size(), hipMemcpyHostToDevice, e->stream));
			return LPP_OK;
		}
		void launch(lpp_engine* e, const double* bra, const double* ket, double* d_out) const
		{
			with_flags([&](auto c) { k_obs_string_dot<c><<<grid, kObsBlock, 0, e->stream>>>(bra, ket, A); }, e->is_complex);
			reduce(e, A.ns, d_out);
		}
	};
};

// the S = 1/2 Heisenberg basis: a string is five masks and a sign, per destination run one source entry (plan and packing:
// lpp_obs_heis_string_plan.h, kernels: lpp_obs_heis_string_kernels.h); nup = szPlusConst, ndown is not read
struct HeisStrings {
	typedef HeisStringPlan Plan;
	static constexpr const char* kBadSector = ": bad sites / sector (szPlusConst <= sites <= 62)";
	static constexpr const char* kNotResident = ": (sites, szPlusConst) is not the sector of the resident states";
	static constexpr const char* kLeaves = ": a string that is identically zero or leaves the sector launches nothing";

	static lpp_status refuse(const lpp_engine* e, const char* who, int conv)
	{
		if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
		if (e->tj.active) return fail(LPP_ERR_INVALID, std::string(who) + ": the t-J model (TjMultiOrb) is not supported, its operator strings are not built yet");
		if (conv != LPP_STRING_MANY_POINT)
			return fail(LPP_ERR_INVALID, std::string(who) + ": the Heisenberg basis has the many-point convention only (the labels of the measure convention are per fermion species)");
		return LPP_OK;
	}
	static lpp_status plan(int, int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t*, int L, int m, int, Plan& P)
	{
		const char* why = nullptr;
		return plan_status(plan_heis_string(nops, ops, sites, spins, L, m, P, &why), why);
	}
	static int64_t sector_size(int L, int m, int) { return heis_sector_size(L, m, 0); }
	static bool has_sector(const Plan&) { return true; } // (this basis has no "no sector": the plan refuses where the reference throws)
	static void new_sector(const Plan& P, int32_t* nup, int32_t* ndn) { *nup = P.m2, *ndn = 0; }
	static int64_t n_src(const Plan& P) { return P.n_src; }
	static int64_t n_dst(const Plan& P) { return P.n_dst; }
	static bool stays(const Plan& P, int m, int) { return !P.dead && P.m2 == m; } // Engine.h:382-383
	static double scale(const Plan&) { return 1.0; }
	static double reached(const Plan& P, int L, int m) { return (double)heis_string_touched(P, L, m); }

	// one launch; none for a dead string: z = 0 or z untouched
	static lpp_status apply(lpp_engine* e, const Plan& P, int L, int m, int, double fr, double fi, const void* d_src, void* d_dst, bool acc)
	{
		lpp_status st = check_vectors(e, fi, d_src, d_dst);
		if (st != LPP_OK) return st;
		if (P.dead) {
			if (!acc) HIP_TRY(hipMemsetAsync(d_dst, 0, e->esz * (size_t)P.n_dst, e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
			return LPP_OK;
		}
		Work W;
		if ((st = W.sector(e, L, P.m2, 1)) != LPP_OK) return st;
		ObsHeisStringApplyArgs A {};
		if ((st = W.fill(e, &P, 1, L, m, A.b, &A.src, &A.low)) != LPP_OK) return st;
		A.fr = fr;
		A.fi = fi;
		st = obs_launch(e, acc, P.n_dst, obs_heis_string_lds_bytes(A.b.nlo),
		                [&](int g, size_t lds, auto c, auto a) { k_obs_string_apply_heis<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
		if (st != LPP_OK) return st;
		HIP_TRY(hipStreamSynchronize(e->stream));
		return LPP_OK;
	}

	// One destination sector on the device: its runs, the two low tables and room for `slots` strings' entries per run.  The host copies stay until the
	// struct goes: the uploads are asynchronous.
	struct Work : DotOut {
		DevBuf runs, low, src;
		std::vector<ObsHeisRun> h_runs;
		std::vector<uint64_t> highs;
		std::vector<uint16_t> h_low; // word, then rank
		std::vector<int64_t> h_src;
		int64_t nruns = 0, n_dst = 0;
		int nlo = 0;
		ObsHeisStringDotArgs A;
		lpp_status sector(lpp_engine* e, int L, int m2, int slots)
		{
			std::vector<uint16_t> rank;
			if (!heis_string_runs(L, m2, true, h_runs, highs, h_low, rank))
				return fail(LPP_ERR_INVALID, "Heisenberg operator string: the sector has more than 2^22 runs of equal high part (the run table's limit)");
			nruns = (int64_t)highs.size();
			n_dst = h_runs.back().dst0;
			nlo = (int)h_low.size();
			h_low.insert(h_low.end(), rank.begin(), rank.end());
			h_src.assign((size_t)slots * (size_t)nruns, 0);
			HIP_TRY_MEM(runs.alloc(sizeof(ObsHeisRun) * h_runs.size()));
			HIP_TRY_MEM(low.alloc(sizeof(uint16_t) * h_low.size()));
			HIP_TRY_MEM(src.alloc(sizeof(int64_t) * h_src.size()));
			HIP_TRY(hipMemcpyAsync(runs.p, h_runs.data(), sizeof(ObsHeisRun) * h_runs.size(), hipMemcpyHostToDevice, e->stream));
			HIP_TRY(hipMemcpyAsync(low.p, h_low.data(), sizeof(uint16_t) * h_low.size(), hipMemcpyHostToDevice, e->stream));
			return LPP_OK;
		}
		// plans[0 .. ns) (none dead) of source sector m packed into the slots and uploaded; B.nlo = 0 where none of them has low-part work
		lpp_status fill(lpp_engine* e, const Plan* plans, int ns, int L, int m, ObsHeisStringBase& B, const int64_t** d_src, ObsHeisStringLow* d_low)
		{
			bool low_work = false;
			const char* why = nullptr;
			if (!heis_string_pack(plans, ns, L, m, highs, h_src, d_low, &low_work, &why)) return fail(LPP_ERR_INVALID, why);
			for (int s = 0; s < ns; s++) d_src[s] = (const int64_t*)src.p + (size_t)s * (size_t)nruns;
			HIP_TRY(hipMemcpyAsync(src.p, h_src.data(), sizeof(int64_t) * (size_t)ns * (size_t)nruns, hipMemcpyHostToDevice, e->stream));
			B = ObsHeisStringBase { (const ObsHeisRun*)runs.p, (const uint16_t*)low.p, (const uint16_t*)low.p + nlo, nruns, n_dst, low_work ? nlo : 0 };
			return LPP_OK;
		}
		lpp_status prepare(lpp_engine* e, int L, int m, int, int64_t nstrings)
		{
			lpp_status st = sector(e, L, m, kObsStringBatch);
			return st != LPP_OK ? st : alloc_out(e, n_dst, nstrings);
		}
		lpp_status load(lpp_engine* e, const Plan* plans, int ns, int L, int m, int)
		{
			A = ObsHeisStringDotArgs {};
			A.partial = (double*)part.p;
			A.ns = ns;
			return fill(e, plans, ns, L, m, A.b, A.src, A.low);
		}
		void launch(lpp_engine* e, const double* bra, const double* ket, double* d_out) const
		{
			const size_t lds = obs_heis_string_lds_bytes(A.b.nlo);
			with_flags([&](auto c) { k_obs_string_dot_heis<c><<<grid, kObsBlock, lds, e->stream>>>(bra, ket, A); }, e->is_complex);
			reduce(e, A.ns, d_out);
		}
	};
};

// the one-orbital t-J basis: a string is a few words, one 32-bit entry per destination down word and a program of pattern steps (plan and upload
// image: lpp_obs_tj_string_plan.h, kernels: lpp_obs_tj_string_kernels.h).  A hole-major engine is admitted: its resident states are kept in the
// basis order (lpp_engine_keep_states_tj), the order lpp_engine_two_point_tj reads them in as well.
struct TjStrings {
	typedef TjStringPlan Plan;
	static constexpr const char* kBadSector = ": bad sites / sector (nup + ndown <= sites <= 30)";
	static constexpr const char* kNotResident = ": (sites, nup, ndown) is not the sector of the resident states";
	static constexpr const char* kLeaves = ": a string that is identically zero, leads to no sector or leaves the sector launches nothing";

	static lpp_status refuse(const lpp_engine* e, const char* who, int conv)
	{
		if (multi(e)) return fail(LPP_ERR_STATE, std::string(who) + ": not on a partitioned (multi-rank) engine");
		if (conv != LPP_STRING_MANY_POINT)
			return fail(LPP_ERR_INVALID, std::string(who) + ": the t-J basis has the many-point convention only (RahulOperator on this basis is not restated)");
		return LPP_OK;
	}
	static lpp_status plan(int, int nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t*, int L, int nup, int ndn, Plan& P)
	{
		const char* why = nullptr;
		return plan_status(obs_string_plan_tj(nops, ops, sites, spins, L, nup, ndn, P, &why), why);
	}
	static int64_t sector_size(int L, int nup, int ndn) { return tj_sector_size(L, nup, ndn); }
	static bool has_sector(const Plan& P) { return P.has; }
	static void new_sector(const Plan& P, int32_t* nup, int32_t* ndn) { *nup = P.nup2, *ndn = P.ndn2; }
	static int64_t n_src(const Plan& P) { return P.n_up_src * P.n_dn_src; }
	static int64_t n_dst(const Plan& P) { return P.n_up_dst * P.n_dn_dst; }
	static bool stays(const Plan& P, int nup, int ndn) { return P.has && !P.dead && P.nup2 == nup && P.ndn2 == ndn; } // Engine.h:364, :382-383
	static double scale(const Plan&) { return 1.0; }
	static double reached(const Plan& P, int, int) { return (double)tj_string_touched(P); }

	// one launch; none for a dead string: z = 0 or z untouched
	static lpp_status apply(lpp_engine* e, const Plan& P, int, int, int, double fr, double fi, const void* d_src, void* d_dst, bool acc)
	{
		lpp_status st = check_vectors(e, fi, d_src, d_dst);
		if (st != LPP_OK) return st;
		if (P.dead) {
			if (!acc) HIP_TRY(hipMemsetAsync(d_dst, 0, e->esz * (size_t)n_dst(P), e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
			return LPP_OK;
		}
		if (n_dst(P) == 0) return LPP_OK;
		Work W;
		if ((st = W.sectors(e, P.L, P.nup, P.ndn, P.nup2, P.ndn2, 1)) != LPP_OK) return st;
		ObsTjStringApplyArgs A {};
		if ((st = W.fill(e, &P, 1, A.b, &A.ent, &A.up)) != LPP_OK) return st;
		A.fr = fr;
		A.fi = fi;
		st = obs_launch(e, acc, n_dst(P), obs_tj_string_lds_bytes(A.b),
		                [&](int g, size_t lds, auto c, auto a) { k_obs_string_apply_tj<c, a><<<g, kObsBlock, lds, e->stream>>>((double*)d_dst, (const double*)d_src, A); });
		if (st != LPP_OK) return st;
		HIP_TRY(hipStreamSynchronize(e->stream));
		return LPP_OK;
	}

	// One pair of sectors on the device: the destination's word lists, the source's rank tables and `slots` tables of down entries in one image.  The
	// fixed part goes up once, the entries of a batch with the batch.  The host copy stays until the struct goes: the uploads are asynchronous.
	struct Work : DotOut {
		DevBuf dev;
		std::vector<int32_t> img;
		TjStringImage G;
		ObsTjStringDotArgs A;
		lpp_status sectors(lpp_engine* e, int L, int nup, int ndn, int nup2, int ndn2, int slots)
		{
			const char* why = nullptr;
			if (!tj_string_image_begin(G, L, nup, ndn, nup2, ndn2, slots, img, &why)) return fail(LPP_ERR_INVALID, why);
			HIP_TRY_MEM(dev.alloc(4 * img.size()));
			HIP_TRY(hipMemcpyAsync(dev.p, img.data(), 4 * G.fixed(), hipMemcpyHostToDevice, e->stream));
			return LPP_OK;
		}
		// plans[0 .. ns) (none dead, all of the image's sectors) packed into the slots and uploaded
		lpp_status fill(lpp_engine* e, const Plan* plans, int ns, ObsTjStringBase& B, const int32_t** d_ent, ObsTjStringUp* d_up)
		{
			const char* why = nullptr;
			if (!tj_string_image_entries(G, plans, ns, img, &why)) return fail(LPP_ERR_INVALID, why);
			const int32_t* d = (const int32_t*)dev.p;
			int stage = 0, need_pat = 0;
			for (int s = 0; s < ns; s++) {
				d_ent[s] = d + G.entries(s);
				d_up[s] = plans[s].up;
				stage |= plans[s].up.changes;
				need_pat |= plans[s].up.n > 0;
			}
			HIP_TRY(hipMemcpyAsync((int32_t*)dev.p + G.entries(0), img.data() + G.entries(0), 4 * (G.entries(ns) - G.entries(0)), hipMemcpyHostToDevice, e->stream));
			B = ObsTjStringBase { (const uint32_t*)(d + G.down_words()), (const uint32_t*)(d + G.patterns()), d + G.hi_base(), (const uint16_t*)(d + G.lo_rank()), G.lb, G.nhi,
				                  G.nlo, stage, need_pat, G.n_up, G.n_dn, G.n_up_src };
			return LPP_OK;
		}
		lpp_status prepare(lpp_engine* e, int L, int nup, int ndn, int64_t nstrings)
		{
			lpp_status st = sectors(e, L, nup, ndn, nup, ndn, kObsStringBatch);
			return st != LPP_OK ? st : alloc_out(e, G.n_up * G.n_dn, nstrings);
		}
		lpp_status load(lpp_engine* e, const Plan* plans, int ns, int, int, int)
		{
			A = ObsTjStringDotArgs {};
			A.partial = (double*)part.p;
			A.ns = ns;
			return fill(e, plans, ns, A.b, A.ent, A.up);
		}
		void launch(lpp_engine* e, const double* bra, const double* ket, double* d_out) const
		{
			const size_t lds = obs_tj_string_lds_bytes(A.b);
			with_flags([&](auto c) { k_obs_string_dot_tj<c><<<grid, kObsBlock, lds, e->stream>>>(bra, ket, A); }, e->is_complex);
			reduce(e, A.ns, d_out);
		}
	};
};

// string s of a list planned on sector (L; nup, ndn)
template <typename F> lpp_status plan_of(int conv, const StringList& S, int s, int L, int nup, int ndn, typename F::Plan& P)
{
	const int64_t o = S.off[s];
	return F::plan(conv, (int)(S.off[s + 1] - o), S.ops + o, S.sites + o, S.spins + o, S.flags ? S.flags + o : nullptr, L, nup, ndn, P);
}

// result[2 s], result[2 s + 1] = re, im of conj(bra) . (string_s ket); 0 for a string the family does not launch (no sector, identically zero, or it
// ends in another sector).  kObsStringBatch strings per launch; the workspace of one batch is reused after a sync; one readback.
template <typename F> lpp_status many_point_dev(lpp_engine* e, int conv, const StringList& S, int L, int nup, int ndn, const double* bra, const double* ket, double* result)
{
	std::vector<typename F::Plan> plans;
	std::vector<int> slot; // the string of each launched plan
	std::vector<double> scale;
	typename F::Work W;
	bool ready = false;
	int launched = 0;
	auto flush = [&]() -> lpp_status {
		if (plans.empty()) return LPP_OK;
		lpp_status st = LPP_OK;
		if (!ready) {
			if ((st = W.prepare(e, L, nup, ndn, S.n)) != LPP_OK) return st;
			ready = true;
		} else {
			HIP_TRY(hipStreamSynchronize(e->stream)); // the launch that still reads the uploads of the batch before
		}
		if ((st = W.load(e, plans.data(), (int)plans.size(), L, nup, ndn)) != LPP_OK) return st;
		W.launch(e, bra, ket, (double*)W.out.p + 2 * launched);
		HIP_TRY(hipGetLastError());
		launched += (int)plans.size();
		plans.clear();
		return LPP_OK;
	};
	for (int s = 0; s < S.n; s++) {
		typename F::Plan P;
		lpp_status st = plan_of<F>(conv, S, s, L, nup, ndn, P);
		if (st != LPP_OK) return st;
		result[2 * s] = result[2 * s + 1] = 0.0;
		if (!F::stays(P, nup, ndn)) continue;
		scale.push_back(F::scale(P));
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
	for (size_t k = 0; k < (size_t)launched; k++) {
		result[2 * slot[k]] = scale[k] * h[2 * k];
		result[2 * slot[k] + 1] = scale[k] * h[2 * k + 1];
	}
	return LPP_OK;
}

// the checks the resident-state form, the host-vector form and the bench share, in this order; *n = the sector's size.  The bench says "bad argument"
// and takes one launch's strings
template <typename F> lpp_status many_point_front(lpp_engine* e, const char* who, bool args_ok, bool bench, int conv, const StringList& S, int L, int nup, int ndn, int64_t* n)
{
	if (!args_ok) return fail(LPP_ERR_INVALID, std::string(who) + (bench ? ": bad argument" : ": null argument"));
	lpp_status st = F::refuse(e, who, conv);
	if (st != LPP_OK) return st;
	if ((st = check_list(S, who)) != LPP_OK) return st;
	if (bench && (S.n < 1 || S.n > kObsStringBatch)) return fail(LPP_ERR_INVALID, std::string(who) + ": 1 to 8 strings (one launch)");
	if ((*n = F::sector_size(L, nup, ndn)) < 0) return fail(LPP_ERR_INVALID, std::string(who) + F::kBadSector);
	return LPP_OK;
}

// bra and ket of `bytes` bytes on the device, 16 spare bytes each: copies of two host vectors, or zeros where there are none
lpp_status stage_pair(lpp_engine* e, size_t bytes, const void* bra, const void* ket, DevBuf& db, DevBuf& dk)
{
	HIP_TRY_MEM(db.alloc(bytes + 16));
	HIP_TRY_MEM(dk.alloc(bytes + 16));
	if (bra) {
		HIP_TRY(hipMemcpyAsync(db.p, bra, bytes, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(dk.p, ket, bytes, hipMemcpyHostToDevice, e->stream));
	} else {
		HIP_TRY(hipMemsetAsync(db.p, 0, bytes + 16, e->stream));
		HIP_TRY(hipMemsetAsync(dk.p, 0, bytes + 16, e->stream));
	}
	return LPP_OK;
}

// lpp_engine_apply_string* (host == false: device vectors) and lpp_engine_apply_string*_host (host vectors staged around the launch)
template <typename F>
lpp_status apply_string_body(const std::string& who, bool host, lpp_engine* e, int32_t conv, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                             const int32_t* flags, int32_t L, int32_t nup, int32_t ndn, double fr, double fi, const void* src, void* dst, int32_t accumulate, int32_t* has,
                             int32_t* nup_new, int32_t* ndown_new)
{
	if (!e || !has || (host && (!src || !dst))) return fail(LPP_ERR_INVALID, who + ": null argument");
	*has = 0;
	lpp_status st = F::refuse(e, who.c_str(), conv);
	if (st != LPP_OK) return st;
	typename F::Plan P;
	if ((st = F::plan(conv, nops, ops, sites, spins, flags, L, nup, ndn, P)) != LPP_OK || !F::has_sector(P)) return st;
	*has = 1;
	int32_t n1 = 0, n2 = 0;
	F::new_sector(P, &n1, &n2);
	if (nup_new) *nup_new = n1;
	if (ndown_new) *ndown_new = n2;
	HIP_TRY(hipSetDevice(e->cfg.device));
	const auto run = [&](const void* d_src, void* d_dst) { return F::apply(e, P, L, nup, ndn, fr, fi, d_src, d_dst, accumulate != 0); };
	return host ? staged(e, e->esz * (size_t)F::n_src(P), e->esz * (size_t)F::n_dst(P), src, dst, accumulate, run) : run(src, dst);
}

template <typename F>
lpp_status many_point_body(const char* who, lpp_engine* e, int32_t conv, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                           const int32_t* flags, int32_t L, int32_t nup, int32_t ndn, int32_t bra_state, int32_t ket_state, double* result)
{
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	int64_t n = 0;
	lpp_status st = many_point_front<F>(e, who, e && result, false, conv, S, L, nup, ndn, &n);
	if (st != LPP_OK) return st;
	double *bra = nullptr, *ket = nullptr;
	if ((st = state_ptr(e, bra_state, who, &bra)) != LPP_OK) return st;
	if ((st = state_ptr(e, ket_state, who, &ket)) != LPP_OK) return st;
	if (e->resident_len != n) return fail(LPP_ERR_INVALID, std::string(who) + F::kNotResident);
	HIP_TRY(hipSetDevice(e->cfg.device));
	return many_point_dev<F>(e, conv, S, L, nup, ndn, bra, ket, result);
}

template <typename F>
lpp_status many_point_host_body(const char* who, lpp_engine* e, int32_t conv, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                const int32_t* spins, const int32_t* flags, int32_t L, int32_t nup, int32_t ndn, const void* bra, const void* ket, double* result)
{
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	int64_t n = 0;
	lpp_status st = many_point_front<F>(e, who, e && result && bra && ket, false, conv, S, L, nup, ndn, &n);
	if (st != LPP_OK) return st;
	HIP_TRY(hipSetDevice(e->cfg.device));
	DevBuf db, dk;
	if ((st = stage_pair(e, e->esz * (size_t)n, bra, ket, db, dk)) != LPP_OK) return st;
	st = many_point_dev<F>(e, conv, S, L, nup, ndn, (const double*)db.p, (const double*)dk.p, result);
	HIP_TRY(hipStreamSynchronize(e->stream));
	return st;
}

// the bracket kernel and its reduction on one batch of strings that all stay in the sector, zeroed vectors
template <typename F>
lpp_status bench_string_dot_body(const char* who, lpp_engine* e, int32_t conv, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                 const int32_t* spins, const int32_t* flags, int32_t L, int32_t nup, int32_t ndn, int32_t warmup, int32_t iters, double* ms_per_launch,
                                 double* model_bytes)
{
	const StringList S { nstrings, offsets, ops, sites, spins, flags };
	int64_t n = 0;
	lpp_status st = many_point_front<F>(e, who, e && ms_per_launch && iters >= 1 && warmup >= 0, true, conv, S, L, nup, ndn, &n);
	if (st != LPP_OK) return st;
	std::vector<typename F::Plan> plans((size_t)nstrings);
	double reached = 0;
	for (int s = 0; s < nstrings; s++) {
		if ((st = plan_of<F>(conv, S, s, L, nup, ndn, plans[(size_t)s])) != LPP_OK) return st;
		if (!F::stays(plans[(size_t)s], nup, ndn)) return fail(LPP_ERR_INVALID, std::string(who) + F::kLeaves);
		reached += F::reached(plans[(size_t)s], L, nup);
	}
	HIP_TRY(hipSetDevice(e->cfg.device));
	DevBuf db, dk;
	if ((st = stage_pair(e, e->esz * (size_t)n, nullptr, nullptr, db, dk)) != LPP_OK) return st;
	typename F::Work W;
	if ((st = W.prepare(e, L, nup, ndn, nstrings)) != LPP_OK) return st;
	if ((st = W.load(e, plans.data(), nstrings, L, nup, ndn)) != LPP_OK) return st;
	st = timed_steps(e, warmup, iters, ms_per_launch, [&] {
		W.launch(e, (const double*)db.p, (const double*)dk.p, (double*)W.out.p);
		return LPP_OK;
	});
	if (st != LPP_OK) return st;
	// bra read once, one ket element per string and destination it reaches (the tables or run entries stay in L2)
	if (model_bytes) *model_bytes = (double)e->esz * ((double)n + reached);
	return LPP_OK;
}

// hasNewParts of the basis for the host (lpp_obs_new_parts*): *has = 0 where the operator leads to no sector
lpp_status new_parts_body(const ObsBasis& B, const std::string& who, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new,
                          int32_t* ndown_new)
{
	if (!has) return fail(LPP_ERR_INVALID, who + ": null argument");
	*has = 0;
	if (spin != LPP_SPIN_UP && spin != LPP_SPIN_DOWN) return fail(LPP_ERR_INVALID, who + ": bad spin");
	if (!B.counts_ok(nsites, nup, ndown)) return fail(LPP_ERR_INVALID, who + ": bad sector");
	if (op == LPP_OP_SZ && B.sz_has_no_parts) return LPP_OK; // HubbardOneOrbital.h:101-102, Heisenberg.h:122-123
	// the reference throws: HubbardOneOrbital.h:104-108, for n and sz TjMultiOrb.h:154-158, for all but splus / sminus Heisenberg.h:129-133
	if (!needs_new_basis(op) || (!B.fermions && (op == LPP_OP_C || op == LPP_OP_CDAGGER))) return fail(LPP_ERR_INVALID, "hasNewParts: unsupported operator");
	int n1 = 0, n2 = 0;
	if (!B.new_parts(op, spin, nsites, nup, B.reads_ndown ? ndown : 0, &n1, &n2))
		return B.no_sector_throws ? fail(LPP_ERR_INVALID, "hasNewParts: S+ to all ups or S- to all downs") : LPP_OK; // the reference throws (Heisenberg.h:239)
	*has = 1;
	if (B.spin_args) n1 = n2, n2 = 0; // (twiceS, szPlusConst') is reported as (szPlusConst', 0)
	if (nup_new) *nup_new = n1;
	if (ndown_new) *ndown_new = n2;
	return LPP_OK;
}

// keep_tj: the solve lets a hole-major engine through (lanczos_impl)
lpp_status keep_states_body(const std::string& who, lpp_engine* e, int32_t k, bool keep_tj)
{
	if (!e || k < 0) return fail(LPP_ERR_INVALID, who + ": bad argument");
	if (e->active) return fail(LPP_ERR_STATE, who + ": a Lanczos run is active");
	if (k > 0) {
		lpp_status st = refuse(e, who.c_str(), keep_tj);
		if (st != LPP_OK) return st;
	}
	e->keep_k = k;
	e->keep_tj = keep_tj;
	return LPP_OK;
}

} // namespace

namespace lpp {
void free_obs(lpp_engine* e)
{
	if (e->obs) {
		delete (ObsCache*)e->obs; // the plans free their tables
		e->obs = nullptr;
	}
	if (e->resident) (void)hipFree(e->resident);
	e->resident = nullptr;
	e->resident_n = e->resident_cap = 0;
}
} // namespace lpp

extern "C" {

// One entry point per family over one body(basis, name, arguments...): the Hubbard product basis, the one-orbital t-J basis, the S = 1/2 Heisenberg basis
// and the spin-S Heisenberg digit basis, whose (nup, ndown) are (twiceS, szPlusConst)
#define OBS_ENTRY(body, hubbard, tj, heis, heis_spin, params, ...)                \
	lpp_status hubbard params { return body(kHubbard, #hubbard, __VA_ARGS__); } \
	lpp_status tj params { return body(kTj, #tj, __VA_ARGS__); }                \
	lpp_status heis params { return body(kHeis, #heis, __VA_ARGS__); }          \
	lpp_status heis_spin params { return body(kHeisSpin, #heis_spin, __VA_ARGS__); }

lpp_status lpp_obs_plan(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                        int64_t* n_up_dst, int64_t* n_down_dst, int32_t* table_up, int32_t* table_down)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan: null argument");
	ObsPlan P;
	bool h = false;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan(op, site, spin, nsites, nup, ndown, &h, P, &why), why);
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

lpp_status lpp_obs_sum_plan(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, const double* w_re, const double* w_im, int32_t* has, int32_t* nup_new,
                            int32_t* ndown_new, int64_t* n_dst, int32_t* width, int64_t* src_index, int32_t* site, double* fac_re, double* fac_im)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_sum_plan: null argument");
	ObsSumPlan P;
	bool h = false;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_sum_plan(op, spin, nsites, nup, ndown, &h, P, &why), why);
	if (st != LPP_OK) return st;
	*has = h ? 1 : 0;
	if (!h) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (n_dst) *n_dst = P.n_up_dst * P.n_dn_dst;
	if (width) *width = obs_sum_width(P);
	if (src_index || site || fac_re || fac_im) {
		if (!src_index || !site || !fac_re || !fac_im || !w_re) return fail(LPP_ERR_INVALID, "lpp_obs_sum_plan: the expansion takes all four tables and the weights");
		obs_sum_expand(P, w_re, w_im, src_index, site, fac_re, fac_im);
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
	lpp_status st = HubbardStrings::plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P);
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


lpp_status lpp_obs_string_plan_heis(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                                    int32_t nup, int32_t ndown, int32_t* nup_new, int32_t* dead, uint64_t* flip, uint64_t* need, uint64_t* want, uint64_t* zmask, int32_t* sign,
                                    int32_t* low_bits, int64_t* n_dst, int64_t* action)
{
	if (convention != LPP_STRING_MANY_POINT) return fail(LPP_ERR_INVALID, "lpp_obs_string_plan_heis: the Heisenberg basis has the many-point convention only");
	HeisStringPlan P;
	lpp_status st = HeisStrings::plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P);
	if (st != LPP_OK) return st;
	if (nup_new) *nup_new = P.m2;
	if (dead) *dead = P.dead ? 1 : 0;
	if (flip) *flip = P.flip;
	if (need) *need = P.need;
	if (want) *want = P.want;
	if (zmask) *zmask = P.zmask;
	if (sign) *sign = P.sign;
	if (low_bits) *low_bits = P.lb;
	if (n_dst) *n_dst = P.n_dst;
	if (action) {
		std::vector<ObsHeisRun> runs;
		std::vector<uint64_t> highs;
		std::vector<uint16_t> word, rank;
		std::vector<int64_t> src;
		if (!heis_string_runs(nsites, P.m2, true, runs, highs, word, rank))
			return fail(LPP_ERR_INVALID, "lpp_obs_string_plan_heis: the sector has more than 2^22 runs of equal high part (the run table's limit)");
		heis_string_sources(P, nsites, nup, highs, src);
		heis_string_expand(P, runs, src, word, rank, action);
	}
	return LPP_OK;
}

lpp_status lpp_obs_string_plan_tj(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                                  int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new, int32_t* dead, uint32_t* words, int32_t* sign, int64_t* n_dst,
                                  int64_t* touched, int64_t* action)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_string_plan_tj: null argument");
	*has = 0;
	if (convention != LPP_STRING_MANY_POINT) return fail(LPP_ERR_INVALID, "lpp_obs_string_plan_tj: the t-J basis has the many-point convention only");
	TjStringPlan P;
	lpp_status st = TjStrings::plan(convention, nops, ops, sites, spins, flags, nsites, nup, ndown, P);
	if (st != LPP_OK) return st;
	*has = P.has ? 1 : 0;
	if (!P.has) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (dead) *dead = P.dead ? 1 : 0;
	if (words) {
		const uint32_t w[7] = { P.flip_up, P.flip_dn, P.touched, P.want_up, P.want_dn, P.par_up, P.par_dn };
		std::memcpy(words, w, sizeof(w));
	}
	if (sign) *sign = P.sign;
	if (n_dst) *n_dst = P.n_up_dst * P.n_dn_dst;
	if (touched) *touched = tj_string_touched(P);
	if (action) {
		const char* why = nullptr;
		if (!tj_string_expand(P, action, nullptr, &why)) return fail(LPP_ERR_INVALID, why);
	}
	return LPP_OK;
}

// One entry point per string family over one body<family>(name, arguments...): the Hubbard product basis, the S = 1/2 Heisenberg basis, the
// one-orbital t-J basis
#define STRING_ENTRY(body, hubbard, heis, tj, params, ...)                             \
	lpp_status hubbard params { return body<HubbardStrings>(#hubbard, __VA_ARGS__); } \
	lpp_status heis params { return body<HeisStrings>(#heis, __VA_ARGS__); }          \
	lpp_status tj params { return body<TjStrings>(#tj, __VA_ARGS__); }

STRING_ENTRY(apply_string_body, lpp_engine_apply_string, lpp_engine_apply_string_heis, lpp_engine_apply_string_tj,
             (lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup,
              int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has, int32_t* nup_new, int32_t* ndown_new),
             false, e, convention, nops, ops, sites, spins, flags, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate, has, nup_new, ndown_new)
STRING_ENTRY(apply_string_body, lpp_engine_apply_string_host, lpp_engine_apply_string_heis_host, lpp_engine_apply_string_tj_host,
             (lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup,
              int32_t ndown, double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has, int32_t* nup_new, int32_t* ndown_new),
             true, e, convention, nops, ops, sites, spins, flags, nsites, nup, ndown, factor_re, factor_im, src, dst, accumulate, has, nup_new, ndown_new)
STRING_ENTRY(many_point_body, lpp_engine_many_point, lpp_engine_many_point_heis, lpp_engine_many_point_tj,
             (lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
              int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, double* result),
             e, convention, nstrings, offsets, ops, sites, spins, flags, nsites, nup, ndown, bra_state, ket_state, result)
STRING_ENTRY(many_point_host_body, lpp_engine_many_point_host, lpp_engine_many_point_heis_host, lpp_engine_many_point_tj_host,
             (lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
              int32_t nsites, int32_t nup, int32_t ndown, const void* bra, const void* ket, double* result),
             e, convention, nstrings, offsets, ops, sites, spins, flags, nsites, nup, ndown, bra, ket, result)
STRING_ENTRY(bench_string_dot_body, lpp_engine_bench_string_dot, lpp_engine_bench_string_dot_heis, lpp_engine_bench_string_dot_tj,
             (lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
              int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes),
             e, convention, nstrings, offsets, ops, sites, spins, flags, nsites, nup, ndown, warmup, iters, ms_per_launch, model_bytes)

lpp_status lpp_obs_plan_tj(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                           int64_t* n_dst, int64_t* action)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan_tj: null argument");
	ObsTjPlan P;
	bool h = false;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_tj(op, site, spin, nsites, nup, ndown, &h, P, &why), why);
	if (st != LPP_OK) return st;
	*has = h ? 1 : 0;
	if (!h) return LPP_OK;
	if (nup_new) *nup_new = P.nup2;
	if (ndown_new) *ndown_new = P.ndn2;
	if (n_dst) *n_dst = P.n_up_dst * P.n_dn_dst;
	if (action) tj_expand(P, action, nullptr);
	return LPP_OK;
}

lpp_status lpp_obs_plan_heis(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                             int64_t* n_dst, int32_t* low_bits, int64_t* action)
{
	(void)ndown;
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan_heis: null argument");
	*has = 0;
	ObsHeisPlan P;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_heis(op, site, spin, nsites, nup, P, &why), why);
	if (st != LPP_OK) return st;
	*has = 1;
	if (nup_new) *nup_new = P.m2;
	if (ndown_new) *ndown_new = 0;
	if (n_dst) *n_dst = P.n_dst;
	if (low_bits) *low_bits = P.lb;
	if (action) heis_expand(P, action, nullptr);
	return LPP_OK;
}

lpp_status lpp_obs_plan_heis_spin(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t* has, int32_t* szPlusConst_new,
                                  int64_t* n_dst, int32_t* low_digits, int64_t* action, double* coef)
{
	if (!has) return fail(LPP_ERR_INVALID, "lpp_obs_plan_heis_spin: null argument");
	*has = 0;
	ObsHeisSpinPlan P;
	const char* why = nullptr;
	lpp_status st = plan_status(obs_plan_heis_spin(op, site, spin, nsites, twiceS, szPlusConst, P, &why), why);
	if (st != LPP_OK) return st;
	*has = 1;
	if (szPlusConst_new) *szPlusConst_new = P.m2;
	if (n_dst) *n_dst = P.n_dst;
	if (low_digits) *low_digits = P.lb;
	if (action || coef) heis_spin_expand(P, action, coef, nullptr);
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

OBS_ENTRY(apply_operator_body, lpp_engine_apply_operator, lpp_engine_apply_operator_tj, lpp_engine_apply_operator_heis, lpp_engine_apply_operator_heis_spin,
          (lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst,
           int32_t accumulate, int32_t* has),
          e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, d_src, d_dst, accumulate, has)
OBS_ENTRY(apply_operator_host_body, lpp_engine_apply_operator_host, lpp_engine_apply_operator_tj_host, lpp_engine_apply_operator_heis_host,
          lpp_engine_apply_operator_heis_spin_host,
          (lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* src, void* dst,
           int32_t accumulate, int32_t* has),
          e, op, site, spin, nsites, nup, ndown, factor_re, factor_im, src, dst, accumulate, has)
OBS_ENTRY(bench_operator_body, lpp_engine_bench_operator, lpp_engine_bench_operator_tj, lpp_engine_bench_operator_heis, lpp_engine_bench_operator_heis_spin,
          (lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters, double* ms_per_launch,
           double* model_bytes),
          e, op, site, spin, nsites, nup, ndown, warmup, iters, ms_per_launch, model_bytes)
OBS_ENTRY(new_parts_body, lpp_obs_new_parts, lpp_obs_new_parts_tj, lpp_obs_new_parts_heis, lpp_obs_new_parts_heis_spin,
          (int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new), op, spin, nsites, nup, ndown, has, nup_new,
          ndown_new)

lpp_status lpp_engine_keep_states(lpp_engine* e, int32_t k) { return keep_states_body("lpp_engine_keep_states", e, k, false); }
lpp_status lpp_engine_keep_states_tj(lpp_engine* e, int32_t k) { return keep_states_body("lpp_engine_keep_states_tj", e, k, true); }

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

OBS_ENTRY(two_point_body, lpp_engine_two_point, lpp_engine_two_point_tj, lpp_engine_two_point_heis, lpp_engine_two_point_heis_spin,
          (lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, void* result, void* trace),
          e, op, spin1, spin2, nsites, nup, ndown, bra_state, ket_state, result, trace)
OBS_ENTRY(spectral_body, lpp_engine_spectral_decomposition, lpp_engine_spectral_decomposition_tj, lpp_engine_spectral_decomposition_heis,
          lpp_engine_spectral_decomposition_heis_spin,
          (lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign, int32_t nsites, int32_t nup, int32_t ndown,
           double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats),
          e, state, sector, op, isite, jsite, spin, isign, nsites, nup, ndown, weight, nsteps, a, b, stats)

OBS_ENTRY(apply_sum_body, lpp_engine_apply_operator_sum, lpp_engine_apply_operator_sum_tj, lpp_engine_apply_operator_sum_heis,
          lpp_engine_apply_operator_sum_heis_spin,
          (lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re, const double* w_im, const void* d_src,
           void* d_dst, int32_t accumulate, int32_t* has),
          e, op, spin, nsites, nup, ndown, nweights, w_re, w_im, d_src, d_dst, accumulate, has)
OBS_ENTRY(apply_sum_host_body, lpp_engine_apply_operator_sum_host, lpp_engine_apply_operator_sum_tj_host, lpp_engine_apply_operator_sum_heis_host,
          lpp_engine_apply_operator_sum_heis_spin_host,
          (lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re, const double* w_im, const void* src,
           void* dst, int32_t accumulate, int32_t* has, int64_t* n_dst),
          e, op, spin, nsites, nup, ndown, nweights, w_re, w_im, src, dst, accumulate, has, n_dst)
OBS_ENTRY(bench_sum_body, lpp_engine_bench_operator_sum, lpp_engine_bench_operator_sum_tj, lpp_engine_bench_operator_sum_heis,
          lpp_engine_bench_operator_sum_heis_spin,
          (lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re, const double* w_im, int32_t accumulate,
           int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes),
          e, op, spin, nsites, nup, ndown, nweights, w_re, w_im, accumulate, warmup, iters, ms_per_launch, model_bytes)
OBS_ENTRY(sum_norm2_body, lpp_engine_sum_norm2, lpp_engine_sum_norm2_tj, lpp_engine_sum_norm2_heis, lpp_engine_sum_norm2_heis_spin,
          (lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re, const double* w_im,
           double* norm2, int32_t* has),
          e, state, op, spin, nsites, nup, ndown, nweights, w_re, w_im, norm2, has)
OBS_ENTRY(spectral_sum_body, lpp_engine_spectral_decomposition_sum, lpp_engine_spectral_decomposition_sum_tj, lpp_engine_spectral_decomposition_sum_heis,
          lpp_engine_spectral_decomposition_sum_heis_spin,
          (lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
           const double* w_im, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats),
          e, state, sector, op, spin, nsites, nup, ndown, nweights, w_re, w_im, weight, nsteps, a, b, stats)

} // extern "C"
