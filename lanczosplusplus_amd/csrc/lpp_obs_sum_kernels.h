// lpp_obs_sum_kernels.h -- a site-weighted sum of one-site operators of the Hubbard product basis applied to a device vector in one launch:
//     z (+)= sum_r f_r O_r src        (f_r: up to 30 complex weights in the kernel arguments; tables: lpp_obs_sum_plan.h)
// the modified state of the momentum-resolved quantities, c_k = sum_r e^{ikr} c_r and the like.  Destination driven like k_obs_apply
// (lpp_obs_kernels.h): a lane owns one 16-byte unit of z and writes it once with a non-temporal store, no atomics, one 64-bit division per tile.
//   k_obs_sum_move_up / _down (one body, obs_sum_move_body<.., DOWN>)   c / cdagger: z[du,dd] (+)= sum_{k<W} f[site_k] sign_k src[source_k], added in ascending k (= ascending site) from 0, so a value
//                    does not depend on the grid.  DOWN = false: the table is indexed by du and the gathers stay inside the source block of N_up_src
//                    contiguous elements (L1 / L2).  DOWN = true: the table is indexed by dd -- a lane reads an entry once for both of its elements
//                    where they share dd -- and the W sources are the contiguous streams src[du + sd_k N_up].
//   k_obs_sum_coef   c[word] = sum_{r in word} f_r per species word, ascending site (obs_sum_coef on the host)
//   k_obs_sum_diag   n / sz: z[du,dd] (+)= (alpha cu[du] + beta cd[dd]) src[du,dd], a stream with two small coefficient tables
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_obs_heis_kernels.h"
#include "lpp_obs_kernels.h"

namespace lpp {

constexpr int kObsSumSites = 30;

struct ObsSumWeights {
	double re[kObsSumSites], im[kObsSumSites];
};

struct ObsSumMoveArgs {
	const int32_t* tab; // W * n entries, k-major: +-(source rank + 1) of the moved species
	const uint8_t* site; // W * n: the site whose weight applies
	int64_t n; // destination words of the moved species
	int W;
	int64_t n_up_dst, n_dn_dst, n_up_src;
	ObsSumWeights w;
};

// the weights into LDS: a lane picks them by a table entry, and arguments indexed per lane would go through scratch
__device__ __forceinline__ void obs_sum_stage_weights(const ObsSumWeights& w, double* s_re, double* s_im)
{
	if (threadIdx.x == 0) {
#pragma unroll
		for (int i = 0; i < kObsSumSites; i++) {
			s_re[i] = w.re[i];
			s_im[i] = w.im[i];
		}
	}
	__syncthreads();
}

// the W terms of destination (du, dd), in ascending k
template <bool CPLX, bool DOWN>
__device__ __forceinline__ void obs_sum_terms(const ObsSumMoveArgs& A, const double* __restrict__ src, const double* s_re, const double* s_im, uint32_t du, int64_t dd,
                                              double& re, double& im)
{
	const int64_t d = DOWN ? dd : (int64_t)du;
	re = 0.0;
	im = 0.0;
	for (int k = 0; k < A.W; k++) {
		const int64_t q = (int64_t)k * A.n + d;
		const int32_t t = A.tab[q];
		const int r = A.site[q];
		const int64_t sr = (int64_t)(t < 0 ? -t : t) - 1;
		const int64_t s = DOWN ? (int64_t)du + sr * A.n_up_src : sr + dd * A.n_up_src;
		const double fr = t < 0 ? -s_re[r] : s_re[r];
		if (CPLX) {
			const double fi = t < 0 ? -s_im[r] : s_im[r];
			const double2 v = ((const double2*)src)[s];
			re += fr * v.x - fi * v.y;
			im += fr * v.y + fi * v.x;
		} else {
			re += fr * src[s];
		}
	}
}

// dst: n_up_dst * n_dn_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (every destination has W >= 1 sources)
template <bool CPLX, bool ACC, bool DOWN> __device__ __forceinline__ void obs_sum_move_body(double* __restrict__ dst, const double* __restrict__ src, const ObsSumMoveArgs& A)
{
	__shared__ double s_re[32], s_im[32];
	obs_sum_stage_weights(A.w, s_re, s_im);
	const int64_t n_dst = A.n_up_dst * A.n_dn_dst;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const uint32_t nup = (uint32_t)A.n_up_dst;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = CPLX ? u0 : 2 * u0; // first element of the tile: one 64-bit division per tile, 32-bit ones per lane
		const int64_t dd0 = e0 / A.n_up_dst;
		const uint32_t du0 = (uint32_t)(e0 - dd0 * A.n_up_dst);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const uint32_t t = (uint32_t)(r * kObsBlock + threadIdx.x);
			const int64_t u = u0 + t;
			if (u >= units) continue;
			double2* const p = (double2*)dst + u;
			if (CPLX) {
				const uint32_t rr = du0 + t, q = rr / nup;
				double re, im;
				obs_sum_terms<true, DOWN>(A, src, s_re, s_im, rr - q * nup, dd0 + q, re, im);
				if (ACC) {
					const double2 o = *p;
					re += o.x;
					im += o.y;
				}
				__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
			} else {
				const uint32_t r0 = du0 + 2 * t, q0 = r0 / nup, r1 = r0 + 1, q1 = r1 / nup;
				const bool two = 2 * u + 1 < n_dst; // an odd length ends in half a unit
				double v0, v1 = 0.0, dummy;
				if (DOWN && two && q0 == q1) { // one table entry serves both elements: the two streams are read side by side
					const uint32_t du = r0 - q0 * nup;
					const int64_t dd = dd0 + q0;
					v0 = 0.0;
					for (int k = 0; k < A.W; k++) {
						const int64_t q = (int64_t)k * A.n + dd;
						const int32_t e = A.tab[q];
						const int s = A.site[q];
						const int64_t sr = (int64_t)(e < 0 ? -e : e) - 1;
						const double f = e < 0 ? -s_re[s] : s_re[s];
						const double* const a = src + (int64_t)du + sr * A.n_up_src;
						v0 += f * a[0];
						v1 += f * a[1];
					}
				} else {
					obs_sum_terms<false, DOWN>(A, src, s_re, s_im, r0 - q0 * nup, dd0 + q0, v0, dummy);
					if (two) obs_sum_terms<false, DOWN>(A, src, s_re, s_im, r1 - q1 * nup, dd0 + q1, v1, dummy);
				}
				if (ACC) {
					if (two) {
						const double2 o = *p;
						v0 += o.x;
						v1 += o.y;
					} else {
						v0 += p->x;
					}
				}
				if (two) {
					__builtin_nontemporal_store(obs_v2 { v0, v1 }, (obs_v2*)p);
				} else {
					p->x = v0;
				}
			}
		}
	}
}

template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_sum_move_up(double* __restrict__ dst, const double* __restrict__ src, const ObsSumMoveArgs A)
{
	obs_sum_move_body<CPLX, ACC, false>(dst, src, A);
}
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_sum_move_down(double* __restrict__ dst, const double* __restrict__ src, const ObsSumMoveArgs A)
{
	obs_sum_move_body<CPLX, ACC, true>(dst, src, A);
}

// c[i] = sum_{r in words[i]} f_r, ascending site from 0; out: n values of the engine's dtype
template <bool CPLX> __global__ __launch_bounds__(kObsBlock) void k_obs_sum_coef(const uint32_t* __restrict__ words, int64_t n, double* __restrict__ out, const ObsSumWeights w)
{
	__shared__ double s_re[32], s_im[32];
	obs_sum_stage_weights(w, s_re, s_im);
	for (int64_t i = (int64_t)blockIdx.x * kObsBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kObsBlock) {
		double re = 0.0, im = 0.0;
		for (uint32_t m = words[i]; m; m &= m - 1) {
			const int r = __builtin_ctz(m);
			re += s_re[r];
			if (CPLX) im += s_im[r];
		}
		if (CPLX) {
			out[2 * i] = re;
			out[2 * i + 1] = im;
		} else {
			out[i] = re;
		}
	}
}

struct ObsSumDiagArgs {
	const double *cu, *cd; // n_up / n_dn coefficients of the engine's dtype
	int64_t n_up, n_dn;
	double alpha, beta;
};

template <bool CPLX> __device__ __forceinline__ void obs_sum_diag_el(const ObsSumDiagArgs& A, const double* __restrict__ src, uint32_t du, int64_t dd, double& re, double& im)
{
	const int64_t s = (int64_t)du + dd * A.n_up;
	if (CPLX) {
		const double2 a = ((const double2*)A.cu)[du], b = ((const double2*)A.cd)[dd], v = ((const double2*)src)[s];
		const double fr = A.alpha * a.x + A.beta * b.x, fi = A.alpha * a.y + A.beta * b.y;
		re = fr * v.x - fi * v.y;
		im = fr * v.y + fi * v.x;
	} else {
		re = (A.alpha * A.cu[du] + A.beta * A.cd[dd]) * src[s];
		im = 0.0;
	}
}

template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_sum_diag(double* __restrict__ dst, const double* __restrict__ src, const ObsSumDiagArgs A)
{
	const int64_t n_dst = A.n_up * A.n_dn;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const uint32_t nup = (uint32_t)A.n_up;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = CPLX ? u0 : 2 * u0;
		const int64_t dd0 = e0 / A.n_up;
		const uint32_t du0 = (uint32_t)(e0 - dd0 * A.n_up);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const uint32_t t = (uint32_t)(r * kObsBlock + threadIdx.x);
			const int64_t u = u0 + t;
			if (u >= units) continue;
			double2* const p = (double2*)dst + u;
			if (CPLX) {
				const uint32_t rr = du0 + t, q = rr / nup;
				double re, im;
				obs_sum_diag_el<true>(A, src, rr - q * nup, dd0 + q, re, im);
				if (ACC) {
					const double2 o = *p;
					re += o.x;
					im += o.y;
				}
				__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
			} else {
				const uint32_t r0 = du0 + 2 * t, q0 = r0 / nup, r1 = r0 + 1, q1 = r1 / nup;
				const bool two = 2 * u + 1 < n_dst; // an odd length ends in half a unit
				double v0, v1 = 0.0, dummy;
				obs_sum_diag_el<false>(A, src, r0 - q0 * nup, dd0 + q0, v0, dummy);
				if (two) obs_sum_diag_el<false>(A, src, r1 - q1 * nup, dd0 + q1, v1, dummy);
				if (ACC) {
					if (two) {
						const double2 o = *p;
						v0 += o.x;
						v1 += o.y;
					} else {
						v0 += p->x;
					}
				}
				if (two) {
					__builtin_nontemporal_store(obs_v2 { v0, v1 }, (obs_v2*)p);
				} else {
					p->x = v0;
				}
			}
		}
	}
}

// ---- the S = 1/2 Heisenberg basis: sum_r f_r sz_r with the raw sz = 1 - 2 bit, diagonal -------------------------------------------------------
// The element factor is F - 2 (hi[run] + sum_{low bits set} f_r), F = sum_r f_r.  The kernel walks the run table of the one-site plans
// (lpp_obs_heis_plan.h: any site's table has the runs and the low words): hi[run] = the weights of the run's high part, one value per run made by
// k_obs_sum_hi_heis before the launch; the low part's sum runs over the at most 14 low bits of the element's word, ascending.

struct ObsSumHeisArgs {
	const ObsHeisRun* runs; // nruns + 1 entries
	const uint16_t* word; // nlo low words ordered by (popcount, rank)
	const double* hi; // nruns values of the engine's dtype
	int nlo;
	int64_t nruns, n_dst;
	double F_re, F_im;
	ObsSumWeights w; // the low sites' weights are read
};

// hi[k] = sum of f_{lb + b} over the set bits b of highs[k], ascending
template <bool CPLX>
__global__ __launch_bounds__(kObsBlock) void k_obs_sum_hi_heis(const uint64_t* __restrict__ highs, int64_t n, int lb, double* __restrict__ out, const ObsSumWeights w)
{
	__shared__ double s_re[32], s_im[32];
	obs_sum_stage_weights(w, s_re, s_im);
	for (int64_t i = (int64_t)blockIdx.x * kObsBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kObsBlock) {
		double re = 0.0, im = 0.0;
		for (uint64_t m = highs[i]; m; m &= m - 1) {
			const int r = lb + __builtin_ctzll(m); // below kObsSumSites: the driver admits no longer chain
			re += s_re[r];
			if (CPLX) im += s_im[r];
		}
		if (CPLX) {
			out[2 * i] = re;
			out[2 * i + 1] = im;
		} else {
			out[i] = re;
		}
	}
}

template <bool CPLX>
__device__ __forceinline__ void obs_sum_heis_el(const ObsSumHeisArgs& A, const double* __restrict__ src, const uint16_t* word, const double* s_re, const double* s_im, int64_t run,
                                                int64_t el, double& re, double& im)
{
	const ObsHeisRun R = A.runs[run];
	double lr = 0.0, li = 0.0;
	for (uint32_t m = word[R.wbase + (int32_t)(el - R.dst0)]; m; m &= m - 1) {
		const int r = __builtin_ctz(m);
		lr += s_re[r];
		if (CPLX) li += s_im[r];
	}
	if (CPLX) {
		const double2 h = ((const double2*)A.hi)[run], v = ((const double2*)src)[el];
		const double fr = A.F_re - 2.0 * (h.x + lr), fi = A.F_im - 2.0 * (h.y + li);
		re = fr * v.x - fi * v.y;
		im = fr * v.y + fi * v.x;
	} else {
		re = (A.F_re - 2.0 * (A.hi[run] + lr)) * src[el];
		im = 0.0;
	}
}

inline size_t obs_sum_heis_lds_bytes(int nlo) { return sizeof(uint16_t) * (size_t)nlo; }

// dst, src: n_dst elements; dynamic LDS: obs_sum_heis_lds_bytes(nlo).  Tiles, units, run search and the closing half unit as in k_obs_apply_heis.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_sum_sz_heis(double* __restrict__ dst, const double* __restrict__ src, const ObsSumHeisArgs A)
{
	extern __shared__ uint16_t obs_sum_heis_lds[];
	__shared__ double s_re[32], s_im[32];
	uint16_t* const word = obs_sum_heis_lds;
	for (int i = threadIdx.x; i < A.nlo; i += kObsBlock) word[i] = A.word[i];
	obs_sum_stage_weights(A.w, s_re, s_im); // (ends in the barrier)
	const int64_t n_dst = A.n_dst;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	constexpr int kPer = CPLX ? 1 : 2;
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = kPer * u0;
		const int64_t e1 = (e0 + kPer * kObsTile < n_dst ? e0 + kPer * kObsTile : n_dst) - 1;
		const int64_t k0 = obs_heis_run_of(A.runs, 0, A.nruns - 1, e0);
		const int64_t k1 = obs_heis_run_of(A.runs, k0, (k0 + (e1 - e0) < A.nruns - 1 ? k0 + (e1 - e0) : A.nruns - 1), e1);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const int64_t u = u0 + (r * kObsBlock + (int)threadIdx.x);
			if (u >= units) continue;
			double2* const p = (double2*)dst + u;
			const int64_t el = kPer * u;
			const int64_t run = obs_heis_run_of(A.runs, k0, k1, el);
			if (CPLX) {
				double re, im;
				obs_sum_heis_el<true>(A, src, word, s_re, s_im, run, el, re, im);
				if (ACC) {
					const double2 o = *p;
					re += o.x;
					im += o.y;
				}
				__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
			} else {
				const bool two = el + 1 < n_dst; // an odd length ends in half a unit
				double v0, v1 = 0.0, dummy;
				obs_sum_heis_el<false>(A, src, word, s_re, s_im, run, el, v0, dummy);
				// (the closing entry makes runs[run + 1] readable)
				if (two) obs_sum_heis_el<false>(A, src, word, s_re, s_im, (A.runs[run + 1].dst0 <= el + 1) ? run + 1 : run, el + 1, v1, dummy);
				if (ACC) {
					if (two) {
						const double2 o = *p;
						v0 += o.x;
						v1 += o.y;
					} else {
						v0 += p->x;
					}
				}
				if (two) {
					__builtin_nontemporal_store(obs_v2 { v0, v1 }, (obs_v2*)p);
				} else {
					p->x = v0;
				}
			}
		}
	}
}

} // namespace lpp
