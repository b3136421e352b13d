// lpp_obs_heis_string_kernels.h -- a PRODUCT of one-site operators of the S = 1/2 Heisenberg basis in one pass: the string applied to a device vector,
// and the bracket <bra| string |ket> of a batch of strings without any intermediate vector.
//
// GPU restatement of Engine::manyPoint (reference src/Engine/Engine.h:341-389: accModifiedState_ step by step through the sectors) for BasisHeisenberg
// with twiceS = 1.  The host composes a string into five bit masks and a sign (lpp_obs_heis_string_plan.h):
//     result[d] = sign * (-1)^popcount((d ^ flip) & zmask) * src[rank(d ^ flip)]   where ((d ^ flip) & need) == want.
// The vectors are in the run structure of lpp_obs_heis_kernels.h: words cut at lb low bits, one run per high part.  Everything that depends on the high
// part is resolved on the host, per destination run and per string: +-(first index of the source run + 1) or 0.  The low part is evaluated here from the
// low lb bits of the masks with the two 16-bit tables of k_obs_apply_heis in LDS (4 * 2^lb bytes; a batch without low-part work stages nothing).  The
// destination runs { first index, popcount of the low part, word base } are shared by all strings of a launch.
// Both kernels are DESTINATION driven like k_obs_apply_heis: one lane owns one 16-byte unit of the destination (of z, or of bra), finds its run by the
// tile / lane bisection and calls obs_heis_string_source, the ONE lookup the host expands a plan with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_common.h"
#include "lpp_obs_heis_kernels.h"
#include "lpp_obs_heis_string_plan.h"
#include "lpp_obs_string_kernels.h"

namespace lpp {

// what both kernels share: the destination sector's runs and the low tables
struct ObsHeisStringBase {
	const ObsHeisRun* runs; // nruns + 1 entries (src not read)
	const uint16_t* word; // nlo low words ordered by (popcount, rank)
	const uint16_t* rank; // nlo: rank of a low word among the words of its popcount
	int64_t nruns, n_dst;
	int nlo; // 0: no string of the launch has low-part work, nothing is staged
};

inline size_t obs_heis_string_lds_bytes(int nlo) { return 2 * sizeof(uint16_t) * (size_t)nlo; }

__device__ __forceinline__ void obs_heis_string_stage(const ObsHeisStringBase& B, uint16_t* word, uint16_t* rank)
{
	if (B.nlo == 0) return; // (uniform)
	for (int i = threadIdx.x; i < B.nlo; i += kObsBlock) {
		word[i] = B.word[i];
		rank[i] = B.rank[i];
	}
	__syncthreads();
}

// one destination element: its run, its position in the run and its low word (0 where nothing is staged)
struct ObsHeisElem {
	int64_t run, r;
	uint32_t w;
};

__device__ __forceinline__ ObsHeisElem obs_heis_elem(const ObsHeisStringBase& B, const uint16_t* word, int64_t run, int64_t el)
{
	const ObsHeisRun R = B.runs[run];
	const int64_t r = el - R.dst0;
	return ObsHeisElem { run, r, B.nlo ? (uint32_t)word[R.wbase + (int32_t)r] : 0u };
}

// the 16-byte units of a destination of n_dst elements, tile by tile as k_obs_apply_heis walks them: f(unit, e0, e1, two) -- c128: one element e0 per
// unit; f64: elements e0 and, when `two`, e1 (an odd length ends in half a unit)
template <bool CPLX, typename F> __device__ __forceinline__ void obs_heis_string_units(const ObsHeisStringBase& B, const uint16_t* word, F&& f)
{
	const int64_t n_dst = B.n_dst;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	constexpr int kPer = CPLX ? 1 : 2; // elements per unit
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = kPer * u0; // first and last element of the tile: one search each per tile, every run holds at least one element
		const int64_t e1 = (e0 + kPer * kObsTile < n_dst ? e0 + kPer * kObsTile : n_dst) - 1;
		const int64_t k0 = obs_heis_run_of(B.runs, 0, B.nruns - 1, e0);
		const int64_t k1 = obs_heis_run_of(B.runs, k0, (k0 + (e1 - e0) < B.nruns - 1 ? k0 + (e1 - e0) : B.nruns - 1), e1);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const int64_t u = u0 + (r * kObsBlock + (int)threadIdx.x);
			if (u >= units) continue;
			const int64_t el = kPer * u;
			const int64_t run = obs_heis_run_of(B.runs, k0, k1, el);
			const ObsHeisElem a = obs_heis_elem(B, word, run, el);
			if (CPLX) {
				f(u, a, a, false);
			} else {
				const bool two = el + 1 < n_dst;
				// (the closing entry makes runs[run + 1] readable)
				f(u, a, two ? obs_heis_elem(B, word, (B.runs[run + 1].dst0 <= el + 1) ? run + 1 : run, el + 1) : a, two);
			}
		}
	}
}

// ---- z (+)= factor * string src ---------------------------------------------------------------------------------------------------------
struct ObsHeisStringApplyArgs {
	ObsHeisStringBase b;
	const int64_t* src; // nruns: the string's entry per destination run
	ObsHeisStringLow low;
	double fr, fi; // factor
};

template <bool CPLX> __device__ __forceinline__ bool obs_heis_string_contrib(const ObsHeisStringApplyArgs& A, const double* __restrict__ src, const uint16_t* rank,
                                                                             const ObsHeisElem& a, double& re, double& im)
{
	int64_t k = obs_heis_string_source(A.low, A.src[a.run], a.r, a.w, rank);
	if (k == 0) return false;
	const double c = k < 0 ? -1.0 : 1.0;
	k = (k < 0 ? -k : k) - 1;
	if (CPLX) {
		const double2 v = ((const double2*)src)[k];
		const double cr = A.fr * c, ci = A.fi * c;
		re = cr * v.x - ci * v.y;
		im = cr * v.y + ci * v.x;
	} else {
		re = (A.fr * c) * src[k];
		im = 0.0;
	}
	return true;
}

// dst: n_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (destinations the string does not reach are written as 0).
// Dynamic LDS: obs_heis_string_lds_bytes(nlo).  Units, tiles, the half unit of an odd-length f64 vector and the stores as in k_obs_apply_heis.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_string_apply_heis(double* __restrict__ dst, const double* __restrict__ src, const ObsHeisStringApplyArgs A)
{
	extern __shared__ uint16_t obs_heis_string_lds[];
	uint16_t* const word = obs_heis_string_lds;
	uint16_t* const rank = obs_heis_string_lds + A.b.nlo;
	obs_heis_string_stage(A.b, word, rank);
	obs_heis_string_units<CPLX>(A.b, word, [&](int64_t u, const ObsHeisElem& a0, const ObsHeisElem& a1, bool two) {
		double2* const p = (double2*)dst + u;
		if (CPLX) {
			double re = 0.0, im = 0.0;
			const bool hit = obs_heis_string_contrib<true>(A, src, rank, a0, re, im);
			if (ACC) {
				if (!hit) return;
				const double2 o = *p;
				re += o.x;
				im += o.y;
			}
			__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
		} else {
			double v0 = 0.0, v1 = 0.0, dummy;
			const bool h0 = obs_heis_string_contrib<false>(A, src, rank, a0, v0, dummy);
			const bool h1 = two && obs_heis_string_contrib<false>(A, src, rank, a1, v1, dummy);
			if (ACC) {
				if (!h0 && !h1) return;
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
	});
}

// ---- out[s] = sum_dst conj(bra[dst]) * coef_s(dst) * ket[src_s(dst)] for a batch of strings that stay in the sector ----------------------------
// bra streams through once, in 16-byte units, for all strings of the batch; the run and the low word of an element are found once for all of them, and
// each string costs its run entry (L2), at most one rank (LDS) and one gathered ket element per destination it reaches.  No atomics: workgroup b
// leaves its sums in partial[b * 2 * kObsStringBatch + 2 * s + (0: re, 1: im)], and k_reduce_final adds the rows in a fixed order.  Every
// accumulation is an explicit fma, and a string's sequence of them depends on the grid alone -- not on its slot in the batch nor on the other
// strings -- so a value is the same bit for bit whatever batch it is computed in.
struct ObsHeisStringDotArgs {
	ObsHeisStringBase b;
	const int64_t* src[kObsStringBatch]; // nruns each
	ObsHeisStringLow low[kObsStringBatch];
	double* partial; // gridDim.x * 2 * kObsStringBatch
	int32_t ns; // strings in this launch, 1 .. kObsStringBatch
};

template <bool CPLX> __global__ __launch_bounds__(kObsBlock) void k_obs_string_dot_heis(const double* __restrict__ bra, const double* __restrict__ ket, const ObsHeisStringDotArgs A)
{
	__shared__ double smem[kBlock / 64];
	extern __shared__ uint16_t obs_heis_string_lds[];
	uint16_t* const word = obs_heis_string_lds;
	uint16_t* const rank = obs_heis_string_lds + A.b.nlo;
	obs_heis_string_stage(A.b, word, rank);
	double ar[kObsStringBatch], ai[kObsStringBatch];
#pragma unroll
	for (int s = 0; s < kObsStringBatch; s++) ar[s] = ai[s] = 0.0;
	obs_heis_string_units<CPLX>(A.b, word, [&](int64_t u, const ObsHeisElem& a0, const ObsHeisElem& a1, bool two) {
		double b0, b1; // c128: re, im of the bra element; f64: the two bra elements
		if (CPLX || two) {
			const double2 b = ((const double2*)bra)[u];
			b0 = b.x;
			b1 = b.y;
		} else {
			b0 = bra[2 * u];
			b1 = 0.0;
		}
#pragma unroll
		for (int s = 0; s < kObsStringBatch; s++) {
			if (s >= A.ns) continue;
			int64_t k = obs_heis_string_source(A.low[s], A.src[s][a0.run], a0.r, a0.w, rank);
			if (CPLX) {
				if (k == 0) continue;
				const double c = k < 0 ? -1.0 : 1.0;
				const double2 v = ((const double2*)ket)[(k < 0 ? -k : k) - 1];
				const double kr = c * v.x, ki = c * v.y; // conj(b) * k = (b0 kr + b1 ki) + i (b0 ki - b1 kr)
				ar[s] = __builtin_fma(b0, kr, ar[s]);
				ar[s] = __builtin_fma(b1, ki, ar[s]);
				ai[s] = __builtin_fma(b0, ki, ai[s]);
				ai[s] = __builtin_fma(-b1, kr, ai[s]);
			} else {
				if (k != 0) ar[s] = __builtin_fma(b0, (k < 0 ? -1.0 : 1.0) * ket[(k < 0 ? -k : k) - 1], ar[s]);
				if (!two) continue;
				k = obs_heis_string_source(A.low[s], A.src[s][a1.run], a1.r, a1.w, rank);
				if (k != 0) ar[s] = __builtin_fma(b1, (k < 0 ? -1.0 : 1.0) * ket[(k < 0 ? -k : k) - 1], ar[s]);
			}
		}
	});
	double* const row = A.partial + (int64_t)blockIdx.x * (2 * kObsStringBatch);
#pragma unroll
	for (int s = 0; s < kObsStringBatch; s++) {
		if (s >= A.ns) continue; // (uniform)
		const double re = block_sum(ar[s], smem);
		const double im = CPLX ? block_sum(ai[s], smem) : 0.0;
		if (threadIdx.x == 0) {
			row[2 * s] = re;
			row[2 * s + 1] = im;
		}
	}
}

} // namespace lpp
