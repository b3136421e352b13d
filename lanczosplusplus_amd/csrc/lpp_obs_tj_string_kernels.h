// lpp_obs_tj_string_kernels.h -- a PRODUCT of one-site operators of the one-orbital t-J basis in one pass: the string applied to a device vector, and
// the bracket <bra| string |ket> of a batch of strings without any intermediate vector.
//
// GPU restatement of Engine::manyPoint (reference src/Engine/Engine.h:341-389: accModifiedState_ step by step through the sectors) for
// BasisTjMultiOrbLanczos with one orbital.  The host composes a string (lpp_obs_tj_string_plan.h) into
//     result[(u, d)] = sign * (-1)^popcount(us & par_up) * (-1)^popcount(ds & par_down) * src[index(us, ds)],   us = u ^ flip_up, ds = d ^ flip_down,
// under conditions on the touched sites of the source, and hands the kernels two things per string: one 32-bit entry per destination down word
// (+-(source down rank + 1) or 0: the down conditions, the down parity and every constant) and a program of at most 16 pattern primitives in
// descending site order (ObsTjStringUp, in the kernel arguments).  Shared by all strings of a launch: the destination's down words and pattern words by
// rank (L2) and the SOURCE sector's split rank tables hi_base / lo_rank, staged in LDS only when a string of the launch changes the pattern.
// Both kernels are DESTINATION driven like k_obs_apply_tj: one lane owns one 16-byte unit of the destination (of z, or of bra), splits its index into
// (pattern rank, down rank) with one 64-bit division per tile and 32-bit ones per lane, and calls obs_tj_string_source, the ONE lookup the host
// expands a plan with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_common.h"
#include "lpp_obs_string_kernels.h"
#include "lpp_obs_tj_kernels.h"
#include "lpp_obs_tj_string_plan.h"

namespace lpp {

// what both kernels share: the destination sector's words and the source sector's rank tables
struct ObsTjStringBase {
	const uint32_t* dnw; // n_dn_dst down words, ascending
	const uint32_t* pat; // n_up_dst patterns, ascending
	const int32_t* hi_base; // nhi entries; ranks in the SOURCE sector
	const uint16_t* lo_rank; // nlo entries
	int lb, nhi, nlo;
	int stage; // 0: no string of the launch changes the pattern, nothing is staged
	int need_pat; // 0: no string of the launch has a step, the pattern words are not read
	int64_t n_up_dst, n_dn_dst, n_up_src;
};

inline size_t obs_tj_string_lds_bytes(const ObsTjStringBase& B) { return B.stage ? obs_tj_lds_bytes(B.nhi, B.nlo) : 0; }

__device__ __forceinline__ void obs_tj_string_stage(const ObsTjStringBase& B, int32_t* hi, uint16_t* lo)
{
	if (!B.stage) return; // (uniform)
	for (int i = threadIdx.x; i < B.nhi; i += kObsBlock) hi[i] = B.hi_base[i];
	for (int i = threadIdx.x; i < B.nlo; i += kObsBlock) lo[i] = B.lo_rank[i];
	__syncthreads();
}

// one destination element: its pattern rank, its pattern word (0 where none is read), its down rank and its down word
struct ObsTjElem {
	uint32_t du, cu, d;
	int64_t dd;
};

__device__ __forceinline__ ObsTjElem obs_tj_elem(const ObsTjStringBase& B, uint32_t du, int64_t dd) { return ObsTjElem { du, B.need_pat ? B.pat[du] : 0u, B.dnw[dd], dd }; }

// the 16-byte units of a destination of n_up_dst * n_dn_dst elements, tile by tile as k_obs_apply_tj walks them: f(unit, a0, a1, two) -- c128: one
// element a0 per unit; f64: elements a0 and, when `two`, a1 (an odd length ends in half a unit)
template <bool CPLX, typename F> __device__ __forceinline__ void obs_tj_string_units(const ObsTjStringBase& B, F&& f)
{
	const int64_t n_dst = B.n_up_dst * B.n_dn_dst;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const uint32_t nup = (uint32_t)B.n_up_dst;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = CPLX ? u0 : 2 * u0; // first element of the tile: one 64-bit division per tile, 32-bit ones per lane
		const int64_t dd0 = e0 / B.n_up_dst;
		const uint32_t du0 = (uint32_t)(e0 - dd0 * B.n_up_dst);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const uint32_t t = (uint32_t)(r * kObsBlock + threadIdx.x);
			const int64_t u = u0 + t;
			if (u >= units) continue;
			if (CPLX) {
				const uint32_t rr = du0 + t, q = rr / nup;
				const ObsTjElem a = obs_tj_elem(B, rr - q * nup, dd0 + q);
				f(u, a, a, false);
			} else {
				const uint32_t r0 = du0 + 2 * t, q0 = r0 / nup, r1 = r0 + 1, q1 = r1 / nup;
				const bool two = 2 * u + 1 < n_dst; // an odd length ends in half a unit
				const ObsTjElem a = obs_tj_elem(B, r0 - q0 * nup, dd0 + q0);
				f(u, a, two ? obs_tj_elem(B, r1 - q1 * nup, dd0 + q1) : a, two);
			}
		}
	}
}

// ---- z (+)= factor * string src ---------------------------------------------------------------------------------------------------------
struct ObsTjStringApplyArgs {
	ObsTjStringBase b;
	const int32_t* ent; // n_dn_dst: the string's entry per destination down word
	ObsTjStringUp up;
	double fr, fi; // factor
};

template <bool CPLX> __device__ __forceinline__ bool obs_tj_string_contrib(const ObsTjStringApplyArgs& A, const double* __restrict__ src, const int32_t* hi, const uint16_t* lo,
                                                                           const ObsTjElem& a, double& re, double& im)
{
	int64_t k = obs_tj_string_source(A.up, A.ent[a.dd], a.d, a.du, a.cu, hi, lo, A.b.lb, A.b.n_up_src);
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

// dst: n_up_dst * n_dn_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (destinations the string does not reach are written as 0).
// Dynamic LDS: obs_tj_string_lds_bytes(A.b).  Units, tiles, the half unit of an odd-length f64 vector and the stores as in k_obs_apply_tj.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_string_apply_tj(double* __restrict__ dst, const double* __restrict__ src, const ObsTjStringApplyArgs A)
{
	extern __shared__ int32_t obs_tj_string_lds[];
	int32_t* const hi = obs_tj_string_lds;
	uint16_t* const lo = (uint16_t*)(obs_tj_string_lds + A.b.nhi);
	obs_tj_string_stage(A.b, hi, lo);
	obs_tj_string_units<CPLX>(A.b, [&](int64_t u, const ObsTjElem& a0, const ObsTjElem& a1, bool two) {
		double2* const p = (double2*)dst + u;
		if (CPLX) {
			double re = 0.0, im = 0.0;
			const bool hit = obs_tj_string_contrib<true>(A, src, hi, lo, a0, re, im);
			if (ACC) {
				if (!hit) return;
				const double2 o = *p;
				re += o.x;
				im += o.y;
			}
			__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
		} else {
			double v0 = 0.0, v1 = 0.0, dummy;
			const bool h0 = obs_tj_string_contrib<false>(A, src, hi, lo, a0, v0, dummy);
			const bool h1 = two && obs_tj_string_contrib<false>(A, src, hi, lo, a1, v1, dummy);
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
// bra streams through once, in 16-byte units, for all strings of the batch; the down word and the pattern word of an element are fetched once for all
// of them, and each string costs its down entry (L2), its pattern steps in registers, at most one rank (LDS) and one gathered ket element per
// destination it reaches.  Source and destination sector are the same, so there is one set of rank tables.  No atomics: workgroup b leaves its sums
// in partial[b * 2 * kObsStringBatch + 2 * s + (0: re, 1: im)], and k_reduce_final adds the rows in a fixed order.  Every accumulation is an
// explicit fma, and a string's sequence of them depends on the grid alone -- not on its slot in the batch nor on the other strings -- so a value is
// the same bit for bit whatever batch it is computed in.
struct ObsTjStringDotArgs {
	ObsTjStringBase b;
	const int32_t* ent[kObsStringBatch]; // n_dn_dst each
	ObsTjStringUp up[kObsStringBatch];
	double* partial; // gridDim.x * 2 * kObsStringBatch
	int32_t ns; // strings in this launch, 1 .. kObsStringBatch
};

template <bool CPLX> __global__ __launch_bounds__(kObsBlock) void k_obs_string_dot_tj(const double* __restrict__ bra, const double* __restrict__ ket, const ObsTjStringDotArgs A)
{
	__shared__ double smem[kBlock / 64];
	extern __shared__ int32_t obs_tj_string_lds[];
	int32_t* const hi = obs_tj_string_lds;
	uint16_t* const lo = (uint16_t*)(obs_tj_string_lds + A.b.nhi);
	obs_tj_string_stage(A.b, hi, lo);
	double ar[kObsStringBatch], ai[kObsStringBatch];
#pragma unroll
	for (int s = 0; s < kObsStringBatch; s++) ar[s] = ai[s] = 0.0;
	obs_tj_string_units<CPLX>(A.b, [&](int64_t u, const ObsTjElem& a0, const ObsTjElem& a1, bool two) {
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
			int64_t k = obs_tj_string_source(A.up[s], A.ent[s][a0.dd], a0.d, a0.du, a0.cu, hi, lo, A.b.lb, A.b.n_up_src);
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
				k = obs_tj_string_source(A.up[s], A.ent[s][a1.dd], a1.d, a1.du, a1.cu, hi, lo, A.b.lb, A.b.n_up_src);
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
