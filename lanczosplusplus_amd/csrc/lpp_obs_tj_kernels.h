// lpp_obs_tj_kernels.h -- one-site operators of the one-orbital t-J basis applied to a device vector.
//
// GPU restatement of Engine::accModifiedState_ (reference src/Engine/Engine.h:416-458) for BasisTjMultiOrbLanczos with one orbital:
//     z[bra] += factor * sign * src[ket]
// with bra from getBraIndex (BasisTjMultiOrbLanczos.h:207-245, :296-315, :414-469) and sign from doSignGf (:163-192); doSignSpSm is BasisBase's 1.
// Both vectors are in the reference's basis order: the sorted words (down << L) | up without double occupancy, that is
//     index = rank(up compressed onto the sites free of down electrons) + rank(down) * C(L - ndown, nup)        (index_of<ASM_TJ>).
//
// The basis is a product once the up word is written as a PATTERN on the free sites, so the kernel keeps k_obs_apply's design: DESTINATION
// driven, one lane owns one 16-byte unit of z, looks its source up and writes the unit once -- no atomics.  Per destination (pattern rank
// du, down rank dd) it does
//   one down lookup   dn[dd] = { +-(source down rank + 1) or 0, p }: whether the site's condition on the down word d' holds, the source down
//                     word's rank, the down share of the sign, and p = popcount(~d' & ((1 << site) - 1)), the site's position among the free sites;
//   one up lookup     the destination's pattern word pat[du], the operator's bit operation at position p in registers (set / clear / delete /
//                     insert, or only a test for n), and the rank of the resulting source pattern through the split rank tables
//                     rank(s) = hi_base[s >> lb] + lo_rank[s & ((1 << lb) - 1)], staged in LDS (the form k_tj_apply ranks its patterns with).
// Only the pattern words (C(L - ndown', nup') of them) and the down table (8 bytes per down word) are read from L2.
// obs_tj_source (lpp_obs_tj_plan.h, with the plan the host makes) is the ONE lookup: the kernel calls it per element, lpp_obs_plan_tj expands the plan
// with it on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_obs_kernels.h"
#include "lpp_obs_tj_plan.h"

namespace lpp {

struct ObsTjArgs {
	const ObsTjDown* dn; // n_dn_dst entries
	const uint32_t* pat; // n_up_dst destination patterns, ascending (unused for TJ_UP_SAME)
	const int32_t* hi_base; // nhi entries; ranks in the SOURCE sector (unused for TJ_UP_SAME)
	const uint16_t* lo_rank; // nlo entries
	int up, lb, nhi, nlo;
	int64_t n_up_dst, n_dn_dst, n_up_src;
	double fr, fi; // factor
};

template <bool CPLX> __device__ __forceinline__ bool obs_tj_contrib(const ObsTjArgs& A, const double* __restrict__ src, const int32_t* hi, const uint16_t* lo, uint32_t du,
                                                                    int64_t dd, double& re, double& im)
{
	int64_t k = obs_tj_source(A.up, A.dn[dd], du, A.pat, hi, lo, A.lb, A.n_up_src);
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

inline size_t obs_tj_lds_bytes(int nhi, int nlo) { return sizeof(int32_t) * (size_t)nhi + sizeof(uint16_t) * (size_t)nlo; }

// dst: n_up_dst * n_dn_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (untouched destinations are written as 0).
// Dynamic LDS: obs_tj_lds_bytes(nhi, nlo).  Tiles, units and the half unit that ends an odd-length f64 vector as in k_obs_apply.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_apply_tj(double* __restrict__ dst, const double* __restrict__ src, const ObsTjArgs A)
{
	extern __shared__ int32_t obs_tj_lds[];
	int32_t* const hi = obs_tj_lds;
	uint16_t* const lo = (uint16_t*)(obs_tj_lds + A.nhi);
	if (A.up != TJ_UP_SAME) {
		for (int i = threadIdx.x; i < A.nhi; i += kObsBlock) hi[i] = A.hi_base[i];
		for (int i = threadIdx.x; i < A.nlo; i += kObsBlock) lo[i] = A.lo_rank[i];
		__syncthreads();
	}
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
				double re = 0.0, im = 0.0;
				const bool hit = obs_tj_contrib<true>(A, src, hi, lo, rr - q * nup, dd0 + q, re, im);
				if (ACC) {
					if (!hit) continue;
					const double2 o = *p;
					re += o.x;
					im += o.y;
				}
				__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
			} else {
				const uint32_t r0 = du0 + 2 * t, q0 = r0 / nup, r1 = r0 + 1, q1 = r1 / nup;
				const bool two = 2 * u + 1 < n_dst; // an odd length ends in half a unit
				double v0 = 0.0, v1 = 0.0, dummy;
				const bool h0 = obs_tj_contrib<false>(A, src, hi, lo, r0 - q0 * nup, dd0 + q0, v0, dummy);
				const bool h1 = two && obs_tj_contrib<false>(A, src, hi, lo, r1 - q1 * nup, dd0 + q1, v1, dummy);
				if (ACC) {
					if (!h0 && !h1) continue;
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
