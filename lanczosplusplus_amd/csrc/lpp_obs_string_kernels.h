// lpp_obs_string_kernels.h -- a PRODUCT of one-site operators of the Hubbard product basis in one pass: the string applied to a device vector, and the
// bracket <bra| string |ket> of a batch of strings without any intermediate vector.
//
// GPU restatement of Engine::manyPoint (reference src/Engine/Engine.h:341-389: accModifiedState_ step by step through the sectors) and of
// ModelBase::rahulMethod (src/Engine/ModelBase.h:89-141, the -m brackets).  Every one-site operator factorises per species (lpp_obs_kernels.h), so a
// product does: the host composes the whole string into the two tables of lpp_obs_kernels.h (lpp_obs_string_plan.h, plan_string),
//     table[destination species rank] = +-(source species rank + 1), 0 = no source,
// with every fermionic sign carried by the entries.  The one thing that does not factorise is the value of sz in the many-point convention, +1 / -1 /
// absent = (up occupied) - (down occupied) of the word the operator meets: a difference, not a product.  The word it meets is the SOURCE word with
// the bits flipped that earlier operators of the string flipped, so each sz is one entry (site, flip_up, flip_down) and its factor is
//     (bit_up(src, site) ^ flip_up) - (bit_down(src, site) ^ flip_down)
// read from the species' word lists of the source sector -- k entries for k sz operators, never 2^k terms.
//
// Both kernels are DESTINATION driven like k_obs_apply: one lane owns one 16-byte unit of the destination (of z, or of bra).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_common.h"
#include "lpp_obs_kernels.h"
#include "lpp_obs_string_plan.h"

namespace lpp {

static_assert(kObsStringMaxOps <= 16, "the sz entries of a string are two 64-bit words of 8-bit entries");
static_assert(kObsBlock == kBlock, "block_sum and k_reduce_final are written for kBlock threads");
constexpr int kObsStringBatch = 8; // strings per launch of k_obs_string_dot

struct ObsString {
	const int32_t* tab_up; // n_up_dst entries (always present: the identity for an untouched species)
	const int32_t* tab_dn; // n_dn_dst entries
	uint64_t sz_lo, sz_hi; // entry k: 8 bits, site | flip_up << 5 | flip_down << 6
	int32_t nsz;
	int32_t pad;
};

// the source of destination (du, dd): false = the string does not reach it; c = the sign times the sz factors (+1 or -1)
__device__ __forceinline__ bool obs_string_source(const ObsString& S, const uint32_t* __restrict__ words_up, const uint32_t* __restrict__ words_dn, int64_t n_up_src,
                                                  uint32_t du, int64_t dd, int64_t& s, double& c)
{
	int32_t tu = S.tab_up[du], td = S.tab_dn[dd];
	if (tu == 0 || td == 0) return false;
	int v = ((tu < 0) != (td < 0)) ? -1 : 1;
	tu = tu < 0 ? -tu : tu;
	td = td < 0 ? -td : td;
	if (S.nsz > 0) {
		const uint32_t a = words_up[tu - 1], b = words_dn[td - 1];
		for (int k = 0; k < S.nsz; k++) {
			const uint32_t e = (uint32_t)(((k < 8) ? S.sz_lo : S.sz_hi) >> (8 * (k & 7))) & 0xffu;
			const uint32_t site = e & 31u;
			v *= (int)(((a >> site) ^ (e >> 5)) & 1u) - (int)(((b >> site) ^ (e >> 6)) & 1u);
		}
		if (v == 0) return false;
	}
	s = (int64_t)(tu - 1) + (int64_t)(td - 1) * n_up_src;
	c = (double)v;
	return true;
}

// the 16-byte units of a destination of n_up_dst * n_dn_dst elements, tile by tile as k_obs_apply walks them: f(unit, du0, dd0, du1, dd1, two) -- c128: one
// element (du0, dd0) per unit; f64: elements (du0, dd0) and, when `two`, (du1, dd1) (an odd length ends in half a unit)
template <bool CPLX, typename F> __device__ __forceinline__ void obs_string_units(int64_t n_up_dst, int64_t n_dst, F&& f)
{
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const uint32_t nup = (uint32_t)n_up_dst;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = CPLX ? u0 : 2 * u0; // one 64-bit division per tile, 32-bit ones per lane
		const int64_t dd0 = e0 / n_up_dst;
		const uint32_t du0 = (uint32_t)(e0 - dd0 * n_up_dst);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const uint32_t t = (uint32_t)(r * kObsBlock + threadIdx.x);
			const int64_t u = u0 + t;
			if (u >= units) continue;
			if (CPLX) {
				const uint32_t rr = du0 + t, q = rr / nup;
				f(u, rr - q * nup, dd0 + q, 0u, (int64_t)0, false);
			} else {
				const uint32_t r0 = du0 + 2 * t, q0 = r0 / nup, r1 = r0 + 1, q1 = r1 / nup;
				f(u, r0 - q0 * nup, dd0 + q0, r1 - q1 * nup, dd0 + q1, 2 * u + 1 < n_dst);
			}
		}
	}
}

// ---- z (+)= factor * string src ---------------------------------------------------------------------------------------------------------
struct ObsStringApplyArgs {
	ObsString s;
	const uint32_t *words_up, *words_dn; // the source sector's species words by rank (read only when s.nsz > 0)
	int64_t n_up_dst, n_dn_dst, n_up_src;
	double fr, fi; // factor, the string's scale folded in
};

template <bool CPLX> __device__ __forceinline__ bool obs_string_contrib(const ObsStringApplyArgs& A, const double* __restrict__ src, uint32_t du, int64_t dd, double& re, double& im)
{
	int64_t s;
	double c;
	if (!obs_string_source(A.s, A.words_up, A.words_dn, A.n_up_src, du, dd, s, c)) return false;
	if (CPLX) {
		const double2 v = ((const double2*)src)[s];
		const double cr = A.fr * c, ci = A.fi * c;
		re = cr * v.x - ci * v.y;
		im = cr * v.y + ci * v.x;
	} else {
		re = (A.fr * c) * src[s];
		im = 0.0;
	}
	return true;
}

// dst: n_up_dst * n_dn_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (destinations the string does not reach are written as 0)
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_string_apply(double* __restrict__ dst, const double* __restrict__ src, const ObsStringApplyArgs A)
{
	obs_string_units<CPLX>(A.n_up_dst, A.n_up_dst * A.n_dn_dst, [&](int64_t u, uint32_t du0, int64_t dd0, uint32_t du1, int64_t dd1, bool two) {
		double2* const p = (double2*)dst + u;
		if (CPLX) {
			double re = 0.0, im = 0.0;
			const bool hit = obs_string_contrib<true>(A, src, du0, dd0, re, im);
			if (ACC) {
				if (!hit) return;
				const double2 o = *p;
				re += o.x;
				im += o.y;
			}
			__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
		} else {
			double v0 = 0.0, v1 = 0.0, dummy;
			const bool h0 = obs_string_contrib<false>(A, src, du0, dd0, v0, dummy);
			const bool h1 = two && obs_string_contrib<false>(A, src, du1, dd1, v1, dummy);
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

// ---- out[s] = sum_dst conj(bra[dst]) * coef_s(dst) * ket[src_s(dst)] for a batch of strings inside one sector ----------------------------------
// bra streams through once, in 16-byte units, for all strings of the batch; each string costs two table lookups (L2) and one gathered ket element per
// destination it reaches.  No atomics: workgroup b leaves its sums in partial[b * 2 * kObsStringBatch + 2 * s + (0: re, 1: im)], and k_reduce_final
// adds the rows in a fixed order.  Every accumulation is an explicit fma, and a string's sequence of them depends on the grid alone -- not on its slot
// in the batch nor on the other strings -- so a value is the same bit for bit whatever batch it is computed in.
struct ObsStringDotArgs {
	ObsString s[kObsStringBatch];
	const uint32_t *words_up, *words_dn;
	int64_t n_up, n_dn; // source and destination are the same sector
	double* partial; // gridDim.x * 2 * kObsStringBatch
	int32_t ns; // strings in this launch, 1 .. kObsStringBatch
};

template <bool CPLX> __global__ __launch_bounds__(kObsBlock) void k_obs_string_dot(const double* __restrict__ bra, const double* __restrict__ ket, const ObsStringDotArgs A)
{
	__shared__ double smem[kBlock / 64];
	double ar[kObsStringBatch], ai[kObsStringBatch];
#pragma unroll
	for (int s = 0; s < kObsStringBatch; s++) ar[s] = ai[s] = 0.0;
	obs_string_units<CPLX>(A.n_up, A.n_up * A.n_dn, [&](int64_t u, uint32_t du0, int64_t dd0, uint32_t du1, int64_t dd1, bool two) {
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
			int64_t k;
			double c;
			if (CPLX) {
				if (!obs_string_source(A.s[s], A.words_up, A.words_dn, A.n_up, du0, dd0, k, c)) continue;
				const double2 v = ((const double2*)ket)[k];
				const double kr = c * v.x, ki = c * v.y; // conj(b) * k = (b0 kr + b1 ki) + i (b0 ki - b1 kr)
				ar[s] = __builtin_fma(b0, kr, ar[s]);
				ar[s] = __builtin_fma(b1, ki, ar[s]);
				ai[s] = __builtin_fma(b0, ki, ai[s]);
				ai[s] = __builtin_fma(-b1, kr, ai[s]);
			} else {
				if (obs_string_source(A.s[s], A.words_up, A.words_dn, A.n_up, du0, dd0, k, c)) ar[s] = __builtin_fma(b0, c * ket[k], ar[s]);
				if (two && obs_string_source(A.s[s], A.words_up, A.words_dn, A.n_up, du1, dd1, k, c)) ar[s] = __builtin_fma(b1, c * ket[k], ar[s]);
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
