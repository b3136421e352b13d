// lpp_obs_kernels.h -- one-site operators of the Hubbard product basis applied to a device vector.
//
// GPU restatement of Engine::accModifiedState_ (reference src/Engine/Engine.h:416-458) for BasisHubbardLanczos:
//     z[bra] += factor * sign * value * src[ket]
// with bra / value from getBraIndex (BasisHubbardLanczos.h:162-246), sign from doSignGf (:106-137) and doSignSpSm (:151-160).
// Both vectors are in the reference's basis order, index = rank(up) + rank(down) * N_up (:59-63).
//
// Every operator of LabeledOperator.h:36-59 factorises per species, so the host plans two small tables (lpp_obs_plan.h, obs_plan):
//     table[destination species rank] = +-(source species rank + 1), 0 = no source; the sign of the entry is the species' part of the sign.
// The kernel is DESTINATION driven: one lane owns one 16-byte unit of z (two f64 elements, or one c128 element), looks its source up through
// the two tables and writes the unit once -- no atomics, z streams through with 16-byte accesses, the tables (at most C(L, L/2) entries each)
// stay in L2.  An up-species operator gathers inside the source block of N_up positions, a down-species operator moves whole blocks,
// splus / sminus use both tables, n is the identity table with holes; sz (value +1 / -1 / none, getBraIndexSz :210-223) reads the two
// occupancy tables and takes their difference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lpp {

constexpr int kObsBlock = 256;
constexpr int kObsUnroll = 4; // 16-byte units per lane and tile
constexpr int kObsTile = kObsBlock * kObsUnroll;
typedef double obs_v2 __attribute__((ext_vector_type(2))); // one 16-byte store

struct ObsArgs {
	const int32_t* tab_up; // n_up_dst entries, null: the up species is untouched
	const int32_t* tab_dn; // n_dn_dst entries, null: the down species is untouched
	int64_t n_up_dst, n_dn_dst, n_up_src;
	int sz; // 1: value = (up occupied) - (down occupied), both tables are occupancy tables
	double fr, fi; // factor
};

// contribution to destination element `el` (du, dd): returns false when the reference does not touch it
template <bool CPLX> __device__ __forceinline__ bool obs_contrib(const ObsArgs& A, const double* __restrict__ src, uint32_t du, int64_t dd, double& re, double& im)
{
	int32_t tu = A.tab_up ? A.tab_up[du] : (int32_t)du + 1;
	int32_t td = A.tab_dn ? A.tab_dn[dd] : (int32_t)dd + 1;
	double c;
	int64_t s;
	if (A.sz) {
		const int v = (tu != 0) - (td != 0);
		if (v == 0) return false;
		c = (double)v;
		s = (int64_t)du + dd * A.n_up_src;
	} else {
		if (tu == 0 || td == 0) return false;
		c = ((tu < 0) != (td < 0)) ? -1.0 : 1.0;
		tu = tu < 0 ? -tu : tu;
		td = td < 0 ? -td : td;
		s = (int64_t)(tu - 1) + (int64_t)(td - 1) * A.n_up_src;
	}
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

// dst: n_up_dst * n_dn_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (untouched destinations are written as 0)
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_apply(double* __restrict__ dst, const double* __restrict__ src, const ObsArgs A)
{
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
				const bool hit = obs_contrib<true>(A, src, rr - q * nup, dd0 + q, re, im);
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
				const bool h0 = obs_contrib<false>(A, src, r0 - q0 * nup, dd0 + q0, v0, dummy);
				const bool h1 = two && obs_contrib<false>(A, src, r1 - q1 * nup, dd0 + q1, v1, dummy);
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
