// lpp_obs_heis_kernels.h -- one-site operators of the S = 1/2 Heisenberg basis applied to a device vector.
//
// GPU restatement of Engine::accModifiedState_ (reference src/Engine/Engine.h:416-458) for BasisHeisenberg with twiceS = 1:
//     z[bra] += factor * value * src[ket]
// with bra / value from getBraIndex (BasisHeisenberg.h:123-139): getBraIndexSplusSminus (:230-254: the bit flipped, value 1, the spin not read) and
// getBraIndex_ (:256-280: n is the bit for SPIN_UP and 1 - bit for SPIN_DOWN, sz is 1 - 2 bit, the index stays).  No sign: the operators are not
// fermionic and doSignSpSm is BasisBase's 1.  Both vectors are in the reference's basis order: the L-bit words with szPlusConst set bits, ascending
// (:42-46), index = position in that list.
//
// The sorted words are no product of two species; they are RUNS.  Cut the word at lb low bits: all words with the same high part h are consecutive
// and ordered by their low part, the run of h has C(lb, m - popcount(h)) elements, and inside a run the position is the rank of the low word among
// the lb-bit words of its popcount.  So
//   a site in the high part   maps a whole destination run onto a whole source run (h with that bit flipped) at the same position: a shifted stream;
//   a site in the low part    stays inside the run of h and gathers through the rank of the low word with the bit flipped;
//   n and sz                  read the bit and keep the index.
// The kernel keeps k_obs_apply's design: DESTINATION driven, one lane owns one 16-byte unit of z, looks its source up and writes the unit once --
// no atomics.  The host plans one table entry per non-empty destination run (lpp_obs_heis_plan.h, obs_plan_heis): { first destination index, +-(first
// source index + 1) or 0, popcount of the low part } -- everything that depends on the high part is resolved there.  The low words by (popcount,
// rank) and the rank of every lb-bit word, 16 bits each, are staged in LDS (4 * 2^lb bytes; nothing is staged for a site in the high part).
// A tile finds the runs of its first and last element by bisection (the same for every lane), a lane then bisects between those two.
// obs_heis_source (lpp_obs_heis_plan.h, with the plan the host makes) is the ONE lookup: the kernel calls it per element, lpp_obs_plan_heis expands the
// plan with it on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_obs_heis_plan.h"
#include "lpp_obs_kernels.h"

namespace lpp {

struct ObsHeisArgs {
	const ObsHeisRun* runs; // nruns + 1 entries
	const uint16_t* word; // nlo low words ordered by (popcount, rank)
	const uint16_t* rank; // nlo: rank of a low word among the words of its popcount
	int mode, nlo;
	uint32_t bit; // the site's bit in the low part (modes other than HEIS_RUN)
	int64_t nruns, n_dst;
	double fr, fi; // factor
};

// the run that holds element el, between runs lo and hi (both inclusive; runs[lo].dst0 <= el)
__device__ __forceinline__ int64_t obs_heis_run_of(const ObsHeisRun* __restrict__ runs, int64_t lo, int64_t hi, int64_t el)
{
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (runs[mid].dst0 <= el) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

template <bool CPLX> __device__ __forceinline__ bool obs_heis_contrib(const ObsHeisArgs& A, const double* __restrict__ src, const uint16_t* word, const uint16_t* rank,
                                                                      int64_t run, int64_t el, double& re, double& im)
{
	const ObsHeisRun R = A.runs[run];
	int64_t k = obs_heis_source(A.mode, R, el - R.dst0, A.bit, word, rank);
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

inline size_t obs_heis_lds_bytes(int mode, int nlo) { return mode == HEIS_RUN ? 0 : 2 * sizeof(uint16_t) * (size_t)nlo; }

// dst: n_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (untouched destinations are written as 0).
// Dynamic LDS: obs_heis_lds_bytes(mode, nlo).  Tiles, units and the half unit that ends an odd-length f64 vector as in k_obs_apply.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_apply_heis(double* __restrict__ dst, const double* __restrict__ src, const ObsHeisArgs A)
{
	extern __shared__ uint16_t obs_heis_lds[];
	uint16_t* const word = obs_heis_lds;
	uint16_t* const rank = obs_heis_lds + A.nlo;
	if (A.mode != HEIS_RUN) {
		for (int i = threadIdx.x; i < A.nlo; i += kObsBlock) {
			word[i] = A.word[i];
			rank[i] = A.rank[i];
		}
		__syncthreads();
	}
	const int64_t n_dst = A.n_dst;
	const int64_t units = CPLX ? n_dst : (n_dst + 1) / 2;
	const int64_t ntiles = (units + kObsTile - 1) / kObsTile;
	constexpr int kPer = CPLX ? 1 : 2; // elements per unit
	for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		const int64_t u0 = tile * kObsTile;
		const int64_t e0 = kPer * u0; // first and last element of the tile: one search each per tile, every run holds at least one element
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
				double re = 0.0, im = 0.0;
				const bool hit = obs_heis_contrib<true>(A, src, word, rank, run, el, re, im);
				if (ACC) {
					if (!hit) continue;
					const double2 o = *p;
					re += o.x;
					im += o.y;
				}
				__builtin_nontemporal_store(obs_v2 { re, im }, (obs_v2*)p);
			} else {
				const bool two = el + 1 < n_dst; // an odd length ends in half a unit
				double v0 = 0.0, v1 = 0.0, dummy;
				const bool h0 = obs_heis_contrib<false>(A, src, word, rank, run, el, v0, dummy);
				// (the closing entry makes runs[run + 1] readable)
				const bool h1 = two && obs_heis_contrib<false>(A, src, word, rank, (A.runs[run + 1].dst0 <= el + 1) ? run + 1 : run, el + 1, v1, dummy);
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
