// lpp_obs_heis_spin_kernels.h -- one-site operators of the spin-S Heisenberg digit basis applied to a device vector.
//
//     z[bra] += factor * value * src[ket]
// with sz, splus and sminus as lpp_obs_heis_spin_plan.h defines them (the project's own definition: the reference throws for spins above 1/2).
// Both vectors are in the basis order: the words of L digits with digit sum szPlusConst, ascending (BasisHeisenberg.h:24-47).
//
// The kernel keeps the shape of k_obs_apply_heis (lpp_obs_heis_kernels.h): DESTINATION driven, one lane owns one 16-byte unit of z, looks its source
// up and writes the unit once -- no atomics.  The sorted words are RUNS of equal high part; the host plans one table entry per non-empty destination
// run (obs_plan_heis_spin), and
//   a site in the high part   maps a whole destination run onto a whole source run at the same position, the value comes from the entry;
//   a site in the low part    stays inside the run's high part and gathers through the rank of the low code with the site's digit one lower (splus)
//                             or one higher (sminus), in the run of the same high part of the source sector;
//   sz                        reads the digit and keeps the index.
// The low strings by (digit sum, rank) and the rank of every raw low code, 16 bits each, are staged in LDS only for a site in the low part.  The
// value is an entry of the plan's table of twiceS + 1 doubles (formed on the host): the kernel calls no sqrt.  A tile finds the runs of its first and
// last element by bisection (the same for every lane), a lane then bisects between those two.  obs_heis_spin_source is the ONE lookup: the kernel
// calls it per element, lpp_obs_plan_heis_spin expands the plan with it on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpp_obs_heis_spin_plan.h"
#include "lpp_obs_kernels.h"

namespace lpp {

struct ObsHeisSpinArgs {
	const ObsHeisSpinRun* runs; // nruns + 1 entries
	const uint16_t* word; // nword low strings ordered by (digit sum, rank)
	const uint16_t* rank; // nrank: rank of a raw low code among the strings of its digit sum
	const double* val; // top + 1 values by the source's digit
	int mode, nword, nrank;
	int shift; // the site's digit in the low part (modes other than HSPIN_RUN)
	uint32_t mask;
	int top; // twiceS
	int64_t nruns, n_dst;
	double fr, fi; // factor
};

// the run that holds element el, between runs lo and hi (both inclusive; runs[lo].dst0 <= el)
__device__ __forceinline__ int64_t obs_heis_spin_run_of(const ObsHeisSpinRun* __restrict__ runs, int64_t lo, int64_t hi, int64_t el)
{
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (runs[mid].dst0 <= el) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

template <bool CPLX> __device__ __forceinline__ bool obs_heis_spin_contrib(const ObsHeisSpinArgs& A, const double* __restrict__ src, const uint16_t* word, const uint16_t* rank,
                                                                           int64_t run, int64_t el, double& re, double& im)
{
	const ObsHeisSpinRun R = A.runs[run];
	int vi = 0;
	const int64_t k = obs_heis_spin_source(A.mode, R, el - R.dst0, A.shift, A.mask, A.top, word, rank, &vi);
	if (k == 0) return false;
	const double c = A.val[vi];
	if (CPLX) {
		const double2 v = ((const double2*)src)[k - 1];
		const double cr = A.fr * c, ci = A.fi * c;
		re = cr * v.x - ci * v.y;
		im = cr * v.y + ci * v.x;
	} else {
		re = (A.fr * c) * src[k - 1];
		im = 0.0;
	}
	return true;
}

inline size_t obs_heis_spin_lds_bytes(int mode, int nword, int nrank) { return mode == HSPIN_RUN ? 0 : sizeof(uint16_t) * ((size_t)nword + (size_t)nrank); }

// dst: n_dst elements, 16-byte aligned; ACC: z += ..., otherwise z = ... (untouched destinations are written as 0).
// Dynamic LDS: obs_heis_spin_lds_bytes(mode, nword, nrank).  Tiles, units and the half unit that ends an odd-length f64 vector as in k_obs_apply.
template <bool CPLX, bool ACC> __global__ __launch_bounds__(kObsBlock) void k_obs_apply_heis_spin(double* __restrict__ dst, const double* __restrict__ src, const ObsHeisSpinArgs A)
{
	extern __shared__ uint16_t obs_heis_spin_lds[];
	uint16_t* const word = obs_heis_spin_lds;
	uint16_t* const rank = obs_heis_spin_lds + A.nword;
	if (A.mode != HSPIN_RUN) {
		for (int i = threadIdx.x; i < A.nword; i += kObsBlock) word[i] = A.word[i];
		for (int i = threadIdx.x; i < A.nrank; i += kObsBlock) rank[i] = A.rank[i];
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
		const int64_t k0 = obs_heis_spin_run_of(A.runs, 0, A.nruns - 1, e0);
		const int64_t k1 = obs_heis_spin_run_of(A.runs, k0, (k0 + (e1 - e0) < A.nruns - 1 ? k0 + (e1 - e0) : A.nruns - 1), e1);
#pragma unroll
		for (int r = 0; r < kObsUnroll; r++) {
			const int64_t u = u0 + (r * kObsBlock + (int)threadIdx.x);
			if (u >= units) continue;
			double2* const p = (double2*)dst + u;
			const int64_t el = kPer * u;
			const int64_t run = obs_heis_spin_run_of(A.runs, k0, k1, el);
			if (CPLX) {
				double re = 0.0, im = 0.0;
				const bool hit = obs_heis_spin_contrib<true>(A, src, word, rank, run, el, re, im);
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
				const bool h0 = obs_heis_spin_contrib<false>(A, src, word, rank, run, el, v0, dummy);
				// (the closing entry makes runs[run + 1] readable)
				const bool h1 = two && obs_heis_spin_contrib<false>(A, src, word, rank, (A.runs[run + 1].dst0 <= el + 1) ? run + 1 : run, el + 1, v1, dummy);
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
