// lpp_rdm_kernels.h -- the reduced density matrix of the low `split` sites, as a gather-SYRK on the f64 MFMA.
//
// GPU restatement of ReducedDensityMatrix::build (reference src/Engine/ReducedDensityMatrix.h:65-76) for BasisHubbardLanczos and the
// S = 1/2 words of BasisHeisenberg:     rdm(alpha, alpha') += conj(psi[i]) * psi[j]   for all i, j with the same environment beta.
// The conjugate sits on the ROW index (:73).
//
// In the basis order (index = rank(up) + rank(down) * N_up, words ascending) the high L - split bits of a species' word are the major sort
// key, so the states that share one high configuration t are ONE contiguous run of ranks ordered by the low word.  For a class
// (k_up, k_down) of particle numbers in the low sites the amplitudes psi(alpha, beta) are therefore a re-indexing of psi,
//     V[r][b] = psi[(a_up + a_down * N_up) + (s_up[t_up] + s_down[t_down] * N_up)],   r = a_up + a_down * du,  b = t_up + t_down * eu,
// with the two run-start tables s_up / s_down planned on the host (lpp_rdm.hip), and the block of the result is  conj(V) V^T  (d x d, K deep).
// Nothing is materialised: the kernel gathers its panels of V straight from psi.
//
// k_rdm_tiles: one workgroup of 4 waves owns one 64 x 64 tile (ti >= tj: one triangle of tiles) of one block over one K range.  K is walked
// in panels of 16 columns staged in LDS (k-major, pitch 80 doubles: the four k rows one MFMA operand reads fall into different halves of the
// banks); the next panel's gather is in flight while the MFMAs of the current one run.  Each wave owns a 32 x 32 quadrant = 2 x 2 MFMA tiles of
// v_mfma_f64_16x16x4_f64:  A operand [lane & 15][k = lane >> 4],  B operand [k = lane >> 4][lane & 15],  C/D col = lane & 15,
// row = (lane >> 4) + 4 * reg.  c128 runs real MFMAs on the re / im planes of the staged panels:
//     Re rho = Vr Vr^T + Vi Vi^T,     Im rho = Vr Vi^T - Vi Vr^T.
// Tails (rows beyond d, columns beyond the K range) are zeros in LDS and are never loaded: no lane forms an address outside psi.
// Only elements with row >= col are stored, each together with its mirror image (conjugated), and the diagonal's imaginary part is written
// as 0: the result is Hermitian bit for bit.
//
// Split-K: a block whose tiles are too few to fill the device has its K range cut into S fixed ranges (planned on the host, a function of the
// sector alone).  Those work items write their raw 64 x 64 partial tile into a workspace and k_rdm_reduce adds the S partial tiles in
// ascending order of the range: no atomics, the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lpp {

constexpr int kRdmBlock = 256;
constexpr int kRdmTile = 64;
constexpr int kRdmPanel = 16; // k columns per staged panel
constexpr int kRdmPitch = 80; // doubles per k column in LDS
constexpr int kRdmTileElems = kRdmTile * kRdmTile;
typedef double rdm_v4 __attribute__((ext_vector_type(4)));

struct RdmBlockDev {
	int64_t out_off; // element offset of the block in the packed result
	int32_t d, du; // rows of the block, rows per down configuration
	int32_t eu; // environment configurations of the up species (b = t_up + t_down * eu)
	int32_t su_off, sd_off; // the class's run starts in the two tables
	int32_t pad;
};

struct RdmItem {
	int32_t block, ti, tj, nsplit; // nsplit: K ranges of the tile (reduce items), unused by the tile kernel
	int64_t k0, k1; // K range (tile items)
	int64_t ws; // partial tile in the workspace, -1: the tile is written to the result
};

struct RdmArgs {
	const double* psi;
	int64_t n_up;
	const RdmBlockDev* blocks;
	const RdmItem* items;
	const int32_t *su, *sd;
	double* out;
	double* ws;
};

// one element of the lower triangle and its mirror image
template <bool CPLX> __device__ __forceinline__ void rdm_store(double* __restrict__ out, int64_t off, int32_t d, int64_t r, int64_t c, double re, double im)
{
	if (r >= d || c > r) return; // c <= r < d
	if (CPLX) {
		double2* o = (double2*)out + off;
		if (r == c) {
			o[r * d + c] = make_double2(re, 0.0);
		} else {
			o[r * d + c] = make_double2(re, im);
			o[c * d + r] = make_double2(re, -im);
		}
	} else {
		out[off + r * d + c] = re;
		if (r != c) out[off + c * d + r] = re;
	}
}

template <bool CPLX> __global__ __launch_bounds__(kRdmBlock) void k_rdm_tiles(RdmArgs A)
{
	constexpr int W = CPLX ? 2 : 1;
	__shared__ double sA[W][kRdmPanel][kRdmPitch];
	__shared__ double sB[W][kRdmPanel][kRdmPitch];
	const RdmItem it = A.items[blockIdx.x];
	const RdmBlockDev B = A.blocks[it.block];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const bool diag = it.ti == it.tj;

	// staging: this thread owns row `lane` of both tiles and the k columns kq, kq + 4, kq + 8, kq + 12 of every panel
	const int kq = tid >> 6;
	const int32_t ra = it.ti * kRdmTile + lane, rb = it.tj * kRdmTile + lane;
	const bool va = ra < B.d, vb = !diag && rb < B.d;
	const int32_t rac = va ? ra : 0, rbc = vb ? rb : 0;
	const int64_t offa = (int64_t)(rac % B.du) + (int64_t)(rac / B.du) * A.n_up;
	const int64_t offb = (int64_t)(rbc % B.du) + (int64_t)(rbc / B.du) * A.n_up;
	const int32_t* __restrict__ su = A.su + B.su_off;
	const int32_t* __restrict__ sd = A.sd + B.sd_off;
	// the environment (t_up, t_down) of this thread's next k column, advanced by 4 per use
	int64_t kn = it.k0 + kq;
	int64_t td = kn / B.eu;
	int32_t tu = (int32_t)(kn - td * B.eu);

	double ga[4][W], gb[4][W];
	auto gather = [&]() {
#pragma unroll
		for (int i = 0; i < 4; i++) {
#pragma unroll
			for (int p = 0; p < W; p++) ga[i][p] = gb[i][p] = 0.0;
			if (kn < it.k1 && (va || vb)) {
				const int64_t col = (int64_t)su[tu] + (int64_t)sd[td] * A.n_up;
				if (va) {
					if (CPLX) {
						const double2 v = ((const double2*)A.psi)[offa + col];
						ga[i][0] = v.x;
						ga[i][W - 1] = v.y;
					} else {
						ga[i][0] = A.psi[offa + col];
					}
				}
				if (vb) {
					if (CPLX) {
						const double2 v = ((const double2*)A.psi)[offb + col];
						gb[i][0] = v.x;
						gb[i][W - 1] = v.y;
					} else {
						gb[i][0] = A.psi[offb + col];
					}
				}
			}
			kn += 4;
			tu += 4;
			while (tu >= B.eu) {
				tu -= B.eu;
				td++;
			}
		}
	};

	// this wave's quadrant and what of it lies inside the block and inside the stored triangle
	const int wr = wave >> 1, wc = wave & 1;
	const int rows_live = min(kRdmTile, B.d - it.ti * kRdmTile), cols_live = min(kRdmTile, B.d - it.tj * kRdmTile);
	bool live[2][2];
#pragma unroll
	for (int m = 0; m < 2; m++)
#pragma unroll
		for (int n = 0; n < 2; n++) {
			const int r0 = wr * 32 + m * 16, c0 = wc * 32 + n * 16;
			live[m][n] = r0 < rows_live && c0 < cols_live && !(diag && c0 > r0);
		}
	rdm_v4 re[2][2], im[2][2];
#pragma unroll
	for (int m = 0; m < 2; m++)
#pragma unroll
		for (int n = 0; n < 2; n++) re[m][n] = im[m][n] = rdm_v4 { 0.0, 0.0, 0.0, 0.0 };

	const int ml = lane & 15, mk = lane >> 4;
	gather();
	for (int64_t kb = it.k0; kb < it.k1; kb += kRdmPanel) {
#pragma unroll
		for (int i = 0; i < 4; i++)
#pragma unroll
			for (int p = 0; p < W; p++) {
				sA[p][kq + 4 * i][lane] = ga[i][p];
				if (!diag) sB[p][kq + 4 * i][lane] = gb[i][p];
			}
		__syncthreads();
		if (kb + kRdmPanel < it.k1) gather();
		double (*sBB)[kRdmPanel][kRdmPitch] = diag ? sA : sB;
#pragma unroll
		for (int ks = 0; ks < kRdmPanel / 4; ks++) {
			const int kk = ks * 4 + mk;
			double ar[2], ai[2], br[2], bi[2];
#pragma unroll
			for (int m = 0; m < 2; m++) {
				ar[m] = sA[0][kk][wr * 32 + m * 16 + ml];
				br[m] = sBB[0][kk][wc * 32 + m * 16 + ml];
				if (CPLX) {
					ai[m] = sA[W - 1][kk][wr * 32 + m * 16 + ml];
					bi[m] = sBB[W - 1][kk][wc * 32 + m * 16 + ml];
				}
			}
#pragma unroll
			for (int m = 0; m < 2; m++)
#pragma unroll
				for (int n = 0; n < 2; n++) {
					if (!live[m][n]) continue; // wave-uniform
					re[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[m], br[n], re[m][n], 0, 0, 0);
					if (CPLX) {
						re[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[m], bi[n], re[m][n], 0, 0, 0);
						im[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[m], bi[n], im[m][n], 0, 0, 0);
						im[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai[m], br[n], im[m][n], 0, 0, 0);
					}
				}
		}
		__syncthreads();
	}

#pragma unroll
	for (int m = 0; m < 2; m++)
#pragma unroll
		for (int n = 0; n < 2; n++)
#pragma unroll
			for (int g = 0; g < 4; g++) {
				const int row = wr * 32 + m * 16 + mk + 4 * g, col = wc * 32 + n * 16 + ml;
				if (it.ws >= 0) { // raw partial tile, every element (zeros where nothing was computed)
					double* w = A.ws + (it.ws * W) * kRdmTileElems + row * kRdmTile + col;
					w[0] = re[m][n][g];
					if (CPLX) w[kRdmTileElems] = im[m][n][g];
				} else if (live[m][n] && it.tj * kRdmTile + col < B.d) {
					rdm_store<CPLX>(A.out, B.out_off, B.d, (int64_t)it.ti * kRdmTile + row, (int64_t)it.tj * kRdmTile + col, re[m][n][g], CPLX ? im[m][n][g] : 0.0);
				}
			}
}

// the S partial tiles of one output tile, added in ascending order of the K range
template <bool CPLX> __global__ __launch_bounds__(kRdmBlock) void k_rdm_reduce(RdmArgs A, const RdmItem* __restrict__ reds)
{
	constexpr int W = CPLX ? 2 : 1;
	const RdmItem it = reds[blockIdx.x];
	const RdmBlockDev B = A.blocks[it.block];
	for (int el = threadIdx.x; el < kRdmTileElems; el += kRdmBlock) {
		const int64_t r = (int64_t)it.ti * kRdmTile + (el >> 6), c = (int64_t)it.tj * kRdmTile + (el & 63);
		if (r >= B.d || c > r) continue;
		double re = 0.0, im = 0.0;
		for (int s = 0; s < it.nsplit; s++) {
			const double* w = A.ws + ((it.ws + s) * W) * kRdmTileElems + el;
			re += w[0];
			if (CPLX) im += w[kRdmTileElems];
		}
		rdm_store<CPLX>(A.out, B.out_off, B.d, r, c, re, im);
	}
}

} // namespace lpp
