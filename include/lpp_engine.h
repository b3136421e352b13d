/*
 * lpp_engine.h -- C ABI of the MI355X-native Lanczos inner engine (liblpp_engine.so).
 *
 * Drop-in boundary for ONE path of g1257/LanczosPlusPlus: the stored-CSR ground-state solve
 *   Engine::computeAllStatesBelow            reference src/Engine/Engine.h:601-657
 *     -> InternalProductStored::matrixVectorProduct   src/Engine/InternalProductStored.h:121-124
 *     -> DefaultSymmetry::matrixVectorProduct         src/Engine/DefaultSymmetry.h:112-116
 *     -> CrsMatrix::matrixVectorProduct / LanczosSolver::computeAllStatesBelow [PsimagLite]
 * The reference has no FFI; its boundary is C++ template duck-typing.  These
 * entry points are what a binding of that path needs; INTEGRATION.md shows the C++ shim
 * (InternalProductStored / LanczosSolver look-alikes) that forwards to them.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns an
 * lpp_status (0 = ok); lpp_last_error() gives the message of the last failure on the calling
 * thread.  One engine per host thread; calls block unless stated.  Host buffers stay owned
 * by the caller (the engine copies); device memory is owned by the engine unless a *_device /
 * comm buffer is handed in.  Values are f64 or interleaved (re,im) f64 pairs ("c128").
 * Row pointers are 64-bit (the reference's int row pointers overflow at 4x4 Hubbard).
 * There is NO CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef LPP_ENGINE_H
#define LPP_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPP_ABI_VERSION 7 /* 7: reduced density matrix -- lpp_rdm_plan, lpp_engine_reduced_density_matrix, _host, lpp_engine_state_reduced_density_matrix, lpp_engine_bench_rdm; 6: observables -- LPP_OP_*, lpp_obs_*, lpp_engine_apply_operator, _keep_states, _state_device, *_device start vectors, _two_point, _spectral_decomposition, lpp_continued_fraction; 5: LPP_SPMV_HOLE_MAJOR (lpp_layout.kernel of the t-J model), lpp_engine_set_model_tj / _heisenberg; 4: lpp_layout.segments, lpp_pb_seg_plan_stats; 2: lpp_layout.stream_bytes, lpp_pb_pack_template(bank_ways), set_solver / stream / _ext / _spin entry points; 3: lpp_layout.pieces / coupling_parts / diagonal_plain / chained_step / split_panel, lpp_stats.reortho_* */

typedef int32_t lpp_status;
enum {
	LPP_OK = 0,
	LPP_ERR_INVALID = 1, /* bad argument / shape mismatch */
	LPP_ERR_HIP = 2, /* HIP runtime error (no device, launch failure, ...) */
	LPP_ERR_NOMEM = 3, /* device or host allocation failed */
	LPP_ERR_NOCONV = 4, /* Lanczos / tridiagonal solve failed (caller may fall back, Engine.h:627) */
	LPP_ERR_STATE = 5, /* call sequence error (e.g. solve before set_csr) */
	LPP_ERR_COMM = 6 /* a communicator callback failed */
};

enum { LPP_F64 = 0, LPP_C128 = 1 };

/* SpMV kernel selection (0 = automatic) */
enum { LPP_SPMV_AUTO = 0, LPP_SPMV_ROWGROUP = 1, LPP_SPMV_SLICED = 2, LPP_SPMV_WINDOW = 3,
       LPP_SPMV_PRODUCT = 4, /* reported by lpp_engine_get_layout only: product-basis layout (device-assembled Hubbard) */
       LPP_SPMV_HOLE_MAJOR = 5 /* reported by lpp_engine_get_layout only (ABI 5): the one-orbital t-J model without a stored matrix -- states
                                  ordered (hole configuration, spin pattern of the occupied sites), every entry re-derived per product from
                                  the block's bonds and hole moves (csrc/lpp_tj_kernels.h); rows_per_block = spin patterns per hole configuration */ };

typedef struct lpp_engine lpp_engine;

/* Solver parameters; mirrors what the reference reads through
 * ParametersForSolver(io,"Lanczos") (Engine.h:609): LanczosSteps=, LanczosEps=, LanczosMinSteps=,
 * LanczosOptions=reortho, lotaMemory (SpinOrbital.cpp:213-216). */
typedef struct lpp_config {
	int32_t abi_version; /* must be LPP_ABI_VERSION */
	int32_t device; /* HIP device ordinal */
	int32_t dtype; /* LPP_F64 | LPP_C128 */
	int32_t max_steps; /* LanczosSteps (default 200) */
	int32_t min_steps; /* LanczosMinSteps (default 4) */
	int32_t reortho; /* 1: blocked CGS2 against the on-device Krylov basis every step */
	int32_t save_vectors; /* lotaMemory: 1 keep Lanczos vectors in HBM, 0 two-pass Ritz vectors, -1 auto */
	int32_t check_lag; /* steps the GPU may run ahead of the host convergence test (default 2) */
	int32_t spmv_kernel; /* LPP_SPMV_* */
	int32_t time_kernels; /* 1: bracket every SpMV launch with HIP events (for bench/roofline) */
	double eps; /* LanczosEps (default 1e-12); <= 0 disables the convergence test */
	uint64_t seed; /* seed of the built-in start vector (used when init == NULL) */
	void* stream; /* hipStream_t to run on; NULL = engine-owned stream */
	int32_t compress_values; /* lossless 8-bit value dictionary when the matrix has <= 256 distinct doubles: -1 auto, 0 off, 1 on */
	int32_t reserved;
} lpp_config;

typedef struct lpp_stats {
	int32_t steps; /* Lanczos steps that define the returned tridiagonal matrix */
	int32_t steps_enqueued; /* including run-ahead steps discarded by the lagged test */
	int32_t converged;
	int32_t vectors_saved;
	int64_t nrows, nnz;
	double seconds_total; /* wall time of the solve call */
	double spmv_ms_total; /* sum of event-timed SpMV launches (time_kernels=1) */
	int64_t spmv_launches;
	double spmv_bytes; /* algorithmic bytes of one SpMV: Z(s+4) + (N+1)8 + 3Ns */
	double reortho_ms_total; /* sum of event-timed blocked Gram-Schmidt calls (time_kernels=1, reortho=1): both CGS2 passes of a step */
	int64_t reortho_calls;
	double reortho_columns; /* Krylov columns orthogonalised against, summed over the timed calls */
} lpp_stats;

/* How a stored matrix is laid out in HBM (introspection for tests, bench.py and DESIGN.md; no effect on results). */
typedef struct lpp_layout {
	int32_t kernel; /* LPP_SPMV_ROWGROUP / _SLICED / _WINDOW actually selected */
	int32_t coded; /* 1: values stored as 8-bit dictionary codes */
	int32_t local16; /* 1: per-row columns stored as 16-bit block-local indices */
	int32_t shared_stride; /* places per 64-row slice for shared-offset entries (0: none) */
	int32_t block_template; /* block-periodic structure: 1 = row lengths and local columns stored once for all row blocks, 2 = value codes too */
	int32_t diagonal_codes; /* 1: the diagonal travels as one dictionary code per row, apart from the per-row entries */
	int64_t nnz; /* entries of the CSR this layout represents */
	int64_t per_row_entries; /* entries kept per row */
	int64_t shared_entries; /* entries stored once per slice, summed over slices */
	int64_t rows_per_block; /* row block of the sliced layout */
	int64_t resident_bytes; /* device bytes held for this matrix */
	int64_t stream_bytes; /* bytes of matrix data ONE product has to read at least once (arrays kept only for
	                         lpp_engine_get_csr and block-0 templates that stay in L2 are not streamed);
	                         stream_bytes + 3*rows*sizeof(value) is the least HBM traffic of x += H y in this layout */
	int32_t pieces; /* product-basis layout: LDS-window pieces a block's row is cut into (1: the whole row fits one window) */
	int32_t coupling_parts; /* product-basis layout: parts of the source-block range the coupling kernel walks per panel (1: whole panel) */
	int32_t diagonal_plain; /* product-basis layout: 1 = the diagonal is a plain f64 stream (more than 256 distinct values), 0 = one code per row */
	int32_t chained_step; /* product-basis layout: 1 = a scale-free Lanczos step is the chained pair of launches (k_pb_up<CHAIN> + k_pb_down<RMW>),
	                         0 = product kernels + one streaming pass that also applies the recurrence update */
	int32_t split_panel; /* general layout: > 0 = the entries that leave the row blocks are held apart in that many matrices (by source block
	                        range), rows in panel-major order (16 positions of every block, then the next 16), each applied by a launch of
	                        its own that gathers from L2 */
	int32_t rows_by_list_length; /* product-basis layout (was `reserved`, always 0, until round 3): 1 = inside a block the positions are stored in the
	                                order of their in-block list lengths, not in the basis order (slices of rows with equal lists: fewer template
	                                slots).  Internal: vectors, lpp_engine_get_csr and the start vector keep the basis order at the boundary */
	int32_t segments; /* product-basis layout, rows beyond one LDS window (ABI 4): > 0 = the in-block matrix is held decomposed by the high sites of
	                     the species' basis word into that many segments (k_pb_up_seg; positions stored segment by segment, longest first -- internal
	                     as above); 0 = one per-position template for the whole row */
	int32_t coupling_rounds; /* product-basis layout (was `reserved2`, always 0, until round 5): pieces of a workgroup's block range the coupling
	                            kernel walks inside every panel, one LDS image of coupling lists each (1: one image per launch; > 1: sectors of
	                            65536 blocks and more); 0: not a product-basis layout */
} lpp_layout;

/* Communicator for the 1-D row-partitioned multi-GPU path.  The engine never
 * opens sockets itself: the host (torch.distributed over RCCL in bench.py) supplies the
 * collectives and owns the exchange buffers.
 *   send_buf : device, shard_stride elements, 16-byte aligned (this rank's slice of the Lanczos vector, zero padded)
 *   gath_buf : device, nranks*shard_stride elems  (slice r at gath_buf + r*shard_stride)
 *   red_buf  : device doubles, red_len >= 6*(max_steps+2)   (a_j, b_j^2 and reortho coefficients)
 * allgather_begin may return before the gather completes (so the local-column SpMV overlaps
 * it); allgather_end makes the engine stream wait for it.  All callbacks return 0 on success. */
typedef struct lpp_comm {
	int32_t rank, nranks;
	void* ctx;
	void* send_buf;
	void* gath_buf;
	double* red_buf;
	int64_t shard_stride;
	int32_t red_len;
	int32_t (*allgather_begin)(void* ctx);
	int32_t (*allgather_end)(void* ctx);
	int32_t (*allreduce_sum)(void* ctx, int32_t offset, int32_t count); /* in place on red_buf[offset..] */
	/* Optional transposition exchange (lpp_engine_assemble_hubbard only; all four NULL/0 = all-gather path).
	 * Two all-to-alls of nranks equal chunks of xchg_chunk elements each:
	 *   which 0: chunk p of send_buf  -> rank p, received into chunk (sender) of gath_buf
	 *   which 1: chunk p of send2_buf -> rank p, received into chunk (sender) of recv2_buf
	 * send_buf, gath_buf, send2_buf, recv2_buf then hold nranks*xchg_chunk elements (zero-initialised by the owner).
	 * xchg_chunk = ceil(N_down/nranks) * peru, peru = up indices per rank >= ceil(N_up/nranks).  With peru rounded up to a
	 * multiple of 16 a real Hubbard matrix takes the product-basis kernels on both parts of the product;
	 * helper: lpp_xchg_chunk(). */
	void* send2_buf;
	void* recv2_buf;
	int64_t xchg_chunk;
	int32_t (*exchange_begin)(void* ctx, int32_t which);
	int32_t (*exchange_end)(void* ctx, int32_t which);
} lpp_comm;

const char* lpp_last_error(void);
int32_t lpp_abi_version(void);
void lpp_config_default(lpp_config* cfg);

lpp_status lpp_engine_create(lpp_engine** out, const lpp_config* cfg);
lpp_status lpp_engine_destroy(lpp_engine* e);
/* the hipStream_t the engine enqueues on (lpp_config.stream, or the engine-owned one): what a communicator
 * (include/lpp_comm_rccl.h) has to order its collectives against */
void* lpp_engine_stream(lpp_engine* e);

/* Solver parameters after creation: the reference builds its LanczosSolver(hamiltonian, params) AFTER the InternalProduct that
 * owns the matrix (Engine.h:608-610), so the shim's LanczosSolver pushes ParametersForSolver (LanczosSteps=, LanczosMinSteps=,
 * LanczosEps=, LanczosOptions=reortho, lotaMemory) into the engine here.  Not while a Lanczos run is active; with a
 * communicator attached comm.red_len must cover the new max_steps.  The matrix stays resident. */
lpp_status lpp_engine_set_solver(lpp_engine* e, int32_t max_steps, int32_t min_steps, double eps, int32_t reortho,
                                 int32_t save_vectors);

/* ---- the stored Hamiltonian (replaces DefaultSymmetry::matrixStored_, DefaultSymmetry.h:120) ---- */

/* Optional layout hint for the NEXT lpp_engine_set_csr / _set_csr_partition: the basis index is blocked in runs of
 * `rows_per_block` consecutive states whose in-block couplings dominate -- N_up for the Hubbard product basis
 * index = i_up + i_down * N_up (BasisHubbardLanczos.h:59-63).  The engine then stages one block of the source vector
 * in LDS per workgroup.  0 = unknown (default).  Results do not depend on it. */
lpp_status lpp_engine_set_row_block(lpp_engine* e, int64_t rows_per_block);

/* Optional description of the MODEL behind the next lpp_engine_set_csr / _set_csr_device (ABI 5; like lpp_engine_set_row_block a layout hint: results
 * never depend on it).  The reference hands its matrix over as a CSR (DefaultSymmetry.h:54-57 -> InternalProductStored.h:116); for two model
 * families the engine has a form that needs no stored matrix at all -- the one-orbital t-J model (TjMultiOrb.h:100-131; arguments as
 * lpp_engine_assemble_tj) and the S = 1/2 Heisenberg chain (Heisenberg.h:80-114; arguments as lpp_engine_assemble_heisenberg).  With a description
 * on record the engine regenerates the matrix from it with its device assembler, compares that with the handed-over CSR BIT FOR BIT, and only
 * if they are the same holds the model in its structured form (lpp_layout.kernel LPP_SPMV_HOLE_MAJOR / LPP_SPMV_PRODUCT) and drops the CSR;
 * any difference, a model the form does not apply to, or no room for the comparison keeps the general layout of the CSR as handed over.
 * The description is used for ONE matrix; nsites == 0 forgets it.  The C++ shim records it from the model object (host/EngineGpu.h). */
lpp_status lpp_engine_set_model_tj(lpp_engine* e, int32_t nsites, int32_t nup, int32_t ndown, const double* hop_re, const double* hop_im,
                                   const double* jpm, const double* jzz, const double* w, const double* potentialV, int32_t npot);
lpp_status lpp_engine_set_model_heisenberg(lpp_engine* e, int32_t nsites, int32_t szPlusConst, const double* jpm, const double* jzz,
                                           const double* field, int32_t nfield);

/* Upload a host CSR (copied).  rowptr[nrows+1], colind[nnz], values[nnz] of the engine dtype. */
lpp_status lpp_engine_set_csr(lpp_engine* e, int64_t nrows, const int64_t* rowptr, const int32_t* colind,
                              const void* values);
/* The same from DEVICE pointers of the engine's GPU (copied device-to-device, validated on the device): for hosts that
 * assemble on the GPU themselves (SURVEY 8(b) `_set_csr_device`).  Honours lpp_engine_set_row_block. */
lpp_status lpp_engine_set_csr_device(lpp_engine* e, int64_t nrows, const int64_t* d_rowptr, const int32_t* d_colind,
                                     const void* d_values);

/* Row-partitioned upload for rank `comm->rank`: rows [row_start, row_start+local_rows) of a
 * global_rows x global_rows matrix, colind holding GLOBAL column indices, rowptr relative to the
 * block (rowptr[0]==0).  shard_starts[nranks+1] gives every rank's first row.  The engine splits
 * the block into a local-column and a remote-column CSR (lpp_split_csr). */
lpp_status lpp_engine_set_csr_partition(lpp_engine* e, const lpp_comm* comm, int64_t global_rows,
                                        const int64_t* shard_starts, const int64_t* rowptr, const int32_t* colind,
                                        const void* values);

/* On-device assembly of the Hubbard Hamiltonian (GPU restatement of HubbardHelper::setupHamiltonian,
 * src/Models/HubbardOneOrbital/HubbardHelper.h:75-103, in the BasisHubbardLanczos ordering
 * rank(up) + rank(down)*N_up, BasisHubbardLanczos.h:59-63).  hop_re/hop_im: L*L row-major
 * hoppings_(i,j) (hop_im NULL for real); U[L]; V[L] (potentialV[i], i<L, both spins).
 * comm == NULL: whole matrix on this GPU.  Otherwise rows are partitioned at multiples of N_up
 * (shard_starts returned through comm-side helper lpp_partition_rows). */
lpp_status lpp_engine_assemble_hubbard(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup,
                                       int32_t ndown, const double* hop_re, const double* hop_im, const double* U,
                                       const double* V);

/* The same with the Coulomb term of Model=HubbardOneBandExtended (ModelSelector.h:76-80): the diagonal gains
 * 0.5 * sum_{i,j} ninj[i*L+j] (n_i,up + n_i,down)(n_j,up + n_j,down), ninj = the second geometry term (HubbardHelper.h:167-177,362-366).
 * ninj == NULL is lpp_engine_assemble_hubbard. */
lpp_status lpp_engine_assemble_hubbard_ext(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup, int32_t ndown,
                                           const double* hop_re, const double* hop_im, const double* U, const double* V,
                                           const double* ninj);

/* Model=SuperHubbardExtended (ModelSelector.h:76-80): Coulomb coupling ninj (geometry term 1) and spin coupling jcoup (term 2):
 * sum_ij J_ij/2 Sz_i Sz_j on the diagonal (HubbardHelper.h:158-165) and the spin-flip terms of setJTermOffDiagonal (:282-330).
 * Either may be NULL.  The spin-flip terms move both species, so the matrix takes the general layout and, on several GPUs, the
 * all-gather exchange.  Model=KaneMeleHubbard needs no entry point of its own: its hoppings are term 0 + term 1 (:63-66). */
lpp_status lpp_engine_assemble_hubbard_super(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup, int32_t ndown,
                                             const double* hop_re, const double* hop_im, const double* U, const double* V,
                                             const double* ninj, const double* jcoup);

/* Matrix-free Hubbard product (the GPU counterpart of SolverOptions=InternalProductOnTheFly:
 * InternalProductOnTheFly.h:120-123 -> HubbardHelper::matrixVectorProduct, HubbardHelper.h:105-134).
 * No CSR is stored: H = H_up (x) 1 + 1 (x) H_down + diag(U n_up n_down) in the BasisHubbardLanczos ordering;
 * only the two one-species matrices live in HBM.  Same arguments as lpp_engine_assemble_hubbard; every
 * solver entry point works unchanged afterwards, lpp_engine_get_csr does not -- except where one species' row fits the LDS
 * window (real hoppings, >= 32 MB per vector): there the matrix-free form is the product-basis layout (the two one-species
 * matrices + one diagonal code per row), the engine lpp_engine_assemble_hubbard builds, and lpp_engine_get_csr / _get_layout work. */
lpp_status lpp_engine_setup_hubbard_onthefly(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup,
                                             int32_t ndown, const double* hop_re, const double* hop_im, const double* U,
                                             const double* V);

lpp_status lpp_engine_setup_hubbard_onthefly_ext(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup, int32_t ndown,
                                                 const double* hop_re, const double* hop_im, const double* U, const double* V,
                                                 const double* ninj);

/* The same for Model=SuperHubbardExtended (ModelSelector.h:76-80): the reference's on-the-fly product applies setJTermOffDiagonal as well
 * (HubbardHelper.h:119-129, :282-330).  Those spin-flip terms move both species, so H is no longer H_up (x) 1 + 1 (x) H_down + D: with a
 * non-zero jcoup every row re-derives its entries from the term list per product (k_asm_apply), storing nothing -- the literal
 * counterpart of the reference's per-row walk, on one GPU.  jcoup == NULL (or all zero) is lpp_engine_setup_hubbard_onthefly_ext. */
lpp_status lpp_engine_setup_hubbard_onthefly_super(lpp_engine* e, const lpp_comm* comm, int32_t nsites, int32_t nup, int32_t ndown,
                                                   const double* hop_re, const double* hop_im, const double* U, const double* V,
                                                   const double* ninj, const double* jcoup);

/* On-device assembly of the S=1/2 Heisenberg Hamiltonian (Heisenberg.h:80-114,242-307) in the
 * BasisHeisenberg ordering (ascending words of fixed popcount, BasisHeisenberg.h:38-46). */
lpp_status lpp_engine_assemble_heisenberg(lpp_engine* e, int32_t nsites, int32_t szPlusConst, const double* jpm,
                                          const double* jzz, const double* field, int32_t nfield);

/* The same for any spin the reference's digit width holds (BasisHeisenberg.h:28-46: a state is L digits m_i + S of
 * bits = 1 + floor(log2(twiceS+1)) bits, one bit less for odd twiceS; ascending words of digit sum szPlusConst), with
 * the S+S- amplitudes of Heisenberg.h:278-307 and the single-ion anisotropy of Heisenberg.h:259.  Odd twiceS whose
 * digits the reference cannot hold (twiceS + 1 not a power of two) -> LPP_ERR_INVALID.  twiceS == 1 gives the matrix
 * of lpp_engine_assemble_heisenberg. */
lpp_status lpp_engine_assemble_heisenberg_spin(lpp_engine* e, int32_t nsites, int32_t twiceS, int32_t szPlusConst,
                                               const double* jpm, const double* jzz, const double* field, int32_t nfield,
                                               const double* anisotropy, int32_t naniso);

/* On-device assembly of the one-orbital t-J Hamiltonian (TjMultiOrb.h:100-131,586-783) in the
 * BasisTjMultiOrbLanczos ordering (sorted (down<<L)|up words without double occupancy). */
lpp_status lpp_engine_assemble_tj(lpp_engine* e, int32_t nsites, int32_t nup, int32_t ndown, const double* hop_re,
                                  const double* hop_im, const double* jpm, const double* jzz, const double* w,
                                  const double* potentialV, int32_t npot);

/* Copy the device CSR back (for parity tests of the assemblers).  Pass NULL pointers to query
 * sizes only.  which: 0 = whole/local-column part, 1 = remote-column part. */
lpp_status lpp_engine_get_csr(lpp_engine* e, int32_t which, int64_t* nrows, int64_t* nnz, int64_t* rowptr,
                              int32_t* colind, void* values);

/* ---- A1: x += H y  (InternalProductStored::matrixVectorProduct) on host buffers ---- */
lpp_status lpp_engine_spmv_acc(lpp_engine* e, void* x_inout, const void* y);

/* ---- A2/A3: the Lanczos solve (LanczosSolver::computeAllStatesBelow, Engine.h:626) ----
 * init: host start vector of local_rows elements or NULL (built-in splitmix64 vector, same as the oracle).
 * eigs[nstates]; ritz_vectors: host buffer nstates*local_rows elements or NULL. */
lpp_status lpp_engine_lanczos(lpp_engine* e, const void* init, int32_t nstates, double* eigs, void* ritz_vectors,
                              lpp_stats* stats);

/* LanczosSolver::decomposition (Engine.h:478): tridiagonal coefficients only.
 * a[max_steps], b[max_steps]; *nsteps receives the number of valid entries. */
lpp_status lpp_engine_decomposition(lpp_engine* e, const void* init, int32_t* nsteps, double* a, double* b,
                                    lpp_stats* stats);

/* ---- incremental interface (bench.py times exactly K steps with it) ---- */
lpp_status lpp_engine_lanczos_begin(lpp_engine* e, const void* init);
lpp_status lpp_engine_lanczos_step(lpp_engine* e, int32_t nsteps); /* enqueue only, no host sync */
lpp_status lpp_engine_sync(lpp_engine* e);
/* copy out the coefficients produced so far (after a sync): a[steps], b[steps] */
lpp_status lpp_engine_lanczos_coeffs(lpp_engine* e, int32_t* steps, double* a, double* b);
lpp_status lpp_engine_get_stats(lpp_engine* e, lpp_stats* stats);
/* which: 0 = local part (or the whole matrix on one GPU), 1 = remote part of a partitioned matrix */
lpp_status lpp_engine_get_layout(lpp_engine* e, int32_t which, lpp_layout* layout);

/* Time `iters` back-to-back SpMV launches (x += H y on resident vectors) with HIP events on the
 * engine stream; returns the average milliseconds per launch. */
lpp_status lpp_engine_bench_spmv(lpp_engine* e, int32_t warmup, int32_t iters, double* ms_per_launch);

/* ---- host-only helpers (no GPU needed; covered by the CPU test-suite) ---- */

/* 1-D contiguous row partition: starts[nranks+1]; boundaries are multiples of `block`
 * (N_up for the Hubbard product basis so that up-hops and the diagonal stay rank-local). */
/* xchg_chunk for the transposition exchange: ceil(n_down/nranks) * (ceil(n_up/nranks) rounded up to a multiple of 16) */
int64_t lpp_xchg_chunk(int64_t n_up, int64_t n_down, int32_t nranks);

lpp_status lpp_partition_rows(int64_t nrows, int32_t nranks, int64_t block, int64_t* starts);

/* Split a row block with global columns into local-column and remote-column CSRs.
 * Local columns become offsets into the rank's own slice; remote columns become indices into the
 * padded gather buffer (owner*shard_stride + offset).  Two-call protocol: with out pointers NULL
 * only nnz_loc / nnz_rem are returned. */
lpp_status lpp_split_csr(int32_t rank, int32_t nranks, const int64_t* shard_starts, int64_t shard_stride,
                         int64_t local_rows, const int64_t* rowptr, const int32_t* colind, const void* values,
                         int32_t elem_bytes, int64_t* nnz_loc, int64_t* nnz_rem, int64_t* rowptr_loc,
                         int32_t* colind_loc, void* values_loc, int64_t* rowptr_rem, int32_t* colind_rem,
                         void* values_rem);

/* Lowest `k` eigenvalues (and optionally eigenvectors, row-major z[j*n+i] = component j of vector i)
 * of the symmetric tridiagonal matrix (d[n], e[n-1]) -- the host part of the Lanczos loop. */
lpp_status lpp_tridiag_lowest(int32_t n, const double* d, const double* e, int32_t k, double* w, double* z);

/* Product-basis layout, host part (used by lpp_engine_assemble_hubbard; exposed for the CPU test-suite): packs the in-block
 * matrix `rows` x `rows` (CSR, diagonal entries skipped) into per-slice, per-value-group streams of 16-bit LDS window indices
 * (chunks of 4 slots = two 32-bit words per lane) with a slot assignment in which no LDS bank is asked for more than
 * `bank_ways` (1..4) different addresses per half-wave and slot.  pitch: multiple of 16, >= rows.  Two-call protocol:
 * off/len/words NULL returns sizes only (ngroups, slices, nwords).  group_values holds 8 doubles; off/len count chunks. */
lpp_status lpp_pb_pack_template(int64_t rows, int64_t pitch, const int64_t* rowptr, const int32_t* colind, const double* values,
                                int32_t* ngroups, double* group_values, int32_t* slices, int64_t* nwords, int32_t* off, uint16_t* len,
                                uint32_t* words, int64_t* entries, int64_t* slots, int32_t bank_ways);

/* Product-basis layout, rows beyond one LDS window, host part (ABI 4; exposed for the CPU test-suite): reads the species' basis (L sites,
 * n particles, ascending words: BasisOneSpin.h:53-61) and the hopping amplitudes off the in-block matrix `rows` x `rows` (CSR, diagonal
 * entries skipped; HubbardHelper.h:191-243 for one species), decomposes it by the high sites of the basis word (csrc/lpp_pbseg.h), expands
 * the packed description again and compares it with the matrix entry by entry, bit by bit.  wcap: longest segment (64..8128).
 * out[0] = 1 if the decomposition applies and reproduces the matrix, then out[1..13] = L, n, high sites, segments, items, item types,
 * longest item, bytes shared by class, bytes per segment, low-low entries of the item types, their lane-slots, value groups, window stride;
 * perm (rows int32, may be NULL): stored position -> basis index. */
lpp_status lpp_pb_seg_plan_stats(int64_t rows, const int64_t* rowptr, const int32_t* colind, const double* values, int32_t wcap, int64_t* out, int32_t* perm);

/* The t-J model's hole-major form, host part (ABI 5; exposed for the CPU test-suite): plans the form from (sites, sector, hoppings, J+-) -- hole
 * configurations, spin patterns and their ranking, work items, every configuration's bonds and moves (csrc/lpp_tj.h) -- and, given a CSR of the
 * model in the reference's basis order (BasisTjMultiOrbLanczos.h:29-42), expands the plan again exactly as the kernel walks it and compares it
 * with the CSR's off-diagonal entries, columns and value bits (the diagonal comes from the device assembler, not from the plan).
 * out[0] = 1 if the plan applies (and reproduces every row when a CSR is given; rowptr NULL: statistics only), out[1..9] = hole configurations,
 * spin patterns, low positions of a segment, work items, bonds, moves, bonds among the low positions, most bonds / moves of one configuration. */
lpp_status lpp_tj_plan_stats(int32_t nsites, int32_t nup, int32_t ndown, const double* hop_re, const double* hop_im, const double* jpm, int64_t nrows,
                             const int64_t* rowptr, const int32_t* colind, const void* values, int32_t is_complex, int64_t* out);

/* ---- observables of the Hubbard product basis (ABI 6; one GPU; csrc/lpp_obs.hip) ----
 * What the reference's users run after the ground state in the same `lanczos` call: -c <op> (Engine::twoPoint, Engine.h:266-338) and
 * -g <op> (Engine::spectralFunction :134-206).  Models: HubbardOneBand, HubbardOneBandExtended, SuperHubbardExtended, KaneMeleHubbard
 * (all on BasisHubbardLanczos).  A partitioned (multi-rank) engine or a hole-major t-J engine handed to any of these entry points returns
 * LPP_ERR_STATE with a message. */

/* operators, numbered as LabeledOperator::Label (LabeledOperator.h:10-17) */
enum { LPP_OP_C = 1, LPP_OP_SZ = 2, LPP_OP_CDAGGER = 3, LPP_OP_N = 4, LPP_OP_SPLUS = 5, LPP_OP_SMINUS = 6 };
enum { LPP_SPIN_UP = 0, LPP_SPIN_DOWN = 1 }; /* ProgramGlobals.h:105 */

/* HubbardOneOrbital::hasNewParts (HubbardOneOrbital.h:87-109, :212-253), host only: *has = 1 and the new (nup, ndown), or *has = 0 where the
 * reference returns false (a count below 0 or above nsites, the (0,0) sector for c / cdagger, sz).  LPP_OP_N: the reference throws -> LPP_ERR_INVALID. */
lpp_status lpp_obs_new_parts(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* The plan of one operator application (host only; exposed for the CPU test-suite): the sector the operator leads to (n and sz stay, LabeledOperator.h:83-90)
 * and the two per-species tables the kernel reads, table[destination species rank] = +-(source species rank + 1) or 0 = none, ranks as
 * BasisOneSpin::perfectIndex (BasisOneSpin.h:73-81).  The entry's sign is the species' share of doSignGf (BasisHubbardLanczos.h:106-137; for SPIN_DOWN
 * the parity of the down bits below the site -- at site 0 the parity of the up electrons, folded into the down table) and doSignSpSm (:151-160).
 * For LPP_OP_SZ the tables are the two occupancy tables of n and the value is (up occupied) - (down occupied) (getBraIndexSz :210-223: +1 / -1 / none, not +-1/2).
 * table_up[n_up_dst], table_down[n_down_dst]; NULL tables: sizes only.  *has = 0: hasNewParts refused, nothing else is written. */
lpp_status lpp_obs_plan(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                        int64_t* n_up_dst, int64_t* n_down_dst, int32_t* table_up, int32_t* table_down);

/* Engine::accModifiedState_ (Engine.h:416-458) on device vectors of the engine's GPU and dtype, both in the basis order rank(up) + rank(down) * N_up
 * (BasisHubbardLanczos.h:59-63):  z[bra] += factor * sign * value * src[ket]  (accumulate = 0: z = ..., destinations the reference does not touch
 * are written as 0).  d_src: C(nsites,nup)*C(nsites,ndown) elements, d_dst: the new sector's, 16-byte aligned.  One launch on the engine's stream,
 * no host sync; destination driven, no atomics (csrc/lpp_obs_kernels.h).  The engine needs no matrix.  *has = 0: no such sector, nothing was done. */
lpp_status lpp_engine_apply_operator(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                     double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
/* the same on host vectors (copied in and out; dst is read only when accumulate != 0) */
lpp_status lpp_engine_apply_operator_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                          double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has);
/* Time `iters` accumulating applications on zeroed resident vectors with HIP events; model_bytes = sizeof(value) * (2 N_dst + source entries read). */
lpp_status lpp_engine_bench_operator(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                     double* ms_per_launch, double* model_bytes);

/* Keep the lowest k Ritz vectors of the NEXT lpp_engine_lanczos / _lanczos_device on the device (Engine::vectors_, Engine.h:601-657), in the basis
 * order -- unpitched, un-permuted whatever the layout stores -- on both Ritz paths (saved Krylov basis, two-pass replay).  The host buffer of
 * lpp_engine_lanczos may then be NULL.  k = 0 (default): nothing is kept.  The states live until the engine is destroyed or the next lpp_engine_lanczos / _lanczos_device
 * starts: from then on pointers returned by lpp_engine_state_device are invalid (the buffer may be reallocated), and a solve that fails leaves no state. */
lpp_status lpp_engine_keep_states(lpp_engine* e, int32_t k);
/* device pointer (16-byte aligned) and length in elements of resident state k */
lpp_status lpp_engine_state_device(lpp_engine* e, int32_t k, void** d_ptr, int64_t* len);
lpp_status lpp_engine_state_to_host(lpp_engine* e, int32_t k, void* host);

/* lpp_engine_lanczos / _lanczos_begin / _decomposition with a DEVICE start vector: d_init holds rows() elements in the basis order on the engine's
 * GPU (not NULL) and is copied into the internal form on the device; everything else as the host-vector entry points. */
lpp_status lpp_engine_lanczos_device(lpp_engine* e, const void* d_init, int32_t nstates, double* eigs, void* ritz_vectors, lpp_stats* stats);
lpp_status lpp_engine_lanczos_begin_device(lpp_engine* e, const void* d_init);
lpp_status lpp_engine_decomposition_device(lpp_engine* e, const void* d_init, int32_t* nsteps, double* a, double* b, lpp_stats* stats);

/* Engine::twoPoint (Engine.h:266-338) for resident states bra_state / ket_state of sector (nup, ndown):
 *   result[i * nsites + j] = (A_j^{spin2} bra) . (A_i^{spin1} ket),  the left factor conjugated for c128,
 * the modified vectors built as Engine::accModifiedState does (:535-599: n directly, sz as n_up/2 - n_down/2, the others as given).  An operator
 * that leads to no sector leaves the matrix at the reference's -100 fill (:303-305).  c / cdagger / splus / sminus with spin1 != spin2 ->
 * LPP_ERR_INVALID (the reference throws, :276-282).  result: nsites*nsites values of the engine dtype; trace (one value, may be NULL): the sum
 * of the diagonal the reference prints as MatrixDiagonal (:337).  The bra vectors are built in panels sized to the free memory and contracted
 * with the panel-dot kernel of the blocked Gram-Schmidt. */
lpp_status lpp_engine_two_point(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                int32_t ket_state, void* result, void* trace);

/* One type of Engine::spectralFunction (Engine.h:160-205): the modified state  A_i gs + isign A_j gs  (getModifiedState :494-533 -- for i == j the
 * state is accumulated twice, as the reference does for this model) is built on the device from resident state `state` of e, *weight = <modif|modif>
 * (calcSpectral :479), and `sector` -- an engine on the same GPU holding the Hamiltonian of the operator's sector (lpp_obs_new_parts) -- runs
 * LanczosSolver::decomposition from it (:478) with its own solver parameters (ParametersForSolver(io,"Spectral")).  a, b, nsteps, stats as
 * lpp_engine_decomposition.  The caller picks the operator of the type (odd: the operator, even: its transpose-conjugate, :163) and isign
 * (-1 for types above 1, :521), keeps the sector engines alive across calls and applies s / s2 of :481-489. */
lpp_status lpp_engine_spectral_decomposition(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                             int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats);

/* Host helper: a record (a[n], b[n], Eg, w = weight*s2, sigma = -s: the argument list of cf.set, Engine.h:489) evaluated at complex z,
 *   G(z) = w / (z + sigma (a_0 - Eg) - b_0^2 / (z + sigma (a_1 - Eg) - b_1^2 / ...)),   b_k = the coefficient lpp_engine_decomposition returns at index k.
 * This is this project's stated convention: PsimagLite's ContinuedFraction was not available to compare with.  out[2] = (re, im). */
lpp_status lpp_continued_fraction(int32_t n, const double* a, const double* b, double eg, double weight, double sigma, double z_re, double z_im, double* out);

/* ---- observables of the one-orbital t-J basis (entry points added under ABI 7, no struct changes; one GPU; csrc/lpp_obs.hip, csrc/lpp_obs_tj_kernels.h) ----
 * The same three user-level results for Model=TjMultiOrb with Orbitals=1 (BasisTjMultiOrbLanczos: the sorted words (down << L) | up without double
 * occupancy, index = rank(up compressed onto the sites the down electrons leave free) + rank(down) * C(L - ndown, nup)).  Operators c, cdagger, n, sz,
 * splus, sminus (BasisTjMultiOrbLanczos.h:163-245, :296-315, :414-469).  Semantics, as the reference RUNS:
 *   - doSignGf (:163-192) carries the parity of the up electrons for SPIN_DOWN at every site, site 0 included (no site-0 quirk as in the Hubbard basis);
 *   - splus / sminus carry no sign (doSignSpSm is BasisBase's 1);
 *   - a raw application of sz is n of the given spin (getBraSzOrN :456-469); two-point and spectral calls build sz as n_up/2 - n_down/2 (Engine.h:535-599);
 *   - Engine.h:519 / :546 test the model name "Tj1Orb.h", which TjMultiOrb never has: a diagonal pair accumulates the modified state twice, as for Hubbard;
 *   - splus / sminus with LPP_SPIN_DOWN -> LPP_ERR_INVALID from every call that applies them: hasNewPartsSplusOrMinus then names the sector
 *     (nup -+ 1, ndown +- 1) while getBraIndex ignores the spin and makes states of (nup +- 1, ndown -+ 1) -- the reference ranks words that are not in
 *     the basis.  lpp_obs_new_parts_tj itself restates hasNewParts and answers for both spins.
 * Sector sizes are C(L, ndown) * C(L - ndown, nup); nup + ndown <= nsites <= 30; an operator that changes the up pattern needs at most 24 sites free of down
 * electrons in the source sector (the pattern rank tables live in LDS) -> LPP_ERR_INVALID beyond.  Only a partitioned engine is refused (LPP_ERR_STATE):
 * `e` and `sector` may be hole-major or general-layout t-J engines.  Every ABI-6 / ABI-7 entry point above and below keeps its behaviour, refusals included. */

/* TjMultiOrb::hasNewParts (TjMultiOrb.h:140-159, :538-584), host only: as lpp_obs_new_parts, plus "nup + ndown > nsites -> no sector", the (0,0) refusal for
 * splus / sminus too, and splus / sminus reading the spin.  LPP_OP_N and LPP_OP_SZ: the reference throws -> LPP_ERR_INVALID. */
lpp_status lpp_obs_new_parts_tj(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* The plan of one operator application, expanded (host only; exposed for the CPU test-suite): action[dst] = +-(src + 1), or 0 where the reference does not
 * touch destination dst; *n_dst entries.  Expanded through the same tables and the same lookup function (obs_tj_source) the kernel uses.  action == NULL:
 * sizes only.  *has = 0: hasNewParts refused, nothing else is written.  An empty species (nup = 0 or ndown = 0) is a valid sector. */
lpp_status lpp_obs_plan_tj(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                           int64_t* n_dst, int64_t* action);

/* lpp_engine_apply_operator / _host / lpp_engine_bench_operator in the t-J basis: arguments and contracts as those calls (basis-order vectors, 16-byte aligned
 * destination, one launch on the engine's stream, no sync; the same byte model).  The engine needs no matrix. */
lpp_status lpp_engine_apply_operator_tj(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                        double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_tj_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                             double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_bench_operator_tj(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                        double* ms_per_launch, double* model_bytes);

/* lpp_engine_keep_states that also accepts a hole-major t-J engine: its resident states are then the host Ritz vectors bit for bit (both are permutations
 * of the same device vector).  A second name only because lpp_engine_keep_states keeps the refusal its ABI-6 block documents; lpp_engine_state_device and
 * lpp_engine_state_to_host serve any resident state.  A later lpp_engine_keep_states call puts the refusal back. */
lpp_status lpp_engine_keep_states_tj(lpp_engine* e, int32_t k);

/* lpp_engine_two_point / lpp_engine_spectral_decomposition in the t-J basis, arguments as those calls; one body serves both families.  A hole-major sector
 * engine takes the modified state through its permutation on the device. */
lpp_status lpp_engine_two_point_tj(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                   int32_t ket_state, void* result, void* trace);
lpp_status lpp_engine_spectral_decomposition_tj(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                                int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats);

/* ---- observables of the S = 1/2 Heisenberg basis (entry points added under ABI 7, no struct changes; one GPU; csrc/lpp_obs.hip, csrc/lpp_obs_heis_kernels.h) ----
 * The same three user-level results for Model=Heisenberg with HeisenbergTwiceS=1 (BasisHeisenberg: the nsites-bit words with szPlusConst set bits, ascending;
 * a set bit is an up spin; index = position in that list).  Arguments as the _tj calls with nup = szPlusConst; ndown is not read, and a new sector is reported
 * as (szPlusConst', 0) -- the convention of LPP_BASIS_SPIN_HALF.  Operators n, sz, splus, sminus (BasisHeisenberg.h:123-139, :230-280).  Semantics, as the
 * reference RUNS:
 *   - splus / sminus flip the bit, value 1, no sign (the operators are not fermionic, doSignSpSm is BasisBase's 1); the spin argument is not read;
 *   - n keeps the index, value = bit for LPP_SPIN_UP and 1 - bit for LPP_SPIN_DOWN (a value of 0 leaves the destination untouched);
 *   - a RAW application of sz (lpp_engine_apply_operator_heis, and so the modified state of lpp_engine_spectral_decomposition_heis, which is what `-g sz`
 *     decomposes) has the value 1 - 2 bit = -2 S^z (getBraIndex_ :273-276): the spectral weights of `-g sz` are 4 times those of S^z;
 *   - lpp_engine_two_point_heis builds sz as n_up/2 - n_down/2 = bit - 1/2, the true S^z (Engine.h:568-587);
 *   - c / cdagger -> LPP_ERR_INVALID from every call (hasNewParts and getBraIndex_ throw);
 *   - S+ on szPlusConst = nsites and S- on szPlusConst = 0 -> LPP_ERR_INVALID from every call, not "no sector": the reference throws (Heisenberg.h:239);
 *   - n and sz stay in the sector (needsNewBasis() is false), so lpp_engine_spectral_decomposition_heis accepts them, unlike the two families above: `sector`
 *     then holds the model's own sector and may be `e` itself (a decomposition does not touch the resident states); the transpose-conjugate of sz is sz,
 *     all four types apply, a diagonal pair keeps types 0 and 1 and accumulates the state twice; s2 *= s (:483) since the operator is not fermionic.
 * Spins above 1/2 have no observables in the reference (BasisHeisenberg.h:130, Heisenberg.h:223 throw): these calls describe one bit per site, and resident
 * states of any other length are refused with LPP_ERR_INVALID.  nsites <= 62; a sector with more than 2^22 runs of equal high part (see the kernel header)
 * -> LPP_ERR_INVALID.  A partitioned engine is refused (LPP_ERR_STATE), and so is a hole-major t-J engine, which cannot hold a state of this basis.
 * The plan cache drops its entries past 1 GiB of run tables (24 MB each at 32 sites).  lpp_engine_keep_states is used as it is: the chain form and the general layout
 * both deliver basis-order vectors.  Every entry point above keeps its behaviour, refusals included. */

/* Heisenberg::hasNewParts (Heisenberg.h:116-134, :218-240), host only: sz -> *has = 0; splus / sminus -> *has = 1 and (szPlusConst +- 1, 0), or LPP_ERR_INVALID
 * at the two throwing ends; every other operator: the reference throws -> LPP_ERR_INVALID. */
lpp_status lpp_obs_new_parts_heis(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* The plan of one operator application, expanded (host only; exposed for the CPU test-suite): action[dst] = +-(src + 1), or 0 where the reference does not
 * touch destination dst; *n_dst entries.  Expanded through the same run table and the same lookup function (obs_heis_source) the kernel uses.  *low_bits:
 * the cut of the word in use -- a site below it gathers inside the runs of equal high part, a site at or above it maps run onto run.  action == NULL: sizes
 * only.  *has is 1 whenever the call succeeds (this model has no "no sector"). */
lpp_status lpp_obs_plan_heis(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new,
                             int64_t* n_dst, int32_t* low_bits, int64_t* action);

/* lpp_engine_apply_operator / _host / lpp_engine_bench_operator in the Heisenberg basis: arguments and contracts as those calls (basis-order vectors, 16-byte
 * aligned destination, one launch on the engine's stream, no sync; the same byte model).  The engine needs no matrix. */
lpp_status lpp_engine_apply_operator_heis(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                          double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_heis_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, double factor_re,
                                               double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_bench_operator_heis(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                          double* ms_per_launch, double* model_bytes);

/* lpp_engine_two_point / lpp_engine_spectral_decomposition in the Heisenberg basis, arguments as those calls; one body serves every family. */
lpp_status lpp_engine_two_point_heis(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state,
                                     int32_t ket_state, void* result, void* trace);
lpp_status lpp_engine_spectral_decomposition_heis(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin, double isign,
                                                  int32_t nsites, int32_t nup, int32_t ndown, double* weight, int32_t* nsteps, double* a, double* b, lpp_stats* stats);

/* ---- reduced density matrix of the lattice cut at a site (ABI 7; one GPU; csrc/lpp_rdm.hip) ----
 * The reference's `-r siteForSplit` (ReducedDensityMatrix.h, LanczosDriver1.h:201-206): part A = sites 0 .. split-1 = the low `split` bits of a species'
 * word, rdm(alpha, alpha') = sum over the environment of conj(psi(alpha, beta)) psi(alpha', beta) -- the conjugate on the ROW index, as the
 * reference has it (:73).  alpha = lo_up + lo_down * 2^split (unpackHubbard :104-123; one species: unpackHeisenberg :90-102).  The matrix is block
 * diagonal in the particle numbers (k_up, k_down) of part A; the engine computes and returns the blocks, packed.  Bases: BasisHubbardLanczos
 * and the S = 1/2 words of BasisHeisenberg, the two the reference supports (:78-88); higher spins are refused in the callers (the reference's masks
 * are not meaningful for several bits per site). */
enum { LPP_BASIS_HUBBARD = 0, LPP_BASIS_SPIN_HALF = 1 }; /* SPIN_HALF: nup = number of set bits, ndown is ignored */

typedef struct lpp_rdm_block {
	int32_t k_up, k_down; /* particles of each species in part A */
	int64_t dim_up, dim_down; /* C(split, k): the block has dim_up * dim_down rows, row = a_up + a_down * dim_up (ranks of the low words) */
	int64_t env_up, env_down; /* environment configurations per species: the sum runs over env_up * env_down terms */
	int64_t offset; /* first element of the block in the packed result (row-major d x d) */
} lpp_rdm_block;

/* The plan (host only; exposed for the CPU test-suite).  Blocks in ascending (k_down, k_up), empty classes left out.  NULL pointers: sizes only.
 * *nblocks, *total = packed elements (sum of d^2), *nrows = sum of d, *nstarts_up / *nstarts_down = entries of the run-start tables;
 * blocks[*nblocks]; alpha[*nrows]: the alpha word of every row of every block, in packed row order; starts_up / starts_down: per class k ascending,
 * then per environment word t ascending (C(nsites - split, n - k) entries per class), the rank of the first state of the run that shares t
 * (ranks as BasisOneSpin::perfectIndex; the run has C(split, k) states ordered by their low word).  split = 0 (one 1 x 1 block, the norm) and
 * split = nsites (one block, one term) are valid; split < 0, split > nsites or an impossible sector -> LPP_ERR_INVALID. */
lpp_status lpp_rdm_plan(int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, int32_t* nblocks, int64_t* total, int64_t* nrows, int64_t* nstarts_up,
                        int64_t* nstarts_down, lpp_rdm_block* blocks, int64_t* alpha, int64_t* starts_up, int64_t* starts_down);

/* The packed blocks of the reduced density matrix of a device vector: d_psi holds C(nsites,nup)*C(nsites,ndown) elements of the engine's dtype in
 * the basis order on the engine's GPU, d_out receives *total elements; both 16-byte aligned.  Launches on the engine's stream, no host sync; the
 * engine needs no matrix.  A gather-SYRK on the f64 MFMA (csrc/lpp_rdm_kernels.h): one triangle of 64 x 64 tiles is computed and mirrored, so
 * the result is Hermitian bit for bit; long sums of small blocks are cut into fixed K ranges and added in a fixed order (no atomics): two calls
 * on the same vector return the same bits.  The plan, its tables and the split-K workspace stay with the engine until another cut is asked for.
 * A workspace that does not fit in the free device memory -> LPP_ERR_NOMEM before any launch; a partitioned or hole-major t-J engine -> LPP_ERR_STATE. */
lpp_status lpp_engine_reduced_density_matrix(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, const void* d_psi, void* d_out);
/* the same on host buffers (copied in and out).  The packed result plus workspace must fit in the free device memory: LPP_ERR_NOMEM with the sizes
 * in the message otherwise, before any launch.  out == NULL: every check is made and nothing is launched (psi is not read). */
lpp_status lpp_engine_reduced_density_matrix_host(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, const void* psi, void* out);
/* the same for resident state `state` (lpp_engine_keep_states before the solve): a missing state -> LPP_ERR_STATE, a sector that is not the
 * resident states' -> LPP_ERR_INVALID.  out_host == NULL: checks only. */
lpp_status lpp_engine_state_reduced_density_matrix(lpp_engine* e, int32_t state, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, void* out_host);
/* Time `iters` calls on a resident pseudo-random vector with HIP events.  *macs = sum over blocks of d^2 * K real multiply-adds (times 4 for c128):
 * BOTH triangles are counted, as a full product would compute them, although the kernel computes one and mirrors it. */
lpp_status lpp_engine_bench_rdm(lpp_engine* e, int32_t basis, int32_t nsites, int32_t nup, int32_t ndown, int32_t split, int32_t warmup, int32_t iters, double* ms_per_call,
                                double* macs);

/* ---- products of one-site operators: many-point correlations and measure brackets (entry points added under ABI 7, no struct changes; one GPU;
 *      Hubbard product basis; csrc/lpp_obs.hip, csrc/lpp_obs_string_kernels.h) ----
 * The reference's -M "op?site?spin;..." (Engine::manyPoint, Engine.h:341-389) and -m "<gs|op;op;...|gs>" (Engine::measure :208-249 through
 * ModelBase::rahulMethod, ModelBase.h:89-141, RahulOperator.h).  A string of 1 .. 16 operators is composed ON THE HOST into one pair of per-species
 * tables in the format of lpp_obs_plan, so <bra| string |ket> is one pass that reads bra and ket once and writes no vector.
 * LPP_STRING_MANY_POINT: ops[] are LPP_OP_* with site and spin; ops[0] acts first on the ket; each step is accModifiedState_ with factor 1 (bra index
 *   and value of getBraIndex, doSignGf for c / cdagger -- the down species drops the up parity for site > 0 --, doSignSpSm for splus / sminus, sz with
 *   value +1 / -1 / absent); the sector walks by hasNewParts (lpp_obs_new_parts) step by step, the (0,0) refusal included: no sector -> *has = 0.
 *   DEVIATION: n and sz act in the CURRENT sector.  The reference's getNeededBasis (:397-400) hands them the basis of the ORIGINAL sector even after
 *   earlier operators have left it and ranks words of another particle number in it (a wrong index or a throw).  Strings whose n / sz occur only
 *   while the sector is the original one are reference-exact.
 * LPP_STRING_MEASURE: ops[] are LPP_OP_C (flags[] bit 0: transpose = c-dagger), LPP_OP_N, LPP_OP_SZ, LPP_OP_IDENTITY; spins[] is the dof (0 up, 1 down);
 *   ops[nops-1] acts first; n keeps occupied bits; sz is -1/2 on an occupied and +1/2 on an empty bit of that species (RahulOperator.h:38-40 as
 *   written); c flips the bit, sign ProgramGlobals::doSign(word after the flip, site) times (-1)^(up electrons) for dof = down.  The result lives in the
 *   original sector: a string that does not conserve both numbers -> LPP_ERR_INVALID.
 * An engine holding a hole-major t-J model -> LPP_ERR_INVALID naming the model; the Python layer and the C++ shim, which know the model of every
 * engine they set up, refuse t-J engines the same way and take Heisenberg engines (twiceS = 1) to the _heis entry points of the next block: the C++ shim
 * by the model, the Python layer where the caller passes basis="spin_half" (without it a Heisenberg engine is refused by the model's name, with that
 * hint).  A partitioned engine -> LPP_ERR_STATE. */
enum { LPP_OP_IDENTITY = 0 };
enum { LPP_STRING_MANY_POINT = 0, LPP_STRING_MEASURE = 1 };

/* The plan of one string (host only; exposed for the CPU test-suite): *has, the final parts, *scale (the product of the 1/2 magnitudes of measure's
 * sz), the two composed tables -- table[destination species rank] = +-(source species rank + 1), 0 = none, every sign carried by the entries --
 * and, for many-point, the sz entries: sz[3k .. 3k+2] = (site, flip_up, flip_down), factor (bit_up(src, site) ^ flip_up) - (bit_down(src, site) ^ flip_down)
 * on the SOURCE words, a destination with a zero factor is not reached.  table_up[*n_up_dst], table_down[*n_down_dst], sz[3 * 16]; NULL: not written. */
lpp_status lpp_obs_string_plan(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                               int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new, double* scale, int64_t* n_up_dst, int64_t* n_down_dst,
                               int32_t* table_up, int32_t* table_down, int32_t* nsz, int32_t* sz);

/* z (+)= factor * string src on device vectors of the engine's GPU and dtype in the basis order, contracts of lpp_engine_apply_operator (16-byte aligned
 * destination; accumulate = 0 writes 0 where the string does not reach).  One launch of k_obs_string_apply, then a stream sync (the tables are the
 * call's own).  *has = 0: no such sector, nothing was done; otherwise the final parts.  _host: host vectors, copied in and out. */
lpp_status lpp_engine_apply_string(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                   int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate,
                                   int32_t* has, int32_t* nup_new, int32_t* ndown_new);
lpp_status lpp_engine_apply_string_host(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                        int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate,
                                        int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* result[2 s], result[2 s + 1] = re, im of conj(bra) . (string_s ket) for resident states of sector (nup, ndown); string s is entries offsets[s] ..
 * offsets[s+1] - 1 of ops / sites / spins / flags (flags may be NULL).  A string that leads to no sector or ends in another sector gives 0 and launches
 * nothing (Engine.h:364, :382-383).  The others go 8 per launch through k_obs_string_dot (bra read once for the 8) and a fixed-order reduction: a
 * value does not depend on the batch it is computed in, and two calls return the same bits.  _host: bra and ket are host vectors of the sector. */
lpp_status lpp_engine_many_point(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                 const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, double* result);
lpp_status lpp_engine_many_point_host(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                      const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, const void* bra, const void* ket, double* result);
/* Time `iters` launches (bracket kernel + reduction) of ONE batch of 1 .. 8 strings on zeroed vectors with HIP events;
 * model_bytes = sizeof(value) * (N + sum over the strings of the destinations they reach): bra once, one ket element per string and destination. */
lpp_status lpp_engine_bench_string_dot(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                       const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes);

/* ---- many-point correlations of the S = 1/2 Heisenberg basis (entry points added under ABI 7, no struct changes; one GPU; csrc/lpp_obs.hip,
 *      csrc/lpp_obs_heis_string_plan.h, csrc/lpp_obs_heis_string_kernels.h) ----
 * The reference's -M for Model=Heisenberg with HeisenbergTwiceS=1: Engine::manyPoint chains accModifiedState_ with factor 1, which
 * BasisHeisenberg::getBraIndex serves for n, sz, splus and sminus (BasisHeisenberg.h:123-139, :230-280).  Argument lists as the calls above; nup =
 * szPlusConst, ndown and flags are not read, the final sector is reported as (szPlusConst', 0).  LPP_STRING_MANY_POINT only: the measure convention's
 * labels are per fermion species -> LPP_ERR_INVALID.  ops[0] acts first:
 *   splus / sminus flip the site's bit where it is clear / set, value 1, the spin is not read; n keeps the index with value bit (LPP_SPIN_UP) or
 *   1 - bit (LPP_SPIN_DOWN); sz keeps it with the reference's raw value 1 - 2 bit = -2 S^z; there is no sign anywhere.  The sector walks by
 *   hasNewPartsSplusOrMinus, szPlusConst +- 1.
 * A whole string composes on the host into five words and no table: result[d] = sign * (-1)^popcount((d ^ flip) & zmask) * src[rank(d ^ flip)] where
 * ((d ^ flip) & need) == want, else 0 -- the conditions and the sz parity are on the SOURCE word.  A string whose conditions contradict each other
 * (splus twice on a site, n up and n down of a site) is identically zero: "dead".
 * LPP_ERR_INVALID, as lpp_engine_apply_operator_heis has it: c / cdagger in a string, S+ met in the all-up sector, S- met in the all-down one (refused at
 * the step that meets it), a site >= nsites, 0 or more than 16 operators.  Engines of spins above 1/2 are refused by the callers that know the model.
 * DEVIATIONS, both where the reference is ill-defined: (1) n and sz act in the sector the string has reached; the reference's getNeededBasis
 * (Engine.h:397-400) hands them the original sector's basis even after the string has left it.  (2) S- is refused when the CURRENT sector is the all-down
 * one; the reference tests the original sector's szPlusConst (Heisenberg.h:233) and otherwise wraps an unsigned number.
 * A partitioned engine -> LPP_ERR_STATE; a hole-major t-J engine -> LPP_ERR_INVALID.  The entry points of the block above keep their behaviour; the Python
 * layer and the C++ shim choose between the two blocks by the engine's model (Python: the explicit basis="spin_half"). */

/* The plan of one string (host only; exposed for the CPU test-suite): the final szPlusConst, *dead, the five words, *low_bits (the cut of the word,
 * lpp_obs_plan_heis) and, where action is not NULL, action[dst] = +-(src + 1) or 0 for the *n_dst destinations, expanded through the per-run entries
 * and the same lookup function (obs_heis_string_source) the kernels use.  All zero for a dead string.  NULL: not written. */
lpp_status lpp_obs_string_plan_heis(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                                    int32_t nup, int32_t ndown, int32_t* nup_new, int32_t* dead, uint64_t* flip, uint64_t* need, uint64_t* want, uint64_t* zmask, int32_t* sign,
                                    int32_t* low_bits, int64_t* n_dst, int64_t* action);

/* lpp_engine_apply_string / _host in the Heisenberg basis, contracts as those calls: one launch of k_obs_string_apply_heis, then a stream sync.  *has = 1
 * whenever the call succeeds (this basis has no "no sector"); a dead string launches nothing and gives z = 0 (accumulate: z unchanged). */
lpp_status lpp_engine_apply_string_heis(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                        int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate,
                                        int32_t* has, int32_t* nup_new, int32_t* ndown_new);
lpp_status lpp_engine_apply_string_heis_host(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                             const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* src, void* dst,
                                             int32_t accumulate, int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* lpp_engine_many_point / _host / lpp_engine_bench_string_dot in the Heisenberg basis, contracts as those calls: a dead string and one that ends in another
 * sector give exactly 0 and launch nothing (Engine.h:382-383); the others go 8 per launch through k_obs_string_dot_heis and a fixed-order reduction, so
 * a value does not depend on the batch it is computed in, and two calls return the same bits. */
lpp_status lpp_engine_many_point_heis(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                      const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, double* result);
lpp_status lpp_engine_many_point_heis_host(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                           const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, const void* bra, const void* ket, double* result);
lpp_status lpp_engine_bench_string_dot_heis(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                            const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                            double* ms_per_launch, double* model_bytes);

/* ---- many-point correlations of the one-orbital t-J basis (entry points added under ABI 7, no struct changes; one GPU; csrc/lpp_obs.hip,
 *      csrc/lpp_obs_tj_string_plan.h, csrc/lpp_obs_tj_string_kernels.h) ----
 * The reference's -M for Model=TjMultiOrb with Orbitals=1: Engine::manyPoint chains accModifiedState_ with factor 1 through the sectors of
 * TjMultiOrb::hasNewParts (no (0,0) sector, none with nup + ndown > sites), served by BasisTjMultiOrbLanczos::getBraIndex (:207-245).  Argument lists as
 * the Hubbard calls; flags are not read.  LPP_STRING_MANY_POINT only: RahulOperator on this basis is not restated -> LPP_ERR_INVALID.  ops[0] acts first,
 * with the rules of lpp_engine_apply_operator_tj: c / cdagger flip the species' own bit (cdagger needs the other species absent) with doSignGf -- spin
 * UP: the parity of the up bits below the site; spin DOWN: the parity of ALL up electrons times the parity of the down bits below the site --, n and a
 * raw sz are both "the bit of the given spin is set" with value 1, splus makes a down site up and sminus an up site down with value 1 and no sign.
 * A site is empty, up or down, and every operator fixes the state it meets and the state it leaves, so a whole string composes on the host into
 *   result[(u, d)] = sign * (-1)^popcount(us & par_up) * (-1)^popcount(ds & par_down) * src[index(us, ds)],  us = u ^ flip_up, ds = d ^ flip_down,
 *   where (us & touched) == want_up and (ds & touched) == want_down, else 0
 * (the conditions and the parities are on the SOURCE words; both species are recorded for every touched site, so the source is always a basis word).
 * A step that meets another state than the steps before left (c twice, n up and n down of one site) makes the string identically zero: "dead".
 * LPP_ERR_INVALID, as lpp_engine_apply_operator_tj has it: an unknown operator or spin, a site >= nsites, a bad sector (nup + ndown <= nsites <= 30),
 * splus / sminus with LPP_SPIN_DOWN, 0 or more than 16 operators, and a string that changes the up pattern with more than 24 sites free of down
 * electrons in its source sector (the pattern rank tables are kept in LDS).  n and sz act in the sector the string has reached (the deviation of the
 * other two families from Engine.h:397-400).  A partitioned engine -> LPP_ERR_STATE; a hole-major t-J engine is served (its resident states are in the
 * basis order, lpp_engine_keep_states_tj).  The entry points of the two blocks above keep their behaviour; the Python layer asks for basis="tj", the
 * C++ shim for the SolverOptions token TjOperatorStrings. */

/* The plan of one string (host only; exposed for the CPU test-suite): *has = 0 where a step leads to no sector; else the final parts, *dead,
 * words[7] = { flip_up, flip_down, touched, want_up, want_down, par_up, par_down }, *sign, *n_dst, *touched_count = the destinations the string
 * reaches in closed form (the byte model's count) and, where action is not NULL, action[dst] = +-(src + 1) or 0 for the *n_dst destinations, expanded
 * through the per-down-word entries and the same lookup function (obs_tj_string_source) the kernels use.  All zero for a dead string.  NULL: not written. */
lpp_status lpp_obs_string_plan_tj(int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags, int32_t nsites,
                                  int32_t nup, int32_t ndown, int32_t* has, int32_t* nup_new, int32_t* ndown_new, int32_t* dead, uint32_t* words, int32_t* sign, int64_t* n_dst,
                                  int64_t* touched_count, int64_t* action);

/* lpp_engine_apply_string / _host in the t-J basis, contracts as those calls: one launch of k_obs_string_apply_tj, then a stream sync.  *has = 0 where
 * the string leads to no sector; a dead string launches nothing and gives z = 0 (accumulate: z unchanged). */
lpp_status lpp_engine_apply_string_tj(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins, const int32_t* flags,
                                      int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate,
                                      int32_t* has, int32_t* nup_new, int32_t* ndown_new);
lpp_status lpp_engine_apply_string_tj_host(lpp_engine* e, int32_t convention, int32_t nops, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                           const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, double factor_re, double factor_im, const void* src, void* dst,
                                           int32_t accumulate, int32_t* has, int32_t* nup_new, int32_t* ndown_new);

/* lpp_engine_many_point / _host / lpp_engine_bench_string_dot in the t-J basis, contracts as those calls: a dead string, one without a sector and one
 * that ends in another sector give exactly 0 and launch nothing (Engine.h:364, :382-383); the others go 8 per launch through k_obs_string_dot_tj and a
 * fixed-order reduction, so a value does not depend on the batch it is computed in, and two calls return the same bits. */
lpp_status lpp_engine_many_point_tj(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites, const int32_t* spins,
                                    const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t bra_state, int32_t ket_state, double* result);
lpp_status lpp_engine_many_point_tj_host(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                         const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, const void* bra, const void* ket, double* result);
lpp_status lpp_engine_bench_string_dot_tj(lpp_engine* e, int32_t convention, int32_t nstrings, const int64_t* offsets, const int32_t* ops, const int32_t* sites,
                                          const int32_t* spins, const int32_t* flags, int32_t nsites, int32_t nup, int32_t ndown, int32_t warmup, int32_t iters,
                                          double* ms_per_launch, double* model_bytes);

/* ---- site-weighted operator sums (entry points added under ABI 7, no struct changes; one GPU; csrc/lpp_obs.hip, csrc/lpp_obs_sum_kernels.h) ----
 *     |phi> = sum_r f_r A_r |src>,   nweights = nsites complex weights f_r = w_re[r] + i w_im[r] (w_im may be NULL: real weights),
 * the modified state of the momentum-resolved quantities: A(k,w) from c_k = sum_r e^{ikr} c_r, N(q,w), S^zz(q,w), S(q,w).  This is the project's own
 * definition (the reference's dynamics1.cpp accumulates such a sum but its phase does not depend on the site).  A_r is what Engine::accModifiedState applies
 * (Engine.h:535-599): c, cdagger, n of the given spin, splus, sminus as lpp_engine_apply_operator; sz = n_up/2 - n_down/2 in the Hubbard and t-J bases; the
 * Heisenberg basis applies its raw sz (1 - 2 bit), as lpp_engine_spectral_decomposition_heis does.  Hubbard c, cdagger, n, sz go through ONE launch
 * (k_obs_sum_move_up / _down, k_obs_sum_diag: destination driven, the terms of a destination added in ascending site from 0, so a value does not depend on the
 * grid and two calls return the same bits), and so does the Heisenberg sz (k_obs_sum_sz_heis); everything else -- the t-J basis, splus / sminus, the Heisenberg n --
 * and everything under LPP_OBS_SUM_CHAIN=1 (read
 * when the engine first plans an operator; for tests and the benchmark) chains the one-site launches over the sites with a non-zero weight.  A complex weight
 * on an f64 engine, nweights != nsites, nsites > 30 -> LPP_ERR_INVALID; engines and operators are refused where the one-site calls refuse them.  Nothing is
 * launched by a refused call. */

/* The fused plan of sum_r f_r A_r in the Hubbard product basis (host only; exposed for the CPU test-suite): *width terms per destination, W = nsites - n or n
 * for c / cdagger (n = the moved species' destination count), 1 for n / sz.  With the four tables (n_dst * width entries each, all or none) the plan is
 * expanded in the kernel's order: term t of destination d reads source src_index[d * width + t] with factor (fac_re, fac_im) = sign * f_site (for n / sz the
 * source is d itself, site = -1 and the factor is the element's whole coefficient under the given weights).  splus / sminus -> LPP_ERR_INVALID: no fused plan.
 * *has = 0: hasNewParts refused, nothing else is written. */
lpp_status lpp_obs_sum_plan(int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, const double* w_re, const double* w_im, int32_t* has, int32_t* nup_new,
                            int32_t* ndown_new, int64_t* n_dst, int32_t* width, int64_t* src_index, int32_t* site, double* fac_re, double* fac_im);

/* z (+)= sum_r f_r A_r src on device vectors (contracts as lpp_engine_apply_operator: basis order, 16-byte aligned destination, the engine's stream, no sync). */
lpp_status lpp_engine_apply_operator_sum(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                         const double* w_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_sum_tj(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                            const double* w_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_sum_heis(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                              const double* w_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
/* the same on host vectors; *n_dst (may be NULL) = the destination's length; src == dst == NULL: *has and *n_dst only */
lpp_status lpp_engine_apply_operator_sum_host(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                              const double* w_im, const void* src, void* dst, int32_t accumulate, int32_t* has, int64_t* n_dst);
lpp_status lpp_engine_apply_operator_sum_tj_host(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                                 const double* w_im, const void* src, void* dst, int32_t accumulate, int32_t* has, int64_t* n_dst);
lpp_status lpp_engine_apply_operator_sum_heis_host(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights,
                                                   const double* w_re, const double* w_im, const void* src, void* dst, int32_t accumulate, int32_t* has, int64_t* n_dst);
/* Time `iters` sums on zeroed vectors with HIP events; model_bytes = sizeof(value) * (N_dst written, once more when accumulating, + N_src: every source
 * element touched once) -- the same model for the fused launch and for the chain, which moves about three destination passes per site instead. */
lpp_status lpp_engine_bench_operator_sum(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                         const double* w_im, int32_t accumulate, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes);
lpp_status lpp_engine_bench_operator_sum_tj(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                            const double* w_im, int32_t accumulate, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes);
lpp_status lpp_engine_bench_operator_sum_heis(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                              const double* w_im, int32_t accumulate, int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes);
/* *norm2 = <phi|phi> for resident state `state` of sector (nup, ndown): the static structure factor; no sector engine.  *has = 0: no such sector, *norm2 = 0. */
lpp_status lpp_engine_sum_norm2(lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                const double* w_im, double* norm2, int32_t* has);
lpp_status lpp_engine_sum_norm2_tj(lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                   const double* w_im, double* norm2, int32_t* has);
lpp_status lpp_engine_sum_norm2_heis(lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown, int32_t nweights, const double* w_re,
                                     const double* w_im, double* norm2, int32_t* has);
/* lpp_engine_spectral_decomposition with |phi> as the modified state (built once: no doubling), *weight = <phi|phi>.  An operator that stays in the sector
 * (n, sz) takes a sector engine of the SAME sector. */
lpp_status lpp_engine_spectral_decomposition_sum(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                                                 int32_t nweights, const double* w_re, const double* w_im, double* weight, int32_t* nsteps, double* a, double* b,
                                                 lpp_stats* stats);
lpp_status lpp_engine_spectral_decomposition_sum_tj(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t nup, int32_t ndown,
                                                    int32_t nweights, const double* w_re, const double* w_im, double* weight, int32_t* nsteps, double* a, double* b,
                                                    lpp_stats* stats);
lpp_status lpp_engine_spectral_decomposition_sum_heis(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t nup,
                                                      int32_t ndown, int32_t nweights, const double* w_re, const double* w_im, double* weight, int32_t* nsteps, double* a,
                                                      double* b, lpp_stats* stats);

/* ---- observables of the spin-S Heisenberg digit basis (opt-in, added under ABI 7 with no struct change) ----
 * BasisHeisenberg (reference BasisHeisenberg.h:24-47) for any twiceS lpp_engine_assemble_heisenberg_spin admits: L digits of `bits` bits, site p at bit
 * offset p * bits, digit d = m + S in [0, twiceS], the words of digit sum szPlusConst ascending.  The reference THROWS for spins above 1/2
 * (BasisHeisenberg.h:130,263, Heisenberg.h:223), so the operators are the project's own definition, with m = d - S of the SOURCE state:
 *   - splus: digit d -> d + 1, value sqrt(S(S+1) - m(m+1)), nothing leaves d = twiceS; sminus: digit d -> d - 1, value sqrt(S(S+1) - m(m-1)), nothing
 *     leaves d = 0; sz: index kept, value m -- the TRUE S^z in every call of this family (there is no raw -2 S^z form), a value of 0 leaves the
 *     destination untouched;
 *   - n, c, cdagger: LPP_ERR_INVALID; the spin arguments are checked to be 0 or 1 and otherwise not read;
 *   - S+ on the top sector (szPlusConst = nsites * twiceS) and S- on szPlusConst = 0 are LPP_ERR_INVALID, not "no sector"; a new sector is reported as
 *     (szPlusConst +- 1, 0); whatever the assembler refuses (odd twiceS with twiceS + 1 no power of two, bits * nsites > 62) is LPP_ERR_INVALID here,
 *     and so is twiceS > 4095.
 * Every call takes (nsites, twiceS, szPlusConst) where the families above take (nsites, nup, ndown); twiceS = 1 is accepted (splus / sminus then
 * equal the _heis calls bit for bit, sz is -1/2 times their raw one).  Otherwise the contracts are those of the _heis calls of the same name:
 * two_point gives result[i][j] = <A_j bra | A_i ket> (<S^z_j S^z_i>, <S^-_j S^+_i>) and the trace; spectral_decomposition builds
 * A_i |state> + isign A_j |state> (a diagonal pair is accumulated twice), sz decomposes in the state's own sector on a sector engine of that sector.
 * Resident states whose length is not the sector's size are refused.  The operator sums always chain the one-site launches (no fused kernel).
 * Operator strings, the reduced density matrix and partitioned engines stay refused for these spins.
 * lpp_obs_plan_heis_spin (host only): *n_dst, *low_digits = the cut lb (a site below it gathers inside the runs of equal high part, a site at or
 * above it maps run onto run), and where not NULL action[dst] = src + 1 or 0 and coef[dst] = the value (0 where untouched), expanded through the
 * run table and the lookup function the kernel uses. */
lpp_status lpp_obs_new_parts_heis_spin(int32_t op, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t* has, int32_t* szPlusConst_new,
                                       int32_t* zero);
lpp_status lpp_obs_plan_heis_spin(int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t* has, int32_t* szPlusConst_new,
                                  int64_t* n_dst, int32_t* low_digits, int64_t* action, double* coef);
lpp_status lpp_engine_apply_operator_heis_spin(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst,
                                               double factor_re, double factor_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_heis_spin_host(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst,
                                                    double factor_re, double factor_im, const void* src, void* dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_bench_operator_heis_spin(lpp_engine* e, int32_t op, int32_t site, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst,
                                               int32_t warmup, int32_t iters, double* ms_per_launch, double* model_bytes);
lpp_status lpp_engine_two_point_heis_spin(lpp_engine* e, int32_t op, int32_t spin1, int32_t spin2, int32_t nsites, int32_t twiceS, int32_t szPlusConst,
                                          int32_t bra_state, int32_t ket_state, void* result, void* trace);
lpp_status lpp_engine_spectral_decomposition_heis_spin(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t isite, int32_t jsite, int32_t spin,
                                                       double isign, int32_t nsites, int32_t twiceS, int32_t szPlusConst, double* weight, int32_t* nsteps, double* a,
                                                       double* b, lpp_stats* stats);
lpp_status lpp_engine_apply_operator_sum_heis_spin(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t nweights,
                                                   const double* w_re, const double* w_im, const void* d_src, void* d_dst, int32_t accumulate, int32_t* has);
lpp_status lpp_engine_apply_operator_sum_heis_spin_host(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t nweights,
                                                        const double* w_re, const double* w_im, const void* src, void* dst, int32_t accumulate, int32_t* has,
                                                        int64_t* n_dst);
lpp_status lpp_engine_bench_operator_sum_heis_spin(lpp_engine* e, int32_t op, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t nweights,
                                                   const double* w_re, const double* w_im, int32_t accumulate, int32_t warmup, int32_t iters, double* ms_per_launch,
                                                   double* model_bytes);
lpp_status lpp_engine_sum_norm2_heis_spin(lpp_engine* e, int32_t state, int32_t op, int32_t spin, int32_t nsites, int32_t twiceS, int32_t szPlusConst, int32_t nweights,
                                          const double* w_re, const double* w_im, double* norm2, int32_t* has);
lpp_status lpp_engine_spectral_decomposition_sum_heis_spin(lpp_engine* e, int32_t state, lpp_engine* sector, int32_t op, int32_t spin, int32_t nsites, int32_t twiceS,
                                                           int32_t szPlusConst, int32_t nweights, const double* w_re, const double* w_im, double* weight,
                                                           int32_t* nsteps, double* a, double* b, lpp_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* LPP_ENGINE_H */
