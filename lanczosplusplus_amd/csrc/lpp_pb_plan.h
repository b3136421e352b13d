// lpp_pb_plan.h -- planning of the product-basis layout  H = 1 (x) T + C (x) 1 + D  (lpp_pb_kernels.h) in plain C++: from T and C as host
// CSRs, the LPP_PB_* switches as values and the number of CUs to everything pb_build (lpp_pb.hip) uploads and every scalar the launches
// read.  No HIP, no environment: lanczosplusplus_amd/host/test_pb_plan.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <stdint.h>
#include <vector>

#include "lpp_host.h"
#include "lpp_switch.h"

namespace lpp {

// complex hoppings (PbState::cplx): pb_build then gets the REALIFIED in-block matrix (2 n_c rows) as t_rp / t_ci / t_va and the couplings'
// structure as c_rp / c_ci (c_va unused); the complex matrices themselves come through this
struct PbCplxInput {
	int64_t n_c; // complex positions per block
	const int64_t* t_rp; // the complex in-block matrix, n_c rows, values as (re, im) pairs
	const int32_t* t_ci;
	const double* t_va;
	const double* c_va; // complex coupling values, (re, im) pairs, aligned with c_ci
};
// What pb_build is given: T and C as host CSRs over one species each (diagonal entries are ignored), sorted 256-entry dictionary holding
// every coupling value; the caller fills pb.dcode (n_blk*pitch codes) afterwards.  Whatever a caller does not set keeps its default.
struct PbBuildInput {
	int64_t n_up = 0, n_blk = 0; // positions per block, blocks
	const int64_t *t_rp = nullptr, *c_rp = nullptr; // the in-block CSR T (null with `pre`) and the coupling CSR C
	const int32_t *t_ci = nullptr, *c_ci = nullptr;
	const double *t_va = nullptr, *c_va = nullptr;
	const double* dict256 = nullptr;
	int ndict = 0;
	// several GPUs (transposition exchange): the rank's block range, the row length of its transposed slice, the blocks of that slice
	int64_t blk0 = 0, nblk_loc = -1, pitch_dn = 0, nblk_padded = 0;
	const PbCplxInput* cx = nullptr; // complex hoppings
	struct SegPlan* pre = nullptr; // a ready-made plan of the segmented form (pb_chain; moved from) standing for pre_nnz entries
	int64_t pre_nnz = 0;
};

struct PbSwitches { // LPP_PB_<NAME> (EnvSwitch, lpp_switch.h), in the order pb_plan consults them
	EnvSwitch big2, big2_four, piece_rows, parts, wide, bank_ways, perm, seg, pre0, down_rounds, order_window, down_image, pace, chain, down_tasks, down_pf,
	    chain_pace, lazy_tx, down_grid;
	bool verbose = false; // LPP_VERBOSE
};
PbSwitches pb_switches_from_env(); // the only getenv of the product-basis build (lpp_pb_plan.cpp)

// The scalar, host-only part of PbState (lpp_engine_impl.h derives from it): the planner fills it, pb_build assigns it in one statement,
// the launches read it under the names they always had.
struct PbForm {
	int64_t n_up = 0, n_blk = 0, pitch = 0;
	int64_t nnz = 0; // entries of the CSR this stands for
	// in-block matrix T (off-diagonal part)
	int G = 0;
	double gval[kPbMaxGroups] = { 0 };
	int spb = 0;
	int64_t tw_words = 0, t_entries = 0, t_slots = 0;
	int pre0 = 4; // chained step, two value groups: chunks of group 0 requested one slice ahead (group 1: 8 - pre0)
	// block couplings C (off-diagonal)
	int64_t c_nnz = 0;
	int rowcap = 0, ids_per_wg = 0, down_grid = 0;
	int down_rounds = 1, ids_per_round = 0; // k_pb_down: pieces of a workgroup's block range per panel (one LDS image each)
	size_t down_lds = 0;
	size_t down_lds_pf = 0; // k_pb_down's PF form: the image plus the task sums
	// launch forms, resolved by the planner from the LPP_PB_* launch switches and from what was planned; the launches read only these
	bool chain_ok = false; // the chained scale-free step serves this layout (LPP_PB_CHAIN; pb_chain_ok adds: no plain-stream diagonal)
	bool down_tasks = false; // plain coupling kernel: tasks handed out by the LDS counter, no pacing (LPP_PB_DOWN_TASKS)
	bool down_pf = false; // chained coupling kernel: the counter form with the u lines touched ahead (LPP_PB_DOWN_PF)
	bool chain_drop_pace = false; // ... and without the pacing (LPP_PB_CHAIN_PACE=1 keeps it)
	bool lazy_tx = false; // transposition exchange: the update rides in the next step's pack kernel (LPP_PB_LAZY_TX)
	// several GPUs, transposition exchange (pb_tx_*): this rank holds the in-block part for its own blocks [blk0, blk0 + nblk_loc)
	// (vectors, u and dcode cover those only) and applies the block couplings to the received transposed slice: all n_blk blocks,
	// rows of pitch_dn positions (= the up-index range of this rank, a multiple of 16)
	bool tx = false;
	int64_t blk0 = 0, nblk_loc = 0, pitch_dn = 0;
	int64_t nnz_loc = 0; // entries of the CSR rows this rank holds (== nnz on one GPU)
	// rows beyond one LDS window / vectors beyond 4 GiB (lpp_pbig_kernels.h)
	bool big = false; // in-block part by pieces of W positions (k_pb_up_big)
	bool big2 = false; // ... two blocks per workgroup and template read (k_pb_up_big2)
	int W = 0, npieces = 1;
	int64_t f_words = 0, f_entries = 0; // entries that leave their piece
	// rows beyond one LDS window, segmented form (lpp_pbseg.h, k_pb_up_seg): T decomposed by the high sites of the species' basis word;
	// the stored order of the positions (perm / inv) is then the segments by length
	bool seg = false;
	bool seg_one = false; // one block per workgroup (pb_chain)
	int seg_nitems = 0, seg_nsegs = 0, seg_ws = 0, seg_wmax = 0, seg_nc = 0, seg_nh = 0, seg_pre0 = 4;
	int64_t seg_bytes = 0; // description of T held on the device
	// complex hoppings: the vectors are complex, a block holds 2 n_c real positions (re, im interleaved; n_up, pitch count doubles), T is
	// stored REALIFIED (row 2i: (2c, Re t), (2c+1, -Im t); row 2i+1: (2c, Im t), (2c+1, Re t)) so that k_pb_up is the real kernel, the couplings
	// keep complex values (cdict, k_pb_down<CPLX>), the diagonal code of a position is stored for both of its doubles.  t_ptr / t_col / t_val
	// keep the complex T of n_c rows ((re, im) pairs) for lpp_engine_get_csr.
	bool cplx = false;
	int64_t n_c = 0; // complex positions per block
	bool wide = false; // vector beyond 4 GiB: k_pb_down<WIDE> (64-bit addresses from line numbers)
	bool parts = false; // couplings over parts of the source range (k_pb_down_parts; 64-bit addresses too)
	int nparts = 1, ent_cap = 0, pace_stride = 0, maxr = 0;
	int64_t part_blocks = 0;
	int ndict = 0; // diagonal codes in use
};

// Everything pb_build needs: `form` and the host vectors it uploads (an empty optional vector was not planned)
struct PbPlan {
	PbForm form;
	// in-block part: stored position -> basis index and back (list-length order of the one-window form, or the segments'; empty: basis order)
	std::vector<int32_t> perm, inv;
	bool seg_tried = false; // (LPP_VERBOSE reports the attempt either way)
	SegPlan seg; // form.seg: the segmented description of T; the per-position template is then not built at all
	PbTemplate T; // words / off / len as k_pb_up reads them (chunk pairs in the one-window form), far lists of the pieces form
	// plain off-diagonal copies of T and C (lpp_engine_get_csr walks them; k_pb_down stages C in LDS), coupling codes, dictionaries
	std::vector<int64_t> tp, cp, base; // base: first CSR entry of every block
	std::vector<int32_t> tc, cc;
	std::vector<double> tv, dict, cdict; // cdict: complex hoppings only
	std::vector<uint8_t> ccode;
	std::vector<int32_t> pstart; // parts form: per block and part, where the part's entries start in the list
	std::vector<int32_t> order; // blocks of every workgroup's range by decreasing list length
	int slots = 0; // coupling workgroups per group (each owns ids_per_wg consecutive blocks)
	size_t image_bytes = 0; // prepared LDS images of all (workgroup, round) pairs (k_pb_down_image); 0: none
	size_t pace_counters = 0; // pacing counters; 0: free-running
};

// complex in-block matrix (n rows, (re, im) pairs, diagonal skipped) -> the realified one of 2n rows (PbState::cplx)
void pb_realify(int64_t n, const int64_t* rp, const int32_t* ci, const double* va, std::vector<int64_t>& rrp, std::vector<int32_t>& rci, std::vector<double>& rva);
// the rows of in.t_* by the chunk counts of their lists, and P T P^T with the columns of a row ascending; perm stays empty where T has no
// off-diagonal value or more than kPbMaxGroups (a step of pb_plan, public for the stand-alone test)
void pb_list_length_order(const PbBuildInput& in, std::vector<int32_t>& perm, std::vector<int32_t>& inv, std::vector<int64_t>& p_rp, std::vector<int32_t>& p_ci,
                          std::vector<double>& p_va);
// LPP_ERR_INVALID with a "pb_build: ..." message: the layout does not hold this matrix, the caller keeps the general one
lpp_status pb_plan(const PbBuildInput& in, const PbSwitches& sw, int num_cus, PbPlan& out);
// pb_plan's last step: every kernel instance the launches of this form ask for is in its list (lpp_pb_instances.h); otherwise
// LPP_ERR_INVALID, "pb_build: no kernel instance for ..."
lpp_status pb_check_instances(const PbForm& B);
// the LPP_VERBOSE lines of a plan, to stderr
void pb_plan_print(const PbPlan& P);

} // namespace lpp
