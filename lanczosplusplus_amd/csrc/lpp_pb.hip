// lpp_pb.hip -- host side of the product-basis stored layout (kernels and rationale: lpp_pb_kernels.h): uploads and launches.
// What is built -- the form, every refusal, every host vector and every scalar of PbState a launch reads -- is planned in plain C++
// (lpp_pb_plan.h / .cpp, sizes in lpp_pb_geom.h; the LPP_PB_* switches are read there, once, by pb_switches_from_env); pb_build below
// only carries the plan to the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "lpp_assemble_kernels.h"
#include "lpp_engine_impl.h"
#include "lpp_launch.h"
#include "lpp_pb_instances.h"
#include "lpp_pbig_kernels.h"
#include "lpp_pbseg_kernels.h"

using namespace lpp;

namespace lpp {

void free_pb(lpp_engine* e)
{
	PbState& B = e->pb;
	for (void* p : { (void*)B.tw, (void*)B.tw_off, (void*)B.tw_len, (void*)B.t_ptr, (void*)B.t_col, (void*)B.t_val, (void*)B.c_ptr, (void*)B.c_col,
	                 (void*)B.c_code, (void*)B.order, (void*)B.down_image, (void*)B.pace, (void*)B.z, (void*)B.u, (void*)B.xy, (void*)B.dict, (void*)B.dcode, (void*)B.blockbase,
	                 (void*)B.fw, (void*)B.f_off, (void*)B.f_len, (void*)B.c_pstart, (void*)B.dval, (void*)B.perm, (void*)B.inv, (void*)B.cdict,
	                 B.seg_items, B.seg_segs, B.seg_cross, B.seg_hh, B.seg_slices, (void*)B.seg_tw, (void*)B.seg_xw })
		if (p) (void)hipFree(p);
	B = PbState();
	e->pitch = e->pitch_rows = e->pitch_blocks = 0;
}

namespace {
template <typename V> lpp_status to_device(V** dst, const std::vector<V>& src, hipStream_t st)
{
	HIP_TRY_MEM(hipMalloc(dst, sizeof(V) * std::max<size_t>(src.size(), 1)));
	if (!src.empty()) HIP_TRY(hipMemcpyAsync(*dst, src.data(), sizeof(V) * src.size(), hipMemcpyHostToDevice, st));
	return LPP_OK;
}
} // namespace

// ---- shared by the builders of the special layouts (lpp_engine_impl.h) -----------------------------------------------------------------
LayoutGate layout_gate(const lpp_engine* e, const char* force_switch, bool keep_plain_csr_refuses, bool any_compress_value)
{
	bool forced = false;
	if (const char* s = getenv(force_switch)) {
		if (atoi(s) == 0) return LayoutGate::Never;
		forced = true;
	}
	const CsrSwitches sw = csr_switches_from_env();
	if (e->cfg.spmv_kernel != LPP_SPMV_AUTO || sw.spmv_kernel.set) return LayoutGate::Never;
	int want = e->cfg.compress_values;
	if (sw.compress_values.set) want = any_compress_value ? 0 : sw.compress_values.v;
	if (want == 0) return LayoutGate::Never;
	// switches of the general layout: measure that one
	if (sw.shared_offsets.set || sw.local16.set || sw.diag_codes.set || sw.block_template.set || sw.window_rows.set) return LayoutGate::Never;
	if (keep_plain_csr_refuses && sw.keep_plain_csr.set) return LayoutGate::Never;
	return forced ? LayoutGate::Forced : LayoutGate::BySize;
}

lpp_status DictTable::init(hipStream_t st)
{
	HIP_TRY_MEM(hipMalloc(&table.p, sizeof(unsigned long long) * kDictTable));
	HIP_TRY_MEM(hipMalloc(&overflow.p, sizeof(int)));
	HIP_TRY(hipMemsetAsync(table.p, 0xff, sizeof(unsigned long long) * kDictTable, st));
	HIP_TRY(hipMemsetAsync(overflow.p, 0, sizeof(int), st));
	return LPP_OK;
}

lpp_status DictTable::fetch(hipStream_t st)
{
	host.resize(kDictTable);
	HIP_TRY(hipMemcpyAsync(host.data(), table.p, sizeof(unsigned long long) * kDictTable, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&ov, overflow.p, sizeof(int), hipMemcpyDeviceToHost, st));
	return LPP_OK;
}

// More than 256 distinct diagonal values (site-dependent hubbardU / potentialV, HubbardHelper.h:138-189: disorder) do not end the layout:
// the diagonal then travels as ONE plain f64 stream (8 instead of 1 byte per row), added by the streaming pass behind the two product
// kernels (PbCombineArgs::d); T and C stay what they are.  LPP_PB_PLAIN_DIAG=1 forces it (tests).
PbDict pb_diag_dict(const DictTable& t, bool honour_switch, const double* extra, size_t n_extra)
{
	PbDict d;
	std::vector<unsigned long long> keys; // (code 0 = +0.0, the padding places of k_pb_down: dict256_from_keys)
	size_t ndiag = 0;
	for (unsigned long long k : t.host)
		if (k != kDictEmpty) ndiag++;
	const char* sw = honour_switch ? getenv("LPP_PB_PLAIN_DIAG") : nullptr;
	d.plain_diag = t.ov != 0 || ndiag > 250 || (sw && atoi(sw) != 0);
	if (d.plain_diag && sw && atoi(sw) == 0) return d; // switched off: general layout
	if (!d.plain_diag)
		for (unsigned long long k : t.host)
			if (k != kDictEmpty) keys.push_back(k);
	for (size_t p = 0; p < n_extra; p++) {
		unsigned long long k;
		std::memcpy(&k, &extra[p], 8);
		keys.push_back(k);
	}
	d.ndict = dict256_from_keys(std::move(keys), d.dict);
	d.applies = d.ndict > 0;
	return d;
}

lpp_status pb_build_host(lpp_engine* e, PbBuildInput in, bool cplx)
{
	if (!cplx) return pb_build(e, in);
	std::vector<int64_t> rrp;
	std::vector<int32_t> rci;
	std::vector<double> rva;
	pb_realify(in.n_up, in.t_rp, in.t_ci, in.t_va, rrp, rci, rva);
	const PbCplxInput cx { in.n_up, in.t_rp, in.t_ci, in.t_va, in.c_va };
	in.cx = &cx;
	in.n_up *= 2;
	in.t_rp = rrp.data();
	in.t_ci = rci.data();
	in.t_va = rva.data();
	in.c_va = nullptr;
	return pb_build(e, in);
}

namespace {
// largest |a - b| and largest |b| as the bit patterns of non-negative doubles (ordered like unsigned integers)
__global__ void k_max_diff(int64_t n, const double* __restrict__ a, const double* __restrict__ b, unsigned long long* __restrict__ out)
{
	double d = 0.0, m = 0.0;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
		d = fmax(d, fabs(a[i] - b[i]));
		m = fmax(m, fabs(b[i]));
		if (a[i] != a[i]) d = 1e300;
	}
	atomicMax(out, (unsigned long long)__double_as_longlong(d));
	atomicMax(out + 1, (unsigned long long)__double_as_longlong(m));
}
__global__ void k_sum_i64(const int64_t* __restrict__ v, int64_t n, unsigned long long* __restrict__ out)
{
	unsigned long long s = 0;
	for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) s += (unsigned long long)v[k];
	for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
	if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}
} // namespace

void sum_i64(hipStream_t st, const int64_t* v, int64_t n, unsigned long long* out) { k_sum_i64<<<1024, 256, 0, st>>>(v, n, out); }

lpp_status row_walk_compare(lpp_engine* e, int64_t n, const double* a, const double* b, bool* same, double* dmax, double* xmax)
{
	*same = false;
	hipStream_t st = e->stream;
	DevBuf d_cmp;
	HIP_TRY_MEM(hipMalloc(&d_cmp.p, sizeof(unsigned long long) * 2));
	HIP_TRY(hipMemsetAsync(d_cmp.p, 0, sizeof(unsigned long long) * 2, st));
	k_max_diff<<<1024, 256, 0, st>>>(n, a, b, (unsigned long long*)d_cmp.p);
	unsigned long long cmp[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(cmp, d_cmp.p, sizeof(cmp), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	std::memcpy(dmax, &cmp[0], 8);
	std::memcpy(xmax, &cmp[1], 8);
	*same = *dmax <= 1e-12 * std::max(*xmax, 1e-300);
	return LPP_OK;
}

// ---- kernel arguments: everything that comes from the state, in one place per struct; whatever is not named here is zero -----------
// k_pb_down (all forms) and k_pb_down_image on rows of `pitch` positions; the caller sets y, z, u_in, shift, partial, sc, u_has_beta, pf_lead
static PbDownArgs down_args(const PbState& B, int64_t pitch)
{
	PbDownArgs d = {};
	d.pitch = pitch;
	d.n_blk = B.n_blk;
	d.npanels = (int)(pitch / 16);
	d.ids_per_wg = B.ids_per_wg;
	d.rounds = B.down_rounds;
	d.ids_per_round = B.ids_per_round;
	d.image = (const uint4*)B.down_image;
	d.rowcap = B.rowcap;
	d.c_ptr = B.c_ptr;
	d.c_col = B.c_col;
	d.c_code = B.c_code;
	d.dict = B.dict;
	d.cdict = (const double2*)B.cdict;
	d.pace = B.pace;
	d.order = B.order;
	return d;
}

// k_pb_up (all forms); the caller sets dcode, n_blk, y, u, partial, sc and, in the chained form, wbuf, ybuf, g_a, g_b2
static PbUpArgs up_args(const PbState& B)
{
	PbUpArgs u = {};
	u.tw = B.tw;
	u.tw_off = B.tw_off;
	u.tw_len = B.tw_len;
	u.G = B.G;
	for (int g = 0; g < kPbMaxGroups; g++) u.gval[g] = B.gval[g];
	u.dict = B.dict;
	u.n_up = B.n_up;
	u.pitch = B.pitch;
	u.spb = B.spb;
	return u;
}

// k_pb_combine; the caller sets a_ptr, b2_prev and the partials it wants
static PbCombineArgs combine_args(const PbState& B, void* x, const void* y, const EpiScale& sc)
{
	PbCombineArgs c = {};
	c.n2 = (B.n_blk * B.pitch) >> 1;
	c.x = (double2*)x;
	c.y = (const double2*)y;
	c.u = (const double2*)B.u;
	c.z = B.c_nnz > 0 ? (const double2*)B.z : nullptr;
	c.sc = sc;
	c.d = (const double2*)B.dval;
	return c;
}

// k_pb_up_big and k_pb_up_big2; the caller sets dcode, n_blk, y, u, partial, sc
static PbUpBigArgs up_big_args(const PbState& B)
{
	PbUpBigArgs a = {};
	a.tw = B.tw;
	a.tw_off = B.tw_off;
	a.tw_len = B.tw_len;
	a.fw = B.fw;
	a.f_off = B.f_off;
	a.f_len = B.f_len;
	a.G = B.G;
	for (int g = 0; g < B.G; g++) a.gval[g] = B.gval[g];
	a.dict = B.dict;
	a.n_up = B.n_up;
	a.pitch = B.pitch;
	a.W = B.W;
	a.npieces = B.npieces;
	return a;
}

// k_pb_up_seg; the caller sets dcode, n_blk, y, u, partial, sc
static PbSegArgs seg_args(const PbState& B)
{
	PbSegArgs g = {};
	g.items = (const SegItem*)B.seg_items;
	g.nitems = B.seg_nitems;
	g.cross = (const SegCross*)B.seg_cross;
	g.hh = (const SegHh*)B.seg_hh;
	g.slices = (const SegSlice*)B.seg_slices;
	g.tw = B.seg_tw;
	g.xw = B.seg_xw;
	g.G = B.G;
	for (int v = 0; v < std::min(B.G, 2); v++) g.gval[v] = B.gval[v];
	g.dict = B.dict;
	g.n_up = B.n_up;
	g.pitch = B.pitch;
	g.ws = B.seg_ws;
	g.wmax = B.seg_wmax;
	g.flat = B.seg_one ? 1 : 0;
	return g;
}

// k_pb_down_parts on rows of `pitch` positions; the caller sets y, z, partial, sc
static PbDownPartsArgs down_parts_args(const PbState& B, int64_t pitch)
{
	PbDownPartsArgs d = {};
	d.pitch = pitch;
	d.n_blk = B.n_blk;
	d.npanels = (int)(pitch / 16);
	d.ids_per_wg = B.ids_per_wg;
	d.nparts = B.nparts;
	d.ent_cap = B.ent_cap;
	d.c_ptr = B.c_ptr;
	d.c_col = B.c_col;
	d.c_code = B.c_code;
	d.c_pstart = B.c_pstart;
	d.order = B.order;
	d.dict = B.dict;
	d.pace = B.pace;
	d.pace_stride = B.pace_stride;
	return d;
}

// ---- kernel instances: a list of lpp_pb_instances.h is instantiated entry by entry, and nothing else is --------------------------------
static_assert(kPbBigPre == kBigPre, "the lists name k_pb_up_big's default depth");
template <typename Args> using Kernel = void (*)(Args);
template <typename Args, typename At, size_t... I> static Kernel<Args> kernel_table_at(int i, At at, std::index_sequence<I...>)
{
	const Kernel<Args> t[] = { at(std::integral_constant<size_t, I> {})... };
	return i < 0 ? nullptr : t[i];
}
// the kernel of `key`, null when the list does not hold it; at(i) names the template instance of the list's entry i
template <typename Args, typename K, size_t N, typename At> static Kernel<Args> kernel_of(const std::array<K, N>& list, const K& key, At at)
{
	return kernel_table_at<Args>(inst_index(list, key), at, std::make_index_sequence<N> {});
}
static Kernel<PbUpArgs> up_kernel(const PbUpInst& key)
{
	return kernel_of<PbUpArgs>(kPbUpInsts, key, [](auto i) -> Kernel<PbUpArgs> {
		constexpr PbUpInst k = kPbUpInsts[decltype(i)::value];
		return k_pb_up<k.dot, k.gt, k.chain, k.pre0>;
	});
}
static Kernel<PbUpBigArgs> big_kernel(const PbBigInst& key)
{
	return kernel_of<PbUpBigArgs>(kPbBigInsts, key, [](auto i) -> Kernel<PbUpBigArgs> {
		constexpr PbBigInst k = kPbBigInsts[decltype(i)::value];
		return k_pb_up_big<k.dot, k.gt, k.pre>;
	});
}
static Kernel<PbUpBigArgs> big2_kernel(const PbBigInst& key)
{
	return kernel_of<PbUpBigArgs>(kPbBig2Insts, key, [](auto i) -> Kernel<PbUpBigArgs> {
		constexpr PbBigInst k = kPbBig2Insts[decltype(i)::value];
		return k_pb_up_big2<k.dot, k.gt, k.pre>;
	});
}
static Kernel<PbSegArgs> seg_kernel(const PbSegInst& key)
{
	return kernel_of<PbSegArgs>(kPbSegInsts, key, [](auto i) -> Kernel<PbSegArgs> {
		constexpr PbSegInst k = kPbSegInsts[decltype(i)::value];
		return k_pb_up_seg<k.dot, k.gt, k.p0, 4, k.shape.nc, k.shape.nh, k.shape.rows>;
	});
}
static Kernel<PbDownArgs> down_kernel(const PbDownInst& key)
{
	return kernel_of<PbDownArgs>(kPbDownInsts, key, [](auto i) -> Kernel<PbDownArgs> {
		constexpr PbDownInst k = kPbDownInsts[decltype(i)::value];
		return k_pb_down<1024, k.rmw, k.wide, k.cplx, k.pf>;
	});
}
static Kernel<PbDownPartsArgs> parts_kernel(const PbPartsInst& key)
{
	return kernel_of<PbDownPartsArgs>(kPbPartsInsts, key, [](auto i) -> Kernel<PbDownPartsArgs> {
		constexpr PbPartsInst k = kPbPartsInsts[decltype(i)::value];
		return k_pb_down_parts<kPbPartsThreads, k.r>;
	});
}

// the kernels of the planned form.  pb_plan has checked every key against the same lists: a miss here is an internal error
static lpp_status resolve_kernels(PbState& B)
{
	PbKernels& k = B.k;
	bool ok = true;
	for (int dot = 0; dot < 2; dot++) {
		if (B.seg) ok = (k.up_seg[dot] = seg_kernel(pb_seg_inst(B, dot != 0))) && ok;
		else if (B.big2) ok = (k.up_big[dot] = big2_kernel(pb_big2_inst(B, dot != 0))) && ok;
		else if (B.big) ok = (k.up_big[dot] = big_kernel(pb_big_inst(B, dot != 0))) && ok;
		else ok = (k.up[dot] = up_kernel(pb_up_inst(B, dot != 0, false))) && ok;
	}
	if (B.parts) ok = (k.down_parts = parts_kernel(pb_parts_inst(B))) && ok;
	else ok = (k.down = down_kernel(pb_down_inst(B, false))) && ok;
	if (B.chain_ok) {
		ok = (k.up_chain = up_kernel(pb_up_inst(B, false, true))) && ok;
		ok = (k.down_chain = down_kernel(pb_down_inst(B, true))) && ok;
	}
	return ok ? LPP_OK : fail(LPP_ERR_STATE, "pb_build: the planned form names a kernel instance that does not exist");
}

// Straight-line: the switches, the plan (lpp_pb_plan.cpp: every decision, refusal and host vector), then uploads and allocations in a fixed
// order.  Nothing here decides anything beyond "was this vector planned".
lpp_status pb_build(lpp_engine* e, const PbBuildInput& in)
{
	free_pb(e);
	PbState& B = e->pb;
	hipStream_t st = e->stream;
	const PbSwitches sw = pb_switches_from_env();
	PbPlan P;
	lpp_status rc = pb_plan(in, sw, e->num_cus, P);
	if (rc != LPP_OK) return rc;
	if (sw.verbose) pb_plan_print(P);
	static_cast<PbForm&>(B) = P.form;
	const PbTemplate& T = P.T;
	const SegPlan& SP = P.seg;
	auto up = [&](auto** dst, const auto& src) { // (after a failure the rest is skipped)
		if (rc == LPP_OK) rc = to_device(dst, src, st);
	};
	if (!P.perm.empty()) {
		up(&B.perm, P.perm);
		up(&B.inv, P.inv);
	}
	if (B.seg) {
		up((SegItem**)&B.seg_items, SP.items);
		up((SegInst**)&B.seg_segs, SP.segs);
		up((SegCross**)&B.seg_cross, SP.cross);
		up((SegHh**)&B.seg_hh, SP.hh);
		up((SegSlice**)&B.seg_slices, SP.slices);
		up(&B.seg_tw, SP.words);
		up(&B.seg_xw, SP.xwords);
	}
	up(&B.tw, T.words);
	up(&B.tw_off, T.off);
	up(&B.tw_len, T.len);
	if (!T.foff.empty()) { // the pieces form's far lists
		up(&B.fw, T.fwords);
		up(&B.f_off, T.foff);
		up(&B.f_len, T.flen);
	}
	up(&B.t_ptr, P.tp);
	up(&B.t_col, P.tc);
	up(&B.t_val, P.tv);
	up(&B.c_ptr, P.cp);
	up(&B.c_col, P.cc);
	up(&B.c_code, P.ccode);
	up(&B.dict, P.dict);
	if (!P.cdict.empty()) up(&B.cdict, P.cdict);
	up(&B.blockbase, P.base);
	if (B.parts) up(&B.c_pstart, P.pstart);
	up(&B.order, P.order);
	if (rc != LPP_OK) return rc;
	if (P.image_bytes > 0) {
		HIP_TRY_MEM(hipMalloc(&B.down_image, P.image_bytes));
		k_pb_down_image<<<P.slots * B.down_rounds, 256, 0, st>>>(down_args(B, B.pitch), (uint4*)B.down_image); // (reads the lists, the order and the round geometry only)
	}
	if (P.pace_counters > 0) HIP_TRY_MEM(hipMalloc(&B.pace, sizeof(int) * P.pace_counters));
	// the two parts of a product (padding stays zero) and the carried scalar; with the transposition exchange the couplings'
	// part is written straight into the exchange buffer
	const size_t loc = (size_t)std::max<int64_t>(B.nblk_loc, 1) * (size_t)B.pitch;
	if (!B.tx) {
		HIP_TRY_MEM(hipMalloc(&B.z, sizeof(double) * loc));
		HIP_TRY(hipMemsetAsync(B.z, 0, sizeof(double) * loc, st));
	}
	HIP_TRY_MEM(hipMalloc(&B.u, sizeof(double) * loc));
	HIP_TRY(hipMemsetAsync(B.u, 0, sizeof(double) * loc, st));
	HIP_TRY_MEM(hipMalloc(&B.xy, sizeof(double) * 2));
	HIP_TRY(hipMemsetAsync(B.xy, 0, sizeof(double) * 2, st));
	HIP_TRY_MEM(hipMalloc(&B.dcode, loc));
	HIP_TRY(hipMemsetAsync(B.dcode, 0, loc, st));
	HIP_TRY(hipStreamSynchronize(st));
	e->pitch = B.cplx ? B.pitch / 2 : B.pitch; // in vector elements
	e->pitch_rows = B.cplx ? B.n_c : B.n_up;
	e->pitch_blocks = B.nblk_loc;
	if ((rc = resolve_kernels(B)) != LPP_OK) return rc;
	B.active = true;
	return LPP_OK;
}

// ---- launches ----------------------------------------------------------------------------------------------------------
// Nothing from here to the handed-over-CSR section reads the environment.  Which form of a kernel a launch takes was decided at the
// end of pb_build and is kept in PbState (chain_ok, down_tasks, down_pf, chain_drop_pace, lazy_tx): LPP_PB_CHAIN, LPP_PB_DOWN_TASKS,
// LPP_PB_DOWN_PF, LPP_PB_CHAIN_PACE and LPP_PB_LAZY_TX take effect when the layout is BUILT, not at the first or at every launch.
// Kernel arguments come from the builders above pb_build (down_args, up_args, ...), the template instance from PbState::k (resolve_kernels,
// at the end of pb_build); a launch site sets only what is its own.
//
// x = beta x + alpha H y (EpiScale semantics of the other product kernels) as two independent kernels that only read y,
//   k_pb_down  z = alpha C y            (+ partials of Re<y|z>)
//   k_pb_up    u = alpha (T y + D y)    (+ partials of Re<y|u>, stored in front of the first kernel's)
// and a streaming pass x = beta x + u + z (k_pb_combine).  defer_combine: the caller runs that pass itself, folded into its own
// pass over x (pb_combine_axpy of the scale-free recurrence).  Returns the number of partials written; their sum is
// Re<y | u + z>, to which the caller adds beta Re<y | x_old> (pb.xy, left by the previous combine pass).
// ---- rows beyond one LDS window / vectors beyond 4 GiB (lpp_pbig_kernels.h) -------------------------------------------
static int big_grid(const lpp_engine* e, int64_t cnt)
{
	const PbState& B = e->pb;
	// one workgroup per CU, items = (pair of blocks of one XCD, piece)
	if (B.big2 || B.seg) return launch_grid((B.seg_one ? cnt : (cnt + 1) / 2) * B.npieces, e->num_cus);
	const size_t lds = pb_big_lds_bytes(B.W);
	return launch_grid(cnt * B.npieces, e->num_cus, std::max(1, std::min(2, (int)(((size_t)160 * 1024) / (lds + 512)))));
}

// in-block part by pieces: `cnt` blocks from `y` (pitched), result to `u`; returns the number of partials written
static int launch_up_big(lpp_engine* e, const double* y, double* u, const uint8_t* dcode, int64_t cnt, double* partial, const EpiScale& sc, hipStream_t st)
{
	const PbState& B = e->pb;
	const int nb = big_grid(e, cnt), dot = partial ? 1 : 0;
	if (B.seg) { // cross / high-high hops per segment: the instance the plan padded its lists for; chunks of value group 0 requested ahead: its choice
		PbSegArgs g = seg_args(B);
		g.dcode = dcode;
		g.n_blk = cnt;
		g.y = y;
		g.u = u;
		g.partial = partial;
		g.sc = sc;
		launch_lds(B.k.up_seg[dot], nb, kSegThreads, pb_seg_lds_bytes(B.seg_ws, B.seg_wmax, B.seg_one ? 1 : 2), st, g);
		return partial ? nb : 0;
	}
	PbUpBigArgs a = up_big_args(B);
	a.dcode = dcode;
	a.n_blk = cnt;
	a.y = y;
	a.u = u;
	a.partial = partial;
	a.sc = sc;
	// (two blocks per workgroup, four value groups: two chunks of each ahead -- three spill: 5.00 against 4.74 ms at 1.47e8 complex states)
	if (B.big2) launch_lds(B.k.up_big[dot], nb, kPbBig2Threads, pb_big2_lds_bytes(B.W), st, a);
	else launch_lds(B.k.up_big[dot], nb, kPbBigThreads, pb_big_lds_bytes(B.W), st, a);
	return partial ? nb : 0;
}

// The plain coupling kernel with the tasks of a step handed out by the LDS counter and NO pacing between the workgroups of a group (k_pb_down<.., PF>
// with pace == null: the barrier per step keeps a workgroup together, the counter keeps its waves on neighbouring tasks): faster where a panel of all blocks
// fits an XCD's L2 with room to spare -- complex couplings at 11440 blocks 2.27 -> 2.08 ms, the 3x6 lattice's (6,6) sector (18564 blocks) 2.72 -> 2.56 ms -- and
// slower where it does not (38760 blocks, 4.96 MB: 28.4 -> 35.8 ms; with pacing on top of the counter 28.5): up to 3 MB per panel (pb_panel_fits_l2), and
// only where the task sums fit LDS (pb_down_pf_fits).  LPP_PB_DOWN_TASKS=0 / 1 overrides the panel test.  PbState::down_tasks
static void pb_launch_down_plain(const PbState& B, PbDownArgs& d, hipStream_t st)
{
	const bool tasks = B.down_tasks;
	if (tasks) d.pace = nullptr;
	if (d.pace) (void)hipMemsetAsync(d.pace, 0, sizeof(int) * 8 * (size_t)d.npanels, st);
	launch_lds(B.k.down, B.down_grid, 1024, tasks ? B.down_lds_pf : B.down_lds, st, d);
}

// block couplings over parts of the source range: z = alpha C y on rows of `pitch` positions; returns the number of partials written
static int launch_down_parts(lpp_engine* e, const double* y, double* z, int64_t pitch, double* partial, const EpiScale& sc, hipStream_t st)
{
	const PbState& B = e->pb;
	PbDownPartsArgs d = down_parts_args(B, pitch);
	d.y = y;
	d.z = z;
	d.partial = partial;
	d.sc = sc;
	if (d.pace) (void)hipMemsetAsync(d.pace, 0, sizeof(int) * 8 * (size_t)B.pace_stride, st);
	launch_lds(B.k.down_parts, B.down_grid, kPbPartsThreads, B.down_lds, st, d);
	return partial ? B.down_grid : 0;
}

// 8192 blocks x 4 elements in flight: 5.2 TB/s for the 4-read 1-write mix (4.7 with 2048 x 2), scripts/experiments/calib_combine.hip
static int combine_blocks(int64_t n2) { return (int)std::max<int64_t>(1, std::min<int64_t>((n2 + 4 * kBlock - 1) / (4 * kBlock), 8192)); }

int pb_launch(lpp_engine* e, const void* y, void* x, double* partial, const EpiScale& sc, bool defer_combine)
{
	PbState& B = e->pb;
	hipStream_t st = e->stream;
	const int nb = B.big ? big_grid(e, B.n_blk) : (int)std::max<int64_t>(1, std::min<int64_t>(B.n_blk, (int64_t)e->num_cus));
	double* const want_dot = partial;
	if (!defer_combine) partial = nullptr; // the combine pass below forms Re<y|x> of the finished x itself
	int np = partial ? nb : 0;
	// (the two kernels only read y; side by side on the same CUs they ran 4.95 instead of 2.69 ms at config 2 -- the in-block kernel's
	// traffic evicts the panel from L2 -- so they run one after the other: scripts/experiments/README.md)
	const bool both = B.c_nnz > 0;
	hipStream_t sd = st;
	if (both && B.parts) {
		const int n = launch_down_parts(e, (const double*)y, B.z, B.pitch, partial ? partial + nb : nullptr, sc, sd);
		if (partial) np += n;
	} else if (both) {
		PbDownArgs d = down_args(B, B.pitch);
		d.y = (const double*)y;
		d.z = B.z;
		d.partial = partial ? partial + nb : nullptr;
		d.sc = sc;
		pb_launch_down_plain(B, d, sd);
		if (partial) np += B.down_grid;
	}
	if (B.big) {
		launch_up_big(e, (const double*)y, B.u, B.dcode, B.n_blk, partial, sc, st); // nb partials, in front of the couplings'
	} else {
		PbUpArgs u = up_args(B);
		u.dcode = B.dcode;
		u.n_blk = B.n_blk;
		u.y = (const double*)y;
		u.u = B.u;
		u.partial = partial;
		u.sc = sc;
		launch_lds(B.k.up[partial ? 1 : 0], nb, kPbUpThreads, pb_up_lds_bytes(B.pitch, B.spb, B.G), st, u);
	}
	if (!defer_combine) {
		PbCombineArgs c = combine_args(B, x, y, sc);
		const int nbc = combine_blocks(c.n2);
		c.partial_nrm = want_dot ? want_dot + nbc : nullptr; // |x|^2 partials: not used by these callers
		c.partial_xy = want_dot;
		k_pb_combine<<<nbc, kBlock, 0, st>>>(c);
		if (want_dot) np = nbc;
	}
	return np;
}

// ---- several GPUs, transposition exchange -----------------------------------------------------------------------------
// Per step and rank (one_step):  pack -> all-to-all #1 || pb_tx_up(first half of the own blocks) -> pb_tx_down on the received
// transposed slice -> all-to-all #2 || pb_tx_up(second half) -> pb_tx_unpack_combine.  Both parts of the product are the
// single-GPU kernels: the in-block kernel on the rank's own blocks, the panel-major coupling kernel on the transposed slice
// (all N_down blocks, rows = this rank's up-index range: the same C (x) 1 structure with narrower rows).
void pb_tx_up(lpp_engine* e, const void* y, const EpiScale& sc, int64_t b0, int64_t cnt)
{
	PbState& B = e->pb;
	if (cnt <= 0) return;
	if (B.big) {
		launch_up_big(e, (const double*)y + b0 * B.pitch, B.u + b0 * B.pitch, B.dcode + b0 * B.pitch, cnt, nullptr, sc, e->stream);
		return;
	}
	PbUpArgs u = up_args(B);
	u.dcode = B.dcode + b0 * B.pitch;
	u.n_blk = cnt;
	u.y = (const double*)y + b0 * B.pitch;
	u.u = B.u + b0 * B.pitch;
	u.sc = sc;
	const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(cnt, (int64_t)e->num_cus));
	launch_lds(B.k.up[0], nb, kPbUpThreads, pb_up_lds_bytes(B.pitch, B.spb, B.G), e->stream, u);
}

void pb_tx_down(lpp_engine* e, const void* gath, void* send2, const EpiScale& sc)
{
	PbState& B = e->pb;
	if (B.parts) {
		launch_down_parts(e, (const double*)gath, (double*)send2, B.pitch_dn, nullptr, sc, e->stream);
		return;
	}
	PbDownArgs d = down_args(B, B.pitch_dn); // (cdict: null here as before -- pb_build refuses complex hoppings on the exchange)
	d.y = (const double*)gath;
	d.z = (double*)send2;
	d.sc = sc;
	pb_launch_down_plain(B, d, e->stream);
}

int pb_tx_unpack_combine(lpp_engine* e, void* x, const void* y, const void* recv2, const EpiScale& sc, int64_t chunk, double* partial, const double* shift)
{
	const PbState& B = e->pb;
	const int64_t n2 = (B.nblk_loc * B.pitch) >> 1;
	const int nb = combine_blocks(n2);
	k_pb_unpack_combine<<<nb, kBlock, 0, e->stream>>>((double2*)x, (const double2*)y, (const double2*)B.u, (const double2*)recv2, B.nblk_loc, B.pitch >> 1,
	                                                  B.pitch_dn >> 1, chunk >> 1, sc, partial, shift, (const double2*)B.dval);
	return nb;
}

// ---- the chained scale-free step (k_pb_up<KC>, k_pb_down<RMW>) -------------------------------------------------
// (a plain-stream diagonal is attached by pb_build's caller, after the build: the streaming pass of the three-kernel form adds it)
bool pb_chain_ok(const lpp_engine* e) { return e->pb.chain_ok && !e->pb.dval; }

// One scale-free Lanczos step in two launches.  In: w (= w_{j-1}, or r_j itself when g_a is null) and y (= r_{j-1}).
// Out: w holds r_j, y holds w_j = alpha H r_j + beta r_{j-1} (the in-block part passes through pb.u); partial holds pairs (Re<r_j|w_j>, |w_j|^2), their number is returned
// (negative: the state is not one the chained kernels serve, nothing was launched).
int pb_launch_chain(lpp_engine* e, void* w, void* y, double* partial, const EpiScale& sc, const double* g_a, const double* g_b2, const double* shift)
{
	PbState& B = e->pb;
	hipStream_t st = e->stream;
	// k_pb_down<RMW> adds u_in and touches the u lines ahead once per panel: one LDS image per workgroup, whatever let the caller in here
	if (B.down_rounds != 1 || !B.k.up_chain || !B.k.down_chain) return -1;
	const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(B.n_blk, (int64_t)e->num_cus));
	PbUpArgs u = up_args(B);
	u.dcode = B.dcode;
	u.n_blk = B.n_blk;
	u.u = B.u;
	u.sc = sc;
	u.wbuf = (double*)w;
	u.ybuf = (double*)y;
	u.g_a = g_a;
	u.g_b2 = g_b2;
	// beta r_{j-1} rides in u (k_pb_up<CHAIN>), so the coupling kernel reads one stream less
	launch_lds(B.k.up_chain, nb, kPbUpThreads, pb_up_lds_bytes(B.pitch, B.spb, B.G), st, u);
	PbDownArgs d = down_args(B, B.pitch);
	d.y = (const double*)w;
	d.z = (double*)y;
	d.u_in = B.u;
	d.shift = shift;
	d.partial = partial;
	d.sc = sc;
	d.u_has_beta = 1; // the in-block kernel has put beta r_{j-1} into u
	// the last wave touches the u lines ahead of the tasks and the tasks are handed out by a counter (k_pb_down<..., PF>): config 2 3.03 -> 2.88 ms
	// per step; LPP_PB_DOWN_PF=0: every wave its fixed share of the tasks, no touching (PbState::down_pf)
	const bool pf = B.down_pf;
	d.pf_lead = 2;
	// ... and with the tasks handed out by a counter and a barrier per panel the workgroups of a group stay together by themselves: the bounded pacing
	// (one atomic, one poll and one more barrier per panel, a memset per launch) only costs here -- config 2 1.51 -> 1.41 ms, the 4x4 lattice's (7,7) sector
	// 1.19 -> 1.08, complex hoppings at (6,6) 1.25 -> 1.09 ms; the plain kernel needs it (3x6 lattice, (6,6): 2.7 ms with, 6.1 without).  LPP_PB_CHAIN_PACE=1: keep it;
	// a panel beyond an XCD's L2 keeps it too (PbState::chain_drop_pace)
	if (B.chain_drop_pace) d.pace = nullptr;
	if (d.pace) (void)hipMemsetAsync(d.pace, 0, sizeof(int) * 8 * (size_t)d.npanels, st);
	launch_lds(B.k.down_chain, B.down_grid, 1024, pf ? B.down_lds_pf : B.down_lds, st, d);
	return B.down_grid;
}

// leave the chained form: run the pending pass y = y - g x and restore the carried <y | x_old>
void pb_materialise(lpp_engine* e, void* y, const void* x, const double* g_a, const double* g_b2, double* partial)
{
	const PbState& B = e->pb;
	const int64_t n2 = (B.n_blk * B.pitch) >> 1;
	const int nb = combine_blocks(n2);
	k_pb_materialise<<<nb, kBlock, 0, e->stream>>>((double2*)y, (const double2*)x, g_a, g_b2, n2, partial);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>(partial, nb, 1, 1, B.xy);
}

int pb_combine_axpy(lpp_engine* e, void* x, const void* y, const EpiScale& sc, const double* a_ptr, const double* b2_prev, double* partial)
{
	const PbState& B = e->pb;
	PbCombineArgs c = combine_args(B, x, y, sc);
	c.a_ptr = a_ptr;
	c.b2_prev = b2_prev;
	const int nb = combine_blocks(c.n2);
	c.partial_nrm = partial;
	c.partial_xy = partial + nb;
	c.partial_dq = B.dval ? partial + 2 * nb : nullptr;
	k_pb_combine<<<nb, kBlock, 0, e->stream>>>(c);
	k_reduce_final<<<1, kBlock, 0, e->stream>>>(partial + nb, nb, 1, 1, B.xy); // next step's <y | x_old>
	if (B.dval) k_reduce_final<<<1, kBlock, 0, e->stream>>>(partial + 2 * nb, nb, 1, 1, B.xy + 1); // and its <y | D y>
	return nb;
}

// ---- a CSR that was handed over (lpp_engine_set_csr / _set_csr_device) -------------------------------------------------
// The reference hands its matrix over as a CSR (DefaultSymmetry.h:54-57 -> InternalProductStored.h:116).  When that CSR is of
// the product-basis form -- basis block n_up (the caller's hint or the detected one), every block's in-block part equal to
// block 0's (= T), every leaving entry a position-preserving block coupling (= C), a stored diagonal in every row (= D) -- it
// is taken into the same layout device assembly builds: T from block 0, C from the first row of every block, D from the
// diagonals, then EVERY row of the CSR is compared with the row (T, C, D) stand for, entry by entry and bit by bit
// (k_pb_csr_verify).  Only a CSR that passes is dropped; anything else keeps the general layout.  *done says which.
lpp_status pb_from_csr(lpp_engine* e, const DevCsr& A, int64_t n_up, bool* done)
{
	*done = false;
	if (n_up < kPbMinRows || A.nrows <= 0 || A.nrows % n_up != 0 || !A.col || !A.val) return LPP_OK;
	const bool cplx = e->is_complex != 0; // complex hoppings: realified in-block matrix, complex couplings (PbState::cplx)
	if (cplx && getenv("LPP_PB_COMPLEX") && atoi(getenv("LPP_PB_COMPLEX")) == 0) return LPP_OK;
	const size_t vd = cplx ? 2 : 1; // doubles per matrix value
	const int64_t n_blk = A.nrows / n_up;
	if (n_blk < 2 || n_blk > 65535) return LPP_OK;
	const LayoutGate gate = layout_gate(e, "LPP_PRODUCT_LAYOUT");
	if (gate == LayoutGate::Never) return LPP_OK;
	if (gate == LayoutGate::BySize && (size_t)A.nrows * vd * sizeof(double) < (cplx ? (size_t)512 << 20 : (size_t)32 << 20)) return LPP_OK; // as for device assembly (assemble_hubbard_pb)
	hipStream_t st = e->stream;
	const int64_t pitch = pb_pitch_for(cplx ? 2 * n_up : n_up); // in doubles
	DevBuf d_bad, d_clen, d_cptr, d_ccol, d_cval, d_dval;
	HIP_TRY_MEM(hipMalloc(&d_bad.p, sizeof(int) * 2));
	HIP_TRY(hipMemsetAsync(d_bad.p, 0, sizeof(int) * 2, st));
	// T: block 0's rows, columns inside the block
	std::vector<int64_t> rp0((size_t)n_up + 1);
	HIP_TRY(hipMemcpyAsync(rp0.data(), A.rowptr, sizeof(int64_t) * (size_t)(n_up + 1), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const int64_t n0 = rp0[(size_t)n_up];
	if (n0 <= 0 || n0 > ((int64_t)1 << 28)) return LPP_OK;
	std::vector<int32_t> c0((size_t)n0);
	std::vector<double> v0((size_t)n0 * vd);
	HIP_TRY(hipMemcpyAsync(c0.data(), A.col, sizeof(int32_t) * (size_t)n0, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(v0.data(), A.val, sizeof(double) * vd * (size_t)n0, hipMemcpyDeviceToHost, st));
	// C: the first row of every block
	HIP_TRY_MEM(hipMalloc(&d_clen.p, sizeof(int64_t) * (size_t)(n_blk + 1)));
	const int nbb = (int)((n_blk + 255) / 256);
	if (cplx)
		k_pb_csr_couplings<false, double2><<<nbb, 256, 0, st>>>(n_up, n_blk, A.rowptr, A.col, (const double2*)A.val, (int64_t*)d_clen.p, nullptr, nullptr, nullptr, (int*)d_bad.p);
	else
		k_pb_csr_couplings<false, double><<<nbb, 256, 0, st>>>(n_up, n_blk, A.rowptr, A.col, (const double*)A.val, (int64_t*)d_clen.p, nullptr, nullptr, nullptr, (int*)d_bad.p);
	std::vector<int64_t> clen((size_t)n_blk), crp((size_t)n_blk + 1, 0);
	HIP_TRY(hipMemcpyAsync(clen.data(), d_clen.p, sizeof(int64_t) * (size_t)n_blk, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int64_t b = 0; b < n_blk; b++) crp[(size_t)b + 1] = crp[(size_t)b] + clen[(size_t)b];
	const int64_t cz = crp[(size_t)n_blk];
	HIP_TRY_MEM(hipMalloc(&d_cptr.p, sizeof(int64_t) * (size_t)(n_blk + 1)));
	HIP_TRY_MEM(hipMalloc(&d_ccol.p, sizeof(int32_t) * (size_t)std::max<int64_t>(cz, 1)));
	HIP_TRY_MEM(hipMalloc(&d_cval.p, sizeof(double) * vd * (size_t)std::max<int64_t>(cz, 1)));
	HIP_TRY(hipMemcpyAsync(d_cptr.p, crp.data(), sizeof(int64_t) * (size_t)(n_blk + 1), hipMemcpyHostToDevice, st));
	if (cplx)
		k_pb_csr_couplings<true, double2><<<nbb, 256, 0, st>>>(n_up, n_blk, A.rowptr, A.col, (const double2*)A.val, nullptr, (const int64_t*)d_cptr.p, (int32_t*)d_ccol.p,
		                                                      (double2*)d_cval.p, (int*)d_bad.p);
	else
		k_pb_csr_couplings<true, double><<<nbb, 256, 0, st>>>(n_up, n_blk, A.rowptr, A.col, (const double*)A.val, nullptr, (const int64_t*)d_cptr.p, (int32_t*)d_ccol.p,
		                                             (double*)d_cval.p, (int*)d_bad.p);
	std::vector<int32_t> cci((size_t)std::max<int64_t>(cz, 1));
	std::vector<double> cva((size_t)std::max<int64_t>(cz, 1) * vd);
	HIP_TRY(hipMemcpyAsync(cci.data(), d_ccol.p, sizeof(int32_t) * (size_t)cz, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(cva.data(), d_cval.p, sizeof(double) * vd * (size_t)cz, hipMemcpyDeviceToHost, st));
	// D: the stored diagonal of every row, pitched
	const size_t loc = (size_t)n_blk * (size_t)pitch;
	HIP_TRY_MEM(hipMalloc(&d_dval.p, sizeof(double) * loc));
	HIP_TRY(hipMemsetAsync(d_dval.p, 0, sizeof(double) * loc, st));
	const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>((A.nrows + 255) / 256, 1 << 16));
	if (cplx)
		k_pb_csr_diagonal_c<<<nbr, 256, 0, st>>>(n_up, n_blk, pitch, A.rowptr, A.col, (const double2*)A.val, (double*)d_dval.p, (int*)d_bad.p);
	else
		k_pb_csr_diagonal<<<nbr, 256, 0, st>>>(n_up, n_blk, pitch, A.rowptr, A.col, (const double*)A.val, (double*)d_dval.p, (int*)d_bad.p);
	// its distinct values
	DictTable table;
	lpp_status rc;
	if ((rc = table.init(st)) != LPP_OK) return rc;
	k_dict_collect<<<2048, kBlock, 0, st>>>((const double*)d_dval.p, (int64_t)loc, table.dev(), table.dev_overflow());
	int bad[2] = { 0, 0 };
	if ((rc = table.fetch(st)) != LPP_OK) return rc;
	HIP_TRY(hipMemcpyAsync(bad, d_bad.p, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	if (bad[0]) return LPP_OK; // a coupling that does not preserve the position, or a row without a stored diagonal
	std::vector<int64_t> trp((size_t)n_up + 1, 0);
	std::vector<int32_t> tci;
	std::vector<double> tva;
	for (int64_t r = 0; r < n_up; r++) {
		for (int64_t p = rp0[(size_t)r]; p < rp0[(size_t)r + 1]; p++)
			if (c0[(size_t)p] >= 0 && c0[(size_t)p] < n_up) { // pb_build skips the diagonal itself
				tci.push_back(c0[(size_t)p]);
				for (size_t k = 0; k < vd; k++) tva.push_back(v0[(size_t)p * vd + k]);
			}
		trp[(size_t)r + 1] = (int64_t)tci.size();
	}
	const PbDict D = pb_diag_dict(table, true, cplx ? nullptr : cva.data(), cplx ? 0 : (size_t)cz); // (complex couplings: a dictionary of their own, pb_build)
	if (!D.applies) return LPP_OK;
	// two work vectors + the two parts of a product + the diagonal must fit once the CSR is gone (it is still resident here)
	PbBuildInput in;
	in.n_up = n_up;
	in.n_blk = n_blk;
	in.t_rp = trp.data();
	in.t_ci = tci.data();
	in.t_va = tva.data();
	in.c_rp = crp.data();
	in.c_ci = cci.data();
	in.c_va = cva.data();
	in.dict256 = D.dict.data();
	in.ndict = D.ndict;
	rc = pb_build_host(e, in, cplx);
	if (rc == LPP_ERR_INVALID || rc == LPP_ERR_NOMEM) { // not representable, or no room beside the CSR: the general layout
		if (getenv("LPP_VERBOSE")) fprintf(stderr, "lpp: the product-basis layout does not apply to the uploaded matrix: %s\n", lpp_last_error());
		free_pb(e);
		return LPP_OK;
	}
	if (rc != LPP_OK) return rc;
	PbState& B = e->pb;
	// until every row has been verified the engine must not describe a product-basis matrix: any early return below drops the layout
	DropUnlessDone undo { e, done, free_pb };
	if (B.perm) { // the diagonal was read off the CSR in the basis order: into the stored order (pb.u is free until the first product)
		k_pb_permute<true><<<nbr, 256, 0, st>>>(B.u, (const double*)d_dval.p, B.perm, n_blk, n_up, pitch);
		HIP_TRY(hipMemcpyAsync(d_dval.p, B.u, sizeof(double) * loc, hipMemcpyDeviceToDevice, st));
	}
	if (D.plain_diag) {
		B.dval = (double*)d_dval.p; // the codes stay 0 (+0.0)
		d_dval.p = nullptr;
	} else {
		k_pb_codes_from_values<<<nbr, 256, 0, st>>>((int64_t)loc, (const double*)d_dval.p, B.dict, B.ndict, B.dcode);
	}
	if (cplx)
		k_pb_csr_verify_c<<<nbr, 256, 0, st>>>(n_up, n_blk, pitch, B.t_ptr, B.t_col, (const double2*)B.t_val, B.c_ptr, B.c_col, B.c_code, B.blockbase, B.dcode, B.dict,
		                                      (const double2*)B.cdict, B.dval, A.rowptr, A.col, (const double2*)A.val, (int*)d_bad.p + 1);
	else
	k_pb_csr_verify<<<nbr, 256, 0, st>>>(n_up, n_blk, pitch, B.t_ptr, B.t_col, B.t_val, B.c_ptr, B.c_col, B.c_code, B.blockbase, B.dcode, B.dict, B.dval, A.rowptr, A.col,
	                                    (const double*)A.val, (int*)d_bad.p + 1, B.inv);
	HIP_TRY(hipMemcpyAsync(bad, d_bad.p, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	if (bad[1] || B.nnz != A.nnz) return LPP_OK; // some row is not what (T, C, D) say: not a product-basis matrix (the guard drops the layout)
	*done = true;
	return LPP_OK;
}

// ---- one block: the S = 1/2 Heisenberg chain ------------------------------------------------------------------------------
lpp_status pb_chain(lpp_engine* e, const AsmParams& P, int L, int n, const std::vector<double>& hv, bool* done)
{
	*done = false;
	if (e->is_complex || P.nloc <= 0 || P.model != ASM_HEISENBERG) return LPP_OK;
	const LayoutGate gate = layout_gate(e, "LPP_PRODUCT_LAYOUT", true); // (the extra switch: inherited as found)
	if (gate == LayoutGate::Never) return LPP_OK;
	const int64_t n_up = P.nloc, pitch = pb_pitch_for(n_up);
	if (gate == LayoutGate::BySize && (size_t)n_up * sizeof(double) < ((size_t)32 << 20)) return LPP_OK; // as for the Hubbard matrices (assemble_hubbard_pb)
	if (getenv("LPP_PB_SEG") && atoi(getenv("LPP_PB_SEG")) == 0) return LPP_OK;
	if ((size_t)(pitch + kPbZeroSlots) * sizeof(double) <= (size_t)156 * 1024 && !getenv("LPP_PB_PIECE_ROWS")) return LPP_OK; // a row that fits one LDS window: the general layout's window kernel
	int wcap = 8128;
	if (const char* s = getenv("LPP_PB_PIECE_ROWS")) wcap = (int)std::max<int64_t>(64, std::min<int64_t>(atoll(s), 8128));
	std::vector<int64_t> cnt((size_t)L * L, 0);
	for (size_t k = 0; k < cnt.size(); k++) cnt[k] = hv[k] != 0.0 ? 1 : 0;
	SegPlan SP;
	bool ok = false;
	lpp_status rc = pb_seg_plan_model(L, n, hv, cnt, wcap, SP, &ok, true);
	if (rc != LPP_OK) return rc;
	if (getenv("LPP_VERBOSE"))
		fprintf(stderr, "lpp: chain as one block of the segmented form %s (L = %d, n = %d, %d high sites, %zu segments, %zu items of <= %d positions, <= %d + %d hops per segment)\n",
		        ok ? "planned" : "does not apply", SP.L, SP.n, SP.s, SP.segs.size(), SP.items.size(), SP.wmax, SP.max_cross, SP.max_hh);
	if (!ok || SP.n_up != n_up || inst_index(kPbSegShapes, PbSegShape { SP.nc_pad, SP.nh_pad, 1 }) < 0) return LPP_OK; // (an instance with one block per workgroup)
	hipStream_t st = e->stream;
	DevBuf d_dval, d_len, d_sum, d_y, d_x, d_ys, d_xs;
	// D: the diagonal of every row straight from the state (the assembler's diag_of: Heisenberg.h:251-275 in the reference's loop order),
	// in the basis order; and the number of entries of the CSR this stands for (the assembler's counting pass)
	const size_t loc = (size_t)pitch;
	HIP_TRY_MEM(hipMalloc(&d_dval.p, sizeof(double) * loc));
	HIP_TRY(hipMemsetAsync(d_dval.p, 0, sizeof(double) * loc, st));
	const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>((n_up + 255) / 256, 1 << 16));
	k_pb_diag_values<ASM_HEISENBERG><<<nbr, kBlock, 0, st>>>(P, pitch, (double*)d_dval.p);
	HIP_TRY_MEM(hipMalloc(&d_len.p, sizeof(int64_t) * (size_t)n_up));
	HIP_TRY_MEM(hipMalloc(&d_sum.p, sizeof(unsigned long long)));
	HIP_TRY(hipMemsetAsync(d_sum.p, 0, sizeof(unsigned long long), st));
	k_asm_count<ASM_HEISENBERG><<<nbr, kBlock, 0, st>>>(P, (int64_t*)d_len.p);
	sum_i64(st, (const int64_t*)d_len.p, n_up, (unsigned long long*)d_sum.p);
	DictTable table;
	if ((rc = table.init(st)) != LPP_OK) return rc;
	k_dict_collect<<<2048, kBlock, 0, st>>>((const double*)d_dval.p, (int64_t)loc, table.dev(), table.dev_overflow());
	unsigned long long nnz = 0;
	if ((rc = table.fetch(st)) != LPP_OK) return rc;
	HIP_TRY(hipMemcpyAsync(&nnz, d_sum.p, sizeof(nnz), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	(void)hipFree(d_len.p);
	d_len.p = nullptr;
	const PbDict D = pb_diag_dict(table, false); // (LPP_PB_PLAIN_DIAG is not honoured here: inherited as found; at most 251 keys, so it always applies)
	const int64_t c_rp[2] = { 0, 0 };
	PbBuildInput in;
	in.n_up = n_up;
	in.n_blk = 1;
	in.c_rp = c_rp;
	in.dict256 = D.dict.data();
	in.ndict = D.ndict;
	in.pre = &SP;
	in.pre_nnz = (int64_t)nnz;
	rc = pb_build(e, in);
	if (rc == LPP_ERR_INVALID || rc == LPP_ERR_NOMEM) {
		if (getenv("LPP_VERBOSE")) fprintf(stderr, "lpp: the chain keeps the general layout: %s\n", lpp_last_error());
		free_pb(e);
		return LPP_OK;
	}
	if (rc != LPP_OK) return rc;
	PbState& B = e->pb;
	DropUnlessDone undo { e, done, free_pb }; // until the check below has passed the engine must not describe a product-basis matrix
	// the diagonal into the stored order of the positions (pb.u is free until the first product)
	k_pb_permute<true><<<nbr, 256, 0, st>>>(B.u, (const double*)d_dval.p, B.perm, 1, n_up, pitch);
	HIP_TRY(hipMemcpyAsync(d_dval.p, B.u, sizeof(double) * loc, hipMemcpyDeviceToDevice, st));
	if (D.plain_diag) {
		B.dval = (double*)d_dval.p; // the codes stay 0 (+0.0)
		d_dval.p = nullptr;
	} else
		k_pb_codes_from_values<<<nbr, 256, 0, st>>>((int64_t)loc, (const double*)d_dval.p, B.dict, B.ndict, B.dcode);
	// the layout against the model: one product of a random vector through it and through the assembler's row walk (every entry re-derived
	// per row from the term list, in the reference's order), element by element
	HIP_TRY_MEM(hipMalloc(&d_y.p, sizeof(double) * loc));
	HIP_TRY_MEM(hipMalloc(&d_x.p, sizeof(double) * loc));
	HIP_TRY_MEM(hipMalloc(&d_ys.p, sizeof(double) * loc));
	HIP_TRY_MEM(hipMalloc(&d_xs.p, sizeof(double) * loc));
	HIP_TRY(hipMemsetAsync(d_y.p, 0, sizeof(double) * loc, st));
	HIP_TRY(hipMemsetAsync(d_x.p, 0, sizeof(double) * loc, st));
	HIP_TRY(hipMemsetAsync(d_xs.p, 0, sizeof(double) * loc, st));
	k_fill_random<<<1024, 256, 0, st>>>((double*)d_y.p, n_up, 0, 4711);
	k_asm_apply<ASM_HEISENBERG, double, false><<<nbr, kBlock, 0, st>>>(P, (const double*)d_y.p, (double*)d_x.p, nullptr, EpiScale { nullptr, nullptr, 0 });
	k_pb_permute<true><<<nbr, 256, 0, st>>>((double*)d_ys.p, (const double*)d_y.p, B.perm, 1, n_up, pitch);
	B.active = true; // (pb_launch reads the state; the guard above drops it again if the check fails)
	e->pitch = pitch;
	pb_launch(e, d_ys.p, d_xs.p, nullptr); // x += H y on a zeroed x
	k_pb_permute<false><<<nbr, 256, 0, st>>>((double*)d_y.p, (const double*)d_xs.p, B.perm, 1, n_up, pitch); // back into the basis order (d_y is free now)
	bool same = false;
	double dmax = 0.0, xmax = 0.0;
	if ((rc = row_walk_compare(e, n_up, (const double*)d_y.p, (const double*)d_x.p, &same, &dmax, &xmax)) != LPP_OK) return rc;
	if (getenv("LPP_VERBOSE")) fprintf(stderr, "lpp: chain layout against the assembler's row walk: largest difference %.3g of %.3g\n", dmax, xmax);
	if (!same) return LPP_OK; // not the same matrix: the general layout (the guard drops this one)
	B.chain_model = true; // (the caller records the model: lpp_engine_get_csr re-runs the assembler from it)
	*done = true;
	return LPP_OK;
}

lpp_status pb_get_csr(lpp_engine* e, int64_t* rowptr, int32_t* colind, void* values)
{
	const PbState& B = e->pb;
	const int64_t n = (B.cplx ? B.n_c : B.n_up) * B.n_blk;
	const size_t vsz = B.cplx ? 2 * sizeof(double) : sizeof(double);
	DevBuf drp, dci, dva;
	if (rowptr) HIP_TRY_MEM(hipMalloc(&drp.p, sizeof(int64_t) * (size_t)(n + 1)));
	if (colind || values) {
		HIP_TRY_MEM(hipMalloc(&dci.p, sizeof(int32_t) * (size_t)std::max<int64_t>(B.nnz, 1)));
		HIP_TRY_MEM(hipMalloc(&dva.p, vsz * (size_t)std::max<int64_t>(B.nnz, 1)));
	}
	if (B.cplx)
		k_pb_rebuild_c<<<(int)((n + 255) / 256), 256, 0, e->stream>>>(B.n_c, B.n_blk, B.pitch, B.t_ptr, B.t_col, (const double2*)B.t_val, B.c_ptr, B.c_col, B.c_code,
		                                                             B.blockbase, B.dcode, B.dict, (const double2*)B.cdict, (int64_t*)drp.p, (int32_t*)dci.p, (double2*)dva.p, B.dval);
	else
	k_pb_rebuild<<<(int)((n + 255) / 256), 256, 0, e->stream>>>(B.n_up, B.n_blk, B.pitch, B.t_ptr, B.t_col, B.t_val, B.c_ptr, B.c_col, B.c_code, B.blockbase,
	                                                           B.dcode, B.dict, (int64_t*)drp.p, (int32_t*)dci.p, (double*)dva.p, B.dval, B.inv);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (rowptr) HIP_TRY(hipMemcpy(rowptr, drp.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
	if (colind) HIP_TRY(hipMemcpy(colind, dci.p, sizeof(int32_t) * (size_t)B.nnz, hipMemcpyDeviceToHost));
	if (values) HIP_TRY(hipMemcpy(values, dva.p, vsz * (size_t)B.nnz, hipMemcpyDeviceToHost));
	return LPP_OK;
}

// ---- vector copies that know the pitched layout ------------------------------------------------
// basis order (`src` / `dst`: host or device memory, as `kind` says) <-> the internal pitched / permuted form (`dev`)
static lpp_status vec_in(lpp_engine* e, double* dev, const void* src, hipMemcpyKind kind)
{
	if (e->pitch > 0) {
		const PbState& B = e->pb;
		// stored order of the positions (PbState::perm): the copy lands in pb.u in the basis order and is gathered from there
		double* const land = B.perm ? B.u : dev;
		HIP_TRY(hipMemsetAsync(land, 0, sizeof(double) * (size_t)e->nd_pad, e->stream));
		HIP_TRY(hipMemcpy2DAsync(land, e->esz * (size_t)e->pitch, src, e->esz * (size_t)e->pitch_rows, e->esz * (size_t)e->pitch_rows, (size_t)e->pitch_blocks, kind, e->stream));
		if (B.perm) {
			k_pb_permute<true><<<2048, 256, 0, e->stream>>>(dev, land, B.perm, e->pitch_blocks, e->pitch_rows, e->pitch);
			HIP_TRY(hipGetLastError());
		}
		return LPP_OK;
	}
	HIP_TRY(hipMemcpyAsync(dev, src, e->esz * (size_t)e->n_local, kind, e->stream));
	return LPP_OK;
}

static lpp_status vec_out(lpp_engine* e, void* dst, const double* dev, hipMemcpyKind kind)
{
	if (e->pitch > 0) {
		const PbState& B = e->pb;
		const double* from = dev;
		if (B.perm) { // back into the basis order, through pb.u (free between products)
			k_pb_permute<false><<<2048, 256, 0, e->stream>>>(B.u, dev, B.perm, e->pitch_blocks, e->pitch_rows, e->pitch);
			HIP_TRY(hipGetLastError());
			from = B.u;
		}
		HIP_TRY(hipMemcpy2DAsync(dst, e->esz * (size_t)e->pitch_rows, from, e->esz * (size_t)e->pitch, e->esz * (size_t)e->pitch_rows, (size_t)e->pitch_blocks, kind, e->stream));
		return LPP_OK;
	}
	HIP_TRY(hipMemcpyAsync(dst, dev, e->esz * (size_t)e->n_local, kind, e->stream));
	return LPP_OK;
}

// the hole-major t-J layout has copies of its own (through its permutation).  Which public entry points hand a device vector to a hole-major
// engine is decided by their callers (begin_run, lanczos_impl), not here.
lpp_status vec_from_host(lpp_engine* e, double* dev, const void* host) { return e->tj.active ? tj_vec_from_host(e, dev, host) : vec_in(e, dev, host, hipMemcpyHostToDevice); }
lpp_status vec_to_host(lpp_engine* e, void* host, const double* dev) { return e->tj.active ? tj_vec_to_host(e, host, dev) : vec_out(e, host, dev, hipMemcpyDeviceToHost); }
lpp_status vec_from_device(lpp_engine* e, double* dev, const void* basis)
{
	return e->tj.active ? tj_vec_from_device(e, dev, basis) : vec_in(e, dev, basis, hipMemcpyDeviceToDevice);
}
lpp_status vec_to_device(lpp_engine* e, void* basis, const double* dev)
{
	return e->tj.active ? tj_vec_to_device(e, basis, dev) : vec_out(e, basis, dev, hipMemcpyDeviceToDevice);
}

void vec_fill_random(lpp_engine* e, double* dev, uint64_t seed)
{
	if (e->tj.active) {
		tj_fill_random(e, dev, seed);
		return;
	}
	if (e->pitch > 0) {
		if (e->pb.cplx) // complex elements: the stream is indexed by doubles (2 per element), rows and pitch counted in doubles
			k_fill_random_pitched<<<1024, 256, 0, e->stream>>>(dev, e->pitch_blocks, e->pb.n_up, e->pb.pitch, e->row_start * 2, seed, nullptr);
		else
			k_fill_random_pitched<<<1024, 256, 0, e->stream>>>(dev, e->pitch_blocks, e->pitch_rows, e->pitch, e->row_start, seed, e->pb.perm);
		return;
	}
	if (e->nd > 0) k_fill_random<<<1024, 256, 0, e->stream>>>(dev, e->nd, e->row_start * (e->is_complex ? 2 : 1), seed);
}

} // namespace lpp
