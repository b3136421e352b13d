// lpp_pb_instances.h -- which template instances of the product-basis kernels exist, in plain C++.  One list per kernel: the launch code
// (lpp_pb.hip) instantiates exactly the entries of a list and finds its kernel by index, the planner (lpp_pb_plan.cpp, lpp_pbseg_host.cpp)
// chooses among them and refuses a form whose key is missing.  A new instance is added HERE, as one more entry, and nowhere else.
// Keys are strict: a key function carries the form's own values, never the nearest instance.
#pragma once
#include <stddef.h>

#include <array>

#include "lpp_pb_plan.h"

namespace lpp {

// position of `key` in `list`, -1 when it has no such instance
template <typename K, size_t N> constexpr int inst_index(const std::array<K, N>& list, const K& key)
{
	for (size_t i = 0; i < N; i++)
		if (list[i] == key) return (int)i;
	return -1;
}
// lists[i] x tails[j] through `join`, i-major (every list below is such a product)
template <typename K, typename A, size_t NA, typename B, size_t NB, typename J>
constexpr std::array<K, NA * NB> inst_product(const std::array<A, NA>& heads, const std::array<B, NB>& tails, J join)
{
	std::array<K, NA * NB> l {};
	for (size_t i = 0; i < NA; i++)
		for (size_t j = 0; j < NB; j++) l[i * NB + j] = join(heads[i], tails[j]);
	return l;
}
struct InstDepth { // value groups unrolled (0: any number, by a loop) and the look-ahead depth that goes with them
	int gt, pre;
	constexpr bool operator==(const InstDepth& o) const { return gt == o.gt && pre == o.pre; }
};

// ---- k_pb_up<DOT, GT, CHAIN, PRE0>: 3 x 5 = 15 ----------------------------------------------------------------------------------------
constexpr int kPreLo = kPbPairs ? 2 : 3, kPreHi = kPbPairs ? 6 : 5; // the unequal look-ahead splits of two value groups
struct PbUpInst {
	bool dot, chain;
	int gt, pre0;
	constexpr bool operator==(const PbUpInst& o) const { return dot == o.dot && chain == o.chain && gt == o.gt && pre0 == o.pre0; }
};
struct PbUpMode { // (the chained step forms its sums in the coupling kernel: no chained form with the dot)
	bool dot, chain;
};
constexpr std::array<PbUpMode, 3> kPbUpModes = { { { false, false }, { true, false }, { false, true } } };
constexpr std::array<InstDepth, 5> kPbUpDepths = { { { 1, kPbPre }, { 2, kPreLo }, { 2, kPbPre }, { 2, kPreHi }, { 0, kPbPre } } };
constexpr std::array<PbUpInst, 15> kPbUpInsts =
    inst_product<PbUpInst>(kPbUpModes, kPbUpDepths, [](const PbUpMode& m, const InstDepth& d) { return PbUpInst { m.dot, m.chain, d.gt, d.pre }; });

// ---- k_pb_up_big<DOT, GT, PRE>: 2 x 4 = 8; k_pb_up_big2<DOT, GT, PRE0>: 2 x 5 = 10 ----------------------------------------------------
constexpr int kPbBigPre = 4; // (= kBigPre of lpp_pbig_kernels.h; lpp_pb.hip asserts it)
struct PbBigInst {
	bool dot;
	int gt, pre;
	constexpr bool operator==(const PbBigInst& o) const { return dot == o.dot && gt == o.gt && pre == o.pre; }
};
constexpr std::array<bool, 2> kInstDots = { { false, true } };
constexpr PbBigInst big_inst_of(const bool& dot, const InstDepth& d) { return PbBigInst { dot, d.gt, d.pre }; }
constexpr std::array<InstDepth, 4> kPbBigDepths = { { { 1, kPbBigPre }, { 2, kPbBigPre }, { 4, 3 }, { 0, kPbBigPre } } };
constexpr std::array<PbBigInst, 8> kPbBigInsts = inst_product<PbBigInst>(kInstDots, kPbBigDepths, big_inst_of);
// (four groups: two chunks of each ahead, three spill)
constexpr std::array<InstDepth, 5> kPbBig2Depths = { { { 1, 4 }, { 4, 2 }, { 2, 3 }, { 2, 4 }, { 2, 5 } } };
constexpr std::array<PbBigInst, 10> kPbBig2Insts = inst_product<PbBigInst>(kInstDots, kPbBig2Depths, big_inst_of);

// ---- k_pb_up_seg<DOT, GT, P0, 4, NC, NH, ROWS>: 2 x 3 x 8 = 48 ------------------------------------------------------------------------
struct PbSegShape { // pairs of cross hops / high-high hops every segment's lists are padded to, blocks per workgroup
	int nc, nh, rows;
	constexpr bool operator==(const PbSegShape& o) const { return nc == o.nc && nh == o.nh && rows == o.rows; }
};
struct PbSegInst {
	bool dot;
	int gt, p0;
	PbSegShape shape;
	constexpr bool operator==(const PbSegInst& o) const { return dot == o.dot && gt == o.gt && p0 == o.p0 && shape == o.shape; }
};
// in the order the planner tries them (pb_seg_shape_for): two blocks per workgroup; one block (chains: one low neighbour per high site)
constexpr std::array<PbSegShape, 8> kPbSegShapes = { { { 2, 2, 2 }, { 5, 4, 2 }, { 6, 8, 2 }, { 2, 2, 1 }, { 1, 12, 1 }, { 1, 16, 1 }, { 2, 12, 1 }, { 2, 16, 1 } } };
constexpr std::array<InstDepth, 3> kPbSegDepths = { { { 1, 4 }, { 2, 2 }, { 2, 4 } } };
struct PbSegMode {
	bool dot;
	InstDepth d;
};
constexpr std::array<PbSegMode, 6> kPbSegModes = inst_product<PbSegMode>(kInstDots, kPbSegDepths, [](const bool& dot, const InstDepth& d) { return PbSegMode { dot, d }; });
constexpr std::array<PbSegInst, 48> kPbSegInsts =
    inst_product<PbSegInst>(kPbSegModes, kPbSegShapes, [](const PbSegMode& m, const PbSegShape& s) { return PbSegInst { m.dot, m.d.gt, m.d.pre, s }; });
// the first listed shape of `rows` blocks per workgroup that holds max_cross pairs of cross hops and max_hh high-high hops; null: none does
inline const PbSegShape* pb_seg_shape_for(int max_cross, int max_hh, int rows)
{
	for (const PbSegShape& s : kPbSegShapes)
		if (s.rows == rows && max_cross <= s.nc && max_hh <= s.nh) return &s;
	return nullptr;
}

// ---- k_pb_down<1024, RMW, WIDE, CPLX, PF>: 8 + 4 = 12 -----------------------------------------------------------------------------------
struct PbDownInst {
	bool rmw, wide, cplx, pf;
	constexpr bool operator==(const PbDownInst& o) const { return rmw == o.rmw && wide == o.wide && cplx == o.cplx && pf == o.pf; }
};
struct PbDownMode { // (the chained step has no form with 64-bit addresses)
	bool rmw, wide;
};
struct PbDownKind {
	bool cplx, pf;
};
constexpr std::array<PbDownMode, 3> kPbDownModes = { { { false, false }, { false, true }, { true, false } } };
constexpr std::array<PbDownKind, 4> kPbDownKinds = { { { false, false }, { false, true }, { true, false }, { true, true } } };
constexpr std::array<PbDownInst, 12> kPbDownInsts =
    inst_product<PbDownInst>(kPbDownModes, kPbDownKinds, [](const PbDownMode& m, const PbDownKind& k) { return PbDownInst { m.rmw, m.wide, k.cplx, k.pf }; });

// ---- k_pb_down_parts<kPbPartsThreads, R>: 6 ---------------------------------------------------------------------------------------------
struct PbPartsInst {
	int r; // rounds of tasks whose sums a wave keeps in registers
	constexpr bool operator==(const PbPartsInst& o) const { return r == o.r; }
};
constexpr std::array<PbPartsInst, 6> kPbPartsInsts = { { { 4 }, { 8 }, { 12 }, { 16 }, { 20 }, { 24 } } };

// ---- keys from the planned form ---------------------------------------------------------------------------------------------------------
// one or two value groups are unrolled, any other number (complex hoppings realified, t-t' models; none at all) runs the loop over groups;
// only two groups split the look-ahead
inline PbUpInst pb_up_inst(const PbForm& B, bool dot, bool chain)
{
	const int gt = B.G == 1 || B.G == 2 ? B.G : 0;
	return { dot, chain, gt, gt == 2 ? B.pre0 : kPbPre };
}
inline PbBigInst pb_big_inst(const PbForm& B, bool dot) // ... here four groups (complex hoppings) are unrolled too, three chunks ahead
{
	const int gt = B.G == 1 || B.G == 2 || B.G == 4 ? B.G : 0;
	return { dot, gt, gt == 4 ? 3 : kPbBigPre };
}
inline PbBigInst pb_big2_inst(const PbForm& B, bool dot) { return { dot, B.G, B.G == 2 ? B.pre0 : B.G == 4 ? 2 : 4 }; }
inline PbSegInst pb_seg_inst(const PbForm& B, bool dot) { return { dot, B.G, B.seg_pre0, { B.seg_nc, B.seg_nh, B.seg_one ? 1 : 2 } }; }
// plain: the tasks by the LDS counter where down_tasks says so; chained (rmw): where down_pf does
inline PbDownInst pb_down_inst(const PbForm& B, bool rmw) { return { rmw, B.wide, B.cplx, rmw ? B.down_pf : B.down_tasks }; }
inline PbPartsInst pb_parts_inst(const PbForm& B) { return { B.maxr }; }

// the look-ahead depths of value group 0 that the two-group instances of the form's in-block kernel have (k_pb_up, or k_pb_up_big2 by pieces)
template <typename F> void pb_for_each_pre0(bool big, F&& f)
{
	for (const InstDepth& d : kPbUpDepths)
		if (!big && d.gt == 2) f(d.pre);
	for (const InstDepth& d : kPbBig2Depths)
		if (big && d.gt == 2) f(d.pre);
}
// ... and the one LPP_PB_PRE0 = v stands for: the deepest that does not exceed it, or the shallowest
inline int pb_listed_pre0(bool big, int v)
{
	int lo = -1, at = -1;
	pb_for_each_pre0(big, [&](int p) {
		if (lo < 0 || p < lo) lo = p;
		if (p <= v && p > at) at = p;
	});
	return at >= 0 ? at : lo;
}

} // namespace lpp
