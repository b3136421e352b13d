// lpp_pb_geom.h -- the constants and LDS size formulas of the product-basis layout that both the kernels (lpp_pb_kernels.h,
// lpp_pbig_kernels.h, lpp_pbseg_kernels.h) and the host planning (lpp_pb_plan.h, lpp_host.cpp) need.  No HIP: plain C++ reads the same
// definitions as the device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lpp_pbseg.h"

namespace lpp {

constexpr int kPbMaxGroups = 8; // distinct off-diagonal values of the in-block matrix
constexpr int kPbZeroSlots = 32; // zero-valued window elements behind the row (one per LDS bank) that padding entries read
constexpr int kPbUpThreads = 1024;
// rows (positions per block) from which the layout is admitted: by itself, and for an uploaded CSR (pb_from_csr) / when
// LPP_PRODUCT_LAYOUT forces it on a device-assembled Hubbard matrix (one slice of 64 rows: small sectors exist to exercise the
// kernels' edges -- waves without a slice, a single panel --, not to be fast)
constexpr int kPbMinRows = 512, kPbMinRowsForced = 64;
constexpr int kPbPre = 4; // chunks (of 4 slots) of every (slice, group) requested one slice ahead
#ifndef LPP_PB_PAIRS
#define LPP_PB_PAIRS 1
#endif
constexpr bool kPbPairs = LPP_PB_PAIRS != 0;
// look-ahead depth of value group g (two groups share 8 chunks as PRE0 + (8 - PRE0); with pairs PRE0 = 6 leaves group 1 four)
LPP_PB_HD constexpr int pb_depth(int GG, int g, int PRE0) { return GG == 2 ? (g == 0 ? PRE0 : (kPbPairs && PRE0 >= 6 ? 4 : 2 * kPbPre - PRE0)) : kPbPre; }

// what a kernel may ask of a CU's 160 KB of LDS: the in-block kernels take all but 64 bytes, the coupling kernels' images 150 KB
constexpr size_t kPbUpLdsMax = 160 * 1024 - 64;
constexpr size_t kPbDownLdsMax = 150 * 1024;

// vectors are PITCHED: a block's row is rounded up to a multiple of 16 positions (one 128-byte line)
inline int64_t pb_pitch_for(int64_t n_up) { return (n_up + 15) & ~(int64_t)15; }

// k_pb_up.  LDS layout (all dynamic, so that the window starts at LDS address 0 and a template word IS the address):
//   [0, (pitch+32)*8) window + zero slots | dcode_s[pitch] | off_s[spb*G] | len_s[spb*G] | dict_s[256] | smem[16] | (pad)
LPP_PB_HD inline size_t pb_up_meta_offset(int64_t pitch) { return sizeof(double) * (size_t)(pitch + kPbZeroSlots) + (size_t)pitch; }
LPP_PB_HD inline size_t pb_up_dict_offset(int64_t pitch, int spb, int G) { return (pb_up_meta_offset(pitch) + (size_t)spb * (size_t)G * 6 + 15) & ~(size_t)15; }
LPP_PB_HD inline size_t pb_up_lds_bytes(int64_t pitch, int spb, int G)
{
	return pb_up_dict_offset(pitch, spb, G) + 256 * sizeof(double) + (kPbUpThreads / 64) * sizeof(double) + 16;
}

// LDS image of k_pb_down: one 32-bit word per place of a block's coupling list (source block | value code << 24), rows of
// `stride` words.  A lane reads the 4 places of a chunk with ONE 16-byte LDS read (the 8 blocks of a task sit `stride` words
// apart: stride / 4 odd puts their 16-byte segments on different bank groups); separate 2-byte index and 1-byte code arrays
// cost 8 LDS instructions per chunk instead, and the LDS pipeline was what the kernel's instruction skeleton waited for
// (0.8 of its 0.875 ms at config 2: scripts/experiments/r03_down_parts_ab.sh).
LPP_PB_HD inline int pb_down_stride(int rowcap) { return ((rowcap >> 2) & 1) ? rowcap : rowcap + 4; }
LPP_PB_HD inline size_t pb_down_lds_bytes(int ids_per_wg, int rowcap) { return (((size_t)ids_per_wg * 8 + 15) & ~(size_t)15) + (size_t)ids_per_wg * (size_t)pb_down_stride(rowcap) * 4 + 16; }
// the PF form's task sums behind the image in k_pb_down's dynamic LDS: two buffers of (Re<y|z>, |z - s y|^2) per task of 8 blocks
LPP_PB_HD inline size_t pb_down_task_sum_bytes(int ids_per_wg) { return (size_t)((ids_per_wg + 7) / 8) * 4 * sizeof(double); }

constexpr int kPbMaxParts = 8;
constexpr int kPbBigThreads = 512;
// the coupling kernel keeps one double2 per task round and lane for the whole panel: 512 threads (8 waves, up to 256 registers
// each) per CU rather than 1024 with 128 -- ten rounds of sums, two chunks of gathers and the addresses spill at 128
constexpr int kPbPartsThreads = 512;
constexpr int kPbBig2Threads = 1024;

// k_pb_up_big.  LDS: window (W + 32 zero slots) | dcode[W] | dict[256] | gval[9] | smem[THREADS/64]
LPP_PB_HD inline size_t pb_big_lds_bytes(int W)
{
	return ((sizeof(double) * (size_t)(W + kPbZeroSlots) + (size_t)W + 15) & ~(size_t)15) + sizeof(double) * (256 + kPbMaxGroups + 1 + kPbBigThreads / 64) + 16;
}
// k_pb_up_big2: the windows of two blocks
LPP_PB_HD inline size_t pb_big2_lds_bytes(int W)
{
	return ((2 * sizeof(double) * (size_t)(W + kPbZeroSlots) + 2 * (size_t)W + 15) & ~(size_t)15) + sizeof(double) * (256 + kPbMaxGroups + 1 + kPbBig2Threads / 64) + 16;
}
// k_pb_down_parts.  LDS image of a workgroup's coupling lists, compact (a padded image -- every part of every list as long as the longest --
// is 170 KB at N_dn = 38760 in four parts; this one 82 KB): line[ids] | pstart[ids][NH+1] (places) | n4[tasks][NH] | idx[ent] | code[ent]
LPP_PB_HD inline size_t pb_parts_lds_bytes(int ids_per_wg, int ent_cap, int nparts)
{
	const size_t ngroups = (size_t)(ids_per_wg + 7) / 8;
	return (size_t)ids_per_wg * (4 + 2 * ((size_t)nparts + 1)) + ((ngroups * (size_t)nparts + 1) & ~(size_t)1) + (size_t)(ent_cap + 8) * 3 + 64;
}

constexpr int kSegThreads = 512; // 8 waves of up to 256 registers: two slices' loads from the rows in flight per wave
// k_pb_up_seg.  LDS: [0, 2 ws) windows | dcode[2][wmax + 32] | 2 x slice heads[160] | 2 x cross[16 * 6] | 2 x hh[16 * 12] | dict[256] | smem[8] | per wave 64 x 2 doubles (high-high sums)
LPP_PB_HD inline size_t pb_seg_dcode_stride(int wmax) { return ((size_t)wmax + 32 + 15) & ~(size_t)15; }
LPP_PB_HD inline size_t pb_seg_tab_offset(int ws, int wmax) { return (2 * sizeof(double) * (size_t)ws + 2 * pb_seg_dcode_stride(wmax) + 15) & ~(size_t)15; }
// (rows: blocks per workgroup; one block per workgroup alternates between TWO sets of tables)
LPP_PB_HD inline size_t pb_seg_lds_bytes(int ws, int wmax, int rows)
{
	return pb_seg_tab_offset(ws, wmax) + (rows == 1 ? 2 : 1) * (sizeof(SegSlice) * kSegMaxSlices + sizeof(SegCross) * kSegMaxSegs * kSegMaxCross + sizeof(SegHh) * kSegMaxSegs * pb_seg_hh_cap(rows)) + sizeof(double) * (256 + kSegThreads / 64 + 2 * kSegThreads) + 16;
}

} // namespace lpp
