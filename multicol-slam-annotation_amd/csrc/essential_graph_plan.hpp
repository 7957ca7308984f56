// The plan of the block-sparse LDL^T of the essential graph (include/mcs_essgraph.h, the
// mcs_essgraph_plan entries): the layout the host planner (essential_graph_plan.cpp) writes and the
// device kernels (essential_graph_sparse.hpp) and the host program of the tests read.
//
// The matrix is the 7 (N - 1) system over the free keyframes in B x B blocks (B = 7 here, a
// template parameter of the numeric code).  The planner orders the free keyframes by nested
// dissection; every separator and every leaf is one supernode: a run of consecutive columns of the
// permuted matrix that share one row list.  A supernode's numbers are a dense panel, row-major,
// (B nr) x (B ns): ns own block columns, nr block rows = its own ns (the triangle above the
// diagonal is never read) and then the rows below, ascending.  The row lists are closed under
// elimination, so the union of the panels is the pattern of L.
//
// A target panel is updated from its sources: the descendant supernodes that have a row in the
// target's columns, in ascending order, each through a map from the source's rows to the target's.
// Levels are heights in the supernodal tree; supernodes of one level share no dependency.
//
// No HIP include: __host__ __device__ under hipcc, inline under a host compiler.
#pragma once
#include "lm_control.hpp"
#include <stdint.h>
#include <string>
#include <vector>

namespace mcs {
namespace esg {

// What the numeric code reads; on the device every pointer is device memory.
struct SpView {
  int n;                  // free keyframes (block rows)
  int S;                  // supernodes
  const int32_t* perm;    // [n] free keyframe -> column of the permuted matrix
  const int32_t* iperm;   // [n] column -> free keyframe
  const int32_t* sn_of;   // [n] column -> supernode
  const int32_t* col0;    // [S + 1] first column
  const int32_t* rowptr;  // [S + 1] into rows
  const int32_t* rows;    // block rows (columns of the permuted matrix), per supernode ascending
  const int32_t* blkoff;  // [S + 1] first block of the panel; the panel starts at B B blkoff doubles
  const int32_t* srcptr;  // [S + 1] into the source lists
  const int32_t* src_s;   // the source supernode
  const int32_t* src_p0;  // its rows [p0, p1) lie in the target's columns, [p0, nr) in its rows
  const int32_t* src_p1;
  const int32_t* src_map; // relmap + src_map[k]: position in the target's rows of source row p0 + i
  const int32_t* relmap;
  const int32_t* lvlptr;  // [levels + 1] into lvlsn
  const int32_t* lvlsn;   // supernodes by level, ascending inside a level
  const uint8_t* ablk;    // per panel block: 1 = a block of A (a planned pair or a diagonal)
};

// position of block row i in the row list of column j's supernode, i >= j, or -1 outside the pattern
MCS_LM_FN int find_pos(const SpView& v, int i, int j) {
  const int s = v.sn_of[j], c0 = v.col0[s], ns = v.col0[s + 1] - c0;
  if (i < c0 + ns) return i - c0;
  const int32_t* rows = v.rows + v.rowptr[s];
  int lo = ns, hi = v.rowptr[s + 1] - v.rowptr[s];
  const int nr = hi;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (rows[m] < i) lo = m + 1; else hi = m;
  }
  return (lo < nr && rows[lo] == i) ? lo : -1;
}

// block index (into ablk) of (row i, column j) of the permuted matrix, i >= j, or -1
MCS_LM_FN int find_block(const SpView& v, int i, int j) {
  const int pos = find_pos(v, i, j), s = v.sn_of[j];
  return pos < 0 ? -1 : v.blkoff[s] + pos * (v.col0[s + 1] - v.col0[s]) + (j - v.col0[s]);
}

// offset in doubles of entry (0, 0) of block (i, j), i >= j, with the panel's row stride, or -1
MCS_LM_FN int64_t block_entry(const SpView& v, int B, int i, int j, int* stride) {
  const int pos = find_pos(v, i, j), s = v.sn_of[j], W = B * (v.col0[s + 1] - v.col0[s]);
  *stride = W;
  return pos < 0 ? -1 : (int64_t)B * B * v.blkoff[s] + (int64_t)B * pos * W + B * (j - v.col0[s]);
}

// Limits, from arithmetic on counts: every index is an int32 and one copy of the pattern of L
// holds at most kPlanMaxBytes (three copies live on the device: the assembled A0, A / L, and the
// transposed rows of L the updates read).
constexpr int64_t kPlanMaxBytes = (int64_t)1 << 30;
constexpr int kPlanDefaultLeaf = 4;
constexpr int kPlanFixedLaunches = 6;    // of a trial beside the solver's: linearise, zero, assemble, update, chi2, end

struct SparsePlan {
  int N = 0, loop = 0, n = 0, S = 0, leaf = 0, levels = 0, max_cols = 0;
  std::vector<int32_t> perm, iperm, sn_of, col0, rowptr, rows, blkoff, srcptr, src_s, src_p0, src_p1, src_map, relmap,
      parent, level, lvlptr, lvlsn;
  std::vector<uint8_t> ablk;
  std::vector<int32_t> launch_lo, launch_hi;   // level ranges, one launch each; a range of several levels is
                                               // the chain of single supernodes at the top, one workgroup
  int64_t a_blocks = 0, l_blocks = 0, panel_blocks = 0, flops = 0, row_blocks = 0;
  uint64_t digest = 0;

  SpView view() const {
    SpView v{};
    v.n = n; v.S = S;
    v.perm = perm.data(); v.iperm = iperm.data(); v.sn_of = sn_of.data(); v.col0 = col0.data();
    v.rowptr = rowptr.data(); v.rows = rows.data(); v.blkoff = blkoff.data(); v.srcptr = srcptr.data();
    v.src_s = src_s.data(); v.src_p0 = src_p0.data(); v.src_p1 = src_p1.data(); v.src_map = src_map.data();
    v.relmap = relmap.data(); v.lvlptr = lvlptr.data(); v.lvlsn = lvlsn.data(); v.ablk = ablk.data();
    return v;
  }
};

// 0, or -1 (bad argument) / -4 (above the limits) with the reason in *err.  edges [E][3] as the
// optimiser takes them; an edge of the fixed keyframe adds no block.  leaf <= 0 = kPlanDefaultLeaf.
int plan_build(int n_kf, int loop, const int32_t* edges, int E, int leaf, int block, SparsePlan* out, std::string* err);

}  // namespace esg
}  // namespace mcs
