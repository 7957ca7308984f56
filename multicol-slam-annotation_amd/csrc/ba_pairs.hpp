// Device build of the Schur pair lists and the k_schur work items, and the zeroing of edges
// that leave the active set.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ba_dev.hpp"
#include "ba_structure.hpp"

namespace mcs::ba {
// ---- device build of the Schur pair lists and the k_schur work items ---------------------
// BlockSolver::buildStructure's per-point product of pose groups (block_solver.hpp:143-295),
// in the order build_pairs_host (ba_structure.hpp) produces on the host: per point, groups of
// its edges by active pose in increasing pose order, for every group pair (P1 >= P2) the
// edges of P1 x the edges of P2 in edge order; points in order; then a stable radix sort by
// block id (rocPRIM) makes the lists block-major with that order kept inside every block.

// The pairs of a point are {(a, b) : h(a) >= h(b) >= 0} over its active edges; after the
// stable sort by block id only their order INSIDE a block matters, and there it is (a, b) in
// edge order -- exactly the order of the plain double loop over the point's edges (pt_edges is
// in edge order).  So every (point, edge a) entry counts and emits its own pairs in b order,
// one thread per entry, at the offset the scan over the entries gives it: no per-point sort.
__device__ __forceinline__ void entry_range(const Dev& d, int q, int* q0, int* q1) {
  const int l = d.point_h[d.e_point[d.pt_edges[q]]];
  *q0 = d.pt_ptr[l];
  *q1 = d.pt_ptr[l + 1];
}
__global__ __launch_bounds__(256) void k_pair_count(Dev d, int32_t* cnt) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q > d.npe) return;
  if (q == d.npe) { cnt[q] = 0; return; }   // the scan's total slot
  const int ha = d.pt_h[q];
  int n = 0;
  if (ha >= 0) {
    int q0, q1;
    entry_range(d, q, &q0, &q1);
    for (int b = q0; b < q1; b++) {
      const int hb = d.pt_h[b];
      n += (hb >= 0 && hb <= ha) ? 1 : 0;
    }
  }
  cnt[q] = n;
}

__global__ __launch_bounds__(256) void k_pair_emit(Dev d, const int32_t* off, uint32_t* keys,
                                                   uint2* vals, int64_t pmax, uint32_t pad_key) {
  const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // padding past the last pair: a key above every block, sorted to the end
  const int64_t total = off[d.npe];
  for (int64_t q = total + gt; q < pmax; q += (int64_t)gridDim.x * 256) {
    keys[q] = pad_key;
    vals[q] = make_uint2(0u, 0u);
  }
  const int q = (int)gt;
  if (q >= d.npe) return;
  const int ha = d.pt_h[q];
  if (ha < 0) return;
  int q0, q1;
  entry_range(d, q, &q0, &q1);
  const uint32_t ea = (uint32_t)d.pt_edges[q];
  int64_t o = off[q];
  for (int b = q0; b < q1; b++) {
    const int hb = d.pt_h[b];
    if (hb < 0 || hb > ha) continue;
    keys[o] = (uint32_t)((int64_t)ha * (ha + 1) / 2 + hb);
    vals[o] = make_uint2(ea, (uint32_t)d.pt_edges[b]);
    o++;
  }
}

// pr_ptr[b] = first sorted pair of block >= b (b = 0..nblk; the padding keys are nblk), and
// the block's chunk count (pairs, or on a diagonal block its pose's edges, per kSchurChunk)
__global__ __launch_bounds__(256) void k_block_ptr(Dev d, const uint32_t* keys, int64_t pmax,
                                                   int nblk, int32_t* pr_ptr, int32_t* nch,
                                                   int32_t* nslot) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b > nblk) return;
  auto lb = [&](uint32_t k) {
    int64_t lo = 0, hi = pmax;
    while (lo < hi) {
      const int64_t m = (lo + hi) >> 1;
      if (keys[m] < k) lo = m + 1; else hi = m;
    }
    return lo;
  };
  const int64_t p0 = lb((uint32_t)b);
  pr_ptr[b] = (int32_t)p0;
  if (b == nblk) { nch[b] = 0; nslot[b] = 0; return; }
  const int np_ = (int)(lb((uint32_t)b + 1) - p0);
  const int bi = d.blk_i[b], bj = d.blk_j[b];
  const int ne = (bi == bj) ? d.ps_ptr[bi + 1] - d.ps_ptr[bi] : 0;
  const int n = max(1, (max(np_, ne) + kSchurChunk - 1) / kSchurChunk);
  nch[b] = n;
  nslot[b] = n > 1 ? n : 0;
}

__global__ __launch_bounds__(256) void k_block_items(int nblk, const int32_t* nch,
                                                     const int32_t* it_off, const int32_t* slot_off,
                                                     int32_t* it_blk, int32_t* it_chunk,
                                                     int32_t* it_slot, int32_t* it_nch,
                                                     int32_t* nitem) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == nblk) *nitem = it_off[nblk];
  if (b >= nblk) return;
  const int n = nch[b], i0 = it_off[b];
  for (int c = 0; c < n; c++) {
    it_blk[i0 + c] = b;
    it_chunk[i0 + c] = c;
    it_slot[i0 + c] = n > 1 ? slot_off[b] + c : -1;
    it_nch[i0 + c] = n;
  }
}

// edges that left the active set (LocalBA culling, Optimizer::remask): zero every per-edge term
// a build kernel reads, so their contributions to Hll / b_l / Hpp / b_p / Schur are exact zeros
__device__ __forceinline__ void zero_edge_terms(const Dev& d, int e) {
  d.w[e] = 0.0;
  d.err[2 * e] = 0.0; d.err[2 * e + 1] = 0.0;
  for (int i = 0; i < 12; i++) d.jp[12 * e + i] = 0.0;
  for (int i = 0; i < 6; i++) d.jl[6 * e + i] = 0.0;
  for (int i = 0; i < 18; i++) { d.hpl[18 * e + i] = 0.0; d.y[18 * e + i] = 0.0; }
  if (d.alt_err) {   // both linearisation buffers (a later run may flip to either)
    d.alt_w[e] = 0.0;
    d.alt_err[2 * e] = 0.0; d.alt_err[2 * e + 1] = 0.0;
    for (int i = 0; i < 12; i++) d.alt_jp[12 * e + i] = 0.0;
    for (int i = 0; i < 6; i++) d.alt_jl[6 * e + i] = 0.0;
    for (int i = 0; i < 18; i++) d.alt_hpl[18 * e + i] = 0.0;
  }
}
__global__ __launch_bounds__(256) void k_zero_edges(Dev d, const int32_t* edges, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  zero_edge_terms(d, edges[k]);
}

}  // namespace mcs::ba
