// LocalBA's culling passes on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ba_dev.hpp"
#include "ba_pairs.hpp"

namespace mcs::ba {
// ---- LocalBA's culling on the device (mcs_local_ba_ex) -----------------------------------
// The culling passes of LocalBundleAdjustment (src/cOptimizer.cpp:798-817 after round 1,
// :830-849 after round 2) walk the edges in vpEdges order with per-point state: observations
// left and the bad flag EraseObservation raises below two (src/cMapPoint.cpp:120-152).  A
// point's decisions depend only on its own edges, in edge order, so one thread per active point
// walks its point-CSR list (pt_edges is in edge order and, in round 1, holds every edge of the
// point) and decides exactly as the sequential pass does.  Round 1 also moves the culled edges to
// level 1 and zeroes their per-edge terms (what Optimizer::remask's k_zero_edges does), counts
// the culled edges per pose and the points left, and its last workgroup reports whether an
// active pose lost all its edges (g2o would drop it from the system: the host then rebuilds from
// scratch).  Round 2 keeps round 1's active list; k_edges / k_edges_end skip its level-1 edges
// (Dev::elevel), whose terms stay zero.  (A one-workgroup compaction of the list took 39 us.)

__global__ __launch_bounds__(256) void k_lba_cull(Dev d, LbaState L, int round1) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= d.nl) return;
  const int v = d.hpt_vtx[l], q0 = d.pt_ptr[l], q1 = d.pt_ptr[l + 1];
  int ol, el;
  bool bad;
  if (round1) {
    el = q1 - q0;
    ol = el + (L.extra ? L.extra[v] : 0);
    bad = false;
    L.edges_all[v] = el;
  } else {
    ol = L.obs_left[v]; el = L.edges_left[v]; bad = L.bad[v] != 0;
  }
  // the point's edges eight at a time: their indices, then their flags and chi2 all in flight,
  // then the sequential decisions in edge order from registers
  for (int qb = q0; qb < q1; qb += 8) {
    int ev[8];
    bool in[8];
    double ch[8];
#pragma unroll
    for (int j = 0; j < 8; j++) ev[j] = d.pt_edges[min(qb + j, q1 - 1)];
#pragma unroll
    for (int j = 0; j < 8; j++) { in[j] = L.inlier[ev[j]] != 0; ch[j] = L.chi[ev[j]]; }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (qb + j >= q1) break;
      const int e = ev[j];
      if (!in[j] || bad || !(ch[j] > L.k2)) continue;
      L.inlier[e] = 0;
      if (round1) { L.level[e] = 1; zero_edge_terms(d, e); }
      el--;
      if (--ol < 2) bad = true;
    }
  }
  L.obs_left[v] = ol; L.edges_left[v] = el; L.bad[v] = bad ? 1 : 0;
  // cOptimizer.cpp:885-902: not bad, TotalNrObservations() > 1, >= 2 vertex edges
  if (!round1 && L.pwrite) L.pwrite[v] = !bad && el > 1 && L.edges_all[v] >= 2;
}

// round 1's bookkeeping after k_lba_cull's decisions: per-pose survivors (one atomic per culled
// edge, integer counts), culled edges and points left (one atomic per wave); the last
// workgroup writes the three counts into host memory
__global__ __launch_bounds__(256) void k_lba_count(Dev d, LbaState L) {
  __shared__ int last;
  const int l = blockIdx.x * 256 + threadIdx.x;
  int culled = 0, alive = 0;
  if (l < d.nl) {
    const int v = d.hpt_vtx[l];
    const int el = L.edges_left[v];
    alive = el > 0 ? 1 : 0;
    culled = L.edges_all[v] - el;
    if (culled) {
      for (int q = d.pt_ptr[l]; q < d.pt_ptr[l + 1]; q++) {
        const int e = d.pt_edges[q];
        const int h = d.pt_h[q];
        if (L.level[e] && h >= 0) atomicSub(&L.pose_cnt[h], 1);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { culled += __shfl_xor(culled, o); alive += __shfl_xor(alive, o); }
  if ((threadIdx.x & 63) == 0) {
    if (culled) atomicAdd(&L.ctr[0], (unsigned)culled);
    if (alive) atomicAdd(&L.ctr[1], (unsigned)alive);
  }
  // every count is an atomic (performed in device-coherent memory): each wave drains its own,
  // then one lane counts the workgroup in; the last one reads them with atomic loads
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(&L.ctr[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  int left = 0;
  for (int h = threadIdx.x; h < d.np; h += 256) left |= __hip_atomic_load(&L.pose_cnt[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0 ? 1 : 0;
  left = __syncthreads_or(left);
  if (threadIdx.x == 0) {
    const unsigned c0 = __hip_atomic_load(&L.ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned c1 = __hip_atomic_load(&L.ctr[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    L.res[0] = d.nae - (int)c0;
    L.res[1] = left;
    L.res[2] = (int)c1;
  }
}

// the culling state before round 1: every edge an inlier at level 0, every point vertex clear
__global__ __launch_bounds__(256) void k_lba_init(Dev d, LbaState L, int ne, int npt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < ne) { L.inlier[i] = 1; L.level[i] = 0; }
  if (i < d.np) L.pose_cnt[i] = d.ps_ptr[i + 1] - d.ps_ptr[i];
  if (i < 4) L.ctr[i] = 0u;
  if (i < npt) {
    L.obs_left[i] = 0; L.edges_left[i] = 0; L.edges_all[i] = 0; L.bad[i] = 0;
    if (L.pwrite) L.pwrite[i] = 0;
  }
}

// LocalBA's round-2 results into host memory: [poses | points | inlier flags | write-back flags]
__global__ __launch_bounds__(256) void k_lba_out(const double* poses, int npo, const double* points, int npt,
                                                 const uint8_t* inl, int ne, const uint8_t* pw, int npw,
                                                 uint8_t* host) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double* hd = reinterpret_cast<double*>(host);
  if (i < npo) hd[i] = poses[i];
  else if (i < npo + npt) hd[i] = points[i - npo];
  uint8_t* hb = host + 8 * (size_t)(npo + npt);
  if (i < ne) hb[i] = inl[i];
  if (i < npw) hb[ne + i] = pw[i];
}

}  // namespace mcs::ba
