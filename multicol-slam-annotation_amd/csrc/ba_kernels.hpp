// The kernels of an LM iteration: per-edge error / Jacobians (k_edges), the end of a
// device-driven step (k_edges_end), the normal equations (k_build), a trial's point part,
// Schur complement and update, and the device halves of the test hooks.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ba_dev.hpp"
#include "ba_edge_math.hpp"
#include "ba_reduce.hpp"
#include "ba_structure.hpp"
#include "ldlt.hpp"

namespace mcs::ba {
// per active edge: error (+ robust chi2) and optionally Jacobians / weight / Hpl = w Jp^T Jl
// (device-driven linearisation: only when the previous trial ended an iteration)
__global__ __launch_bounds__(256) void k_edges(Dev d0, int linearize) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (lm_done(d0) || (linearize && d0.ctl && !d0.ctl->lin)) return;
  const Dev d = lin_buf(d0, false);
  if (!linearize && d.part_chi) {   // trial chi2 of a device-driven step: + workgroup partial
    double r0 = 0.0;
    const int e = k < d.nae ? (d.aedge ? d.aedge[k] : k) : 0;
    if (k < d.nae && d.elevel && d.elevel[e]) {
      d.rchi[k] = 0.0;   // level 1: outside the graph
    } else if (k < d.nae) {
      const int pi = d.e_pose[e], li = d.e_point[e], ci = d.e_cam[e];
      double er[2];
      edge_error(d.poses + 6 * pi, d.points + 3 * li, d.mc + 6 * ci, d.cam + 17 * ci, d.e_meas + 2 * e, er);
      const double c2 = d.e_info[e] * (er[0] * er[0] + er[1] * er[1]);
      double r1;
      huber(c2, d.delta, d.dsqr, &r0, &r1);
      d.err[2 * e] = er[0]; d.err[2 * e + 1] = er[1];
      d.chi[e] = c2;
      d.rchi[k] = r0;
    }
    const double sum = block_sum256(r0);
    if (threadIdx.x == 0) d.part_chi[blockIdx.x] = sum;
    return;
  }
  if (k >= d.nae) return;
  const int e = d.aedge ? d.aedge[k] : k;   // null: every edge
  if (d.elevel && d.elevel[e]) { d.rchi[k] = 0.0; return; }   // level 1: terms stay zero
  const int pi = d.e_pose[e], li = d.e_point[e], ci = d.e_cam[e];
  const double* pose = d.poses + 6 * pi;
  const double* X = d.points + 3 * li;
  double er[2];
  edge_error(pose, X, d.mc + 6 * ci, d.cam + 17 * ci, d.e_meas + 2 * e, er);
  const double c2 = d.e_info[e] * (er[0] * er[0] + er[1] * er[1]);
  double r0, r1;
  huber(c2, d.delta, d.dsqr, &r0, &r1);
  d.err[2 * e] = er[0]; d.err[2 * e + 1] = er[1];
  d.chi[e] = c2;
  d.rchi[k] = r0;
  if (linearize) {
    double jp[12], jl[6];
    edge_jac(pose, X, d.mc + 6 * ci, d.cam + 17 * ci, jp, jl);
    for (int i = 0; i < 12; i++) d.jp[12 * e + i] = jp[i];
    for (int i = 0; i < 6; i++) d.jl[6 * e + i] = jl[i];
    const double w = r1 * d.e_info[e];
    d.w[e] = w;
    if (d.hpl && d.pose_h[pi] >= 0 && d.point_h[li] >= 0) {
      for (int a = 0; a < 6; a++)
        for (int bb = 0; bb < 3; bb++)
          d.hpl[18 * e + 3 * a + bb] = w * (jp[a] * jl[bb] + jp[6 + a] * jl[3 + bb]);
    }
  }
}

// after a trial (k_edges_end's last workgroup, one thread): lm_step (lm_control.hpp) with the
// caller's stop flag as the host last published it; flag = the solve's status bits
__device__ void lm_control(LmCtl* c, const double* sc, int flag, LmSig* sig) {
  const int stop = __hip_atomic_load(&sig->ext_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
  lm_step(c, sc, (flag & ldlt::kFlagZeroPivot) != 0, (flag & ldlt::kFlagTimeout) != 0, stop);
}

// The end of a device-driven step, run by the last-arriving workgroup of k_edges_end: the
// trial's three sums from the workgroup partials (each summed exactly as k_reduce3's 1024-thread
// workgroups do: 1024 strided slots, then the LDS tree -- emulated here by kRedNT threads, so
// the bits are the same), the LM control (lm_control) and the pop of a rejected trial.
__device__ __forceinline__ void lm_publish(const LmCtl* c, const LmEnd& le) {
  // relaxed: a stale `done` only costs the host one more (no-op) step
  __hip_atomic_store(&le.sig->done, c->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&le.sig->iter, c->iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&le.sig->seq, le.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// (blockDim >= 256: threads past 256 only take part in the barriers)
__device__ void lm_end_body(const Dev& d, const Sum3& q, const LmEnd& le) {
  static_assert(kRedNT == 256, "the tree below folds 1024 slots onto 256 threads");
  __shared__ double s[3][256];
  __shared__ int rej;
  LmCtl* c = d.ctl;
  const int t = threadIdx.x;
  const bool act = t < 256;
  // slot ts = t + 256 u (u = 0..3) sums v[ts], v[ts + 1024], ... in order; the tree levels 512
  // and 256 (s[ts] += s[ts + o]) pair slots of one thread, so they run in registers; 128 and 64
  // cross waves (LDS); 32 .. 1 stay in wave 0 (shuffles).  Same additions in the same order.
  double a[3];
  if (act) {
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const double* v = q.v[b];
      double x[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        double acc = 0.0;
        // sc1 loads: k_edges_end's partials arrive write-through, without an acquire
        for (int i = t + 256 * u; i < q.n[b]; i += 1024)
          acc = acc + __longlong_as_double((long long)__hip_atomic_load(
                          (const __attribute__((address_space(1))) unsigned long long*)(v + i), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT));
        x[u] = acc;
      }
      x[0] = x[0] + x[2];   // o = 512
      x[1] = x[1] + x[3];
      a[b] = x[0] + x[1];   // o = 256
      s[b][t] = a[b];
    }
  }
  __syncthreads();
  if (t < 128)
    for (int b = 0; b < 3; b++) a[b] = s[b][t] + s[b][t + 128];   // o = 128
  __syncthreads();
  if (t < 128)
    for (int b = 0; b < 3; b++) s[b][t] = a[b];
  __syncthreads();
  if (t < 64) {
    for (int b = 0; b < 3; b++) {
      double w = s[b][t] + s[b][t + 64];                           // o = 64
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) w = w + __shfl_down(w, o, 64);
      if (t == 0) le.sc[b] = w;
    }
  }
  if (t == 0) {
    lm_control(c, le.sc, *le.flag, le.sig);
    rej = c->restore;
  }
  __syncthreads();
  if (rej && act) {   // pop: every pose and point back to the backups of the trial's push
    for (int i = t; i < d.n_pose_dbl; i += kRedNT) d.poses[i] = d.push_poses[i];
    for (int i = t; i < d.n_point_dbl; i += kRedNT) d.points[i] = d.push_points[i];
  }
  // the run's last step: the control block straight into host memory (the report), read by
  // the host once the stream has drained -- no readback copy
  if (le.host_ctl && c->done && act) {
    constexpr int nw = (int)(sizeof(LmCtl) / 4);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(c);
    uint32_t* dst = reinterpret_cast<uint32_t*>(le.host_ctl);
    for (int i = t; i < nw; i += kRedNT) dst[i] = src[i];
  }
  if (t == 0) lm_publish(c, le);
}

// The trial's evaluation (k_edges without linearisation: error, robust chi2, workgroup partial)
// and the end of the step in one launch: each workgroup releases its partial and counts itself
// in; the last one (device-scope counter, agent-scope acquire) closes the step.  A step past
// the end still publishes its sequence number (workgroup 0), as the host waits for each.
// A workgroup holds 256 edges and 512 threads: waves 0-3 evaluate the error / robust chi2 / weight
// of edge k (slot t), waves 4-7 its Jacobians (speculative linearisation), the two independent
// halves of one edge's dependent chain side by side; Hpl = w Jp^T Jl follows once the weight
// has crossed over in LDS.  Every value is the single-thread form's, bit for bit.
__global__ __launch_bounds__(kEdgeEndNT) void k_edges_end(Dev d0, Sum3 q, LmEnd le) {
  __shared__ int last;
  __shared__ double wsh[256];
  __shared__ double sm[4];
  LmCtl* c = d0.ctl;
  if (c->done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) lm_publish(c, le);
    return;
  }
  // with speculative linearisation the trial's error, Jacobians, weight and Hpl go to the
  // other buffer: if lm_control accepts the trial they are the next iteration's linearisation
  // (k_edges at the accepted state, the same arithmetic), and no linearising launch is needed
  const bool spec = c->spec_lin != 0;
  const Dev d = lin_buf(d0, spec);
  const int slot = threadIdx.x & 255;
  const bool jac = threadIdx.x >= 256;   // wave-uniform
  const int k = blockIdx.x * 256 + slot;
  double r0 = 0.0;
  int e = 0, pi = 0, li = 0, ci = 0;
  double jp[12], jl[6];
  bool live = k < d.nae;
  if (live) {
    e = d.aedge ? d.aedge[k] : k;
    if (d.elevel && d.elevel[e]) {   // level 1: outside the graph, terms stay zero
      live = false;
      if (!jac) d.rchi[k] = 0.0;
    }
  }
  if (live) {
    pi = d.e_pose[e]; li = d.e_point[e]; ci = d.e_cam[e];
    const double* pose = d.poses + 6 * pi;
    const double* X = d.points + 3 * li;
    if (!jac) {
      double er[2];
      edge_error(pose, X, d.mc + 6 * ci, d.cam + 17 * ci, d.e_meas + 2 * e, er);
      const double c2 = d.e_info[e] * (er[0] * er[0] + er[1] * er[1]);
      double r1;
      huber(c2, d.delta, d.dsqr, &r0, &r1);
      d.err[2 * e] = er[0]; d.err[2 * e + 1] = er[1];
      d.chi[e] = c2;
      d.rchi[k] = r0;
      if (spec) {
        const double w = r1 * d.e_info[e];
        d.w[e] = w;
        wsh[slot] = w;
      }
    } else if (spec) {
      edge_jac(pose, X, d.mc + 6 * ci, d.cam + 17 * ci, jp, jl);
      for (int i = 0; i < 12; i++) d.jp[12 * e + i] = jp[i];
      for (int i = 0; i < 6; i++) d.jl[6 * e + i] = jl[i];
    }
  }
  __syncthreads();
  if (jac && spec && live && d.hpl && d.pose_h[pi] >= 0 && d.point_h[li] >= 0) {
    const double w = wsh[slot];
    for (int a = 0; a < 6; a++)
      for (int bb = 0; bb < 3; bb++)
        d.hpl[18 * e + 3 * a + bb] = w * (jp[a] * jl[bb] + jp[6 + a] * jl[3 + bb]);
  }
  // block_sum256 over the error waves (0-3): the same butterfly and wave order
  {
    double v = r0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (!jac && (threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  // The partial goes write-through (sc1 store), its wait drains before the arrival add, and the
  // last workgroup reads every partial with sc1 loads (lm_end_body): the hand-off of
  // MI355X_MICROARCH.md's first table row, with no L2 write-back (a __threadfence per workgroup
  // wrote back the ~6 MB of Jacobians this kernel leaves dirty) and no acquire.
  if (threadIdx.x == 0) {
    __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)(d.part_chi + blockIdx.x),
                       (unsigned long long)__double_as_longlong(((sm[0] + sm[1]) + sm[2]) + sm[3]),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(&c->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) __hip_atomic_store(&c->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next step
  lm_end_body(d0, q, le);
}

// chi2 of the starting point -> currentChi (lm_control.hpp)
__global__ void k_lm_start(LmCtl* c, const double* sc) {
  if (threadIdx.x != 0) return;
  lm_start_body(c, sc[0]);
}
// the LM control block of a run, by value (no pageable host copy on the stream)
// (+ the per-block chunk counters of k_schur's fused fin, zeroed)
__global__ void k_ctl_init(LmCtl h0, LmCtl* c, uint32_t* blk_arrive, int nblk) {
  constexpr int nw = (int)(sizeof(LmCtl) / 4);
  static_assert(sizeof(LmCtl) % 4 == 0, "word copy");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&h0);
  uint32_t* dst = reinterpret_cast<uint32_t*>(c);
  for (int i = threadIdx.x; i < nw; i += blockDim.x) dst[i] = src[i];
  if (blk_arrive)
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) blk_arrive[i] = 0u;
}
__global__ void k_lm_lambda0(LmCtl* c, const double* sc) {
  if (threadIdx.x != 0 || c->done) return;
  lm_lambda0_body(c, sc[1], sc[2]);
}

// Test hooks (mcs_ba_lm_replay, mcs_ba_huber_eval): the production device functions replayed on
// scripted inputs, so the LM control and the robust kernel can be checked statement for
// statement against the reference text (tests/golden/gen_g2o_solver.py).
// in = {chi0, maxdiag points, maxdiag poses}; trials [n][4] = {robust chi2 of the trial,
// points' model decrease, poses' model decrease, solve failed}; out [n][10] per trial =
// {lambda used, lambda after, ni, accepted, qmax, nBad, iterations done, done, stop_out,
// currentChi}.  One thread.
__global__ void k_lm_replay(LmCtl* c, LmSig* sig, const double* in, const double* trials, int n,
                            double* out, int* n_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  lm_start_body(c, in[0]);
  if (!c->done) lm_lambda0_body(c, in[1], in[2]);
  int t = 0;
  for (; t < n && !c->done; t++) {
    const double* tr = trials + 4 * t;
    const double sc[3] = {tr[0], tr[1], tr[2]};
    const double lam = c->lambda;
    lm_control(c, sc, tr[3] != 0.0 ? ldlt::kFlagZeroPivot : 0, sig);
    double* o = out + 10 * t;
    o[0] = lam; o[1] = c->lambda; o[2] = c->ni; o[3] = c->restore ? 0.0 : 1.0; o[4] = c->qmax;
    o[5] = c->nBad; o[6] = c->iter; o[7] = c->done; o[8] = c->stop_out; o[9] = c->currentChi;
  }
  *n_out = t;
}

__global__ void k_huber_eval(const double* e, int n, double delta, double dsqr, double* rho0, double* rho1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) huber(e[i], delta, dsqr, &rho0[i], &rho1[i]);
}

// Y_e = Hpl_e Dinv of one (point, edge) entry whose pose is active
__device__ __forceinline__ void y_of(const Dev& d, int e, const double (&Di)[9]) {
  ybl_of(d.hpl + 18 * e, Di, d.y + 18 * e);
}

// per landmark: Dinv, db and one edge's Y from the production helpers (mcs_ba_point_block_eval)
__global__ void k_point_block_eval(const double* H, double lam, const double* b, const double* hpl, int n,
                                   double* Dinv, double* db, double* Y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double Di[9];
  dinv_of(H + 9 * i, lam, Di);
  for (int k = 0; k < 9; k++) Dinv[9 * i + k] = Di[k];
  db_of(Di, b + 3 * i, db + 3 * i);
  ybl_of(hpl + 18 * i, Di, Y + 18 * i);
}

// per active point: Hll (3x3), b_l over its edges in edge order; diag -> red (for lambda init)
// four lanes per point (edges q0 + sub, q0 + sub + 4, ...), the quad's partial sums combined
// in a fixed order ((l0 + l1) + (l2 + l3)): deterministic, and 4x the threads of one lane per
// point (config C: 3000 points would occupy 12 workgroups)
// TRIAL (k_build_trial): the same quad then carries k_point_trial's point part -- Dinv, db and
// the Y of the point's edges -- from the H and b it holds (LIN: just built; otherwise the
// iteration's stored Hll / b_l: a rejected trial re-solves the same linearisation)
template <bool TRIAL>
__device__ __forceinline__ void points_build_body(const Dev& d, int block, bool lin) {
  const int gt = block * kBuildNT + threadIdx.x;
  const int l = gt >> 2, sub = gt & 3;
  const bool act = l < d.nl;
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  if (lin) {
    if (act) {
      auto term = [&](int e) {
        const double* jl = d.jl + 6 * e;
        const double w = d.w[e];
        const double we0 = -w * d.err[2 * e], we1 = -w * d.err[2 * e + 1];
        for (int a = 0; a < 3; a++) {
          for (int bb = 0; bb < 3; bb++) H[3 * a + bb] += w * (jl[a] * jl[bb] + jl[3 + a] * jl[3 + bb]);
          b[a] += jl[a] * we0 + jl[3 + a] * we1;
        }
      };
      // the quad lane's entries q and q + 4 with their index loads together, added in q order
      const int q1 = d.pt_ptr[l + 1];
      for (int q = d.pt_ptr[l] + sub; q < q1; q += 8) {
        const bool two = q + 4 < q1;
        const int ea = d.pt_edges[q], eb = d.pt_edges[two ? q + 4 : q];
        term(ea);
        if (two) term(eb);
      }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = quad_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] = quad_sum(b[i]);
    if (act && sub == 0) {
      for (int i = 0; i < 9; i++) d.Hll[9 * l + i] = H[i];
      for (int i = 0; i < 3; i++) d.bl[3 * l + i] = b[i];
      d.red[l] = fmax(fmax(fabs(H[0]), fabs(H[4])), fabs(H[8]));
    }
  } else if (TRIAL && act) {
    for (int i = 0; i < 9; i++) H[i] = d.Hll[9 * l + i];
    for (int i = 0; i < 3; i++) b[i] = d.bl[3 * l + i];
  }
  if (!TRIAL || !act) return;
  double Di[9];
  dinv_of(H, lam_of(d), Di);
  if (sub == 0) {
    for (int k = 0; k < 9; k++) d.Dinv[9 * l + k] = Di[k];
    db_of(Di, b, d.db + 3 * l);
  }
  for (int q = d.pt_ptr[l] + sub; q < d.pt_ptr[l + 1]; q += 4) {
    // pt_h[q] = pose_h[e_pose[pt_edges[q]]] (host-built): one load instead of a chain of three
    if (d.pt_h[q] >= 0) y_of(d, d.pt_edges[q], Di);
  }
}

// One level of a wave's recursive halving over N values (of NA slots): values [0, H) and
// [H, N) (zero-padded to H) split by lane bit O; the lane keeps one half in acc[0, H) and adds
// its partner's copy of that half.  Own + partner at every level is what a full xor butterfly
// forms for every value, bit for bit, with ~N exchanges instead of 6 N.
template <int NA, int N, int O>
__device__ __forceinline__ void wave_halve(double (&acc)[NA], int lane) {
  constexpr int H = (N + 1) / 2;
  const bool hi = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const double a = acc[i], b = (H + i < N) ? acc[H + i] : 0.0;
    const double keep = hi ? b : a, give = hi ? a : b;
    acc[i] = keep + __shfl_xor(give, O);
  }
}
// the six levels (bits 32 .. 1) over N <= 64 values; returns the value whose wave sum the lane
// then holds in acc[0] (-1: a padding slot).  The split points are the static H of each level;
// a lane's real count shrinks to n - H on the high side, so some slots of the last levels are
// zero padding.
template <int N, int NA>
__device__ __forceinline__ int wave_halve_all(double (&acc)[NA], int lane) {
  static_assert(N <= 64 && N <= NA, "one value per lane at most");
  constexpr int N1 = (N + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2,
                N5 = (N4 + 1) / 2;
  wave_halve<NA, N, 32>(acc, lane);
  wave_halve<NA, N1, 16>(acc, lane);
  wave_halve<NA, N2, 8>(acc, lane);
  wave_halve<NA, N3, 4>(acc, lane);
  wave_halve<NA, N4, 2>(acc, lane);
  wave_halve<NA, N5, 1>(acc, lane);
  int idx = 0, n = N, nk = N;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const int h = (nk + 1) / 2;
    if (lane & (32 >> k)) { idx += h; n -= h; } else n = n < h ? n : h;
    nk = h;
  }
  return n > 0 ? idx : -1;
}

// Deterministic block sum of NV per-thread partials over a workgroup of NW waves: the fixed
// xor-butterfly's sums inside each wave, then the NW wave sums in wave order.  On return
// sm[v * NW] holds sum v (after the barrier).
template <int NV, int NW>
__device__ __forceinline__ void block_sum_vec(double (&acc)[NV], double* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // the wave sums by recursive halving (the xor butterfly's sums, bit for bit); sum v ends in
  // one lane, which writes it
  const int mine = wave_halve_all<NV>(acc, lane);
  if (mine >= 0) sm[mine * NW + w] = acc[0];
  __syncthreads();
  if (threadIdx.x < NV) {
    const int v = threadIdx.x;
    double t = sm[v * NW];
#pragma unroll
    for (int k = 1; k < NW; k++) t += sm[v * NW + k];
    sm[v * NW] = t;
  }
  __syncthreads();
}

constexpr int kUpper6[21][2] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {0, 5}, {1, 1},
                                {1, 2}, {1, 3}, {1, 4}, {1, 5}, {2, 2}, {2, 3}, {2, 4},
                                {2, 5}, {3, 3}, {3, 4}, {3, 5}, {4, 4}, {4, 5}, {5, 5}};

// per active pose: Hpp (6x6, upper 21 mirrored), b_p; edges of the pose split over the
// workgroup's threads (fixed stride), block tree sum.  Also the diagonal and b_p into the
// exchange area.
__device__ __forceinline__ void poses_build_body(const Dev& d, int i) {
  __shared__ double sm[27 * (kBuildNT / 64)];
  const int t = threadIdx.x;
  double acc[27];
#pragma unroll
  for (int v = 0; v < 27; v++) acc[v] = 0.0;
  // a thread's edges t, t + 256, ... in that order; kU of them per pass with every load issued
  // before the first sum (the edge -> Jacobian gather is two dependent round trips, and a
  // pose has ~1500 edges at config C: one at a time the chain was the whole kernel).  Loads
  // past the list read the last edge (unconditional: no merge waits) and are not summed.
#ifndef MCS_BUILD_KU
#define MCS_BUILD_KU 4
#endif
  constexpr int kU = MCS_BUILD_KU;
  const int q0 = d.ps_ptr[i], q1 = d.ps_ptr[i + 1];
  for (int qb = q0 + t; qb < q1; qb += kU * kBuildNT) {
    int e[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) e[u] = d.ps_edges[min(qb + u * kBuildNT, q1 - 1)];
    double j0[kU][6], j1[kU][6], w[kU], er0[kU], er1[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const double* jp = d.jp + 12 * e[u];
#pragma unroll
      for (int a = 0; a < 6; a++) { j0[u][a] = jp[a]; j1[u][a] = jp[6 + a]; }
      w[u] = d.w[e[u]];
      er0[u] = d.err[2 * e[u]];
      er1[u] = d.err[2 * e[u] + 1];
    }
#pragma unroll
    for (int u = 0; u < kU; u++) {
      if (qb + u * kBuildNT >= q1) break;
      const double we0 = -w[u] * er0[u], we1 = -w[u] * er1[u];
#pragma unroll
      for (int v = 0; v < 21; v++) {
        const int a = kUpper6[v][0], bb = kUpper6[v][1];
        acc[v] += w[u] * (j0[u][a] * j0[u][bb] + j1[u][a] * j1[u][bb]);
      }
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] += j0[u][a] * we0 + j1[u][a] * we1;
    }
  }
  constexpr int NW = kBuildNT / 64;
  block_sum_vec<27, NW>(acc, sm);
  if (t < 21) {
    const int a = kUpper6[t][0], bb = kUpper6[t][1];
    const double h = sm[t * NW];
    d.Hpp[36 * i + 6 * a + bb] = h;
    d.Hpp[36 * i + 6 * bb + a] = h;
    if (a == bb) d.hdiag[6 * i + a] = h;
  } else if (t < 27) {
    d.bp[6 * i + t - 21] = sm[t * NW];
    d.bpf[6 * i + t - 21] = sm[t * NW];
  }
}
// both builds in one launch: workgroups [0, np) per pose, the rest four lanes per point
__global__ __launch_bounds__(kBuildNT) void k_build(Dev d0) {
  if (lm_done(d0) || (d0.ctl && !d0.ctl->lin)) return;
  const Dev d = lin_buf(d0, false);
  if ((int)blockIdx.x < d.np) poses_build_body(d, blockIdx.x);
  else points_build_body<false>(d, blockIdx.x - d.np, true);
}

// the trial's push (backup of every pose and point) and the solve-flag reset, grid-strided
__device__ __forceinline__ void trial_push(const Dev& d, int q, int stride) {
  for (int i = q; i < d.n_pose_dbl; i += stride) d.push_poses[i] = d.poses[i];
  for (int i = q; i < d.n_point_dbl; i += stride) d.push_points[i] = d.points[i];
  if (q == 0) *d.flag = 0;
}

// One thread per (point, edge) entry of the point CSR: D = Hll + lambda I -> Dinv (cofactors,
// recomputed per entry: identical bits), Y_e = Hpl_e Dinv; the first entry of each point
// also stores Dinv and db = Dinv b_l.
__global__ __launch_bounds__(256) void k_point_trial(Dev d0) {
  if (lm_done(d0)) return;
  const Dev d = lin_buf(d0, false);
  const int q = blockIdx.x * 256 + threadIdx.x;
  trial_push(d, q, gridDim.x * 256);
  if (q >= d.npe) return;
  const int e = d.pt_edges[q];
  const int l = d.point_h[d.e_point[e]];
  const bool first = (q == d.pt_ptr[l]);
  const bool pose_act = d.pt_h[q] >= 0;
  if (!first && !pose_act) return;
  double Di[9];
  dinv_of(d.Hll + 9 * l, lam_of(d), Di);
  if (first) {
    for (int k = 0; k < 9; k++) d.Dinv[9 * l + k] = Di[k];
    db_of(Di, d.bl + 3 * l, d.db + 3 * l);
  }
  if (pose_act) y_of(d, e, Di);
}

// Device-driven steps after the first: k_build (when the step linearises) and k_point_trial in
// one launch -- the point quads go on from their H / b to Dinv, db and Y (same arithmetic,
// same bits), every thread takes part in the push.  Step 0 keeps the two launches: lambda's
// initial value needs the built diagonal first.
__global__ __launch_bounds__(kBuildNT) void k_build_trial(Dev d0) {
  if (lm_done(d0)) return;
  const Dev d = lin_buf(d0, false);
  const bool lin = d.ctl->lin != 0;
  trial_push(d, blockIdx.x * kBuildNT + threadIdx.x, gridDim.x * kBuildNT);
  if ((int)blockIdx.x < d.np) { if (lin) poses_build_body(d, blockIdx.x); }
  else points_build_body<true>(d, blockIdx.x - d.np, lin);
}


// reduced camera system, lower blocks (i >= j): S_ij = [i==j](Hpp_i + lam0 I)
//   - sum over (e1 in pose i, e2 in pose j, same point) Y_e1 Hpl_e2^T;
// diagonal blocks also form bschur_i = b_i - sum_e Hpl_e db(point(e)).
// Work items (host-built, `build_schur_items`): item = (block, chunk c of nch); chunk c covers
// pairs [q0 + c*CH, ...) and, on a diagonal block, pose edges [e0 + c*CH, ...).  One wave per
// item: lane L accumulates entries L, L+64, ... in registers, a fixed recursive halving over
// the wave (wave_halve_all) leaves each of the 42 sums in one lane.  A block with one chunk (config E: ~90 pairs per
// block) writes S / bschur directly; otherwise the chunk's sums go to a partial slot and
// the wave that completes the block's last chunk adds the slots in chunk order (config C: 55
// blocks of thousands of pairs, so a
// block per wave would leave the GPU idle).  Every order is fixed: bitwise reproducible.
// lam0 = lambda on rank 0 and 0 elsewhere (the sharded sum then holds lambda once).

__device__ __forceinline__ void schur_write(const Dev& d, int bi, int bj, double lam0, int lane,
                                            double v) {
  if (lane < 36) {
    const int a = lane / 6, c = lane % 6;
    if (bi == bj && c > a) return;   // lower triangle of the diagonal block only
    double s0 = 0.0;
    if (bi == bj) { s0 = d.Hpp[36 * bi + 6 * a + c]; if (a == c) s0 += lam0; }
    d.S[ldlt::sidx(6 * bi + a, 6 * bj + c, d.T)] = s0 - v;
  } else if (lane < 42 && bi == bj) {
    const int a = lane - 36;
    d.bs[6 * bi + a] = d.bp[6 * bi + a] - v;
  }
}


__global__ __launch_bounds__(256) void k_schur(Dev d0) {
  if (lm_done(d0)) return;
  const Dev d = lin_buf(d0, false);
  const double lam0 = lam0_of(d);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int it = blockIdx.x * 4 + w;
  if (it >= *d.nitem) return;
  const int blk = d.it_blk[it], c = d.it_chunk[it], slot = d.it_slot[it];
  const int bi = d.blk_i[blk], bj = d.blk_j[blk];
  const int q0 = min(d.pr_ptr[blk] + c * kSchurChunk, d.pr_ptr[blk + 1]);
  const int q1 = min(q0 + kSchurChunk, d.pr_ptr[blk + 1]);
  double acc[42];
#pragma unroll
  for (int v = 0; v < 42; v++) acc[v] = 0.0;
  // the next pair's index is loaded ahead, so each pair costs one dependent round trip (its
  // rows), not two
  int q = q0 + lane;
  uint2 pqn = q < q1 ? d.pr[q] : make_uint2(0u, 0u);
  for (; q < q1; q += 64) {
    const uint2 pq = pqn;
    if (q + 64 < q1) pqn = d.pr[q + 64];
    const double* Y = d.y + 18 * pq.x;
    const double* B = d.hpl + 18 * pq.y;
    double y[18], bb[18];
#pragma unroll
    for (int k = 0; k < 18; k++) { y[k] = Y[k]; bb[k] = B[k]; }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int cc = 0; cc < 6; cc++)
        acc[6 * a + cc] += y[3 * a] * bb[3 * cc] + y[3 * a + 1] * bb[3 * cc + 1] + y[3 * a + 2] * bb[3 * cc + 2];
  }
  int nact = q1 - q0;
  if (bi == bj) {
    const int e0 = min(d.ps_ptr[bi] + c * kSchurChunk, d.ps_ptr[bi + 1]);
    const int e1 = min(e0 + kSchurChunk, d.ps_ptr[bi + 1]);
    nact = max(nact, e1 - e0);
    auto term = [&](int e, int lh) {
      if (lh < 0) return;   // fixed point (pose-only BA): no Schur term
      const double* B = d.hpl + 18 * e;
      const double* g = d.db + 3 * lh;
      const double g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
      for (int a = 0; a < 6; a++) acc[36 + a] += B[3 * a] * g0 + B[3 * a + 1] * g1 + B[3 * a + 2] * g2;
    };
    // a lane's edges q and q + 64 (the chunk is 2 x 64) with their three-deep index chains
    // interleaved, then added in q order
    for (int q = e0 + lane; q < e1; q += 128) {
      const bool two = q + 64 < e1;
      const int ea = d.ps_edges[q], eb = d.ps_edges[two ? q + 64 : q];
      const int la = d.point_h[d.e_point[ea]], lb = d.point_h[d.e_point[eb]];
      term(ea, la);
      if (two) term(eb, lb);
    }
  }
  (void)nact;
  // the 42 wave sums by recursive halving: at level o a lane keeps the half of its values
  // selected by lane bit o and adds its partner's copy of that half (own + partner: the same
  // sum, bit for bit, as a full xor butterfly forms for every value), so 44 exchanges instead
  // of 6 x 42, and sum v ends in one lane (wave_halve_all), which writes it
  const int v = wave_halve_all<42>(acc, lane);
  if (slot < 0) {
    if (v >= 0) schur_write(d, bi, bj, lam0, v, acc[0]);
    return;
  }
  if (!d.blk_arrive) {   // k_schur_fin adds the slots
    if (v >= 0) d.schur_part[(size_t)slot * 42 + v] = acc[0];
    return;
  }
  // Fused fin (one-tile systems): the slot goes write-through (sc1), the wave's stores drain, one
  // lane counts the chunk in; the wave whose chunk arrives last adds the block's slots in chunk
  // order with sc1 loads (k_schur_fin's order and bits) and writes S / bschur.  Each wave hands
  // off for itself (MI355X_MICROARCH.md, first table row): no fence, no extra launch.
  if (v >= 0)
    __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)(d.schur_part + (size_t)slot * 42 + v),
                       (unsigned long long)__double_as_longlong(acc[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int n = d.blk_nch[blk];
  unsigned prev = 0;
  if (lane == 0) prev = __hip_atomic_fetch_add(&d.blk_arrive[blk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  prev = __builtin_amdgcn_readfirstlane(prev);
  if ((int)prev != n - 1) return;
  if (lane == 0) __hip_atomic_store(&d.blk_arrive[blk], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next step
  const int s0 = d.blk_slot0[blk];
  double sum = 0.0;
  if (lane < 42) {
    const __attribute__((address_space(1))) unsigned long long* P =
        (const __attribute__((address_space(1))) unsigned long long*)(d.schur_part + (size_t)s0 * 42 + lane);
    int cc = 0;
    for (; cc + 8 <= n; cc += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; u++)
        t[u] = __longlong_as_double((long long)__hip_atomic_load(P + (size_t)(cc + u) * 42, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
      for (int u = 0; u < 8; u++) sum += t[u];
    }
    for (; cc < n; cc++)
      sum += __longlong_as_double((long long)__hip_atomic_load(P + (size_t)cc * 42, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  schur_write(d, bi, bj, lam0, lane, sum);
}

// blocks split into several chunks: sum the chunk slots in chunk order, then write (one wave
// per block; blocks of one chunk were written by k_schur).  Measured against finishing in
// k_schur by the wave whose chunk arrives last (agent release / atomic / acquire): equal at
// config C, 2.6x slower k_schur at config E, whose 199 diagonal blocks split 16 ways.
__global__ __launch_bounds__(256) void k_schur_fin(Dev d, int nblk) {
  if (lm_done(d) || d.blk_arrive) return;
  const double lam0 = lam0_of(d);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= nblk) return;
  const int n = d.blk_nch[b];
  if (n <= 1) return;
  const int s0 = d.blk_slot0[b];
  double v = 0.0;
  if (lane < 42) {
    // eight slots' loads in flight, then added in chunk order (the same sum, bit for bit, as
    // one slot at a time, without a dependent round trip per slot)
    const double* P = d.schur_part + (size_t)s0 * 42 + lane;
    int c = 0;
    for (; c + 8 <= n; c += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; u++) t[u] = P[(size_t)(c + u) * 42];
#pragma unroll
      for (int u = 0; u < 8; u++) v += t[u];
    }
    for (; c < n; c++) v += P[(size_t)c * 42];
  }
  schur_write(d, d.blk_i[b], d.blk_j[b], lam0, lane, v);
}


// x_l = Dinv (b_l - sum_e Hpl_e^T x_p); point = backup + x_l; model-decrease terms:
// red[k] (points, k < nl) and red[nl + i] (poses) summed separately (poses are replicated
// across shards, points are not).
__global__ __launch_bounds__(256) void k_update(Dev d0) {
  if (lm_done(d0)) return;
  const Dev d = lin_buf(d0, false);
  const int gt = blockIdx.x * 256 + threadIdx.x;
  const double lam = lam_of(d);
  double spt = 0.0, sps = 0.0;   // this thread's point / pose model-decrease term
  if (gt < 4 * d.nl) {   // points: four lanes per point, as the point build
    const int k = gt >> 2, sub = gt & 3;
    double c[3] = {0.0, 0.0, 0.0};
    auto term = [&](int e, int i1) {
      if (i1 < 0) return;
      const double* B = d.hpl + 18 * e;
      for (int b = 0; b < 3; b++)
        for (int a = 0; a < 6; a++) c[b] -= B[3 * a + b] * d.xp[6 * i1 + a];
    };
    // the quad lane's entries q and q + 4 with their index loads together, applied in q order
    const int q1 = d.pt_ptr[k + 1];
    for (int q = d.pt_ptr[k] + sub; q < q1; q += 8) {
      const bool two = q + 4 < q1;
      const int qb = two ? q + 4 : q;
      const int ea = d.pt_edges[q], eb = d.pt_edges[qb];
      const int ia = d.pt_h[q], ib = d.pt_h[qb];
      term(ea, ia);
      if (two) term(eb, ib);
    }
#pragma unroll
    for (int b = 0; b < 3; b++) c[b] = d.bl[3 * k + b] + quad_sum(c[b]);
    if (sub == 0) {
      const double* Di = d.Dinv + 9 * k;
      double s = 0;
      const int v = d.hpt_vtx[k];
      for (int a = 0; a < 3; a++) {
        const double xa = Di[3 * a] * c[0] + Di[3 * a + 1] * c[1] + Di[3 * a + 2] * c[2];
        d.points[3 * v + a] = d.points_bk[3 * v + a] + xa;
        s += xa * (lam * xa + d.bl[3 * k + a]);
      }
      d.red[k] = s;
      spt = s;
    }
  } else if (gt < 4 * d.nl + d.np) {
    const int i = gt - 4 * d.nl;
    const int v = d.hpose_vtx[i];
    double s = 0;
    for (int a = 0; a < 6; a++) {
      const double xa = d.xp[6 * i + a];
      d.poses[6 * v + a] = d.poses_bk[6 * v + a] + xa;
      s += xa * (lam * xa + d.bpf[6 * i + a]);
    }
    d.red[d.nl + i] = s;
    sps = s;
  }
  if (d.part_pt) {   // device-driven step: workgroup partials of both sums
    const double a = block_sum256(spt);
    const double b = block_sum256(sps);
    if (threadIdx.x == 0) { d.part_pt[blockIdx.x] = a; d.part_ps[blockIdx.x] = b; }
  }
}

// the trial's pop (restore every pose and point from the backups) in one launch
__global__ __launch_bounds__(256) void k_restore(Dev d) {
  const int q = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  for (int i = q; i < d.n_pose_dbl; i += stride) d.poses[i] = d.push_poses[i];
  for (int i = q; i < d.n_point_dbl; i += stride) d.points[i] = d.push_points[i];
}

}  // namespace mcs::ba
