// cOptimizer::OptimizeSim3 on the device: ONE current keyframe KF1 against a batch of T loop
// candidates, the whole function in one launch, one workgroup per candidate.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cOptimizer::OptimizeSim3                             src/cOptimizerLoopStuff.cpp:63-270
//   VertexSim3Expmap_Multi, the two projection edges     include/g2o_MultiCol_sim3_expmap.h:117-260
//   g2o::Sim3                                            ThirdParty/g2o/g2o/types/sim3.h:41-292
//   OptimizationAlgorithmLevenberg::solve                ThirdParty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   vpMapPointMatches of ComputeSim3                     src/cLoopClosing.cpp:354-369
// The math is csrc/sim3_opt_math.hpp (the same functions the host program of the tests runs), the
// LM control csrc/lm_control.hpp.  k_sim3_opt mirrors optimize_sim3_one: the kept slots are
// compacted in slot order (ballot prefix, no atomics), the 2N edges are spread over 256 threads,
// a fixed-order reduction gives the 28 + 7 + 1 sums of a trial, thread 0 solves the 7x7, applies
// the update and runs lm_step; everyone re-evaluates.  The linearisation of a trial's state is
// summed together with its chi2, so an accepted trial needs no second pass.
// FP64, -ffp-contract=off, no floating-point atomics: identical bits from run to run.
#include "host_util.hpp"
#include "sim3_opt_math.hpp"
#include <climits>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <vector>

namespace mcs {
namespace s3o {

constexpr int kMaxCams = 8;
constexpr int kMaxKp = 1 << 19;
constexpr int kNT = 256;           // threads of the one workgroup per candidate
constexpr int kMaxTrials = 64;

struct Set {
  int n_kp_total;
  const int32_t* off; const float* kp_xy; const int32_t* kp_oct; const int32_t* kp_cam;
  const double* m_t; const double* m_c; const double* cam;
};

struct Out {
  int32_t* n_in; int32_t* n_corr; int32_t* n_bad; int32_t* n_undefined;
  double* s12; double* q12; double* R12; double* t12;
  int32_t* iters; double* chi2; double* lambda; int32_t* trials; double* edge_chi2;
};

struct Args {
  Set k1, k2;
  const double* pos1; const double* pos2;
  int32_t* matches12; const uint8_t* ok1; const uint8_t* ok2; const int32_t* first2;
  const double* inv_sigma2_1; const double* sigma2_2;
  const double* s12; const double* R12; const double* t12;
  mcs_sim3_opt_options o;
  Out out;
  Row* rows;                       // [T][n1]
  int n1, C, L;
};

// what lives in LDS for the workgroup's candidate; thread 0 is the only writer of ctl, S and the
// sums, always between two barriers
struct Shared {
  ba::LmCtl ctl;
  Sim3 S, bak;
  double cur[kSums], tri[kSums], part[kNT / 64][kSums];
  double imc[kMaxCams * 12], cam[kMaxCams * 17], h[24];
  int w[kNT / 64], u[kNT / 64];
  int n, live, n_bad, stop;
  int iters[2], trials[2][kMaxIts];
  double chi2[2], lambda[2];
};

// the sums of all live edges at sh.S -> dst (in LDS), e12 of every pair before e21; the order is
// fixed by thread and stride, then by lane (xor butterfly) and wave
__device__ void block_sums(Shared& sh, const Row* __restrict__ rows, double delta, double dsqr, double* dst) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = sh.n;
  const Sim3 S = sh.S, Si = sim3_inverse(S);
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; k++) acc[k] = 0.0;
  for (int e = threadIdx.x; e < 2 * n; e += kNT) {
    const int kind = e >= n, j = kind ? e - n : e;
    const Row r = rows[j];
    if (r.alive) edge_accumulate(S, Si, r, kind, sh.imc, sh.cam, delta, dsqr, acc);
  }
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    double v = acc[k];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    if (lane == 0) sh.part[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < kSums; k++) dst[k] = ((sh.part[0][k] + sh.part[1][k]) + sh.part[2][k]) + sh.part[3][k];
}

// optimize(its) of one round: run_round of sim3_opt_math.hpp with the sums taken by the workgroup.
// Every branch is on a kernel argument or on a value read from LDS after a barrier.
__device__ void block_round(Shared& sh, const Row* __restrict__ rows, const mcs_sim3_opt_options& o, int its,
                            int round) {
  const double delta = 1.345 * o.std_sim, dsqr = huber_dsqr(delta);
  if (threadIdx.x == 0) {
    sh.iters[round] = 0; sh.chi2[round] = 0.0; sh.lambda[round] = 0.0;
    for (int k = 0; k < kMaxIts; k++) sh.trials[round][k] = 0;
    int live = 0;
    for (int j = 0; j < sh.n; j++) live += rows[j].alive != 0;
    sh.live = live;
  }
  __syncthreads();
  if (sh.live == 0) return;                    // "0 vertices to optimize": optimize returns -1
  block_sums(sh, rows, delta, dsqr, sh.cur);
  if (threadIdx.x == 0) {
    ba::lm_init(sh.ctl, lm_options(o, its));
    ba::lm_start_body(&sh.ctl, sh.cur[35]);
    sh.ctl.done = (its <= 0 || sh.stop) ? 1 : 0;
  }
  __syncthreads();
  const int bound = its * o.max_trials;
  for (int g = 0; g < bound; g++) {
    const int done = sh.ctl.done;              // written before the last barrier
    if (done) break;
    double x[7], scale = 0.0;
    bool ok = true;
    if (threadIdx.x == 0) {
      if (sh.ctl.lin && sh.ctl.iter == 0) { const double mx = max_diag(sh.cur); ba::lm_lambda0_body(&sh.ctl, mx, mx); }
      ok = solve7(sh.cur, sh.ctl.lambda, x, &scale);
      sh.bak = sh.S;
      sh.S = sim3_mul(sim3_exp(x), sh.bak);    // oplusImpl
    }
    __syncthreads();
    block_sums(sh, rows, delta, dsqr, sh.tri);
    if (threadIdx.x == 0) {
      const double sc[3] = {sh.tri[35], 0.0, scale};
      const int it = sh.ctl.iter;
      ba::lm_step(&sh.ctl, sc, !ok, false, sh.stop);
      if (it < kMaxIts) sh.trials[round][it]++;
      if (sh.ctl.restore) sh.S = sh.bak;
      else for (int k = 0; k < kSums; k++) sh.cur[k] = sh.tri[k];
      if (sh.ctl.stop_out) sh.stop = 1;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sh.iters[round] = sh.ctl.iter;
    sh.chi2[round] = sh.ctl.currentChi;
    sh.lambda[round] = sh.ctl.iter > 0 ? sh.ctl.lambda_final : 0.0;
  }
  __syncthreads();
}

// :212-232 / :247-263 over the live pairs -> how many were taken out (the same value in every thread)
__device__ int block_cull(Shared& sh, Row* __restrict__ rows, double std_sim, int32_t* __restrict__ m12,
                          double* __restrict__ echi) {
  const double dh = 1.345 * std_sim, dh2 = dh * dh;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = sh.n;
  const Sim3 S = sh.S, Si = sim3_inverse(S);
  int bad = 0;
  for (int j0 = 0; j0 < n; j0 += kNT) {
    const int j = j0 + threadIdx.x;
    bool out = false;
    if (j < n && rows[j].alive) {
      const Row r = rows[j];
      double e[2];
      edge_eval(S, Si, r, 0, sh.imc, sh.cam, e, nullptr);
      const double c12 = edge_chi2(e, r.w1);
      edge_eval(S, Si, r, 1, sh.imc, sh.cam, e, nullptr);
      const double c21 = edge_chi2(e, r.w2);
      if (echi) { echi[2 * r.slot] = c12; echi[2 * r.slot + 1] = c21; }
      out = c12 > dh2 || c21 > dh2;
      if (out) { rows[j].alive = 0; m12[r.slot] = -1; }
    }
    bad += __popcll(__ballot(out));
  }
  if (lane == 0) sh.w[wv] = bad;
  __syncthreads();
  const int tot = sh.w[0] + sh.w[1] + sh.w[2] + sh.w[3];
  __syncthreads();
  return tot;
}

__global__ __launch_bounds__(kNT) void k_sim3_opt(Args a) {
  __shared__ Shared sh;
  const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n1 = a.n1;
  const int o1 = min(max(a.k1.off[0], 0), a.k1.n_kp_total);
  const int n_1 = min(min(max(a.k1.off[1] - o1, 0), a.k1.n_kp_total - o1), n1);
  const int o2 = min(max(a.k2.off[t], 0), a.k2.n_kp_total);
  const int n_2 = min(max(a.k2.off[t + 1] - o2, 0), a.k2.n_kp_total - o2);
  int32_t* m12 = a.matches12 + (int64_t)t * n1;
  Row* rows = a.rows + (int64_t)t * n1;
  double* echi = a.out.edge_chi2 ? a.out.edge_chi2 + 2 * (int64_t)t * n1 : nullptr;
  if ((int)threadIdx.x < a.C) inv_mat44(a.k1.m_c + 16 * threadIdx.x, sh.imc + 12 * threadIdx.x, sh.imc + 12 * threadIdx.x + 9);
  if (threadIdx.x == 64) inv_mat44(a.k1.m_t, sh.h, sh.h + 9);
  if (threadIdx.x == 65) inv_mat44(a.k2.m_t + 16 * (int64_t)t, sh.h + 12, sh.h + 21);
  for (int k = threadIdx.x; k < 17 * a.C; k += kNT) sh.cam[k] = a.k1.cam[k];
  if (threadIdx.x == 128) {
    sh.S = sim3_from_srt(a.s12[t], a.R12 + 9 * (int64_t)t, a.t12 + 3 * (int64_t)t);
    sh.stop = 0;
  }
  if (echi)
    for (int k = threadIdx.x; k < 2 * n1; k += kNT) echi[k] = __builtin_nan("");
  __syncthreads();
  // the slot rules (:122-161), kNT slots per round; kept slots get consecutive rows in slot order
  const KfView v1{n_1, a.k1.kp_xy + 2 * (int64_t)o1, a.k1.kp_oct + o1, a.k1.kp_cam + o1};
  const KfView v2{n_2, a.k2.kp_xy + 2 * (int64_t)o2, a.k2.kp_oct + o2, a.k2.kp_cam + o2};
  int base = 0, undef = 0;
  for (int i0 = 0; i0 < n1; i0 += kNT) {
    const int i = i0 + threadIdx.x;
    Row r;
    int what = 0, m = -1;
    if (i < n_1) {
      m = m12[i];
      what = slot_rule(v1, v2, i, m, a.ok1, a.ok2 + o2, a.first2 + o2, a.L, a.C, a.o.flags & MCS_SIM3OPT_OWN_CAMERA,
                       a.inv_sigma2_1, a.sigma2_2, &r);
    }
    const uint64_t bal = __ballot(what == 1), ubal = __ballot(what == 2);
    if (lane == 0) { sh.w[wv] = __popcll(bal); sh.u[wv] = __popcll(ubal); }
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < kNT / 64; w++) { pre += w < wv ? sh.w[w] : 0; tot += sh.w[w]; undef += sh.u[w]; }
    if (what == 2) m12[i] = -1;
    if (what == 1) {
      hom_mul(sh.h, sh.h + 9, a.pos1 + 3 * (int64_t)(o1 + i), r.X1);         // invMat(M_t1) * (Xw1, 1)
      hom_mul(sh.h + 12, sh.h + 21, a.pos2 + 3 * (int64_t)(o2 + m), r.X2);   // invMat(M_t2) * (Xw2, 1)
      rows[base + pre + __popcll(bal & dev::lanemask_lt())] = r;
    }
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) sh.n = base;
  __syncthreads();
  const Sim3 S0 = sh.S;
  block_round(sh, rows, a.o, a.o.its_round1, 0);
  const int n_bad = block_cull(sh, rows, a.o.std_sim, m12, echi);
  if (threadIdx.x == 0) {
    sh.iters[1] = 0; sh.chi2[1] = 0.0; sh.lambda[1] = 0.0;
    for (int k = 0; k < kMaxIts; k++) sh.trials[1][k] = 0;
  }
  int n_in = 0;
  const bool recover = base - n_bad >= 3;      // :240-241 (the same value in every thread)
  if (recover) {
    block_round(sh, rows, a.o, n_bad > 0 ? a.o.its_culled : a.o.its_clean, 1);
    n_in = base - n_bad - block_cull(sh, rows, a.o.std_sim, m12, echi);
  }
  if (threadIdx.x == 0) {
    const Sim3 S = recover ? sh.S : S0;
    a.out.n_in[t] = n_in; a.out.n_corr[t] = base; a.out.n_bad[t] = n_bad; a.out.n_undefined[t] = undef;
    a.out.s12[t] = S.s;
    double R[9];
    if (recover) quat_to_rot(S.q, R);
    else for (int k = 0; k < 9; k++) R[k] = a.R12[9 * (int64_t)t + k];
    for (int k = 0; k < 4; k++) a.out.q12[4 * (int64_t)t + k] = S.q[k];
    for (int k = 0; k < 9; k++) a.out.R12[9 * (int64_t)t + k] = R[k];
    for (int k = 0; k < 3; k++) a.out.t12[3 * (int64_t)t + k] = S.t[k];
    for (int r = 0; r < 2; r++) {
      a.out.iters[2 * t + r] = sh.iters[r];
      a.out.chi2[2 * t + r] = sh.chi2[r];
      a.out.lambda[2 * t + r] = sh.lambda[r];
      if (a.out.trials)
        for (int k = 0; k < kMaxIts; k++) a.out.trials[(2 * (int64_t)t + r) * kMaxIts + k] = sh.trials[r][k];
    }
  }
}

// vpMapPointMatches of ComputeSim3 (src/cLoopClosing.cpp:354-369)
__global__ __launch_bounds__(256) void k_sim3_merge(int64_t n, const int32_t* __restrict__ bow,
                                                    const uint8_t* __restrict__ inlier,
                                                    const int32_t* __restrict__ fresh, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = fresh[i];
  out[i] = inlier[i] != 0 ? bow[i] : f >= 0 ? f : -1;
}

using host::bad_arg;

static int check_opts(const mcs_sim3_opt_options* o) {
  if (!o) return bad_arg("optimize sim3: null options");
  for (int its : {o->its_round1, o->its_clean, o->its_culled})
    if (its < 0 || its > kMaxIts) return bad_arg("optimize sim3: iteration counts must lie in [0, 16]");
  if (o->max_trials < 1 || o->max_trials > kMaxTrials) return bad_arg("optimize sim3: max_trials must lie in [1, 64]");
  if (!(o->std_sim > 0.0) || !std::isfinite(o->std_sim)) return bad_arg("optimize sim3: std_sim must be positive");
  if (o->flags & ~MCS_SIM3OPT_OWN_CAMERA) return bad_arg("optimize sim3: unknown flag");
  return MCS_OK;
}

// host = the host-buffer form: the pointers of `out` are nullable there
static int check_call(const mcs_fuse_targets* k1, const mcs_sim3_points* p1, const mcs_fuse_targets* k2,
                      const mcs_sim3_points* p2, const void* m12, const void* ok1, const void* ok2, const void* f2,
                      const void* is1, const void* s2, const void* s12, const void* R12, const void* t12,
                      const mcs_sim3_opt_options* o, const mcs_sim3_opt_out* out, bool host) {
  if (!k1 || !k2) return bad_arg("optimize sim3: null keyframe set");
  if (k1->n_targets != 1) return bad_arg("optimize sim3: kf1 must be a set of exactly one keyframe");
  if (k1->n_cams < 1 || k1->n_cams > kMaxCams || k1->n_cams != k2->n_cams || k1->n_levels != k2->n_levels)
    return bad_arg("optimize sim3: 1 to 8 cameras; n_cams and n_levels of kf1 and kf2s must agree (shared rig)");
  if (k2->n_targets < 0 || k1->n_kp_total < 0 || k2->n_kp_total < 0 || k1->n_levels < 1)
    return bad_arg("optimize sim3: negative count or empty pyramid");
  if (k1->n_kp_total >= kMaxKp) return bad_arg("optimize sim3: keypoints per keyframe must be below 2^19");
  if (!p1 || !p2 || !out) return bad_arg("optimize sim3: null points / outputs");
  if (p1->n != k1->n_kp_total || p2->n != k2->n_kp_total)
    return bad_arg("optimize sim3: the points must hold one slot per keypoint of their set");
  if (int rc = check_opts(o)) return rc;
  if ((int64_t)k2->n_targets * std::max(k1->n_kp_total, 1) >= INT_MAX / 2)
    return bad_arg("optimize sim3: batch too large for one launch");
  if (k2->n_targets == 0) return MCS_OK;
  for (const mcs_fuse_targets* k : {k1, k2})
    if (!k->off || !k->m_t || !k->m_c || !k->cam || (k->n_kp_total > 0 && (!k->kp_xy || !k->kp_octave || !k->kp_cam)))
      return bad_arg("optimize sim3: null buffer");
  if (!is1 || !s2 || !s12 || !R12 || !t12) return bad_arg("optimize sim3: null buffer");
  if (k1->n_kp_total > 0 && (!p1->pos || !m12 || !ok1)) return bad_arg("optimize sim3: null buffer");
  if (k2->n_kp_total > 0 && (!p2->pos || !ok2 || !f2)) return bad_arg("optimize sim3: null buffer");
  if (!host && (!out->n_in || !out->n_corr || !out->n_bad || !out->n_undefined || !out->s12 || !out->q12 ||
                !out->R12 || !out->t12 || !out->iters || !out->chi2 || !out->lambda))
    return bad_arg("optimize sim3: null buffer");
  return MCS_OK;
}

static Set dev_set(const mcs_fuse_targets* k) {
  return Set{k->n_kp_total, k->off, k->kp_xy, k->kp_octave, k->kp_cam, k->m_t, k->m_c, k->cam};
}

}  // namespace s3o
}  // namespace mcs

using namespace mcs;

struct mcs_sim3_opt_workspace {
  int device = 0, max_targets = 0, max_kp = 0;
  s3o::Row* rows = nullptr;    // [max_targets][max_kp]
};

extern "C" {

void mcs_sim3_opt_default_options(mcs_sim3_opt_options* o) {
  if (!o) return;
  o->std_sim = 4.0; o->its_round1 = 5; o->its_clean = 5; o->its_culled = 10;
  o->terminate_max_iter = 15; o->gain_threshold = 1e-6; o->tau = 1e-5; o->max_trials = 10; o->flags = 0;
}

int mcs_sim3_opt_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp, mcs_sim3_opt_workspace** out) {
  if (!out || max_targets < 1 || max_kp < 1 || max_kp >= s3o::kMaxKp || (int64_t)max_targets * max_kp >= INT_MAX / 2) {
    set_error("optimize sim3 workspace: bad argument");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "optimize sim3 workspace")) return rc;
  mcs_sim3_opt_workspace* w = new mcs_sim3_opt_workspace;
  w->device = device;
  w->max_targets = max_targets;
  w->max_kp = max_kp;
  hipError_t e = hipMalloc((void**)&w->rows, (size_t)max_targets * max_kp * sizeof(s3o::Row));
  if (e != hipSuccess) {
    mcs_sim3_opt_workspace_destroy(w);
    set_hip_error(e, "optimize sim3 workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_sim3_opt_workspace_destroy(mcs_sim3_opt_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->rows) (void)hipFree(w->rows);
  delete w;
}

int mcs_optimize_sim3_device(mcs_sim3_opt_workspace* ws, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                             const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2, int32_t* d_matches12,
                             const uint8_t* d_ok1, const uint8_t* d_ok2, const int32_t* d_first2,
                             const double* d_inv_sigma2_1, const double* d_sigma2_2, const double* d_s12,
                             const double* d_R12, const double* d_t12, const mcs_sim3_opt_options* opts,
                             const mcs_sim3_opt_out* out, void* stream) {
  int rc = s3o::check_call(kf1, pts1, kf2s, pts2, d_matches12, d_ok1, d_ok2, d_first2, d_inv_sigma2_1, d_sigma2_2,
                           d_s12, d_R12, d_t12, opts, out, false);
  if (rc) return rc;
  const int T = kf2s->n_targets, n1 = kf1->n_kp_total;
  if (T == 0) return MCS_OK;
  if (ws && (T > ws->max_targets || n1 > ws->max_kp)) {
    set_error("optimize sim3: more candidates or keypoints than the workspace holds");
    return MCS_ERR_ARG;
  }
  mcs_sim3_opt_workspace* tmp = nullptr;
  if (!ws) {
    int dev = 0;
    MCS_HIP_CHECK(hipGetDevice(&dev));
    rc = mcs_sim3_opt_workspace_create(dev, T, std::max(n1, 1), &tmp);
    if (rc) return rc;
    ws = tmp;
  } else {
    MCS_HIP_CHECK(hipSetDevice(ws->device));
  }
  s3o::Args a;
  a.k1 = s3o::dev_set(kf1); a.k2 = s3o::dev_set(kf2s);
  a.pos1 = pts1->pos; a.pos2 = pts2->pos;
  a.matches12 = d_matches12; a.ok1 = d_ok1; a.ok2 = d_ok2; a.first2 = d_first2;
  a.inv_sigma2_1 = d_inv_sigma2_1; a.sigma2_2 = d_sigma2_2;
  a.s12 = d_s12; a.R12 = d_R12; a.t12 = d_t12;
  a.o = *opts;
  a.out = s3o::Out{out->n_in, out->n_corr, out->n_bad, out->n_undefined, out->s12, out->q12, out->R12, out->t12,
                   out->iters, out->chi2, out->lambda, out->trials, out->edge_chi2};
  a.rows = ws->rows;
  a.n1 = n1; a.C = kf1->n_cams; a.L = kf1->n_levels;
  hipLaunchKernelGGL(s3o::k_sim3_opt, dim3(T), dim3(s3o::kNT), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    mcs_sim3_opt_workspace_destroy(tmp);
  }
  MCS_HIP_CHECK(e);
  return MCS_OK;
}

int mcs_sim3_merge_matches_device(const int32_t* d_bow12, const uint8_t* d_inlier, const int32_t* d_new12, int32_t T,
                                  int32_t n1, int32_t* d_matches12, void* stream) {
  if (T < 0 || n1 < 0 || (int64_t)T * n1 >= (int64_t)INT_MAX) return host::bad_arg("sim3 merge: bad counts");
  const int64_t n = (int64_t)T * n1;
  if (n == 0) return MCS_OK;
  if (!d_bow12 || !d_inlier || !d_new12 || !d_matches12) return host::bad_arg("sim3 merge: null buffer");
  hipLaunchKernelGGL(s3o::k_sim3_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     d_bow12, d_inlier, d_new12, d_matches12);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_optimize_sim3(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                      const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2, int32_t* matches12,
                      const uint8_t* ok1, const uint8_t* ok2, const int32_t* first2, const double* inv_sigma2_1,
                      const double* sigma2_2, const double* s12, const double* R12, const double* t12,
                      const mcs_sim3_opt_options* opts, const mcs_sim3_opt_out* out) {
  int rc = s3o::check_call(kf1, pts1, kf2s, pts2, matches12, ok1, ok2, first2, inv_sigma2_1, sigma2_2, s12, R12, t12,
                           opts, out, true);
  if (rc) return rc;
  const int T = kf2s->n_targets;
  if (T == 0) return MCS_OK;
  for (const mcs_fuse_targets* k : {kf1, kf2s})
    if ((rc = host::check_set_offsets(k->off, k->n_targets, k->n_kp_total, 0, "optimize sim3"))) return rc;
  if ((rc = host::open_device(device, "optimize sim3"))) return rc;
  host::DevBufs B;
  const size_t n1 = (size_t)kf1->n_kp_total, n2 = (size_t)kf2s->n_kp_total, nr = (size_t)T * n1, L = (size_t)kf1->n_levels;
  auto upload = [&](const mcs_fuse_targets* k, const mcs_sim3_points* p, mcs_fuse_targets* d, mcs_sim3_points* dp) {
    *dp = *p;
    dp->pos = B.up(p->pos, 3 * (size_t)k->n_kp_total);
    dp->dist = nullptr; dp->desc = dp->mask = nullptr;
    const int r = host::upload_kf_set(B, *k, host::kKfCam, d);   // no search: neither grids nor descriptors
    d->kp_xy = B.up(k->kp_xy, 2 * (size_t)k->n_kp_total);
    return r;
  };
  mcs_fuse_targets d1, d2;
  mcs_sim3_points dp1, dp2;
  if ((rc = upload(kf1, pts1, &d1, &dp1)) || (rc = upload(kf2s, pts2, &d2, &dp2))) return rc;
  int32_t* d_m12 = B.up(matches12, nr);
  mcs_sim3_opt_out d{};
  d.n_in = B.alloc<int32_t>(T); d.n_corr = B.alloc<int32_t>(T); d.n_bad = B.alloc<int32_t>(T);
  d.n_undefined = B.alloc<int32_t>(T);
  d.s12 = B.alloc<double>(T); d.q12 = B.alloc<double>(4 * (size_t)T); d.R12 = B.alloc<double>(9 * (size_t)T);
  d.t12 = B.alloc<double>(3 * (size_t)T);
  d.iters = B.alloc<int32_t>(2 * (size_t)T); d.chi2 = B.alloc<double>(2 * (size_t)T);
  d.lambda = B.alloc<double>(2 * (size_t)T);
  d.trials = out->trials ? B.alloc<int32_t>(2 * (size_t)T * s3o::kMaxIts) : nullptr;
  d.edge_chi2 = out->edge_chi2 ? B.alloc<double>(2 * nr) : nullptr;
  const uint8_t* d_ok1 = B.up(ok1, n1);
  const uint8_t* d_ok2 = B.up(ok2, n2);
  const int32_t* d_f2 = B.up(first2, n2);
  const double* d_is1 = B.up(inv_sigma2_1, L);
  const double* d_s2 = B.up(sigma2_2, L);
  const double* d_s = B.up(s12, (size_t)T);
  const double* d_R = B.up(R12, 9 * (size_t)T);
  const double* d_t = B.up(t12, 3 * (size_t)T);
  if (B.err != hipSuccess) { set_hip_error(B.err, "optimize sim3 upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if ((rc = mcs_optimize_sim3_device(nullptr, &d1, &dp1, &d2, &dp2, d_m12, d_ok1, d_ok2, d_f2, d_is1, d_s2, d_s, d_R,
                                     d_t, opts, &d, nullptr)))
    return rc;
  MCS_HIP_CHECK(hipDeviceSynchronize());
  B.down(matches12, d_m12, nr);
  B.down(out->n_in, d.n_in, (size_t)T);
  B.down(out->n_corr, d.n_corr, (size_t)T);
  B.down(out->n_bad, d.n_bad, (size_t)T);
  B.down(out->n_undefined, d.n_undefined, (size_t)T);
  B.down(out->s12, d.s12, (size_t)T);
  B.down(out->q12, d.q12, 4 * (size_t)T);
  B.down(out->R12, d.R12, 9 * (size_t)T);
  B.down(out->t12, d.t12, 3 * (size_t)T);
  B.down(out->iters, d.iters, 2 * (size_t)T);
  B.down(out->chi2, d.chi2, 2 * (size_t)T);
  B.down(out->lambda, d.lambda, 2 * (size_t)T);
  B.down(out->trials, d.trials, 2 * (size_t)T * s3o::kMaxIts);
  B.down(out->edge_chi2, d.edge_chi2, 2 * nr);
  if (B.err != hipSuccess) { set_hip_error(B.err, "optimize sim3 download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
