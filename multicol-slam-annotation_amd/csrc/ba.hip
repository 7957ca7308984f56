// MultiCol bundle adjustment on gfx950: per-edge residual/Jacobian, Huber-weighted
// normal equations, Schur complement onto the MultiKeyFrame poses, LDL^T of the reduced
// camera system, point back-substitution and the Levenberg-Marquardt control of g2o.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   EdgeProjectXYZ2MCS::computeError / linearizeOplus   src/g2o_MultiCol_vertices_edges.cpp:32-129
//   WorldToImg                                          src/cam_model_omni.cpp:147-163
//   cayley2rot / cayley2hom / invMat                    include/misc.h:134-226, src/cConverter.cpp:31-44
//   BaseMultiEdge::constructQuadraticForm + Huber       ThirdParty/g2o/g2o/core/base_multi_edge.hpp:36-48,171-222
//   BlockSolver<6,3>::buildSystem / solve (Schur)       ThirdParty/g2o/g2o/core/block_solver.hpp:354-604
//   OptimizationAlgorithmLevenberg::solve               ThirdParty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   SparseOptimizer::optimize / TerminateAction         sparse_optimizer.cpp:354-435, sparse_optimizer_terminate_action.cpp:21-72
//   cOptimizer::LocalBundleAdjustment rounds            src/cOptimizer.cpp:771-903
//
// Every reduction runs in a fixed order (no float atomics): results are bitwise
// reproducible run to run.  The LM accept/reject decision needs two scalars per trial
// (robust chi2, model decrease); lm_control.hpp decides, on the device or driven from the host.
// This file is the C-ABI and the LocalBA driver; the rest of the translation unit is in the
// ba_*.hpp headers, one per concern.
#include "ba_optimizer.hpp"
#include <new>

// cOptimizer::LocalBundleAdjustment's two rounds (src/cOptimizer.cpp:771-903) over Optimizer:
// round 1, the culling pass, round 2 at the culled levels, the final culling pass and the
// write-back flags.  The culling runs on the device when both rounds' LM loops do.
namespace {

struct LocalBa {
  mcs_ba_ctx* c;
  const mcs_ba_problem* p;
  double* poses; double* points;
  uint8_t* edge_inlier; uint8_t* point_write; int32_t* write_back;
  volatile int32_t* stop_flag;   // the caller's (nullable)
  volatile int32_t* sf;          // the force-stop flag both rounds share
  mcs_ba_report* r1; mcs_ba_report* r2;
  mcs_ba_options o;
  // cMapPoint bookkeeping: observations left (good-keyframe edges + observations from bad
  // keyframes) and the bad flag EraseObservation raises below two (src/cMapPoint.cpp:120-152)
  std::vector<uint8_t> level;
  std::vector<double> chi;
  std::vector<int32_t> obs_left, edges_left;
  std::vector<uint8_t> pt_bad;

  void init(const int32_t* point_extra_obs) {
    level.assign(p->n_edges, 0);
    chi.resize(p->n_edges);
    obs_left.assign(p->n_points, 0);
    edges_left.assign(p->n_points, 0);
    pt_bad.assign(p->n_points, 0);
    for (int e = 0; e < p->n_edges; e++) edges_left[p->edge_point[e]]++;
    for (int i = 0; i < p->n_points; i++)
      obs_left[i] = edges_left[i] + (point_extra_obs ? point_extra_obs[i] : 0);
    if (point_write) std::memset(point_write, 0, (size_t)p->n_points);
    *write_back = 0;
    for (int e = 0; e < p->n_edges; e++) edge_inlier[e] = 1;
  }
  // culling pass (:798-817, :830-849): edges in vpEdges order, a bad point's edges skipped
  void cull(bool disable) {
    const double huberK2 = p->huber_delta * p->huber_delta;
    for (int e = 0; e < p->n_edges; e++) {
      const int pt = p->edge_point[e];
      if (!edge_inlier[e] || pt_bad[pt] || !(chi[e] > huberK2)) continue;
      edge_inlier[e] = 0;
      if (disable) level[e] = 1;
      edges_left[pt]--;
      if (--obs_left[pt] < 2) pt_bad[pt] = 1;
    }
  }
  // the host-culled rounds' end (:885-902): the points to write back are those not bad, with
  // TotalNrObservations() > 1 and >= 2 vertex edges
  int write_out() {
    *write_back = 1;
    if (point_write) {
      std::vector<int32_t> edges_all(p->n_points, 0);
      for (int e = 0; e < p->n_edges; e++) edges_all[p->edge_point[e]]++;
      for (int i = 0; i < p->n_points; i++)
        point_write[i] = !pt_bad[i] && edges_left[i] > 1 && edges_all[i] >= 2;
    }
    return MCS_OK;
  }

  // Round 2 at `level` with the culling on the host: on round 1's device state (reuse), or
  // rebuilt from scratch when a pose left the system; then the final culling pass
  int round2_host(Optimizer* reuse) {
    int rc = reuse ? reuse->run(&o, poses, points, chi.data(), sf, r2)
                   : mcs_ba_optimize(c, p, &o, poses, points, level.data(), chi.data(), sf, r2);
    if (rc) return rc;
    if (r2->n_active_poses + r2->n_active_points == 0) return MCS_OK;   // :822-826
    cull(false);
    return write_out();
  }

  // The culling passes run on the device between and after the rounds (k_lba_cull): round 2
  // follows round 1 without a download, and only the results come back.
  int device_culled(Optimizer& opt, const int32_t* point_extra_obs) {
    opt.lba.on = true;
    opt.lba.extra = point_extra_obs;
    int rc = opt.setup(poses, points, level.data(), nullptr);
    if (rc) return rc;
    opt.lba.tail = Optimizer::LbaTail::Round1;
    rc = opt.run(&o, poses, points, nullptr, sf, r1);
    if (rc) return rc;
    if (r1->n_active_poses + r1->n_active_points == 0) return MCS_OK;   // :784-788 (nothing moved)
    if (stop_flag && *stop_flag) return opt.fetch_state(poses, points);   // bDoMore = false (:790-794)
    o.max_iterations = 15;                                    // :819-820
    if (opt.lba.res[1]) return pose_left(opt);
    opt.remask_device();
    // round 2's report counts (run_device) decide whether the final culling runs (:822-826)
    const bool empty2 = (opt.s.np + opt.nl_glob) == 0;
    opt.lba.tail = empty2 ? Optimizer::LbaTail::Round2NoCull : Optimizer::LbaTail::Round2;
    opt.lba.inlier_out = edge_inlier;
    opt.lba.pwrite_out = empty2 ? nullptr : point_write;
    rc = opt.run(&o, poses, points, nullptr, sf, r2);
    if (rc) return rc;
    if (r2->n_active_poses + r2->n_active_points == 0) return MCS_OK;   // :822-826
    *write_back = 1;
    return MCS_OK;
  }

  // device_culled's fallback: an active pose lost every edge.  g2o's initializeOptimization
  // drops it from the system, so round 2 rebuilds from scratch on the host's copy of round 1's state
  int pose_left(Optimizer& opt) {
    std::vector<int32_t> obs_d(p->n_points), el_d(p->n_points);
    if (int rc = opt.lba_fetch(poses, points, level.data(), edge_inlier, obs_d.data(), el_d.data(), pt_bad.data()))
      return rc;
    for (int i = 0; i < p->n_points; i++)
      if (edges_left[i] > 0) { obs_left[i] = obs_d[i]; edges_left[i] = el_d[i]; }
    return round2_host(nullptr);
  }

  // Both culling passes on the host (a host-driven LM loop: timing, or a long trace).  Round 1
  // builds the structure and uploads the problem; round 2 (the same graph with the culled edges
  // at level 1) reuses both (Optimizer::remask) unless a pose left the system
  int host_culled(Optimizer& opt) {
    int rc = opt.setup(poses, points, level.data(), nullptr);
    if (rc) return rc;
    rc = opt.run(&o, poses, points, chi.data(), sf, r1);
    if (rc) return rc;
    // optimize() returns -1 == OptimizationAlgorithm::Fail only for an empty active graph
    if (r1->n_active_poses + r1->n_active_points == 0) return MCS_OK;   // :784-788
    if (stop_flag && *stop_flag) return MCS_OK;               // bDoMore = false (:790-794)
    {
      HostClock hc;
      cull(true);
      hc.mark(c->host_ms, 4);
    }
    o.max_iterations = 15;                                    // :819-820
    rc = opt.remask(level.data());
    if (rc < 0) return rc;
    return round2_host(rc == 0 ? &opt : nullptr);
  }
};

}  // namespace

extern "C" {

void mcs_ba_default_options(mcs_ba_options* o) {
  if (!o) return;
  o->max_iterations = 10; o->gain_threshold = 1e-6; o->terminate_max_iter = 15;
  o->max_trials = 10; o->tau = 1e-5;
}

int mcs_ba_create(int32_t device, mcs_ba_ctx** out) {
  if (!out) return MCS_ERR_ARG;
  *out = nullptr;
  if (int rc = host::open_device(device, "ba_create")) return rc;
  mcs_ba_ctx* c = new (std::nothrow) mcs_ba_ctx();
  if (!c) return MCS_ERR_ARG;
  c->device = device;
  MCS_HIP_CHECK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
  MCS_HIP_CHECK(hipHostMalloc((void**)&c->pinned, 64, hipHostMallocDefault));
  MCS_HIP_CHECK(hipHostMalloc((void**)&c->pinned_i, 64, hipHostMallocMapped));   // k_lba_count writes it
  MCS_HIP_CHECK(hipHostMalloc((void**)&c->sig, sizeof(TrialSig), hipHostMallocCoherent | hipHostMallocMapped));
  std::memset((void*)c->sig, 0, sizeof(TrialSig));
  MCS_HIP_CHECK(hipHostMalloc((void**)&c->lsig, sizeof(LmSig), hipHostMallocCoherent | hipHostMallocMapped));
  MCS_HIP_CHECK(hipHostMalloc((void**)&c->pinned_ctl, sizeof(LmCtl), hipHostMallocMapped));   // k_edges_end writes it
  std::memset((void*)c->lsig, 0, sizeof(LmSig));
  *out = c;
  return MCS_OK;
}

void mcs_ba_destroy(mcs_ba_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->st);
  c->release();
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->pinned_i) (void)hipHostFree(c->pinned_i);
  if (c->sig) (void)hipHostFree(c->sig);
  if (c->lsig) (void)hipHostFree(c->lsig);
  if (c->pinned_ctl) (void)hipHostFree(c->pinned_ctl);
  c->stage.release();
  c->stage2.release();
  if (c->st) (void)hipStreamDestroy(c->st);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  delete c;
}

int mcs_ba_enable_timing(mcs_ba_ctx* c, int32_t on) {
  if (!c) return MCS_ERR_ARG;
  MCS_HIP_CHECK(hipSetDevice(c->device));
  if (on && !c->ev[0])
    for (auto& e : c->ev) MCS_HIP_CHECK(hipEventCreate(&e));
  c->timing = on != 0;
  return MCS_OK;
}

int mcs_ba_read_timing(mcs_ba_ctx* c, double* ms, int32_t* n_iterations, int32_t* n_trials,
                       int32_t* last_n, int32_t reset) {
  if (!c) return MCS_ERR_ARG;
  for (int k = 0; k < MCS_BA_NSTAGES; k++) if (ms) ms[k] = c->acc_ms[k];
  if (n_iterations) *n_iterations = c->n_iter;
  if (n_trials) *n_trials = c->n_trial;
  if (last_n) *last_n = c->last_n;
  if (reset) {
    for (double& v : c->acc_ms) v = 0.0;
    c->n_iter = c->n_trial = 0;
  }
  return MCS_OK;
}

int mcs_ba_read_solve_shape(mcs_ba_ctx* c, int32_t* n, int32_t* tiles, int32_t* band, int32_t* pipelined) {
  if (!c) return MCS_ERR_ARG;
  if (n) *n = c->shape_n;
  if (tiles) *tiles = c->shape_T;
  if (band) *band = c->shape_band;
  if (pipelined) *pipelined = c->shape_pipe;
  return MCS_OK;
}

int mcs_ba_set_ldlt_mode(mcs_ba_ctx* c, int32_t mode) {
  if (!c || mode < 0 || mode > 2) return MCS_ERR_ARG;
  c->ldlt_mode = mode;
  return MCS_OK;
}

int mcs_ba_check_structure(mcs_ba_ctx* c, const mcs_ba_problem* p, const uint8_t* edge_level) {
  if (!c || !p) return MCS_ERR_ARG;
  Optimizer opt(c, p, false);
  int rc = opt.setup(p->poses, p->points, edge_level, nullptr);
  if (rc) return rc;
  HostStruct h = c->hs;
  build_pairs_host(*p, h);
  const int nb = opt.nblk;
  std::vector<int32_t> pr_ptr(nb + 1), items;
  int32_t nitem = 0;
  MCS_HIP_CHECK(hipMemcpyAsync(pr_ptr.data(), opt.d.pr_ptr, 4 * (size_t)(nb + 1), hipMemcpyDeviceToHost, c->st));
  MCS_HIP_CHECK(hipMemcpyAsync(&nitem, opt.d.nitem, 4, hipMemcpyDeviceToHost, c->st));
  MCS_HIP_CHECK(hipStreamSynchronize(c->st));
  int64_t bad = 0;
  for (int b = 0; b <= nb; b++) bad += pr_ptr[b] != h.pr_ptr[b];
  if (bad) return (int)std::min<int64_t>(bad, INT32_MAX);
  const int np_ = pr_ptr[nb];
  std::vector<uint2> pr(std::max(1, np_));
  if (np_) MCS_HIP_CHECK(hipMemcpy(pr.data(), opt.d.pr, 8 * (size_t)np_, hipMemcpyDeviceToHost));
  for (int q = 0; q < np_; q++) bad += ((int)pr[q].x != h.pr_e1[q]) + ((int)pr[q].y != h.pr_e2[q]);
  bad += nitem != (int32_t)h.it_blk.size();
  if (!bad && nitem > 0) {
    std::vector<int32_t> v(nitem);
    const int32_t* src[4] = {opt.d.it_blk, opt.d.it_chunk, opt.d.it_slot, opt.it_nch_dev};
    const std::vector<int32_t>* ref[4] = {&h.it_blk, &h.it_chunk, &h.it_slot, &h.it_nch};
    for (int k = 0; k < 4; k++) {
      MCS_HIP_CHECK(hipMemcpy(v.data(), src[k], 4 * (size_t)nitem, hipMemcpyDeviceToHost));
      for (int i = 0; i < nitem; i++) bad += v[i] != (*ref[k])[i];
    }
  }
  return (int)std::min<int64_t>(bad, INT32_MAX);
}

int mcs_ba_read_host_timing(mcs_ba_ctx* c, double* ms, int32_t* n_calls, int32_t reset) {
  if (!c) return MCS_ERR_ARG;
  for (int k = 0; k < MCS_BA_NHOST; k++) if (ms) ms[k] = c->host_ms[k];
  if (n_calls) *n_calls = c->host_calls;
  if (reset) {
    for (double& v : c->host_ms) v = 0.0;
    c->host_calls = 0;
  }
  return MCS_OK;
}

int mcs_ba_optimize(mcs_ba_ctx* c, const mcs_ba_problem* p, const mcs_ba_options* o,
                    double* poses, double* points, const uint8_t* edge_level, double* edge_chi2,
                    volatile int32_t* stop_flag, mcs_ba_report* rep) {
  return optimize_impl(c, p, o, poses, points, edge_level, edge_chi2, stop_flag, rep, nullptr, false);
}

int64_t mcs_ba_xchg_doubles(int32_t n_poses) { return xchg_doubles(n_poses); }

int mcs_ba_optimize_sharded(mcs_ba_ctx* c, const mcs_ba_problem* p, const mcs_ba_options* o,
                            double* poses, double* points, const uint8_t* edge_level,
                            double* edge_chi2, volatile int32_t* stop_flag, mcs_ba_report* rep,
                            const mcs_ba_shard* shard) {
  return optimize_impl(c, p, o, poses, points, edge_level, edge_chi2, stop_flag, rep, shard, false);
}

int mcs_global_ba(mcs_ba_ctx* c, const mcs_ba_problem* p, int32_t pose_only, double* poses,
                  double* points, volatile int32_t* stop_flag, mcs_ba_report* rep,
                  const mcs_ba_shard* shard) {
  mcs_ba_options o;
  mcs_ba_default_options(&o);
  o.max_iterations = 15;   // optimizer.optimize(15) (src/cOptimizer.cpp:241)
  return optimize_impl(c, p, &o, poses, points, nullptr, nullptr, stop_flag, rep, shard, pose_only != 0);
}

int mcs_local_ba_ex(mcs_ba_ctx* c, const mcs_ba_problem* p, const int32_t* point_extra_obs,
                    double* poses, double* points, uint8_t* edge_inlier, uint8_t* point_write,
                    int32_t* write_back, volatile int32_t* stop_flag, mcs_ba_report* r1,
                    mcs_ba_report* r2) {
  if (!c || !p || !poses || !points || !edge_inlier || !write_back) return MCS_ERR_ARG;
  // pbStopFlag == NULL: the terminate action raises its own auxiliary flag and g2o keeps it
  // installed as the force-stop flag, so a round 1 that converged leaves round 2 with zero
  // iterations (sparse_optimizer_terminate_action.cpp:64-72, sparse_optimizer.cpp:376)
  volatile int32_t aux = 0;
  mcs_ba_report t1{}, t2{};
  LocalBa lb{c, p, poses, points, edge_inlier, point_write, write_back, stop_flag,
             stop_flag ? stop_flag : &aux, r1 ? r1 : &t1, r2 ? r2 : &t2};
  mcs_ba_default_options(&lb.o);
  lb.init(point_extra_obs);
  if (stop_flag && *stop_flag) return MCS_OK;               // :771-773
  lb.o.max_iterations = 10;
  Optimizer opt(c, p, false);
  if (opt.device_driven(&lb.o, lb.r1) && opt.device_driven(&lb.o, lb.r2))
    return lb.device_culled(opt, point_extra_obs);
  return lb.host_culled(opt);
}

int mcs_local_ba(mcs_ba_ctx* c, const mcs_ba_problem* p, double* poses, double* points,
                 uint8_t* edge_inlier, int32_t* write_back, volatile int32_t* stop_flag,
                 mcs_ba_report* r1, mcs_ba_report* r2) {
  return mcs_local_ba_ex(c, p, nullptr, poses, points, edge_inlier, nullptr, write_back, stop_flag,
                         r1, r2);
}

int mcs_pose_optimization(mcs_ba_ctx* c, const mcs_ba_problem* p, double* pose, uint8_t* outlier,
                          int32_t* n_good, double* bad_ratio, mcs_ba_report* r1, mcs_ba_report* r2) {
  if (!c || !p || !pose || !n_good || (p->n_edges > 0 && !outlier)) return MCS_ERR_ARG;
  if (p->n_poses != 1) {
    set_error("PoseOptimization: the problem must hold exactly one pose vertex");
    return MCS_ERR_ARG;
  }
  mcs_ba_problem q = *p;
  const uint8_t not_fixed = 0;
  q.pose_fixed = &not_fixed;                                // vSE3->setFixed(false) (:299)
  mcs_ba_options o;
  mcs_ba_default_options(&o);                               // gain 1e-6, max 15 (:290-291)
  o.max_iterations = 10;                                    // optimize(10) (:434, :457)
  const double th2 = p->huber_delta * p->huber_delta;      // thHuber = 1.345 * mult (:344)
  const int N = p->n_edges;
  std::vector<uint8_t> level(N, 0);
  std::vector<double> chi(N), pts(p->points, p->points + 3 * (size_t)p->n_points);
  // no setForceStopFlag: the terminate action's own flag is shared by both optimize() calls
  volatile int32_t aux = 0;
  mcs_ba_report t1{}, t2{};
  int rc = optimize_impl(c, &q, &o, pose, pts.data(), level.data(), chi.data(), &aux,
                         r1 ? r1 : &t1, nullptr, true);    // map points fixed (:382)
  if (rc) return rc;
  int nBad = 0;
  for (int e = 0; e < N; e++) {                             // :439-454
    if (chi[e] > th2) { outlier[e] = 1; level[e] = 1; nBad++; }
    else outlier[e] = 0;
  }
  rc = optimize_impl(c, &q, &o, pose, pts.data(), level.data(), chi.data(), &aux,
                     r2 ? r2 : &t2, nullptr, true);
  if (rc) return rc;
  for (int e = 0; e < N; e++) {                             // :460-474
    if (level[e]) continue;
    if (chi[e] > th2) { outlier[e] = 1; nBad++; }
    else outlier[e] = 0;
  }
  *n_good = N - nBad;                                       // return value (:485)
  if (bad_ratio) *bad_ratio = N > 0 ? (double)nBad / N : 0.0;   // `inliers` (:481-483)
  return MCS_OK;
}

int mcs_ba_linearize(mcs_ba_ctx* c, const mcs_ba_problem* p, double* err, double* jac_pose,
                     double* jac_point) {
  if (!c || !p || !err || !jac_pose || !jac_point) return MCS_ERR_ARG;
  MCS_HIP_CHECK(hipSetDevice(c->device));
  c->free_all();
  // the problem through the optimizer's packed upload; no active list: k_edges takes every edge
  Optimizer opt(c, p, false);
  const int NE = opt.NE = p->n_edges;
  double *poses_bk = nullptr, *points_bk = nullptr;
  Packer pk;
  opt.add_problem(pk, p->poses, p->points, &poses_bk, &points_bk);
  opt.he = pk.flush(c);
  Dev& d = opt.d;
  d.delta = p->huber_delta; d.dsqr = huber_dsqr(p->huber_delta);
  d.poses = opt.d_poses; d.points = opt.d_points;
  d.nae = NE;
  d.err = opt.dz(2 * (size_t)NE); d.w = opt.dz(NE); d.jp = opt.dz(12 * (size_t)NE); d.jl = opt.dz(6 * (size_t)NE);
  d.chi = opt.dz(NE); d.rchi = opt.dz(NE);
  if (opt.he != hipSuccess) { set_hip_error(opt.he, "BA linearize upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  hipLaunchKernelGGL(k_edges, dim3(gb(NE)), dim3(256), 0, c->st, d, 1);
  MCS_HIP_CHECK(hipMemcpyAsync(err, d.err, 16 * (size_t)NE, hipMemcpyDeviceToHost, c->st));
  MCS_HIP_CHECK(hipMemcpyAsync(jac_pose, d.jp, 96 * (size_t)NE, hipMemcpyDeviceToHost, c->st));
  MCS_HIP_CHECK(hipMemcpyAsync(jac_point, d.jl, 48 * (size_t)NE, hipMemcpyDeviceToHost, c->st));
  MCS_HIP_CHECK(hipStreamSynchronize(c->st));
  return MCS_OK;
}

int mcs_ba_lm_replay(int32_t device, const mcs_ba_options* o, const double* in3, const double* trials,
                     int32_t n, double* out, int32_t* n_out) {
  if (!o || !in3 || (n > 0 && (!trials || !out)) || !n_out || n < 0) {
    set_error("lm_replay: null argument or n < 0");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "lm_replay")) return rc;
  LmCtl h0;
  lm_init(h0, *o);
  h0.done = o->max_iterations <= 0 ? 1 : 0;
  host::DevBufs B;
  LmCtl* dc = B.up(&h0, 1);
  LmSig* ds = B.alloc<LmSig>(1);
  const double* din = B.up(in3, 3);
  const double* dtr = B.up(trials, 4 * (size_t)n);
  double* dout = B.alloc<double>(10 * (size_t)n);
  int32_t* dn = B.alloc<int32_t>(1);
  if (B.err == hipSuccess) B.err = hipMemset(ds, 0, sizeof(LmSig));
  if (B.err == hipSuccess) B.err = hipMemset(dn, 0, 4);
  if (B.err != hipSuccess) { set_hip_error(B.err, "lm_replay upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  hipLaunchKernelGGL(k_lm_replay, dim3(1), dim3(64), 0, 0, dc, ds, din, dtr, n, dout, dn);
  MCS_HIP_CHECK(hipGetLastError());
  MCS_HIP_CHECK(hipDeviceSynchronize());
  int32_t m = 0;
  B.down(&m, dn, 1);
  B.down(out, dout, 10 * (size_t)m);
  if (B.err != hipSuccess) { set_hip_error(B.err, "lm_replay download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  *n_out = m;
  return MCS_OK;
}

int mcs_ba_huber_eval(int32_t device, const double* e, int32_t n, double delta, double* rho0, double* rho1) {
  if (n < 0 || (n > 0 && (!e || !rho0 || !rho1))) {
    set_error("huber_eval: null argument or n < 0");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "huber_eval")) return rc;
  if (n == 0) return MCS_OK;
  host::DevBufs B;
  const double* de = B.up(e, (size_t)n);
  double* d0 = B.alloc<double>((size_t)n);
  double* d1 = B.alloc<double>((size_t)n);
  if (B.err != hipSuccess) { set_hip_error(B.err, "huber_eval upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  hipLaunchKernelGGL(k_huber_eval, dim3((n + 255) / 256), dim3(256), 0, 0, de, n, delta, huber_dsqr(delta), d0, d1);
  MCS_HIP_CHECK(hipGetLastError());
  B.down(rho0, d0, (size_t)n);
  B.down(rho1, d1, (size_t)n);
  if (B.err != hipSuccess) { set_hip_error(B.err, "huber_eval download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

int mcs_ba_point_block_eval(int32_t device, const double* H, double lambda, const double* b, const double* hpl,
                            int32_t n, double* Dinv, double* db, double* Y) {
  if (n < 0 || (n > 0 && (!H || !b || !hpl || !Dinv || !db || !Y))) {
    set_error("point_block_eval: null argument or n < 0");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "point_block_eval")) return rc;
  if (n == 0) return MCS_OK;
  const size_t N = (size_t)n;
  host::DevBufs B;
  const double* dH = B.up(H, 9 * N);
  const double* dB = B.up(b, 3 * N);
  const double* dP = B.up(hpl, 18 * N);
  double* dDi = B.alloc<double>(9 * N);
  double* dDb = B.alloc<double>(3 * N);
  double* dY = B.alloc<double>(18 * N);
  if (B.err != hipSuccess) { set_hip_error(B.err, "point_block_eval upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  hipLaunchKernelGGL(k_point_block_eval, dim3((n + 255) / 256), dim3(256), 0, 0, dH, lambda, dB, dP, n, dDi, dDb, dY);
  MCS_HIP_CHECK(hipGetLastError());
  B.down(Dinv, dDi, 9 * N);
  B.down(db, dDb, 3 * N);
  B.down(Y, dY, 18 * N);
  if (B.err != hipSuccess) { set_hip_error(B.err, "point_block_eval download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
