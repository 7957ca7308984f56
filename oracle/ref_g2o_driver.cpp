// ============================================================================
// REFERENCE DRIVER -- TEST INFRASTRUCTURE ONLY (never in the product, never committed built).
//
// Runs the reference's own g2o (compiled from its checkout by oracle/ref_g2o.mk):
// SparseOptimizer + BlockSolver_6_3 + LinearSolverEigen (Eigen's SimplicialLDLT) +
// OptimizationAlgorithmLevenberg + SparseOptimizerTerminateAction + RobustKernelHuber (or, as
// PoseOptimization sets it up, BlockSolverX + LinearSolverDense), on the
// graph shape of the MultiCol bundle adjustment: vertices Mt (6), point (3, marginalised),
// Mc (6, fixed), IO (17, fixed), all additive (oplus = estimate + update), and one multi-edge
// of dimension 2 over (Mt, point, Mc, IO).
//
// THE ONE SEAM: the edge's error and Jacobian are oracle_ba_edge (oracle/ba_oracle.cpp).  The
// reference's own edge needs OpenCV and cannot be compiled; its error text and its generated
// Jacobian are pinned elsewhere (mcsjacs1.npz, the computeError text).  Everything from
// initializeOptimization to the linear solve is the reference's binary.
//
// Graph handling follows what the reference's optimiser calls do: setLevel per edge,
// initializeOptimization(0), optimize(n), the terminate action as a post-iteration action,
// setForceStopFlag only when the caller has a flag, Huber through setDelta.
// ============================================================================
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <vector>

#include <g2o/core/base_multi_edge.h>
#include <g2o/core/base_vertex.h>
#include <g2o/core/block_solver.h>
#include <g2o/core/optimization_algorithm_levenberg.h>
#include <g2o/core/robust_kernel_impl.h>
#include <g2o/core/sparse_block_matrix.h>
#include <g2o/core/sparse_optimizer.h>
#include <g2o/core/sparse_optimizer_terminate_action.h>
#include <g2o/solvers/linear_solver_dense.h>
#include <g2o/solvers/linear_solver_eigen.h>

#include "../include/mcs_ba.h"

extern "C" int oracle_ba_edge(const double* pose, const double* X, const double* mc,
                              const double* cam, const double* meas, double* err, double* jp,
                              double* jl);

namespace {

template <int D>
struct AdditiveVertex : g2o::BaseVertex<D, Eigen::Matrix<double, D, 1>> {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  typedef Eigen::Matrix<double, D, 1> Vec;
  void setToOriginImpl() override { this->_estimate.setZero(); }
  void oplusImpl(const double* u) override {
    const Vec s = this->_estimate + Eigen::Map<const Vec>(u);
    this->setEstimate(s);
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};
struct VertexMt : AdditiveVertex<6> {};
struct VertexPoint : AdditiveVertex<3> {};
struct VertexMc : AdditiveVertex<6> {};
struct VertexIO : AdditiveVertex<17> {};

struct EdgeMcs : g2o::BaseMultiEdge<2, g2o::Vector2D> {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  EdgeMcs() {
    information().setIdentity();
    resize(4);
  }
  const double* est(int i) const {
    switch (i) {
      case 0: return static_cast<const VertexMt*>(_vertices[0])->estimate().data();
      case 1: return static_cast<const VertexPoint*>(_vertices[1])->estimate().data();
      case 2: return static_cast<const VertexMc*>(_vertices[2])->estimate().data();
      default: return static_cast<const VertexIO*>(_vertices[3])->estimate().data();
    }
  }
  void computeError() override {
    double e[2];
    oracle_ba_edge(est(0), est(1), est(2), est(3), _measurement.data(), e, nullptr, nullptr);
    _error[0] = e[0];
    _error[1] = e[1];
  }
  void linearizeOplus() override {
    double e[2], jp[12], jl[6];
    oracle_ba_edge(est(0), est(1), est(2), est(3), _measurement.data(), e, jp, jl);
    for (int r = 0; r < 2; r++) {
      for (int c = 0; c < 6; c++) _jacobianOplus[0](r, c) = jp[6 * r + c];
      for (int c = 0; c < 3; c++) _jacobianOplus[1](r, c) = jl[3 * r + c];
    }
    _jacobianOplus[2].setZero();   // Mc and IO are fixed: never read by the quadratic form
    _jacobianOplus[3].setZero();
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

// tau has no setter; the reference runs the constructor's value, which the options repeat
struct Levenberg : g2o::OptimizationAlgorithmLevenberg {
  explicit Levenberg(g2o::Solver* s) : g2o::OptimizationAlgorithmLevenberg(s) {}
  void setTau(double t) { _tau = t; }
};

// post-iteration record: robust chi2 and the LM trials of the iteration just run
struct Recorder : g2o::HyperGraphAction {
  Levenberg* lm = nullptr;
  std::vector<double> chi2;
  std::vector<int32_t> trials;
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph* graph, Parameters*) override {
    g2o::SparseOptimizer* o =
        const_cast<g2o::SparseOptimizer*>(static_cast<const g2o::SparseOptimizer*>(graph));
    o->computeActiveErrors();
    chi2.push_back(o->activeRobustChi2());
    trials.push_back(lm->levenbergIteration());
    return this;
  }
};

typedef g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType> EigenSolver;

struct Session {
  g2o::SparseOptimizer opt;   // owns the algorithm, the vertices and the edges
  g2o::SparseOptimizerTerminateAction term;
  Recorder rec;
  Levenberg* lm = nullptr;
  bool flag = false;          // the caller's pbStopFlag, when there is one
  bool has_flag = false;
  std::vector<VertexMt*> poses;
  std::vector<VertexPoint*> points;
  std::vector<EdgeMcs*> edges;
  int n_refused = 0;          // vertices addVertex refused (an id registered twice)
};

std::vector<int32_t> g_last_trials;

}  // namespace

extern "C" {

// One SparseOptimizer for one problem; rounds share it as the reference's rounds do (the
// terminate action, and with it the auxiliary flag it installs, lives as long as the graph).
// poses / points: initial estimates.  pose_id / point_id nullable: ids ascend in slot order,
// poses, then Mc, then IO, then points.  With ids given, Mc and IO follow the largest id.
// solver_kind 0: BlockSolver_6_3 over LinearSolverEigen (LocalBundleAdjustment,
// BundleAdjustment); 1: BlockSolverX over LinearSolverDense (PoseOptimization).
void* ref_g2o_create_ex(const mcs_ba_problem* p, const mcs_ba_options* o, const double* poses,
                        const double* points, int32_t points_fixed, int32_t has_stop_flag,
                        const int64_t* pose_id, const int64_t* point_id, int32_t solver_kind) {
  Session* s = new Session;
  s->opt.setVerbose(false);
  g2o::Solver* bs;
  if (solver_kind == 1)
    bs = new g2o::BlockSolverX(new g2o::LinearSolverDense<g2o::BlockSolverX::PoseMatrixType>());
  else
    bs = new g2o::BlockSolver_6_3(new EigenSolver());
  s->lm = new Levenberg(bs);
  s->lm->setTau(o->tau);
  s->lm->setMaxTrialsAfterFailure(o->max_trials);
  s->opt.setAlgorithm(s->lm);
  s->term.setGainThreshold(o->gain_threshold);
  s->term.setMaxIterations(o->terminate_max_iter);
  s->opt.addPostIterationAction(&s->term);
  s->rec.lm = s->lm;
  s->opt.addPostIterationAction(&s->rec);
  s->has_flag = has_stop_flag != 0;
  if (s->has_flag) s->opt.setForceStopFlag(&s->flag);

  int64_t next = 0;
  for (int i = 0; i < p->n_poses; i++) next = std::max<int64_t>(next, (pose_id ? pose_id[i] : i) + 1);
  if (point_id)
    for (int i = 0; i < p->n_points; i++) next = std::max<int64_t>(next, point_id[i] + 1);
  for (int i = 0; i < p->n_poses; i++) {
    VertexMt* v = new VertexMt;
    v->setEstimate(Eigen::Map<const VertexMt::Vec>(poses + 6 * i));
    v->setId((int)(pose_id ? pose_id[i] : i));
    v->setFixed(p->pose_fixed[i] != 0);
    if (!s->opt.addVertex(v)) { s->n_refused++; delete v; v = nullptr; }
    s->poses.push_back(v);
  }
  std::vector<VertexMc*> mcs;
  std::vector<VertexIO*> ios;
  for (int c = 0; c < p->n_cams; c++) {
    VertexMc* v = new VertexMc;
    v->setEstimate(Eigen::Map<const VertexMc::Vec>(p->mc + 6 * c));
    v->setId((int)next++);
    v->setFixed(true);
    s->opt.addVertex(v);
    mcs.push_back(v);
  }
  for (int c = 0; c < p->n_cams; c++) {
    VertexIO* v = new VertexIO;
    v->setEstimate(Eigen::Map<const VertexIO::Vec>(p->cam + 17 * c));
    v->setId((int)next++);
    v->setFixed(true);
    s->opt.addVertex(v);
    ios.push_back(v);
  }
  for (int i = 0; i < p->n_points; i++) {
    VertexPoint* v = new VertexPoint;
    v->setEstimate(Eigen::Map<const VertexPoint::Vec>(points + 3 * i));
    v->setId((int)(point_id ? point_id[i] : next + i));
    v->setFixed(points_fixed != 0);
    v->setMarginalized(true);
    if (!s->opt.addVertex(v)) { s->n_refused++; delete v; v = nullptr; }
    s->points.push_back(v);
  }
  for (int e = 0; e < p->n_edges; e++) {
    VertexMt* vp = s->poses[p->edge_pose[e]];
    VertexPoint* vl = s->points[p->edge_point[e]];
    if (!vp || !vl) { s->edges.push_back(nullptr); continue; }
    EdgeMcs* ed = new EdgeMcs;
    ed->setVertex(0, vp);
    ed->setVertex(1, vl);
    ed->setVertex(2, mcs[p->edge_cam[e]]);
    ed->setVertex(3, ios[p->edge_cam[e]]);
    ed->setMeasurement(g2o::Vector2D(p->edge_meas[2 * e], p->edge_meas[2 * e + 1]));
    ed->setInformation(Eigen::Matrix2d::Identity() * p->edge_info[e]);
    g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber;
    rk->setDelta(p->huber_delta);
    ed->setRobustKernel(rk);
    s->opt.addEdge(ed);
    s->edges.push_back(ed);
  }
  return s;
}

void* ref_g2o_create(const mcs_ba_problem* p, const mcs_ba_options* o, const double* poses,
                     const double* points, int32_t points_fixed, int32_t has_stop_flag,
                     const int64_t* pose_id, const int64_t* point_id) {
  return ref_g2o_create_ex(p, o, poses, points, points_fixed, has_stop_flag, pose_id, point_id, 0);
}

int32_t ref_g2o_refused_vertices(void* h) { return static_cast<Session*>(h)->n_refused; }

// initializeOptimization(0) + optimize(max_iterations) with the given edge levels; returns
// optimize()'s own return value (-1: nothing to optimise).  Outputs nullable.
int ref_g2o_round(void* h, const uint8_t* edge_level, int32_t max_iterations, int32_t* stop_flag,
                  mcs_ba_report* rep, double* poses, double* points, double* edge_chi2) {
  Session* s = static_cast<Session*>(h);
  g2o::SparseOptimizer& opt = s->opt;
  for (size_t e = 0; e < s->edges.size(); e++)
    if (s->edges[e]) s->edges[e]->setLevel(edge_level ? edge_level[e] : 0);
  if (s->has_flag && stop_flag) s->flag = *stop_flag != 0;
  opt.initializeOptimization(0);
  int np = 0, nl = 0;
  for (size_t i = 0; i < opt.indexMapping().size(); i++)
    (opt.indexMapping()[i]->marginalized() ? nl : np)++;
  double chi0 = 0;
  if (np + nl > 0) {
    opt.computeActiveErrors();
    chi0 = opt.activeRobustChi2();
  }
  s->rec.chi2.clear();
  s->rec.trials.clear();
  const int ret = opt.optimize(max_iterations);
  g_last_trials = s->rec.trials;
  const bool stopped = opt.forceStopFlag() ? *opt.forceStopFlag() : false;
  if (s->has_flag && stop_flag) *stop_flag = s->flag ? 1 : 0;
  if (rep) {
    rep->n_active_edges = (int32_t)opt.activeEdges().size();
    rep->n_active_poses = np;
    rep->n_active_points = nl;
    rep->iterations = (int32_t)s->rec.chi2.size();
    rep->stop_flag = stopped ? 1 : 0;
    rep->chi2_initial = chi0;
    rep->chi2_final = 0;
    if (np + nl > 0) {
      opt.computeActiveErrors();
      rep->chi2_final = opt.activeRobustChi2();
    }
    rep->lambda_final = s->lm->currentLambda();
    if (rep->trace_chi2)
      for (int i = 0; i < rep->trace_cap && i < (int)s->rec.chi2.size(); i++)
        rep->trace_chi2[i] = s->rec.chi2[i];
  }
  if (poses)
    for (size_t i = 0; i < s->poses.size(); i++)
      if (s->poses[i]) std::memcpy(poses + 6 * i, s->poses[i]->estimate().data(), 6 * sizeof(double));
  if (points)
    for (size_t i = 0; i < s->points.size(); i++)
      if (s->points[i]) std::memcpy(points + 3 * i, s->points[i]->estimate().data(), 3 * sizeof(double));
  if (edge_chi2)
    for (size_t e = 0; e < s->edges.size(); e++) {
      edge_chi2[e] = 0;
      if (!s->edges[e]) continue;
      s->edges[e]->computeError();
      edge_chi2[e] = s->edges[e]->chi2();
    }
  return ret;
}

void ref_g2o_destroy(void* h) { delete static_cast<Session*>(h); }

// levenbergIteration() after every iteration of the last round run
int32_t ref_g2o_last_trials(int32_t* out, int32_t cap) {
  for (int32_t i = 0; i < cap && i < (int32_t)g_last_trials.size(); i++) out[i] = g_last_trials[i];
  return (int32_t)g_last_trials.size();
}

// One graph, one round: the semantics of oracle_ba_optimize_ex (poses / points in and out).
int ref_g2o_optimize(const mcs_ba_problem* p, const mcs_ba_options* o, double* poses,
                     double* points, const uint8_t* edge_level, double* edge_chi2,
                     int32_t* stop_flag, mcs_ba_report* rep, int32_t points_fixed,
                     const int64_t* pose_id, const int64_t* point_id) {
  void* h = ref_g2o_create(p, o, poses, points, points_fixed, stop_flag != nullptr, pose_id, point_id);
  const int ret = ref_g2o_round(h, edge_level, o->max_iterations, stop_flag, rep, poses, points, edge_chi2);
  ref_g2o_destroy(h);
  return ret;
}

// LinearSolverEigen<6x6>::solve on a SparseBlockMatrix of n_blocks upper-triangle blocks
// (block_rows[k] <= block_cols[k], blocks[k] row-major 6x6); the order is that of the largest
// block index.  Returns solve()'s bool, -1 on a block below the diagonal.
int ref_g2o_linear_solve(int32_t n_blocks, const int32_t* block_rows, const int32_t* block_cols,
                         const double* blocks, const double* b, double* x) {
  typedef g2o::BlockSolver_6_3::PoseMatrixType Block;
  int nb = 0;
  for (int k = 0; k < n_blocks; k++) {
    if (block_rows[k] > block_cols[k] || block_rows[k] < 0) return -1;
    nb = std::max(nb, block_cols[k] + 1);
  }
  std::vector<int> ends(nb);
  for (int i = 0; i < nb; i++) ends[i] = 6 * (i + 1);
  g2o::SparseBlockMatrix<Block> A(ends.data(), ends.data(), nb, nb);
  for (int k = 0; k < n_blocks; k++) {
    Block* m = A.block(block_rows[k], block_cols[k], true);
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) (*m)(r, c) = blocks[36 * k + 6 * r + c];
  }
  EigenSolver solver;
  solver.init();
  std::vector<double> rhs(b, b + 6 * nb);
  return solver.solve(A, x, rhs.data()) ? 1 : 0;
}

}  // extern "C"
