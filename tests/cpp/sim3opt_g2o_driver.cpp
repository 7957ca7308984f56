// cOptimizer::OptimizeSim3 (reference src/cOptimizerLoopStuff.cpp:63-270) restated over the
// reference's own g2o, for tests/golden/gen_sim3opt_ref.py only: compiled by the generator into a
// temporary directory against the reference checkout's g2o / Eigen headers, linked with
// oracle/_ref/libg2o_ref.so (g2o's core) and oracle/build/liboracle.so (oracle_cam_world_to_img,
// which tests/test_refmath.py pins to the text).  Never part of the product.
//
//   sim3opt_g2o_driver CASE MODE    result lines of tests/cpp/sim3opt_io.hpp for every candidate
//     MODE 0   g2o's own numeric differentiation (delta = 1e-9, base_binary_edge.hpp:147-172)
//     MODE 1   the same central scheme in an edge subclass of this file, delta = 0.5e-9
//     MODE 2   likewise, delta = 2e-9
// The vertex and the edges follow include/g2o_MultiCol_sim3_expmap.h:117-260; keypoints, map
// points and keyframes are the flat arrays of the case file.  Slots whose crossed camera lookup
// leaves its map (undefined in the text) are the caller's to leave out: they abort here.
#include <cmath>
#include <cstdlib>
#include <limits>
#include <unordered_map>

#include <g2o/core/base_binary_edge.h>
#include <g2o/core/base_vertex.h>
#include <g2o/core/block_solver.h>
#include <g2o/core/optimization_algorithm_levenberg.h>
#include <g2o/core/robust_kernel_impl.h>
#include <g2o/core/sparse_optimizer.h>
#include <g2o/core/sparse_optimizer_terminate_action.h>
#include <g2o/solvers/linear_solver_dense.h>
#include <g2o/types/sim3.h>

#include "../../include/mcs_extractor.h"
#include "sim3opt_io.hpp"

extern "C" int oracle_cam_world_to_img(const mcs_cam_model* m, double x, double y, double z, double* uv);

namespace {

// cConverter::invMat (src/cConverter.cpp:31-44) of a row-major 4x4 -> 4x4
void inv_mat(const double* M, double* O) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O[4 * i + j] = M[4 * j + i];
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += -O[4 * i + k] * M[4 * k + 3];
    O[4 * i + 3] = s;
  }
  O[12] = O[13] = O[14] = 0.0;
  O[15] = 1.0;
}

// rows 0..2 of a cv::Matx44d times (x, 1)
void hom(const double* M, const double* x, double* y) {
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += M[4 * i + k] * x[k];
    y[i] = s + M[4 * i + 3] * 1.0;
  }
}

struct Rig {
  int C;
  std::vector<double> inv_mc;           // invMat(Get_M_c(c))
  std::vector<mcs_cam_model> model;
};

struct VertexSim3 : g2o::BaseVertex<7, g2o::Sim3> {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  const Rig* rig = nullptr;
  std::unordered_map<size_t, int> keypoint_to_cam1, keypoint_to_cam2;
  bool _fix_scale = false;
  void setToOriginImpl() override { _estimate = g2o::Sim3(); }
  void oplusImpl(const double* update_) override {
    Eigen::Map<g2o::Vector7d> update(const_cast<double*>(update_));
    if (_fix_scale) update[6] = 0;
    g2o::Sim3 s(update);
    setEstimate(s * estimate());
  }
  Eigen::Vector2d cam_map(const std::unordered_map<size_t, int>& k2c, const Eigen::Vector3d& v, int ptIdx) const {
    auto it = k2c.find((size_t)ptIdx);
    if (it == k2c.end()) { std::fprintf(stderr, "camera lookup outside its map (undefined in the text)\n"); std::abort(); }
    const int c = it->second;
    double p[3];
    const double x[3] = {v[0], v[1], v[2]};
    hom(&rig->inv_mc[16 * c], x, p);
    double uv[2];
    oracle_cam_world_to_img(&rig->model[c], p[0], p[1], p[2], uv);
    return Eigen::Vector2d(uv[0], uv[1]);
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

struct VertexPoint : g2o::BaseVertex<3, Eigen::Vector3d> {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  int ptID = 0;
  void setToOriginImpl() override { _estimate.setZero(); }
  void oplusImpl(const double* u) override { _estimate += Eigen::Vector3d(u[0], u[1], u[2]); }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

typedef g2o::BaseBinaryEdge<2, g2o::Vector2D, VertexPoint, VertexSim3> EdgeBase;

// g2o's central scheme (base_binary_edge.hpp:147-172) for the Sim3 vertex, at this file's delta;
// the point vertex is fixed, which the scheme skips
struct EdgeNum : EdgeBase {
  void central(double delta) {
    VertexSim3* vj = static_cast<VertexSim3*>(_vertices[1]);
    const double scalar = 1.0 / (2 * delta);
    ErrorVector errorBak;
    const ErrorVector errorBeforeNumeric = _error;
    double add_vj[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int d = 0; d < 7; ++d) {
      vj->push();
      add_vj[d] = delta;
      vj->oplus(add_vj);
      computeError();
      errorBak = _error;
      vj->pop();
      vj->push();
      add_vj[d] = -delta;
      vj->oplus(add_vj);
      computeError();
      errorBak -= _error;
      vj->pop();
      add_vj[d] = 0.0;
      _jacobianOplusXj.col(d) = scalar * errorBak;
    }
    _error = errorBeforeNumeric;
  }
};

double g_delta = 0.0;   // 0 = g2o's own linearizeOplus

struct Edge12 : EdgeNum {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  void computeError() override {
    const VertexSim3* v1 = static_cast<const VertexSim3*>(_vertices[1]);
    const VertexPoint* v2 = static_cast<const VertexPoint*>(_vertices[0]);
    const Eigen::Vector2d m = v1->cam_map(v1->keypoint_to_cam1, v1->estimate().map(v2->estimate()), v2->ptID);
    _error[0] = _measurement[0] - m[0];
    _error[1] = _measurement[1] - m[1];
  }
  void linearizeOplus() override {
    if (g_delta == 0.0) EdgeBase::linearizeOplus(); else central(g_delta);
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

struct Edge21 : EdgeNum {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  void computeError() override {
    const VertexSim3* v1 = static_cast<const VertexSim3*>(_vertices[1]);
    const VertexPoint* v2 = static_cast<const VertexPoint*>(_vertices[0]);
    const Eigen::Vector2d m =
        v1->cam_map(v1->keypoint_to_cam2, v1->estimate().inverse().map(v2->estimate()), v2->ptID);
    _error[0] = _measurement[0] - m[0];
    _error[1] = _measurement[1] - m[1];
  }
  void linearizeOplus() override {
    if (g_delta == 0.0) EdgeBase::linearizeOplus(); else central(g_delta);
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

struct Levenberg : g2o::OptimizationAlgorithmLevenberg {
  explicit Levenberg(g2o::Solver* s) : g2o::OptimizationAlgorithmLevenberg(s) {}
  void setTau(double t) { _tau = t; }
};

struct Recorder : g2o::HyperGraphAction {
  Levenberg* lm = nullptr;
  std::vector<int> trials;
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters*) override {
    trials.push_back(lm->levenbergIteration());
    return this;
  }
};

// the body of :63-270 for candidate k of the case
void optimize_sim3(const s3io::Case& c, s3io::Cand& k, const Rig& rig, s3io::Out& out) {
  g2o::SparseOptimizer optimizer;
  g2o::BlockSolverX::LinearSolverType* linearSolver =
      new g2o::LinearSolverDense<g2o::BlockSolverX::PoseMatrixType>();
  g2o::BlockSolverX* solver_ptr = new g2o::BlockSolverX(linearSolver);
  Levenberg* solver = new Levenberg(solver_ptr);
  solver->setTau(c.tau);
  solver->setMaxTrialsAfterFailure(c.max_trials);
  optimizer.setAlgorithm(solver);
  g2o::SparseOptimizerTerminateAction* terminateAction = new g2o::SparseOptimizerTerminateAction;
  terminateAction->setGainThreshold(c.gain);
  terminateAction->setMaxIterations(c.term_max);
  optimizer.addPostIterationAction(terminateAction);
  Recorder rec;
  rec.lm = solver;
  optimizer.addPostIterationAction(&rec);
  optimizer.setVerbose(false);

  const bool own = (c.flags & 1) != 0;
  VertexSim3* vSim3 = new VertexSim3;
  vSim3->rig = &rig;
  for (int i = 0; i < c.n1; i++) vSim3->keypoint_to_cam1[(size_t)i] = c.kf1.cam[i];
  for (int i = 0; i < k.kf.n; i++) vSim3->keypoint_to_cam2[(size_t)i] = k.kf.cam[i];
  Eigen::Matrix3d R;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R(i, j) = k.R[3 * i + j];
  const g2o::Sim3 g2oS12(R, Eigen::Vector3d(k.t[0], k.t[1], k.t[2]), k.s);
  vSim3->setEstimate(g2oS12);
  vSim3->setId(0);
  vSim3->setFixed(false);
  optimizer.addVertex(vSim3);

  const int N = c.n1;
  std::vector<Edge12*> vpEdges12;
  std::vector<Edge21*> vpEdges21;
  std::vector<size_t> vnIndexEdge;
  const double deltaHuber = 1.345 * c.std_sim;
  const double deltaHuber2 = deltaHuber * deltaHuber;
  int nCorrespondences = 0;
  double invM_t1[16], invM_t2[16];
  inv_mat(c.kf1.m_t, invM_t1);
  inv_mat(k.kf.m_t, invM_t2);
  const Eigen::Matrix2d I2x2 = Eigen::Matrix2d::Identity();

  for (int i = 0; i < N; i++) {
    const int m = k.matches12[i];
    if (m < 0) continue;                               // !vpMatches1[i]
    const int id1 = 2 * i + 1, id2 = 2 * (i + 1);
    const int i2 = k.first2[m];
    if (!(c.ok1[i] && k.ok2[m] && i2 >= 0)) continue;   // pMP1 && !bad1 && !bad2 && i2 >= 0
    double X1[3], X2[3];
    hom(invM_t1, &c.kf1.pos[3 * i], X1);
    hom(invM_t2, &k.kf.pos[3 * m], X2);
    VertexPoint* vPoint1 = new VertexPoint;
    vPoint1->setEstimate(Eigen::Vector3d(X1[0], X1[1], X1[2]));
    vPoint1->setId(id1);
    vPoint1->setFixed(true);
    vPoint1->ptID = own ? i2 : i;
    optimizer.addVertex(vPoint1);
    VertexPoint* vPoint2 = new VertexPoint;
    vPoint2->setEstimate(Eigen::Vector3d(X2[0], X2[1], X2[2]));
    vPoint2->setId(id2);
    vPoint2->setFixed(true);
    vPoint2->ptID = own ? i : i2;
    optimizer.addVertex(vPoint2);
    nCorrespondences++;

    Edge12* e12 = new Edge12;
    e12->setVertex(0, optimizer.vertex(id2));
    e12->setVertex(1, optimizer.vertex(0));
    e12->setMeasurement(Eigen::Vector2d((double)c.kf1.xy[2 * i], (double)c.kf1.xy[2 * i + 1]));
    e12->setInformation(I2x2 * c.inv_sigma2_1[c.kf1.oct[i]]);
    g2o::RobustKernelHuber* rk1 = new g2o::RobustKernelHuber;
    e12->setRobustKernel(rk1);
    rk1->setDelta(deltaHuber);
    optimizer.addEdge(e12);

    Edge21* e21 = new Edge21;
    e21->setVertex(0, optimizer.vertex(id1));
    e21->setVertex(1, optimizer.vertex(0));
    e21->setMeasurement(Eigen::Vector2d((double)k.kf.xy[2 * i2], (double)k.kf.xy[2 * i2 + 1]));
    e21->setInformation(I2x2 * c.sigma2_2[k.kf.oct[i2]]);
    g2o::RobustKernelHuber* rk2 = new g2o::RobustKernelHuber;
    e21->setRobustKernel(rk2);
    rk2->setDelta(deltaHuber);
    optimizer.addEdge(e21);

    vpEdges12.push_back(e12);
    vpEdges21.push_back(e21);
    vnIndexEdge.push_back((size_t)i);
  }

  auto record = [&](int round, int ret) {
    out.iters[round] = ret > 0 ? ret : 0;
    for (size_t j = 0; j < rec.trials.size() && j < 16; j++) out.trials[round][j] = rec.trials[j];
    rec.trials.clear();
    if (optimizer.activeEdges().size()) {
      optimizer.computeActiveErrors();
      out.chi2[round] = optimizer.activeRobustChi2();
    }
    out.lambda[round] = ret > 0 ? solver->currentLambda() : 0.0;
    for (size_t j = 0; j < vpEdges12.size(); j++)
      if (vpEdges12[j] && vpEdges21[j]) {
        out.edge_chi2[2 * vnIndexEdge[j]] = vpEdges12[j]->chi2();
        out.edge_chi2[2 * vnIndexEdge[j] + 1] = vpEdges21[j]->chi2();
      }
    if (round == 0) out.edge_chi2_r1 = out.edge_chi2;
  };

  out.n_corr = nCorrespondences;
  out.s = g2oS12.scale();
  const Eigen::Quaterniond q0 = g2oS12.rotation();
  out.q[0] = q0.w(); out.q[1] = q0.x(); out.q[2] = q0.y(); out.q[3] = q0.z();
  for (int j = 0; j < 3; j++) out.t[j] = g2oS12.translation()[j];

  optimizer.initializeOptimization();
  record(0, optimizer.optimize(c.its1));

  int nBad = 0;
  for (size_t i = 0; i < vpEdges12.size(); i++) {
    Edge12* e12 = vpEdges12[i];
    Edge21* e21 = vpEdges21[i];
    if (!e12 || !e21) continue;
    if (e12->chi2() > deltaHuber2 || e21->chi2() > deltaHuber2) {
      k.matches12[vnIndexEdge[i]] = -1;
      optimizer.removeEdge(e12);
      optimizer.removeEdge(e21);
      vpEdges12[i] = nullptr;
      vpEdges21[i] = nullptr;
      nBad++;
    }
  }
  out.n_bad = nBad;
  const int nMoreIterations = nBad > 0 ? c.its_culled : c.its_clean;
  if (nCorrespondences - nBad < 3) { out.n_in = 0; return; }

  optimizer.initializeOptimization();
  record(1, optimizer.optimize(nMoreIterations));

  int nIn = 0;
  for (size_t i = 0; i < vpEdges12.size(); i++) {
    Edge12* e12 = vpEdges12[i];
    Edge21* e21 = vpEdges21[i];
    if (!e12 || !e21) continue;
    if (e12->chi2() > deltaHuber2 || e21->chi2() > deltaHuber2) k.matches12[vnIndexEdge[i]] = -1;
    else nIn++;
  }
  const g2o::Sim3 S = static_cast<VertexSim3*>(optimizer.vertex(0))->estimate();
  out.s = S.scale();
  const Eigen::Quaterniond q = S.rotation();
  out.q[0] = q.w(); out.q[1] = q.x(); out.q[2] = q.y(); out.q[3] = q.z();
  for (int j = 0; j < 3; j++) out.t[j] = S.translation()[j];
  out.n_in = nIn;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: sim3opt_g2o_driver CASE MODE\n"); return 2; }
  s3io::Case c;
  if (!s3io::read_case(argv[1], c)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int mode = std::atoi(argv[2]);
  g_delta = mode == 1 ? 0.5e-9 : mode == 2 ? 2e-9 : 0.0;
  Rig rig;
  rig.C = c.C;
  rig.inv_mc.resize(16 * c.C);
  rig.model.resize(c.C);
  for (int j = 0; j < c.C; j++) {
    inv_mat(&c.m_c[16 * j], &rig.inv_mc[16 * j]);
    mcs_cam_model& m = rig.model[j];
    m = mcs_cam_model{};
    const double* v = &c.cam[17 * j];
    m.c = v[0]; m.d = v[1]; m.e = v[2]; m.u0 = v[3]; m.v0 = v[4];
    m.invp_deg = 12;
    for (int i = 0; i < 12; i++) m.invp[i] = v[5 + i];
  }
  for (int t = 0; t < c.T; t++) {
    s3io::Out out;
    out.edge_chi2.assign(2 * (size_t)c.n1, std::numeric_limits<double>::quiet_NaN());
    optimize_sim3(c, c.cands[t], rig, out);
    out.matches12 = c.cands[t].matches12;
    s3io::print_out(t, out);
  }
  return 0;
}
