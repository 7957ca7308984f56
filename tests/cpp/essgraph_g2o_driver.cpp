// cOptimizer::OptimizeEssentialGraph (reference src/cOptimizerLoopStuff.cpp:273-519) restated over
// the reference's own g2o, for tests/golden/gen_essgraph_ref.py only: compiled by the generator
// into a temporary directory against the reference checkout's g2o / Eigen headers and linked with
// oracle/_ref/libg2o_ref.so (g2o's core).  Never part of the product.
//
//   essgraph_g2o_driver CASE MODE
//     MODE 0   g2o's own numeric differentiation (delta = 1e-9, base_binary_edge.hpp:147-199)
//     MODE 1   the same central scheme in an edge subclass of this file, delta = 0.5e-9
//     MODE 2   likewise, delta = 2e-9
//     MODE 3   CASE is a list: "log s qw qx qy qz tx ty tz" -> Sim3::log, "exp w0 w1 w2 u0 u1 u2 sigma"
//              -> Sim3(update) as s q t
//     MODE 4   only the edge list the loops of :355-470 produce from the graph arrays
// The vertex and the edge follow include/g2o_MultiCol_sim3_expmap.h:51-115.  Keyframes are the flat
// arrays of the case file in ascending id order, which is the order the loops run in here (the
// text's std::map / std::set iterate in pointer order); no keyframe is bad.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include <g2o/core/base_binary_edge.h>
#include <g2o/core/base_vertex.h>
#include <g2o/core/block_solver.h>
#include <g2o/core/optimization_algorithm_levenberg.h>
#include <g2o/core/sparse_optimizer.h>
#include <g2o/core/sparse_optimizer_terminate_action.h>
#include <g2o/solvers/linear_solver_eigen.h>
#include <g2o/types/sim3.h>

#include "essgraph_io.hpp"

namespace {

double g_delta = 0.0;            // 0 = g2o's own linearizeOplus
double g_branch_margin = 1e300;  // min over the linearisation points of | |sigma| / 1e-5 - 1 |, | (1 - d) / 1e-5 - 1 |

struct VertexSim3 : g2o::BaseVertex<7, g2o::Sim3> {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  bool _fix_scale = false;
  void setToOriginImpl() override { _estimate = g2o::Sim3(); }
  void oplusImpl(const double* update_) override {
    Eigen::Map<g2o::Vector7d> update(const_cast<double*>(update_));
    if (_fix_scale) update[6] = 0;
    g2o::Sim3 s(update);
    setEstimate(s * estimate());
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

typedef g2o::BaseBinaryEdge<7, g2o::Sim3, VertexSim3, VertexSim3> EdgeBase;

struct EdgeSim3 : EdgeBase {
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  void computeError() override {
    const VertexSim3* v1 = static_cast<const VertexSim3*>(_vertices[0]);
    const VertexSim3* v2 = static_cast<const VertexSim3*>(_vertices[1]);
    g2o::Sim3 C(_measurement);
    g2o::Sim3 error_ = C * v1->estimate() * v2->estimate().inverse();
    _error = error_.log();
  }
  // sigma and d of Sim3::log at the linearisation point, as its branches test them
  void note_branch_margin() const {
    const VertexSim3* v1 = static_cast<const VertexSim3*>(_vertices[0]);
    const VertexSim3* v2 = static_cast<const VertexSim3*>(_vertices[1]);
    const g2o::Sim3 error_ = g2o::Sim3(_measurement) * v1->estimate() * v2->estimate().inverse();
    const Eigen::Matrix3d R = error_.rotation().toRotationMatrix();
    const double d = 0.5 * (R(0, 0) + R(1, 1) + R(2, 2) - 1), sigma = std::log(error_.scale());
    g_branch_margin = std::min(g_branch_margin, std::fabs(std::fabs(sigma) / 1e-5 - 1.0));
    g_branch_margin = std::min(g_branch_margin, std::fabs((1.0 - d) / 1e-5 - 1.0));
  }
  // g2o's central scheme for both vertices at this file's delta, a fixed vertex skipped
  template <class V, class Jac>
  void central(V* v, Jac& J, double delta) {
    if (v->fixed()) return;
    const double scalar = 1.0 / (2 * delta);
    ErrorVector errorBak;
    double add[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int d = 0; d < 7; ++d) {
      v->push();
      add[d] = delta;
      v->oplus(add);
      computeError();
      errorBak = _error;
      v->pop();
      v->push();
      add[d] = -delta;
      v->oplus(add);
      computeError();
      errorBak -= _error;
      v->pop();
      add[d] = 0.0;
      J.col(d) = scalar * errorBak;
    }
  }
  void linearizeOplus() override {
    note_branch_margin();
    if (g_delta == 0.0) { EdgeBase::linearizeOplus(); return; }
    const ErrorVector errorBeforeNumeric = _error;
    central(static_cast<VertexSim3*>(_vertices[0]), _jacobianOplusXi, g_delta);
    central(static_cast<VertexSim3*>(_vertices[1]), _jacobianOplusXj, g_delta);
    _error = errorBeforeNumeric;
  }
  bool read(std::istream&) override { return false; }
  bool write(std::ostream&) const override { return false; }
};

struct Recorder : g2o::HyperGraphAction {
  g2o::OptimizationAlgorithmLevenberg* lm = nullptr;
  g2o::SparseOptimizer* opt = nullptr;
  std::vector<int> trials;
  std::vector<double> chi2;
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters*) override {
    trials.push_back(lm->levenbergIteration());
    opt->computeActiveErrors();
    chi2.push_back(opt->activeRobustChi2());
    return this;
  }
};

g2o::Sim3 load(const double* p) {
  return g2o::Sim3(Eigen::Quaterniond(p[1], p[2], p[3], p[4]), Eigen::Vector3d(p[5], p[6], p[7]), p[0]);
}
void store(const g2o::Sim3& S, double* p) {
  p[0] = S.scale();
  const Eigen::Quaterniond& q = S.rotation();
  p[1] = q.w(); p[2] = q.x(); p[3] = q.y(); p[4] = q.z();
  for (int k = 0; k < 3; k++) p[5 + k] = S.translation()[k];
}

// cConverter::invMat (src/cConverter.cpp:31-44) of [R t; 0 1] -> row-major 4x4
void inv_se3(const Eigen::Matrix3d& R, const Eigen::Vector3d& t, double* O) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O[4 * i + j] = R(j, i);
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += -O[4 * i + k] * t[k];
    O[4 * i + 3] = s;
  }
  O[12] = O[13] = O[14] = 0.0;
  O[15] = 1.0;
}

// the body of :281-518; optimise = false stops after the edge list
void optimize_essential_graph(const egio::Case& c, bool optimise, egio::Out& out) {
  g2o::SparseOptimizer optimizer;
  optimizer.setVerbose(false);
  g2o::BlockSolver_7_3::LinearSolverType* linearSolver =
      new g2o::LinearSolverEigen<g2o::BlockSolver_7_3::PoseMatrixType>();
  g2o::BlockSolver_7_3* solver_ptr = new g2o::BlockSolver_7_3(linearSolver);
  g2o::OptimizationAlgorithmLevenberg* solver = new g2o::OptimizationAlgorithmLevenberg(solver_ptr);
  solver->setUserLambdaInit(c.lambda0);
  solver->setMaxTrialsAfterFailure(c.max_trials);
  optimizer.setAlgorithm(solver);
  g2o::SparseOptimizerTerminateAction* terminateAction = new g2o::SparseOptimizerTerminateAction;
  terminateAction->setGainThreshold(c.gain);
  terminateAction->setMaxIterations(c.term_max);
  optimizer.addPostIterationAction(terminateAction);
  Recorder rec;
  rec.lm = solver;
  rec.opt = &optimizer;
  optimizer.addPostIterationAction(&rec);

  const int N = c.N;
  int64_t nMaxMKFid = 0;
  for (int i = 0; i < N; i++) nMaxMKFid = std::max(nMaxMKFid, c.id[i]);
  std::vector<g2o::Sim3, Eigen::aligned_allocator<g2o::Sim3>> vScw(nMaxMKFid + 1), vScw_corrected(nMaxMKFid + 1);
  std::vector<g2o::Sim3, Eigen::aligned_allocator<g2o::Sim3>> nonCorrected(N);
  const int64_t curId = c.id[c.cur], loopId = c.id[c.loop];

  for (int i = 0; i < N; i++) {
    VertexSim3* VSim3 = new VertexSim3();
    const int MKFid = (int)c.id[i];
    // CorrectedSim3[kf] when present, else Sim3(R, t, 1) of GetPoseInverse(): both arrive as Scw
    vScw[MKFid] = load(&c.Scw[8 * i]);
    VSim3->setEstimate(vScw[MKFid]);
    nonCorrected[i] = load(&c.Snc[8 * i]);    // NonCorrectedSim3 where present, else vScw
    if (i == c.loop) VSim3->setFixed(true);
    VSim3->setId(MKFid);
    VSim3->setMarginalized(false);
    optimizer.addVertex(VSim3);
  }

  const Eigen::Matrix<double, 7, 7> matLambda = Eigen::Matrix<double, 7, 7>::Identity();
  std::vector<EdgeSim3*> all;
  auto add = [&](int i, int j, const g2o::Sim3& meas, int kind, int source) {
    EdgeSim3* e = new EdgeSim3();
    e->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex((int)c.id[j])));
    e->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex((int)c.id[i])));
    e->setMeasurement(meas);
    e->information() = matLambda;
    optimizer.addEdge(e);
    all.push_back(e);
    out.edges.push_back(i); out.edges.push_back(j); out.edges.push_back(kind);
    out.counts[source]++;
  };

  // loop-connection edges (:355-382)
  for (int i = 0; i < N; i++) {
    if (c.lc_ptr[i] == c.lc_ptr[i + 1]) continue;          // not a key of LoopConnections
    const int64_t MKFid_i = c.id[i];
    const g2o::Sim3 Siw = vScw[MKFid_i];
    const g2o::Sim3 Swi = Siw.inverse();
    for (int k = c.lc_ptr[i]; k < c.lc_ptr[i + 1]; k++) {
      const int j = c.lc_idx[k];
      const int64_t MKFid_j = c.id[j];
      if ((MKFid_i != curId || MKFid_j != loopId) && c.lc_w[k] < c.min_weight) continue;
      const g2o::Sim3 Sjw = vScw[MKFid_j];
      add(i, j, Sjw * Swi, 0, 0);
    }
  }
  // normal edges (:385-470)
  for (int i = 0; i < N; i++) {
    const int64_t MKFid_i = c.id[i];
    const g2o::Sim3 Swi = nonCorrected[i].inverse();
    const int kind_i = c.has_corr[i];
    if (c.parent[i] >= 0) {
      const int j = c.parent[i];
      add(i, j, nonCorrected[j] * Swi, (kind_i || c.has_corr[j]) ? 1 : 0, 1);
    }
    for (int k = c.loop_ptr[i]; k < c.loop_ptr[i + 1]; k++) {
      const int l = c.loop_idx[k];
      if (c.id[l] < MKFid_i) add(i, l, nonCorrected[l] * Swi, (kind_i || c.has_corr[l]) ? 1 : 0, 2);
    }
    for (int k = c.cov_ptr[i]; k < c.cov_ptr[i + 1]; k++) {
      if (c.cov_w[k] < c.min_weight) continue;             // GetCovisiblesByWeight(minNumFeat)
      const int nb = c.cov_idx[k];
      if (c.id[nb] < MKFid_i) add(i, nb, nonCorrected[nb] * Swi, (kind_i || c.has_corr[nb]) ? 1 : 0, 3);
    }
  }
  if (!optimise) return;

  optimizer.initializeOptimization(0);
  optimizer.computeActiveErrors();
  out.chi2_initial = optimizer.activeRobustChi2();
  const int ret = optimizer.optimize(c.iterations);
  out.iterations = ret > 0 ? ret : 0;
  out.trials = rec.trials;
  out.chi2 = rec.chi2;
  out.lambda = ret > 0 ? solver->currentLambda() : 0.0;
  optimizer.computeActiveErrors();
  for (EdgeSim3* e : all) out.edge_chi2.push_back(e->chi2());

  out.sim3.resize(8 * (size_t)N);
  out.pose.resize(16 * (size_t)N);
  for (int i = 0; i < N; i++) {
    const int MKFid_i = (int)c.id[i];
    VertexSim3* VSim3 = static_cast<VertexSim3*>(optimizer.vertex(MKFid_i));
    g2o::Sim3 CorrectedSiw = VSim3->estimate();
    vScw_corrected[MKFid_i] = CorrectedSiw.inverse();
    store(CorrectedSiw, &out.sim3[8 * (size_t)i]);
    double scale = CorrectedSiw.scale();
    Eigen::Matrix3d R = CorrectedSiw.rotation().toRotationMatrix();
    Eigen::Vector3d t = CorrectedSiw.translation() / scale;
    inv_se3(R, t, &out.pose[16 * (size_t)i]);
  }
  out.points = c.pos;
  for (int j = 0; j < c.P; j++) {
    if (c.bad[j]) continue;
    int64_t MP_ref_MKFid = 0;
    if (c.corrected_by[j] == curId) MP_ref_MKFid = c.corrected_ref[j];
    else MP_ref_MKFid = c.ref_kf[j];
    g2o::Sim3 Srw = vScw[MP_ref_MKFid];
    g2o::Sim3 corrected_Swr = vScw_corrected[MP_ref_MKFid];
    const Eigen::Vector3d x(c.pos[3 * j], c.pos[3 * j + 1], c.pos[3 * j + 2]);
    const Eigen::Vector3d y = corrected_Swr.map(Srw.map(x));
    for (int k = 0; k < 3; k++) out.points[3 * j + k] = y[k];
  }
  out.branch_margin = g_branch_margin;
}

int list_mode(const char* path) {
  std::ifstream f(path);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream is(line);
    std::string tag;
    is >> tag;
    if (tag == "log") {
      double p[8];
      for (double& v : p) is >> v;
      const g2o::Vector7d r = load(p).log();
      egio::print_vec("log", r.data(), 7);
    } else if (tag == "exp") {
      g2o::Vector7d u;
      for (int k = 0; k < 7; k++) is >> u[k];
      double p[8];
      store(g2o::Sim3(u), p);
      egio::print_vec("exp", p, 8);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: essgraph_g2o_driver CASE MODE\n"); return 2; }
  const int mode = std::atoi(argv[2]);
  if (mode == 3) return list_mode(argv[1]);
  egio::Case c;
  if (!egio::read_case(argv[1], c)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  g_delta = mode == 1 ? 0.5e-9 : mode == 2 ? 2e-9 : 0.0;
  egio::Out out;
  optimize_essential_graph(c, mode != 4, out);
  if (mode == 4) egio::print_edges(out);
  else egio::print_out(out);
  return 0;
}
