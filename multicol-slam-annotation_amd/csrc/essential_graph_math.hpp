// cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:273-519) as plain functions:
// g2o::Sim3::log (ThirdParty/g2o/g2o/types/sim3.h:148-230), the edgeSim3 error
// (include/g2o_MultiCol_sim3_expmap.h:90-98), the 7x7 Jacobians of an edge by g2o's central
// differences (base_binary_edge.hpp:147-199; the edge has no linearizeOplus), the write-back
// (:479-518) and a serial optimize_essential_graph_host over lm_control.hpp with a plain dense
// LDL^T.  essential_graph.hip runs the same functions spread over lanes.
//
// sim3_log reproduces all four branches of the text as written: the thresholds |sigma| < 1e-5 and
// d > 1 - 1e-5, omega = 0.5 deltaR(R) in the small-angle branches (not the series), the
// B = (sigma^2/2 - sigma + 1) s / sigma^3 of the theta -> 0, sigma != 0 branch (the closed form
// has a further "- 1" in the numerator; the text's value grows like 1/sigma^3),
// and upsilon = W.lu().solve(t), Eigen's partial-pivot LU.
//
// No HIP include: __host__ __device__ under hipcc, inline under a host compiler.  Needs
// -ffp-contract=off.
#pragma once
#include "sim3_opt_math.hpp"
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
#endif

namespace mcs {
namespace esg {

using s3o::Sim3;

// The step of the central differences.  g2o's own is 1e-9; the host program over the six fixture
// cases (DESIGN 3.14, table of the four candidates) has its worst difference-to-tolerance ratio
// smallest at this one.  It must stay well under the 1e-5 branch thresholds of exp / log.
constexpr double kDiffStep = 1e-8;

constexpr int kMaxIterations = 64;   // LmCtl::trace holds this many

// (s, q, t) as the entries carry a Sim3: s, qw qx qy qz, tx ty tz
MCS_LM_FN Sim3 sim3_load(const double* p) {
  Sim3 S;
  S.s = p[0];
  for (int i = 0; i < 4; i++) S.q[i] = p[1 + i];
  for (int i = 0; i < 3; i++) S.t[i] = p[5 + i];
  return S;
}
MCS_LM_FN void sim3_store(const Sim3& S, double* p) {
  p[0] = S.s;
  for (int i = 0; i < 4; i++) p[1 + i] = S.q[i];
  for (int i = 0; i < 3; i++) p[5 + i] = S.t[i];
}

// x = W^-1 t by PartialPivLU (Eigen/src/LU/PartialPivLU.h, unblocked): per column the row of the
// largest |entry| is swapped up, the column below the pivot divided by it, the trailing block
// updated; then L y = P t forward and U x = y backward
MCS_LM_FN void lu3_solve(const double* Win, const double* t, double* x) {
  double W[9], y[3] = {t[0], t[1], t[2]};
  for (int k = 0; k < 9; k++) W[k] = Win[k];
  for (int k = 0; k < 3; k++) {
    int p = k;
    double best = __builtin_fabs(W[3 * k + k]);
    for (int i = k + 1; i < 3; i++) {
      const double a = __builtin_fabs(W[3 * i + k]);
      if (a > best) { best = a; p = i; }
    }
    if (p != k) {
      for (int j = 0; j < 3; j++) { const double w = W[3 * k + j]; W[3 * k + j] = W[3 * p + j]; W[3 * p + j] = w; }
      const double w = y[k]; y[k] = y[p]; y[p] = w;
    }
    if (best != 0.0)
      for (int i = k + 1; i < 3; i++) W[3 * i + k] /= W[3 * k + k];
    for (int i = k + 1; i < 3; i++)
      for (int j = k + 1; j < 3; j++) W[3 * i + j] -= W[3 * i + k] * W[3 * k + j];
  }
  for (int i = 1; i < 3; i++)
    for (int j = 0; j < i; j++) y[i] -= W[3 * i + j] * y[j];
  for (int i = 2; i >= 0; i--) {
    double s = y[i];
    for (int j = i + 1; j < 3; j++) s -= W[3 * i + j] * x[j];
    x[i] = s / W[3 * i + i];
  }
}

// Sim3::log -> (omega, upsilon, sigma)
MCS_LM_FN void sim3_log(const Sim3& S, double* res) {
  const double s = S.s;
  const double sigma = log(s);
  double R[9];
  s3o::quat_to_rot(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  double omega[3], A, B, C;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta = acos(d);
      const double theta2 = theta * theta;
      const double k = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; i++) omega[i] = k * dR[i];
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
      A = ((sigma - 1) * s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      const double k = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; i++) omega[i] = k * dR[i];
      const double theta2 = theta * theta;
      const double a = s * sin(theta);
      const double b = s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double Om[9] = {0.0, -omega[2], omega[1], omega[2], 0.0, -omega[0], -omega[1], omega[0], 0.0};
  double Om2[9], W[9];
  s3o::mat3_mul(Om, Om, Om2);
  for (int k = 0; k < 9; k++) W[k] = A * Om[k] + B * Om2[k] + (k % 4 == 0 ? C : 0.0);
  lu3_solve(W, S.t, res + 3);
  for (int i = 0; i < 3; i++) res[i] = omega[i];
  res[6] = sigma;
}

// setMeasurement(Sjw * Swi) (:377, :414, :439, :465): v0 = i, v1 = j
MCS_LM_FN Sim3 edge_measurement(const Sim3& S_v0, const Sim3& S_v1) {
  return s3o::sim3_mul(S_v1, s3o::sim3_inverse(S_v0));
}

// edgeSim3::computeError: log(C * v0 * v1^-1), evaluated left to right
MCS_LM_FN void edge_error(const Sim3& C, const Sim3& S0, const Sim3& S1, double* e) {
  const Sim3 E = s3o::sim3_mul(s3o::sim3_mul(C, S0), s3o::sim3_inverse(S1));
  sim3_log(E, e);
}

MCS_LM_FN double edge_chi2(const double* e) {
  double s = 0.0;
  for (int k = 0; k < 7; k++) s += e[k] * e[k];
  return s;
}

// Column k of d error / d vertex `which` (0 / 1): (e(exp(+delta e_k) S) - e(exp(-delta e_k) S)) / (2 delta)
MCS_LM_FN void edge_jac_col(const Sim3& C, const Sim3& S0, const Sim3& S1, int which, int k, double delta,
                            double* col) {
  double add[7] = {0, 0, 0, 0, 0, 0, 0}, ep[7], em[7];
  const double scalar = 1 / (2 * delta);
  add[k] = delta;
  const Sim3 Sp = s3o::sim3_mul(s3o::sim3_exp(add), which ? S1 : S0);
  add[k] = -delta;
  const Sim3 Sm = s3o::sim3_mul(s3o::sim3_exp(add), which ? S1 : S0);
  if (which) { edge_error(C, S0, Sp, ep); edge_error(C, S0, Sm, em); }
  else { edge_error(C, Sp, S1, ep); edge_error(C, Sm, S1, em); }
  for (int r = 0; r < 7; r++) col[r] = scalar * (ep[r] - em[r]);
}

// :479-490: the world pose invMat(toCvSE3(R, t / s)) of an optimised Siw, row-major 4x4; R9 (nullable)
MCS_LM_FN void pose_from_sim3(const Sim3& S, double* M, double* R9) {
  double R[9];
  s3o::quat_to_rot(S.q, R);
  const double t[3] = {S.t[0] / S.s, S.t[1] / S.s, S.t[2] / S.s};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[4 * i + j] = R[3 * j + i];
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += -M[4 * i + k] * t[k];
    M[4 * i + 3] = s;
  }
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
  if (R9) for (int k = 0; k < 9; k++) R9[k] = R[k];
}

// :510-516: corrected_Swr.map(Srw.map(x)) with corrected_Swr = (optimised Srw)^-1
MCS_LM_FN void correct_point(const Sim3& Srw, const Sim3& Srw_opt, const double* x, double* y) {
  double m[3];
  s3o::sim3_map(Srw, x, m);
  s3o::sim3_map(s3o::sim3_inverse(Srw_opt), m, y);
}

// :501-507: the keyframe (by id) whose Sim3 pair moves the point
MCS_LM_FN int64_t point_ref_id(int64_t corrected_by, int64_t corrected_ref, int64_t ref_kf, int64_t current_id) {
  return corrected_by == current_id ? corrected_ref : ref_kf;
}

// row of the reduced system of keyframe i (the fixed vertex is left out), -1 for the fixed one
MCS_LM_FN int free_index(int i, int loop) { return i == loop ? -1 : (i < loop ? i : i - 1); }

#if !defined(__HIP_DEVICE_COMPILE__)
struct HostResult {
  std::vector<Sim3> S;              // [N] optimised Siw
  std::vector<double> pose;         // [N][16]
  std::vector<double> edge_chi2;    // [E]
  int iterations = 0;
  int trials[kMaxIterations] = {0};
  double chi2[kMaxIterations] = {0};
  double chi2_initial = 0.0, lambda = 0.0;
};

struct HostOptions { int iterations = 20, terminate_max_iter = 15, max_trials = 10; double gain = 1e-6, lambda0 = 1e-6; };

// (H + lambda I) x = b, H dense n x n (lower used), plain LDL^T without pivoting; false = an exact
// zero pivot
inline bool dense_ldlt_solve(const std::vector<double>& H, const std::vector<double>& b, int n, double lambda,
                             std::vector<double>& x) {
  std::vector<double> L((size_t)n * n), d(n), y(n);
  bool ok = true;
  for (int j = 0; j < n; j++) {
    double dj = H[(size_t)j * n + j] + lambda;
    for (int m = 0; m < j; m++) dj -= L[(size_t)j * n + m] * L[(size_t)j * n + m] * d[m];
    if (dj == 0.0) { ok = false; dj = 1.0; }
    d[j] = dj;
    for (int i = j + 1; i < n; i++) {
      double s = H[(size_t)i * n + j];
      for (int m = 0; m < j; m++) s -= L[(size_t)i * n + m] * L[(size_t)j * n + m] * d[m];
      L[(size_t)i * n + j] = s / dj;
    }
  }
  for (int i = 0; i < n; i++) {
    double s = b[i];
    for (int m = 0; m < i; m++) s -= L[(size_t)i * n + m] * y[m];
    y[i] = s;
  }
  x.assign(n, 0.0);
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i] / d[i];
    for (int m = i + 1; m < n; m++) s -= L[(size_t)m * n + i] * x[m];
    x[i] = s;
  }
  return ok;
}

// The solve of :281-474 and the pose write-back for N keyframes (Scw / Snc [N][8]) and E edges
// (v0, v1, kind).  delta = the difference step.  The caller has checked the indices.
inline void optimize_essential_graph_host(int N, const double* Scw, const double* Snc, int loop, int E,
                                          const int32_t* edges, const HostOptions& o, double delta, HostResult* res) {
  std::vector<Sim3> S(N), C(E);
  for (int i = 0; i < N; i++) S[i] = sim3_load(Scw + 8 * i);
  for (int e = 0; e < E; e++) {
    const double* tab = edges[3 * e + 2] ? Snc : Scw;
    C[e] = edge_measurement(sim3_load(tab + 8 * edges[3 * e]), sim3_load(tab + 8 * edges[3 * e + 1]));
  }
  auto chi_all = [&](std::vector<double>* per_edge) {
    double chi = 0.0;
    for (int e = 0; e < E; e++) {
      double err[7];
      edge_error(C[e], S[edges[3 * e]], S[edges[3 * e + 1]], err);
      const double c = edge_chi2(err);
      if (per_edge) (*per_edge)[e] = c;
      chi += c;
    }
    return chi;
  };
  const int n = 7 * (N - 1);
  *res = HostResult();
  ba::LmCtl ctl;
  mcs_ba_options bo{};
  bo.max_iterations = o.iterations; bo.gain_threshold = o.gain; bo.terminate_max_iter = o.terminate_max_iter;
  bo.max_trials = o.max_trials; bo.tau = 0.0;
  ba::lm_init(ctl, bo);
  res->chi2_initial = chi_all(nullptr);
  ba::lm_start_body(&ctl, res->chi2_initial);
  ctl.done = (o.iterations <= 0 || n <= 0 || E <= 0) ? 1 : 0;   // "0 vertices to optimize"
  std::vector<double> H((size_t)n * n), b(n), x, J(98 * (size_t)E), err(7 * (size_t)E);
  for (int g = 0; g < o.iterations * o.max_trials && !ctl.done; g++) {
    if (ctl.lin) {
      std::fill(H.begin(), H.end(), 0.0);
      std::fill(b.begin(), b.end(), 0.0);
      for (int e = 0; e < E; e++) {
        const int v[2] = {edges[3 * e], edges[3 * e + 1]};
        const int u[2] = {free_index(v[0], loop), free_index(v[1], loop)};
        double* Je = &J[98 * (size_t)e];
        double* ee = &err[7 * (size_t)e];
        edge_error(C[e], S[v[0]], S[v[1]], ee);
        for (int w = 0; w < 2; w++)
          for (int k = 0; k < 7 && u[w] >= 0; k++) {
            double col[7];
            edge_jac_col(C[e], S[v[0]], S[v[1]], w, k, delta, col);
            for (int r = 0; r < 7; r++) Je[49 * w + 7 * r + k] = col[r];
          }
        for (int a = 0; a < 2; a++) {
          if (u[a] < 0) continue;
          for (int i = 0; i < 7; i++) {
            double s = 0.0;
            for (int r = 0; r < 7; r++) s += Je[49 * a + 7 * r + i] * ee[r];
            b[7 * u[a] + i] += -s;
          }
          for (int c2 = 0; c2 < 2; c2++) {
            if (u[c2] < 0) continue;
            for (int i = 0; i < 7; i++)
              for (int j = 0; j < 7; j++) {
                double s = 0.0;
                for (int r = 0; r < 7; r++) s += Je[49 * a + 7 * r + i] * Je[49 * c2 + 7 * r + j];
                H[(size_t)(7 * u[a] + i) * n + 7 * u[c2] + j] += s;
              }
          }
        }
      }
      if (ctl.iter == 0) { ctl.lambda = o.lambda0; ctl.ni = 2; ctl.nBad = 0; }   // setUserLambdaInit (:288)
    }
    const bool ok = dense_ldlt_solve(H, b, n, ctl.lambda, x);
    const std::vector<Sim3> bak = S;
    double scale = 0.0;
    for (int i = 0; i < n; i++) scale += x[i] * (ctl.lambda * x[i] + b[i]);
    for (int i = 0; i < N; i++) {
      const int u = free_index(i, loop);
      if (u >= 0) S[i] = s3o::sim3_mul(s3o::sim3_exp(&x[7 * u]), bak[i]);
    }
    const double sc[3] = {chi_all(nullptr), 0.0, scale};
    const int it = ctl.iter;
    ba::lm_step(&ctl, sc, !ok, false, 0);
    if (it < kMaxIterations) res->trials[it]++;
    if (ctl.restore) S = bak;
  }
  res->iterations = ctl.iter;
  for (int i = 0; i < ctl.iter && i < kMaxIterations; i++) res->chi2[i] = ctl.trace[i];
  res->lambda = ctl.iter > 0 ? ctl.lambda_final : 0.0;
  res->edge_chi2.assign(E, 0.0);
  chi_all(&res->edge_chi2);
  res->S = S;
  res->pose.assign(16 * (size_t)N, 0.0);
  for (int i = 0; i < N; i++) pose_from_sim3(S[i], &res->pose[16 * (size_t)i], nullptr);
}
#endif

}  // namespace esg
}  // namespace mcs
