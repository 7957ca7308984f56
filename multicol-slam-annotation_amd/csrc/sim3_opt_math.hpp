// cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:63-270) for ONE candidate, as plain
// functions: g2o::Sim3 (ThirdParty/g2o/g2o/types/sim3.h:41-292) with Eigen's quaternion
// conversions, the two edges of include/g2o_MultiCol_sim3_expmap.h:193-260, their analytic 2x7
// Jacobians, the 7x7 solve and the two-round loop over g2o's LM control (lm_control.hpp).
// k_sim3_opt (sim3_opt.hip) runs the same functions with the edges spread over a workgroup; its
// control flow mirrors optimize_sim3_one below.  invMat, the homogeneous product and WorldToImg
// are frm:: of omni_geom.hpp.  No HIP include: __host__ __device__ under hipcc, inline under a
// host compiler.  Needs -ffp-contract=off.
#pragma once
#include "lm_control.hpp"
#include "omni_geom.hpp"
#include "../../include/mcs_matcher.h"
#include <math.h>

// full unrolling keeps the small fixed-size arrays in registers on the device
#if defined(__clang__)
#define MCS_S3O_UNROLL _Pragma("unroll")
#else
#define MCS_S3O_UNROLL
#endif

namespace mcs {
namespace s3o {

constexpr int kMaxIts = 16;        // iterations per round the trial log holds
constexpr int kSums = 36;          // 28 upper entries of H, 7 of b, chi2

struct Sim3 { double q[4], t[3], s; };   // q = w x y z

// one kept slot (:139-200): the fixed points in their rig frames, both observations with their
// informations, the camera each edge projects with, the slot
struct Row {
  double X1[3], X2[3], o1[2], o2[2], w1, w2;
  int32_t c12, c21, slot, alive;
};

// ---------------------------------------------------------------------------- Eigen's quaternion
// Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<.., 3, 3>)
MCS_LM_FN void quat_from_rot(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (m[7] - m[5]) * t;
    q[2] = (m[2] - m[6]) * t;
    q[3] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[3 * k + j] - m[3 * j + k]) * t;
    q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t;
    q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t;
  }
}

// toRotationMatrix
MCS_LM_FN void quat_to_rot(const double* q, double* R) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// q * v (_transformVector): uv = 2 (vec x v); v + w uv + vec x uv
MCS_LM_FN void quat_rot(const double* q, const double* v, double* o) {
  double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
  for (int i = 0; i < 3; i++) uv[i] += uv[i];
  const double c[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
  for (int i = 0; i < 3; i++) o[i] = v[i] + q[0] * uv[i] + c[i];
}

MCS_LM_FN void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

// ---------------------------------------------------------------------------- g2o::Sim3
MCS_LM_FN Sim3 sim3_from_srt(double s, const double* R, const double* t) {   // sim3.h:64-67
  Sim3 S;
  quat_from_rot(R, S.q);
  for (int i = 0; i < 3; i++) S.t[i] = t[i];
  S.s = s;
  return S;
}

MCS_LM_FN void mat3_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += A[3 * i + k] * B[3 * k + j];
      C[3 * i + j] = s;
    }
}

// Sim3(Vector7d update), update = (omega, upsilon, sigma) (sim3.h:70-142) with its eps branches
MCS_LM_FN Sim3 sim3_exp(const double* u) {
  const double* w = u;
  const double sigma = u[6];
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double Om[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double Om2[9], R[9];
  mat3_mul(Om, Om, Om2);
  Sim3 S;
  S.s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C;
  if (fabs(sigma) < eps) {
    C = 1.0;
    if (theta < eps) {
      A = 1. / 2.;
      B = 1. / 6.;
      for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + Om[k] + Om2[k];
    } else {
      const double theta2 = theta * theta;
      A = (1.0 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
      const double a = sin(theta) / theta, b = (1.0 - cos(theta)) / (theta * theta);
      for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + a * Om[k] + b * Om2[k];
    }
  } else {
    C = (S.s - 1.0) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
      for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + Om[k] + Om2[k];
    } else {
      const double a1 = sin(theta) / theta, b1 = (1.0 - cos(theta)) / (theta * theta);
      for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + a1 * Om[k] + b1 * Om2[k];
      const double a = S.s * sin(theta), b = S.s * cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  quat_from_rot(R, S.q);
  for (int i = 0; i < 3; i++) {          // t = (A Omega + B Omega2 + C I) upsilon
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += (A * Om[3 * i + k] + B * Om2[3 * i + k] + (i == k ? C : 0.0)) * u[3 + k];
    S.t[i] = s;
  }
  return S;
}

MCS_LM_FN void sim3_map(const Sim3& S, const double* x, double* y) {   // s * (r * xyz) + t
  double r[3];
  quat_rot(S.q, x, r);
  for (int i = 0; i < 3; i++) y[i] = S.s * r[i] + S.t[i];
}

MCS_LM_FN Sim3 sim3_mul(const Sim3& a, const Sim3& b) {                // sim3.h:266-272
  Sim3 o;
  quat_mul(a.q, b.q, o.q);
  double r[3];
  quat_rot(a.q, b.t, r);
  for (int i = 0; i < 3; i++) o.t[i] = a.s * r[i] + a.t[i];
  o.s = a.s * b.s;
  return o;
}

MCS_LM_FN Sim3 sim3_inverse(const Sim3& a) {                           // sim3.h:233-236
  Sim3 o;
  o.q[0] = a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = -a.q[3];
  const double k = -1. / a.s;
  const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
  quat_rot(o.q, v, o.t);
  o.s = 1. / a.s;
  return o;
}

// ---------------------------------------------------------------------------- the projection
// invMat of a row-major 4x4 and rows 0..2 of [R t; 0 0 0 1] * (x, 1): the shared definitions
using frm::hom_mul;
using frm::inv_mat44;

// WorldToImg (frm::world_to_img of omni_geom.hpp), cam = c d e u0 v0 invP[12]; with Jp the 2x3
// derivative with respect to (x, y, z): the chain through norm, theta and the 12-term polynomial
MCS_LM_FN void world_to_img_jac(const double* cam, const double* p, double* uv, double* Jp) {
  const double x = p[0], y = p[1], z = p[2];
  double n = sqrt(x * x + y * y);   // the norm, theta and rho that WorldToImg forms and does not return
  if (n == 0.0) n = 1e-14;
  const double theta = atan(-z / n);
  const double rho = frm::horner(cam + 5, 12, theta);
  const double cx = x / n, cy = y / n;
  frm::world_to_img(cam, x, y, z, uv[0], uv[1]);
  if (!Jp) return;
  double drho = 0.0;
  for (int i = 11; i >= 1; i--) drho = drho * theta + i * cam[5 + i];
  const double r2 = n * n + z * z;
  const double th_n = z / r2, th_z = -n / r2;                // d theta / d norm, d theta / d z
  const double th_x = th_n * cx, th_y = th_n * cy;
  const double in = 1.0 / n;
  // uu = x rho / n
  const double du[3] = {rho * in - cx * cx * rho * in + cx * drho * th_x, -cx * cy * rho * in + cx * drho * th_y,
                        cx * drho * th_z};
  const double dv[3] = {-cx * cy * rho * in + cy * drho * th_x, rho * in - cy * cy * rho * in + cy * drho * th_y,
                        cy * drho * th_z};
  for (int k = 0; k < 3; k++) {
    Jp[k] = du[k] * cam[0] + dv[k] * cam[1];
    Jp[3 + k] = du[k] * cam[2] + dv[k];
  }
}

// ---------------------------------------------------------------------------- the edges
// kind 0: EdgeSim3ProjectXYZ_Multi (:200-213), err = obs1 - cam_map1(S.map(X2));
// kind 1: EdgeInverseSim3ProjectXYZ_Multi (:234-247), err = obs2 - cam_map2(S^-1.map(X1)).
// imc [C][12] = invMat(M_c) as R 9, t 3; cam [C][17].  J (nullable) [2][7]: d err / d delta of
// the left update exp(delta) * S at delta = 0, delta = (omega, upsilon, sigma):
//   kind 0: d (exp(delta) Y) = [-[Y]x | I | Y] with Y = S X2
//   kind 1: d ((exp(delta) S)^-1 X1) = (1 / s) R^T [[X1]x | -I | -X1]
MCS_LM_FN void edge_eval(const Sim3& S, const Sim3& Si, const Row& r, int kind, const double* imc,
                         const double* cam, double* err, double* J) {
  const int c = kind ? r.c21 : r.c12;
  const double* X = kind ? r.X1 : r.X2;
  const double* obs = kind ? r.o2 : r.o1;
  double Y[3], p[3], uv[2], Jp[6];
  sim3_map(kind ? Si : S, X, Y);
  hom_mul(imc + 12 * c, imc + 12 * c + 9, Y, p);
  world_to_img_jac(cam + 17 * c, p, uv, J ? Jp : nullptr);
  err[0] = obs[0] - uv[0];
  err[1] = obs[1] - uv[1];
  if (!J) return;
  double D[21];                            // 3 x 7
  if (!kind) {
    const double M[21] = {0.0,   Y[2], -Y[1], 1.0, 0.0, 0.0, Y[0],
                          -Y[2], 0.0,  Y[0],  0.0, 1.0, 0.0, Y[1],
                          Y[1], -Y[0], 0.0,   0.0, 0.0, 1.0, Y[2]};
    for (int k = 0; k < 21; k++) D[k] = M[k];
  } else {
    double A[9];
    quat_to_rot(Si.q, A);
    for (int k = 0; k < 9; k++) A[k] *= Si.s;
    const double M[21] = {0.0,  -X[2], X[1], -1.0, 0.0,  0.0,  -X[0],
                          X[2], 0.0,  -X[0], 0.0,  -1.0, 0.0,  -X[1],
                          -X[1], X[0], 0.0,  0.0,  0.0,  -1.0, -X[2]};
    MCS_S3O_UNROLL
    for (int i = 0; i < 3; i++)
      MCS_S3O_UNROLL
      for (int j = 0; j < 7; j++) D[7 * i + j] = A[3 * i] * M[j] + A[3 * i + 1] * M[7 + j] + A[3 * i + 2] * M[14 + j];
  }
  double G[6];                             // Jp * R(invMat(M_c))
  const double* Rc = imc + 12 * c;
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) G[3 * i + j] = Jp[3 * i] * Rc[j] + Jp[3 * i + 1] * Rc[3 + j] + Jp[3 * i + 2] * Rc[6 + j];
  MCS_S3O_UNROLL
  for (int i = 0; i < 2; i++)
    MCS_S3O_UNROLL
    for (int j = 0; j < 7; j++) J[7 * i + j] = -(G[3 * i] * D[j] + G[3 * i + 1] * D[7 + j] + G[3 * i + 2] * D[14 + j]);
}

MCS_LM_FN double edge_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// RobustKernelHuber (robust_kernel_impl.cpp:65-91): dsqr is a float member
MCS_LM_FN double huber_dsqr(double delta) { return (double)(float)(delta * delta); }
MCS_LM_FN void huber(double e, double delta, double dsqr, double* rho0, double* rho1) {
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
  else { const double sq = sqrt(e); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

// one edge into acc[kSums]: H (upper, row-major 28) += J^T (rho1 w) J, b (7) += -J^T rho1 w e,
// chi2 += rho0 (base_binary_edge.hpp:91-113 with the Sim3 as the one free vertex)
MCS_LM_FN void edge_accumulate(const Sim3& S, const Sim3& Si, const Row& r, int kind, const double* imc,
                               const double* cam, double delta, double dsqr, double* acc) {
  double e[2], J[14], rho0, rho1;
  edge_eval(S, Si, r, kind, imc, cam, e, J);
  const double w = kind ? r.w2 : r.w1;
  huber(edge_chi2(e, w), delta, dsqr, &rho0, &rho1);
  const double wr = rho1 * w;
  int k = 0;
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++)
    MCS_S3O_UNROLL
    for (int j = i; j < 7; j++) acc[k++] += wr * (J[i] * J[j] + J[7 + i] * J[7 + j]);
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++) acc[28 + i] += -wr * (J[i] * e[0] + J[7 + i] * e[1]);
  acc[35] += rho0;
}

MCS_LM_FN double max_diag(const double* acc) {
  double m = 0.0;
  int k = 0;
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++) { m = __builtin_fmax(__builtin_fabs(acc[k]), m); k += 7 - i; }
  return m;
}

// (H + lambda I) x = b by LDL^T without pivoting; false = a pivot that is not positive.  Also the
// LM model decrease sum x (lambda x + b) (computeScale, optimization_algorithm_levenberg.cpp:182-189)
MCS_LM_FN bool solve7(const double* acc, double lambda, double* x, double* scale) {
  double L[7][7], d[7], y[7];
  int k = 0;
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++)
    MCS_S3O_UNROLL
    for (int j = i; j < 7; j++) { L[j][i] = acc[k++]; if (i == j) L[i][i] += lambda; }
  bool ok = true;
  MCS_S3O_UNROLL
  for (int j = 0; j < 7; j++) {
    double dj = L[j][j];
    MCS_S3O_UNROLL
    for (int m = 0; m < j; m++) dj -= L[j][m] * L[j][m] * d[m];
    if (!(dj > 0.0)) { ok = false; dj = 1.0; }
    d[j] = dj;
    MCS_S3O_UNROLL
    for (int i = j + 1; i < 7; i++) {
      double s = L[i][j];
      MCS_S3O_UNROLL
      for (int m = 0; m < j; m++) s -= L[i][m] * L[j][m] * d[m];
      L[i][j] = s / dj;
    }
  }
  const double* b = acc + 28;
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++) {
    double s = b[i];
    MCS_S3O_UNROLL
    for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
    y[i] = s;
  }
  MCS_S3O_UNROLL
  for (int i = 6; i >= 0; i--) {
    double s = y[i] / d[i];
    MCS_S3O_UNROLL
    for (int m = i + 1; m < 7; m++) s -= L[m][i] * x[m];
    x[i] = s;
  }
  double sc = 0.0;
  MCS_S3O_UNROLL
  for (int i = 0; i < 7; i++) sc += x[i] * (lambda * x[i] + b[i]);
  *scale = sc;
  return ok;
}

// ---------------------------------------------------------------------------- the slot rules
// :122-161 for slot i of KF1 against one candidate.  k* = the keyframe's own arrays (already at its
// first keypoint), n_1 / n_2 its keypoint counts, m = matches12[i].  0 = skipped, 1 = kept (row
// filled except the points), 2 = dropped because the crossed camera lookup leaves its map.
struct KfView {
  int n;
  const float* xy; const int32_t* oct; const int32_t* cam;
};

MCS_LM_FN int slot_rule(const KfView& k1, const KfView& k2, int i, int m, const uint8_t* ok1, const uint8_t* ok2,
                        const int32_t* first2, int L, int C, int own_camera, const double* inv_sigma2_1,
                        const double* sigma2_2, Row* r) {
  if (m < 0 || m >= k2.n || i >= k1.n) return 0;
  if (ok1[i] == 0 || ok2[m] == 0) return 0;
  const int i2 = first2[m];
  if (i2 < 0 || i2 >= k2.n) return 0;
  const int a = own_camera ? i : i2, b = own_camera ? i2 : i;   // keypoint_to_cam1[a], keypoint_to_cam2[b]
  if (a >= k1.n || b >= k2.n) return 2;
  const int oc1 = k1.oct[i], oc2 = k2.oct[i2], c12 = k1.cam[a], c21 = k2.cam[b];
  if (oc1 < 0 || oc1 >= L || oc2 < 0 || oc2 >= L || c12 < 0 || c12 >= C || c21 < 0 || c21 >= C) return 0;
  if (r) {
    r->o1[0] = (double)k1.xy[2 * i]; r->o1[1] = (double)k1.xy[2 * i + 1];
    r->o2[0] = (double)k2.xy[2 * i2]; r->o2[1] = (double)k2.xy[2 * i2 + 1];
    r->w1 = inv_sigma2_1[oc1];
    r->w2 = sigma2_2[oc2];
    r->c12 = c12; r->c21 = c21; r->slot = i; r->alive = 1;
  }
  return 1;
}

// ---------------------------------------------------------------------------- one candidate
struct Result {
  int n_in, n_corr, n_bad;
  Sim3 S;
  int iters[2];
  double chi2[2], lambda[2];
  int trials[2][kMaxIts];      // LM trials of every iteration (levenbergIteration())
};

MCS_LM_FN mcs_ba_options lm_options(const mcs_sim3_opt_options& o, int its) {
  mcs_ba_options b;
  b.max_iterations = its; b.gain_threshold = o.gain_threshold; b.terminate_max_iter = o.terminate_max_iter;
  b.max_trials = o.max_trials; b.tau = o.tau;
  return b;
}

// the sums of all live edges at S, in row order, e12 before e21
MCS_LM_FN void sums_at(const Sim3& S, const Row* rows, int n, const double* imc, const double* cam, double delta,
                       double dsqr, double* acc) {
  const Sim3 Si = sim3_inverse(S);
  for (int k = 0; k < kSums; k++) acc[k] = 0.0;
  for (int kind = 0; kind < 2; kind++)
    for (int j = 0; j < n; j++)
      if (rows[j].alive) edge_accumulate(S, Si, rows[j], kind, imc, cam, delta, dsqr, acc);
}

// optimize(its) of one round (sparse_optimizer.cpp:354-419 over lm_control.hpp): *stop is the
// terminate action's flag, which lives across the rounds
MCS_LM_FN void run_round(Sim3* S, const Row* rows, int n, const double* imc, const double* cam,
                         const mcs_sim3_opt_options& o, int its, int* stop, int round, Result* res) {
  const double delta = 1.345 * o.std_sim, dsqr = huber_dsqr(delta);
  res->iters[round] = 0; res->chi2[round] = 0.0; res->lambda[round] = 0.0;
  for (int k = 0; k < kMaxIts; k++) res->trials[round][k] = 0;
  int live = 0;
  for (int j = 0; j < n; j++) live += rows[j].alive != 0;
  if (live == 0) return;                       // "0 vertices to optimize": optimize returns -1
  ba::LmCtl ctl;
  ba::lm_init(ctl, lm_options(o, its));
  double cur[kSums], tri[kSums], x[7], scale;
  sums_at(*S, rows, n, imc, cam, delta, dsqr, cur);
  ba::lm_start_body(&ctl, cur[35]);
  ctl.done = (its <= 0 || *stop) ? 1 : 0;
  for (int g = 0; g < its * o.max_trials && !ctl.done; g++) {
    if (ctl.lin && ctl.iter == 0) { const double mx = max_diag(cur); ba::lm_lambda0_body(&ctl, mx, mx); }
    const bool ok = solve7(cur, ctl.lambda, x, &scale);
    const Sim3 bak = *S;
    *S = sim3_mul(sim3_exp(x), bak);           // oplusImpl (:131-140)
    sums_at(*S, rows, n, imc, cam, delta, dsqr, tri);
    const double sc[3] = {tri[35], 0.0, scale};
    const int it = ctl.iter;
    ba::lm_step(&ctl, sc, !ok, false, *stop);
    if (it < kMaxIts) res->trials[round][it]++;
    if (ctl.restore) *S = bak;
    else for (int k = 0; k < kSums; k++) cur[k] = tri[k];
    if (ctl.stop_out) *stop = 1;
  }
  res->iters[round] = ctl.iter;
  res->chi2[round] = ctl.currentChi;
  res->lambda[round] = ctl.iter > 0 ? ctl.lambda_final : 0.0;
}

// :212-232 / :247-263: every live pair with a chi2 strictly above deltaHuber2 is taken out and
// its match nulled; returns how many.  edge_chi2 (nullable) [n1][2] gets the pair's two values.
MCS_LM_FN int cull(const Sim3& S, Row* rows, int n, const double* imc, const double* cam, double std_sim,
                   int32_t* matches12, double* edge_chi2_out) {
  const double dh = 1.345 * std_sim, dh2 = dh * dh;
  const Sim3 Si = sim3_inverse(S);
  int bad = 0;
  for (int j = 0; j < n; j++) {
    if (!rows[j].alive) continue;
    double e[2];
    edge_eval(S, Si, rows[j], 0, imc, cam, e, nullptr);
    const double c12 = edge_chi2(e, rows[j].w1);
    edge_eval(S, Si, rows[j], 1, imc, cam, e, nullptr);
    const double c21 = edge_chi2(e, rows[j].w2);
    if (edge_chi2_out) { edge_chi2_out[2 * rows[j].slot] = c12; edge_chi2_out[2 * rows[j].slot + 1] = c21; }
    if (c12 > dh2 || c21 > dh2) { rows[j].alive = 0; matches12[rows[j].slot] = -1; bad++; }
  }
  return bad;
}

// The function body after the rows are built (:207-269).  Returns nIn; *S is the recovered Sim3,
// untouched on the `< 3` return.
MCS_LM_FN int optimize_sim3_one(Row* rows, int n, const double* imc, const double* cam,
                                const mcs_sim3_opt_options& o, int32_t* matches12, double* edge_chi2_out,
                                Sim3* S, Result* res) {
  Sim3 W = *S;
  int stop = 0;
  res->n_corr = n;
  run_round(&W, rows, n, imc, cam, o, o.its_round1, &stop, 0, res);
  res->n_bad = cull(W, rows, n, imc, cam, o.std_sim, matches12, edge_chi2_out);
  res->iters[1] = 0; res->chi2[1] = 0.0; res->lambda[1] = 0.0;
  for (int k = 0; k < kMaxIts; k++) res->trials[1][k] = 0;
  res->S = *S;
  res->n_in = 0;
  if (n - res->n_bad < 3) return 0;
  run_round(&W, rows, n, imc, cam, o, res->n_bad > 0 ? o.its_culled : o.its_clean, &stop, 1, res);
  const int bad2 = cull(W, rows, n, imc, cam, o.std_sim, matches12, edge_chi2_out);
  res->n_in = n - res->n_bad - bad2;
  *S = W;
  res->S = W;
  return res->n_in;
}

}  // namespace s3o
}  // namespace mcs
