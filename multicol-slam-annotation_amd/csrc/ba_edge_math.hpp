// The BA edge math that is pinned against the reference text: the projection error of
// EdgeProjectXYZ2MCS and its analytic Jacobians, g2o's Huber kernel and the 3x3 point-block
// algebra of BlockSolver<6,3> (same operation order as oracle/ba_oracle.cpp).  The Cayley
// rotation, M_t M_c, invMat, WorldToImg and the Horner polynomial are frm:: of omni_geom.hpp.
// No device state: every function takes plain pointers, so another solver can include it.
#pragma once
#include <hip/hip_runtime.h>
#include "omni_geom.hpp"

namespace mcs::ba {
// err = meas - WorldToImg((M_t M_c)^-1 X): the reference's 4x4 path (computeError), every
// cv::Matx row from s = 0: M_t M_c, its invMat, the homogeneous product, WorldToImg
__device__ void edge_error(const double* pose, const double* X, const double* mc,
                           const double* cam, const double* meas, double* err) {
  double R[9], t[3], Ri[9], ti[3], Xc[3], u, v;
  frm::mtmc0(pose, mc, R, t);
  frm::inv_rt(R, t, Ri, ti);
  frm::hom_mul(Ri, ti, X, Xc);
  frm::world_to_img(cam, Xc[0], Xc[1], Xc[2], u, v);
  err[0] = meas[0] - u;
  err[1] = meas[1] - v;
}

__device__ void dcay(const double* c, int k, const double* R, double* D) {
  const double s = 1 + c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double v = (i == j) ? -2 * c[k] : 0.0;
      v += 2 * (((i == k) ? c[j] : 0.0) + ((j == k) ? c[i] : 0.0));
      // [e_k]x
      double ex = 0;
      if (k == 0) ex = (i == 1 && j == 2) ? -1 : ((i == 2 && j == 1) ? 1 : 0);
      if (k == 1) ex = (i == 0 && j == 2) ? 1 : ((i == 2 && j == 0) ? -1 : 0);
      if (k == 2) ex = (i == 0 && j == 1) ? -1 : ((i == 1 && j == 0) ? 1 : 0);
      v += 2 * ex;
      D[3 * i + j] = v / s - R[3 * i + j] * 2 * c[k] / s;
    }
}

// analytic Jacobians of err: jp [2][6], jl [2][3].  X_c comes by the 3x3
// path R^T (X - t), not edge_error's 4x4 path.
__device__ void edge_jac(const double* pose, const double* X, const double* mc, const double* cam,
                         double* jp, double* jl) {
  double Rt[9], Rc[9], R[9];
  frm::cay2rot(pose, Rt);
  frm::cay2rot(mc, Rc);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += Rt[3 * i + k] * Rc[3 * k + j];
      R[3 * i + j] = s;
    }
  double t[3];
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += Rt[3 * i + k] * mc[3 + k];
    t[i] = s + pose[3 + i];
  }
  double Xc[3];
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += R[3 * k + i] * (X[k] - t[k]);
    Xc[i] = s;
  }
  const double x = Xc[0], y = Xc[1], z = Xc[2];
  double rho = sqrt(x * x + y * y);
  if (rho == 0.0) rho = 1e-14;
  const double theta = atan(-z / rho);
  const double* a = cam + 5;
  const double r = frm::horner(a, 12, theta);
  double dr = 0;
  for (int k = 11; k >= 1; k--) dr = dr * theta + k * a[k];
  const double den = rho * rho + z * z;
  const double dth_dx = z / den * x / rho, dth_dy = z / den * y / rho, dth_dz = -rho / den;
  const double g = r / rho;
  const double dg_dx = dr * dth_dx / rho - r * x / (rho * rho * rho);
  const double dg_dy = dr * dth_dy / rho - r * y / (rho * rho * rho);
  const double dg_dz = dr * dth_dz / rho;
  const double dm[2][3] = {{g + x * dg_dx, x * dg_dy, x * dg_dz}, {y * dg_dx, g + y * dg_dy, y * dg_dz}};
  const double c = cam[0], d = cam[1], e = cam[2];
  double Jm[2][3];
  for (int j = 0; j < 3; j++) {
    Jm[0][j] = c * dm[0][j] + d * dm[1][j];
    Jm[1][j] = e * dm[0][j] + dm[1][j];
  }
  double JX[2][3];
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += Jm[i][k] * R[3 * j + k];
      JX[i][j] = s;
    }
  const double q[3] = {X[0] - pose[3], X[1] - pose[4], X[2] - pose[5]};
  for (int k = 0; k < 3; k++) {
    double D[9];
    dcay(pose, k, Rt, D);
    double w[3], dx[3];
    for (int i = 0; i < 3; i++) {
      double s = 0;
      for (int m = 0; m < 3; m++) s += D[3 * m + i] * q[m];
      w[i] = s;
    }
    for (int i = 0; i < 3; i++) {
      double s = 0;
      for (int m = 0; m < 3; m++) s += Rc[3 * m + i] * w[m];
      dx[i] = s;
    }
    for (int i = 0; i < 2; i++) {
      double s = 0;
      for (int m = 0; m < 3; m++) s += Jm[i][m] * dx[m];
      jp[6 * i + k] = -s;
    }
  }
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      jp[6 * i + 3 + j] = JX[i][j];
      jl[3 * i + j] = -JX[i][j];
    }
}

// RobustKernelHuber keeps delta^2 in a FLOAT member (ThirdParty/g2o/g2o/core/robust_kernel_impl.h:84,
// `float dsqr;`, set by setDelta as dsqr = delta*delta, robust_kernel_impl.cpp:65-69), so the
// inlier test and rho(e) = 2 sqrt(e) delta - dsqr use delta^2 rounded to float.  (The culling
// thresholds of cOptimizer, thHuber2 = thHuber*thHuber, stay double: src/cOptimizer.cpp:436.)
static inline double huber_dsqr(double delta) { return (double)(float)(delta * delta); }

__device__ __forceinline__ void huber(double e, double delta, double dsqr, double* rho0, double* rho1) {
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
  else { const double sq = sqrt(e); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

// D = Hll + lambda I -> Dinv = D.inverse() as the reference's Eigen 3.2.10 computes a fixed
// 3x3 inverse (ThirdParty/Eigen/Eigen/src/LU/Inverse.h:117-159): cofactor(i, j) =
// m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1) with i1 = i+1, i2 = i+2, j1 = j+1, j2 = j+2 (mod 3);
// det = the column-0 cofactors times column 0, summed by redux_novec_unroller (Redux.h:77-106:
// a 3-vector of Matrix<double,3,1> is not packet-aligned in 3.2, so c0 + (c1 + c2)); row 0 of
// the inverse = the column-0 cofactors, entry (r, c) otherwise = cofactor(c, r), each times
// 1 / det.  Pinned by tests/golden/g2o_schur.npz.  (k_point_trial and k_build_trial share it.)
__host__ __device__ __forceinline__ void dinv_of(const double* H, double lam, double (&Di)[9]) {
  double m[9];
  for (int k = 0; k < 9; k++) m[k] = H[k];
  m[0] += lam; m[4] += lam; m[8] += lam;
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
  };
  const double k0 = cof(0, 0), k1 = cof(1, 0), k2 = cof(2, 0);
  const double det = k0 * m[0] + (k1 * m[3] + k2 * m[6]);
  const double id = 1.0 / det;
  Di[0] = k0 * id; Di[1] = k1 * id; Di[2] = k2 * id;
  Di[3] = cof(0, 1) * id; Di[4] = cof(1, 1) * id; Di[5] = cof(2, 1) * id;
  Di[6] = cof(0, 2) * id; Di[7] = cof(1, 2) * id; Di[8] = cof(2, 2) * id;
}
// db = Dinv * b_l (CoeffBasedProduct, CoeffBasedProduct.h:240-258: k ascending)
__host__ __device__ __forceinline__ void db_of(const double (&Di)[9], const double* b, double* db) {
  for (int a = 0; a < 3; a++) db[a] = Di[3 * a] * b[0] + Di[3 * a + 1] * b[1] + Di[3 * a + 2] * b[2];
}
// Y = Hpl * Dinv (BDinv = (*Bi) * Dinv, block_solver.hpp:403), same product order
__host__ __device__ __forceinline__ void ybl_of(const double* B, const double (&Di)[9], double* Y) {
  double bb[18];
  for (int k = 0; k < 18; k++) bb[k] = B[k];
  for (int a = 0; a < 6; a++)
    for (int c = 0; c < 3; c++)
      Y[3 * a + c] = bb[3 * a] * Di[c] + bb[3 * a + 1] * Di[3 + c] + bb[3 * a + 2] * Di[6 + c];
}

}  // namespace mcs::ba
