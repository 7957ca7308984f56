// The camera and pose math that is held to the reference's bits, one definition each, for the
// host and for the device: the Scaramuzza model (Horner, ImgToWorld, WorldToImg), cayley2rot,
// M_t * M_c, invMat, the homogeneous products, WorldToCamHom_fast, ComputeE,
// CheckDistEpipolarLine, isPointInMirrorMask and the predicted pyramid level.  Every kernel and
// host entry that needs one of them calls it here, so all of them give the same bits.
//
// Written with plain operators, so the one requirement is that every includer is compiled with
// -ffp-contract=off: a fused multiply-add would change a rounding.  The build sets it for every
// translation unit of the library (build_hip in __graft_entry__.py), and every host build of the
// tests passes it too.  __host__ __device__ under hipcc, plain inline under a host compiler.
//
// cv::Matx products accumulate s = 0; s += a(i,k) * b(k,j), k ascending.  0.0 + (-0.0) is +0.0, so
// a row that starts from 0 and one that starts from its first product are different sequences.
// Where the callers hold both, both are here under two names (the `0` suffix starts from 0), and
// neither is to be changed into the other.
#pragma once
#include <cmath>
#include <cstdint>
#include "atan_cr.hpp"
#include "../../include/mcs_extractor.h"

namespace mcs {
namespace frm {

// horner (include/misc.h:117-124): c[0] + c[1] x + ... + c[n-1] x^(n-1).  Trailing zero
// coefficients leave a finite x's result as it is (0 * x + 0 = 0, then 0 + c = c exactly), so a
// polynomial padded to 12 terms and the same one at its own degree agree.
MCS_HD inline double horner(const double* c, int n, double x) {
  double r = 0.0;
  for (int i = n - 1; i >= 0; i--) r = r * x + c[i];
  return r;
}

// ImgToWorld (src/cam_model_omni.cpp:49-67)
MCS_HD inline void img_to_world(const mcs_cam_model& m, double u, double v, double* X) {
  const double invAffine = m.c - m.d * m.e;
  const double u_t = u - m.u0, v_t = v - m.v0;
  const double x = (u_t - m.d * v_t) / invAffine;
  const double y = (-m.e * u_t + m.c * v_t) / invAffine;
  const double X2 = x * x, Y2 = y * y;
  const double z = -horner(m.p, m.p_deg, sqrt(X2 + Y2));
  const double norm = sqrt(X2 + Y2 + z * z);
  X[0] = x / norm; X[1] = y / norm; X[2] = z / norm;
}

// The two camera layouts WorldToImg reads: mcs_cam_model at its own degree, and the packed
// cam = c d e u0 v0 invP[12] (zero padded) of the matchers and the BA.  The packed one is read in
// place and where the body uses it (references, the polynomial's address formed in inv_poly), so
// the kernels load a field where they did when each held its own copy of the body.  That only
// keeps their instruction order; no result depends on it.
struct PackedCam { const double &c, &d, &e, &u0, &v0; const double* cam; };
MCS_HD inline double inv_poly(const mcs_cam_model& m, double theta) { return horner(m.invp, m.invp_deg, theta); }
MCS_HD inline double inv_poly(const PackedCam& m, double theta) { return horner(m.cam + 5, 12, theta); }

// WorldToImg (src/cam_model_omni.cpp:147-163).  CR: theta from the correctly rounded atan_cr (the
// host libm's result wherever the libm rounds correctly) for entries whose projection is held to
// the reference's bits on the device; the default is the platform's atan, the device library's
// there and the libm's on the host.
template <bool CR, class Cam>
MCS_HD inline void world_to_img_of(const Cam& m, double x, double y, double z, double& u, double& v) {
  double norm = sqrt(x * x + y * y);
  if (norm == 0.0) norm = 1e-14;
  const double theta = CR ? atan_cr(-z / norm) : atan(-z / norm);
  const double rho = inv_poly(m, theta);
  const double uu = x / norm * rho, vv = y / norm * rho;
  u = uu * m.c + vv * m.d + m.u0;
  v = uu * m.e + vv + m.v0;
}
template <bool CR = false>
MCS_HD inline void world_to_img(const mcs_cam_model& m, double x, double y, double z, double& u,
                                double& v) {
  world_to_img_of<CR>(m, x, y, z, u, v);
}
template <bool CR = false>
MCS_HD inline void world_to_img(const double* cam, double x, double y, double z, double& u,
                                double& v) {
  world_to_img_of<CR>(PackedCam{cam[0], cam[1], cam[2], cam[3], cam[4], cam}, x, y, z, u, v);
}

// cayley2rot (include/misc.h:134-162): R = (1 / scale) * R
MCS_HD inline void cay2rot(const double* c, double* R) {
  const double c1 = c[0], c2 = c[1], c3 = c[2];
  const double c1s = c1 * c1, c2s = c2 * c2, c3s = c3 * c3;
  const double scale = 1.0 + c1s + c2s + c3s;
  const double inv = 1.0 / scale;
  R[0] = inv * (1.0 + c1s - c2s - c3s);
  R[1] = inv * (2.0 * (c1 * c2 - c3));
  R[2] = inv * (2.0 * (c1 * c3 + c2));
  R[3] = inv * (2.0 * (c1 * c2 + c3));
  R[4] = inv * (1.0 - c1s + c2s - c3s);
  R[5] = inv * (2.0 * (c2 * c3 - c1));
  R[6] = inv * (2.0 * (c1 * c3 - c2));
  R[7] = inv * (2.0 * (c2 * c3 + c1));
  R[8] = inv * (1.0 - c1s - c2s + c3s);
}

// cayley2hom (include/misc.h:213-226): the 4x4 [cayley2rot(p) | p[3..5]; 0 0 0 1], row-major
MCS_HD inline void cayley2hom(const double* p, double* T) {
  double R[9];
  cay2rot(p, R);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = p[3 + i];
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
}

// M = M_t * M_c from the minimal pose and mc [6], rows 0..2 of the 4x4 product as R [9], t [3];
// k = 0..3 with the fourth column's 0 and 1 multiplied in.  mtmc starts each row from its first
// product (isInFrustum and the tracking queries), mtmc0 from 0 as cv::Matx does (the BA's
// computeError).
MCS_HD inline void mtmc(const double* pose, const double* mc, double* R, double* t) {
  double Rt[9], Rc[9];
  cay2rot(pose, Rt);
  cay2rot(mc, Rc);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      double s = Rt[3 * i] * Rc[j];
      s += Rt[3 * i + 1] * Rc[3 + j];
      s += Rt[3 * i + 2] * Rc[6 + j];
      s += pose[3 + i] * 0.0;
      R[3 * i + j] = s;
    }
    double s = Rt[3 * i] * mc[3];
    s += Rt[3 * i + 1] * mc[4];
    s += Rt[3 * i + 2] * mc[5];
    s += pose[3 + i] * 1.0;
    t[i] = s;
  }
}
MCS_HD inline void mtmc0(const double* pose, const double* mc, double* R, double* t) {
  double Rt[9], Rc[9];
  cay2rot(pose, Rt);
  cay2rot(mc, Rc);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      s += Rt[3 * i] * Rc[j];
      s += Rt[3 * i + 1] * Rc[3 + j];
      s += Rt[3 * i + 2] * Rc[6 + j];
      s += pose[3 + i] * 0.0;
      R[3 * i + j] = s;
    }
    double s = 0.0;
    s += Rt[3 * i] * mc[3];
    s += Rt[3 * i + 1] * mc[4];
    s += Rt[3 * i + 2] * mc[5];
    s += pose[3 + i] * 1.0;
    t[i] = s;
  }
}

// the same product from the 4x4 matrices themselves (16 doubles row-major, what Get_M_t and
// M_c hold): rows 0..2 of M_t * M_c, cv::Matx order s = 0; s += a(i,k) b(k,j), k = 0..3
MCS_HD inline void mtmc44(const double* Mt, const double* Mc, double* R, double* t) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += Mt[4 * i + k] * Mc[4 * k + j];
      if (j < 3) R[3 * i + j] = s; else t[i] = s;
    }
}

// invMat (src/cConverter.cpp:31-44) of a row-major 4x4: R' = R^T, t' = -R' * t from s = 0
MCS_HD inline void inv_mat44(const double* M, double* R, double* t) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = M[4 * j + i];
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += -R[3 * i + k] * M[4 * k + 3];
    t[i] = s;
  }
}
// the same of [R | t] held as R [9], t [3] (k_fuse_setup, k_np_verdict's table, the host's E table)
MCS_HD inline void inv_rt(const double* R, const double* t, double* Ri, double* ti) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Ri[3 * i + j] = R[3 * j + i];
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += t[k] * -R[3 * k + i];
    ti[i] = s;
  }
}

// rows 0..2 of the 4x4 [A b; 0 0 0 1] times (x, 1): s = 0; s += a(i,k) x(k), k = 0..2; + b * 1.0
MCS_HD inline void hom_mul(const double* A, const double* b, const double* x, double* y) {
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += A[3 * i + k] * x[k];
    y[i] = s + b[i] * 1.0;
  }
}

// y = A * x + b: the Matx33d * Vec3d product (s = 0; s += a(i,k) x(k)), then the Vec sum
MCS_HD inline void rot_add(const double* A, const double* x, const double* b, double* y) {
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += A[3 * i + k] * x[k];
    y[i] = s + b[i];
  }
}

// WorldToCamHom_fast (src/cam_system_omni.cpp:92-112): invMat(M_t M_c) * [X 1], then WorldToImg,
// from M_t M_c as R [9], t [3].  The rows of invMat's t' and of the point start from their first
// products (the projections of the frame and the matchers).  The same from s = 0, as cv::Matx
// does, is inv_rt, hom_mul and world_to_img in turn (the BA's edge_error).
template <bool CR = false>
MCS_HD inline void world_to_cam_img(const double* R, const double* t, const double* cam,
                                    const double* X, double& u, double& v) {
  double ti[3];   // invMat: R' = R^T, t' = -R' t (src/cConverter.cpp:31-44)
  for (int i = 0; i < 3; i++) {
    double s = -R[i] * t[0];
    s += -R[3 + i] * t[1];
    s += -R[6 + i] * t[2];
    ti[i] = s;
  }
  double Xc[3];
  for (int i = 0; i < 3; i++) {
    double s = R[i] * X[0];
    s += R[3 + i] * X[1];
    s += R[6 + i] * X[2];
    s += ti[i] * 1.0;
    Xc[i] = s;
  }
  world_to_img<CR>(cam, Xc[0], Xc[1], Xc[2], u, v);
}
// ComputeE (src/misc.cpp:72-86) of T1 = [R1w | t1w] and T2 = [R2w | t2w] (R [9], t [3]; the
// matcher passes KF1's MtMc_inv and KF2's MtMc), E [9].  Every product accumulates from s = 0 in
// k order (cv::Matx), `t12 /= norm` multiplies by 1. / norm (cv::Vec::operator/=), norm = sqrt
// of the in-order sum of squares.
MCS_HD inline void compute_e(const double* R1w, const double* t1w, const double* R2w,
                             const double* t2w, double* E) {
  double R12[9], t12[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {   // R12 = R1w * R2w.t()
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += R1w[3 * i + k] * R2w[3 * j + k];
      R12[3 * i + j] = s;
    }
    double s = 0.0;                 // t12 = -R1w * R2w.t() * t2w + t1w
    for (int j = 0; j < 3; j++) {
      double a = 0.0;
      for (int k = 0; k < 3; k++) a += -R1w[3 * i + k] * R2w[3 * j + k];
      s += a * t2w[j];
    }
    t12[i] = s + t1w[i];
  }
  double ss = 0.0;
  for (int i = 0; i < 3; i++) ss += t12[i] * t12[i];
  const double ialpha = 1. / sqrt(ss);   // t12 /= cv::norm(t12)
  for (int i = 0; i < 3; i++) t12[i] = t12[i] * ialpha;
  const double S[9] = {0.0, -t12[2], t12[1], t12[2], 0.0, -t12[0], -t12[1], t12[0], 0.0};   // Skew
  for (int i = 0; i < 3; i++)       // t12x * R12
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += S[3 * i + k] * R12[3 * k + j];
      E[3 * i + j] = s;
    }
}

// CheckDistEpipolarLine (src/misc.cpp:54-70).  nom = (ray2^T E12) ray1 evaluated left to right
// as cv::Matx does; (ray2^T E12)_c = sum_r ray2_r E_rc is exactly Etx2_c, so nom = Etx2 . ray1.
// The host entry and the device searches give the same verdict bit for bit.
MCS_HD inline bool epi_check(const double* r1, const double* r2, const double* Em, double thresh) {
  double Ex1[3], Etx2[3];
  for (int r = 0; r < 3; r++) {
    Ex1[r] = Em[3 * r] * r1[0] + Em[3 * r + 1] * r1[1] + Em[3 * r + 2] * r1[2];
    Etx2[r] = r2[0] * Em[r] + r2[1] * Em[3 + r] + r2[2] * Em[6 + r];
  }
  const double nom = Etx2[0] * r1[0] + Etx2[1] * r1[1] + Etx2[2] * r1[2];
  const double den = Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1] + Ex1[2] * Ex1[2] + Etx2[0] * Etx2[0] +
                     Etx2[1] * Etx2[1] + Etx2[2] * Etx2[2];
  if (den == 0.0) return false;
  return (nom * nom) / den < thresh;
}

// isPointInMirrorMask(u, v, 0) (src/cam_model_omni.cpp:165-180) on camera c's mask of
// mask [n_cams][mh][mw]: cvRound, bounds (> 0 and < size), mask > 0
MCS_HD inline bool in_mirror_mask(const uint8_t* mask, int c, int mw, int mh, double u, double v) {
  const int ur = (int)rint(u), vr = (int)rint(v);
  return !(ur >= mw || ur <= 0 || vr >= mh || vr <= 0) &&
         mask[(int64_t)c * mw * mh + (int64_t)vr * mw + ur] != 0;
}

// nPredictedLevel = lower_bound(mvScaleFactors, dist / minDistance), capped at L - 1
MCS_HD inline int predict_level(const double* scale, int L, double ratio) {
  int lv = 0;
  while (lv < L && scale[lv] < ratio) lv++;
  if (lv >= L) lv = L - 1;
  return lv;
}

}  // namespace frm
}  // namespace mcs
