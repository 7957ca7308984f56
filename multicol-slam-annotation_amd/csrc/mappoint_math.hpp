// Device arithmetic of cMapPoint::UpdateNormalAndDepth (src/cMapPoint.cpp:453-496), shared by
// mappoint.hip (the batched refresh) and new_points.hip (the admit step of CreateNewMapPoints):
// one definition each, so both give the same bits.  The reference's cv::Vec3d arithmetic:
// v / a is v * (1. / a) (Vec operator/ -> Matx_ScaleOp), sums in observation order.
// Translation units that include this are compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace mcs {
namespace mpt {

// cv::norm of a Vec3d: sqrt of the in-order sum of squares (normL2Sqr)
__device__ __forceinline__ double norm3(double x, double y, double z) {
  double s = 0.0;
  s = __dadd_rn(s, __dmul_rn(x, x));
  s = __dadd_rn(s, __dmul_rn(y, y));
  s = __dadd_rn(s, __dmul_rn(z, z));
  return __dsqrt_rn(s);
}

// normal = normal + normali / cv::norm(normali), normali = Pos - Owi (:474-476)
__device__ __forceinline__ void add_view_dir(double X, double Y, double Z, const double* O, double& nx,
                                             double& ny, double& nz) {
  const double ax = __dsub_rn(X, O[0]), ay = __dsub_rn(Y, O[1]), az = __dsub_rn(Z, O[2]);
  const double ia = __ddiv_rn(1.0, norm3(ax, ay, az));
  nx = __dadd_rn(nx, __dmul_rn(ax, ia));
  ny = __dadd_rn(ny, __dmul_rn(ay, ia));
  nz = __dadd_rn(nz, __dmul_rn(az, ia));
}

// dist = cv::norm(Pos - pRefKF->GetCameraCenter()) (:480-481)
__device__ __forceinline__ double ref_dist(double X, double Y, double Z, const double* R) {
  return norm3(__dsub_rn(X, R[0]), __dsub_rn(Y, R[1]), __dsub_rn(Z, R[2]));
}

// mfMinDistance / mfMaxDistance (:486-493); level must lie inside [0, nlev)
__device__ __forceinline__ void dist_range(double dist, const double* scale, int nlev, int level,
                                           double& dmin, double& dmax) {
  const double sf = scale[level];
  dmin = __ddiv_rn(__dmul_rn(__ddiv_rn(1.0, sf), dist), sf);
  dmax = __dmul_rn(__dmul_rn(sf, dist), scale[nlev - 1 - level]);
}

// mNormalVector = normal / n (:494)
__device__ __forceinline__ void mean_dir(double nx, double ny, double nz, int cnt, double* out) {
  const double in = __ddiv_rn(1.0, (double)cnt);
  out[0] = __dmul_rn(nx, in);
  out[1] = __dmul_rn(ny, in);
  out[2] = __dmul_rn(nz, in);
}

}  // namespace mpt
}  // namespace mcs
