// Query generation of the tracking matchers on the device (track_match.hip): one
// GetFeaturesInArea call of the reference per query, written as k_track_window reads it.
//
// Reference: SearchByProjection(F, vpMapPoints, th) src/cORBmatcher.cpp:67-166 with
// RadiusByViewingCos; SearchByProjection(CurrentFrame, LastFrame, th) :1991-2123.  Rule 1
// projects with the functions k_in_frustum uses (mtmc, world_to_cam_img, in_mirror_mask of
// omni_geom.hpp) on the same frame description; its projection is the window's centre and is
// held to the reference's bits, so WorldToImg's angle comes from atan_cr (correctly rounded:
// equal to the host libm's atan except at the about 2.5 arguments in ten thousand the libm
// misrounds, one ulp apart there) where k_in_frustum keeps the device library's atan: the two
// can differ in the last place of a pixel coordinate.
#pragma once
#include "omni_geom.hpp"
#include "track_grid.hpp"

namespace mcs {
namespace trk {

__device__ __forceinline__ void put_query(double* q_xyr, int32_t* q_cl, int32_t* q_idx, int64_t q,
                                          double x, double y, double r, int cam, int minL, int maxL,
                                          int idx) {
  q_xyr[3 * q] = x; q_xyr[3 * q + 1] = y; q_xyr[3 * q + 2] = r;
  q_cl[3 * q] = cam; q_cl[3 * q + 1] = minL; q_cl[3 * q + 2] = maxL;
  q_idx[q] = idx;
}

// rule 0: query p * C + c from isInFrustum's outputs of (point p, camera c)
__global__ __launch_bounds__(256) void k_queries_mappoints(const uint8_t* __restrict__ in_view,
                                                           const double* __restrict__ proj,
                                                           const int32_t* __restrict__ level,
                                                           const double* __restrict__ view_cos,
                                                           const uint8_t* __restrict__ skip, int n,
                                                           int C, const double* __restrict__ scale,
                                                           int L, double th, double* __restrict__ q_xyr,
                                                           int32_t* __restrict__ q_cl,
                                                           int32_t* __restrict__ q_idx) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)n * C) return;
  const int p = (int)(q / C), c = (int)(q - (int64_t)p * C);
  bool live = !(skip && skip[p]) && in_view[q] != 0;   // isBad() / already seen, mbTrackInView[cam]
  const int lv = live ? level[q] : 0;
  if (lv < 0 || lv >= L) live = false;
  if (!live) { put_query(q_xyr, q_cl, q_idx, q, 0.0, 0.0, 0.0, -1, -1, -1, p); return; }
  double r = view_cos[q] > 0.998 ? 2.5 : 4.0;         // RadiusByViewingCos
  if (th != 1.0) r = r * th;                           // bFactor
  put_query(q_xyr, q_cl, q_idx, q, proj[2 * q], proj[2 * q + 1], r * scale[lv], c, lv - 1, lv, p);
}

// rule 1: query i from slot i of the last frame
__global__ __launch_bounds__(256) void k_queries_lastframe(const double* __restrict__ pose,
                                                           const double* __restrict__ mc,
                                                           const double* __restrict__ camv, int C,
                                                           const uint8_t* __restrict__ masks, int mw,
                                                           int mh, const double* __restrict__ pos,
                                                           const uint8_t* __restrict__ valid,
                                                           const int32_t* __restrict__ kp_cam,
                                                           const int32_t* __restrict__ kp_oct,
                                                           const int32_t* __restrict__ d_n, int cap,
                                                           const double* __restrict__ scale, int L,
                                                           double th, double* __restrict__ q_xyr,
                                                           int32_t* __restrict__ q_cl,
                                                           int32_t* __restrict__ q_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  bool live = i < clamped_count(d_n, cap) && valid[i] != 0;
  const int c = live ? kp_cam[i] : 0, oc = live ? kp_oct[i] : 0;
  if (c < 0 || c >= C || oc < 0 || oc >= L) live = false;
  double u = 0.0, v = 0.0;
  if (live) {
    double R[9], t[3];
    frm::mtmc(pose, mc + 6 * c, R, t);
    frm::world_to_cam_img<true>(R, t, camv + 17 * c, pos + 3 * (int64_t)i, u, v);
    live = frm::in_mirror_mask(masks, c, mw, mh, u, v);
  }
  if (!live) { put_query(q_xyr, q_cl, q_idx, i, 0.0, 0.0, 0.0, -1, -1, -1, i); return; }
  put_query(q_xyr, q_cl, q_idx, i, u, v, th * scale[oc], c, oc - 1, oc + 1, i);
}

}  // namespace trk
}  // namespace mcs
