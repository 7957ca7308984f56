// Device functions shared by frame.hip, window.hip, track_match.hip, hamming.hip, fuse.hip,
// sim3_match.hip and sim3_solver.hip: the
// omni projection (cayley2rot, M_t M_c, invMat, WorldToCamHom_fast / WorldToImg, ImgToWorld,
// isPointInMirrorMask), the predicted pyramid level, the window
// cell range of GetFeaturesInArea, the descriptor distance of a window candidate, the
// wave-per-query candidate and best-candidate walks and CheckDistEpipolarLine.  One definition
// each, so every entry that uses them gives the same bits.
// Translation units that include this are compiled with -ffp-contract=off; double ops are spelled
// with _rn intrinsics where an FMA could otherwise be formed.
#pragma once
#include "common.hpp"
#include "atan_cr.hpp"
#include "../../include/mcs_extractor.h"
#include "../../include/mcs_matcher.h"

namespace mcs {
namespace frm {

constexpr int kGridCols = 64, kGridRows = 48;   // FRAME_GRID_COLS / ROWS (include/cMultiFrame.h:47-48)

__device__ __forceinline__ double horner_n(const double* c, int s, double x) {   // misc.h:117-124
  double r = 0.0;
  for (int i = s - 1; i >= 0; i--) r = __dadd_rn(__dmul_rn(r, x), c[i]);
  return r;
}

// ImgToWorld (cam_model_omni.cpp:49-67)
__device__ inline void img_to_world(const mcs_cam_model& m, double u, double v, double* X) {
  const double invAffine = __dsub_rn(m.c, __dmul_rn(m.d, m.e));
  const double u_t = __dsub_rn(u, m.u0), v_t = __dsub_rn(v, m.v0);
  double x = __ddiv_rn(__dsub_rn(u_t, __dmul_rn(m.d, v_t)), invAffine);
  double y = __ddiv_rn(__dadd_rn(__dmul_rn(-m.e, u_t), __dmul_rn(m.c, v_t)), invAffine);
  const double X2 = __dmul_rn(x, x), Y2 = __dmul_rn(y, y);
  double z = -horner_n(m.p, m.p_deg, __dsqrt_rn(__dadd_rn(X2, Y2)));
  const double norm = __dsqrt_rn(__dadd_rn(__dadd_rn(X2, Y2), __dmul_rn(z, z)));
  X[0] = __ddiv_rn(x, norm); X[1] = __ddiv_rn(y, norm); X[2] = __ddiv_rn(z, norm);
}

// cayley2rot (misc.h:134-162): R = (1 / scale) * R
__device__ inline void cay2rot(const double* c, double* R) {
  const double c1 = c[0], c2 = c[1], c3 = c[2];
  const double c1s = __dmul_rn(c1, c1), c2s = __dmul_rn(c2, c2), c3s = __dmul_rn(c3, c3);
  const double scale = __dadd_rn(__dadd_rn(__dadd_rn(1.0, c1s), c2s), c3s);
  const double inv = __ddiv_rn(1.0, scale);
  R[0] = __dmul_rn(inv, __dsub_rn(__dsub_rn(__dadd_rn(1.0, c1s), c2s), c3s));
  R[1] = __dmul_rn(inv, __dmul_rn(2.0, __dsub_rn(__dmul_rn(c1, c2), c3)));
  R[2] = __dmul_rn(inv, __dmul_rn(2.0, __dadd_rn(__dmul_rn(c1, c3), c2)));
  R[3] = __dmul_rn(inv, __dmul_rn(2.0, __dadd_rn(__dmul_rn(c1, c2), c3)));
  R[4] = __dmul_rn(inv, __dsub_rn(__dadd_rn(__dsub_rn(1.0, c1s), c2s), c3s));
  R[5] = __dmul_rn(inv, __dmul_rn(2.0, __dsub_rn(__dmul_rn(c2, c3), c1)));
  R[6] = __dmul_rn(inv, __dmul_rn(2.0, __dsub_rn(__dmul_rn(c1, c3), c2)));
  R[7] = __dmul_rn(inv, __dmul_rn(2.0, __dadd_rn(__dmul_rn(c2, c3), c1)));
  R[8] = __dmul_rn(inv, __dadd_rn(__dsub_rn(__dsub_rn(1.0, c1s), c2s), c3s));
}

// M = M_t * M_c as 4x4 products (Matx sum over k = 0..3 left to right): R [9], t [3]
__device__ inline void mtmc(const double* pose, const double* mc, double* R, double* t) {
  double Rt[9], Rc[9];
  cay2rot(pose, Rt);
  cay2rot(mc, Rc);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      double s = __dmul_rn(Rt[3 * i], Rc[j]);
      s = __dadd_rn(s, __dmul_rn(Rt[3 * i + 1], Rc[3 + j]));
      s = __dadd_rn(s, __dmul_rn(Rt[3 * i + 2], Rc[6 + j]));
      s = __dadd_rn(s, __dmul_rn(pose[3 + i], 0.0));
      R[3 * i + j] = s;
    }
    double s = __dmul_rn(Rt[3 * i], mc[3]);
    s = __dadd_rn(s, __dmul_rn(Rt[3 * i + 1], mc[4]));
    s = __dadd_rn(s, __dmul_rn(Rt[3 * i + 2], mc[5]));
    s = __dadd_rn(s, __dmul_rn(pose[3 + i], 1.0));
    t[i] = s;
  }
}

// the same product from the 4x4 matrices themselves (16 doubles row-major, what Get_M_t and
// M_c hold): rows 0..2 of M_t * M_c, cv::Matx order s = 0; s += a(i,k) b(k,j), k = 0..3
__device__ inline void mtmc44(const double* Mt, const double* Mc, double* R, double* t) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s = __dadd_rn(s, __dmul_rn(Mt[4 * i + k], Mc[4 * k + j]));
      if (j < 3) R[3 * i + j] = s; else t[i] = s;
    }
}

// WorldToImg (cam_model_omni.cpp:147-163); cam = c d e u0 v0 invP[12].  CR: theta from the
// correctly rounded atan_cr (the host libm's result wherever the libm rounds correctly)
// instead of the device library's atan, for entries whose projection is held to the
// reference's bits; the default keeps every existing entry's bits.
template <bool CR = false>
__device__ __forceinline__ void world_to_img(const double* cam, double x, double y, double z,
                                             double& u, double& v) {
  double norm = __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
  if (norm == 0.0) norm = 1e-14;
  const double theta = CR ? atan_cr(__ddiv_rn(-z, norm)) : atan(__ddiv_rn(-z, norm));
  const double rho = horner_n(cam + 5, 12, theta);
  const double uu = __dmul_rn(__ddiv_rn(x, norm), rho), vv = __dmul_rn(__ddiv_rn(y, norm), rho);
  u = __dadd_rn(__dadd_rn(__dmul_rn(uu, cam[0]), __dmul_rn(vv, cam[1])), cam[3]);
  v = __dadd_rn(__dadd_rn(__dmul_rn(uu, cam[2]), vv), cam[4]);
}

// WorldToCamHom_fast (cam_system_omni.cpp:92-112): invMat(M_t M_c) * [X 1], then WorldToImg
template <bool CR = false>
__device__ inline void world_to_cam_img(const double* R, const double* t, const double* cam,
                                        const double* X, double& u, double& v) {
  double ti[3];   // invMat: R' = R^T, t' = -R' t (cConverter.cpp:31-44)
  for (int i = 0; i < 3; i++) {
    double s = __dmul_rn(-R[i], t[0]);
    s = __dadd_rn(s, __dmul_rn(-R[3 + i], t[1]));
    s = __dadd_rn(s, __dmul_rn(-R[6 + i], t[2]));
    ti[i] = s;
  }
  double Xc[3];
  for (int i = 0; i < 3; i++) {
    double s = __dmul_rn(R[i], X[0]);
    s = __dadd_rn(s, __dmul_rn(R[3 + i], X[1]));
    s = __dadd_rn(s, __dmul_rn(R[6 + i], X[2]));
    s = __dadd_rn(s, __dmul_rn(ti[i], 1.0));
    Xc[i] = s;
  }
  world_to_img<CR>(cam, Xc[0], Xc[1], Xc[2], u, v);
}

// invMat (cConverter.cpp:31-44) of a row-major 4x4: R' = R^T, t' = -R' * t
__device__ __forceinline__ void inv_mat44(const double* M, double* R, double* t) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = M[4 * j + i];
  for (int i = 0; i < 3; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(-R[3 * i + k], M[4 * k + 3]));
    t[i] = s;
  }
}

// isPointInMirrorMask(u, v, 0) (cam_model_omni.cpp:165-180) on camera c's mask of
// mask [n_cams][mh][mw]: cvRound, bounds (> 0 and < size), mask > 0
__device__ __forceinline__ bool in_mirror_mask(const uint8_t* mask, int c, int mw, int mh, double u,
                                               double v) {
  const int ur = (int)rint(u), vr = (int)rint(v);
  return !(ur >= mw || ur <= 0 || vr >= mh || vr <= 0) &&
         mask[(int64_t)c * mw * mh + (int64_t)vr * mw + ur] != 0;
}

// nPredictedLevel = lower_bound(mvScaleFactors, dist / minDistance), capped at L - 1
__device__ __forceinline__ int predict_level(const double* scale, int L, double ratio) {
  int lv = 0;
  while (lv < L && scale[lv] < ratio) lv++;
  if (lv >= L) lv = L - 1;
  return lv;
}

}  // namespace frm

namespace win {

constexpr int kCols = MCS_GRID_COLS, kRows = MCS_GRID_ROWS;

// window cell range of GetFeaturesInArea (cMultiFrame.cpp:280-298, cMultiKeyFrame.cpp:711-729);
// gp = {min_x, min_y, grid_w_inv, grid_h_inv} of the camera; false = empty window
__device__ __forceinline__ bool cell_range(const double* gp, double x, double y, double r,
                                           int* x0, int* x1, int* y0, int* y1) {
  const double mnx = gp[0], mny = gp[1];
  const double wi = gp[2], hi = gp[3];
  int nx0 = (int)floor((x - mnx - r) * wi);
  nx0 = max(0, nx0);
  if (nx0 >= kCols) return false;
  int nx1 = (int)ceil((x - mnx + r) * wi);
  nx1 = min(kCols - 1, nx1);
  if (nx1 < 0) return false;
  int ny0 = (int)floor((y - mny - r) * hi);
  ny0 = max(0, ny0);
  if (ny0 >= kRows) return false;
  int ny1 = (int)ceil((y - mny + r) * hi);
  ny1 = min(kRows - 1, ny1);
  if (ny1 < 0) return false;
  *x0 = nx0; *x1 = nx1; *y0 = ny0; *y1 = ny1;
  return true;
}

// DescriptorDistance64 / ...Masked over 32-bit words (the masked total is halved once, as
// the reference does over its 64-bit words)
__device__ __forceinline__ int ham(const uint8_t* q, const uint8_t* t, const uint8_t* mq,
                                  const uint8_t* mt, int bytes) {
  const uint32_t* a = reinterpret_cast<const uint32_t*>(q);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(t);
  int d = 0;
  if (!mq) {
    for (int w = 0; w < bytes / 4; w++) d += __popc(a[w] ^ b[w]);
    return d;
  }
  const uint32_t* ma = reinterpret_cast<const uint32_t*>(mq);
  const uint32_t* mb = reinterpret_cast<const uint32_t*>(mt);
  for (int w = 0; w < bytes / 4; w++) {
    const uint32_t x = a[w] ^ b[w];
    d += __popc(x & ma[w]) + __popc(x & mb[w]);
  }
  return d / 2;
}

// One frame's keypoints and feature grid as the candidate walk reads them.
struct CandFrame {
  const int32_t* cell_ptr; const int32_t* cell_kp; const double* gp; int n_cams;
  const float* kp_xy; const int32_t* kp_oct; const uint8_t* kp_desc; const uint8_t* kp_mask;
  int bytes;
};

// GetFeaturesInArea + the distance of every candidate, one wave per query (k_window and
// k_track_window).  The window's cells are taken 64 at a time, one per lane in the
// reference's loop order (ix outer, iy inner); a wave prefix sum over the cell sizes flattens
// their keypoints (insertion order within a cell), so a step costs two dependent loads for 64
// cells instead of a chain per cell.  Candidates passing the level and |dx|, |dy| <= r tests
// are compacted by ballot rank, which keeps the reference's order.  Returns the count.
// COUNT: count only; else write (keypoint, distance) from `base`.  CLAMP: the grid is device
// data nobody checked: cell ranges and entries are clamped to n_kp (as walk_best does) and
// nothing is written at or past `end`.
template <bool COUNT, bool CLAMP>
__device__ __forceinline__ int window_candidates(const CandFrame& a, int lane, double x, double y,
                                                 double r, int cam, int minL, int maxL,
                                                 const uint8_t* qd, const uint8_t* qm, int n_kp,
                                                 int base, int end, int32_t* cand_kp,
                                                 int32_t* cand_dist) {
  int cnt = 0;
  int x0, x1, y0, y1;
  if (cam >= 0 && cam < a.n_cams && cell_range(a.gp + 4 * cam, x, y, r, &x0, &x1, &y0, &y1)) {
    const bool check = !(minL == -1 && maxL == -1);
    const bool same = check && (minL == maxL);
    const int ncy = y1 - y0 + 1, ncell = (x1 - x0 + 1) * ncy;
    for (int cb = 0; cb < ncell; cb += 64) {
      const int ci = cb + lane;
      int start = 0, len = 0;
      if (ci < ncell) {
        const int cell = (cam * kCols + x0 + ci / ncy) * kRows + y0 + ci % ncy;
        start = a.cell_ptr[cell];
        len = a.cell_ptr[cell + 1] - start;
        if (CLAMP) {
          start = min(max(start, 0), n_kp);
          len = min(max(len, 0), n_kp - start);
        }
      }
      const int incl = dev::wave_incl_scan(len);
      const int off = incl - len;
      const int tot = __shfl(incl, 63);
      for (int e0 = 0; e0 < tot; e0 += 64) {
        const int e = e0 + lane;
        // owning cell = the last lane whose offset is <= e (an empty cell shares its offset
        // with the next cell, lanes past the window hold tot)
        int o = 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
          if (__shfl(off, o + s) <= e) o += s;
        const int so = __shfl(start, o), oo = __shfl(off, o);
        bool ok = false;
        int k = 0;
        if (e < tot) {
          k = a.cell_kp[so + (e - oo)];
          ok = !CLAMP || (k >= 0 && k < n_kp);
          if (ok) {
            const int oc = a.kp_oct[k];
            if (check && !same) ok = !(oc < minL || oc > maxL);
            else if (same) ok = (oc == minL);
          }
          if (ok) {
            const double dx = (double)a.kp_xy[2 * k] - x, dy = (double)a.kp_xy[2 * k + 1] - y;
            ok = !(fabs(dx) > r || fabs(dy) > r);
          }
        }
        const uint64_t bal = __ballot(ok);
        if (!COUNT && ok) {
          const int pos = base + cnt + __popcll(bal & dev::lanemask_lt());
          if (!CLAMP || pos < end) {
            cand_kp[pos] = k;
            cand_dist[pos] = ham(qd, a.kp_desc + (int64_t)k * a.bytes, qm,
                                 a.kp_mask ? a.kp_mask + (int64_t)k * a.bytes : nullptr, a.bytes);
          }
        }
        cnt += __popcll(bal);
      }
    }
  }
  return cnt;
}

// The window walk of the wave-per-query searches (k_fuse, k_sim3_search), after cell_range said
// the window is not empty.  The whole wave calls it with wave-uniform arguments.  Cells are taken
// 64 at a time in ix-major order (GetFeaturesInArea's enumeration, cMultiKeyFrame.cpp:731-743), a
// wave prefix sum over the cell sizes flattens their keypoints.  A candidate passing
// |dx| <= r && |dy| <= r and the level test (octave lv - 1 or lv) gets the key
// dist << kPosBits | position-in-enumeration; the wave minimum is the reference's first minimum
// under strict <.  o = the keyframe's first keypoint in the packed arrays, n_t = its (clamped)
// count, cptr = its cell_ptr row, ckp = its cell_kp list; cell ranges and entries are clamped to
// n_t.  use_dist = 0: every candidate counts as distance 0.  false = no candidate passed.
constexpr int kPosBits = 20;       // key = dist << 20 | position in the window's enumeration

__device__ __forceinline__ bool walk_best(int lane, int c, int x0, int x1, int y0, int y1,
                                          const int32_t* cptr, const int32_t* ckp, int64_t o, int n_t,
                                          const float* kp_xy, const int32_t* kp_oct,
                                          const uint8_t* desc, const uint8_t* mask, int bytes,
                                          const uint8_t* qd, const uint8_t* qm, double u, double v,
                                          double r, int lv, int use_dist, int* out_dist, int* out_k) {
  uint32_t best = 0xFFFFFFFFu;
  int bestk = -1, pos = 0;
  const int ncy = y1 - y0 + 1, ncell = (x1 - x0 + 1) * ncy;
  for (int cb = 0; cb < ncell; cb += 64) {
    const int ci = cb + lane;
    int start = 0, len = 0;
    if (ci < ncell) {
      const int cell = (c * kCols + x0 + ci / ncy) * kRows + y0 + ci % ncy;
      start = min(max(cptr[cell], 0), n_t);
      len = min(max(cptr[cell + 1] - start, 0), n_t - start);
    }
    const int incl = dev::wave_incl_scan(len);
    const int off = incl - len;
    const int tot = __shfl(incl, 63);
    for (int e0 = 0; e0 < tot; e0 += 64) {
      const int e = e0 + lane;
      int ow = 0;   // owning cell = the last lane whose offset is <= e
#pragma unroll
      for (int s = 32; s > 0; s >>= 1)
        if (__shfl(off, ow + s) <= e) ow += s;
      const int so = __shfl(start, ow), oo = __shfl(off, ow);
      if (e < tot) {
        const int k = ckp[so + (e - oo)];
        if (k >= 0 && k < n_t) {
          const int64_t g = o + k;
          const int oc = kp_oct[g];
          const double dx = (double)kp_xy[2 * g] - u, dy = (double)kp_xy[2 * g + 1] - v;
          if (fabs(dx) <= r && fabs(dy) <= r && !(oc < lv - 1 || oc > lv)) {
            const int dist = use_dist ? ham(qd, desc + g * bytes, qm, mask ? mask + g * bytes : nullptr, bytes)
                                      : 0;
            const uint32_t key = ((uint32_t)dist << kPosBits) | ((uint32_t)(pos + e) & ((1u << kPosBits) - 1));
            if (key < best) { best = key; bestk = k; }
          }
        }
      }
    }
    pos += tot;
  }
  uint32_t mn = best;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, s, 64));
  if (mn == 0xFFFFFFFFu) return false;
  const int src = __ffsll((unsigned long long)__ballot(best == mn)) - 1;
  *out_k = __shfl(bestk, src);
  *out_dist = (int)(mn >> kPosBits);
  return true;
}

}  // namespace win

// CheckDistEpipolarLine (src/misc.cpp:54-70).  nom = (ray2^T E12) ray1 evaluated left to right
// as cv::Matx does; (ray2^T E12)_c = sum_r ray2_r E_rc is exactly Etx2_c, so nom = Etx2 . ray1.
// One definition for the host entry and the device searches (same operation order, no FMA
// contraction on either side: -ffp-contract=off), so both give the same verdict bit for bit.
__host__ __device__ __forceinline__ bool epi_check(const double* r1, const double* r2,
                                                   const double* Em, double thresh) {
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

}  // namespace mcs
