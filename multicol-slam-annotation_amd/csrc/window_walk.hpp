// The window walks of the projection matchers (window.hip, track_match.hip, fuse.hip,
// sim3_match.hip), one definition each: the window cell range of GetFeaturesInArea, the
// descriptor distance of a window candidate, and the wave-per-query candidate and best-candidate
// walks.  The projection that gives a window its centre is frm:: of omni_geom.hpp.
#pragma once
#include "common.hpp"
#include "../../include/mcs_matcher.h"

namespace mcs {
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
}  // namespace mcs
