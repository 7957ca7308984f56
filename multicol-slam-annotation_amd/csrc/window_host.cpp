// The host halves of the windowed matching (C-ABI of include/mcs_matcher.h): the cMultiFrame
// feature grid and the reference's sequential best / second-best selection rules.  Plain C++: no
// device.  The device half is window.hip.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   grid build (part of the cMultiFrame ctor)            src/cMultiFrame.cpp:154-184
//   PosInGrid                                            src/cMultiFrame.cpp:342-353
//   SearchByProjection(F, MPs)       (rule 0)            src/cORBmatcher.cpp:67-166
//   SearchByProjection(Cur, Last)    (rule 1)            src/cORBmatcher.cpp:1991-2123
//   SearchForInitialization          (rule 2)            src/cORBmatcher.cpp:579-726
//   WindowSearch                     (rule 3)            src/cORBmatcher.cpp:326-473
#include "../../include/mcs_matcher.h"
#include <climits>
#include <cmath>
#include <vector>

namespace {
constexpr int kCols = MCS_GRID_COLS, kRows = MCS_GRID_ROWS;
inline int cv_round(double v) { return (int)std::lrint(v); }   // cvRound: round half to even
}  // namespace

extern "C" {

int mcs_frame_grid_build(const float* kp_xy, const int32_t* kp_cam, int32_t n_kp, int32_t n_cams,
                         const double* gp, int32_t* cell_ptr, int32_t* cell_kp,
                         int32_t* n_in_grid) {
  if (n_kp < 0 || n_cams < 1 || !gp || !cell_ptr || (n_kp > 0 && (!kp_xy || !kp_cam || !cell_kp)))
    return MCS_ERR_ARG;
  const int ncell = n_cams * kCols * kRows;
  std::vector<int32_t> cell(n_kp, -1), cnt(ncell + 1, 0);
  for (int i = 0; i < n_kp; i++) {
    const int c = kp_cam[i];
    if (c < 0 || c >= n_cams) continue;
    // PosInGrid: cvRound((kp.pt.x - mnMinX) * inv); float - int (mnMinX is an int) is a float
    const float fx = kp_xy[2 * i] - (float)gp[4 * c], fy = kp_xy[2 * i + 1] - (float)gp[4 * c + 1];
    const int px = cv_round((double)fx * gp[4 * c + 2]);
    const int py = cv_round((double)fy * gp[4 * c + 3]);
    if (px < 0 || px >= kCols || py < 0 || py >= kRows) continue;
    cell[i] = (c * kCols + px) * kRows + py;
    cnt[cell[i] + 1]++;
  }
  for (int k = 0; k < ncell; k++) cnt[k + 1] += cnt[k];
  for (int k = 0; k <= ncell; k++) cell_ptr[k] = cnt[k];
  for (int i = 0; i < n_kp; i++)     // keypoints in index order = push_back order (:180-181)
    if (cell[i] >= 0) cell_kp[cnt[cell[i]]++] = i;
  if (n_in_grid) *n_in_grid = cell_ptr[ncell];
  return MCS_OK;
}

int mcs_window_select(int32_t rule, int32_t nq, const int32_t* cand_ptr, const int32_t* cand_kp,
                      const int32_t* cand_dist, const int32_t* kp_octave, int32_t n_kp,
                      int32_t th, double nnratio, uint8_t* kp_assigned, int32_t* match,
                      int32_t* n_matches) {
  if (rule < 0 || rule > 3 || nq < 0 || n_kp < 0 || !cand_ptr || !match || !n_matches) return MCS_ERR_ARG;
  if (rule != 2 && n_kp > 0 && !kp_assigned) return MCS_ERR_ARG;
  if (rule == 0 && n_kp > 0 && !kp_octave) return MCS_ERR_ARG;
  if (nq > 0 && cand_ptr[nq] > 0 && (!cand_kp || !cand_dist)) return MCS_ERR_ARG;
  for (int q = 0; q < nq; q++) match[q] = -1;
  int nm = 0;
  if (rule == 2) {
    // SearchForInitialization (:596-690): a train keypoint keeps the closest query so far
    std::vector<int> matched_dist(n_kp, INT_MAX), m21(n_kp, -1);
    for (int q = 0; q < nq; q++) {
      int best = INT_MAX, best2 = INT_MAX, bi = -1;
      for (int c = cand_ptr[q]; c < cand_ptr[q + 1]; c++) {
        const int k = cand_kp[c], d = cand_dist[c];
        if (matched_dist[k] <= d) continue;
        if (d < best) { best2 = best; best = d; bi = k; }
        else if (d < best2) best2 = d;
      }
      if (best <= th && best < (double)best2 * nnratio) {
        if (m21[bi] >= 0) { match[m21[bi]] = -1; nm--; }
        match[q] = bi;
        m21[bi] = q;
        matched_dist[bi] = best;
        nm++;
      }
    }
    *n_matches = nm;
    return MCS_OK;
  }
  for (int q = 0; q < nq; q++) {
    int best = INT_MAX, best2 = INT_MAX, bi = -1, lvl = -1, lvl2 = -1;
    for (int c = cand_ptr[q]; c < cand_ptr[q + 1]; c++) {
      const int k = cand_kp[c], d = cand_dist[c];
      if (kp_assigned[k]) continue;
      if (d < best) {
        best2 = best; best = d;
        lvl2 = lvl; lvl = rule == 0 ? kp_octave[k] : 0;
        bi = k;
      } else if (d < best2) {
        lvl2 = rule == 0 ? kp_octave[k] : 0;
        best2 = d;
      }
    }
    bool accept;
    if (rule == 0) accept = best <= th && !(lvl == lvl2 && best > nnratio * best2);   // :154-157
    else if (rule == 1) accept = best <= th;                                          // :2078
    else accept = best <= best2 * nnratio && best <= th;                              // :416
    if (accept) {
      kp_assigned[bi] = 1;
      match[q] = bi;
      nm++;
    }
  }
  *n_matches = nm;
  return MCS_OK;
}

}  // extern "C"
