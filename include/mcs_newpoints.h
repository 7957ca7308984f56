/*
 * mcs_newpoints.h -- C-ABI boundary for local mapping's CreateNewMapPoints on the device.
 *
 * Replaces (billamiable/MultiCol-SLAM-Annotation):
 *   void cLocalMapping::CreateNewMapPoints()        src/cLocalMapping.cpp:224-386
 *     the neighbour loop                            :241-384
 *     the per-match loop                            :272-382
 *   cv::Vec3d triangulate_point(t12, R12, v1, v2)   src/misc.cpp:26-51
 *   cMultiCamSys_::WorldToCamHom_fast               src/cam_system_omni.cpp:92-112
 *   the order of vMatchedPairs                      src/cORBmatcher.cpp:1140-1152
 *   cMapPoint::ComputeDistinctiveDescriptors        src/cMapPoint.cpp:297-390 (N = 2: BestIdx = 0, :367-383)
 *   cMapPoint::UpdateNormalAndDepth                 src/cMapPoint.cpp:453-496
 *
 * Keyframes are the resident form mcs_fuse_targets (include/mcs_matcher.h); of it off, kp_xy,
 * kp_octave, kp_cam, desc, mask, rays, m_t, m_c, cam and scale are read.  Everything is FP64 in
 * the text's operation order; device entries are asynchronous on `stream`.
 */
#ifndef MCS_NEWPOINTS_H
#define MCS_NEWPOINTS_H

#include <stdint.h>
#include "mcs_common.h"
#include "mcs_matcher.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Verdict of one KF1 keypoint (:272-364), in the order the text tests:
 * 0 no match (also: a match index outside [0, n2) or a camera outside [0, n_cams)),
 * 1 created, 2 parallax (:305), 3 behind / at camera 1 (:326-328), 4 reprojection 1 (:332),
 * 5 behind / at camera 2 (:340-342), 6 reprojection 2 (:346), 7 distance (:362-364). */
#define MCS_NP_NONE 0
#define MCS_NP_CREATED 1
#define MCS_NP_PARALLAX 2
#define MCS_NP_BEHIND1 3
#define MCS_NP_REPROJ1 4
#define MCS_NP_BEHIND2 5
#define MCS_NP_REPROJ2 6
#define MCS_NP_DISTANCE 7

/* The map points CreateNewMapPoints makes (:365-380), in creation order: neighbour by neighbour
 * and inside a neighbour in idx1 order (the order of vMatchedPairs, src/cORBmatcher.cpp:1140-1152). */
typedef struct mcs_new_points {      /* device buffers, capacity cap; appended across neighbours */
  int32_t cap;
  int32_t* count;                     /* [1]; keeps counting past cap, writes are clamped */
  int32_t *kp1, *kp2, *neighbour;     /* [cap] idx1 in KF1, idx2 in the neighbour, the neighbour number */
  double *pos, *normal;               /* [cap][3] x3D (:313-317), mNormalVector (src/cMapPoint.cpp:494) */
  double *min_dist, *max_dist;        /* [cap] mfMinDistance, mfMaxDistance (src/cMapPoint.cpp:492-493) */
  uint8_t *desc, *mask;               /* [cap][bytes]; mask nullable iff the keyframes have none */
} mcs_new_points;

/* Device scratch of the entries below for a KF1 of <= max_n1 keypoints: verdicts, the triangulated
 * points, the block totals of the ordered compaction, a match list when the caller keeps none. */
typedef struct mcs_newpts_workspace mcs_newpts_workspace;
int mcs_newpts_workspace_create(int32_t device, int32_t max_n1, mcs_newpts_workspace** out);
void mcs_newpts_workspace_destroy(mcs_newpts_workspace* ws);

/* The per-match loop (:272-382) for ONE neighbour, the step after
 * mcs_search_for_triangulation_raw_device: KF1 = target i1 of kfs, KF2 = target i2.
 *   n1            keypoints of KF1 (sizes the launch; also clamped to the set's own count)
 *   neighbour     the number written to out->neighbour
 *   d_matches12   [n1] the matcher's output (-1 = none)
 *   kf2_first     nonzero = KF2 precedes KF1 in the std::map<cMultiKeyFrame*, ...> of the new point
 *                 (pointer order): ComputeDistinctiveDescriptors then copies KF2's descriptor row
 *                 (and mask), else KF1's (src/cMapPoint.cpp:317-333, :367-389 with N = 2)
 *   d_has_mp1/2   [n1] / [n2] set to 1 at every created pair (AddMapPoint on both, :370-371)
 *   d_verdict     [n1] nullable
 * Per match, exactly as written: Tcw = Get_MtMc (camera -> world), rayRot = Rcw * ray, the
 * parallax gate `cosParallax < 0 || cosParallax > cos(3 pi / 180)` (a NaN passes), relOri =
 * Tcw1inv * Tcw2 with camIdx1 and camIdx2 read separately, triangulate_point in camera 1's frame
 * (the 2 x 2 inverse as d = 1 / det, adjugate * d; zero when det == 0), x3D4 = Tcw1 * x3D4, the two
 * WorldToCamHom_fast gates (z <= 0 rejects; cv::sqrt(ex^2 + ey^2) > 4.0 against the float keypoint
 * widened to double, at every octave), `dist == 0 || dist > 25.0` for either camera centre
 * (GetCameraCenter = the translation of M_t).  sigmaSquare*, ratio1, Rwc* and tcw* of the text are
 * never read and not computed.  Survivors are appended at *out->count in idx1 order; normal and
 * distances are UpdateNormalAndDepth for the observations {KF1, KF2} with reference keyframe KF1
 * and level kp_octave1[idx1] (clamped to the pyramid).
 * Two launches, stream-ordered, no host synchronisation, no allocation.  Offsets, counts, match
 * indices, cameras and octaves are device data and are clamped or rejected in the kernel: a
 * malformed set reads nothing outside its buffers.
 * MCS_ERR_ARG (before any device use): more than 8 cameras, bytes not 16 / 32 / 64, a mask on one
 * side only (kfs->mask against out->mask), i1 == i2 or outside the set, n1 above the workspace,
 * cap < 0, a null buffer. */
int mcs_new_points_pair_device(mcs_newpts_workspace* ws, const mcs_fuse_targets* kfs, int32_t i1,
                               int32_t i2, int32_t n1, int32_t neighbour,
                               const int32_t* d_matches12, int32_t kf2_first, uint8_t* d_has_mp1,
                               uint8_t* d_has_mp2, uint8_t* d_verdict, const mcs_new_points* out,
                               void* stream);

/* The whole neighbour loop (:241-384).  kfs target 0 is the current keyframe, targets 1..T its
 * neighbours in visiting order (T = kfs->n_targets - 1).
 *   h_n_kp [T + 1]        the keypoint counts, on the host (the matcher takes n1 and n2 as
 *                         arguments); their sum must be kfs->n_kp_total
 *   h_skip [T]            nonzero = the caller's `ratioBaselineDepth < 0.01` gate (:248-256).  It can
 *                         be evaluated for all neighbours up front: a point created with neighbour i
 *                         is observed by KF1 and neighbour i only, so it cannot change another
 *                         neighbour's median depth
 *   h_kf2_first [T]       kf2_first per neighbour
 *   d_E [T][C][C][9]      mcs_compute_e_rig(KF1, neighbour i) per neighbour
 *   d_has_mp [n_kp_total] packed like the keyframes; read and written in place
 *   th_low, epi_thresh    as mcs_search_for_triangulation_raw_device
 *   d_matches12 / d_verdict [T][n1] nullable, for inspection (-1 / 0 rows for a skipped neighbour)
 * For each neighbour not skipped: matcher -> pair kernels on the one stream, so neighbour i + 1 is
 * searched with the flags neighbour i set.  out->count is zeroed first.  No host synchronisation
 * and no allocation.  MCS_ERR_ARG as the pair entry, also for n_targets < 1 and counts that do not
 * add up; the matcher's own limits (n2 < 2^19, its workspace) are reported by the matcher. */
int mcs_create_new_map_points_device(mcs_newpts_workspace* ws, mcs_tri_workspace* tri,
                                     const mcs_fuse_targets* kfs, const int32_t* h_n_kp,
                                     const uint8_t* h_skip, const uint8_t* h_kf2_first,
                                     const double* d_E, uint8_t* d_has_mp, int32_t th_low,
                                     double epi_thresh, int32_t* d_matches12, uint8_t* d_verdict,
                                     const mcs_new_points* out, void* stream);

/* Host-buffer form for the reference's call site (src/cLocalMapping.cpp:99): every pointer inside
 * kfs and out and every other pointer is a host pointer; the counts are taken from kfs->off.
 * Uploads, runs the device entry on `device` and downloads (has_mp is updated in place).
 * *out->count is the number created; MCS_ERR_CAPACITY when it exceeds out->cap (the first cap
 * points are returned).  All argument errors (also malformed offsets, a keyframe of 2^19 keypoints
 * or more, a kp_cam outside [0, n_cams) and a device ordinal outside range) are returned before any
 * device use; MCS_ERR_NO_DEVICE without a GPU. */
int mcs_create_new_map_points(int32_t device, const mcs_fuse_targets* kfs, const uint8_t* skip,
                              const uint8_t* kf2_first, const double* E, uint8_t* has_mp,
                              int32_t th_low, double epi_thresh, int32_t* matches12,
                              uint8_t* verdict, const mcs_new_points* out);

#ifdef __cplusplus
}
#endif
#endif /* MCS_NEWPOINTS_H */
