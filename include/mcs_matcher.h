/*
 * mcs_matcher.h -- C-ABI drop-in boundary for the binary-descriptor matcher.
 *
 * Replaces (billamiable/MultiCol-SLAM-Annotation):
 *   int DescriptorDistance64(const uint64_t*, const uint64_t*, const int& dim)
 *                                                include/cORBmatcher.h:43-45, src/cORBmatcher.cpp:2443-2455
 *   int DescriptorDistance64Masked(...)          include/cORBmatcher.h:48-52, src/cORBmatcher.cpp:2457-2477
 *   the O(N1*N2) Hamming loop + selection of cORBmatcher::SearchForTriangulationRaw
 *                                                include/cORBmatcher.h:111-117, src/cORBmatcher.cpp:968-1156
 *   the best / second-best Hamming scans of the windowed matchers (SearchByProjection
 *   src/cORBmatcher.cpp:67-163, WindowSearch :326-475) -> mcs_hamming_top2_*.
 *   both SearchByBoW overloads (src/cORBmatcher.cpp:179-323 relocalisation, :885-966 loop
 *   detection), one frame against a batch of candidates -> mcs_search_by_bow*.
 *   the three Fuse overloads (src/cORBmatcher.cpp:1265-1418, :1420-1567, :1570-1719), one set of
 *   map points against a batch of target keyframes -> mcs_fuse*, mcs_fuse_select.
 *
 * `dim` / `bytes` is the descriptor length in BYTES (the reference passes featDim = 32
 * and loops dim/8 uint64 words).  Device entry points are asynchronous on `stream`.
 */
#ifndef MCS_MATCHER_H
#define MCS_MATCHER_H

#include <stdint.h>
#include "mcs_common.h"
#include "mcs_extractor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exact reference semantics; returns the distance (not a status). */
int mcs_descriptor_distance64(const uint64_t* d1, const uint64_t* d2, int32_t dim);
int mcs_descriptor_distance64_masked(const uint64_t* d1, const uint64_t* d2, const uint64_t* m1,
                                     const uint64_t* m2, int32_t dim);

/* Dense distances D[i*nb + j] = Hamming(A_i, B_j) (uint16), device buffers. */
int mcs_hamming_dense_device(const uint8_t* d_a, int32_t na, const uint8_t* d_b, int32_t nb,
                             int32_t bytes, uint16_t* d_dist, void* stream);

/* For each query i: best = min distance over all train rows (ties -> lowest train index),
 * second = second smallest distance counting multiplicity (ORB-SLAM bestDist/bestDist2
 * update rule), second_idx its train index.  nt == 0 -> best_idx = -1, dists = 256*8+1. */
int mcs_hamming_top2_device(const uint8_t* d_q, int32_t nq, const uint8_t* d_t, int32_t nt,
                            int32_t bytes, int32_t* d_best_idx, int32_t* d_best_dist,
                            int32_t* d_second_idx, int32_t* d_second_dist, void* stream);

/* Batched top-2 straight on the extractor's batch output: descriptor sets are
 * d_desc[set][cap][bytes] with d_counts[set] valid rows; pair p matches set
 * d_pairs[2p] (queries) against set d_pairs[2p+1] (train).  Outputs [n_pairs][cap]. */
int mcs_hamming_top2_batch_device(const uint8_t* d_desc, const int32_t* d_counts,
                                  const int32_t* d_pairs, int32_t n_pairs, int32_t cap,
                                  int32_t bytes, int32_t* d_best_idx, int32_t* d_best_dist,
                                  int32_t* d_second_idx, int32_t* d_second_dist, void* stream);

/* SearchForTriangulationRaw, match-list part (src/cORBmatcher.cpp:968-1156, with
 * mbCheckOrientation = false as constructed by the reference, include/cORBmatcher.h:40):
 * for each unmatched keypoint of KF1 (in index order), brute-force over unmatched
 * keypoints of KF2 of the SAME camera, keep dist <= th_low, visit candidates in
 * (dist, idx2) order up to cvRound(2*best), accept the first passing
 * CheckDistEpipolarLine(ray1, ray2, E[cam1][cam2], epi_thresh) (src/misc.cpp:54-70).
 * Host buffers: desc1 n1 x bytes, cam1 n1, has_mp1 n1 (nonzero = already has a map point),
 * rays1 n1 x 3 doubles; same for KF2; E = ncams*ncams 3x3 row-major doubles (E[c1][c2]).
 * Output matches12[n1] (-1 = none); *n_matches.  Distances are computed on the GPU. */
int mcs_search_for_triangulation_raw(const uint8_t* desc1, const int32_t* cam1,
                                     const uint8_t* has_mp1, const double* rays1, int32_t n1,
                                     const uint8_t* desc2, const int32_t* cam2,
                                     const uint8_t* has_mp2, const double* rays2, int32_t n2,
                                     int32_t ncams, const double* E, int32_t bytes,
                                     int32_t th_low, double epi_thresh, int32_t* matches12,
                                     int32_t* n_matches);

/* Same with mdBRIEF descriptor masks (cORBmatcher built with havingMasks = true, whose
 * TH_LOW is floor(featDim), src/cORBmatcher.cpp:52-65): distances are
 * DescriptorDistance64Masked(d1, d2, m1, m2) (src/cORBmatcher.cpp:1052-1056, 2457-2477).
 * mask1 [n1][bytes], mask2 [n2][bytes] host, both required.  Both entries reject
 * n2 >= 2^19 and cameras outside [0, ncams) with MCS_ERR_ARG (the device search keeps a
 * vbMatched2 bitmap of KF2 in LDS). */
int mcs_search_for_triangulation_raw_masked(const uint8_t* desc1, const uint8_t* mask1,
                                            const int32_t* cam1, const uint8_t* has_mp1,
                                            const double* rays1, int32_t n1,
                                            const uint8_t* desc2, const uint8_t* mask2,
                                            const int32_t* cam2, const uint8_t* has_mp2,
                                            const double* rays2, int32_t n2, int32_t ncams,
                                            const double* E, int32_t bytes, int32_t th_low,
                                            double epi_thresh, int32_t* matches12,
                                            int32_t* n_matches);

/* Device-resident SearchForTriangulationRaw for CreateNewMapPoints' neighbour loop
 * (src/cLocalMapping.cpp:223-266 -> src/cORBmatcher.cpp:968-1156): the same match list as
 * the two host entries above, on device buffers and stream-ordered (no host synchronisation),
 * so a caller keeps KF descriptors, rays and has-map-point flags resident and runs one call per
 * neighbour keyframe, updating d_has_mp1 between calls as the reference's triangulation does
 * (mcs_create_new_map_points_device of mcs_newpoints.h runs that loop: search, triangulation and
 * the flag update per neighbour on one stream).
 * d_mask1 / d_mask2: both null (ORB, DescriptorDistance64) or both set (mdBRIEF, ...Masked).
 * d_E [ncams][ncams][9] (mcs_compute_e_rig).  Out: d_matches12[n1] (-1 = none), *d_n_matches.
 * Keypoints whose camera lies outside [0, ncams) never match (the host entries reject them).
 * The workspace holds per-query candidate slots; n1 <= max_n1, n2 <= max_n2 < 2^19, ncams <= 8. */
typedef struct mcs_tri_workspace mcs_tri_workspace;
int mcs_tri_workspace_create(int32_t device, int32_t max_n1, int32_t max_n2, mcs_tri_workspace** out);
void mcs_tri_workspace_destroy(mcs_tri_workspace* ws);
int mcs_search_for_triangulation_raw_device(mcs_tri_workspace* ws, const uint8_t* d_desc1,
                                            const uint8_t* d_mask1, const int32_t* d_cam1,
                                            const uint8_t* d_has_mp1, const double* d_rays1,
                                            int32_t n1, const uint8_t* d_desc2,
                                            const uint8_t* d_mask2, const int32_t* d_cam2,
                                            const uint8_t* d_has_mp2, const double* d_rays2,
                                            int32_t n2, int32_t ncams, const double* d_E,
                                            int32_t bytes, int32_t th_low, double epi_thresh,
                                            int32_t* d_matches12, int32_t* d_n_matches,
                                            void* stream);

/* The essential matrices SearchForTriangulationRaw precomputes per camera pair
 * (src/cORBmatcher.cpp:985-998): E[i][j] = ComputeE(KF1.Get_MtMc_inv(i), KF2.Get_MtMc(j))
 * (src/misc.cpp:72-86), the rig poses given as the Cayley 6-vectors the keyframes hold
 * (cMultiCamSys_::Set_M_t_from_min, src/cam_system_omni.cpp:170-183): mt1, mt2 [6],
 * mc [ncams][6].  Out: E [ncams][ncams][9] row-major, the `E` input of the two entries above.
 * Host math in the reference's cv::Matx operation order. */
int mcs_compute_e_rig(const double* mt1, const double* mt2, const double* mc, int32_t ncams,
                      double* E);

/* The same from the 4 x 4 matrices themselves, for callers that hold Get_M_t() and M_c (the
 * resident keyframe form mcs_fuse_targets): m_t1, m_t2 [16], m_c [ncams][16], row-major. */
int mcs_compute_e_rig_hom(const double* m_t1, const double* m_t2, const double* m_c, int32_t ncams,
                          double* E);

/* CheckDistEpipolarLine(ray1, ray2, E12, thresh) (src/misc.cpp:54-70): 1 = passes (squared
 * epipolar distance < thresh), 0 = fails (or den == 0), < 0 = argument error.  The check the
 * triangulation entries apply to every candidate. */
int mcs_check_dist_epipolar_line(const double* ray1, const double* ray2, const double* E12,
                                 double thresh);

/* ---- Projection-guided (windowed) matching -------------------------------------------
 * cMultiFrame feature grid (src/cMultiFrame.cpp:154-184, PosInGrid :342-353; 64 x 48 cells
 * per camera, include/cMultiFrame.h FRAME_GRID_COLS / FRAME_GRID_ROWS) and
 * GetFeaturesInArea (:272-340), feeding the best / second-best Hamming scans of
 *   SearchByProjection(F, vpMapPoints, th)          src/cORBmatcher.cpp:67-166   (rule 0)
 *   SearchByProjection(CurrentFrame, LastFrame, th) src/cORBmatcher.cpp:1991-2123 (rule 1)
 *   SearchForInitialization(F1, F2, ...)            src/cORBmatcher.cpp:579-726  (rule 2)
 *   WindowSearch(F1, F2, windowSize, ...)           src/cORBmatcher.cpp:326-473  (rule 3)
 * with checkOrientation = false (include/cORBmatcher.h:40).
 * Split: two forms over the same candidate walk (cells ix-major, then iy, then insertion
 * order; the Hamming distance of every candidate), which give the same bits.
 *   Host-split form (mcs_frame_grid_build, mcs_window_search_device, mcs_window_select,
 *   mcs_window_match): the grid is built on the host (it is part of the cMultiFrame
 *   constructor), the device enumerates the candidates, the host applies the reference's
 *   sequential selection rule (it depends on earlier queries' assignments).  Serves all four
 *   rules; the search synchronises once and the candidate lists are downloaded.
 *   Device form (mcs_track_*, mcs_frame_grid_build_device; rules 0, 1 and 3): grid, queries,
 *   candidates and the ordered selection all run stream-ordered on the device over a
 *   workspace, with no allocation, no synchronisation and no copy to the host; capacity
 *   overflow is reported in device memory (d_status).  Rule 2 un-matches earlier queries and
 *   runs once per session: it stays with the host-split form. */
#define MCS_GRID_COLS 64
#define MCS_GRID_ROWS 48

/* grid_params[cam] = {min_x, min_y, grid_w_inv, grid_h_inv} (mnMinX, mnMinY,
 * mfGridElementWidthInv, mfGridElementHeightInv).  kp_xy [n_kp][2] float (cv::KeyPoint.pt),
 * kp_cam [n_kp].  Out: cell_ptr [n_cams*64*48 + 1] (cell = (cam*64 + ix)*48 + iy), cell_kp
 * [n_kp] (keypoints outside the grid are dropped; *n_in_grid entries used).  Host memory. */
int mcs_frame_grid_build(const float* kp_xy, const int32_t* kp_cam, int32_t n_kp, int32_t n_cams,
                         const double* grid_params, int32_t* cell_ptr, int32_t* cell_kp,
                         int32_t* n_in_grid);

/* Device window search.  Queries: q_xyr [nq][3] doubles (x, y, r), q_cam_lvl [nq][3]
 * (cam, minLevel, maxLevel; -1/-1 = any level), q_desc [nq][bytes] (+ q_mask nullable).
 * Keypoints: kp_xy [n][2] float, kp_octave [n], kp_desc [n][bytes] (+ kp_mask nullable; with
 * masks the distance is DescriptorDistance64Masked).  Grid: device copies of the
 * mcs_frame_grid_build outputs and grid_params.  Out: cand_ptr [nq+1], cand_kp / cand_dist
 * [cap]; *total = number of candidates (MCS_ERR_CAPACITY if > cap; nothing else written).
 * Synchronises `stream` once to read the total. */
int mcs_window_search_device(const int32_t* d_cell_ptr, const int32_t* d_cell_kp,
                             const double* d_grid_params, int32_t n_cams, const float* d_kp_xy,
                             const int32_t* d_kp_octave, const uint8_t* d_kp_desc,
                             const uint8_t* d_kp_mask, int32_t bytes, int32_t nq,
                             const double* d_q_xyr, const int32_t* d_q_cam_lvl,
                             const uint8_t* d_q_desc, const uint8_t* d_q_mask,
                             int32_t* d_cand_ptr, int32_t* d_cand_kp, int32_t* d_cand_dist,
                             int64_t cap, int64_t* total, void* stream);

/* Host selection over the candidate lists (queries in the reference's loop order).
 * rule 0: SearchByProjection(F, MPs): skip assigned keypoints, best / second with octaves,
 *         accept best <= th unless (same octave and best > nnratio * second), assign.
 * rule 1: SearchByProjection(Current, Last): skip assigned keypoints, best only,
 *         accept best <= th, assign.
 * rule 2: SearchForInitialization: skip candidates whose vMatchedDistance <= dist, accept
 *         best <= th and best < second * nnratio, a re-matched train keypoint drops its
 *         previous query.
 * rule 3: WindowSearch: skip keypoints matched earlier in the call, accept
 *         best <= second * nnratio and best <= th, assign.
 * th = TH_HIGH (rules 0, 1, 3) or TH_LOW (rule 2) of cORBmatcher (src/cORBmatcher.cpp:46-65).
 * kp_assigned [n_kp] in/out (rules 0, 1, 3: keypoint already holds a map point).  match [nq]
 * out (keypoint index or -1; rule 2: vnMatches12).  *n_matches = match count. */
int mcs_window_select(int32_t rule, int32_t nq, const int32_t* cand_ptr, const int32_t* cand_kp,
                      const int32_t* cand_dist, const int32_t* kp_octave, int32_t n_kp,
                      int32_t th, double nnratio, uint8_t* kp_assigned, int32_t* match,
                      int32_t* n_matches);

/* Host-buffer entry point for the reference's call sites (cv::Mat / std::vector data): builds
 * the grid, uploads the frame and the queries, runs mcs_window_search_device and
 * mcs_window_select on `device` (no CPU fallback).  kp_assigned may be NULL (= none). */
typedef struct mcs_window_frame {
  int32_t n_cams, n_kp, bytes;
  const double* grid_params;     /* [n_cams][4], as above */
  const float* kp_xy;            /* [n_kp][2] mvKeys pt */
  const int32_t* kp_cam;         /* [n_kp] keypoint_to_cam */
  const int32_t* kp_octave;      /* [n_kp] */
  const uint8_t* desc;           /* [n_kp][bytes] mDescriptors in camera order */
  const uint8_t* desc_mask;      /* nullable [n_kp][bytes] mDescriptorMasks (mdBRIEF) */
} mcs_window_frame;
int mcs_window_match(int32_t device, int32_t rule, const mcs_window_frame* frame, int32_t nq,
                     const double* q_xyr, const int32_t* q_cam_lvl, const uint8_t* q_desc,
                     const uint8_t* q_mask, int32_t th, double nnratio, uint8_t* kp_assigned,
                     int32_t* match, int32_t* n_matches);

/* -- Device form: the windowed matchers of tracking with nothing downloaded ---------------
 *   TrackWithMotionModel -> SearchByProjection(Current, Last)      (rule 1)
 *   TrackLocalMap        -> isInFrustum + SearchByProjection(F, MPs) (rule 0)
 *   TrackPreviousFrame   -> WindowSearch                           (rule 3)
 * Every d_ pointer is device memory and every call is asynchronous on `stream`.  A workspace
 * serves one stream at a time. */
#define MCS_TRACK_MAX_CAMS 8
#define MCS_TRACK_OVERFLOW 1            /* d_status[1] bit 0: candidates exceeded cand_cap */
#define MCS_TRACK_ROUNDS(flags) ((int32_t)((uint64_t)(flags) >> 32))   /* settle rounds of the call */

/* Workspace of the device form: grid-build scratch, the candidate lists (cand_cap entries)
 * and the selection's marks and query lists, for frames of at most max_kp keypoint slots and
 * calls of at most max_queries queries. */
typedef struct mcs_track_workspace mcs_track_workspace;
int mcs_track_workspace_create(int32_t device, int32_t max_kp, int32_t max_queries,
                               int64_t cand_cap, mcs_track_workspace** out);
void mcs_track_workspace_destroy(mcs_track_workspace* ws);

/* mcs_frame_grid_build on the device, bit-identical for finite coordinates whose grid
 * position fits an int (beyond that the host's lrint and the device's saturating conversion
 * part): the same PosInGrid arithmetic (float subtraction, cvRound of the double product),
 * keypoints outside the grid or with a camera outside [0, n_cams) dropped, ascending keypoint
 * index within a cell.  d_kp_xy [cap][2],
 * d_kp_cam [cap]; d_n_kp = the keypoint count on the device (clamped to [0, cap]; slots past
 * it are not read), NULL = cap.  Out: d_cell_ptr [n_cams*64*48 + 1], d_cell_kp [cap],
 * d_n_in_grid (nullable).  cap <= the workspace's max_kp, n_cams <= MCS_TRACK_MAX_CAMS. */
int mcs_frame_grid_build_device(mcs_track_workspace* ws, const float* d_kp_xy,
                                const int32_t* d_kp_cam, const int32_t* d_n_kp, int32_t cap,
                                int32_t n_cams, const double* d_grid_params, int32_t* d_cell_ptr,
                                int32_t* d_cell_kp, int32_t* d_n_in_grid, void* stream);

/* mvKeys rows as mcs_multiframe_concat_device leaves them (d_keys [cap], d_n = its d_total
 * entry, NULL = cap) -> d_kp_xy [cap][2] (pt) and d_kp_octave [cap] (both nullable).  Its
 * d_kp_to_cam and d_total are taken by the entries here as they are; its d_grid_pos subtracts
 * in double, so the grid is built from the unpacked positions. */
int mcs_track_unpack_keys_device(const mcs_keypoint* d_keys, const int32_t* d_n, int32_t cap,
                                 float* d_kp_xy, int32_t* d_kp_octave, void* stream);

/* Queries of rule 0 from the outputs of mcs_is_in_frustum_device ([n_points][n_cams]), one per
 * (map point, camera) in that loop order: at (projX, projY), r = (viewCos > 0.998 ? 2.5 : 4.0),
 * r *= th if th != 1.0, then r * scale[level]; levels (level - 1, level); descriptor index =
 * the point.  d_skip [n_points] (nullable): the caller's snapshot of isBad() and of
 * mnLastFrameSeen == the current frame (src/cTracking.cpp:961-1017).  A skipped point, a
 * camera not in view or a level outside [0, n_levels) gives cam = -1 (an empty window).
 * Out: d_q_xyr [nq][3], d_q_cam_lvl [nq][3], d_q_desc_idx [nq], nq = n_points * n_cams. */
int mcs_track_queries_mappoints_device(const uint8_t* d_in_view, const double* d_proj,
                                       const int32_t* d_level, const double* d_view_cos,
                                       const uint8_t* d_skip, int32_t n_points, int32_t n_cams,
                                       const double* d_scale, int32_t n_levels, double th,
                                       double* d_q_xyr, int32_t* d_q_cam_lvl,
                                       int32_t* d_q_desc_idx, void* stream);

/* Queries of rule 1, one per keypoint slot of the last frame: d_pos [cap][3] the slot's map
 * point in the world, d_valid [cap] = has a point, not bad, not mvbOutlier; projected with the
 * current frame (pose, rig and level-0 mirror masks as mcs_is_in_frustum_device takes them)
 * into the slot's own camera d_kp_cam [cap], through isPointInMirrorMask; r = th *
 * scale[octave], levels (octave - 1, octave + 1); descriptor index = the slot.  d_n (nullable
 * = cap): the last frame's keypoint count.  Invalid slots, slots past the count, a camera or
 * octave out of range and projections outside the mask give cam = -1.  WorldToImg's angle is a
 * correctly rounded atan: the projection has the reference's bits wherever the host libm's
 * atan, which the reference calls, is correctly rounded too (all but about 2.5 arguments in
 * ten thousand, and then they are one ulp apart).  It can differ in the last place from
 * mcs_is_in_frustum_device's, which uses the device library's atan. */
int mcs_track_queries_lastframe_device(const double* d_pose, const double* d_mc,
                                       const double* d_cam, int32_t n_cams, const uint8_t* d_masks,
                                       int32_t mask_w, int32_t mask_h, const double* d_pos,
                                       const uint8_t* d_valid, const int32_t* d_kp_cam,
                                       const int32_t* d_kp_octave, const int32_t* d_n, int32_t cap,
                                       const double* d_scale, int32_t n_levels, double th,
                                       double* d_q_xyr, int32_t* d_q_cam_lvl,
                                       int32_t* d_q_desc_idx, void* stream);

/* The frame searched (device pointers in the device entry).  n_kp = keypoint slots; the grid
 * says which of them exist.  Grid counts and entries are clamped to n_kp when read. */
typedef struct mcs_track_frame {
  int32_t n_cams, n_kp, bytes;
  const double* grid_params;     /* [n_cams][4] */
  const int32_t* cell_ptr;       /* [n_cams*64*48 + 1] */
  const int32_t* cell_kp;        /* [n_kp] */
  const float* kp_xy;            /* [n_kp][2] */
  const int32_t* kp_octave;      /* [n_kp] */
  const uint8_t* desc;           /* [n_kp][bytes] */
  const uint8_t* desc_mask;      /* nullable [n_kp][bytes] */
} mcs_track_frame;

/* The queries: query q reads row q_desc_idx[q] (NULL = q) of q_desc_src [n_src][bytes] (+
 * q_mask_src, given exactly when the frame has masks); an index outside [0, n_src) is an
 * empty window, like cam = -1. */
typedef struct mcs_track_queries {
  int32_t nq, n_src;
  const double* q_xyr;           /* [nq][3] */
  const int32_t* q_cam_lvl;      /* [nq][3] */
  const int32_t* q_desc_idx;     /* nullable [nq] */
  const uint8_t* q_desc_src;     /* [n_src][bytes] */
  const uint8_t* q_mask_src;     /* nullable [n_src][bytes] */
} mcs_track_queries;

/* Count pass, scan, fill pass and the ordered selection of rule 0, 1 or 3 (rule 2:
 * MCS_ERR_UNSUPPORTED), bit-equal to mcs_window_select over the same candidates.
 * d_kp_assigned [n_kp] in/out; out: d_match [nq], d_kp_query [n_kp] (the query that took the
 * keypoint in this call, or -1: what writes mvpMapPoints[bestIdx] = pMP), d_n_matches,
 * d_status int64 [2] = {required candidate total, flags}.  When the total exceeds the
 * workspace's cand_cap: d_match / d_kp_query all -1, d_n_matches 0, d_kp_assigned untouched,
 * MCS_TRACK_OVERFLOW set; read the status when the results are read.
 * The selection runs rounds in one launch, one workgroup per camera (no query crosses
 * cameras): every unsettled query marks its unassigned candidates with an atomic (the lowest
 * query wins); a query holding all its marks has no earlier unsettled query on any of its
 * candidates, so it scans them in list order as the sequential loop would and settles; under
 * rules 1 and 3 a match also stands as soon as no earlier unsettled query lists its best
 * candidate (earlier queries only take keypoints away). */
int mcs_track_search_device(mcs_track_workspace* ws, int32_t rule, const mcs_track_frame* frame,
                            const mcs_track_queries* queries, int32_t th_high, double nnratio,
                            uint8_t* d_kp_assigned, int32_t* d_match, int32_t* d_kp_query,
                            int32_t* d_n_matches, int64_t* d_status, void* stream);

/* The selection alone over the candidate lists the workspace holds from its last search with
 * the same queries (d_q_cam_lvl [nq][3], d_kp_octave [n_kp]).  d_status: the total and the
 * overflow flag as the search left them; the rounds field is set to this call's. */
int mcs_track_select_device(mcs_track_workspace* ws, int32_t rule, int32_t nq,
                            const int32_t* d_q_cam_lvl, const int32_t* d_kp_octave, int32_t n_kp,
                            int32_t n_cams, int32_t th_high, double nnratio,
                            uint8_t* d_kp_assigned, int32_t* d_match, int32_t* d_kp_query,
                            int32_t* d_n_matches, int64_t* d_status, void* stream);

/* Host-buffer entries for the reference's call sites: upload, run the device form on `device`
 * and download (MCS_ERR_NO_DEVICE without a GPU, no CPU fallback).  mcs_track_search builds
 * the grid on the device and sizes the candidate lists itself; kp_assigned and kp_query may
 * be NULL.  The two query entries run the kernels above on host arrays. */
int mcs_track_search(int32_t device, int32_t rule, const mcs_window_frame* frame,
                     const mcs_track_queries* queries, int32_t th_high, double nnratio,
                     uint8_t* kp_assigned, int32_t* match, int32_t* kp_query, int32_t* n_matches);
int mcs_track_queries_mappoints(int32_t device, const uint8_t* in_view, const double* proj,
                                const int32_t* level, const double* view_cos, const uint8_t* skip,
                                int32_t n_points, int32_t n_cams, const double* scale,
                                int32_t n_levels, double th, double* q_xyr, int32_t* q_cam_lvl,
                                int32_t* q_desc_idx);
int mcs_track_queries_lastframe(int32_t device, const double* pose, const double* mc,
                                const double* cam, int32_t n_cams, const uint8_t* masks,
                                int32_t mask_w, int32_t mask_h, const double* pos,
                                const uint8_t* valid, const int32_t* kp_cam,
                                const int32_t* kp_octave, int32_t n, const double* scale,
                                int32_t n_levels, double th, double* q_xyr, int32_t* q_cam_lvl,
                                int32_t* q_desc_idx);

/* ---- SearchByBoW: relocalisation and loop detection -------------------------------------
 *   int SearchByBoW(cMultiKeyFrame* pKF, cMultiFrame& F, vpMapPointMatches)
 *                                          src/cORBmatcher.cpp:179-323  ("overload A"), called per
 *       candidate keyframe by cTracking::Relocalisation (src/cTracking.cpp:1191-1203)
 *   int SearchByBoW(cMultiKeyFrame* pKF1, cMultiKeyFrame* pKF2, vpMatches12)
 *                                          src/cORBmatcher.cpp:885-966  ("overload B"), called per
 *       loop candidate by cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:285-304)
 * Both call sites match ONE frame against a batch of candidates; one call here takes the batch.
 *
 * A set is n_frames frames packed back to back: frame k owns keypoints off[k] .. off[k+1] of
 * desc / mask / angle / has_mp, and its FeatureVector (the CSR form mcs_vocab_transform and
 * mcs_feature_vector_device emit, feature indices local to the frame) lies at fv_node + off[k],
 * fv_ptr + off[k] + k (n_kp + 1 entries), fv_feat + off[k], with fv_n[k] node entries.
 * n_kp_total = off[n_frames] is given on the host (it sizes launches); it must be < 2^19.
 * For the device entries every pointer is a device pointer, for the host entries a host pointer.
 *   mask    nullable: mdBRIEF masks (havingMasks, DescriptorDistance64Masked, :2457-2477);
 *           the two sets of one call have both masks or none
 *   angle   cv::KeyPoint::angle, read only with check_orientation
 *   has_mp  nonzero = the keypoint holds a map point that is not bad (:214-220, :903-907,
 *           :922-927); not read for the frame F of overload A (:185 starts from all-NULL)
 *   fv_*    not read by overload B (it uses no vocabulary, :901-963) */
typedef struct mcs_bow_set {
  int32_t n_frames, n_kp_total;
  const int32_t* off;        /* [n_frames + 1], off[0] = 0, non-decreasing */
  const uint8_t* desc;       /* [n_kp_total][bytes] */
  const uint8_t* mask;       /* nullable [n_kp_total][bytes] */
  const float* angle;        /* [n_kp_total] */
  const uint8_t* has_mp;     /* [n_kp_total] */
  const uint32_t* fv_node;   /* node ids, strictly ascending per frame */
  const int32_t* fv_ptr;     /* [n_kp_total + n_frames] */
  const uint32_t* fv_feat;   /* feature (keypoint) indices of each node, in feature order */
  const int32_t* fv_n;       /* [n_frames] */
} mcs_bow_set;

/* Workspace of the device entries below: frames of at most max_kp keypoints, batches of at
 * most max_candidates candidates (overload B keeps candidate slots per query and candidate). */
typedef struct mcs_bow_workspace mcs_bow_workspace;
int mcs_bow_workspace_create(int32_t device, int32_t max_kp, int32_t max_candidates,
                             mcs_bow_workspace** out);
void mcs_bow_workspace_destroy(mcs_bow_workspace* ws);

/* The FeatureVector of TemplatedVocabulary::transform(features, BowVector&, FeatureVector&,
 * levelsup) (TemplatedVocabulary.h:1126-1196) from the per-descriptor d_node / d_weight that
 * mcs_vocab_transform_words_device writes, without leaving the device: d_fv_node ascending
 * (capacity n), d_fv_ptr (capacity n + 1), d_fv_feat in feature order (capacity n), *d_fv_n.
 * Descriptors with weight <= 0 (stopped words) are dropped, as mcs_vocab_transform does.
 * Stream-ordered, no host synchronisation; n <= max_kp. */
int mcs_feature_vector_device(mcs_bow_workspace* ws, const uint32_t* d_node, const double* d_weight,
                              int32_t n, uint32_t* d_fv_node, int32_t* d_fv_ptr,
                              uint32_t* d_fv_feat, int32_t* d_fv_n, void* stream);

/* Overload A for frame f (a set of one frame) against the n_frames keyframes of kfs, one
 * launch for the batch.  Per keyframe: shared nodes in ascending id (:203-300), KF keypoints
 * of a node in list order, skipped without a good map point; candidates are the node's F
 * keypoints not yet assigned in this call; best with strict <, second-best counting
 * multiplicity (:252-261); accepted when best <= th_low and (double)best < nnratio *
 * (double)second (:264-266).  check_orientation: the 30-bin histogram of
 * cvRound((angleKF - angleF [+ 360]) * (1.0f / 30)) and ComputeThreeMaxima (:272-282,
 * :303-321, :2399-2441); matches outside the kept bins are removed after the walk.
 * th_low = TH_LOW_ of the cORBmatcher ctor (:46-65): 2 * bytes, or bytes with masks.
 * Out: d_match_f [n_kf][n_f] = index (local to the keyframe) of the KF keypoint whose map point
 * F's keypoint received, -1 for none; d_n_matches [n_kf] = the return value per keyframe.
 * Stream-ordered, no host synchronisation.  MCS_ERR_ARG: bytes not 16 / 32 / 64, one mask
 * without the other, f->n_frames != 1, sizes above the workspace or >= 2^19.  A FeatureVector
 * entry that points outside its frame is skipped by the kernel (the host entry rejects it). */
int mcs_search_by_bow_device(mcs_bow_workspace* ws, const mcs_bow_set* f, const mcs_bow_set* kfs,
                             int32_t bytes, int32_t th_low, double nnratio,
                             int32_t check_orientation, int32_t* d_match_f, int32_t* d_n_matches,
                             void* stream);

/* Host-buffer convenience for one or more candidates: checks the arguments (MCS_ERR_ARG also
 * for a FeatureVector whose nodes are not strictly ascending or whose ranges are malformed, and
 * for a feature index >= its frame's keypoint count), then uploads, runs the device entry on
 * `device` and downloads.  MCS_ERR_NO_DEVICE without a GPU (there is no CPU fallback). */
int mcs_search_by_bow(int32_t device, const mcs_bow_set* f, const mcs_bow_set* kfs, int32_t bytes,
                      int32_t th_low, double nnratio, int32_t check_orientation, int32_t* match_f,
                      int32_t* n_matches);

/* Overload B for keyframe kf1 (a set of one frame) against the n_frames candidates of kf2s:
 * KF1 keypoints with a good map point in index order, brute force over KF2 keypoints with a
 * good map point not yet taken (vbMatched2), the same best / second-best rule, accepted when
 * best < th_low (strict, :952) and the ratio test passes; no orientation check.
 * Out: d_matches12 [n_kf][n1] = KF2 keypoint index (vpMatches12[idx1] = vpMapPoints2[idx2]) or
 * -1; d_n_matches [n_kf].  Same error behaviour as overload A. */
int mcs_search_by_bow_kf_device(mcs_bow_workspace* ws, const mcs_bow_set* kf1,
                                const mcs_bow_set* kf2s, int32_t bytes, int32_t th_low,
                                double nnratio, int32_t* d_matches12, int32_t* d_n_matches,
                                void* stream);
int mcs_search_by_bow_kf(int32_t device, const mcs_bow_set* kf1, const mcs_bow_set* kf2s,
                         int32_t bytes, int32_t th_low, double nnratio, int32_t* matches12,
                         int32_t* n_matches);

/* ---- Fuse: map-point fusion of local mapping and loop closing ------------------------------
 *   int Fuse(cMultiKeyFrame* pKF, cMultiKeyFrame* curKF, vector<cMapPoint*>& vpMapPoints, th)
 *                                          src/cORBmatcher.cpp:1265-1418  (rule 0), called once per
 *       target keyframe by cLocalMapping::SearchInNeighbors (src/cLocalMapping.cpp:388-457)
 *   int Fuse(cMultiKeyFrame* pKF, vector<cMapPoint*>& vpMapPoints, th)
 *                                          src/cORBmatcher.cpp:1420-1567  (rule 1), called once with
 *       the union of the neighbours' map points (src/cLocalMapping.cpp:453)
 *   int Fuse(cMultiKeyFrame* pKF, cv::Matx44d Scw, const vector<cMapPoint*>& vpPoints, th)
 *                                          src/cORBmatcher.cpp:1570-1719  (rule 2), called per
 *       corrected keyframe by cLoopClosing::SearchAndFuse (src/cLoopClosing.cpp:670-690)
 * Split: per (target keyframe t, query map point i, camera c) the projection
 * (WorldToCamHom_fast, src/cam_system_omni.cpp:92-112), isPointInMirrorMask
 * (src/cam_model_omni.cpp:165-180), the distance test against Get{Min,Max}DistanceInvariance
 * (src/cMapPoint.cpp:498-508), the predicted level, cMultiKeyFrame::GetFeaturesInArea
 * (src/cMultiKeyFrame.cpp:703-746) and the best-distance scan do not depend on map state and run
 * on the device, ONE query set against a batch of T targets per call.  The state-dependent tails
 * (:1379-1415, :1536-1563, :1692-1715) are mcs_fuse_select on the host, one target at a time.
 *
 * What the three rules differ in (all reproduced):
 *   dist3D is `const float` in rules 0 and 1 (:1306, :1464: cv::norm rounded to float, then
 *   compared and divided in double) and double in rule 2 (:1623);
 *   the camera centre is the translation of M_t (cMultiKeyFrame::GetCameraCenter,
 *   src/cMultiKeyFrame.cpp:159-165; rule 2: Hom2T(Get_M_t()), :1585);
 *   rule 1 never assigns `dist` (:1511, :1514 discard the result): bestDist is 0 and bestIdx the
 *   first window candidate whose level passes :1501.  MCS_FUSE_USE_DISTANCE makes rule 1 scan
 *   distances as rules 0 and 2 do (the evidently intended behaviour; not what the reference runs);
 *   rule 0 computes E12 = ComputeE(curKF.Get_MtMc_inv(cam) * pKF.Get_MtMc(cam))
 *   (include/misc.h:235-243, the one-argument form) with `cam` the projection camera in pKF for
 *   BOTH keyframes (:1392-1396) and tests CheckDistEpipolarLine(ray of curKF keypoint i, ray of
 *   the best pKF keypoint, E12, 1e-2) (:1390-1398, src/misc.cpp:54-70);
 *   rule 2 takes M_t = invMat(Rt2Hom(sRcw / s, tcw / s)) (:1576-1585): the caller builds it on
 *   the host (host/mcs_multicol.hpp does, in the reference's operation order).
 * Shared: level = min(lower_bound(scaleFactors, dist3D / minDistance), nLevels - 1), radius =
 * th * scaleFactors[level], a candidate's octave must be level - 1 or level, the first minimum
 * in GetFeaturesInArea order wins (strict <), a camera contributes when bestDist <= th_low.
 *
 * Batch contract: the device result for target t is the reference's result provided no query's
 * descriptor changed before its turn at t.  Inside a Fuse sequence a map point's descriptor changes only
 * when it survives a Replace as pMPinKF (ComputeDistinctiveDescriptors, src/cMapPoint.cpp:244);
 * positions and distances do not change.  mcs_fuse_select reports the REPLACE survivors that are
 * themselves queries; the caller refreshes those descriptor rows and re-runs the remaining
 * targets (mcs::Fuse of host/mcs_multicol.hpp does).  Inside ONE target a descriptor can change
 * before its point's turn only when the point is listed more than once and rule 2 runs it again
 * (rules 0 and 1 skip the repeat through IsInKeyFrame once it added or was replaced): a point that
 * added at its first listing, then survived another query's Replace, is scanned at its second
 * listing with the row computed from its old descriptor.  A caller that lists a point twice under
 * rule 2 runs that target again when mcs_fuse_select reports the point among the survivors;
 * mcs::Fuse does not.  q_skip is the caller's snapshot of the
 * per-target skip condition (isBad / IsInKeyFrame / already found); those only grow during a
 * sequence, so a snapshot never skips a pair the reference would process. */
#define MCS_FUSE_USE_DISTANCE 1   /* flags: rule 1 scans descriptor distances */

/* T target keyframes packed back to back: target t owns keypoints off[t] .. off[t+1] of kp_xy /
 * kp_octave / kp_cam / desc / mask / rays / cell_kp; keypoint and grid indices are local to the
 * target.  All targets share the rig (m_c, cam, mirror, grid_params) and the scale pyramid.
 * n_kp_total = off[n_targets] is given on the host.  Every target holds < 2^19 keypoints (the
 * position field of the selection key): mcs_fuse checks each target and rejects a larger one;
 * for mcs_fuse_device the per-target counts are device data, so this is the caller's
 * precondition, and the kernel reads at most the first 2^19 - 1 keypoints of a target.  The
 * total over the batch is not limited.  The bottom rows of m_t / m_c are 0 0 0 1. */
typedef struct mcs_fuse_targets {
  int32_t n_targets, n_kp_total, n_cams, bytes, n_levels, mirror_w, mirror_h;
  const int32_t* off;          /* [n_targets + 1], off[0] = 0, non-decreasing */
  const float* kp_xy;          /* [n_kp_total][2] mvKeys pt */
  const int32_t* kp_octave;    /* [n_kp_total] */
  const int32_t* kp_cam;       /* [n_kp_total] keypoint_to_cam; read by mcs_fuse only (grid build) */
  const uint8_t* desc;         /* [n_kp_total][bytes] */
  const uint8_t* mask;         /* nullable [n_kp_total][bytes] mdBRIEF masks (havingMasks) */
  const double* rays;          /* [n_kp_total][3] GetKeyPointRay; rule 0 only */
  const double* m_t;           /* [n_targets][16] Get_M_t(), row-major 4x4 */
  const double* m_c;           /* [n_cams][16] M_c, row-major 4x4 */
  const double* cam;           /* [n_cams][17] as mcs_is_in_frustum_device: c d e u0 v0 invP[12] */
  const uint8_t* mirror;       /* [n_cams][mirror_h][mirror_w] mirrorMasks[0] */
  const double* grid_params;   /* [n_cams][4] as mcs_frame_grid_build */
  const double* scale;         /* [n_levels] mvScaleFactors */
  const int32_t* cell_ptr;     /* [n_targets][n_cams*64*48 + 1] mcs_frame_grid_build per target */
  const int32_t* cell_kp;      /* [n_kp_total], target t's list at off[t]; mcs_fuse builds both */
} mcs_fuse_targets;

typedef struct mcs_fuse_queries {
  int32_t nq;
  const double* pos;           /* [nq][3] GetWorldPos */
  const double* dist;          /* [nq][2] mfMinDistance, mfMaxDistance (the 0.8 / 1.2 are applied) */
  const uint8_t* desc;         /* [nq][bytes] GetDescriptorPtr */
  const uint8_t* mask;         /* nullable [nq][bytes]; given iff the targets have masks */
  const double* rays;          /* rule 0: [nq][3] curKF->GetKeyPointRay(i) */
  const double* m_t;           /* rule 0: [16] curKF Get_M_t() */
} mcs_fuse_queries;

/* Device scratch of mcs_fuse_device (per target and camera: M_t M_c and, for rule 0, E12). */
typedef struct mcs_fuse_workspace mcs_fuse_workspace;
int mcs_fuse_workspace_create(int32_t device, int32_t max_targets, mcs_fuse_workspace** out);
void mcs_fuse_workspace_destroy(mcs_fuse_workspace* ws);

/* The device part for all targets in two launches.  Every pointer inside targets / queries and
 * every d_* is a device pointer.  Out, each [n_targets][nq][n_cams]:
 *   d_best_kp    bestIdx (local to the target) when bestDist <= th_low, else -1
 *   d_best_dist  bestDist of the scan (also when above th_low); INT_MAX when the camera was left
 *                before the scan or no candidate passed the level test
 *   d_epi_ok     rule 0 (else nullable, not written): the CheckDistEpipolarLine verdict for every
 *                hit, 0 where best_kp is -1; whether the text consults it depends on map state
 * d_q_skip nullable [n_targets][nq]: nonzero = -1 / INT_MAX / 0 for all cameras, no work.
 * th = the search radius factor (2.5 / 3.0 in the callers), th_low = TH_LOW_ of the cORBmatcher
 * ctor (:46-65).  Stream-ordered, no host synchronisation, no allocation with a workspace; ws
 * NULL = a temporary one is allocated and freed (which synchronises).  Offsets, counts and grid
 * entries are device data and are clamped in the kernel: a malformed set reads nothing outside
 * its buffers.  MCS_ERR_ARG: rule outside 0..2, bytes not 16 / 32 / 64, more than 8 cameras,
 * a mask on one side only, n_targets above the workspace, a null buffer; mcs_fuse also for a
 * target of 2^19 keypoints or more and for malformed offsets. */
int mcs_fuse_device(mcs_fuse_workspace* ws, int32_t rule, int32_t flags,
                    const mcs_fuse_targets* targets, const mcs_fuse_queries* queries, double th,
                    int32_t th_low, const uint8_t* d_q_skip, int32_t* d_best_kp,
                    int32_t* d_best_dist, uint8_t* d_epi_ok, void* stream);

/* Host-buffer form for the reference's call sites: builds every target's grid
 * (mcs_frame_grid_build; cell_ptr / cell_kp of `targets` are ignored), uploads, runs
 * mcs_fuse_device on `device` and downloads.  MCS_ERR_NO_DEVICE without a GPU. */
int mcs_fuse(int32_t device, int32_t rule, int32_t flags, const mcs_fuse_targets* targets,
             const mcs_fuse_queries* queries, double th, int32_t th_low, const uint8_t* q_skip,
             int32_t* best_kp, int32_t* best_dist, uint8_t* epi_ok);

/* The state-dependent tail of Fuse for ONE target (:1279-1287 + :1379-1415, :1433-1440 +
 * :1536-1563, :1596-1602 + :1692-1715) over a flat stand-in of the map.  Host code, no GPU.
 *   q_mp [nq]             map-point id of query i, -1 = NULL (skipped)
 *   best_kp [nq][n_cams]  the target's rows of mcs_fuse_device; epi_ok likewise (rule 0)
 *   mp_bad [n_mp]         in/out cMapPoint::isBad
 *   mp_in_kf [n_mp]       in/out cMapPoint::IsInKeyFrame(target) (src/cMapPoint.cpp:447-451)
 *   kp_mp [n_kp]          in/out the target's mvpMapPoints as ids, -1 = NULL.  A map point with
 *                         mp_in_kf set observes the target at exactly the slots that hold it.
 * Queries in order; a query is skipped when bad or in the keyframe (rules 0, 1) or when bad or in
 * spAlreadyFound = the non-bad points in the slots at entry (rule 2, :1588, :1601).  For each
 * camera with best_kp >= 0, in camera order: an occupied slot fuses when its point is not bad
 * (rule 0: and epi_ok), REPLACE = pMP->Replace(pMPinKF) (src/cMapPoint.cpp:208-250) then
 * ++nFused (also when Replace returns early on equal ids); an empty slot gives ADD =
 * AddObservation (:90-96) + AddMapPoint (src/cMultiKeyFrame.cpp:273-277).  The effects on the
 * target's own state are applied as the text does: ADD fills the slot and sets mp_in_kf; REPLACE
 * marks the query bad, clears its mp_in_kf and moves the slots it holds to the survivor, or
 * erases them when the survivor is already in the keyframe (the IsInKeyFrame branch of Replace);
 * a query that has turned bad still runs its remaining cameras.
 * Out: actions [n_actions][4] = (kind, query, keypoint, other_id) in execution order, kind
 * MCS_FUSE_ADD (other_id = the query's map point) or MCS_FUSE_REPLACE (other_id = the
 * survivor); the caller replays them onto the other keyframes of its map.  action_cap >=
 * nq * n_cams always suffices (MCS_ERR_CAPACITY otherwise).  *n_fused = the return value.
 * requery_ids (nullable, capacity nq) / *n_requery: the distinct REPLACE survivors (other than
 * the replaced point itself) that are also in q_mp, in order of first survival: their
 * descriptors change (batch contract above). */
#define MCS_FUSE_ADD 0
#define MCS_FUSE_REPLACE 1
int mcs_fuse_select(int32_t rule, int32_t nq, int32_t n_cams, const int32_t* q_mp,
                    const int32_t* best_kp, const uint8_t* epi_ok, int32_t n_mp, uint8_t* mp_bad,
                    uint8_t* mp_in_kf, int32_t n_kp, int32_t* kp_mp, int32_t* actions,
                    int32_t action_cap, int32_t* n_actions, int32_t* n_fused,
                    int32_t* requery_ids, int32_t* n_requery);

/* ---- SearchBySim3: mutual projection matching under a loop Sim3 -----------------------------
 *   int SearchBySim3(cMultiKeyFrame* pKF1, cMultiKeyFrame* pKF2, vector<cMapPoint*>& vpMatches12,
 *                    const double& s12, const cv::Matx33d& R12, const cv::Vec3d& t12, double th)
 *                                          src/cORBmatcher.cpp:1721-1988, called per loop candidate
 *       by cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:369) with th = 10
 * The whole function runs on the device, ONE current keyframe KF1 against a batch of T
 * candidates KF2_t, each with its own Sim3: the transforms (GetPoseInverse,
 * src/cMultiKeyFrame.cpp:152-157; invMat, src/cConverter.cpp:31-44; sR12, sR21, t21, :1741-1743),
 * direction 1 (:1779-1872: every active map point of KF1 into KF2_t), direction 2 (:1874-1967:
 * every active map point of KF2_t into KF1) and the agreement check (:1969-1987).  Nothing in it
 * depends on map state that changes during the call, so there is no host tail.
 *
 * Per keypoint, as the text has it: only the keypoint's own camera c is searched
 * (keypoint_to_cam, :1790, :1884); p3Dc = the Sim3 chain in the rig frame, p4Dc =
 * invMat(M_c[c]) * (p3Dc, 1); the point is left when the RIG-frame z is negative (:1798, :1892:
 * p3Dc2(2), not the camera-frame depth); WorldToImg (src/cam_model_omni.cpp:147-163) and
 * isPointInMirrorMask(u, v, 0) (:165-180); dist3D = cv::norm of the camera-frame point in double
 * against Get{Min,Max}DistanceInvariance (src/cMapPoint.cpp:498-508); level =
 * min(lower_bound(scaleFactors, dist3D / minDistance), nLevels - 1), radius = th *
 * scaleFactors[level]; GetFeaturesInArea(c, u, v, radius) (src/cMultiKeyFrame.cpp:703-746) in its
 * enumeration order, octave level - 1 or level, DescriptorDistance64[Masked] between the MAP
 * POINT's descriptor and the keypoint's row, first minimum under strict <, a match when bestDist
 * <= th_high.  Direction 1 takes the camera model and M_c from KF2's rig; direction 2 takes the
 * camera model from KF2's rig and M_c from KF1's (:1885, :1889).  Both keyframes share the rig in
 * the reference; here n_cams, bytes, n_levels and the mirror size of the two sets must agree.
 *
 * Keyframes are mcs_fuse_targets sets: kf1 with n_targets == 1, kf2s with the T candidates.
 * Unlike mcs_fuse_device, the device entry READS kp_cam (the keypoint's camera); rays is unused. */

/* The map points in the keypoint slots of a packed keyframe set: slot i belongs to keypoint i of
 * the set's packed arrays (n = the set's n_kp_total).  Rows of slots that are not active are not
 * read. */
typedef struct mcs_sim3_points {
  int32_t n;
  const double* pos;           /* [n][3] GetWorldPos */
  const double* dist;          /* [n][2] mfMinDistance, mfMaxDistance (the 0.8 / 1.2 are applied) */
  const uint8_t* desc;         /* [n][bytes] GetDescriptorPtr: the map point's descriptor, not the keypoint's row */
  const uint8_t* mask;         /* nullable [n][bytes]; given iff the keyframes have masks */
} mcs_sim3_points;

/* Device scratch of mcs_search_by_sim3_device for batches of <= max_targets candidates of
 * <= max_kp keypoints each (and a KF1 of <= max_kp): the transforms, and vnMatch1 / vnMatch2
 * when the caller does not ask for them. */
typedef struct mcs_sim3_workspace mcs_sim3_workspace;
int mcs_sim3_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp,
                              mcs_sim3_workspace** out);
void mcs_sim3_workspace_destroy(mcs_sim3_workspace* ws);

/* SearchBySim3 (src/cORBmatcher.cpp:1721-1988) for all candidates in three launches.  Every
 * pointer inside the sets / points and every d_* is a device pointer.  n1 = kf1->n_kp_total.
 *   d_active1 [T][n1]           the caller's snapshot of pMP && !vbAlreadyMatched1 && !pMP->isBad()
 *                               (:1784-1788) per candidate, as vpMatches12 differs per candidate
 *   d_active2 [n_kp_total of kf2s]  the same for :1878-1882, packed like the candidates
 *   d_s12 [T], d_R12 [T][9] row-major, d_t12 [T][3]
 *   th = the radius factor (10 at the call site), th_high = TH_HIGH_ of the cORBmatcher ctor
 *   (:46-65): 3 * bytes, or floor(1.5 * bytes) with masks
 * Out, indices local to their keyframe:
 *   d_match1 [T][n1]            vnMatch1 (nullable: kept in the workspace)
 *   d_match2 [n_kp_total]       vnMatch2, packed like the candidates (nullable likewise)
 *   d_matches12 [T][n1]         idx2 when vnMatch1[i1] = idx2 >= 0 and vnMatch2[idx2] == i1, else -1
 *                               (vpMatches12[i1] = vpMapPoints2[idx2], :1981)
 *   d_n_found [T]               the return value per candidate
 * A direction-1 hit on a KF2 keypoint that is not active gives no match: its vnMatch2 is -1.
 * Stream-ordered, no host synchronisation, no allocation with a workspace; ws NULL = a temporary
 * one is allocated and freed (which synchronises).  Offsets, counts, cell entries and camera
 * indices are device data and are clamped in the kernel: a malformed set reads nothing outside
 * its buffers, and a keypoint whose camera is outside [0, n_cams) never matches.
 * MCS_ERR_ARG: bytes not 16 / 32 / 64, more than 8 cameras, masks on one side only,
 * kf1->n_targets != 1, T or the keypoint counts above the workspace, a keyframe of 2^19
 * keypoints or more (kf1 here; per candidate it is the caller's precondition, as in
 * mcs_fuse_device), a null buffer, n_cams / bytes / n_levels / mirror size differing between kf1
 * and kf2s. */
int mcs_search_by_sim3_device(mcs_sim3_workspace* ws, const mcs_fuse_targets* kf1,
                              const mcs_sim3_points* pts1, const mcs_fuse_targets* kf2s,
                              const mcs_sim3_points* pts2, const uint8_t* d_active1,
                              const uint8_t* d_active2, const double* d_s12, const double* d_R12,
                              const double* d_t12, double th, int32_t th_high, int32_t* d_match1,
                              int32_t* d_match2, int32_t* d_matches12, int32_t* d_n_found,
                              void* stream);

/* Host-buffer form for the call site (src/cLoopClosing.cpp:369): builds every grid
 * (mcs_frame_grid_build; cell_ptr / cell_kp of the sets are ignored), uploads, runs
 * mcs_search_by_sim3_device on `device` and downloads; match1 / match2 nullable.  Also
 * MCS_ERR_ARG for malformed offsets, a candidate of 2^19 keypoints or more and a kp_cam outside
 * [0, n_cams); all argument errors are returned before any device use.  MCS_ERR_NO_DEVICE
 * without a GPU. */
int mcs_search_by_sim3(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                       const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2,
                       const uint8_t* active1, const uint8_t* active2, const double* s12,
                       const double* R12, const double* t12, double th, int32_t th_high,
                       int32_t* match1, int32_t* match2, int32_t* matches12, int32_t* n_found);

/* ---- cSim3Solver: the loop-closing Sim3 RANSAC ------------------------------------------------
 *   cSim3Solver::cSim3Solver(pKF1, pKF2, vpMatched12, camSys)     src/cSim3Solver.cpp:44-137
 *   SetRansacParameters(probability, minInliers, maxIterations)   src/cSim3Solver.cpp:139-165
 *   iterate(nIterations, bNoMore, vbInliers, nInliers, result)    src/cSim3Solver.cpp:167-254
 *   find                                                          src/cSim3Solver.cpp:256-262
 *   centroid, computeT (Horn 1987 on three points)                src/cSim3Solver.cpp:264-371
 *   CheckInliers                                                  src/cSim3Solver.cpp:374-415
 * called per loop candidate by cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:311-364) between
 * SearchByBoW(KF, KF) and SearchBySim3.  Here ONE current keyframe KF1 against a batch of T
 * candidates: the constructor, the RANSAC and the hand-over to SearchBySim3 are stream-ordered
 * device entries, so BoW -> prepare -> iterate -> active -> SearchBySim3 runs with nothing
 * downloaded.  Keyframes are mcs_fuse_targets sets (kf1 with n_targets == 1, kf2s with the T
 * candidates), map points mcs_sim3_points of which only pos is read.  Everything is FP64.
 *
 * A hypothesis depends on no RANSAC state: every iteration samples afresh from mvAllIndices
 * (:202).  So one call evaluates all its iterations of all candidates in parallel and only the
 * acceptance rule (:228-253) is applied in iteration order.  The text draws with
 * std::random_device, which cannot be reproduced: the ABI takes the sample triples from the
 * caller.  cv::eigen and cv::Rodrigues are OpenCV internals, so a hypothesis's (s, R, t) is
 * Horn's solution to rounding (cyclic Jacobi on the 4x4), not bitwise; where the top eigenvalue
 * of N is not simple (a repeated index, a collinear triple) the text itself does not define the
 * rotation.  Everything after the hypothesis follows the text's operation order exactly. */

/* The three correspondence indices of each iteration from its three dis(gen) values, exactly as
 * :202-222 do (host, integers only; no GPU).  vAvailableIndices starts as 0 .. n-1 (mvAllIndices),
 * the distribution stays 0 .. n-1 while the vector shrinks, and the swap is written to the drawn
 * VALUE (`vAvailableIndices[idx] = back()`, :220), not to the drawn position: a triple can
 * repeat an index.  A draw at or past the vector's current size reads out of range in the text;
 * here the vector is an array of n whose popped elements keep their value, which is what an
 * unchecked std::vector does.  draws, samples [n_its][3].  MCS_ERR_ARG: n < 3, a draw outside
 * [0, n), a null buffer. */
int mcs_sim3_draw_samples(int32_t n, const int32_t* draws, int32_t n_its, int32_t* samples);

/* What the constructor builds, per candidate t, rows t * cap .. t * cap + n[t], cap = n1 =
 * kf1->n_kp_total, in i1 order (the order of mvnIndices1).  m_c / cam / n_cams are camSysLocal
 * (:51), the rig CheckInliers projects with (:391-398): the caller sets them, at the call site
 * to KF1's m_c and cam.  In the host-buffer form the pointers are host outputs, each nullable,
 * and m_c / cam are ignored (KF1's are taken). */
typedef struct mcs_sim3_corr {
  int32_t n_targets, cap, n_cams;
  const double* m_c;           /* [n_cams][16] */
  const double* cam;           /* [n_cams][17] c d e u0 v0 invP[12] */
  int32_t* n;                  /* [T] N = mvpMapPoints1.size() */
  int32_t* idx1;               /* [T][cap] mvnIndices1 */
  double* X1;                  /* [T][cap][3] mvX3Dc1 */
  double* X2;                  /* [T][cap][3] mvX3Dc2 */
  double* p1;                  /* [T][cap][2] mvP1im1 */
  double* p2;                  /* [T][cap][2] mvP2im2 */
  int32_t* cam1;               /* [T][cap] camIdx1 */
  int32_t* cam2;               /* [T][cap] camIdx2 */
  double* maxerr1;             /* [T][cap] mvnMaxError1 (whole numbers: the text stores size_t) */
  double* maxerr2;             /* [T][cap] mvnMaxError2 */
} mcs_sim3_corr;

/* The solver's members that live across iterate calls (in/out) and the outputs of one call. */
typedef struct mcs_sim3_ransac {
  int32_t* iterations;         /* [T] mnIterations */
  int32_t* best_inliers;       /* [T] mnBestInliers */
  int32_t* max_its;            /* [T] mRansacMaxIts; 0 when N < min_inliers (the text leaves it undefined) */
  uint64_t* best_words;        /* [T][(cap + 63) / 64] mvbBestInliers, bit i = correspondence i */
  double* s12;                 /* [T] mBestScale */
  double* R12;                 /* [T][9] mBestRotation, row-major */
  double* t12;                 /* [T][3] mBestTranslation */
  double* T12;                 /* [T][16] mBestT12 (`result` on a success) */
  int32_t* success;            /* out [T] the return value */
  int32_t* no_more;            /* out [T] bNoMore */
  int32_t* n_inliers;          /* out [T] nInliers */
  uint8_t* inlier;             /* out [T][cap] vbInliers, scattered through idx1 */
  double* hyp_srt;             /* out, nullable [T][n_iterations][13] s, R, t of every hypothesis evaluated */
  int32_t* hyp_inl;            /* out, nullable [T][n_iterations] mnInliersi; -1 = not evaluated */
} mcs_sim3_ransac;

/* The constructor (:44-137) for all T candidates in one launch.  Device pointers throughout.
 *   d_matches12 [T][n1]   KF2 keypoint index whose slot holds pMP2 = vpMatched12[i1], -1 = none:
 *                         the output format of mcs_search_by_bow_kf_device
 *   d_ok1 [n1]            KF1's slot i1 holds a point that is not bad (:77, :82)
 *   d_ok2 [n_kp_total of kf2s]  the slot's point is not bad (:82), packed like the candidates
 *   d_first1 [n1]         (int)GetIndexInKeyFrame(pKF1)[0] of the slot's point, local to the
 *                         keyframe; -1 when the point does not observe it (src/cMapPoint.cpp:436-445)
 *   d_first2              the same for the candidates, packed like them
 *   d_sigma2 [n_levels]   mvLevelSigma2
 * A slot is skipped without a match, with !ok1, with !ok2 of the matched slot, or when either
 * first index is negative (:73-98).  Octave, camera and projection are those of keypoint `first`
 * (idxs[0], :94-125), not of i1 / the matched slot; the positions are those of the slots' points.
 * X = Hom2R(invMat(M_t)) * Xw + Hom2T(invMat(M_t)) in cv::Matx operation order (:118, :127), p =
 * WorldToCamHom_fast in the camera of keypoint `first` (:116, :125), maxerr = 9.210 * sigma2[octave
 * of keypoint first] truncated toward zero (:106-107: mvnMaxError1 / 2 are std::vector<size_t>,
 * include/cSim3Solver.h:92-93; CheckInliers compares against the integer as a double).  Rows are compacted in i1 order (a ballot prefix, no atomics).
 * Indices that are device data are clamped: a match or first index outside its keyframe, an octave
 * outside [0, n_levels) or a camera outside [0, n_cams) skips the slot (the text reads out of range
 * there).  Stream-ordered, no host synchronisation, no allocation.  MCS_ERR_ARG: kf1->n_targets !=
 * 1, n_cams / n_levels differing between the sets, more than 8 cameras, a KF1 of 2^19 keypoints or
 * more, points not matching their set, corr's n_targets / cap / n_cams not T / n1 / n_cams, a null
 * buffer. */
int mcs_sim3_solver_prepare_device(const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                                   const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2,
                                   const int32_t* d_matches12, const uint8_t* d_ok1,
                                   const uint8_t* d_ok2, const int32_t* d_first1,
                                   const int32_t* d_first2, const double* d_sigma2,
                                   const mcs_sim3_corr* corr, void* stream);

/* Device scratch of mcs_sim3_solver_iterate_device for <= max_targets candidates of <= max_kp
 * correspondences and calls of <= max_its_cap iterations: the hypotheses, their inlier words and
 * counts, invMat(M_c). */
typedef struct mcs_sim3_solver_workspace mcs_sim3_solver_workspace;
int mcs_sim3_solver_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp,
                                     int32_t max_its_cap, mcs_sim3_solver_workspace** out);
void mcs_sim3_solver_workspace_destroy(mcs_sim3_solver_workspace* ws);

#define MCS_SIM3_SET_PARAMS 1   /* SetRansacParameters (:139-165): max_its from n[t], iterations = 0 */
#define MCS_SIM3_INIT 2         /* the constructor's state (:48-49) as well: best_inliers = 0, mBest* = 0 */

/* iterate (:167-254) for all candidates: iterations [iterations[t], min(iterations[t] +
 * n_iterations, max_its[t])) of every candidate in four launches (parameters and invMat(M_c);
 * computeT per (candidate, iteration); CheckInliers with lanes over correspondences and the rows
 * staged per block; the acceptance rule, one wave per candidate).
 *   d_samples [T][max_its_cap][3]  the correspondence indices of iteration k of candidate t
 *                                  (mcs_sim3_draw_samples), any value in [0, n[t]), repeats included
 *   flags  MCS_SIM3_INIT at the first call after prepare, MCS_SIM3_SET_PARAMS for a later
 *          SetRansacParameters, 0 to go on.  max_its = max(1, min(ceil(log(1 - prob) /
 *          log(1 - pow(min_inliers / N, 3))), max_its_cap)), 1 when N == min_inliers, computed on
 *          the device from n[t]; max_its_cap where pow(.., 3) underflows against 1 (the text's int
 *          conversion of -inf is undefined there).  For N < min_inliers iterate returns at :177 whatever
 *          mRansacMaxIts holds: max_its = 0, no_more = 1, success = 0.
 * The running best updates when mnInliersi >= mnBestInliers (:228: ties take the later
 * iteration); a hit is the first iteration that does so with mnInliersi > min_inliers (:237), and
 * iterations stops behind it; no_more = no hit in this call and iterations >= max_its (:250).
 * mBest* are updated whenever the text updates them, also without a hit.  find (:256-262) is
 * n_iterations = max_its_cap.  A NaN hypothesis (a repeated index gives den == 0) has no inliers.
 * Launch sizes come from T, n_iterations and cap only.  Stream-ordered, no host synchronisation,
 * no allocation with a workspace; ws NULL = a temporary one is allocated and freed (which
 * synchronises).  Counts, indices and cameras in corr and d_samples are device data and are
 * clamped.  MCS_ERR_ARG: n_iterations outside [1, max_its_cap], min_inliers < 1, prob outside
 * (0, 1), an unknown flag, more than the workspace holds, a null buffer. */
int mcs_sim3_solver_iterate_device(mcs_sim3_solver_workspace* ws, const mcs_sim3_corr* corr,
                                   const int32_t* d_samples, int32_t n_iterations, double prob,
                                   int32_t min_inliers, int32_t max_its_cap, int32_t flags,
                                   const mcs_sim3_ransac* ransac, void* stream);

/* The hand-over to SearchBySim3: d_active1 [T][n1] and d_active2 (packed like the candidates) as
 * src/cORBmatcher.cpp:1758-1774 and the loops' skip conditions see them when vpMatches12 holds
 * the inliers' entries alone (src/cLoopClosing.cpp:354-360).  d_good1 [n1] / d_good2 (packed):
 * the slot holds a map point that is not bad.  active1 = good1 && !inlier; active2 = good2,
 * cleared at first2 of the slot every inlier is matched to, when that lies in [0, N2).  Two
 * launches, stream-ordered. */
int mcs_sim3_solver_active_device(const mcs_fuse_targets* kf1, const mcs_fuse_targets* kf2s,
                                  const uint8_t* d_inlier, const uint8_t* d_good1,
                                  const uint8_t* d_good2, const int32_t* d_matches12,
                                  const int32_t* d_first2, uint8_t* d_active1, uint8_t* d_active2,
                                  void* stream);

/* Host-buffer form for the call site (src/cLoopClosing.cpp:311-364): uploads, runs prepare,
 * iterate and (when active1 / active2 are given) the hand-over on `device`, downloads.  Of the
 * keyframe sets off, kp_octave, kp_cam, m_t, m_c and cam are read.  samples [T][max_its_cap][3];
 * corr nullable; the state arrays of `ransac` are host in/out (read unless flags has
 * MCS_SIM3_INIT).  Also MCS_ERR_ARG for malformed offsets; all argument errors are returned
 * before any device use.  MCS_ERR_NO_DEVICE without a GPU. */
int mcs_sim3_solver(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                    const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2,
                    const int32_t* matches12, const uint8_t* ok1, const uint8_t* ok2,
                    const int32_t* first1, const int32_t* first2, const double* sigma2,
                    const int32_t* samples, int32_t n_iterations, double prob, int32_t min_inliers,
                    int32_t max_its_cap, int32_t flags, const mcs_sim3_corr* corr,
                    const mcs_sim3_ransac* ransac, const uint8_t* good1, const uint8_t* good2,
                    uint8_t* active1, uint8_t* active2);

/* ---- OptimizeSim3: the Sim3 refinement of a loop candidate ------------------------------------
 *   int cOptimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12)   src/cOptimizerLoopStuff.cpp:63-270
 *   VertexSim3Expmap_Multi, EdgeSim3ProjectXYZ_Multi, EdgeInverseSim3ProjectXYZ_Multi
 *                                                    include/g2o_MultiCol_sim3_expmap.h:117-260
 *   g2o::Sim3 (exp, map, inverse, operator*)         ThirdParty/g2o/g2o/types/sim3.h:41-292
 * called per loop candidate by cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:372-378) after
 * SearchBySim3.  Here ONE current keyframe KF1 against a batch of T candidates, one workgroup per
 * candidate, the whole function in one launch: the slot rules (:122-161), both rounds of
 * Levenberg-Marquardt on the one 7-dof vertex (:209-210, :243-245), the cull between them
 * (:212-232), the `< 3` return (:240-241), the final flags (:247-263) and the recover (:265-267).
 * Everything is FP64.  The LM control is g2o's (csrc/lm_control.hpp); the terminate action's stop
 * flag lives across both rounds, so round 2 runs no iteration after a gain stop in round 1.
 *
 * Reproduced as written:
 *   - e21's information is GetSigma2(octave of keypoint i2), sigma^2 and not 1 / sigma^2 (:194);
 *   - the observation of e21 is KF2's keypoint i2 = GetIndexInKeyFrame(pKF2)[0], not the matched
 *     slot (:133, :186);
 *   - the camera lookup is crossed: e12 projects with camera keypoint_to_cam1[i2] (vPoint2 carries
 *     SetID(i2), :154), e21 with keypoint_to_cam2[i] (vPoint1 carries SetID(i), :145).  Where that
 *     lookup leaves the map (i2 >= n1, or i >= n2 of the candidate) the text dereferences end():
 *     such a slot is dropped, its match set to -1 and it is counted in n_undefined.
 *     MCS_SIM3OPT_OWN_CAMERA takes keypoint_to_cam1[i] and keypoint_to_cam2[i2] instead;
 *   - after round 1 a pair is culled when either chi2 is strictly above (1.345 * std_sim)^2;
 *     with fewer than 3 pairs left the function returns 0 with those matches already nulled and
 *     the Sim3 unchanged.
 * The text's edges define no linearizeOplus, so g2o differentiates numerically (delta = 1e-9,
 * base_binary_edge.hpp:147-172); here the Jacobian is analytic, which agrees with the text to the
 * scatter of that difference quotient, while every count and flag is exact. */
#define MCS_SIM3OPT_OWN_CAMERA 1   /* flags: each edge projects with its own observation's camera */

typedef struct mcs_sim3_opt_options {
  double std_sim;               /* cOptimizer::stdSim: 4.0 (:55); Huber delta = 1.345 * std_sim (:114) */
  int32_t its_round1;           /* optimize(5) (:210) */
  int32_t its_clean;            /* nMoreIterations when nBad == 0: 5 (:238) */
  int32_t its_culled;           /* nMoreIterations when nBad > 0: 10 (:236) */
  int32_t terminate_max_iter;   /* SparseOptimizerTerminateAction max iterations: 15 (:81) */
  double gain_threshold;        /* its gain threshold: 1e-6 (:80) */
  double tau;                   /* LM lambda init factor: 1e-5 (g2o default) */
  int32_t max_trials;           /* LM maxTrialsAfterFailure: 10 (g2o default) */
  int32_t flags;                /* MCS_SIM3OPT_* */
} mcs_sim3_opt_options;

/* The reference's values (:55, :80-81, :210, :234-238 and g2o's defaults), flags = 0. */
void mcs_sim3_opt_default_options(mcs_sim3_opt_options* o);

/* Outputs of one call, per candidate t; device pointers in the device form, host in the other. */
typedef struct mcs_sim3_opt_out {
  int32_t* n_in;               /* [T] the return value (:269); 0 on the `< 3` return (:241) */
  int32_t* n_corr;             /* [T] nCorrespondences (:163) */
  int32_t* n_bad;              /* [T] nBad after round 1 (:213-232) */
  int32_t* n_undefined;        /* [T] slots dropped because the crossed camera lookup leaves its map */
  double* s12;                 /* [T] the recovered Sim3 (:266-267); the input on the `< 3` return */
  double* q12;                 /* [T][4] w, x, y, z (Eigen's conversion of the input R on that return) */
  double* R12;                 /* [T][9] row-major */
  double* t12;                 /* [T][3] */
  int32_t* iters;              /* [T][2] iterations run by optimize() in round 1 / round 2 */
  double* chi2;                /* [T][2] activeRobustChi2 after each round (0 where it did not run) */
  double* lambda;              /* [T][2] the LM lambda after each round (0 where no iteration ran) */
  int32_t* trials;             /* nullable [T][2][16] LM trials of every iteration (levenbergIteration()) */
  double* edge_chi2;           /* nullable [T][n1][2] chi2 of e12 / e21 after the last round run, NaN = slot not kept */
} mcs_sim3_opt_out;

/* Device scratch of mcs_optimize_sim3_device for <= max_targets candidates and a KF1 of <= max_kp
 * keypoint slots: the compacted rows of the kept slots. */
typedef struct mcs_sim3_opt_workspace mcs_sim3_opt_workspace;
int mcs_sim3_opt_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp,
                                  mcs_sim3_opt_workspace** out);
void mcs_sim3_opt_workspace_destroy(mcs_sim3_opt_workspace* ws);

/* OptimizeSim3 (src/cOptimizerLoopStuff.cpp:63-270) for all T candidates in one launch.  The
 * slot data are those of mcs_sim3_solver_prepare_device:
 *   d_matches12 [T][n1]   in: KF2 keypoint index whose slot holds pMP2 = vpMatches1[i], -1 = NULL
 *                         (:124); out: -1 wherever the text nulls the match (:225, :259) and at
 *                         slots dropped as undefined
 *   d_ok1 [n1]            KF1's slot i holds a point that is not bad (:135-137)
 *   d_ok2 [n_kp_total of kf2s]  the matched slot's point is not bad (:137)
 *   d_first2              i2 = (int)GetIndexInKeyFrame(pKF2)[0] (:133), -1 = does not observe KF2
 *   d_inv_sigma2_1 [n_levels]   KF1's mvInvLevelSigma2 (:176)
 *   d_sigma2_2 [n_levels]       KF2's mvLevelSigma2 (:194)
 *   d_s12 [T], d_R12 [T][9] row-major, d_t12 [T][3]   g2oS12 on entry: Sim3(R, t, s)
 * Of the sets kp_xy, kp_octave, kp_cam, off, m_t, m_c and cam are read; of the points pos.
 * A match, first index, octave or camera outside its range drops the slot.  Deterministic: no
 * floating-point atomics, a reduction order fixed by thread and stride, identical bits from run
 * to run and for a candidate alone or in a batch.  Stream-ordered, no host synchronisation, no
 * allocation with a workspace; ws NULL = a temporary one is allocated and freed (which
 * synchronises).  MCS_ERR_ARG: kf1->n_targets != 1, T or n1 above the workspace, more than 8
 * cameras, a KF1 of 2^19 keypoints or more, n_cams / n_levels differing between kf1 and kf2s,
 * points not matching their set, iteration counts outside [0, 16], max_trials outside [1, 64],
 * std_sim not positive, an unknown flag, a null buffer. */
int mcs_optimize_sim3_device(mcs_sim3_opt_workspace* ws, const mcs_fuse_targets* kf1,
                             const mcs_sim3_points* pts1, const mcs_fuse_targets* kf2s,
                             const mcs_sim3_points* pts2, int32_t* d_matches12, const uint8_t* d_ok1,
                             const uint8_t* d_ok2, const int32_t* d_first2,
                             const double* d_inv_sigma2_1, const double* d_sigma2_2,
                             const double* d_s12, const double* d_R12, const double* d_t12,
                             const mcs_sim3_opt_options* opts, const mcs_sim3_opt_out* out,
                             void* stream);

/* vpMapPointMatches as ComputeSim3 hands it to OptimizeSim3 (src/cLoopClosing.cpp:354-369), one
 * launch: d_matches12[t][i] = d_bow12[t][i] where d_inlier[t][i] (the RANSAC inliers' BoW
 * matches, :354-360), else d_new12[t][i] when >= 0 (SearchBySim3 fills the empty entries, :369),
 * else -1.  All [T][n1].  MCS_ERR_ARG: negative counts, T * n1 >= 2^31, a null buffer. */
int mcs_sim3_merge_matches_device(const int32_t* d_bow12, const uint8_t* d_inlier,
                                  const int32_t* d_new12, int32_t T, int32_t n1,
                                  int32_t* d_matches12, void* stream);

/* Host-buffer form for the call site (src/cLoopClosing.cpp:372): uploads, runs
 * mcs_optimize_sim3_device on `device`, downloads; matches12 is in-out, the pointers of `out` are
 * host outputs, each nullable.  Also MCS_ERR_ARG for malformed offsets; all argument errors are
 * returned before any device use.  MCS_ERR_NO_DEVICE without a GPU. */
int mcs_optimize_sim3(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                      const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2, int32_t* matches12,
                      const uint8_t* ok1, const uint8_t* ok2, const int32_t* first2,
                      const double* inv_sigma2_1, const double* sigma2_2, const double* s12,
                      const double* R12, const double* t12, const mcs_sim3_opt_options* opts,
                      const mcs_sim3_opt_out* out);

#ifdef __cplusplus
}
#endif
#endif /* MCS_MATCHER_H */
