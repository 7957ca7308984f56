// Header-only C++ host mirror of the reference operator surface, implemented on top of the
// C-ABI of libmcs_amd.so (include/mcs_extractor.h, mcs_matcher.h, mcs_ba.h).  A MultiCol-SLAM
// build keeps its call sites and swaps the types:
//
//   reference                                        here
//   mdBRIEFextractorOct(nfeatures, scaleFactor, ...)  mcs::mdBRIEFextractorOct(same args, w, h)
//     include/mdBRIEFextractorOct.h:339-351
//   operator()(image, mask, kps, camModel, desc,      operator()(image, stride, mask, mstride,
//              descMasks)  :355-361                      kps, camModel, desc, descMasks)
//   DescriptorDistance64 (include/cORBmatcher.h:43)   mcs::DescriptorDistance64
//   cOptimizer::LocalBundleAdjustment (cOptimizer.h:61) mcs::LocalBA::run(problem, ...)
//   cOptimizer::BundleAdjustment / GlobalBundleAdjustment (cOptimizer.h:50-59)
//                                                     mcs::GlobalBA::run(map, poseOnly, pbStopFlag)
//   cOptimizer::PoseOptimization (cOptimizer.h:67-69) mcs::PoseOptimizer::run(frame, inliers,
//                                                                        huberMultiplier)
//   cORBmatcher::SearchByProjection(F, vpMapPoints, th) / (CurrentFrame, LastFrame, th)
//     (src/cORBmatcher.cpp:67-166, :1991-2123)       mcs::SearchByProjection(rig, F, mapPoints, th, ...) /
//                                                     mcs::SearchByProjection(rig, mc6, Current, Last, ...)
//   cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:224-386)
//                                                     mcs::CreateNewMapPoints(rig, cur, neighbours, ...)
//   cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp:43-340)
//                                                     mcs::KeyFrameDatabase<cMultiKeyFrame>: add, erase, clear,
//                                                     DetectLoopCandidates, DetectRelocalisationCandidates, MinScore
//
// cv::KeyPoint-compatible: mcs_keypoint has cv::KeyPoint's field order and size (28 B), so a
// std::vector<mcs_keypoint> can be copied into std::vector<cv::KeyPoint> member-wise.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mcs_ba.h"
#include "../../include/mcs_essgraph.h"
#include "../../include/mcs_extractor.h"
#include "../../include/mcs_kfdb.h"
#include "../../include/mcs_matcher.h"
#include "../../include/mcs_newpoints.h"

namespace mcs {

inline void check(int rc, const char* what) {
  if (rc != MCS_OK)
    throw std::runtime_error(std::string(what) + ": " + mcs_last_error() + " (" + std::to_string(rc) + ")");
}

class mdBRIEFextractorOct {
 public:
  mdBRIEFextractorOct(int nfeatures, float scaleFactor, int nlevels, int edgeThreshold,
                      int firstLevel, int scoreType, int patchSize, int fastThreshold,
                      bool useAgast, int fastAgastType, bool do_dBrief, bool learnMasks,
                      int descSize, int width, int height, int device = 0) {
    mcs_extractor_params p;
    p.nfeatures = nfeatures; p.scale_factor = scaleFactor; p.nlevels = nlevels;
    p.edge_threshold = edgeThreshold; p.first_level = firstLevel; p.score_type = scoreType;
    p.patch_size = patchSize; p.fast_threshold = fastThreshold; p.use_agast = useAgast;
    p.fast_agast_type = fastAgastType; p.do_dbrief = do_dBrief; p.learn_masks = learnMasks;
    p.desc_size = descSize;
    check(mcs_extractor_create(&p, width, height, 1, device, &h_), "mcs_extractor_create");
    desc_size_ = descSize;
    do_dbrief_ = do_dBrief;
    learn_masks_ = learnMasks;
    nlevels_ = nlevels;
    scale_factor_ = scaleFactor;
  }
  ~mdBRIEFextractorOct() { mcs_extractor_destroy(h_); }
  mdBRIEFextractorOct(const mdBRIEFextractorOct&) = delete;
  mdBRIEFextractorOct& operator=(const mdBRIEFextractorOct&) = delete;

  // operator()(image, mask, kps, camModel, desc, descMasks) (:355-361).  The camera model is
  // read only by the dBRIEF / mdBRIEF branches (keypoint undistortion :1304-1316 and the
  // re-distorted pattern :250-283); it is forwarded to the device when it changes.
  void operator()(const uint8_t* image, int stride, const uint8_t* mask, int mask_stride,
                  std::vector<mcs_keypoint>& kps, const mcs_cam_model& camModel,
                  std::vector<uint8_t>& desc, std::vector<uint8_t>& descMasks) {
    if ((do_dbrief_ || learn_masks_) &&
        (!cam_set_ || std::memcmp(&cam_, &camModel, sizeof(cam_)) != 0)) {
      check(mcs_extractor_set_cam_models(h_, &camModel, 1), "mcs_extractor_set_cam_models");
      cam_ = camModel;
      cam_set_ = true;
    }
    const int cap = mcs_extractor_capacity(h_);
    kps.resize(cap);
    desc.resize((size_t)cap * desc_size_);
    descMasks.resize((size_t)cap * desc_size_);
    int32_t n = 0;
    check(mcs_extract(h_, image, stride, mask, mask_stride, kps.data(), cap, &n, desc.data(),
                      descMasks.data()),
          "mcs_extract");
    kps.resize(n);
    desc.resize((size_t)n * desc_size_);
    descMasks.resize((size_t)n * desc_size_);
  }

  int GetLevels() const { return nlevels_; }
  double GetScaleFactor() const { return (double)scale_factor_; }
  bool GetMasksLearned() const { return learn_masks_; }   // mdBRIEFextractorOct.h:367
  int GetDescriptorSize() const { return desc_size_; }
  mcs_extractor* handle() { return h_; }

 private:
  mcs_extractor* h_ = nullptr;
  int desc_size_ = 32, nlevels_ = 8;
  float scale_factor_ = 1.2f;
  bool do_dbrief_ = false, learn_masks_ = false, cam_set_ = false;
  mcs_cam_model cam_{};
};

inline int DescriptorDistance64(const uint64_t* d1, const uint64_t* d2, const int& dim) {
  return mcs_descriptor_distance64(d1, d2, dim);
}
inline int DescriptorDistance64Masked(const uint64_t* d1, const uint64_t* d2, const uint64_t* m1,
                                      const uint64_t* m2, const int& dim) {
  return mcs_descriptor_distance64_masked(d1, d2, m1, m2, dim);
}

// LocalBundleAdjustment after the host has collected local/fixed keyframes and observations
// (src/cOptimizer.cpp:503-769) into an mcs_ba_problem.
class LocalBA {
 public:
  explicit LocalBA(int device = 0) { check(mcs_ba_create(device, &c_), "mcs_ba_create"); }
  ~LocalBA() { mcs_ba_destroy(c_); }
  LocalBA(const LocalBA&) = delete;
  LocalBA& operator=(const LocalBA&) = delete;

  struct Result {
    std::vector<double> poses, points;
    std::vector<uint8_t> edge_inlier;
    bool write_back = false;
    mcs_ba_report round1{}, round2{};
  };

  Result run(const mcs_ba_problem& p, volatile int32_t* pbStopFlag) {
    Result r;
    r.poses.assign(p.poses, p.poses + 6 * (size_t)p.n_poses);
    r.points.assign(p.points, p.points + 3 * (size_t)p.n_points);
    r.edge_inlier.assign(p.n_edges, 1);
    int32_t wb = 0;
    check(mcs_local_ba(c_, &p, r.poses.data(), r.points.data(), r.edge_inlier.data(), &wb,
                       pbStopFlag, &r.round1, &r.round2),
          "mcs_local_ba");
    r.write_back = wb != 0;
    return r;
  }

 private:
  mcs_ba_ctx* c_ = nullptr;
};


// cOptimizer::BundleAdjustment (src/cOptimizer.cpp:73-261): the keyframe / map-point lists of
// GlobalBundleAdjustment (pMap->GetAllKeyFrames(), GetAllMapPoints(), :64-68) as flat arrays,
// graph assembly by mcs_global_ba_select (vertex ids, maxKF rule, bad skips), one optimize(15)
// by mcs_global_ba, and the write-back of :240-259 through the select's slots.
class GlobalBA {
 public:
  explicit GlobalBA(int device = 0) { check(mcs_ba_create(device, &c_), "mcs_ba_create"); }
  ~GlobalBA() { mcs_ba_destroy(c_); }
  GlobalBA(const GlobalBA&) = delete;
  GlobalBA& operator=(const GlobalBA&) = delete;

  struct Map {
    std::vector<int64_t> kf_id;       // vpKFs: mnId
    std::vector<uint8_t> kf_bad;      //        isBad()
    std::vector<double> kf_pose;      //        [n_kf][6] hom2cayley(GetPose())
    std::vector<int64_t> pt_id;       // vpMP:  mnId
    std::vector<uint8_t> pt_bad;      //        isBad()
    std::vector<double> pt_pos;       //        [n_points][3] GetWorldPos()
    std::vector<int32_t> pt_obs_off;  // [n_points + 1]: GetObservations() in std::map order
    std::vector<int32_t> obs_kf;      // vpKFs index of the observing keyframe
    std::vector<int32_t> obs_cam;     // keypoint_to_cam[obsIdx]
    std::vector<double> obs_meas;     // [n_obs][2] GetKeyPoint(obsIdx).pt
    std::vector<double> mc;           // [n_cams][6] vpKFs[0]->camSystem.Get_M_c_min(c)
    std::vector<double> cam;          // [n_cams][17] GetCamModelObj(c).toVector()
  };
  struct Result {
    std::vector<double> kf_pose, pt_pos;      // the lists' poses / positions after the write-back
    std::vector<uint8_t> kf_written, pt_written;
    mcs_ba_report report{};
  };

  // Throws on an id collision (g2o's addVertex FATAL) or any other error.
  Result run(const Map& m, bool poseOnly, volatile int32_t* pbStopFlag = nullptr) {
    const int nk = (int)m.kf_id.size(), np = (int)m.pt_id.size(), nc = (int)m.mc.size() / 6;
    mcs_gba_map gm{nk, m.kf_id.data(), m.kf_bad.data(), np, m.pt_id.data(), m.pt_bad.data(),
                   m.pt_obs_off.data(), m.obs_kf.data(), nc};
    const int nobs = (int)m.obs_kf.size();
    std::vector<int32_t> pose_kf(nk), points(np), kf_slot(nk), pt_slot(np), eo(nobs), ep(nobs), eq(nobs);
    std::vector<uint8_t> pose_fixed(nk);
    mcs_gba_graph g{pose_kf.data(), pose_fixed.data(), 0, points.data(), nullptr, 0, -1, -1,
                    kf_slot.data(), pt_slot.data(), eo.data(), ep.data(), eq.data(), 0, nobs, -1};
    check(mcs_global_ba_select(&gm, &g), "mcs_global_ba_select");
    std::vector<double> poses(6 * (size_t)g.n_poses), pts(3 * (size_t)g.n_points), meas(2 * (size_t)g.n_edges);
    std::vector<int32_t> ecam(g.n_edges);
    std::vector<double> info(g.n_edges, 1.0);                       // Identity (:209)
    for (int i = 0; i < g.n_poses; i++) std::memcpy(&poses[6 * i], &m.kf_pose[6 * (size_t)pose_kf[i]], 48);
    for (int i = 0; i < g.n_points; i++) std::memcpy(&pts[3 * i], &m.pt_pos[3 * (size_t)points[i]], 24);
    for (int e = 0; e < g.n_edges; e++) {
      ecam[e] = m.obs_cam[eo[e]];
      meas[2 * e] = m.obs_meas[2 * (size_t)eo[e]];
      meas[2 * e + 1] = m.obs_meas[2 * (size_t)eo[e] + 1];
    }
    mcs_ba_problem p{g.n_poses, g.n_points, g.n_edges, nc, poses.data(), pose_fixed.data(), pts.data(),
                     m.mc.data(), m.cam.data(), ep.data(), eq.data(), ecam.data(), meas.data(), info.data(),
                     std::sqrt(5.991)};                             // thHuber (:161)
    Result r;
    check(mcs_global_ba(c_, &p, poseOnly ? 1 : 0, poses.data(), pts.data(), pbStopFlag, &r.report, nullptr),
          "mcs_global_ba");
    r.kf_pose = m.kf_pose;
    r.pt_pos = m.pt_pos;
    r.kf_written.assign(nk, 0);
    r.pt_written.assign(np, 0);
    for (int i = 0; i < nk; i++)
      if (kf_slot[i] >= 0) { std::memcpy(&r.kf_pose[6 * (size_t)i], &poses[6 * (size_t)kf_slot[i]], 48); r.kf_written[i] = 1; }
    for (int i = 0; i < np; i++)
      if (pt_slot[i] >= 0) { std::memcpy(&r.pt_pos[3 * (size_t)i], &pts[3 * (size_t)pt_slot[i]], 24); r.pt_written[i] = 1; }
    return r;
  }

 private:
  mcs_ba_ctx* c_ = nullptr;
};

// cOptimizer::PoseOptimization(pFrame, inliers, huberMultiplier) (src/cOptimizer.cpp:264-486):
// the frame's map-point matches as indices, graph assembly by mcs_pose_optimization_select,
// both rounds and the outlier classification by mcs_pose_optimization.
class PoseOptimizer {
 public:
  explicit PoseOptimizer(int device = 0) { check(mcs_ba_create(device, &c_), "mcs_ba_create"); }
  ~PoseOptimizer() { mcs_ba_destroy(c_); }
  PoseOptimizer(const PoseOptimizer&) = delete;
  PoseOptimizer& operator=(const PoseOptimizer&) = delete;

  struct Frame {
    std::vector<int32_t> key_mp;      // mvpMapPoints[i]: index into pt_id / pt_pos, -1 = NULL
    std::vector<int32_t> key_cam;     // keypoint_to_cam[i]
    std::vector<double> key_pt;       // [N][2] mvKeys[i].pt
    std::vector<int32_t> key_octave;  // mvKeys[i].octave
    std::vector<double> inv_level_sigma2;   // mvInvLevelSigma2
    std::vector<int64_t> pt_id;       // map points: mnId
    std::vector<double> pt_pos;       //             [n][3] GetWorldPos()
    std::vector<double> pose;         // [6] GetPoseMin()
    std::vector<double> mc, cam;      // camSystem: [n_cams][6], [n_cams][17]
  };
  struct Result {
    int n_good = 0;                   // the reference's return value
    double inliers = 0.0;             // its `inliers` output (nBad / nInitialCorrespondences)
    std::vector<uint8_t> outlier;     // mvbOutlier
    std::vector<double> pose;         // Set_M_t_from_min
    mcs_ba_report round1{}, round2{};
  };

  Result run(const Frame& f, double huberMultiplier = 2) {
    const int N = (int)f.key_mp.size(), nmp = (int)f.pt_id.size(), nc = (int)f.mc.size() / 6;
    mcs_po_frame pf{N, f.key_mp.data(), nmp, f.pt_id.data(), nc};
    std::vector<int32_t> points(nmp), eo(N), eq(N);
    mcs_po_graph g{points.data(), nullptr, 0, eo.data(), eq.data(), 0, N};
    check(mcs_pose_optimization_select(&pf, &g), "mcs_pose_optimization_select");
    std::vector<double> pts(3 * (size_t)g.n_points), meas(2 * (size_t)g.n_edges), info(g.n_edges);
    std::vector<int32_t> ecam(g.n_edges), epose(g.n_edges, 0);
    for (int i = 0; i < g.n_points; i++) std::memcpy(&pts[3 * i], &f.pt_pos[3 * (size_t)points[i]], 24);
    for (int e = 0; e < g.n_edges; e++) {
      const int k = eo[e];
      ecam[e] = f.key_cam[k];
      meas[2 * e] = f.key_pt[2 * (size_t)k];
      meas[2 * e + 1] = f.key_pt[2 * (size_t)k + 1];
      info[e] = f.inv_level_sigma2[f.key_octave[k]];               // :405-406
    }
    const uint8_t not_fixed = 0;
    mcs_ba_problem p{1, g.n_points, g.n_edges, nc, f.pose.data(), &not_fixed, pts.data(), f.mc.data(),
                     f.cam.data(), epose.data(), eq.data(), ecam.data(), meas.data(), info.data(),
                     1.345 * huberMultiplier};                     // :344
    Result r;
    r.pose = f.pose;
    std::vector<uint8_t> eout(std::max(1, g.n_edges));
    int32_t good = 0;
    check(mcs_pose_optimization(c_, &p, r.pose.data(), eout.data(), &good, &r.inliers, &r.round1, &r.round2),
          "mcs_pose_optimization");
    r.n_good = good;
    r.outlier.assign(N, 0);                                        // :367
    for (int e = 0; e < g.n_edges; e++) r.outlier[eo[e]] = eout[e];
    return r;
  }

 private:
  mcs_ba_ctx* c_ = nullptr;
};

// cORBmatcher::SearchByBoW, both overloads (src/cORBmatcher.cpp:179-323, :885-966), one frame
// against a batch of candidates in one call.  A BowFrame is a frame or keyframe as flat arrays.
struct BowFrame {
  std::vector<uint8_t> desc;        // [n][bytes] descriptors in keypoint (camera-concatenated) order
  std::vector<uint8_t> mask;        // empty, or [n][bytes] mdBRIEF masks
  std::vector<float> angle;         // mvKeys[i].angle (read with checkOrientation only)
  std::vector<uint8_t> has_mp;      // GetMapPointMatches()[i] && !isBad()
  std::vector<uint32_t> fv_node;    // mFeatVec: node ids ascending,
  std::vector<int32_t> fv_ptr;      //   fv_feat[fv_ptr[j] .. fv_ptr[j + 1]) = features of node j
  std::vector<uint32_t> fv_feat;    //   (mcs_vocab_transform's output)
};

namespace detail {
struct BowPacked {
  std::vector<int32_t> off, fv_ptr, fv_n;
  std::vector<uint8_t> desc, mask, has_mp;
  std::vector<float> angle;
  std::vector<uint32_t> fv_node, fv_feat;
  mcs_bow_set set{};
};
inline void bow_pack(const BowFrame* const* frames, int n_frames, int bytes, bool fv, BowPacked& p) {
  p.off.assign(1, 0);
  for (int k = 0; k < n_frames; k++) p.off.push_back(p.off.back() + (int32_t)(frames[k]->desc.size() / bytes));
  const size_t tot = (size_t)p.off.back();
  const bool masked = n_frames > 0 && !frames[0]->mask.empty();
  p.desc.assign(tot * bytes, 0); p.has_mp.assign(tot, 0); p.angle.assign(tot, 0.f);
  if (masked) p.mask.assign(tot * bytes, 0);
  p.fv_node.assign(tot, 0); p.fv_feat.assign(tot, 0); p.fv_ptr.assign(tot + n_frames, 0); p.fv_n.assign(n_frames, 0);
  for (int k = 0; k < n_frames; k++) {
    const BowFrame& f = *frames[k];
    const size_t o = (size_t)p.off[k], n = (size_t)(p.off[k + 1] - p.off[k]);
    if (masked != !f.mask.empty()) throw std::invalid_argument("SearchByBoW: masks for every frame or none");
    if (n) std::memcpy(&p.desc[o * bytes], f.desc.data(), n * bytes);
    if (masked && n) std::memcpy(&p.mask[o * bytes], f.mask.data(), n * bytes);
    for (size_t i = 0; i < n && i < f.has_mp.size(); i++) p.has_mp[o + i] = f.has_mp[i];
    for (size_t i = 0; i < n && i < f.angle.size(); i++) p.angle[o + i] = f.angle[i];
    if (!fv) continue;
    const size_t m = f.fv_node.size();
    if (m > n || f.fv_feat.size() > n || (m && f.fv_ptr.size() != m + 1))
      throw std::invalid_argument("SearchByBoW: FeatureVector larger than its frame");
    p.fv_n[k] = (int32_t)m;
    for (size_t j = 0; j < m; j++) p.fv_node[o + j] = f.fv_node[j];
    for (size_t j = 0; j < f.fv_ptr.size(); j++) p.fv_ptr[o + k + j] = f.fv_ptr[j];
    for (size_t j = 0; j < f.fv_feat.size(); j++) p.fv_feat[o + j] = f.fv_feat[j];
  }
  p.set = mcs_bow_set{n_frames, (int32_t)tot, p.off.data(), p.desc.data(), masked ? p.mask.data() : nullptr,
                      p.angle.data(), p.has_mp.data(), p.fv_node.data(), p.fv_ptr.data(), p.fv_feat.data(),
                      p.fv_n.data()};
}
}  // namespace detail

// SearchByBoW(pKF, F, vpMapPointMatches) for every candidate keyframe of Relocalisation's loop
// (src/cTracking.cpp:1191-1203).  match_f[k][i] = keypoint of kfs[k] whose map point F's
// keypoint i received (the caller sets vpMapPointMatches[i] = kfs[k]->GetMapPoint(that)), -1 =
// NULL.  Returns nmatches per candidate.  th_low = matcher's TH_LOW_ (2 * bytes, or bytes with
// masks), nnratio / checkOrientation as given to the cORBmatcher ctor.
inline std::vector<int> SearchByBoW(const BowFrame& F, const std::vector<const BowFrame*>& kfs, int bytes,
                                    int th_low, double nnratio, bool checkOrientation,
                                    std::vector<std::vector<int32_t>>& match_f, int device = 0) {
  detail::BowPacked pf, pk;
  const BowFrame* fp = &F;
  detail::bow_pack(&fp, 1, bytes, true, pf);
  detail::bow_pack(kfs.data(), (int)kfs.size(), bytes, true, pk);
  const size_t nf = (size_t)pf.set.n_kp_total;
  std::vector<int32_t> m(kfs.size() * nf + 1), n(kfs.size() + 1);
  check(mcs_search_by_bow(device, &pf.set, &pk.set, bytes, th_low, nnratio, checkOrientation ? 1 : 0, m.data(),
                          n.data()), "mcs_search_by_bow");
  match_f.assign(kfs.size(), std::vector<int32_t>());
  for (size_t k = 0; k < kfs.size(); k++) match_f[k].assign(m.begin() + k * nf, m.begin() + (k + 1) * nf);
  return std::vector<int>(n.begin(), n.begin() + kfs.size());
}

// SearchByBoW(pKF1, pKF2, vpMatches12) for every loop candidate of ComputeSim3
// (src/cLoopClosing.cpp:285-304).  matches12[k][i1] = keypoint of kf2s[k] (vpMatches12[i1] =
// its map point), -1 = NULL.
inline std::vector<int> SearchByBoW(const BowFrame& KF1, const std::vector<const BowFrame*>& kf2s, int bytes,
                                    int th_low, double nnratio,
                                    std::vector<std::vector<int32_t>>& matches12, int device = 0) {
  detail::BowPacked p1, p2;
  const BowFrame* fp = &KF1;
  detail::bow_pack(&fp, 1, bytes, false, p1);
  detail::bow_pack(kf2s.data(), (int)kf2s.size(), bytes, false, p2);
  const size_t n1 = (size_t)p1.set.n_kp_total;
  std::vector<int32_t> m(kf2s.size() * n1 + 1), n(kf2s.size() + 1);
  check(mcs_search_by_bow_kf(device, &p1.set, &p2.set, bytes, th_low, nnratio, m.data(), n.data()),
        "mcs_search_by_bow_kf");
  matches12.assign(kf2s.size(), std::vector<int32_t>());
  for (size_t k = 0; k < kf2s.size(); k++) matches12[k].assign(m.begin() + k * n1, m.begin() + (k + 1) * n1);
  return std::vector<int>(n.begin(), n.begin() + kf2s.size());
}

// cORBmatcher::Fuse, the three overloads (src/cORBmatcher.cpp:1265-1418 rule 0, :1420-1567 rule 1,
// :1570-1719 rule 2): one set of map points against a batch of target keyframes.  The device does
// the projection / window / best-distance part for all targets in one call (mcs_fuse); the tails
// run target by target on the host (mcs_fuse_select) against the caller's map, reached through
// the FuseMap callbacks.
struct FuseRig {                    // what all keyframes of the rig share
  int n_cams = 0, mirror_w = 0, mirror_h = 0;
  std::vector<double> m_c;          // [n_cams][16] M_c row-major
  std::vector<double> cam;          // [n_cams][17] c d e u0 v0 invP[12]
  std::vector<uint8_t> mirror;      // [n_cams][mirror_h][mirror_w] mirrorMasks[0]
  std::vector<double> grid_params;  // [n_cams][4] mnMinX mnMinY mfGridElementWidthInv ...HeightInv
  std::vector<double> scale;        // mvScaleFactors
};
struct FuseKeyFrame {               // a target keyframe as flat arrays
  std::vector<float> kp_xy;         // [n][2] mvKeys pt
  std::vector<int32_t> kp_octave, kp_cam;
  std::vector<uint8_t> desc, mask;  // [n][bytes]; mask empty or mdBRIEF masks
  std::vector<double> rays;         // [n][3] GetKeyPointRay (rule 0)
  double m_t[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // Get_M_t(); rule 2: FuseSim3ToMt(Scw)
};
struct FusePoints {                 // the query map points (vpMapPoints / vpPoints)
  std::vector<int32_t> mp;          // map-point id per query, -1 = NULL
  std::vector<double> pos, dist;    // [nq][3] GetWorldPos, [nq][2] mfMinDistance mfMaxDistance
  std::vector<uint8_t> desc, mask;  // [nq][bytes]
  std::vector<double> rays;         // rule 0: [nq][3] curKF->GetKeyPointRay(i)
  double cur_m_t[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // rule 0: curKF Get_M_t()
};
struct FuseAction { int32_t kind, query, keypoint, other; };   // mcs_fuse_select's action rows
struct FuseMap {
  int n_mp = 0;
  // the state of target t as mcs_fuse_select takes it: isBad per map point, IsInKeyFrame(target)
  // per map point, the target's mvpMapPoints as ids
  virtual void state(int t, std::vector<uint8_t>& mp_bad, std::vector<uint8_t>& mp_in_kf,
                     std::vector<int32_t>& kp_mp) = 0;
  // after target t's tail: the updated state and the ordered actions, to replay onto the map
  // (AddObservation + AddMapPoint, Replace with its effect on the other keyframes)
  virtual void apply(int t, const std::vector<FuseAction>& actions, const std::vector<uint8_t>& mp_bad,
                     const std::vector<uint8_t>& mp_in_kf, const std::vector<int32_t>& kp_mp) = 0;
  // the descriptor (and mask) of map point mp after ComputeDistinctiveDescriptors
  // (src/cMapPoint.cpp:244), written into the query's rows
  virtual void descriptor(int mp, uint8_t* desc, uint8_t* mask) = 0;
  virtual ~FuseMap() {}
};

// Rule 2's pose from Scw (:1576-1585): M_t = invMat(Rt2Hom(sRcw / s, tcw / s)), the reference's
// operation order (dot and Matx products accumulate s = 0; s += a * b in index order).
inline void FuseSim3ToMt(const double* Scw, double* Mt) {
  double dot = 0;
  for (int j = 0; j < 3; j++) dot += Scw[j] * Scw[j];
  const double inv = 1.0 / std::sqrt(dot);
  double R[9], t[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[3 * i + j] = Scw[4 * i + j] * inv;
    t[i] = Scw[4 * i + 3] * inv;
  }
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int k = 0; k < 3; k++) {
      Mt[4 * i + k] = R[3 * k + i];
      s += (R[3 * k + i] * -1.0) * t[k];
    }
    Mt[4 * i + 3] = s;
  }
  Mt[12] = Mt[13] = Mt[14] = 0.0;
  Mt[15] = 1.0;
}

// Returns nFused per target.  When a Replace survivor is itself a query its descriptor changes
// (batch contract of include/mcs_matcher.h): its rows are refreshed through map.descriptor and
// the remaining targets are run again.  th: 2.5 (rule 0 in SearchInNeighbors), 3.0 (rule 1) or
// the caller's; th_low = the matcher's TH_LOW_.
inline std::vector<int> Fuse(int rule, const FuseRig& rig, const std::vector<const FuseKeyFrame*>& targets,
                             FusePoints& pts, int bytes, double th, int th_low, FuseMap& map, int flags = 0,
                             int device = 0) {
  const int T = (int)targets.size(), C = rig.n_cams, nq = (int)pts.mp.size();
  std::vector<int> n_fused(T, 0);
  const bool masked = !pts.mask.empty();
  std::vector<uint8_t> bad, in_kf;
  std::vector<int32_t> kp_mp;
  for (int t0 = 0; t0 < T;) {
    const int nt = T - t0;
    std::vector<int32_t> off(1, 0), oct, cam;
    std::vector<float> xy;
    std::vector<uint8_t> desc, mask, skip((size_t)nt * nq, 0);
    std::vector<double> rays, m_t;
    for (int t = t0; t < T; t++) {
      const FuseKeyFrame& k = *targets[t];
      if (masked != !k.mask.empty()) throw std::invalid_argument("Fuse: masks for the points and every keyframe or none");
      off.push_back(off.back() + (int32_t)k.kp_octave.size());
      xy.insert(xy.end(), k.kp_xy.begin(), k.kp_xy.end());
      oct.insert(oct.end(), k.kp_octave.begin(), k.kp_octave.end());
      cam.insert(cam.end(), k.kp_cam.begin(), k.kp_cam.end());
      desc.insert(desc.end(), k.desc.begin(), k.desc.end());
      mask.insert(mask.end(), k.mask.begin(), k.mask.end());
      rays.insert(rays.end(), k.rays.begin(), k.rays.end());
      m_t.insert(m_t.end(), k.m_t, k.m_t + 16);
      map.state(t, bad, in_kf, kp_mp);   // the skip snapshot: these conditions only grow
      std::vector<uint8_t> found;
      if (rule == 2) {
        found.assign(map.n_mp, 0);
        for (int32_t m : kp_mp) if (m >= 0 && !bad[m]) found[m] = 1;
      }
      for (int i = 0; i < nq; i++) {
        const int m = pts.mp[i];
        skip[(size_t)(t - t0) * nq + i] = m < 0 || bad[m] || (rule == 2 ? found[m] : in_kf[m]);
      }
    }
    mcs_fuse_targets tg{nt, off.back(), C, bytes, (int32_t)rig.scale.size(), rig.mirror_w, rig.mirror_h,
                        off.data(), xy.data(), oct.data(), cam.data(), desc.data(),
                        masked ? mask.data() : nullptr, rule == 0 ? rays.data() : nullptr, m_t.data(),
                        rig.m_c.data(), rig.cam.data(), rig.mirror.data(), rig.grid_params.data(),
                        rig.scale.data(), nullptr, nullptr};
    mcs_fuse_queries q{nq, pts.pos.data(), pts.dist.data(), pts.desc.data(), masked ? pts.mask.data() : nullptr,
                       rule == 0 ? pts.rays.data() : nullptr, rule == 0 ? pts.cur_m_t : nullptr};
    const size_t per = (size_t)nq * C;
    std::vector<int32_t> bk(nt * per + 1), bd(nt * per + 1), req(nq + 1);
    std::vector<uint8_t> ep(nt * per + 1);
    check(mcs_fuse(device, rule, flags, &tg, &q, th, th_low, skip.data(), bk.data(), bd.data(), ep.data()), "mcs_fuse");
    int next = T;
    for (int t = t0; t < T; t++) {
      map.state(t, bad, in_kf, kp_mp);
      std::vector<FuseAction> act(per + 1);
      int32_t na = 0, nf = 0, nr = 0;
      check(mcs_fuse_select(rule, nq, C, pts.mp.data(), bk.data() + (t - t0) * per, ep.data() + (t - t0) * per,
                            map.n_mp, bad.data(), in_kf.data(), (int32_t)kp_mp.size(), kp_mp.data(),
                            &act[0].kind, (int32_t)per, &na, &nf, req.data(), &nr), "mcs_fuse_select");
      act.resize(na);
      n_fused[t] = nf;
      map.apply(t, act, bad, in_kf, kp_mp);
      if (nr > 0 && t + 1 < T) {   // refresh the survivors' rows, run the remaining targets again
        for (int r = 0; r < nr; r++)
          for (int i = 0; i < nq; i++)
            if (pts.mp[i] == req[r])
              map.descriptor(req[r], &pts.desc[(size_t)i * bytes], masked ? &pts.mask[(size_t)i * bytes] : nullptr);
        next = t + 1;
        break;
      }
    }
    t0 = next;
  }
  return n_fused;
}

// cORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/cORBmatcher.cpp:67-166) at
// cTracking::SearchReferencePointsInFrustum (src/cTracking.cpp:961-1017) and
// SearchByProjection(CurrentFrame, LastFrame, th) (:1991-2123) at TrackWithMotionModel, on the
// host-buffer entries of the device form (mcs_track_queries_*, mcs_track_search): queries, grid,
// candidates and the ordered selection all run on the device.  A frame is a FuseKeyFrame (its
// keypoints and descriptors) with its mvpMapPoints as ids.
struct TrackFrame {
  const FuseKeyFrame* keys = nullptr;
  std::vector<int32_t> map_point;   // [n] mvpMapPoints as map-point ids, -1 = NULL (in / out)
  double pose[6] = {0, 0, 0, 0, 0, 0};   // M_t in its minimal form: Cayley rotation, translation
};
struct TrackMapPoints {             // vpMapPoints after isInFrustum ran on each of them
  std::vector<int32_t> mp;          // [n] map-point id
  std::vector<uint8_t> skip;        // [n] isBad(), or mnLastFrameSeen == the frame (already matched)
  std::vector<uint8_t> in_view;     // [n][n_cams] mbTrackInView
  std::vector<double> proj;         // [n][n_cams][2] mTrackProjX / Y
  std::vector<int32_t> level;       // [n][n_cams] mnTrackScaleLevel
  std::vector<double> view_cos;     // [n][n_cams] mTrackViewCos
  std::vector<uint8_t> desc, mask;  // [n][bytes] GetDescriptor (+ mask)
};
struct TrackLastPoints {            // the last frame's slots as :2006-2018 read them
  std::vector<uint8_t> valid;       // [n] has a point, not isBad(), not mvbOutlier
  std::vector<double> pos;          // [n][3] GetWorldPos (any value where not valid)
};

namespace detail {
inline mcs_window_frame track_window_frame(const FuseRig& rig, const FuseKeyFrame& k, int bytes) {
  return mcs_window_frame{rig.n_cams, (int32_t)k.kp_octave.size(), bytes, rig.grid_params.data(),
                          k.kp_xy.data(), k.kp_cam.data(), k.kp_octave.data(), k.desc.data(),
                          k.mask.empty() ? nullptr : k.mask.data()};
}
// runs the search and writes mvpMapPoints[bestIdx] = the query's point; id_of(query) names it
template <class IdOf>
inline int track_search(int device, int rule, const FuseRig& rig, TrackFrame& F, int bytes,
                        const std::vector<double>& q_xyr, const std::vector<int32_t>& q_cl,
                        const std::vector<int32_t>& q_idx, const std::vector<uint8_t>& src,
                        const std::vector<uint8_t>& src_mask, int th_high, double nnratio, IdOf id_of) {
  const int n = (int)F.keys->kp_octave.size(), nq = (int)q_idx.size();
  if ((int)F.map_point.size() != n) throw std::runtime_error("SearchByProjection: map_point size");
  const mcs_window_frame wf = track_window_frame(rig, *F.keys, bytes);
  const mcs_track_queries q{nq, (int32_t)(src.size() / (size_t)bytes), q_xyr.data(), q_cl.data(), q_idx.data(),
                            src.data(), src_mask.empty() ? nullptr : src_mask.data()};
  std::vector<uint8_t> assigned((size_t)std::max(1, n), 0);
  for (int i = 0; i < n; i++) assigned[i] = F.map_point[i] >= 0;
  std::vector<int32_t> match((size_t)std::max(1, nq)), kp_query((size_t)std::max(1, n));
  int32_t nm = 0;
  check(mcs_track_search(device, rule, &wf, &q, th_high, nnratio, assigned.data(), match.data(), kp_query.data(),
                         &nm), "mcs_track_search");
  for (int i = 0; i < n; i++)
    if (kp_query[i] >= 0) F.map_point[i] = id_of(kp_query[i]);
  return nm;
}
}  // namespace detail

// th_high = the matcher's TH_HIGH_ (3 * bytes, or floor(1.5 * bytes) with masks), nnratio its
// mfNNratio.  Returns nmatches; F.map_point receives the matched points.
inline int SearchByProjection(const FuseRig& rig, TrackFrame& F, const TrackMapPoints& mps, double th, int bytes,
                              int th_high, double nnratio, int device = 0) {
  const int n = (int)mps.mp.size(), C = rig.n_cams;
  const size_t nq = (size_t)n * C;
  std::vector<double> q_xyr(3 * nq + 1);
  std::vector<int32_t> q_cl(3 * nq + 1), q_idx(nq);
  check(mcs_track_queries_mappoints(device, mps.in_view.data(), mps.proj.data(), mps.level.data(),
                                    mps.view_cos.data(), mps.skip.empty() ? nullptr : mps.skip.data(), n, C,
                                    rig.scale.data(), (int32_t)rig.scale.size(), th, q_xyr.data(), q_cl.data(),
                                    q_idx.data()), "mcs_track_queries_mappoints");
  return detail::track_search(device, 0, rig, F, bytes, q_xyr, q_cl, q_idx, mps.desc, mps.mask, th_high, nnratio,
                              [&](int q) { return mps.mp[(size_t)q / C]; });
}

// mc6 [n_cams][6]: M_c of every camera in the same minimal form as the pose.  last_mp = the last
// frame's mvpMapPoints ids; Current.map_point receives them.
inline int SearchByProjection(const FuseRig& rig, const std::vector<double>& mc6, TrackFrame& Current,
                              const TrackFrame& Last, const TrackLastPoints& last_pts, double th, int bytes,
                              int th_high, double nnratio, int device = 0) {
  const FuseKeyFrame& L = *Last.keys;
  const int n = (int)L.kp_octave.size();
  std::vector<double> q_xyr(3 * (size_t)n + 1);
  std::vector<int32_t> q_cl(3 * (size_t)n + 1), q_idx((size_t)n);
  check(mcs_track_queries_lastframe(device, Current.pose, mc6.data(), rig.cam.data(), rig.n_cams, rig.mirror.data(),
                                    rig.mirror_w, rig.mirror_h, last_pts.pos.data(), last_pts.valid.data(),
                                    L.kp_cam.data(), L.kp_octave.data(), n, rig.scale.data(),
                                    (int32_t)rig.scale.size(), th, q_xyr.data(), q_cl.data(), q_idx.data()),
        "mcs_track_queries_lastframe");
  return detail::track_search(device, 1, rig, Current, bytes, q_xyr, q_cl, q_idx, L.desc, L.mask, th_high, nnratio,
                              [&](int q) { return Last.map_point[(size_t)q]; });
}

// cORBmatcher::SearchBySim3 (src/cORBmatcher.cpp:1721-1988) at cLoopClosing::ComputeSim3
// (src/cLoopClosing.cpp:369): the current keyframe against every loop candidate whose RANSAC has
// returned a Sim3, in one device call (mcs_search_by_sim3).  There is no host tail.
struct Sim3KeyFrame {               // a keyframe and the map points in its keypoint slots
  const FuseKeyFrame* kf = nullptr;
  std::vector<uint8_t> has_mp, bad; // [n] GetMapPointMatches()[i] != NULL, ->isBad()
  std::vector<double> pos, dist;    // [n][3] GetWorldPos, [n][2] mfMinDistance mfMaxDistance
  std::vector<uint8_t> desc, mask;  // [n][bytes] GetDescriptorPtr / GetDescriptorMaskPtr (the point's, not the row's)
};
struct Sim3Candidate {
  Sim3KeyFrame kf2;
  double s12 = 1.0, R12[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t12[3] = {0, 0, 0};
  std::vector<int32_t> matches12;   // in / out [n1]: vpMatches12 as a keypoint of kf2 (its map point), -1 = NULL
  // [n1] (int)vpMatches12[i]->GetIndexInKeyFrame(pKF2)[0]: the FIRST keypoint of kf2 the point
  // observes, -1 when it observes none (src/cMapPoint.cpp:436-445); read where matches12[i] >= 0
  std::vector<int32_t> first_idx_in_kf2;
};

// vbAlreadyMatched1 / 2 exactly as :1758-1774 build them (only the first index of a matched
// point, and only when it lies in [0, N2)), then the conditions under which the two loops take a
// slot (:1784-1788, :1878-1882): a point, not already matched, not bad.
inline void Sim3Flags(const Sim3KeyFrame& kf1, const Sim3Candidate& c, std::vector<uint8_t>& already1,
                      std::vector<uint8_t>& already2, std::vector<uint8_t>& active1,
                      std::vector<uint8_t>& active2) {
  const int N1 = (int)kf1.has_mp.size(), N2 = (int)c.kf2.has_mp.size();
  if ((int)c.matches12.size() != N1 || (int)c.first_idx_in_kf2.size() != N1 || (int)kf1.bad.size() != N1 ||
      (int)c.kf2.bad.size() != N2)
    throw std::invalid_argument("SearchBySim3: matches12 / first_idx_in_kf2 / bad do not fit the keyframes");
  already1.assign(N1, 0); already2.assign(N2, 0);
  for (int i = 0; i < N1; i++) {
    if (c.matches12[i] < 0) continue;
    already1[i] = 1;
    const int idx2 = c.first_idx_in_kf2[i];
    if (idx2 >= 0 && idx2 < N2) already2[idx2] = 1;
  }
  active1.assign(N1, 0); active2.assign(N2, 0);
  for (int i = 0; i < N1; i++) active1[i] = kf1.has_mp[i] && !already1[i] && !kf1.bad[i];
  for (int i = 0; i < N2; i++) active2[i] = c.kf2.has_mp[i] && !already2[i] && !c.kf2.bad[i];
}

// Returns nFound per candidate and writes the new matches into each candidate's matches12
// (vpMatches12[i1] = vpMapPoints2[idx2], :1981).  th = 10 at the call site; th_high = the matcher's
// TH_HIGH_ (3 * bytes, or floor(1.5 * bytes) with masks).
inline std::vector<int> SearchBySim3(const FuseRig& rig, const Sim3KeyFrame& kf1, std::vector<Sim3Candidate>& cands,
                                     int bytes, double th, int th_high, int device = 0) {
  const int T = (int)cands.size(), C = rig.n_cams;
  if (T == 0) return {};
  if (!kf1.kf) throw std::invalid_argument("SearchBySim3: kf1 has no keyframe");
  const int n1 = (int)kf1.kf->kp_octave.size();
  const bool masked = !kf1.kf->mask.empty();
  std::vector<int32_t> off(1, 0), oct, cam;
  std::vector<float> xy;
  std::vector<uint8_t> desc, mask, pdesc, pmask, act1, act2, a1, a2, am1, am2;
  std::vector<double> m_t, pos, dist, s12, R12, t12;
  for (Sim3Candidate& c : cands) {
    if (!c.kf2.kf) throw std::invalid_argument("SearchBySim3: a candidate has no keyframe");
    const FuseKeyFrame& k = *c.kf2.kf;
    if (masked != !k.mask.empty() || masked != !c.kf2.mask.empty() || masked != !kf1.mask.empty())
      throw std::invalid_argument("SearchBySim3: masks for every keyframe and every point or none");
    Sim3Flags(kf1, c, am1, am2, a1, a2);
    act1.insert(act1.end(), a1.begin(), a1.end());
    act2.insert(act2.end(), a2.begin(), a2.end());
    off.push_back(off.back() + (int32_t)k.kp_octave.size());
    xy.insert(xy.end(), k.kp_xy.begin(), k.kp_xy.end());
    oct.insert(oct.end(), k.kp_octave.begin(), k.kp_octave.end());
    cam.insert(cam.end(), k.kp_cam.begin(), k.kp_cam.end());
    desc.insert(desc.end(), k.desc.begin(), k.desc.end());
    mask.insert(mask.end(), k.mask.begin(), k.mask.end());
    m_t.insert(m_t.end(), k.m_t, k.m_t + 16);
    pos.insert(pos.end(), c.kf2.pos.begin(), c.kf2.pos.end());
    dist.insert(dist.end(), c.kf2.dist.begin(), c.kf2.dist.end());
    pdesc.insert(pdesc.end(), c.kf2.desc.begin(), c.kf2.desc.end());
    pmask.insert(pmask.end(), c.kf2.mask.begin(), c.kf2.mask.end());
    s12.push_back(c.s12);
    R12.insert(R12.end(), c.R12, c.R12 + 9);
    t12.insert(t12.end(), c.t12, c.t12 + 3);
  }
  const int32_t L = (int32_t)rig.scale.size(), one[2] = {0, n1};
  const FuseKeyFrame& k1 = *kf1.kf;
  mcs_fuse_targets s1{1, n1, C, bytes, L, rig.mirror_w, rig.mirror_h, one, k1.kp_xy.data(), k1.kp_octave.data(),
                      k1.kp_cam.data(), k1.desc.data(), masked ? k1.mask.data() : nullptr, nullptr, k1.m_t,
                      rig.m_c.data(), rig.cam.data(), rig.mirror.data(), rig.grid_params.data(), rig.scale.data(),
                      nullptr, nullptr};
  mcs_fuse_targets s2{T, off.back(), C, bytes, L, rig.mirror_w, rig.mirror_h, off.data(), xy.data(), oct.data(),
                      cam.data(), desc.data(), masked ? mask.data() : nullptr, nullptr, m_t.data(), rig.m_c.data(),
                      rig.cam.data(), rig.mirror.data(), rig.grid_params.data(), rig.scale.data(), nullptr, nullptr};
  mcs_sim3_points p1{n1, kf1.pos.data(), kf1.dist.data(), kf1.desc.data(), masked ? kf1.mask.data() : nullptr};
  mcs_sim3_points p2{off.back(), pos.data(), dist.data(), pdesc.data(), masked ? pmask.data() : nullptr};
  std::vector<int32_t> m12((size_t)T * n1 + 1), nf(T + 1);
  check(mcs_search_by_sim3(device, &s1, &p1, &s2, &p2, act1.data(), act2.data(), s12.data(), R12.data(), t12.data(), th,
                           th_high, nullptr, nullptr, m12.data(), nf.data()), "mcs_search_by_sim3");
  for (int t = 0; t < T; t++)
    for (int i = 0; i < n1; i++)
      if (m12[(size_t)t * n1 + i] >= 0) cands[t].matches12[i] = m12[(size_t)t * n1 + i];
  return std::vector<int>(nf.begin(), nf.begin() + T);
}

// cSim3Solver (src/cSim3Solver.cpp) at cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:311-364):
// one solver per loop candidate with the reference's surface, on mcs_sim3_solver.  The solver's
// members (mnIterations, mnBestInliers, mRansacMaxIts, mvbBestInliers, mBest*) are kept between
// calls as host copies and handed to the library each time, so the 50-iterations-per-visit loop
// of ComputeSim3 works unchanged, a second iterate after a success included.  The text draws from
// std::random_device inside iterate; here the draws of all maxIterations iterations come from one
// std::mt19937 + std::uniform_int_distribution<>(0, N - 1), three per iteration in iteration
// order, through mcs_sim3_draw_samples.  With N < 3 no triple can be drawn: every sample is 0.
// The solver keeps references to rig, kf1 and kf2 (as the text keeps pKF1 / pKF2): they must outlive
// it.  Every iterate uploads the keyframes and runs the constructor's kernel again; callers that
// visit often use the device entries, which keep everything resident.
class Sim3Solver {
 public:
  // matches12 [n1]: vpMatched12 as a keypoint of kf2 (its slot's map point), -1 = NULL.
  // first1 [n1] / first2 [n2]: (int)GetIndexInKeyFrame(pKF)[0] of the slot's point, -1 when it
  // observes nothing.  sigma2: mvLevelSigma2.  camSys is KF1's rig, as at the call site.
  Sim3Solver(const FuseRig& rig, const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2,
             const std::vector<int32_t>& matches12, const std::vector<int32_t>& first1,
             const std::vector<int32_t>& first2, const std::vector<double>& sigma2,
             unsigned seed = std::random_device{}(), int device = 0)
      : rig_(rig), kf1_(kf1), kf2_(kf2), m12_(matches12), f1_(first1), f2_(first2), sigma2_(sigma2), gen_(seed),
        device_(device) {
    if (!kf1.kf || !kf2.kf) throw std::invalid_argument("Sim3Solver: a keyframe is missing");
    n1_ = (int)kf1.kf->kp_octave.size();
    n2_ = (int)kf2.kf->kp_octave.size();
    if ((int)m12_.size() != n1_ || (int)f1_.size() != n1_ || (int)f2_.size() != n2_ || (int)kf1.has_mp.size() != n1_ ||
        (int)kf1.bad.size() != n1_ || (int)kf2.bad.size() != n2_ || (int)sigma2_.size() != (int)rig.scale.size())
      throw std::invalid_argument("Sim3Solver: matches12 / first / bad / sigma2 do not fit the keyframes");
    ok1_.resize(n1_); ok2_.resize(n2_);
    for (int i = 0; i < n1_; i++) ok1_[i] = kf1.has_mp[i] && !kf1.bad[i];    // :77, :82
    for (int i = 0; i < n2_; i++) ok2_[i] = !kf2.bad[i];                      // :82
    N_ = 0;                                                                   // the skip rules of :73-98
    const int L = (int)rig.scale.size(), C = rig.n_cams;
    for (int i = 0; i < n1_; i++) {
      const int m = m12_[i];
      if (m < 0 || m >= n2_ || !ok1_[i] || !ok2_[m] || f1_[i] < 0 || f1_[i] >= n1_ || f2_[m] < 0 || f2_[m] >= n2_) continue;
      const int o1 = kf1.kf->kp_octave[f1_[i]], o2 = kf2.kf->kp_octave[f2_[m]];
      const int c1 = kf1.kf->kp_cam[f1_[i]], c2 = kf2.kf->kp_cam[f2_[m]];
      N_ += o1 >= 0 && o1 < L && o2 >= 0 && o2 < L && c1 >= 0 && c1 < C && c2 >= 0 && c2 < C;
    }
    words_.assign((size_t)(n1_ + 63) / 64 + 1, 0);
    flags_ = MCS_SIM3_INIT;
    SetRansacParameters();                                                    // :136
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    if (maxIterations < 1) throw std::invalid_argument("Sim3Solver: maxIterations must be at least 1");
    prob_ = probability; min_ = minInliers; cap_ = maxIterations;
    flags_ |= MCS_SIM3_SET_PARAMS;
    samples_.assign(3 * (size_t)cap_, 0);
    if (N_ >= 3) {
      std::uniform_int_distribution<> dis(0, N_ - 1);
      std::vector<int32_t> draws(3 * (size_t)cap_);
      for (int32_t& d : draws) d = dis(gen_);
      check(mcs_sim3_draw_samples(N_, draws.data(), cap_, samples_.data()), "mcs_sim3_draw_samples");
    }
  }

  // result: 16 doubles, row-major T12; written on a success only, as the text does
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, double* result) {
    bNoMore = false;
    vbInliers.assign(n1_, false);
    nInliers = 0;
    if (nIterations < 1) {                                                    // the loop of :196 does not run
      bNoMore = flags_ == 0 && its_ >= max_its_;
      return false;
    }
    const int32_t L = (int32_t)rig_.scale.size(), C = rig_.n_cams, one[2] = {0, n1_}, two[2] = {0, n2_};
    const FuseKeyFrame &a = *kf1_.kf, &b = *kf2_.kf;
    mcs_fuse_targets s1{1, n1_, C, 32, L, rig_.mirror_w, rig_.mirror_h, one, nullptr, a.kp_octave.data(),
                        a.kp_cam.data(), nullptr, nullptr, nullptr, a.m_t, rig_.m_c.data(), rig_.cam.data(), nullptr,
                        nullptr, nullptr, nullptr, nullptr};
    mcs_fuse_targets s2{1, n2_, C, 32, L, rig_.mirror_w, rig_.mirror_h, two, nullptr, b.kp_octave.data(),
                        b.kp_cam.data(), nullptr, nullptr, nullptr, b.m_t, rig_.m_c.data(), rig_.cam.data(), nullptr,
                        nullptr, nullptr, nullptr, nullptr};
    mcs_sim3_points p1{n1_, kf1_.pos.data(), nullptr, nullptr, nullptr}, p2{n2_, kf2_.pos.data(), nullptr, nullptr, nullptr};
    int32_t ok = 0, no_more = 0, n_inl = 0;
    std::vector<uint8_t> inl((size_t)n1_ + 1);
    mcs_sim3_ransac r{&its_, &best_, &max_its_, words_.data(), &s_, R_, t_, T_, &ok, &no_more, &n_inl, inl.data(),
                      nullptr, nullptr};
    check(mcs_sim3_solver(device_, &s1, &p1, &s2, &p2, m12_.data(), ok1_.data(), ok2_.data(), f1_.data(), f2_.data(),
                          sigma2_.data(), samples_.data(), nIterations < cap_ ? nIterations : cap_, prob_, min_, cap_,
                          flags_, nullptr, &r, nullptr, nullptr, nullptr, nullptr), "mcs_sim3_solver");
    flags_ = 0;
    bNoMore = no_more != 0;
    if (ok) {
      nInliers = n_inl;
      for (int i = 0; i < n1_; i++) vbInliers[i] = inl[i] != 0;
      if (result) std::memcpy(result, T_, sizeof(T_));
    }
    return ok != 0;
  }

  bool find(std::vector<bool>& vbInliers12, int& nInliers, double* result) {
    bool flag;
    return iterate(cap_, flag, vbInliers12, nInliers, result);               // :261: mRansacMaxIts <= maxIterations
  }

  const double* GetEstimatedRotation() const { return R_; }                   // [9] row-major
  const double* GetEstimatedTranslation() const { return t_; }                // [3]
  double GetEstimatedScale() const { return s_; }
  int N() const { return N_; }
  const std::vector<int32_t>& samples() const { return samples_; }   // [maxIterations][3], iteration k's triple
  int iterations() const { return its_; }
  int max_iterations() const { return max_its_; }

 private:
  const FuseRig& rig_;
  const Sim3KeyFrame &kf1_, &kf2_;
  std::vector<int32_t> m12_, f1_, f2_;
  std::vector<double> sigma2_;
  std::mt19937 gen_;
  int device_, n1_ = 0, n2_ = 0, N_ = 0, flags_ = 0, min_ = 6, cap_ = 300;
  double prob_ = 0.99;
  std::vector<uint8_t> ok1_, ok2_;
  std::vector<int32_t> samples_;
  std::vector<uint64_t> words_;
  int32_t its_ = 0, best_ = 0, max_its_ = 0;
  double s_ = 0, R_[9] = {0}, t_[3] = {0}, T_[16] = {0};
};

// cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:63-270) at cLoopClosing::ComputeSim3
// (src/cLoopClosing.cpp:372): int OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12), on
// mcs_optimize_sim3.  vpMatches1 [n1] (in / out): the matched point as a keypoint of kf2 (its
// slot's map point), -1 = NULL; entries the text nulls come back as -1.  first2 [n2]:
// (int)GetIndexInKeyFrame(pKF2)[0] of the slot's point.  inv_sigma2_1 / sigma2_2: KF1's
// mvInvLevelSigma2 and KF2's mvLevelSigma2 (the text weights e21 with sigma^2, :194).
// g2oS12 (in / out) is left as it was when fewer than 3 pairs survive round 1 (:240-241).
// Returns nIn.  options NULL = the reference's values; its flags select MCS_SIM3OPT_OWN_CAMERA.
struct Sim3Transform {              // g2o::Sim3(R, t, s)
  double s = 1.0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
};
inline int OptimizeSim3(const FuseRig& rig, const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2,
                        std::vector<int32_t>& vpMatches1, const std::vector<int32_t>& first2,
                        const std::vector<double>& inv_sigma2_1, const std::vector<double>& sigma2_2,
                        Sim3Transform& g2oS12, const mcs_sim3_opt_options* options = nullptr, int device = 0) {
  if (!kf1.kf || !kf2.kf) throw std::invalid_argument("OptimizeSim3: a keyframe is missing");
  const int n1 = (int)kf1.kf->kp_octave.size(), n2 = (int)kf2.kf->kp_octave.size();
  const int32_t L = (int32_t)rig.scale.size(), C = rig.n_cams, one[2] = {0, n1}, two[2] = {0, n2};
  if ((int)vpMatches1.size() != n1 || (int)first2.size() != n2 || (int)kf1.has_mp.size() != n1 ||
      (int)kf1.bad.size() != n1 || (int)kf2.bad.size() != n2 || (int)inv_sigma2_1.size() != L ||
      (int)sigma2_2.size() != L || (int)kf1.pos.size() != 3 * n1 || (int)kf2.pos.size() != 3 * n2)
    throw std::invalid_argument("OptimizeSim3: matches / first2 / bad / pos / sigma2 do not fit the keyframes");
  std::vector<uint8_t> ok1((size_t)n1 + 1), ok2((size_t)n2 + 1);
  for (int i = 0; i < n1; i++) ok1[i] = kf1.has_mp[i] && !kf1.bad[i];    // pMP1 && !pMP1->isBad() (:135-137)
  for (int i = 0; i < n2; i++) ok2[i] = !kf2.bad[i];                      // !pMP2->isBad() (:137)
  const FuseKeyFrame &a = *kf1.kf, &b = *kf2.kf;
  mcs_fuse_targets s1{1, n1, C, 32, L, rig.mirror_w, rig.mirror_h, one, a.kp_xy.data(), a.kp_octave.data(),
                      a.kp_cam.data(), nullptr, nullptr, nullptr, a.m_t, rig.m_c.data(), rig.cam.data(), nullptr,
                      nullptr, nullptr, nullptr, nullptr};
  mcs_fuse_targets s2{1, n2, C, 32, L, rig.mirror_w, rig.mirror_h, two, b.kp_xy.data(), b.kp_octave.data(),
                      b.kp_cam.data(), nullptr, nullptr, nullptr, b.m_t, rig.m_c.data(), rig.cam.data(), nullptr,
                      nullptr, nullptr, nullptr, nullptr};
  mcs_sim3_points p1{n1, kf1.pos.data(), nullptr, nullptr, nullptr}, p2{n2, kf2.pos.data(), nullptr, nullptr, nullptr};
  mcs_sim3_opt_options o;
  if (options) o = *options; else mcs_sim3_opt_default_options(&o);
  int32_t n_in = 0, n_corr = 0, n_bad = 0, n_undef = 0, iters[2];
  double s = 0, q[4], R[9], t[3], chi2[2], lambda[2];
  mcs_sim3_opt_out out{&n_in, &n_corr, &n_bad, &n_undef, &s, q, R, t, iters, chi2, lambda, nullptr, nullptr};
  std::vector<int32_t> m12(vpMatches1);
  m12.push_back(-1);
  check(mcs_optimize_sim3(device, &s1, &p1, &s2, &p2, m12.data(), ok1.data(), ok2.data(), first2.data(),
                          inv_sigma2_1.data(), sigma2_2.data(), &g2oS12.s, g2oS12.R, g2oS12.t, &o, &out),
        "mcs_optimize_sim3");
  std::copy(m12.begin(), m12.begin() + n1, vpMatches1.begin());
  g2oS12.s = s;
  std::memcpy(g2oS12.R, R, sizeof(R));
  std::memcpy(g2oS12.t, t, sizeof(t));
  return n_in;
}

// cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:273-519) at cLoopClosing::CorrectLoop
// (src/cLoopClosing.cpp:648): void OptimizeEssentialGraph(pMap, pLoopMKF, pCurMKF, Scurw,
// NonCorrectedSim3, CorrectedSim3, LoopConnections), on mcs_essgraph_select_edges and
// mcs_optimize_essential_graph over the flat map.  Keyframes in ascending mnId, none bad.
struct EssentialGraphKeyFrame {
  int64_t id = 0;                        // mnId
  double pose_inv[16] = {0};             // in: GetPoseInverse(), row-major (read when !has_corrected, :331-336)
  double pose[16] = {0};                 // out: the SetPose argument (:490)
  int32_t parent = -1;                   // GetParent() as an index into the keyframe list
  bool has_corrected = false;            // key of CorrectedSim3 / NonCorrectedSim3
  double corrected[8] = {1, 1, 0, 0, 0, 0, 0, 0};      // CorrectedSim3[kf] as s, qw qx qy qz, tx ty tz
  double non_corrected[8] = {1, 1, 0, 0, 0, 0, 0, 0};  // NonCorrectedSim3[kf]
  std::vector<int32_t> loop_edges;       // GetLoopEdges() as indices
  std::vector<int32_t> covisibles, cov_weights;         // GetCovisiblesByWeight(0) order with GetWeight
  std::vector<int32_t> loop_connections, lc_weights;    // LoopConnections[kf] with GetWeight
};
struct EssentialGraphPoints {            // GetAllMapPoints()
  std::vector<double> pos;               // [P][3] GetWorldPos(), corrected in place
  std::vector<int64_t> corrected_by, corrected_ref, ref_kf;   // mnCorrectedByKF, mnCorrectedReference, reference mnId
  std::vector<uint8_t> bad;
};
struct EssentialGraphReport {
  int32_t iterations = 0, n_edges = 0, counts[4] = {0, 0, 0, 0};
  double chi2 = 0, lambda = 0;
  bool sparse = false;                   // the block-sparse solver ran (mcs_optimize_essential_graph_sparse)
};
// Auto: the dense solver wherever it takes the map (every result it gives keeps its bits), the
// block-sparse one where it answers MCS_ERR_UNSUPPORTED (more than 878 keyframes).
enum class EssentialGraphSolver { Auto, Dense, Sparse };

inline EssentialGraphReport OptimizeEssentialGraph(std::vector<EssentialGraphKeyFrame>& kfs, EssentialGraphPoints& pts,
                                                   int loop_index, int cur_index,
                                                   const mcs_essgraph_options* options = nullptr, int device = 0,
                                                   EssentialGraphSolver solver = EssentialGraphSolver::Auto) {
  const int N = (int)kfs.size(), P = (int)pts.bad.size();
  if (N < 1 || loop_index < 0 || loop_index >= N || cur_index < 0 || cur_index >= N)
    throw std::invalid_argument("OptimizeEssentialGraph: loop / current keyframe outside the list");
  if ((int)pts.pos.size() != 3 * P || (int)pts.corrected_by.size() != P || (int)pts.corrected_ref.size() != P ||
      (int)pts.ref_kf.size() != P)
    throw std::invalid_argument("OptimizeEssentialGraph: the point arrays do not agree in length");
  std::vector<int64_t> ids(N);
  std::vector<int32_t> parent(N), lp(1, 0), li, cp(1, 0), ci, cw, kp(1, 0), ki, kw;
  std::vector<uint8_t> hc(N);
  std::vector<double> Scw(8 * (size_t)N), Snc(8 * (size_t)N);
  std::unordered_map<int64_t, int32_t> index_of;
  for (int i = 0; i < N; i++) {
    const EssentialGraphKeyFrame& k = kfs[i];
    if (k.covisibles.size() != k.cov_weights.size() || k.loop_connections.size() != k.lc_weights.size())
      throw std::invalid_argument("OptimizeEssentialGraph: neighbours and weights do not agree in length");
    ids[i] = k.id; parent[i] = k.parent; hc[i] = k.has_corrected;
    index_of[k.id] = i;
    li.insert(li.end(), k.loop_edges.begin(), k.loop_edges.end()); lp.push_back((int32_t)li.size());
    ci.insert(ci.end(), k.covisibles.begin(), k.covisibles.end());
    cw.insert(cw.end(), k.cov_weights.begin(), k.cov_weights.end()); cp.push_back((int32_t)ci.size());
    ki.insert(ki.end(), k.loop_connections.begin(), k.loop_connections.end());
    kw.insert(kw.end(), k.lc_weights.begin(), k.lc_weights.end()); kp.push_back((int32_t)ki.size());
    double* S = &Scw[8 * (size_t)i];
    if (k.has_corrected) {
      std::memcpy(S, k.corrected, sizeof(k.corrected));
      std::memcpy(&Snc[8 * (size_t)i], k.non_corrected, sizeof(k.non_corrected));
    } else {
      // g2o::Sim3(R, t, 1.0) of GetPoseInverse() (:331-336): Eigen's Quaterniond(Matrix3d)
      const double* M = k.pose_inv;
      const double m[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
      double q[4], t = m[0] + m[4] + m[8];
      if (t > 0.0) {
        t = std::sqrt(t + 1.0); q[0] = 0.5 * t; t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t;
      } else {
        int a = 0;
        if (m[4] > m[0]) a = 1;
        if (m[8] > m[4 * a]) a = 2;
        const int b = (a + 1) % 3, c = (b + 1) % 3;
        t = std::sqrt(m[4 * a] - m[4 * b] - m[4 * c] + 1.0); q[1 + a] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[3 * c + b] - m[3 * b + c]) * t;
        q[1 + b] = (m[3 * b + a] + m[3 * a + b]) * t; q[1 + c] = (m[3 * c + a] + m[3 * a + c]) * t;
      }
      S[0] = 1.0; S[1] = q[0]; S[2] = q[1]; S[3] = q[2]; S[4] = q[3]; S[5] = M[3]; S[6] = M[7]; S[7] = M[11];
      std::memcpy(&Snc[8 * (size_t)i], S, 8 * sizeof(double));
    }
  }
  mcs_essgraph_map m{N, ids.data(), parent.data(), hc.data(), lp.data(), li.data(), cp.data(), ci.data(), cw.data(),
                     kp.data(), ki.data(), kw.data(), cur_index, loop_index, 100};
  EssentialGraphReport rep;
  int32_t E = 0;
  int rc = mcs_essgraph_select_edges(&m, nullptr, 0, &E, rep.counts);
  if (rc != MCS_OK && rc != MCS_ERR_CAPACITY) check(rc, "mcs_essgraph_select_edges");
  std::vector<int32_t> edges(3 * (size_t)E + 3);
  check(mcs_essgraph_select_edges(&m, edges.data(), E, &E, rep.counts), "mcs_essgraph_select_edges");
  rep.n_edges = E;
  std::vector<int32_t> ref(P + 1);
  for (int j = 0; j < P; j++) {          // :501-507
    const int64_t id = pts.corrected_by[j] == kfs[cur_index].id ? pts.corrected_ref[j] : pts.ref_kf[j];
    auto it = index_of.find(id);
    if (it == index_of.end() && !pts.bad[j]) throw std::invalid_argument("OptimizeEssentialGraph: a point names no keyframe");
    ref[j] = it == index_of.end() ? 0 : it->second;
  }
  mcs_essgraph_options o;
  if (options) o = *options; else mcs_essgraph_default_options(&o);
  if (o.tile_band == 0) o.tile_band = mcs_essgraph_tile_band(N, loop_index, edges.data(), E);
  std::vector<double> pose(16 * (size_t)N), chi2(MCS_ESSGRAPH_MAX_ITERATIONS);
  int32_t status = 0;
  mcs_essgraph_out out{nullptr, nullptr, pose.data(), &rep.iterations, nullptr, chi2.data(), &rep.lambda, nullptr, &status};
  pts.pos.resize(3 * (size_t)P + 3);
  pts.bad.resize((size_t)P + 1);
  rep.sparse = solver == EssentialGraphSolver::Sparse ||
               (solver == EssentialGraphSolver::Auto && mcs_essgraph_supported(N, o.tile_band) == MCS_ERR_UNSUPPORTED);
  rc = (rep.sparse ? mcs_optimize_essential_graph_sparse : mcs_optimize_essential_graph)(
      device, N, Scw.data(), Snc.data(), loop_index, E, edges.data(), P, pts.pos.data(), ref.data(), pts.bad.data(), &o,
      &out);
  pts.pos.resize(3 * (size_t)P);
  pts.bad.resize((size_t)P);
  check(rc, rep.sparse ? "mcs_optimize_essential_graph_sparse" : "mcs_optimize_essential_graph");
  for (int i = 0; i < N; i++) std::memcpy(kfs[i].pose, &pose[16 * (size_t)i], 16 * sizeof(double));
  rep.chi2 = rep.iterations > 0 ? chi2[rep.iterations - 1] : 0.0;
  return rep;
}

// cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:224-386) at its call site (:99): the
// neighbour loop (SearchForTriangulationRaw, then the per-match loop :272-382) in one device call
// (mcs_create_new_map_points).  The caller does what needs the map: the neighbours
// (GetBestCovisibilityKeyFrames(5)), `skip` = the ratioBaselineDepth < 0.01 gate (:248-256) per
// neighbour, `kf2_first` = whether the neighbour precedes the current keyframe in the new point's
// std::map<cMultiKeyFrame*, ...> (pointer order: pKF2 < mpCurrentMultiKeyFrame), and afterwards
// `new cMapPoint`, AddObservation, AddMapPoint and mpMap->AddMapPoint for every returned point.
struct NewMapPoint {
  int neighbour = 0, idx1 = 0, idx2 = 0;   // index into `neighbours`, keypoint of cur, keypoint of the neighbour
  double pos[3] = {0, 0, 0}, normal[3] = {0, 0, 0}, minDist = 0, maxDist = 0;   // mWorldPos, mNormalVector, mf{Min,Max}Distance
  std::vector<uint8_t> desc, mask;         // mDescriptor, mDescriptorMask (empty without masks)
};

// has_mp [1 + T]: nonzero = the keypoint holds a map point (mvpMapPoints[i] != NULL), the current
// keyframe first; updated as AddMapPoint does (:370-371).  TH_LOW = the matcher's TH_LOW_ (2 * featDim,
// or featDim with masks); rays must be filled.  Keypoints must lie in cameras [0, n_cams).
inline std::vector<NewMapPoint> CreateNewMapPoints(const FuseRig& rig, const FuseKeyFrame& cur,
                                                   const std::vector<const FuseKeyFrame*>& neighbours,
                                                   std::vector<std::vector<uint8_t>*>& has_mp,
                                                   const std::vector<uint8_t>& skip,
                                                   const std::vector<uint8_t>& kf2_first, int featDim, int TH_LOW,
                                                   double epi_thresh = 1e-2, int device = 0) {
  const int T = (int)neighbours.size(), C = rig.n_cams;
  if ((int)skip.size() != T || (int)kf2_first.size() != T || (int)has_mp.size() != T + 1)
    throw std::invalid_argument("CreateNewMapPoints: skip, kf2_first and has_mp must fit the neighbours");
  const bool masked = !cur.mask.empty();
  std::vector<int32_t> off(1, 0), oct, cam;
  std::vector<float> xy;
  std::vector<uint8_t> desc, mask, has;
  std::vector<double> rays, m_t, E((size_t)T * C * C * 9 + 1);
  for (int t = 0; t <= T; t++) {
    const FuseKeyFrame& k = t ? *neighbours[t - 1] : cur;
    const size_t n = k.kp_octave.size();
    if (masked != !k.mask.empty() || has_mp[t]->size() != n || k.rays.size() != 3 * n)
      throw std::invalid_argument("CreateNewMapPoints: masks for every keyframe or none; has_mp and rays per keypoint");
    off.push_back(off.back() + (int32_t)n);
    xy.insert(xy.end(), k.kp_xy.begin(), k.kp_xy.end());
    oct.insert(oct.end(), k.kp_octave.begin(), k.kp_octave.end());
    cam.insert(cam.end(), k.kp_cam.begin(), k.kp_cam.end());
    desc.insert(desc.end(), k.desc.begin(), k.desc.end());
    mask.insert(mask.end(), k.mask.begin(), k.mask.end());
    rays.insert(rays.end(), k.rays.begin(), k.rays.end());
    has.insert(has.end(), has_mp[t]->begin(), has_mp[t]->end());
    m_t.insert(m_t.end(), k.m_t, k.m_t + 16);
    if (t)   // Es[i][j] of SearchForTriangulationRaw (src/cORBmatcher.cpp:985-998)
      check(mcs_compute_e_rig_hom(cur.m_t, k.m_t, rig.m_c.data(), C, &E[(size_t)(t - 1) * C * C * 9]), "mcs_compute_e_rig_hom");
  }
  mcs_fuse_targets kfs{T + 1, off.back(), C, featDim, (int32_t)rig.scale.size(), rig.mirror_w, rig.mirror_h,
                       off.data(), xy.data(), oct.data(), cam.data(), desc.data(), masked ? mask.data() : nullptr,
                       rays.data(), m_t.data(), rig.m_c.data(), rig.cam.data(), nullptr, nullptr, rig.scale.data(),
                       nullptr, nullptr};
  const size_t n1 = cur.kp_octave.size(), cap = n1 * (size_t)(T > 0 ? T : 1) + 1, nb = (size_t)featDim;
  int32_t count = 0;
  std::vector<int32_t> kp1(cap), kp2(cap), nbr(cap);
  std::vector<double> pos(3 * cap), nrm(3 * cap), dmin(cap), dmax(cap);
  std::vector<uint8_t> od(cap * nb), om(masked ? cap * nb : 1);
  mcs_new_points out{(int32_t)cap, &count, kp1.data(), kp2.data(), nbr.data(), pos.data(), nrm.data(), dmin.data(),
                     dmax.data(), od.data(), masked ? om.data() : nullptr};
  check(mcs_create_new_map_points(device, &kfs, skip.data(), kf2_first.data(), E.data(), has.data(), TH_LOW, epi_thresh,
                                  nullptr, nullptr, &out), "mcs_create_new_map_points");
  for (int t = 0; t <= T; t++) std::copy(has.begin() + off[t], has.begin() + off[t + 1], has_mp[t]->begin());
  std::vector<NewMapPoint> pts((size_t)count);
  for (int p = 0; p < count; p++) {
    NewMapPoint& q = pts[p];
    q.neighbour = nbr[p]; q.idx1 = kp1[p]; q.idx2 = kp2[p];
    for (int j = 0; j < 3; j++) { q.pos[j] = pos[3 * (size_t)p + j]; q.normal[j] = nrm[3 * (size_t)p + j]; }
    q.minDist = dmin[p]; q.maxDist = dmax[p];
    q.desc.assign(od.begin() + (size_t)p * nb, od.begin() + (size_t)(p + 1) * nb);
    if (masked) q.mask.assign(om.begin() + (size_t)p * nb, om.begin() + (size_t)(p + 1) * nb);
  }
  return pts;
}

// ---- cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp) on mcs_kfdb -----------------------
// The device database names a keyframe by its slot (the add sequence number); the caller's code
// names it by pointer.  KfSlots is that bookkeeping: pointer -> slot for every keyframe ever added
// (an erased keyframe keeps its slot: it can still be somebody's neighbour and can still be
// returned as pBestKF, as the reference's object stays alive), slot -> pointer for the results.
template <class KF>
class KfSlots {
 public:
  // the slot the next add receives
  int32_t next() const { return (int32_t)kf_.size(); }
  // records pKF at `slot` (the value mcs_kfdb_add returned); a pointer added again gets the new slot
  void bind(const KF* pKF, int32_t slot) {
    if (slot != next()) throw std::logic_error("KfSlots: slots are handed out in sequence");
    kf_.push_back(pKF);
    alive_.push_back(1);
    map_[pKF] = slot;
  }
  // -1 when pKF was never added
  int32_t slot(const KF* pKF) const {
    const auto it = map_.find(pKF);
    return it == map_.end() ? -1 : it->second;
  }
  const KF* kf(int32_t slot) const { return slot >= 0 && slot < next() ? kf_[slot] : nullptr; }
  bool alive(int32_t slot) const { return slot >= 0 && slot < next() && alive_[slot]; }
  // the slot to erase, or -1 when pKF is not in the database (erase of an absent keyframe is a no-op, :52-73)
  int32_t erase(const KF* pKF) {
    const int32_t s = slot(pKF);
    if (!alive(s)) return -1;
    alive_[s] = 0;
    return s;
  }
  void clear() { kf_.clear(); alive_.clear(); map_.clear(); }
  // flags [size] of a container of KF* (GetConnectedKeyFrames)
  template <class Set> std::vector<uint8_t> flags(const Set& connected) const {
    std::vector<uint8_t> f((size_t)next(), 0);
    for (const KF* p : connected) {
      const int32_t s = slot(p);
      if (s >= 0) f[s] = 1;
    }
    return f;
  }
  // [size][MCS_KFDB_NEIGH] slots of neighbours(kf) = GetBestCovisibilityKeyFrames(10), -1 padded;
  // a neighbour that was never added is -1 too and keeps its position
  template <class Fn> std::vector<int32_t> neighbours(Fn&& best_covisibles) const {
    std::vector<int32_t> ng((size_t)next() * MCS_KFDB_NEIGH, -1);
    for (int32_t s = 0; s < next(); s++) {
      int k = 0;
      for (const KF* p : best_covisibles(kf_[s])) {
        if (k == MCS_KFDB_NEIGH) break;
        ng[(size_t)s * MCS_KFDB_NEIGH + k++] = slot(p);
      }
    }
    return ng;
  }

 private:
  std::vector<const KF*> kf_;
  std::vector<uint8_t> alive_;
  std::unordered_map<const KF*, int32_t> map_;
};

// KF is the caller's keyframe type and F its frame type.  Needed from them, as in the reference:
//   mnId, mBowVec (an ordered container of (word, value) pairs: DBoW2::BowVector),
//   GetConnectedKeyFrames() and GetBestCovisibilityKeyFrames(int) -> containers of KF*, isBad().
template <class KF>
class KeyFrameDatabase {
 public:
  KeyFrameDatabase(const mcs_vocab* voc, int max_keyframes, int max_entries, int device = 0) {
    check(mcs_kfdb_create(device, voc, max_keyframes, max_entries, &db_), "mcs_kfdb_create");
  }
  ~KeyFrameDatabase() { mcs_kfdb_destroy(db_); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  void add(KF* pKF) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    unpack(pKF->mBowVec, w, v);
    int32_t slot = -1;
    // mRelocScore is uninitialised in the reference; 0 is this adapter's choice (mcs_kfdb.h)
    check(mcs_kfdb_add(db_, w.data(), v.data(), (int32_t)w.size(), 0.0, &slot), "mcs_kfdb_add");
    slots_.bind(pKF, slot);
  }
  void erase(KF* pKF) {
    const int32_t s = slots_.erase(pKF);
    if (s >= 0) check(mcs_kfdb_erase(db_, s, nullptr), "mcs_kfdb_erase");
  }
  void clear() {
    check(mcs_kfdb_clear(db_, nullptr), "mcs_kfdb_clear");
    slots_.clear();
  }

  // the minScore loop of cLoopClosing::DetectLoop (src/cLoopClosing.cpp:141-157)
  double MinScore(KF* pKF) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    unpack(pKF->mBowVec, w, v);
    std::vector<int32_t> list;
    for (KF* p : pKF->GetConnectedKeyFrames())
      if (!p->isBad()) list.push_back(slots_.slot(p));
    double m = 1.0;
    check(mcs_kfdb_min_score(db_, w.data(), v.data(), (int32_t)w.size(), list.data(), (int32_t)list.size(), &m),
          "mcs_kfdb_min_score");
    return m;
  }

  std::vector<KF*> DetectLoopCandidates(KF* pKF, double minScore) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    unpack(pKF->mBowVec, w, v);
    const std::vector<uint8_t> conn = slots_.flags(pKF->GetConnectedKeyFrames());
    const std::vector<int32_t> ng = neighbours();
    std::vector<int32_t> cand((size_t)slots_.next() + 1);
    int32_t n = 0;
    check(mcs_kfdb_detect_loop(db_, w.data(), v.data(), (int32_t)w.size(), (int64_t)pKF->mnId, conn.data(), minScore,
                               ng.data(), cand.data(), slots_.next(), &n, nullptr, nullptr), "mcs_kfdb_detect_loop");
    return pointers(cand, n);
  }

  template <class F>
  std::vector<KF*> DetectRelocalisationCandidates(F* frame) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    unpack(frame->mBowVec, w, v);
    const std::vector<int32_t> ng = neighbours();
    std::vector<int32_t> cand((size_t)slots_.next() + 1);
    int32_t n = 0;
    check(mcs_kfdb_detect_reloc(db_, w.data(), v.data(), (int32_t)w.size(), (int64_t)frame->mnId, ng.data(),
                                cand.data(), slots_.next(), &n, nullptr, nullptr), "mcs_kfdb_detect_reloc");
    return pointers(cand, n);
  }

  const KfSlots<KF>& slots() const { return slots_; }

 private:
  template <class Bow> static void unpack(const Bow& bow, std::vector<uint32_t>& w, std::vector<double>& v) {
    for (const auto& e : bow) { w.push_back((uint32_t)e.first); v.push_back((double)e.second); }
  }
  std::vector<int32_t> neighbours() const {
    return slots_.neighbours([](const KF* k) { return const_cast<KF*>(k)->GetBestCovisibilityKeyFrames(MCS_KFDB_NEIGH); });
  }
  std::vector<KF*> pointers(const std::vector<int32_t>& cand, int32_t n) const {
    std::vector<KF*> out;
    for (int32_t i = 0; i < n; i++) out.push_back(const_cast<KF*>(slots_.kf(cand[i])));
    return out;
  }
  mcs_kfdb* db_ = nullptr;
  KfSlots<KF> slots_;
};

}  // namespace mcs
