// cORBmatcher::SearchBySim3 on the device: the whole function, for ONE current keyframe KF1
// against a batch of T candidate keyframes KF2_t, each with its own Sim3 (s12, R12, t12).
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   cORBmatcher::SearchBySim3                            src/cORBmatcher.cpp:1721-1988
//   cMultiKeyFrame::GetPoseInverse                       src/cMultiKeyFrame.cpp:152-157
//   cConverter::invMat                                   src/cConverter.cpp:31-44
//   cCamModelGeneral_::WorldToImg / isPointInMirrorMask  src/cam_model_omni.cpp:147-180
//   cMultiKeyFrame::GetFeaturesInArea                    src/cMultiKeyFrame.cpp:703-746
//   Get{Min,Max}DistanceInvariance                       src/cMapPoint.cpp:498-508
// Three launches: the transforms per candidate (:1729-1743 and the invMat(M_c) of :1795, :1889),
// both projection passes (:1779-1967) with one wave per (candidate, direction, keypoint), and
// the agreement check (:1969-1987).  Nothing depends on map state that changes during the call,
// so there is no host tail.  The window walk is win::walk_best of window_walk.hpp, shared with
// k_fuse; invMat, the Matx products and WorldToImg are frm:: of omni_geom.hpp.  Compiled with
// -ffp-contract=off; every rounding follows the reference's expression order (cv::Matx products:
// s = 0; s += a_k * b_k, k ascending).
#include "host_util.hpp"
#include "omni_geom.hpp"
#include "window_walk.hpp"
#include <algorithm>
#include <climits>
#include <vector>

namespace mcs {
namespace sim3 {

constexpr int kWPB = 4;            // waves per 256-thread workgroup, one (t, direction, keypoint) each
constexpr int kMaxCams = 8;
constexpr int kMaxKp = 1 << 19;    // per keyframe: the position field of walk_best's key
constexpr int kXf = 36;            // doubles per candidate: R2w 9, t2w 3, sR12 9, sR21 9, t21 3, t12 3
constexpr int kCells = win::kCols * win::kRows;

// one packed keyframe set as the kernels read it (device pointers)
struct Set {
  int n_kp_total;
  const int32_t* off; const float* kp_xy; const int32_t* kp_oct; const int32_t* kp_cam;
  const uint8_t* desc; const uint8_t* mask; const double* cam; const uint8_t* mirror;
  const double* gp; const double* scale; const int32_t* cell_ptr; const int32_t* cell_kp;
};

// the map points of a set's keypoint slots
struct Pts {
  const double* pos; const double* dist; const uint8_t* desc; const uint8_t* mask;
};

struct Args {
  int T, n1, C, bytes, L, mw, mh, th_high;
  double th;
  Set k1, k2;
  Pts p1, p2;
  const uint8_t* active1; const uint8_t* active2;
  const double* xf;        // workspace [T][kXf]
  const double* T1;        // workspace [12]: R1w, t1w
  const double* imc1;      // workspace [C][12]: invMat(KF1's M_c[c]), rows 0..2 as R [9], t [3]
  const double* imc2;      // the same of the candidates' rig
  int32_t* match1; int32_t* match2;
};

// Thread t < T: candidate t's T2 = GetPoseInverse (:1730), sR12, sR21, t21 (:1741-1743), and
// n_found[t] = 0.  Thread T: KF1's T1 (:1729).  Threads T + 1 + c and T + 1 + C + c: invMat of
// M_c[c] of KF1's rig and of the candidates' rig (:1889, :1795).
__global__ __launch_bounds__(64) void k_sim3_setup(const double* __restrict__ mt1,
                                                   const double* __restrict__ mt2,
                                                   const double* __restrict__ mc1,
                                                   const double* __restrict__ mc2,
                                                   const double* __restrict__ s12,
                                                   const double* __restrict__ R12,
                                                   const double* __restrict__ t12, int T, int C,
                                                   double* __restrict__ xf, double* __restrict__ T1,
                                                   double* __restrict__ imc1, double* __restrict__ imc2,
                                                   int32_t* __restrict__ n_found) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx > T + 2 * C) return;
  if (idx == T) { frm::inv_mat44(mt1, T1, T1 + 9); return; }
  if (idx > T) {
    const int c = idx - T - 1;
    if (c < C) frm::inv_mat44(mc1 + 16 * c, imc1 + 12 * c, imc1 + 12 * c + 9);
    else frm::inv_mat44(mc2 + 16 * (c - C), imc2 + 12 * (c - C), imc2 + 12 * (c - C) + 9);
    return;
  }
  double* o = xf + kXf * (int64_t)idx;
  frm::inv_mat44(mt2 + 16 * (int64_t)idx, o, o + 9);
  const double s = s12[idx], inv = __ddiv_rn(1.0, s);
  const double* R = R12 + 9 * (int64_t)idx;
  const double* tt = t12 + 3 * (int64_t)idx;
  double* sR12 = o + 12;
  double* sR21 = o + 21;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      sR12[3 * i + j] = __dmul_rn(R[3 * i + j], s);       // s12 * R12
      sR21[3 * i + j] = __dmul_rn(R[3 * j + i], inv);     // (1.0 / s12) * R12.t()
    }
  for (int i = 0; i < 3; i++) {                           // t21 = -sR21 * t12
    double a = 0.0;
    for (int k = 0; k < 3; k++) a = __dadd_rn(a, __dmul_rn(-sR21[3 * i + k], tt[k]));
    o[30 + i] = a;
    o[33 + i] = tt[i];
  }
  n_found[idx] = 0;
}

// One wave per (t, direction, keypoint): waves [0, T * n1) are direction 1 (:1779-1872), wave
// T * n1 + j is direction 2 (:1874-1967) for keypoint j of the packed candidates.  Every lane
// computes the front half (it is wave-uniform).  `from` is the keyframe whose map point is
// projected, `to` the one whose grid is searched; the camera is the keypoint's own, the camera
// model and the mirror mask are the candidates' rig's in both directions (:1791, :1885), M_c is
// the searched keyframe's rig's (:1795, :1889).
__global__ __launch_bounds__(256) void k_sim3_search(Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWPB + (threadIdx.x >> 6);
  const int64_t nd1 = (int64_t)a.T * a.n1;
  if (w >= nd1 + a.k2.n_kp_total) return;
  const bool d1 = w < nd1;
  int t, il;             // candidate, keypoint index local to the projected keyframe
  int64_t gi;            // the same keypoint in the packed arrays of its set
  int32_t* out;
  bool ok = true;
  // the first keypoint and the count of both keyframes, clamped to their buffers
  const int o1 = min(max(a.k1.off[0], 0), a.k1.n_kp_total);
  const int n_1 = min(min(max(a.k1.off[1] - o1, 0), a.k1.n_kp_total - o1), kMaxKp - 1);
  if (d1) {
    t = (int)(w / a.n1);
    il = (int)(w - (int64_t)t * a.n1);
    gi = (int64_t)o1 + il;
    out = a.match1 + w;
    ok = il < n_1 && a.active1[w] != 0;
  } else {
    const int j = (int)(w - nd1);
    out = a.match2 + j;
    int lo = 0, hi = a.T;          // the last t with off[t] <= j; verified below, as off is device data
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.k2.off[mid] <= j) lo = mid; else hi = mid;
    }
    t = lo;
    gi = j;
    il = 0;
  }
  const int o2 = min(max(a.k2.off[t], 0), a.k2.n_kp_total);
  const int n_2 = min(min(max(a.k2.off[t + 1] - o2, 0), a.k2.n_kp_total - o2), kMaxKp - 1);
  if (!d1) {
    il = (int)(gi - o2);
    ok = il >= 0 && il < n_2 && a.active2[gi] != 0;
  }
  const Set& from = d1 ? a.k1 : a.k2;
  const Set& to = d1 ? a.k2 : a.k1;
  const Pts& pt = d1 ? a.p1 : a.p2;
  int res = -1;
  const int c = ok ? from.kp_cam[gi] : -1;
  if (c >= 0 && c < a.C) {
    const double* xf = a.xf + kXf * (int64_t)t;
    const double* P = pt.pos + 3 * gi;
    const double Pw[3] = {P[0], P[1], P[2]};
    double pa[3], pb[3], pc[3];
    if (d1) {
      frm::rot_add(a.T1, Pw, a.T1 + 9, pa);        // p3Dc1 = R1w * p3Dw + t1w
      frm::rot_add(xf + 21, pa, xf + 30, pb);      // p3Dc2 = sR21 * p3Dc1 + t21
    } else {
      frm::rot_add(xf, Pw, xf + 9, pa);            // p3Dc2 = R2w * p3Dw + t2w
      frm::rot_add(xf + 12, pa, xf + 33, pb);      // p3Dc1 = sR12 * p3Dc2 + t12
    }
    const double* im = (d1 ? a.imc2 : a.imc1) + 12 * c;
    frm::hom_mul(im, im + 9, pb, pc);         // invMat(M_c) * toVec4d(p): k = 0..3
    double u = 0.0, v = 0.0, r = 0.0;
    int lv = 0, x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    bool go = !(pb[2] < 0.0);                 // the depth test is on the rig-frame z (:1798, :1892)
    if (go) {
      frm::world_to_img(a.k2.cam + 17 * c, pc[0], pc[1], pc[2], u, v);
      go = frm::in_mirror_mask(a.k2.mirror, c, a.mw, a.mh, u, v);
    }
    if (go) {
      const double maxD = __dmul_rn(1.2, pt.dist[2 * gi + 1]);
      const double minD = __dmul_rn(0.8, pt.dist[2 * gi]);
      const double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(pc[0], pc[0]), __dmul_rn(pc[1], pc[1])),
                                            __dmul_rn(pc[2], pc[2])));
      go = !(d < minD || d > maxD);
      if (go) {
        lv = frm::predict_level(to.scale, a.L, __ddiv_rn(d, minD));
        r = __dmul_rn(a.th, to.scale[lv]);
        go = win::cell_range(to.gp + 4 * c, u, v, r, &x0, &x1, &y0, &y1);
      }
    }
    if (go) {
      const int o = d1 ? o2 : o1, n_t = d1 ? n_2 : n_1;
      const int32_t* cptr = to.cell_ptr + (d1 ? (int64_t)t * (a.C * kCells + 1) : 0);
      int bd = INT_MAX, k = -1;
      if (win::walk_best(lane, c, x0, x1, y0, y1, cptr, to.cell_kp + o, o, n_t, to.kp_xy, to.kp_oct,
                         to.desc, to.mask, a.bytes, pt.desc + gi * a.bytes,
                         pt.mask ? pt.mask + gi * a.bytes : nullptr, u, v, r, lv, 1, &bd, &k) &&
          bd <= a.th_high)
        res = k;
    }
  }
  if (lane == 0) *out = res;
}

// One thread per (t, i1), a block stays inside one t (:1969-1987).
__global__ __launch_bounds__(256) void k_sim3_agree(const int32_t* __restrict__ match1,
                                                    const int32_t* __restrict__ match2,
                                                    const int32_t* __restrict__ off2, int n1,
                                                    int n_kp_total2, int32_t* __restrict__ matches12,
                                                    int32_t* __restrict__ n_found) {
  const int t = blockIdx.y, i1 = blockIdx.x * blockDim.x + threadIdx.x;
  int hit = 0;
  if (i1 < n1) {
    const int o2 = min(max(off2[t], 0), n_kp_total2);
    const int n_2 = min(max(off2[t + 1] - o2, 0), n_kp_total2 - o2);
    const int idx2 = match1[(int64_t)t * n1 + i1];
    hit = idx2 >= 0 && idx2 < n_2 && match2[o2 + idx2] == i1;
    matches12[(int64_t)t * n1 + i1] = hit ? idx2 : -1;
  }
  const int cnt = __popcll(__ballot(hit));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_found + t, cnt);
}

using host::bad_arg;

static bool set_has_nulls(const mcs_fuse_targets* k, bool grid) {
  if (!k->off || !k->m_t || !k->m_c || !k->cam || !k->mirror || !k->grid_params || !k->scale) return true;
  if (k->n_kp_total > 0 && (!k->kp_xy || !k->kp_octave || !k->kp_cam || !k->desc)) return true;
  return grid && (!k->cell_ptr || (k->n_kp_total > 0 && !k->cell_kp));
}

// what both entries check; `grid`: cell_ptr / cell_kp must be given (the device entry)
static int check_args(const mcs_fuse_targets* k1, const mcs_sim3_points* p1, const mcs_fuse_targets* k2,
                      const mcs_sim3_points* p2, const void* act1, const void* act2, const void* s12,
                      const void* R12, const void* t12, const void* matches12, const void* n_found,
                      bool grid) {
  if (!k1 || !p1 || !k2 || !p2) return bad_arg("sim3: null keyframe set / points");
  if (int rc = host::check_desc_bytes(k1->bytes, "sim3")) return rc;
  if (k1->n_cams < 1 || k1->n_cams > kMaxCams || k2->n_cams > kMaxCams) return bad_arg("sim3: 1 to 8 cameras");
  if (k1->n_targets != 1) return bad_arg("sim3: kf1 must be a set of exactly one keyframe");
  if (k1->n_cams != k2->n_cams || k1->bytes != k2->bytes || k1->n_levels != k2->n_levels ||
      k1->mirror_w != k2->mirror_w || k1->mirror_h != k2->mirror_h)
    return bad_arg("sim3: n_cams, bytes, n_levels and the mirror size of kf1 and kf2s must agree (shared rig)");
  if (k2->n_targets < 0 || k1->n_kp_total < 0 || k2->n_kp_total < 0 || k1->n_levels < 1 ||
      k1->mirror_w < 1 || k1->mirror_h < 1)
    return bad_arg("sim3: negative count or empty pyramid / mirror mask");
  if (p1->n != k1->n_kp_total || p2->n != k2->n_kp_total)
    return bad_arg("sim3: the points must hold one slot per keypoint of their set");
  // an empty side has no rows to point at: the sides that hold keypoints must agree
  int with = 0, sides = 0;
  if (k1->n_kp_total > 0) { sides += 2; with += (k1->mask != nullptr) + (p1->mask != nullptr); }
  if (k2->n_kp_total > 0) { sides += 2; with += (k2->mask != nullptr) + (p2->mask != nullptr); }
  if (with != 0 && with != sides)
    return bad_arg("sim3: descriptor masks for both keyframe sets and both point sets, or for none");
  if (k1->n_kp_total >= kMaxKp) return bad_arg("sim3: keypoints per keyframe must be below 2^19 (position field of the key)");
  if ((int64_t)k2->n_targets * k1->n_kp_total + k2->n_kp_total >= (int64_t)INT_MAX)
    return bad_arg("sim3: batch too large for one launch");
  if (k2->n_targets == 0) return MCS_OK;
  if (set_has_nulls(k1, grid) || set_has_nulls(k2, grid) || !s12 || !R12 || !t12 || !n_found ||
      (k1->n_kp_total > 0 && (!p1->pos || !p1->dist || !p1->desc || !act1 || !matches12)) ||
      (k2->n_kp_total > 0 && (!p2->pos || !p2->dist || !p2->desc || !act2)))
    return bad_arg("sim3: null buffer");
  return MCS_OK;
}

// the host entry sees the offsets and the cameras
static int check_host_set(const mcs_fuse_targets* k) {
  if (int rc = host::check_set_offsets(k->off, k->n_targets, k->n_kp_total, kMaxKp, "sim3")) return rc;
  return host::check_kp_cam(k->kp_cam, k->n_kp_total, k->n_cams, "sim3");
}

static Set dev_set(const mcs_fuse_targets* k) {
  return Set{k->n_kp_total, k->off, k->kp_xy, k->kp_octave, k->kp_cam, k->desc, k->mask, k->cam,
             k->mirror, k->grid_params, k->scale, k->cell_ptr, k->cell_kp};
}

}  // namespace sim3
}  // namespace mcs

using namespace mcs;

struct mcs_sim3_workspace {
  int device = 0, max_targets = 0, max_kp = 0;
  double* xf = nullptr;      // [max_targets][kXf], then T1 [12], imc1 [8][12], imc2 [8][12]
  int32_t* match = nullptr;  // [2][max_targets * max_kp]: vnMatch1 / vnMatch2 when the caller wants neither
};

extern "C" {

int mcs_sim3_workspace_create(int32_t device, int32_t max_targets, int32_t max_kp,
                              mcs_sim3_workspace** out) {
  if (!out || max_targets < 1 || max_kp < 1 || max_kp >= sim3::kMaxKp ||
      (int64_t)max_targets * max_kp >= INT_MAX / 2) {
    set_error("sim3 workspace: bad argument");
    return MCS_ERR_ARG;
  }
  if (int rc = host::open_device(device, "sim3 workspace")) return rc;
  mcs_sim3_workspace* w = new mcs_sim3_workspace;
  w->device = device;
  w->max_targets = max_targets;
  w->max_kp = max_kp;
  const size_t nx = (size_t)max_targets * sim3::kXf + 12 + 2 * 12 * sim3::kMaxCams;
  hipError_t e = hipMalloc((void**)&w->xf, nx * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->match, 2 * (size_t)max_targets * max_kp * sizeof(int32_t));
  if (e != hipSuccess) {
    mcs_sim3_workspace_destroy(w);
    set_hip_error(e, "sim3 workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_sim3_workspace_destroy(mcs_sim3_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->xf) (void)hipFree(w->xf);
  if (w->match) (void)hipFree(w->match);
  delete w;
}

int mcs_search_by_sim3_device(mcs_sim3_workspace* ws, const mcs_fuse_targets* kf1,
                              const mcs_sim3_points* pts1, const mcs_fuse_targets* kf2s,
                              const mcs_sim3_points* pts2, const uint8_t* d_active1,
                              const uint8_t* d_active2, const double* d_s12, const double* d_R12,
                              const double* d_t12, double th, int32_t th_high, int32_t* d_match1,
                              int32_t* d_match2, int32_t* d_matches12, int32_t* d_n_found,
                              void* stream) {
  int rc = sim3::check_args(kf1, pts1, kf2s, pts2, d_active1, d_active2, d_s12, d_R12, d_t12,
                            d_matches12, d_n_found, true);
  if (rc) return rc;
  const int T = kf2s->n_targets, n1 = kf1->n_kp_total, n2 = kf2s->n_kp_total, C = kf1->n_cams;
  if (T == 0) return MCS_OK;
  if (ws && (T > ws->max_targets || n1 > ws->max_kp || n2 > (int64_t)ws->max_targets * ws->max_kp)) {
    set_error("sim3: more candidates or keypoints than the workspace holds");
    return MCS_ERR_ARG;
  }
  mcs_sim3_workspace* tmp = nullptr;
  if (!ws) {
    int dev = 0;
    MCS_HIP_CHECK(hipGetDevice(&dev));
    const int64_t per = std::max<int64_t>(std::max<int64_t>(n1, (n2 + T - 1) / T), 1);
    if (per >= sim3::kMaxKp) return host::bad_arg("sim3: keypoints per keyframe must be below 2^19 (position field of the key)");
    rc = mcs_sim3_workspace_create(dev, T, (int32_t)per, &tmp);
    if (rc) return rc;
    ws = tmp;
  } else {
    MCS_HIP_CHECK(hipSetDevice(ws->device));
  }
  hipStream_t st = (hipStream_t)stream;
  double* T1 = ws->xf + (size_t)ws->max_targets * sim3::kXf;
  double* imc1 = T1 + 12;
  double* imc2 = imc1 + 12 * sim3::kMaxCams;
  int32_t* m1 = d_match1 ? d_match1 : ws->match;
  int32_t* m2 = d_match2 ? d_match2 : ws->match + (size_t)ws->max_targets * ws->max_kp;
  const int ns = T + 1 + 2 * C;
  hipLaunchKernelGGL(sim3::k_sim3_setup, dim3((ns + 63) / 64), dim3(64), 0, st, kf1->m_t, kf2s->m_t,
                     kf1->m_c, kf2s->m_c, d_s12, d_R12, d_t12, T, C, ws->xf, T1, imc1, imc2, d_n_found);
  const int64_t nw = (int64_t)T * n1 + n2;
  if (nw > 0) {
    sim3::Args a{T, n1, C, kf1->bytes, kf1->n_levels, kf1->mirror_w, kf1->mirror_h, th_high, th,
                 sim3::dev_set(kf1), sim3::dev_set(kf2s),
                 sim3::Pts{pts1->pos, pts1->dist, pts1->desc, pts1->mask},
                 sim3::Pts{pts2->pos, pts2->dist, pts2->desc, pts2->mask},
                 d_active1, d_active2, ws->xf, T1, imc1, imc2, m1, m2};
    hipLaunchKernelGGL(sim3::k_sim3_search, dim3((unsigned)((nw + sim3::kWPB - 1) / sim3::kWPB)),
                       dim3(256), 0, st, a);
  }
  if (n1 > 0)
    hipLaunchKernelGGL(sim3::k_sim3_agree, dim3((n1 + 255) / 256, T), dim3(256), 0, st, m1, m2,
                       kf2s->off, n1, n2, d_matches12, d_n_found);
  hipError_t e = hipGetLastError();
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    mcs_sim3_workspace_destroy(tmp);
  }
  MCS_HIP_CHECK(e);
  return MCS_OK;
}

int mcs_search_by_sim3(int32_t device, const mcs_fuse_targets* kf1, const mcs_sim3_points* pts1,
                       const mcs_fuse_targets* kf2s, const mcs_sim3_points* pts2,
                       const uint8_t* active1, const uint8_t* active2, const double* s12,
                       const double* R12, const double* t12, double th, int32_t th_high,
                       int32_t* match1, int32_t* match2, int32_t* matches12, int32_t* n_found) {
  int rc = sim3::check_args(kf1, pts1, kf2s, pts2, active1, active2, s12, R12, t12, matches12, n_found,
                            false);
  if (rc) return rc;
  const int T = kf2s->n_targets;
  if (T == 0) return MCS_OK;
  if ((rc = sim3::check_host_set(kf1)) || (rc = sim3::check_host_set(kf2s))) return rc;
  if ((rc = host::open_device(device, "sim3"))) return rc;
  const size_t nb = (size_t)kf1->bytes;
  const size_t n1 = (size_t)kf1->n_kp_total, n2 = (size_t)kf2s->n_kp_total;
  host::DevBufs B;
  auto upload = [&](const mcs_fuse_targets* k, const mcs_sim3_points* p, mcs_fuse_targets* d, mcs_sim3_points* dp) {
    const size_t nk = (size_t)k->n_kp_total;
    *dp = *p;
    dp->pos = B.up(p->pos, 3 * nk);
    dp->dist = B.up(p->dist, 2 * nk);
    dp->desc = B.up(p->desc, nk * nb);
    dp->mask = B.up(p->mask, nk * nb);
    return host::upload_kf_set(B, *k, host::kKfSearch | host::kKfCam, d);
  };
  mcs_fuse_targets d1, d2;
  mcs_sim3_points dp1, dp2;
  if ((rc = upload(kf1, pts1, &d1, &dp1)) || (rc = upload(kf2s, pts2, &d2, &dp2))) return rc;
  const uint8_t* d_a1 = B.up(active1, (size_t)T * n1);
  const uint8_t* d_a2 = B.up(active2, n2);
  const double* d_s = B.up(s12, (size_t)T);
  const double* d_R = B.up(R12, 9 * (size_t)T);
  const double* d_t = B.up(t12, 3 * (size_t)T);
  int32_t* d_m1 = B.alloc<int32_t>((size_t)T * n1);
  int32_t* d_m2 = B.alloc<int32_t>(n2);
  int32_t* d_m12 = B.alloc<int32_t>((size_t)T * n1);
  int32_t* d_nf = B.alloc<int32_t>((size_t)T);
  if (B.err != hipSuccess) { set_hip_error(B.err, "sim3 upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  rc = mcs_search_by_sim3_device(nullptr, &d1, &dp1, &d2, &dp2, d_a1, d_a2, d_s, d_R, d_t, th, th_high,
                                 d_m1, d_m2, d_m12, d_nf, nullptr);
  if (rc) return rc;
  B.down(match1, d_m1, (size_t)T * n1);
  B.down(match2, d_m2, n2);
  B.down(matches12, d_m12, (size_t)T * n1);
  B.down(n_found, d_nf, (size_t)T);
  if (B.err != hipSuccess) { set_hip_error(B.err, "sim3 download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
