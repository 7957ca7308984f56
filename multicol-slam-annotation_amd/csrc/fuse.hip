// cORBmatcher::Fuse on the device: the part of the three overloads that does not depend on map
// state, for ONE query set of map points against a batch of T target keyframes per call.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   Fuse(pKF, curKF, vpMapPoints, th)   (rule 0)         src/cORBmatcher.cpp:1265-1418
//   Fuse(pKF, vpMapPoints, th)          (rule 1)         src/cORBmatcher.cpp:1420-1567
//   Fuse(pKF, Scw, vpPoints, th)        (rule 2)         src/cORBmatcher.cpp:1570-1719
//   cMultiKeyFrame::GetFeaturesInArea                    src/cMultiKeyFrame.cpp:703-746
//   cMultiKeyFrame::GetCameraCenter                      src/cMultiKeyFrame.cpp:159-165
//   WorldToCamHom_fast / isPointInMirrorMask             src/cam_system_omni.cpp:92-112,
//                                                        src/cam_model_omni.cpp:165-180
//   Get{Min,Max}DistanceInvariance                       src/cMapPoint.cpp:498-508
//   ComputeE(Trel), CheckDistEpipolarLine                include/misc.h:235-243, src/misc.cpp:54-70
// Per (target t, query i, camera c): project, mirror mask, distance window, predicted level,
// GetFeaturesInArea, best Hamming distance.  The state-dependent tails (:1379-1415, :1536-1563,
// :1692-1715) are mcs_fuse_select (fuse_select.cpp) on the host.
// Compiled with -ffp-contract=off; every rounding follows the reference's expression order.
// The projection and the epipolar check are frm:: of omni_geom.hpp.
#include "host_util.hpp"
#include "omni_geom.hpp"
#include "window_walk.hpp"
#include <algorithm>
#include <climits>
#include <vector>

namespace mcs {
namespace fuse {

constexpr int kWPB = 4;            // waves per 256-thread workgroup, one (t, i, c) each
constexpr int kMaxCams = 8;
constexpr int kMaxKpPerTarget = 1 << 19;
constexpr double kEpiThresh = 1e-2;   // :1398

struct Args {
  int T, nq, C, bytes, L, mw, mh, n_kp_total, rule, use_dist, th_low;
  double th;
  const int32_t* off; const float* kp_xy; const int32_t* kp_oct; const uint8_t* desc;
  const uint8_t* mask; const double* rays; const double* m_t; const double* cam;
  const uint8_t* mirror; const double* gp; const double* scale;
  const int32_t* cell_ptr; const int32_t* cell_kp;
  const double* q_pos; const double* q_dist; const uint8_t* q_desc; const uint8_t* q_mask;
  const double* q_rays;
  const double* Rt; const double* E;   // workspace: [T][C][12] (R, t of M_t M_c), [T][C][9]
  const uint8_t* q_skip;
  int32_t* best_kp; int32_t* best_dist; uint8_t* epi_ok;
};

// One thread per (t, c): rows 0..2 of M_t M_c, and for rule 0
// E12 = ComputeE(curKF.Get_MtMc_inv(c) * pKF.Get_MtMc(c)) (:1394-1396, misc.h:235-243).
// Every product is cv::Matx's s = 0; s += a(i,k) b(k,j); the matrices' bottom rows are 0 0 0 1.
__global__ __launch_bounds__(64) void k_fuse_setup(const double* __restrict__ m_t,
                                                   const double* __restrict__ m_c,
                                                   const double* __restrict__ cur_mt, int T, int C,
                                                   int rule, double* __restrict__ Rt,
                                                   double* __restrict__ E) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= T * C) return;
  const int t = idx / C, c = idx - t * C;
  double R[9], tt[3];
  frm::mtmc44(m_t + 16 * (int64_t)t, m_c + 16 * c, R, tt);
  double* o = Rt + 12 * (int64_t)idx;
  for (int k = 0; k < 9; k++) o[k] = R[k];
  for (int k = 0; k < 3; k++) o[9 + k] = tt[k];
  if (rule != 0) return;
  double R1[9], t1[3], Ri[9], ti[3];
  frm::mtmc44(cur_mt, m_c + 16 * c, R1, t1);
  frm::inv_rt(R1, t1, Ri, ti);   // Get_MtMc_inv
  double Rr[9], tr[3];   // Trel = T1 * T2, rows 0..2
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(Ri[3 * i + k], R[3 * k + j]));
      Rr[3 * i + j] = __dadd_rn(s, __dmul_rn(ti[i], 0.0));
    }
    double s = 0.0;
    for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(Ri[3 * i + k], tt[k]));
    tr[i] = __dadd_rn(s, __dmul_rn(ti[i], 1.0));
  }
  double ss = 0.0;   // t /= cv::norm(t): times 1. / sqrt(in-order sum of squares)
  for (int k = 0; k < 3; k++) ss = __dadd_rn(ss, __dmul_rn(tr[k], tr[k]));
  const double ia = __ddiv_rn(1.0, __dsqrt_rn(ss));
  for (int k = 0; k < 3; k++) tr[k] = __dmul_rn(tr[k], ia);
  const double S[9] = {0.0, -tr[2], tr[1], tr[2], 0.0, -tr[0], -tr[1], tr[0], 0.0};   // Skew
  double* e = E + 9 * (int64_t)idx;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn(S[3 * i + k], Rr[3 * k + j]));
      e[3 * i + j] = s;
    }
}

// The front half of one (t, i, c) (:1295-1327 and its twins): false = the camera is left before
// the window; else the projection, the predicted level and the radius.  Wave-uniform.
__device__ __forceinline__ bool project(const Args& a, int t, int i, int c, double* u, double* v,
                                        int* level, double* radius) {
  const double* Rt = a.Rt + 12 * ((int64_t)t * a.C + c);
  const double* P = a.q_pos + 3 * (int64_t)i;
  frm::world_to_cam_img(Rt, Rt + 9, a.cam + 17 * c, P, *u, *v);
  if (!frm::in_mirror_mask(a.mirror, c, a.mw, a.mh, *u, *v)) return false;
  const double maxD = __dmul_rn(1.2, a.q_dist[2 * (int64_t)i + 1]);
  const double minD = __dmul_rn(0.8, a.q_dist[2 * (int64_t)i]);
  const double* Mt = a.m_t + 16 * (int64_t)t;   // Ow = Hom2T(M_t)
  const double PO[3] = {__dsub_rn(P[0], Mt[3]), __dsub_rn(P[1], Mt[7]), __dsub_rn(P[2], Mt[11])};
  double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(PO[0], PO[0]), __dmul_rn(PO[1], PO[1])),
                                  __dmul_rn(PO[2], PO[2])));
  if (a.rule != 2) d = (double)(float)d;   // `const float dist3D` (:1306, :1464); double at :1623
  if (d < minD || d > maxD) return false;
  const int lv = frm::predict_level(a.scale, a.L, __ddiv_rn(d, minD));
  *level = lv;
  *radius = __dmul_rn(a.th, a.scale[lv]);
  return true;
}

// One wave per (t, i, c).  Every lane computes the front half (it is wave-uniform); the window is
// walked by win::walk_best (window_walk.hpp), whose wave minimum is the reference's first minimum
// under strict <; use_dist = 0 is rule 1 as written, which never assigns dist (:1507-1514).
// Offsets, cell ranges and cell entries are clamped to the target.
__global__ __launch_bounds__(256) void k_fuse(Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWPB + (threadIdx.x >> 6);
  if (w >= (int64_t)a.T * a.nq * a.C) return;
  const int c = (int)(w % a.C);
  const int64_t ti = w / a.C;
  const int i = (int)(ti % a.nq), t = (int)(ti / a.nq);
  int bk = -1, bd = INT_MAX;
  uint8_t ep = 0;
  double u, v, r;
  int lv, x0, x1, y0, y1;
  const bool skip = a.q_skip && a.q_skip[ti] != 0;
  if (!skip && project(a, t, i, c, &u, &v, &lv, &r) &&
      win::cell_range(a.gp + 4 * c, u, v, r, &x0, &x1, &y0, &y1)) {
    const int o = min(max(a.off[t], 0), a.n_kp_total);
    // a target holds < 2^19 keypoints (position field of the key); the host entry rejects more
    const int n_t = min(min(max(a.off[t + 1] - o, 0), a.n_kp_total - o), kMaxKpPerTarget - 1);
    const int32_t* cptr = a.cell_ptr + (int64_t)t * (a.C * win::kCols * win::kRows + 1);
    const int32_t* ckp = a.cell_kp + o;
    const uint8_t* qd = a.q_desc + (int64_t)i * a.bytes;
    const uint8_t* qm = a.q_mask ? a.q_mask + (int64_t)i * a.bytes : nullptr;
    int k = -1;
    if (win::walk_best(lane, c, x0, x1, y0, y1, cptr, ckp, o, n_t, a.kp_xy, a.kp_oct, a.desc, a.mask,
                       a.bytes, qd, qm, u, v, r, lv, a.use_dist, &bd, &k)) {
      if (bd <= a.th_low) {
        bk = k;
        if (a.rule == 0 && a.epi_ok)
          ep = frm::epi_check(a.q_rays + 3 * (int64_t)i, a.rays + 3 * ((int64_t)o + k),
                              a.E + 9 * ((int64_t)t * a.C + c), kEpiThresh) ? 1 : 0;
      }
    }
  }
  if (lane == 0) {
    a.best_kp[w] = bk;
    a.best_dist[w] = bd;
    if (a.epi_ok) a.epi_ok[w] = ep;
  }
}

static int check_args(int rule, const mcs_fuse_targets* tg, const mcs_fuse_queries* q) {
  if (!tg || !q) { set_error("fuse: null targets / queries"); return MCS_ERR_ARG; }
  if (rule < 0 || rule > 2) { set_error("fuse: rule must be 0, 1 or 2"); return MCS_ERR_ARG; }
  if (int rc = host::check_desc_bytes(tg->bytes, "fuse")) return rc;
  if (tg->n_cams < 1 || tg->n_cams > kMaxCams) { set_error("fuse: 1 to 8 cameras"); return MCS_ERR_ARG; }
  if (tg->n_targets < 0 || tg->n_kp_total < 0 || q->nq < 0 || tg->n_levels < 1 || tg->mirror_w < 1 || tg->mirror_h < 1) {
    set_error("fuse: negative count or empty pyramid / mirror mask");
    return MCS_ERR_ARG;
  }
  if ((tg->mask != nullptr) != (q->mask != nullptr)) { set_error("fuse: descriptor masks for the queries and the targets, or for neither"); return MCS_ERR_ARG; }
  if ((int64_t)tg->n_targets * q->nq * tg->n_cams >= (int64_t)INT_MAX * kWPB) { set_error("fuse: batch too large for one launch"); return MCS_ERR_ARG; }
  if (tg->n_targets > 0 && q->nq > 0) {
    if (!tg->off || !tg->m_t || !tg->m_c || !tg->cam || !tg->mirror || !tg->grid_params || !tg->scale ||
        !q->pos || !q->dist || !q->desc || (rule == 0 && (!q->rays || !q->m_t)) ||
        (tg->n_kp_total > 0 && (!tg->kp_xy || !tg->kp_octave || !tg->desc || (rule == 0 && !tg->rays)))) {
      set_error("fuse: null buffer");
      return MCS_ERR_ARG;
    }
  }
  return MCS_OK;
}

}  // namespace fuse
}  // namespace mcs

using namespace mcs;

struct mcs_fuse_workspace {
  int device = 0, max_targets = 0;
  double* Rt = nullptr;
  double* E = nullptr;
};

extern "C" {

int mcs_fuse_workspace_create(int32_t device, int32_t max_targets, mcs_fuse_workspace** out) {
  if (!out || max_targets < 1) { set_error("fuse workspace: bad argument"); return MCS_ERR_ARG; }
  if (int rc = host::open_device(device, "fuse workspace")) return rc;
  mcs_fuse_workspace* w = new mcs_fuse_workspace;
  w->device = device;
  w->max_targets = max_targets;
  const size_t n = (size_t)max_targets * fuse::kMaxCams;
  hipError_t e = hipMalloc((void**)&w->Rt, n * 12 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->E, n * 9 * sizeof(double));
  if (e != hipSuccess) {
    mcs_fuse_workspace_destroy(w);
    set_hip_error(e, "fuse workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_fuse_workspace_destroy(mcs_fuse_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->Rt) (void)hipFree(w->Rt);
  if (w->E) (void)hipFree(w->E);
  delete w;
}

int mcs_fuse_device(mcs_fuse_workspace* ws, int32_t rule, int32_t flags,
                    const mcs_fuse_targets* tg, const mcs_fuse_queries* q, double th,
                    int32_t th_low, const uint8_t* d_q_skip, int32_t* d_best_kp,
                    int32_t* d_best_dist, uint8_t* d_epi_ok, void* stream) {
  int rc = fuse::check_args(rule, tg, q);
  if (rc) return rc;
  const int64_t nw = (int64_t)tg->n_targets * q->nq * tg->n_cams;
  if (nw == 0) return MCS_OK;
  if (!d_best_kp || !d_best_dist || (rule == 0 && !d_epi_ok) || !tg->cell_ptr ||
      (tg->n_kp_total > 0 && !tg->cell_kp)) {
    set_error("fuse: null device buffer");
    return MCS_ERR_ARG;
  }
  if (ws && tg->n_targets > ws->max_targets) {
    set_error("fuse: more targets than the workspace holds");
    return MCS_ERR_ARG;
  }
  mcs_fuse_workspace* tmp = nullptr;
  if (!ws) {
    int dev = 0;
    MCS_HIP_CHECK(hipGetDevice(&dev));
    rc = mcs_fuse_workspace_create(dev, tg->n_targets, &tmp);
    if (rc) return rc;
    ws = tmp;
  } else {
    MCS_HIP_CHECK(hipSetDevice(ws->device));
  }
  hipStream_t st = (hipStream_t)stream;
  const int tc = tg->n_targets * tg->n_cams;
  hipLaunchKernelGGL(fuse::k_fuse_setup, dim3((tc + 63) / 64), dim3(64), 0, st, tg->m_t, tg->m_c,
                     q->m_t, tg->n_targets, tg->n_cams, rule, ws->Rt, ws->E);
  fuse::Args a{tg->n_targets, q->nq, tg->n_cams, tg->bytes, tg->n_levels, tg->mirror_w, tg->mirror_h,
               tg->n_kp_total, rule, (rule != 1 || (flags & MCS_FUSE_USE_DISTANCE)) ? 1 : 0, th_low,
               th, tg->off, tg->kp_xy, tg->kp_octave, tg->desc, tg->mask, tg->rays, tg->m_t, tg->cam,
               tg->mirror, tg->grid_params, tg->scale, tg->cell_ptr, tg->cell_kp, q->pos, q->dist,
               q->desc, q->mask, q->rays, ws->Rt, ws->E, d_q_skip, d_best_kp, d_best_dist,
               rule == 0 ? d_epi_ok : nullptr};
  hipLaunchKernelGGL(fuse::k_fuse, dim3((unsigned)((nw + fuse::kWPB - 1) / fuse::kWPB)), dim3(256), 0,
                     st, a);
  hipError_t e = hipGetLastError();
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    mcs_fuse_workspace_destroy(tmp);
  }
  MCS_HIP_CHECK(e);
  return MCS_OK;
}

int mcs_fuse(int32_t device, int32_t rule, int32_t flags, const mcs_fuse_targets* tg,
             const mcs_fuse_queries* q, double th, int32_t th_low, const uint8_t* q_skip,
             int32_t* best_kp, int32_t* best_dist, uint8_t* epi_ok) {
  int rc = fuse::check_args(rule, tg, q);
  if (rc) return rc;
  const int T = tg->n_targets, nq = q->nq;
  const size_t nw = (size_t)T * nq * tg->n_cams;
  if (nw == 0) return MCS_OK;
  if (!best_kp || !best_dist || (rule == 0 && !epi_ok) || (tg->n_kp_total > 0 && !tg->kp_cam)) {
    set_error("fuse: null host buffer");
    return MCS_ERR_ARG;
  }
  if ((rc = host::check_set_offsets(tg->off, T, tg->n_kp_total, fuse::kMaxKpPerTarget, "fuse"))) return rc;
  if ((rc = host::open_device(device, "fuse"))) return rc;
  const size_t nb = (size_t)tg->bytes;
  host::DevBufs B;
  mcs_fuse_targets d;
  if ((rc = host::upload_kf_set(B, *tg, host::kKfSearch | (rule == 0 ? host::kKfRays : 0), &d))) return rc;
  mcs_fuse_queries dq = *q;
  dq.pos = B.up(q->pos, 3 * (size_t)nq);
  dq.dist = B.up(q->dist, 2 * (size_t)nq);
  dq.desc = B.up(q->desc, (size_t)nq * nb);
  dq.mask = B.up(q->mask, (size_t)nq * nb);
  dq.rays = rule == 0 ? B.up(q->rays, 3 * (size_t)nq) : nullptr;
  dq.m_t = rule == 0 ? B.up(q->m_t, 16) : nullptr;
  const uint8_t* d_skip = B.up(q_skip, (size_t)T * nq);
  int32_t* d_bk = B.alloc<int32_t>(nw);
  int32_t* d_bd = B.alloc<int32_t>(nw);
  uint8_t* d_ep = rule == 0 ? B.alloc<uint8_t>(nw) : nullptr;
  if (B.err != hipSuccess) { set_hip_error(B.err, "fuse upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  rc = mcs_fuse_device(nullptr, rule, flags, &d, &dq, th, th_low, d_skip, d_bk, d_bd, d_ep, nullptr);
  if (rc) return rc;
  B.down(best_kp, d_bk, nw);
  B.down(best_dist, d_bd, nw);
  if (rule == 0) B.down(epi_ok, d_ep, nw);
  if (B.err != hipSuccess) { set_hip_error(B.err, "fuse download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
