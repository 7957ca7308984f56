// The windowed matchers of tracking with nothing downloaded (C-ABI of include/mcs_matcher.h,
// "device form" of the window section): the cMultiFrame grid from device keypoints
// (track_grid.hpp), the queries of SearchByProjection(F, MPs) and SearchByProjection(Current,
// Last) from device data (track_queries.hpp), the candidate walk of window.hip through an index
// into the descriptor source, and the reference's ordered selection in one launch
// (track_select.hpp).  With a workspace the host allocates nothing, copies nothing back and never
// waits; a candidate overflow is reported in device memory.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   TrackWithMotionModel -> SearchByProjection(Cur, Last)  src/cORBmatcher.cpp:1991-2123 (rule 1)
//   TrackLocalMap -> SearchReferencePointsInFrustum        src/cTracking.cpp:961-1017
//                 -> SearchByProjection(F, MPs)            src/cORBmatcher.cpp:67-166    (rule 0)
//   TrackPreviousFrame -> WindowSearch                     src/cORBmatcher.cpp:326-473   (rule 3)
// SearchForInitialization (rule 2) un-matches earlier queries: it stays with mcs_window_select.
#include "host_util.hpp"
#include "track_queries.hpp"
#include "track_select.hpp"
#include <algorithm>
#include <vector>

namespace mcs {
namespace trk {

constexpr int kQPB = 4;   // queries (waves) per 256-thread workgroup

struct WindowArgs {
  win::CandFrame f; int n_kp; int nq; int n_src;
  const double* q_xyr; const int32_t* q_cl; const int32_t* q_idx;
  const uint8_t* q_desc; const uint8_t* q_mask;
  int32_t* cand_ptr; int32_t* cand_kp; int32_t* cand_dist;
  const int64_t* status; int64_t cap;
};

// One wave per query: win::window_candidates with every grid value clamped.  COUNT: count
// only; else write (keypoint, distance) from cand_ptr[q], unless the total overflowed.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_track_window(WindowArgs a) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * kQPB + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  if (!COUNT && a.status[0] > a.cap) return;
  const double x = a.q_xyr[3 * q], y = a.q_xyr[3 * q + 1], r = a.q_xyr[3 * q + 2];
  int cam = a.q_cl[3 * q];
  const int minL = a.q_cl[3 * q + 1], maxL = a.q_cl[3 * q + 2];
  int src = a.q_idx ? a.q_idx[q] : q;
  if (src < 0 || src >= a.n_src) { cam = -1; src = 0; }
  const uint8_t* qd = a.q_desc + (int64_t)src * a.f.bytes;
  const uint8_t* qm = a.q_mask ? a.q_mask + (int64_t)src * a.f.bytes : nullptr;
  int base = 0, end = 0;
  if (!COUNT) {
    const int lim = (int)a.status[0];
    base = min(max(a.cand_ptr[q], 0), lim);
    end = min(max(a.cand_ptr[q + 1], base), lim);
  }
  const int cnt = win::window_candidates<COUNT, true>(a.f, lane, x, y, r, cam, minL, maxL, qd, qm,
                                                      a.n_kp, base, end, a.cand_kp, a.cand_dist);
  if (COUNT && lane == 0) a.cand_ptr[q + 1] = cnt;
}

}  // namespace trk
}  // namespace mcs

using namespace mcs;

struct mcs_track_workspace {
  int device = 0, max_kp = 0, max_q = 0;
  int64_t cand_cap = 0;
  int32_t* cursor = nullptr;            // [kMaxCams * 64 * 48] next free slot of every cell
  int32_t* tmp_kp = nullptr;            // [max_kp] cell lists before the rank sort
  int32_t* cand_ptr = nullptr;          // [max_q + 1]
  int32_t* cand_kp = nullptr;           // [cand_cap]
  int32_t* cand_dist = nullptr;         // [cand_cap]
  unsigned long long* mark = nullptr;   // [max_kp]
  int32_t* live = nullptr;              // [2][kMaxCams][max_q]
};

namespace {

template <class T> hipError_t ws_alloc(hipError_t e, T** p, size_t n) {
  return e != hipSuccess ? e : hipMalloc((void**)p, std::max<size_t>(1, n) * sizeof(T));
}

int check_rule(int rule, const char* who) {
  if (rule == 2) {
    set_error("track search: rule 2 (SearchForInitialization) runs on the host (mcs_window_select)");
    return MCS_ERR_UNSUPPORTED;
  }
  if (rule < 0 || rule > 3) return host::bad_arg(who);
  return MCS_OK;
}

// what the device and the host-buffer search entries check alike
int check_search(int rule, int n_cams, int n_kp, int bytes, bool kp_mask, const mcs_track_queries* q) {
  if (int rc = check_rule(rule, "track search: rule must be 0, 1 or 3")) return rc;
  if (!q || q->nq < 0 || q->n_src < 0 || n_kp < 0) return host::bad_arg("track search: bad argument");
  if (n_cams < 1 || n_cams > trk::kMaxCams) return host::bad_arg("track search: 1 to 8 cameras");
  if (int rc = host::check_desc_bytes(bytes, "track search")) return rc;
  if (q->nq > 0 && (!q->q_xyr || !q->q_cam_lvl || !q->q_desc_src))
    return host::bad_arg("track search: queries without q_xyr, q_cam_lvl or q_desc_src");
  if (q->nq > 0 && (q->q_mask_src == nullptr) != !kp_mask)
    return host::bad_arg("track search: query and keypoint masks must both be given or both be null");
  return MCS_OK;
}

int launch_select(mcs_track_workspace* ws, int rule, int nq, const int32_t* d_q_cl,
                  const int32_t* d_kp_oct, int n_kp, int n_cams, int th, double nnratio,
                  uint8_t* d_assigned, int32_t* d_match, int32_t* d_kp_query, int32_t* d_n_matches,
                  int64_t* d_status, hipStream_t st) {
  if (nq > 0) MCS_HIP_CHECK(hipMemsetAsync(d_match, 0xFF, (size_t)nq * sizeof(int32_t), st));
  if (n_kp > 0) {
    MCS_HIP_CHECK(hipMemsetAsync(d_kp_query, 0xFF, (size_t)n_kp * sizeof(int32_t), st));
    MCS_HIP_CHECK(hipMemsetAsync(ws->mark, 0, (size_t)n_kp * sizeof(unsigned long long), st));
  }
  MCS_HIP_CHECK(hipMemsetAsync(d_n_matches, 0, sizeof(int32_t), st));
  // the rounds of this call only: the flags' high half (little-endian) starts from zero
  MCS_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char*>(d_status + 1) + 4, 0, 4, st));
  if (nq > 0 && n_kp > 0) {
    trk::SelectArgs s{rule, nq, n_kp, th, ws->max_q, nnratio, ws->cand_cap, d_q_cl, ws->cand_ptr,
                      ws->cand_kp, ws->cand_dist, d_kp_oct, d_status, d_assigned, d_match, d_kp_query,
                      d_n_matches, ws->mark, ws->live};
    hipLaunchKernelGGL(trk::k_track_select, dim3(n_cams), dim3(trk::kSelThreads), 0, st, s);
  }
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int check_select_out(const mcs_track_workspace* ws, int nq, int n_kp, const void* assigned,
                     const void* match, const void* kp_query, const void* n_matches, const void* status) {
  if (!ws) return host::bad_arg("track search: no workspace");
  if (nq > ws->max_q || n_kp > ws->max_kp)
    return host::bad_arg("track search: nq or n_kp beyond the workspace");
  if (!n_matches || !status || (nq > 0 && !match) || (n_kp > 0 && (!assigned || !kp_query)))
    return host::bad_arg("track search: missing output");
  return MCS_OK;
}

}  // namespace

extern "C" {

int mcs_track_workspace_create(int32_t device, int32_t max_kp, int32_t max_queries, int64_t cand_cap,
                               mcs_track_workspace** out) {
  if (!out || max_kp < 1 || max_queries < 1 || cand_cap < 1 || cand_cap > INT32_MAX)
    return host::bad_arg("track workspace: bad argument");
  if (int rc = host::open_device(device, "track workspace")) return rc;
  mcs_track_workspace* w = new mcs_track_workspace;
  w->device = device;
  w->max_kp = max_kp;
  w->max_q = max_queries;
  w->cand_cap = cand_cap;
  hipError_t e = ws_alloc(hipSuccess, &w->cursor, (size_t)trk::kMaxCams * trk::kCellsPerCam);
  e = ws_alloc(e, &w->tmp_kp, (size_t)max_kp);
  e = ws_alloc(e, &w->cand_ptr, (size_t)max_queries + 1);
  e = ws_alloc(e, &w->cand_kp, (size_t)cand_cap);
  e = ws_alloc(e, &w->cand_dist, (size_t)cand_cap);
  e = ws_alloc(e, &w->mark, (size_t)max_kp);
  e = ws_alloc(e, &w->live, (size_t)2 * trk::kMaxCams * max_queries);
  if (e != hipSuccess) {
    mcs_track_workspace_destroy(w);
    set_hip_error(e, "track workspace", __FILE__, __LINE__);
    return MCS_ERR_HIP;
  }
  *out = w;
  return MCS_OK;
}

void mcs_track_workspace_destroy(mcs_track_workspace* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  void* all[] = {w->cursor, w->tmp_kp, w->cand_ptr, w->cand_kp, w->cand_dist, w->mark, w->live};
  for (void* p : all)
    if (p) (void)hipFree(p);
  delete w;
}

int mcs_frame_grid_build_device(mcs_track_workspace* ws, const float* d_kp_xy, const int32_t* d_kp_cam,
                                const int32_t* d_n_kp, int32_t cap, int32_t n_cams,
                                const double* d_gp, int32_t* d_cell_ptr, int32_t* d_cell_kp,
                                int32_t* d_n_in_grid, void* stream) {
  if (!ws || cap < 0 || n_cams < 1 || n_cams > trk::kMaxCams || !d_gp || !d_cell_ptr ||
      (cap > 0 && (!d_kp_xy || !d_kp_cam || !d_cell_kp)))
    return host::bad_arg("grid build: bad argument");
  if (cap > ws->max_kp) return host::bad_arg("grid build: cap beyond the workspace");
  hipStream_t st = (hipStream_t)stream;
  const int ncell = n_cams * trk::kCellsPerCam;
  MCS_HIP_CHECK(hipMemsetAsync(d_cell_ptr, 0, ((size_t)ncell + 1) * sizeof(int32_t), st));
  const unsigned g = (unsigned)((cap + 255) / 256);
  if (cap > 0)
    hipLaunchKernelGGL(trk::k_grid_count, dim3(g), dim3(256), 0, st, d_kp_xy, d_kp_cam, d_n_kp, cap,
                       n_cams, d_gp, d_cell_ptr);
  hipLaunchKernelGGL(trk::k_scan, dim3(1), dim3(1024), 0, st, d_cell_ptr, ncell, ws->cursor,
                     d_n_in_grid, (int64_t*)nullptr, (int64_t)0);
  if (cap > 0) {
    hipLaunchKernelGGL(trk::k_grid_place, dim3(g), dim3(256), 0, st, d_kp_xy, d_kp_cam, d_n_kp, cap,
                       n_cams, d_gp, ws->cursor, ws->tmp_kp);
    hipLaunchKernelGGL(trk::k_grid_sort, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, st,
                       (const int32_t*)d_cell_ptr, ncell, cap, (const int32_t*)ws->tmp_kp, d_cell_kp);
  }
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_track_unpack_keys_device(const mcs_keypoint* d_keys, const int32_t* d_n, int32_t cap,
                                 float* d_kp_xy, int32_t* d_kp_octave, void* stream) {
  if (cap < 0 || (cap > 0 && !d_keys)) return host::bad_arg("unpack keys: bad argument");
  if (cap == 0) return MCS_OK;
  hipLaunchKernelGGL(trk::k_unpack_keys, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, d_keys, d_n, cap, d_kp_xy, d_kp_octave);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_track_queries_mappoints_device(const uint8_t* d_in_view, const double* d_proj,
                                       const int32_t* d_level, const double* d_view_cos,
                                       const uint8_t* d_skip, int32_t n, int32_t n_cams,
                                       const double* d_scale, int32_t n_levels, double th,
                                       double* d_q_xyr, int32_t* d_q_cl, int32_t* d_q_idx, void* stream) {
  if (n < 0 || n_cams < 1 || n_cams > trk::kMaxCams || n_levels < 1 ||
      (n > 0 && (!d_in_view || !d_proj || !d_level || !d_view_cos || !d_scale || !d_q_xyr || !d_q_cl ||
                 !d_q_idx)))
    return host::bad_arg("track queries (map points): bad argument");
  const int64_t nq = (int64_t)n * n_cams;
  if (nq > INT32_MAX) return host::bad_arg("track queries (map points): too many queries");
  if (nq == 0) return MCS_OK;
  hipLaunchKernelGGL(trk::k_queries_mappoints, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, d_in_view, d_proj, d_level, d_view_cos, d_skip, n, n_cams,
                     d_scale, n_levels, th, d_q_xyr, d_q_cl, d_q_idx);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_track_queries_lastframe_device(const double* d_pose, const double* d_mc, const double* d_cam,
                                       int32_t n_cams, const uint8_t* d_masks, int32_t mask_w,
                                       int32_t mask_h, const double* d_pos, const uint8_t* d_valid,
                                       const int32_t* d_kp_cam, const int32_t* d_kp_octave,
                                       const int32_t* d_n, int32_t cap, const double* d_scale,
                                       int32_t n_levels, double th, double* d_q_xyr, int32_t* d_q_cl,
                                       int32_t* d_q_idx, void* stream) {
  if (cap < 0 || n_cams < 1 || n_cams > trk::kMaxCams || n_levels < 1 || mask_w < 1 || mask_h < 1 ||
      (cap > 0 && (!d_pose || !d_mc || !d_cam || !d_masks || !d_pos || !d_valid || !d_kp_cam ||
                   !d_kp_octave || !d_scale || !d_q_xyr || !d_q_cl || !d_q_idx)))
    return host::bad_arg("track queries (last frame): bad argument");
  if (cap == 0) return MCS_OK;
  hipLaunchKernelGGL(trk::k_queries_lastframe, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, d_pose, d_mc, d_cam, n_cams, d_masks, mask_w, mask_h, d_pos,
                     d_valid, d_kp_cam, d_kp_octave, d_n, cap, d_scale, n_levels, th, d_q_xyr, d_q_cl,
                     d_q_idx);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_track_search_device(mcs_track_workspace* ws, int32_t rule, const mcs_track_frame* f,
                            const mcs_track_queries* q, int32_t th_high, double nnratio,
                            uint8_t* d_kp_assigned, int32_t* d_match, int32_t* d_kp_query,
                            int32_t* d_n_matches, int64_t* d_status, void* stream) {
  if (!f) return host::bad_arg("track search: no frame");
  if (int rc = check_search(rule, f->n_cams, f->n_kp, f->bytes, f->desc_mask != nullptr, q)) return rc;
  if (int rc = check_select_out(ws, q->nq, f->n_kp, d_kp_assigned, d_match, d_kp_query, d_n_matches,
                                d_status)) return rc;
  if (q->nq > 0 && (!f->grid_params || !f->cell_ptr ||
                    (f->n_kp > 0 && (!f->cell_kp || !f->kp_xy || !f->kp_octave || !f->desc))))
    return host::bad_arg("track search: incomplete frame");
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  hipStream_t st = (hipStream_t)stream;
  const int nq = q->nq;
  trk::WindowArgs a{{f->cell_ptr, f->cell_kp, f->grid_params, f->n_cams, f->kp_xy, f->kp_octave, f->desc,
                     f->desc_mask, f->bytes},
                    f->n_kp, nq, q->n_src, q->q_xyr, q->q_cam_lvl, q->q_desc_idx, q->q_desc_src,
                    q->q_mask_src, ws->cand_ptr, ws->cand_kp, ws->cand_dist, d_status, ws->cand_cap};
  const unsigned g = (unsigned)((nq + trk::kQPB - 1) / trk::kQPB);
  if (nq > 0) hipLaunchKernelGGL(trk::k_track_window<true>, dim3(g), dim3(256), 0, st, a);
  hipLaunchKernelGGL(trk::k_scan, dim3(1), dim3(1024), 0, st, ws->cand_ptr, nq, (int32_t*)nullptr,
                     (int32_t*)nullptr, d_status, ws->cand_cap);
  if (nq > 0) hipLaunchKernelGGL(trk::k_track_window<false>, dim3(g), dim3(256), 0, st, a);
  MCS_HIP_CHECK(hipGetLastError());
  return launch_select(ws, rule, nq, q->q_cam_lvl, f->kp_octave, f->n_kp, f->n_cams, th_high, nnratio,
                       d_kp_assigned, d_match, d_kp_query, d_n_matches, d_status, st);
}

int mcs_track_select_device(mcs_track_workspace* ws, int32_t rule, int32_t nq, const int32_t* d_q_cl,
                            const int32_t* d_kp_octave, int32_t n_kp, int32_t n_cams, int32_t th_high,
                            double nnratio, uint8_t* d_kp_assigned, int32_t* d_match,
                            int32_t* d_kp_query, int32_t* d_n_matches, int64_t* d_status, void* stream) {
  if (int rc = check_rule(rule, "track select: rule must be 0, 1 or 3")) return rc;
  if (nq < 0 || n_kp < 0 || n_cams < 1 || n_cams > trk::kMaxCams ||
      (nq > 0 && n_kp > 0 && (!d_q_cl || !d_kp_octave)))
    return host::bad_arg("track select: bad argument");
  if (int rc = check_select_out(ws, nq, n_kp, d_kp_assigned, d_match, d_kp_query, d_n_matches, d_status))
    return rc;
  MCS_HIP_CHECK(hipSetDevice(ws->device));
  return launch_select(ws, rule, nq, d_q_cl, d_kp_octave, n_kp, n_cams, th_high, nnratio, d_kp_assigned,
                       d_match, d_kp_query, d_n_matches, d_status, (hipStream_t)stream);
}

int mcs_track_search(int32_t device, int32_t rule, const mcs_window_frame* f, const mcs_track_queries* q,
                     int32_t th_high, double nnratio, uint8_t* kp_assigned, int32_t* match,
                     int32_t* kp_query, int32_t* n_matches) {
  if (!f || !f->grid_params || !n_matches) return host::bad_arg("track search: bad argument");
  if (int rc = check_search(rule, f->n_cams, f->n_kp, f->bytes, f->desc_mask != nullptr, q)) return rc;
  if (f->n_kp > 0 && (!f->kp_xy || !f->kp_cam || !f->kp_octave || !f->desc))
    return host::bad_arg("track search: incomplete frame");
  if (q->nq > 0 && !match) return host::bad_arg("track search: missing output");
  if (q->q_desc_idx == nullptr && q->n_src < q->nq) return host::bad_arg("track search: n_src below nq");
  if (int rc = host::open_device(device, "track search")) return rc;
  const size_t nk = (size_t)f->n_kp, nb = (size_t)f->bytes, nq = (size_t)q->nq, C = (size_t)f->n_cams;
  host::DevBufs B;
  mcs_track_frame df{f->n_cams, f->n_kp, f->bytes};
  df.grid_params = B.up(f->grid_params, 4 * C);
  df.kp_xy = B.up(f->kp_xy, 2 * nk);
  df.kp_octave = B.up(f->kp_octave, nk);
  df.desc = B.up(f->desc, nk * nb);
  df.desc_mask = B.up(f->desc_mask, nk * nb);
  const int32_t* d_cam = B.up(f->kp_cam, nk);
  int32_t* d_cptr = B.alloc<int32_t>(C * trk::kCellsPerCam + 1);
  int32_t* d_ckp = B.alloc<int32_t>(nk);
  df.cell_ptr = d_cptr;
  df.cell_kp = d_ckp;
  mcs_track_queries dq{q->nq, q->n_src};
  dq.q_xyr = B.up(q->q_xyr, 3 * nq);
  dq.q_cam_lvl = B.up(q->q_cam_lvl, 3 * nq);
  dq.q_desc_idx = B.up(q->q_desc_idx, nq);
  dq.q_desc_src = B.up(q->q_desc_src, (size_t)q->n_src * nb);
  dq.q_mask_src = B.up(q->q_mask_src, (size_t)q->n_src * nb);
  std::vector<uint8_t> fresh;
  if (!kp_assigned) { fresh.assign(std::max<size_t>(1, nk), 0); kp_assigned = fresh.data(); }
  uint8_t* d_as = B.up(kp_assigned, nk);
  int32_t* d_match = B.alloc<int32_t>(nq);
  int32_t* d_kq = B.alloc<int32_t>(nk);
  int32_t* d_nm = B.alloc<int32_t>(1);
  int64_t* d_status = B.alloc<int64_t>(2);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track search upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  int64_t cap = std::max<int64_t>(1024, 32 * (int64_t)q->nq), status[2] = {0, 0};
  for (int pass = 0; pass < 2; pass++) {   // the second pass has the capacity the first one asked for
    mcs_track_workspace* ws = nullptr;
    int rc = mcs_track_workspace_create(device, std::max(1, f->n_kp), std::max(1, q->nq), cap, &ws);
    if (rc) return rc;
    if (pass == 0)
      rc = mcs_frame_grid_build_device(ws, df.kp_xy, d_cam, nullptr, f->n_kp, f->n_cams, df.grid_params,
                                       d_cptr, d_ckp, nullptr, nullptr);
    if (!rc)
      rc = mcs_track_search_device(ws, rule, &df, &dq, th_high, nnratio, d_as, d_match, d_kq, d_nm,
                                   d_status, nullptr);
    hipError_t e = hipMemcpy(status, d_status, sizeof status, hipMemcpyDeviceToHost);   // waits for the kernels
    mcs_track_workspace_destroy(ws);
    if (rc) return rc;
    MCS_HIP_CHECK(e);
    if (!(status[1] & MCS_TRACK_OVERFLOW)) break;
    if (pass == 1 || status[0] > INT32_MAX) {
      set_error("track search: candidate lists too large");
      return MCS_ERR_CAPACITY;
    }
    cap = status[0];
  }
  B.down(kp_assigned, (const uint8_t*)d_as, nk);
  B.down(match, (const int32_t*)d_match, nq);
  B.down(kp_query, (const int32_t*)d_kq, nk);
  B.down(n_matches, (const int32_t*)d_nm, (size_t)1);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track search download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

int mcs_track_queries_mappoints(int32_t device, const uint8_t* in_view, const double* proj,
                                const int32_t* level, const double* view_cos, const uint8_t* skip,
                                int32_t n, int32_t n_cams, const double* scale, int32_t n_levels,
                                double th, double* q_xyr, int32_t* q_cl, int32_t* q_idx) {
  if (n < 0 || n_cams < 1 || n_cams > trk::kMaxCams || n_levels < 1 ||
      (n > 0 && (!in_view || !proj || !level || !view_cos || !scale || !q_xyr || !q_cl || !q_idx)))
    return host::bad_arg("track queries (map points): bad argument");
  if (int rc = host::open_device(device, "track queries")) return rc;
  const size_t nq = (size_t)n * n_cams;
  host::DevBufs B;
  const uint8_t* d_iv = B.up(in_view, nq);
  const double* d_pj = B.up(proj, 2 * nq);
  const int32_t* d_lv = B.up(level, nq);
  const double* d_vc = B.up(view_cos, nq);
  const uint8_t* d_sk = B.up(skip, (size_t)n);
  const double* d_sc = B.up(scale, (size_t)n_levels);
  double* d_q = B.alloc<double>(3 * nq);
  int32_t* d_cl = B.alloc<int32_t>(3 * nq);
  int32_t* d_ix = B.alloc<int32_t>(nq);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track queries upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (int rc = mcs_track_queries_mappoints_device(d_iv, d_pj, d_lv, d_vc, d_sk, n, n_cams, d_sc, n_levels,
                                                  th, d_q, d_cl, d_ix, nullptr)) return rc;
  B.down(q_xyr, (const double*)d_q, 3 * nq);
  B.down(q_cl, (const int32_t*)d_cl, 3 * nq);
  B.down(q_idx, (const int32_t*)d_ix, nq);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track queries download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

int mcs_track_queries_lastframe(int32_t device, const double* pose, const double* mc, const double* cam,
                                int32_t n_cams, const uint8_t* masks, int32_t mask_w, int32_t mask_h,
                                const double* pos, const uint8_t* valid, const int32_t* kp_cam,
                                const int32_t* kp_octave, int32_t n, const double* scale,
                                int32_t n_levels, double th, double* q_xyr, int32_t* q_cl, int32_t* q_idx) {
  if (n < 0 || n_cams < 1 || n_cams > trk::kMaxCams || n_levels < 1 || mask_w < 1 || mask_h < 1 ||
      (n > 0 && (!pose || !mc || !cam || !masks || !pos || !valid || !kp_cam || !kp_octave || !scale ||
                 !q_xyr || !q_cl || !q_idx)))
    return host::bad_arg("track queries (last frame): bad argument");
  if (int rc = host::open_device(device, "track queries")) return rc;
  const size_t ns = (size_t)n, C = (size_t)n_cams;
  host::DevBufs B;
  const double* d_po = B.up(pose, (size_t)6);
  const double* d_mc = B.up(mc, 6 * C);
  const double* d_cm = B.up(cam, 17 * C);
  const uint8_t* d_mk = B.up(masks, C * mask_w * mask_h);
  const double* d_ps = B.up(pos, 3 * ns);
  const uint8_t* d_va = B.up(valid, ns);
  const int32_t* d_kc = B.up(kp_cam, ns);
  const int32_t* d_ko = B.up(kp_octave, ns);
  const double* d_sc = B.up(scale, (size_t)n_levels);
  double* d_q = B.alloc<double>(3 * ns);
  int32_t* d_cl = B.alloc<int32_t>(3 * ns);
  int32_t* d_ix = B.alloc<int32_t>(ns);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track queries upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  if (int rc = mcs_track_queries_lastframe_device(d_po, d_mc, d_cm, n_cams, d_mk, mask_w, mask_h, d_ps, d_va,
                                                  d_kc, d_ko, nullptr, n, d_sc, n_levels, th, d_q, d_cl,
                                                  d_ix, nullptr)) return rc;
  B.down(q_xyr, (const double*)d_q, 3 * ns);
  B.down(q_cl, (const int32_t*)d_cl, 3 * ns);
  B.down(q_idx, (const int32_t*)d_ix, ns);
  if (B.err != hipSuccess) { set_hip_error(B.err, "track queries download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  return MCS_OK;
}

}  // extern "C"
