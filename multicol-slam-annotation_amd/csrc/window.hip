// Projection-guided (windowed) matching: the cMultiFrame feature grid on the host, then
// GetFeaturesInArea and the Hamming distance of every window candidate on the device, then the
// reference's sequential best / second-best selection rules on the host.  The two host steps
// (mcs_frame_grid_build, mcs_window_select) are window_host.cpp.
//
// Reference (billamiable/MultiCol-SLAM-Annotation):
//   grid build (part of the cMultiFrame ctor)            src/cMultiFrame.cpp:154-184
//   PosInGrid                                            src/cMultiFrame.cpp:342-353
//   GetFeaturesInArea                                    src/cMultiFrame.cpp:272-340
//   SearchByProjection(F, MPs)       (rule 0)            src/cORBmatcher.cpp:67-166
//   SearchByProjection(Cur, Last)    (rule 1)            src/cORBmatcher.cpp:1991-2123
//   SearchForInitialization          (rule 2)            src/cORBmatcher.cpp:579-726
//   WindowSearch                     (rule 3)            src/cORBmatcher.cpp:326-473
//   DescriptorDistance64[Masked]                         src/cORBmatcher.cpp:2443-2477
// checkOrientation is false in the reference (include/cORBmatcher.h:40), so no rotation
// histograms.  GetFeaturesInArea's abs(kp.pt.x - x) is the double overload (the operand is a
// double), i.e. fabs.
#include "host_util.hpp"
#include "window_walk.hpp"
#include "../../include/mcs_matcher.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace mcs {
namespace win {

constexpr int kQPB = 4;   // queries (waves) per 256-thread workgroup

struct SearchArgs {
  const int32_t* cell_ptr; const int32_t* cell_kp; const double* gp; int n_cams;
  const float* kp_xy; const int32_t* kp_oct; const uint8_t* kp_desc; const uint8_t* kp_mask;
  int bytes; int nq;
  const double* q_xyr; const int32_t* q_cl; const uint8_t* q_desc; const uint8_t* q_mask;
  int32_t* cand_ptr; int32_t* cand_kp; int32_t* cand_dist;
};

// One wave per query: win::window_candidates (window_walk.hpp), the grid taken as given.
// COUNT: count only; else write (keypoint, distance) from cand_ptr[q].
template <bool COUNT>
__global__ __launch_bounds__(256) void k_window(SearchArgs a) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * kQPB + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  const double x = a.q_xyr[3 * q], y = a.q_xyr[3 * q + 1], r = a.q_xyr[3 * q + 2];
  const int cam = a.q_cl[3 * q], minL = a.q_cl[3 * q + 1], maxL = a.q_cl[3 * q + 2];
  const CandFrame f{a.cell_ptr, a.cell_kp, a.gp, a.n_cams, a.kp_xy, a.kp_oct, a.kp_desc, a.kp_mask,
                    a.bytes};
  const uint8_t* qd = a.q_desc + (int64_t)q * a.bytes;
  const uint8_t* qm = a.q_mask ? a.q_mask + (int64_t)q * a.bytes : nullptr;
  const int cnt = window_candidates<COUNT, false>(f, lane, x, y, r, cam, minL, maxL, qd, qm, 0,
                                                  COUNT ? 0 : a.cand_ptr[q], 0, a.cand_kp,
                                                  a.cand_dist);
  if (COUNT && lane == 0) a.cand_ptr[q + 1] = cnt;
}

// in-place inclusive scan of cand_ptr[1..nq] (cand_ptr[0] = 0), one workgroup, fixed order
__global__ __launch_bounds__(1024) void k_scan(int32_t* p, int nq, int64_t* total) {
  __shared__ int64_t carry;
  __shared__ int part[1024 / 64 + 1];
  if (threadIdx.x == 0) { carry = 0; p[0] = 0; }
  __syncthreads();
  for (int b = 0; b < nq; b += 1024) {
    const int i = b + (int)threadIdx.x;
    const int v = i < nq ? p[i + 1] : 0;
    int tot;
    const int ex = dev::block_excl_scan<1024>(v, part, &tot);
    if (i < nq) p[i + 1] = (int32_t)(carry + ex + v);
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

}  // namespace win
}  // namespace mcs

using namespace mcs;

extern "C" {

int mcs_window_search_device(const int32_t* d_cell_ptr, const int32_t* d_cell_kp,
                             const double* d_grid_params, int32_t n_cams, const float* d_kp_xy,
                             const int32_t* d_kp_octave, const uint8_t* d_kp_desc,
                             const uint8_t* d_kp_mask, int32_t bytes, int32_t nq,
                             const double* d_q_xyr, const int32_t* d_q_cam_lvl,
                             const uint8_t* d_q_desc, const uint8_t* d_q_mask,
                             int32_t* d_cand_ptr, int32_t* d_cand_kp, int32_t* d_cand_dist,
                             int64_t cap, int64_t* total, void* stream) {
  if (!total || nq < 0 || n_cams < 1) return MCS_ERR_ARG;
  if (int rc = host::check_desc_bytes(bytes, "window search")) return rc;
  if (!d_cand_ptr || (nq > 0 && (!d_q_xyr || !d_q_cam_lvl || !d_q_desc || !d_grid_params ||
                                 !d_cell_ptr))) return MCS_ERR_ARG;
  if ((d_q_mask == nullptr) != (d_kp_mask == nullptr)) {
    set_error("window search: query and keypoint masks must both be given or both be null");
    return MCS_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  win::SearchArgs a{d_cell_ptr, d_cell_kp, d_grid_params, n_cams, d_kp_xy, d_kp_octave, d_kp_desc,
                    d_kp_mask, bytes, nq, d_q_xyr, d_q_cam_lvl, d_q_desc, d_q_mask, d_cand_ptr,
                    d_cand_kp, d_cand_dist};
  int64_t* d_total = nullptr;
  MCS_HIP_CHECK(hipMalloc((void**)&d_total, sizeof(int64_t)));
  const unsigned g = (unsigned)((nq + win::kQPB - 1) / win::kQPB);
  if (nq > 0) hipLaunchKernelGGL(win::k_window<true>, dim3(g), dim3(256), 0, st, a);
  hipLaunchKernelGGL(win::k_scan, dim3(1), dim3(1024), 0, st, d_cand_ptr, nq, d_total);
  int64_t tot = 0;
  hipError_t e = hipMemcpyAsync(&tot, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_total);
  MCS_HIP_CHECK(e);
  *total = tot;
  if (tot > cap || (tot > 0 && (!d_cand_kp || !d_cand_dist))) {
    set_error("window search: candidate capacity too small (required size in *total)");
    return MCS_ERR_CAPACITY;
  }
  if (nq > 0 && tot > 0) hipLaunchKernelGGL(win::k_window<false>, dim3(g), dim3(256), 0, st, a);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_window_match(int32_t device, int32_t rule, const mcs_window_frame* f, int32_t nq,
                     const double* q_xyr, const int32_t* q_cam_lvl, const uint8_t* q_desc,
                     const uint8_t* q_mask, int32_t th, double nnratio, uint8_t* kp_assigned,
                     int32_t* match, int32_t* n_matches) {
  if (!f || f->n_cams < 1 || f->n_kp < 0 || nq < 0 || !f->grid_params || !match || !n_matches)
    return MCS_ERR_ARG;
  if (f->n_kp > 0 && (!f->kp_xy || !f->kp_cam || !f->kp_octave || !f->desc)) return MCS_ERR_ARG;
  if (nq > 0 && (!q_xyr || !q_cam_lvl || !q_desc)) return MCS_ERR_ARG;
  int rc = host::open_device(device, "window match");
  if (rc) return rc;
  const int ncell = f->n_cams * win::kCols * win::kRows;
  std::vector<int32_t> cell_ptr(ncell + 1), cell_kp(std::max(1, f->n_kp));
  rc = mcs_frame_grid_build(f->kp_xy, f->kp_cam, f->n_kp, f->n_cams, f->grid_params,
                                cell_ptr.data(), cell_kp.data(), nullptr);
  if (rc) return rc;
  const size_t nk = (size_t)f->n_kp, nb = (size_t)f->bytes, nqs = (size_t)nq;
  host::DevBufs B;
  const double* d_gp = B.up(f->grid_params, 4 * (size_t)f->n_cams);
  const int32_t* d_cptr = B.up(cell_ptr.data(), cell_ptr.size());
  const int32_t* d_ckp = B.up(cell_kp.data(), (size_t)cell_ptr[ncell]);
  const float* d_xy = B.up(f->kp_xy, 2 * nk);
  const int32_t* d_oct = B.up(f->kp_octave, nk);
  const uint8_t* d_desc = B.up(f->desc, nk * nb);
  const uint8_t* d_mask = B.up(f->desc_mask, nk * nb);
  const double* d_q = B.up(q_xyr, 3 * nqs);
  const int32_t* d_ql = B.up(q_cam_lvl, 3 * nqs);
  const uint8_t* d_qd = B.up(q_desc, nqs * nb);
  const uint8_t* d_qm = B.up(q_mask, nqs * nb);
  int32_t* d_cp = B.alloc<int32_t>(nqs + 1);
  int64_t cap = std::max<int64_t>(1024, 32 * (int64_t)nq), total = 0;
  int32_t* d_ck = B.alloc<int32_t>((size_t)cap);
  int32_t* d_cd = B.alloc<int32_t>((size_t)cap);
  if (B.err != hipSuccess) { set_hip_error(B.err, "window match upload", __FILE__, __LINE__); return MCS_ERR_HIP; }
  rc = mcs_window_search_device(d_cptr, d_ckp, d_gp, f->n_cams, d_xy, d_oct, d_desc, d_mask, f->bytes,
                                nq, d_q, d_ql, d_qd, d_qm, d_cp, d_ck, d_cd, cap, &total, nullptr);
  if (rc == MCS_ERR_CAPACITY) {
    cap = total;
    d_ck = B.alloc<int32_t>((size_t)cap);
    d_cd = B.alloc<int32_t>((size_t)cap);
    if (B.err != hipSuccess) { set_hip_error(B.err, "window match alloc", __FILE__, __LINE__); return MCS_ERR_HIP; }
    rc = mcs_window_search_device(d_cptr, d_ckp, d_gp, f->n_cams, d_xy, d_oct, d_desc, d_mask, f->bytes,
                                  nq, d_q, d_ql, d_qd, d_qm, d_cp, d_ck, d_cd, cap, &total, nullptr);
  }
  if (rc) return rc;
  std::vector<int32_t> cp(nqs + 1), ck(std::max<int64_t>(1, total)), cd(std::max<int64_t>(1, total));
  B.down(cp.data(), d_cp, nqs + 1);
  B.down(ck.data(), d_ck, (size_t)total);
  B.down(cd.data(), d_cd, (size_t)total);
  if (B.err != hipSuccess) { set_hip_error(B.err, "window match download", __FILE__, __LINE__); return MCS_ERR_HIP; }
  std::vector<uint8_t> fresh;
  if (!kp_assigned) { fresh.assign(std::max(1, f->n_kp), 0); kp_assigned = fresh.data(); }
  return mcs_window_select(rule, nq, cp.data(), ck.data(), cd.data(), f->kp_octave, f->n_kp, th,
                           nnratio, kp_assigned, match, n_matches);
}

}  // extern "C"
