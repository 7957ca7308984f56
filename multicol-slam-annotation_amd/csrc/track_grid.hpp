// The cMultiFrame feature grid on the device (track_match.hip): mcs_frame_grid_build's CSR
// lists from device keypoints, and the unpacking of mvKeys rows.
//
// Reference: grid build src/cMultiFrame.cpp:154-184, PosInGrid :342-353.  The cell of a
// keypoint is the host entry's arithmetic word for word (window_host.cpp): float subtraction,
// cvRound (ties to even) of the double product.  Counting uses atomics (counts are order-free);
// placing uses them too and a rank sort of every cell then restores ascending keypoint index,
// the reference's push_back order, so the lists do not depend on scheduling.
#pragma once
#include "window_walk.hpp"

namespace mcs {
namespace trk {

constexpr int kMaxCams = MCS_TRACK_MAX_CAMS;
constexpr int kCellsPerCam = win::kCols * win::kRows;

__device__ __forceinline__ int clamped_count(const int32_t* d_n, int cap) {
  return d_n ? min(max(*d_n, 0), cap) : cap;
}

// cell of keypoint i, or -1 when PosInGrid fails or the camera is outside the rig.  Equal to the
// host entry while the product fits an int: past that the host's (int)lrint wraps a long where
// this conversion saturates (and drops the keypoint); image coordinates are nowhere near.
__device__ __forceinline__ int grid_cell(const float* kp_xy, const int32_t* kp_cam, const double* gp,
                                         int n_cams, int i) {
  const int c = kp_cam[i];
  if (c < 0 || c >= n_cams) return -1;
  const float fx = kp_xy[2 * i] - (float)gp[4 * c], fy = kp_xy[2 * i + 1] - (float)gp[4 * c + 1];
  const int px = (int)rint((double)fx * gp[4 * c + 2]);
  const int py = (int)rint((double)fy * gp[4 * c + 3]);
  if (px < 0 || px >= win::kCols || py < 0 || py >= win::kRows) return -1;
  return (c * win::kCols + px) * win::kRows + py;
}

// cell_ptr (zeroed) [cell + 1] += 1
__global__ __launch_bounds__(256) void k_grid_count(const float* __restrict__ kp_xy,
                                                    const int32_t* __restrict__ kp_cam,
                                                    const int32_t* __restrict__ d_n, int cap,
                                                    int n_cams, const double* __restrict__ gp,
                                                    int32_t* __restrict__ cell_ptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= clamped_count(d_n, cap)) return;
  const int cell = grid_cell(kp_xy, kp_cam, gp, n_cams, i);
  if (cell >= 0) atomicAdd(&cell_ptr[cell + 1], 1);
}

// in-place inclusive scan of p[1..n] (p[0] = 0), one workgroup, fixed order; cursor[i] = p[i]
// (nullable), *total32 / *total64 (nullable) = p[n]
__global__ __launch_bounds__(1024) void k_scan(int32_t* __restrict__ p, int n,
                                               int32_t* __restrict__ cursor,
                                               int32_t* __restrict__ total32,
                                               int64_t* __restrict__ total64, int64_t cap) {
  __shared__ int64_t carry;
  __shared__ int part[1024 / 64 + 1];
  if (threadIdx.x == 0) { carry = 0; p[0] = 0; }
  __syncthreads();
  for (int b = 0; b < n; b += 1024) {
    const int i = b + (int)threadIdx.x;
    const int v = i < n ? p[i + 1] : 0;
    int tot;
    const int ex = dev::block_excl_scan<1024>(v, part, &tot);
    if (i < n) {
      p[i + 1] = (int32_t)(carry + ex + v);
      if (cursor) cursor[i] = (int32_t)(carry + ex);
    }
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (total32) *total32 = (int32_t)carry;
    if (total64) { total64[0] = carry; total64[1] = carry > cap ? MCS_TRACK_OVERFLOW : 0; }
  }
}

// tmp[cursor[cell]++] = i: every cell's keypoints in its range of tmp, in any order
__global__ __launch_bounds__(256) void k_grid_place(const float* __restrict__ kp_xy,
                                                    const int32_t* __restrict__ kp_cam,
                                                    const int32_t* __restrict__ d_n, int cap,
                                                    int n_cams, const double* __restrict__ gp,
                                                    int32_t* __restrict__ cursor,
                                                    int32_t* __restrict__ tmp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= clamped_count(d_n, cap)) return;
  const int cell = grid_cell(kp_xy, kp_cam, gp, n_cams, i);
  if (cell < 0) return;
  const int pos = atomicAdd(&cursor[cell], 1);
  if (pos >= 0 && pos < cap) tmp[pos] = i;
}

// one wave per cell: the rank of a keypoint index among the cell's (all different) is its place
__global__ __launch_bounds__(256) void k_grid_sort(const int32_t* __restrict__ cell_ptr, int ncell,
                                                   int cap, const int32_t* __restrict__ tmp,
                                                   int32_t* __restrict__ cell_kp) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= ncell) return;
  const int s = min(max(cell_ptr[cell], 0), cap);
  const int len = min(max(cell_ptr[cell + 1] - s, 0), cap - s);
  for (int j = lane; j < len; j += 64) {
    const int v = tmp[s + j];
    int rank = 0;
    for (int t = 0; t < len; t++) rank += tmp[s + t] < v;
    cell_kp[s + rank] = v;
  }
}

// mvKeys rows -> pt and octave
__global__ __launch_bounds__(256) void k_unpack_keys(const mcs_keypoint* __restrict__ keys,
                                                     const int32_t* __restrict__ d_n, int cap,
                                                     float* __restrict__ kp_xy,
                                                     int32_t* __restrict__ kp_oct) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= clamped_count(d_n, cap)) return;
  const mcs_keypoint kp = keys[i];
  if (kp_xy) { kp_xy[2 * i] = kp.x; kp_xy[2 * i + 1] = kp.y; }
  if (kp_oct) kp_oct[i] = kp.octave;
}

}  // namespace trk
}  // namespace mcs
