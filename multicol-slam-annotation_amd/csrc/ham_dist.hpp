// Descriptor distances and tile sizes shared by the matcher translation units (hamming.hip,
// tri_search.hip, bow_match.hip).  A descriptor row of W dwords (16, 32 or 64 bytes) is read with
// 16-byte vector loads.
#pragma once
#include "common.hpp"

namespace mcs {

constexpr int kHamThreads = 256;
constexpr int kHamTile = 256;      // train rows per LDS tile

// DescriptorDistance64 (src/cORBmatcher.cpp:2443-2455)
template <int W>
__device__ __forceinline__ int ham_dist_v(const uint32_t (&q)[W], const uint4* t4) {
  int d = 0;
#pragma unroll
  for (int w4 = 0; w4 < W / 4; w4++) {
    const uint4 v = t4[w4];
    d += __popc(q[4 * w4 + 0] ^ v.x);
    d += __popc(q[4 * w4 + 1] ^ v.y);
    d += __popc(q[4 * w4 + 2] ^ v.z);
    d += __popc(q[4 * w4 + 3] ^ v.w);
  }
  return d;
}

// DescriptorDistance64Masked (src/cORBmatcher.cpp:2457-2477): (sum popc(x & m1) +
// sum popc(x & m2)) / 2 over the whole descriptor, integer division of the total.
template <int W>
__device__ __forceinline__ int ham_dist_masked_v(const uint32_t (&q)[W], const uint32_t (&qm)[W],
                                                 const uint4* t4, const uint4* m4) {
  int d = 0;
#pragma unroll
  for (int w4 = 0; w4 < W / 4; w4++) {
    const uint4 v = t4[w4], m = m4[w4];
    const uint32_t x0 = q[4 * w4 + 0] ^ v.x, x1 = q[4 * w4 + 1] ^ v.y;
    const uint32_t x2 = q[4 * w4 + 2] ^ v.z, x3 = q[4 * w4 + 3] ^ v.w;
    d += __popc(x0 & qm[4 * w4 + 0]) + __popc(x0 & m.x);
    d += __popc(x1 & qm[4 * w4 + 1]) + __popc(x1 & m.y);
    d += __popc(x2 & qm[4 * w4 + 2]) + __popc(x2 & m.z);
    d += __popc(x3 & qm[4 * w4 + 3]) + __popc(x3 & m.w);
  }
  return d >> 1;
}

template <int W>
__device__ __forceinline__ void load_desc_row(uint32_t (&q)[W], const uint8_t* row) {
  const uint4* qp = reinterpret_cast<const uint4*>(row);
#pragma unroll
  for (int w4 = 0; w4 < W / 4; w4++) {
    const uint4 v = qp[w4];
    q[4 * w4] = v.x; q[4 * w4 + 1] = v.y; q[4 * w4 + 2] = v.z; q[4 * w4 + 3] = v.w;
  }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

}  // namespace mcs
