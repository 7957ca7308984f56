// Hamming matching on gfx950: XOR + v_bcnt_u32_b32 popcount-accumulate, trains staged in
// LDS and broadcast to a wave of 64 queries (one query per lane, descriptor in VGPRs), and the
// 32-byte top-2 on the FP4 matrix cores.  SearchForTriangulationRaw is tri_search.hip, the
// ComputeE rig geometry epipolar.cpp.
//
// Reference: DescriptorDistance64 / ...Masked   src/cORBmatcher.cpp:2443-2477
//            best/second-best scans             src/cORBmatcher.cpp:67-163, 326-475
#include "host_util.hpp"
#include "ham_dist.hpp"
#include "top2_net.hpp"
#include "../../include/mcs_matcher.h"

namespace mcs {

// Top-2 over one (query set, train set) pair; blockIdx.x = query tile, blockIdx.y = pair.
// Each lane owns kQPT queries (descriptors in VGPRs) so one LDS broadcast read of a train
// row feeds kQPT distances.  The running best/second-best are kept as packed keys
// (dist << 16 | train index): trains are scanned in index order, so the strict-< rule of the
// reference scans (first minimum wins, :2447) equals "two smallest keys", maintained four keys
// at a time with v_min3_u32 / v_med3_u32 (top2_net.hpp; best <= second always).
constexpr int kQPT = 2;

// popcount-accumulate as one v_bcnt_u32_b32 (the compiler otherwise reassociates the sum
// into bcnt(x, 0) + v_add3 chains, 25 % more VALU)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

template <int W>
__global__ __launch_bounds__(kHamThreads) void k_top2(
    const uint8_t* __restrict__ qbase, const uint8_t* __restrict__ tbase,
    const int32_t* __restrict__ counts, const int32_t* __restrict__ pairs, int64_t set_stride,
    int nq_fixed, int nt_fixed, int cap_out, int32_t* __restrict__ best_idx,
    int32_t* __restrict__ best_dist, int32_t* __restrict__ second_idx,
    int32_t* __restrict__ second_dist) {
  __shared__ uint4 tile[kHamTile * (W / 4)];
  const int p = blockIdx.y;
  const uint8_t* Q;
  const uint8_t* T;
  int nq, nt;
  if (pairs) {
    const int qs = pairs[2 * p], ts = pairs[2 * p + 1];
    Q = qbase + (int64_t)qs * set_stride;
    T = tbase + (int64_t)ts * set_stride;
    nq = counts[qs];
    nt = counts[ts];
  } else {
    Q = qbase; T = tbase; nq = nq_fixed; nt = nt_fixed;
  }
  const int q0 = blockIdx.x * (kHamThreads * kQPT);
  if (q0 >= nq) return;  // uniform per block
  uint32_t q[kQPT][W];
#pragma unroll
  for (int k = 0; k < kQPT; k++) {
    const int qi = q0 + k * kHamThreads + threadIdx.x;
    if (qi < nq) {
      const uint4* qp = reinterpret_cast<const uint4*>(Q + (int64_t)qi * W * 4);
#pragma unroll
      for (int w4 = 0; w4 < W / 4; w4++) {
        const uint4 v = qp[w4];
        q[k][4 * w4] = v.x; q[k][4 * w4 + 1] = v.y; q[k][4 * w4 + 2] = v.z; q[k][4 * w4 + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int w = 0; w < W; w++) q[k][w] = 0;
    }
  }
  uint32_t k1[kQPT], k2[kQPT];
#pragma unroll
  for (int k = 0; k < kQPT; k++) { k1[k] = 0xFFFFFFFFu; k2[k] = 0xFFFFFFFFu; }
  for (int t0 = 0; t0 < nt; t0 += kHamTile) {
    const int nt_tile = min(kHamTile, nt - t0);
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(T + (int64_t)t0 * W * 4);
    for (int i = threadIdx.x; i < nt_tile * (W / 4); i += kHamThreads) tile[i] = src[i];
    __syncthreads();
    // the keys of train row j of the tile against this lane's kQPT queries
    auto keys_of = [&](int j, uint32_t (&key)[kQPT]) {
      const uint4* tr = &tile[j * (W / 4)];
      const uint32_t idx = (uint32_t)(t0 + j);
      uint32_t d[kQPT];
#pragma unroll
      for (int k = 0; k < kQPT; k++) d[k] = 0;
#pragma unroll
      for (int w4 = 0; w4 < W / 4; w4++) {
        const uint4 v = tr[w4];
#pragma unroll
        for (int k = 0; k < kQPT; k++) {
          d[k] = bcnt_acc(q[k][4 * w4 + 0] ^ v.x, d[k]);
          d[k] = bcnt_acc(q[k][4 * w4 + 1] ^ v.y, d[k]);
          d[k] = bcnt_acc(q[k][4 * w4 + 2] ^ v.z, d[k]);
          d[k] = bcnt_acc(q[k][4 * w4 + 3] ^ v.w, d[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < kQPT; k++) key[k] = (d[k] << 16) | idx;
    };
    int j = 0;
    for (; j + 4 <= nt_tile; j += 4) {
      uint32_t ka[kQPT], kb[kQPT], kc[kQPT], kd[kQPT];
      keys_of(j, ka); keys_of(j + 1, kb); keys_of(j + 2, kc); keys_of(j + 3, kd);
#pragma unroll
      for (int k = 0; k < kQPT; k++) top2_update4(k1[k], k2[k], ka[k], kb[k], kc[k], kd[k]);
    }
    for (; j < nt_tile; j++) {
      uint32_t ka[kQPT];
      keys_of(j, ka);
#pragma unroll
      for (int k = 0; k < kQPT; k++) top2_update1(k1[k], k2[k], ka[k]);
    }
  }
  const int none = 8 * 4 * W + 1;
#pragma unroll
  for (int k = 0; k < kQPT; k++) {
    const int qi = q0 + k * kHamThreads + threadIdx.x;
    if (qi < nq) {
      const int64_t o = (int64_t)p * cap_out + qi;
      const bool h1 = k1[k] != 0xFFFFFFFFu, h2 = k2[k] != 0xFFFFFFFFu;
      best_idx[o] = h1 ? (int)(k1[k] & 0xFFFF) : -1;
      best_dist[o] = h1 ? (int)(k1[k] >> 16) : none;
      second_idx[o] = h2 ? (int)(k2[k] & 0xFFFF) : -1;
      second_dist[o] = h2 ? (int)(k2[k] >> 16) : none;
    }
  }
}

// ---------------------------------------------------------------------------
// 32-byte descriptors on the FP4 matrix cores: a descriptor bit becomes one FP4 e2m1 element,
// +1.0 (nibble 0b0010) for a clear bit and -1.0 (0b1010) for a set one, and the query side is
// complemented, so a bit position adds +1 where the two descriptors differ and -1 where they
// agree: dot(train, ~query) = 2 Hamming - 256, exactly (small integers in f32).
// v_mfma_scale_f32_32x32x64_f8f6f4: A = 32 train rows, B = 32 query columns, K = 64 bits per
// instruction (32 per lane half, 4 VGPRs), 4 instructions per 256-bit descriptor.  Both
// operands are built from a descriptor dword by the same rule (expand32_fp4), so whichever K
// position the hardware gives a (lane half, register, nibble), the two sides agree on it.
// A workgroup (4 waves) owns 256 queries of one pair; each wave keeps the expanded bits of its
// 64 queries in registers (B operands of both 32-column groups) and streams 128-train tiles,
// expanded once per workgroup into LDS.  The accumulator puts one query column on each lane
// and 16 train rows in its registers, so the running best/second-best keys are updated
// lane-locally; the two lane halves (different train rows) are merged at the end.
//
// KEYED form (every train index < 2^13): the matrix cores produce the top-2 key itself.  The
// E8M0 block scales are 2^6 and 2^7, so a bit position weighs +-2^13 and the product sum is
// 2^14 Hamming - 2^21; the accumulator starts at float(2^21 + 2^13 + the row's place in its
// 32-train sub-tile), a loop constant, so the result is float(2^14 Hamming + 2^13 + place).
// The running keys are kept relative to the sub-tile at hand: after each sub-tile they drop by
// 32.0f (4 subtractions instead of 16 accumulator set-ups), so an earlier row's place is
// negative and 2^13 + place stays in [0, 2^14) for every train index < 2^13: the keys order as
// (Hamming, train index).  Every partial sum is an integer below 2^23, exact in f32, and
// non-negative floats order like their bit patterns: min / med3 run on the raw bits, rows past
// nt get kMfNone (a float so large that - 32.0f leaves it unchanged, sorting last), and only
// the two winners become integers again.
// Unkeyed form (nt > 8192): unit scales, C = 0, the key (dist << 16 | train) formed per distance.
// ---------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// 32 bits -> 32 FP4 elements (4 dwords): nibble n of dword r <-> bit 4 n + r
__device__ __forceinline__ v4i expand32_fp4(uint32_t bits) {
  v4i r;
  r.x = (int)(((bits << 3) & 0x88888888u) | 0x22222222u);
  r.y = (int)(((bits << 2) & 0x88888888u) | 0x22222222u);
  r.z = (int)(((bits << 1) & 0x88888888u) | 0x22222222u);
  r.w = (int)((bits & 0x88888888u) | 0x22222222u);
  return r;
}
constexpr int kKeyBits = 14;                 // keyed form: key = dist << 14 | (2^13 + relative train index)
constexpr uint32_t kMfNone = 0x7F000000u;    // keyed form: no train (2^127 as a float)
constexpr int kMfKeyedMax = 1 << 13;         // keyed form: at most this many trains

constexpr int kMfTileT = 128;                 // trains per LDS tile
constexpr int kMfSub = kMfTileT / 32;         // 32-train sub-tiles of a tile
constexpr int kMfFetch = kMfTileT * 8 / 256;  // dwords of a tile per thread
constexpr int kMfPitch = 128 + 16;            // expanded train row (bytes), padded against bank conflicts

// float(bits) - 32.0f on the raw bits, as one plain v_add_f32 (the compiler otherwise pairs two
// into v_pk_add_f32, which costs more than two adds beside MFMAs)
__device__ __forceinline__ uint32_t sub32f(uint32_t k) {
  uint32_t r;
  asm("v_add_f32_e32 %0, 0xc2000000, %1" : "=v"(r) : "v"(k));
  return r;
}

// one K = 64 step; the E8M0 scales (every byte of a scale dword the same) are 2^6 and 2^7 in
// the keyed form, 2^0 otherwise
template <bool KEYED>
__device__ __forceinline__ v16f mfma_fp4(v4i a, v4i b, v16f c) {
  constexpr int kScaleA = KEYED ? (int)0x85858585u : 0x7F7F7F7F;
  constexpr int kScaleB = KEYED ? (int)0x86868686u : 0x7F7F7F7F;
  const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0}, b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, kScaleA, 0, kScaleB);
}

#ifndef MCS_TOP2_MINB
#define MCS_TOP2_MINB 4   // 128 VGPRs, accumulators in VGPRs (no AGPR reads)
#endif
template <bool KEYED>
__global__ __launch_bounds__(256, MCS_TOP2_MINB) void k_top2_mfma32(
    const uint8_t* __restrict__ qbase, const uint8_t* __restrict__ tbase,
    const int32_t* __restrict__ counts, const int32_t* __restrict__ pairs, int64_t set_stride,
    int nq_fixed, int nt_fixed, int cap_out, int32_t* __restrict__ best_idx,
    int32_t* __restrict__ best_dist, int32_t* __restrict__ second_idx,
    int32_t* __restrict__ second_dist) {
  __shared__ __attribute__((aligned(16))) uint8_t s_t[kMfTileT * kMfPitch];
  const int p = blockIdx.y;
  const uint8_t* Q;
  const uint8_t* T;
  int nq, nt;
  if (pairs) {
    const int qs = pairs[2 * p], ts = pairs[2 * p + 1];
    Q = qbase + (int64_t)qs * set_stride;
    T = tbase + (int64_t)ts * set_stride;
    nq = counts[qs];
    nt = counts[ts];
  } else {
    Q = qbase; T = tbase; nq = nq_fixed; nt = nt_fixed;
  }
  const int q_blk = blockIdx.x * 256;
  if (q_blk >= nq) return;   // uniform per block
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int h = lane >> 5, col = lane & 31;
  // ---- B operands: this wave's 64 queries (2 column groups x 4 k-steps), complemented; lane
  // half h holds dword 2 s + h of k-step s
  v4i bq[2][4];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int qi = q_blk + wv * 64 + c * 32 + col;
    const uint32_t* qd = reinterpret_cast<const uint32_t*>(Q + (int64_t)min(qi, max(nq - 1, 0)) * 32);
    uint32_t w[4];
#pragma unroll
    for (int s = 0; s < 4; s++) w[s] = qd[2 * s + h];
#pragma unroll
    for (int s = 0; s < 4; s++) bq[c][s] = expand32_fp4(~w[s]);
  }
  constexpr uint32_t kNone = KEYED ? kMfNone : 0xFFFFFFFFu;
  uint32_t k1[2] = {kNone, kNone}, k2[2] = {kNone, kNone};
  // KEYED: what accumulator register r starts from, 2^21 + 2^13 + its row's place in a sub-tile
  v16f cinit = {0};
  if (KEYED) {
#pragma unroll
    for (int r = 0; r < 16; r++) cinit[r] = (float)((1 << 21) + (1 << 13) + 4 * h + (r & 3) + 8 * (r >> 2));
  }
  // train tile bits, one tile ahead: the next tile's loads are in flight while this one is
  // expanded and multiplied (each thread kMfFetch dwords of 128 trains x 8 dwords)
  uint32_t nb[kMfFetch];
  auto fetch = [&](int t0n) {
#pragma unroll
    for (int r = 0; r < kMfFetch; r++) {
      const int e = tid + 256 * r;
      const int tr = e >> 3, dw = e & 7;
      nb[r] = t0n + tr < nt ? reinterpret_cast<const uint32_t*>(T + (int64_t)(t0n + tr) * 32)[dw] : 0u;
    }
  };
  fetch(0);
  for (int t0 = 0; t0 < nt; t0 += kMfTileT) {
    const int ntile = min(kMfTileT, nt - t0);
    uint32_t cb[kMfFetch];
#pragma unroll
    for (int r = 0; r < kMfFetch; r++) cb[r] = nb[r];
    if (t0 + kMfTileT < nt) fetch(t0 + kMfTileT);
    __syncthreads();
    // ---- expand the tile: each dword -> 16 bytes at [train][dword]
#pragma unroll
    for (int r = 0; r < kMfFetch; r++) {
      const int e = tid + 256 * r;
      const int tr = e >> 3, dw = e & 7;
      *reinterpret_cast<v4i*>(s_t + tr * kMfPitch + dw * 16) = expand32_fp4(cb[r]);
    }
    __syncthreads();
    // ---- the tile's 32-train sub-tiles
#pragma unroll
    for (int st = 0; st < kMfSub; st++) {
      if (st * 32 >= ntile) break;
      const int tb = t0 + st * 32 + 4 * h;
      // KEYED: both accumulators start from the rows' key offsets, so the MFMA result is the key
      v16f acc0 = cinit, acc1 = cinit;
      const uint8_t* arow = s_t + (st * 32 + col) * kMfPitch + 16 * h;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * s);
        acc0 = mfma_fp4<KEYED>(a, bq[0][s], acc0);
        acc1 = mfma_fp4<KEYED>(a, bq[1][s], acc1);
      }
      uint32_t key0[16], key1[16];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        if (KEYED) {
          key0[r] = __float_as_uint(acc0[r]);
          key1[r] = __float_as_uint(acc1[r]);
        } else {   // acc = 2 Hamming - 256
          const uint32_t trow = (uint32_t)(tb + (r & 3) + 8 * (r >> 2));
          key0[r] = ((uint32_t)((int)acc0[r] + 256) >> 1 << 16) | trow;
          key1[r] = ((uint32_t)((int)acc1[r] + 256) >> 1 << 16) | trow;
        }
      }
      if (st * 32 + 32 > ntile) {   // the last, partial tile (a scalar branch: no selects in full tiles)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (tb + (r & 3) + 8 * (r >> 2) >= nt) { key0[r] = kNone; key1[r] = kNone; }
      }
      // The compiler pads the wait states between an MFMA and a VALU read of its result only
      // for instructions it knows, not for the operands of an asm statement (min3_u32).  So the
      // first reads of both accumulators are plain medians, which the compiler pads, and
      // nothing is scheduled across the barrier behind them; the first updates below reuse
      // the two values.
      const uint32_t lead0 = med3_u32(key0[0], key0[1], key0[2]);
      const uint32_t lead1 = med3_u32(key1[0], key1[1], key1[2]);
      asm volatile("" :: "v"(lead0), "v"(lead1));
      __builtin_amdgcn_sched_barrier(0);
      // four keys per update: registers 4 g .. 4 g + 2 are the triple, 4 g + 3 the single
#pragma unroll
      for (int g = 0; g < 4; g++) {
        top2_update4(k1[0], k2[0], key0[4 * g], key0[4 * g + 1], key0[4 * g + 2], key0[4 * g + 3]);
        top2_update4(k1[1], k2[1], key1[4 * g], key1[4 * g + 1], key1[4 * g + 2], key1[4 * g + 3]);
      }
      if (KEYED) {   // re-base the running keys to the next sub-tile
#pragma unroll
        for (int c = 0; c < 2; c++) {
          k1[c] = sub32f(k1[c]);
          k2[c] = sub32f(k2[c]);
        }
      }
    }
  }
  // ---- merge the two lane halves (same query, disjoint train rows) and write
  const int none = 8 * 32 + 1;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t o1 = __shfl_xor(k1[c], 32), o2 = __shfl_xor(k2[c], 32);
    const uint32_t b1 = min(k1[c], o1), b2 = min(max(k1[c], o1), min(k2[c], o2));
    const int qi = q_blk + wv * 64 + c * 32 + col;
    if (h == 0 && qi < nq) {
      const int64_t o = (int64_t)p * cap_out + qi;
      const bool h1 = b1 != kNone, h2 = b2 != kNone;
      // KEYED: the winners are floats holding the integer key, its index field 2^13 + the train
      // index relative to the end of the last sub-tile
      const uint32_t v1 = KEYED && h1 ? (uint32_t)__uint_as_float(b1) : b1;
      const uint32_t v2 = KEYED && h2 ? (uint32_t)__uint_as_float(b2) : b2;
      constexpr int kIb = KEYED ? kKeyBits : 16;
      constexpr uint32_t kIm = (1u << kIb) - 1u;
      const int ibase = KEYED ? ((nt + 31) & ~31) - (1 << 13) : 0;
      best_idx[o] = h1 ? (int)(v1 & kIm) + ibase : -1;
      best_dist[o] = h1 ? (int)(v1 >> kIb) : none;
      second_idx[o] = h2 ? (int)(v2 & kIm) + ibase : -1;
      second_dist[o] = h2 ? (int)(v2 >> kIb) : none;
    }
  }
}

template <int W>
__global__ __launch_bounds__(kHamThreads) void k_dense(const uint8_t* __restrict__ A, int na,
                                                       const uint8_t* __restrict__ B, int nb,
                                                       uint16_t* __restrict__ D) {
  __shared__ uint4 tile[kHamTile * (W / 4)];
  const int qi = blockIdx.x * kHamThreads + threadIdx.x;
  const int t0 = blockIdx.y * kHamTile;
  const int nt_tile = min(kHamTile, nb - t0);
  const uint4* src = reinterpret_cast<const uint4*>(B + (int64_t)t0 * W * 4);
  for (int i = threadIdx.x; i < nt_tile * (W / 4); i += kHamThreads) tile[i] = src[i];
  __syncthreads();
  if (qi >= na) return;
  uint32_t q[W];
  const uint4* qp = reinterpret_cast<const uint4*>(A + (int64_t)qi * W * 4);
#pragma unroll
  for (int w4 = 0; w4 < W / 4; w4++) {
    const uint4 v = qp[w4];
    q[4 * w4] = v.x; q[4 * w4 + 1] = v.y; q[4 * w4 + 2] = v.z; q[4 * w4 + 3] = v.w;
  }
  for (int j = 0; j < nt_tile; j++) D[(int64_t)qi * nb + t0 + j] = (uint16_t)ham_dist_v<W>(q, &tile[j * (W / 4)]);
}

#define MCS_DISPATCH_W(bytes, KERNEL, ...)                                                  \
  do {                                                                                     \
    if ((bytes) == 16) hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);                         \
    else if ((bytes) == 32) hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);                    \
    else hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__);                                      \
  } while (0)

}  // namespace mcs

using namespace mcs;

extern "C" {

int mcs_descriptor_distance64(const uint64_t* d1, const uint64_t* d2, int32_t dim) {
  uint64_t dist = 0;
  for (int d = 0; d < dim / 8; ++d) dist += (uint64_t)__builtin_popcountll(d1[d] ^ d2[d]);
  return (int)dist;
}

int mcs_descriptor_distance64_masked(const uint64_t* d1, const uint64_t* d2, const uint64_t* m1,
                                     const uint64_t* m2, int32_t dim) {
  uint64_t dist = 0;
  for (int i = 0; i < dim / 8; ++i) {
    const uint64_t x = d1[i] ^ d2[i];
    dist += (uint64_t)__builtin_popcountll(x & m1[i]) + (uint64_t)__builtin_popcountll(x & m2[i]);
  }
  return (int)(dist / 2);
}

int mcs_hamming_dense_device(const uint8_t* d_a, int32_t na, const uint8_t* d_b, int32_t nb,
                             int32_t bytes, uint16_t* d_dist, void* stream) {
  int rc = host::check_desc_bytes(bytes, "matcher");
  if (rc) return rc;
  if (na <= 0 || nb <= 0) return MCS_OK;
  dim3 g((na + kHamThreads - 1) / kHamThreads, (nb + kHamTile - 1) / kHamTile);
  MCS_DISPATCH_W(bytes, k_dense, g, dim3(kHamThreads), 0, (hipStream_t)stream, d_a, na, d_b, nb,
                 d_dist);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_hamming_top2_device(const uint8_t* d_q, int32_t nq, const uint8_t* d_t, int32_t nt,
                            int32_t bytes, int32_t* d_best_idx, int32_t* d_best_dist,
                            int32_t* d_second_idx, int32_t* d_second_dist, void* stream) {
  int rc = host::check_desc_bytes(bytes, "matcher");
  if (rc) return rc;
  if (nq <= 0) return MCS_OK;
  if (nt > 65535) { set_error("top2: at most 65535 train descriptors"); return MCS_ERR_ARG; }
  if (bytes == 32) {
    auto* kfn = nt <= kMfKeyedMax ? k_top2_mfma32<true> : k_top2_mfma32<false>;
    hipLaunchKernelGGL(kfn, dim3((nq + 255) / 256, 1), dim3(256), 0, (hipStream_t)stream,
                       d_q, d_t, (const int32_t*)nullptr, (const int32_t*)nullptr, (int64_t)0, nq,
                       nt, nq, d_best_idx, d_best_dist, d_second_idx, d_second_dist);
    MCS_HIP_CHECK(hipGetLastError());
    return MCS_OK;
  }
  dim3 g((nq + kHamThreads * kQPT - 1) / (kHamThreads * kQPT), 1);
  MCS_DISPATCH_W(bytes, k_top2, g, dim3(kHamThreads), 0, (hipStream_t)stream, d_q, d_t,
                 (const int32_t*)nullptr, (const int32_t*)nullptr, (int64_t)0, nq, nt, nq,
                 d_best_idx, d_best_dist, d_second_idx, d_second_dist);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

int mcs_hamming_top2_batch_device(const uint8_t* d_desc, const int32_t* d_counts,
                                  const int32_t* d_pairs, int32_t n_pairs, int32_t cap,
                                  int32_t bytes, int32_t* d_best_idx, int32_t* d_best_dist,
                                  int32_t* d_second_idx, int32_t* d_second_dist, void* stream) {
  int rc = host::check_desc_bytes(bytes, "matcher");
  if (rc) return rc;
  if (n_pairs <= 0) return MCS_OK;
  if (!d_desc || !d_counts || !d_pairs || cap <= 0) return MCS_ERR_ARG;
  if (cap > 65535) { set_error("top2: capacity above 65535"); return MCS_ERR_ARG; }
  if (bytes == 32) {   // a pair's train count is <= cap
    auto* kfn = cap <= kMfKeyedMax ? k_top2_mfma32<true> : k_top2_mfma32<false>;
    hipLaunchKernelGGL(kfn, dim3((cap + 255) / 256, n_pairs), dim3(256), 0,
                       (hipStream_t)stream, d_desc, d_desc, d_counts, d_pairs,
                       (int64_t)cap * bytes, 0, 0, cap, d_best_idx, d_best_dist, d_second_idx,
                       d_second_dist);
    MCS_HIP_CHECK(hipGetLastError());
    return MCS_OK;
  }
  dim3 g((cap + kHamThreads * kQPT - 1) / (kHamThreads * kQPT), n_pairs);
  MCS_DISPATCH_W(bytes, k_top2, g, dim3(kHamThreads), 0, (hipStream_t)stream, d_desc, d_desc,
                 d_counts, d_pairs, (int64_t)cap * bytes, 0, 0, cap, d_best_idx, d_best_dist,
                 d_second_idx, d_second_dist);
  MCS_HIP_CHECK(hipGetLastError());
  return MCS_OK;
}

}  // extern "C"
