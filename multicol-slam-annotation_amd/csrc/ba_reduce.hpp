// The deterministic reductions of the BA kernels: every sum runs in a fixed order (no float
// atomics), so results are bitwise reproducible run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "ba_dev.hpp"

namespace mcs::ba {
// deterministic sum over a 256-thread workgroup: xor butterfly per wave, then the 4 wave sums
// in wave order (every thread calls; the result is valid in every thread)
__device__ __forceinline__ double block_sum256(double v) {
  __shared__ double sm[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();   // sm may still be read by a previous call
  if (lane == 0) sm[w] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// sum over a quad of lanes in a fixed order ((l0 + l1) + (l2 + l3))
__device__ __forceinline__ double quad_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// deterministic sum / max|.| of n doubles -> out[0], two stages with fixed orders:
// k_reduce_part: workgroup g owns the contiguous chunk [g*chunk, (g+1)*chunk), each thread
// 8 strided accumulators (loads in flight, short add chains), a fixed tree over the block;
// k_reduce: one workgroup over the partials.  Small inputs skip the first stage.
constexpr int kRedPartMax = 256;
template <bool MAX>
__global__ __launch_bounds__(256) void k_reduce_part(const double* __restrict__ v, int n, int chunk,
                                                     double* __restrict__ part) {
  __shared__ double s[256];
  const int g = blockIdx.x, t = threadIdx.x;
  const int b0 = g * chunk, b1 = min(n, b0 + chunk);
  double acc[8];
#pragma unroll
  for (int u = 0; u < 8; u++) acc[u] = 0.0;
  for (int i = b0 + t; i < b1; i += 8 * 256) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int q = i + u * 256;
      if (q < b1) acc[u] = MAX ? fmax(acc[u], fabs(v[q])) : acc[u] + v[q];
    }
  }
  double a = acc[0];
#pragma unroll
  for (int u = 1; u < 8; u++) a = MAX ? fmax(a, acc[u]) : a + acc[u];
  s[t] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) s[t] = MAX ? fmax(s[t], s[t + o]) : s[t] + s[t + o];
    __syncthreads();
  }
  if (t == 0) part[g] = s[0];
}

template <bool MAX>
__global__ __launch_bounds__(1024) void k_reduce(const double* __restrict__ v, int n, double* out) {
  __shared__ double s[1024];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc = MAX ? fmax(acc, fabs(v[i])) : acc + v[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o) s[threadIdx.x] = MAX ? fmax(s[threadIdx.x], s[threadIdx.x + o]) : s[threadIdx.x] + s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s[0];
}

// The closing sums of an LM trial (robust chi2, point and pose step norms), one workgroup
// each, in exactly k_reduce<false>'s order (1024-strided partials, then the LDS tree); every
// sum goes straight to host-coherent memory with its own released sequence number (the solve
// flag with the first), so the host sees the trial's outcome without a readback copy or a
// stream synchronisation.
__global__ __launch_bounds__(1024) void k_reduce3(Sum3 q, const int* flag, TrialSig* sig, uint64_t seq) {
  __shared__ double s[1024];
  const int t = threadIdx.x, b = blockIdx.x;
  const double* v = q.v[b];
  const int n = q.n[b];
  double acc = 0.0;
  for (int i = t; i < n; i += 1024) acc = acc + v[i];
  s[t] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) s[t] = s[t] + s[t + o];
    __syncthreads();
  }
  if (t == 0) {
    sig->v[b] = s[0];
    if (b == 0) sig->flag = *flag;
    __hip_atomic_store(&sig->seq[b], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// launch helper: part = kRedPartMax doubles of scratch (stream-ordered reuse is safe)
template <bool MAX>
void reduce_dev(const double* v, int n, double* out, double* part, hipStream_t st) {
  if (n <= 32768) {
    hipLaunchKernelGGL(k_reduce<MAX>, dim3(1), dim3(1024), 0, st, v, n, out);
    return;
  }
  const int chunk = std::max(8 * 256, (n + kRedPartMax - 1) / kRedPartMax);
  const int g = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(k_reduce_part<MAX>, dim3(g), dim3(256), 0, st, v, n, chunk, part);
  hipLaunchKernelGGL(k_reduce<MAX>, dim3(1), dim3(1024), 0, st, (const double*)part, g, out);
}

}  // namespace mcs::ba
