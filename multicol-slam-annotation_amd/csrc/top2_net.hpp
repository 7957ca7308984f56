// Running best / second-best over packed keys (smaller key = better match), shared by the
// top-2 matcher kernels of hamming.hip.  The invariant is k1 <= k2; "none" is any key that
// sorts last.  The host side is plain comparisons and needs no HIP header, so a CPU program can
// check the device formulas (tests/cpp/top2_net_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MCS_TOP2_FN __host__ __device__ __forceinline__
#else
#define MCS_TOP2_FN inline
#endif

namespace mcs {

MCS_TOP2_FN uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
MCS_TOP2_FN uint32_t max_u32(uint32_t a, uint32_t b) { return a < b ? b : a; }

// v_min3_u32.  Written as min(min(a, b), c) it would share min(a, b) with the median of the
// same three values, and the compiler then keeps the shared v_min_u32 and issues three
// instructions for the pair where two do; the asm keeps them apart.
MCS_TOP2_FN uint32_t min3_u32(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return min_u32(min_u32(a, b), c);
#endif
}

// v_med3_u32: the compiler matches this form (each inner min / max used once)
MCS_TOP2_FN uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
  return max_u32(min_u32(a, b), min_u32(max_u32(a, b), c));
}

// one key: 2 ops
MCS_TOP2_FN void top2_update1(uint32_t& k1, uint32_t& k2, uint32_t key) {
  k2 = med3_u32(k1, key, k2);
  k1 = min_u32(k1, key);
}

// four keys in 5 ops (1.25 per key), equal to four top2_update1 steps for every input: the
// two smallest of {k1, k2, a, b, c, d} lie among k1, k2, d and the two smallest (m <= t) of the
// triple.  The smallest is min3(k1, m, d).  The second smallest of {k1, m, d} is their median
// u, and adding an x that is >= some element already present turns the second smallest s into
// min(s, x): that holds for k2 (>= k1) and for t (>= m), so the second is min3(k2, t, u).
MCS_TOP2_FN void top2_update4(uint32_t& k1, uint32_t& k2, uint32_t a, uint32_t b, uint32_t c,
                              uint32_t d) {
  const uint32_t m = min3_u32(a, b, c), t = med3_u32(a, b, c);
  const uint32_t u = med3_u32(k1, m, d);
  k1 = min3_u32(k1, m, d);
  k2 = min3_u32(k2, t, u);
}

}  // namespace mcs
