// Exhaustive CPU check of the matcher's running best / second-best update (csrc/top2_net.hpp).
// Plain C++: builds with g++ alone, with or without sanitizers.  Prints one "ok ..." line and
// returns 0, or prints the first mismatch and returns 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../multicol-slam-annotation_amd/csrc/top2_net.hpp"

using mcs::top2_update1;
using mcs::top2_update4;

int main() {
  constexpr uint32_t V = 6;   // values 0..5: six operands, so every order and every tie pattern
  long n_single = 0, n_chain = 0;
  // (1) one update against sorting, and against four sequential steps
  for (uint32_t k1 = 0; k1 < V; k1++)
    for (uint32_t k2 = k1; k2 < V; k2++)
      for (uint32_t a = 0; a < V; a++)
        for (uint32_t b = 0; b < V; b++)
          for (uint32_t c = 0; c < V; c++)
            for (uint32_t d = 0; d < V; d++) {
              uint32_t s[6] = {k1, k2, a, b, c, d};
              std::sort(s, s + 6);
              uint32_t n1 = k1, n2 = k2;
              top2_update4(n1, n2, a, b, c, d);
              uint32_t q1 = k1, q2 = k2;
              top2_update1(q1, q2, a);
              top2_update1(q1, q2, b);
              top2_update1(q1, q2, c);
              top2_update1(q1, q2, d);
              if (n1 != s[0] || n2 != s[1] || q1 != s[0] || q2 != s[1]) {
                std::printf("mismatch k=(%u,%u) keys=(%u,%u,%u,%u): net (%u,%u) seq (%u,%u) sorted (%u,%u)\n",
                            k1, k2, a, b, c, d, n1, n2, q1, q2, s[0], s[1]);
                return 1;
              }
              n_single++;
            }
  // (2) the same with "none" keys as the kernels use them (all ones; the keyed form's 0x7F000000)
  // on every subset of the six operands, the others distinct small keys
  const uint32_t nones[2] = {0xFFFFFFFFu, 0x7F000000u};
  for (uint32_t none : nones)
    for (uint32_t mask = 0; mask < 64; mask++)
      for (uint32_t rot = 0; rot < 6; rot++) {
        uint32_t v[6];
        for (uint32_t i = 0; i < 6; i++) v[i] = (mask >> i & 1) ? none : ((i + rot) % 6) * 0x4000u + 7;
        if (v[0] > v[1]) std::swap(v[0], v[1]);
        uint32_t s[6];
        std::copy(v, v + 6, s);
        std::sort(s, s + 6);
        uint32_t n1 = v[0], n2 = v[1];
        top2_update4(n1, n2, v[2], v[3], v[4], v[5]);
        if (n1 != s[0] || n2 != s[1]) {
          std::printf("mismatch with none %08x mask %u rot %u: (%08x,%08x) sorted (%08x,%08x)\n", none,
                      mask, rot, n1, n2, s[0], s[1]);
          return 1;
        }
        n_single++;
      }
  // (3) chained over 16 keys (one accumulator of k_top2_mfma32: four groups of four) against
  // the sequential scan: keys from a small LCG over 0..5 so ties are frequent, from every
  // ordered start (k1 <= k2), plus the sorted and the reversed runs
  uint32_t lcg = 12345u;
  for (int it = 0; it < 200000; it++) {
    uint32_t key[16];
    for (int r = 0; r < 16; r++) {
      lcg = lcg * 1664525u + 1013904223u;
      key[r] = (lcg >> 24) % V;
    }
    if (it % 3 == 1) std::sort(key, key + 16);
    if (it % 3 == 2) std::sort(key, key + 16, [](uint32_t x, uint32_t y) { return x > y; });
    for (uint32_t k1 = 0; k1 < V; k1++)
      for (uint32_t k2 = k1; k2 < V; k2++) {
        uint32_t n1 = k1, n2 = k2, q1 = k1, q2 = k2;
        for (int g = 0; g < 4; g++)
          top2_update4(n1, n2, key[4 * g], key[4 * g + 1], key[4 * g + 2], key[4 * g + 3]);
        for (int r = 0; r < 16; r++) top2_update1(q1, q2, key[r]);
        if (n1 != q1 || n2 != q2) {
          std::printf("chain mismatch at it %d start (%u,%u): net (%u,%u) seq (%u,%u)\n", it, k1, k2, n1,
                      n2, q1, q2);
          return 1;
        }
        n_chain++;
      }
  }
  std::printf("ok single %ld chain %ld\n", n_single, n_chain);
  return 0;
}
