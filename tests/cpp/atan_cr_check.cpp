// csrc/atan_cr.hpp on the host against the libm: how many of n arguments round differently and
// by how many units in the last place at the most.  Arguments: tan of uniform angles (what
// WorldToImg sees) and powers of two times [0.55, 1.45] over 2^-30 .. 2^40, both signs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../multicol-slam-annotation_amd/csrc/atan_cr.hpp"

static int64_t bits(double v) {
  int64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

int main() {
  std::mt19937_64 g(7);
  std::uniform_real_distribution<double> ang(-1.55, 1.55), ex(-30, 40);
  const long n = 1000000;
  long differ = 0, max_ulp = 0;
  for (long i = 0; i < n; i++) {
    const double x = (i & 1) ? std::tan(ang(g)) : std::ldexp(1.0 + ang(g) * 0.29, (int)ex(g)) * ((i & 2) ? 1 : -1);
    const int64_t d = bits(std::atan(x)) - bits(mcs::atan_cr(x));
    if (d) differ++;
    if (d > max_ulp) max_ulp = d;
    if (-d > max_ulp) max_ulp = -d;
  }
  const double sp[] = {0.0, -0.0, 1.0, -1.0, 1e300, -1e300, 1e-300, 0x1p-28, 0x1p60};
  long special = 0;
  for (double x : sp) special += bits(std::atan(x)) != bits(mcs::atan_cr(x));
  std::printf("n %ld differ %ld max_ulp %ld special %ld\n", n, differ, max_ulp, special);
  return 0;
}
