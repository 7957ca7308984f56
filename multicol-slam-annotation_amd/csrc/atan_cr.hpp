// atan rounded to nearest from a double-double evaluation, the same code on the host and on
// the device.  The reference projects through the host libm's atan (WorldToImg,
// cam_model_omni.cpp:147-163), which is good to under one ulp and gives the correctly rounded
// result for all but about 2.5 arguments in ten thousand (tests/cpp/atan_cr_check.cpp); the
// device library's atan misses it for a few in a hundred, which shows in the last place of a
// projected pixel.  A kernel held to the reference's bits calls this: it then equals the libm
// except where the libm itself misrounds, and is never more than one ulp from it.
//
// |x| > 1 goes through pi/2 - atan(1/x); four halvings atan(t) = 2 atan(t / (1 + sqrt(1 + t^2)))
// bring t below 0.05; the Taylor series to t^29 is summed by Horner.  Every step is in
// double-double (error-free sums and products, the product's error from fma), about 2^-100
// relative, so the rounding of hi + lo is the rounding of the exact value unless that lies within
// 2^-45 ulp of a midpoint.  Needs -ffp-contract=off (the error terms must not be contracted).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCS_HD __host__ __device__
#else
#define MCS_HD
#endif

namespace mcs {
namespace ddm {

struct dd { double hi, lo; };

MCS_HD inline dd two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return dd{s, (a - (s - bb)) + (b - bb)};
}
MCS_HD inline dd fast_two_sum(double a, double b) {   // |a| >= |b|
  const double s = a + b;
  return dd{s, b - (s - a)};
}
MCS_HD inline dd two_prod(double a, double b) {
  const double p = a * b;
  return dd{p, fma(a, b, -p)};
}
MCS_HD inline dd add(dd a, dd b) {
  dd s = two_sum(a.hi, b.hi);
  const dd t = two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = fast_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return fast_two_sum(s.hi, s.lo);
}
MCS_HD inline dd neg(dd a) { return dd{-a.hi, -a.lo}; }
MCS_HD inline dd mul(dd a, dd b) {
  dd p = two_prod(a.hi, b.hi);
  p.lo += a.hi * b.lo + a.lo * b.hi;
  return fast_two_sum(p.hi, p.lo);
}
MCS_HD inline dd mul_d(dd a, double b) {
  dd p = two_prod(a.hi, b);
  p.lo += a.lo * b;
  return fast_two_sum(p.hi, p.lo);
}
MCS_HD inline dd div(dd a, dd b) {
  const double q1 = a.hi / b.hi;
  dd r = add(a, neg(mul_d(b, q1)));
  const double q2 = r.hi / b.hi;
  r = add(r, neg(mul_d(b, q2)));
  const double q3 = r.hi / b.hi;
  return add(fast_two_sum(q1, q2), dd{q3, 0.0});
}
MCS_HD inline dd sqrt_dd(dd a) {   // a > 0
  const double s = sqrt(a.hi);
  const dd r = add(a, neg(two_prod(s, s)));
  return fast_two_sum(s, r.hi / (2.0 * s));
}

}  // namespace ddm

MCS_HD inline double atan_cr(double x) {
  using namespace ddm;
  if (x != x || x == 0.0) return x;
  const double ax = fabs(x);
  const dd half_pi{1.5707963267948966, 6.123233995736766e-17};
  double r;
  if (ax > 0x1p60) {
    r = half_pi.hi;
  } else if (ax < 0x1p-28) {
    r = ax;                         // x - x^3 / 3 rounds to x
  } else {
    const bool inv = ax > 1.0;
    dd t = inv ? div(dd{1.0, 0.0}, dd{ax, 0.0}) : dd{ax, 0.0};
    for (int k = 0; k < 4; k++)
      t = div(t, add(dd{1.0, 0.0}, sqrt_dd(add(dd{1.0, 0.0}, mul(t, t)))));
    // 1 / (2 n + 1), n = 0 .. 14, as double-double
    const dd inv_odd[15] = {
        {1.0, 0.0},
        {0.3333333333333333, 1.850371707708594e-17},
        {0.2, -1.1102230246251566e-17},
        {0.14285714285714285, 7.93016446160826e-18},
        {0.1111111111111111, 6.1679056923619804e-18},
        {0.09090909090909091, -2.523234146875356e-18},
        {0.07692307692307693, -4.270088556250602e-18},
        {0.06666666666666667, 9.251858538542971e-19},
        {0.058823529411764705, 8.163404592832033e-19},
        {0.05263157894736842, 2.921639538487254e-18},
        {0.047619047619047616, 2.64338815386942e-18},
        {0.043478260869565216, 1.206764157201257e-18},
        {0.04, -8.326672684688674e-19},
        {0.037037037037037035, 2.05596856412066e-18},
        {0.034482758620689655, 4.785444071660157e-19}};
    const dd t2 = mul(t, t);
    dd s = inv_odd[14];
    for (int n = 13; n >= 0; n--) s = add(inv_odd[n], neg(mul(t2, s)));
    dd a = mul(t, s);
    a.hi *= 16.0;
    a.lo *= 16.0;
    if (inv) a = add(half_pi, neg(a));
    r = a.hi + a.lo;
  }
  return x < 0.0 ? -r : r;
}

}  // namespace mcs
