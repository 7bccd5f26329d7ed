// n2v_powb.h -- x^b for x > 0 and a finite b > 0 as ONE spelled fp32 sequence, so that n2v_umap.hip and its CPU
// restatement (tests/cpu_umap/n2v_umap_cpu.c, C fmaf) give the same bits (DESIGN.md "UMAP").
//
//   x = +inf or NaN: x itself.  x below 2^-126 is scaled by 2^24 first (exact) and 24 is taken off the exponent.
//   x = 2^k m with m in [sqrt(1/2), sqrt(2)): k = (bits(x) - bits(sqrt(1/2))) >> 23, m = bits(x) - (k << 23).
//   f = m - 1 (exact);  lg = f * g(f), g a degree-10 Horner chain for log2(1 + f) / f;  e = (float)k
//   u = b * lg;  y = fmaf(b, e, u);  y < -151 (or NaN): +0;  y > 129: +inf
//   n = rintf(y);  r = fmaf(b, e, -n) + u  (b e - n is exact up to one rounding of a number of size 1)
//   p = a degree-7 Horner chain for 2^r on [-0.52, 0.52];  2^n as two powers of two, as n2v_logistic.h's exp_neg:
//   (p * 2^(n / 2)) * 2^(n - n / 2), exact while the result is normal, one rounding below that.
#pragma once

#include "n2v_common.h"

namespace {

__device__ inline float powb(float x, float b) {
  if (!(x <= 0x1.fffffep+127f)) return x;
  int32_t adj = 0;
  if (x < 0x1.0p-126f) {
    x = x * 0x1.0p+24f;
    adj = -24;
  }
  const int32_t ix = __float_as_int(x);
  const int32_t k = (ix - 0x3f3504f3) >> 23;
  const float m = __int_as_float(ix - k * 0x00800000);
  const float e = (float)(k + adj);
  const float f = m - 1.0f;
  float g = 0x1.84705ap-4f;
  g = __fmaf_rn(g, f, -0x1.5766fep-3f);
  g = __fmaf_rn(g, f, 0x1.60f96ep-3f);
  g = __fmaf_rn(g, f, -0x1.6efbc4p-3f);
  g = __fmaf_rn(g, f, 0x1.a3eb38p-3f);
  g = __fmaf_rn(g, f, -0x1.ec6fd6p-3f);
  g = __fmaf_rn(g, f, 0x1.278062p-2f);
  g = __fmaf_rn(g, f, -0x1.7154b2p-2f);
  g = __fmaf_rn(g, f, 0x1.ec708p-2f);
  g = __fmaf_rn(g, f, -0x1.715476p-1f);
  g = __fmaf_rn(g, f, 0x1.715476p+0f);
  const float lg = g * f;
  const float u = b * lg;
  const float y = __fmaf_rn(b, e, u);
  if (!(y >= -151.0f)) return 0.0f;
  if (y > 129.0f) return __int_as_float(0x7f800000);
  const float n = rintf(y);
  float r = __fmaf_rn(b, e, -n);
  r = r + u;
  float p = 0x1.00d2c8p-16f;
  p = __fmaf_rn(p, r, 0x1.448988p-13f);
  p = __fmaf_rn(p, r, 0x1.5d875ep-10f);
  p = __fmaf_rn(p, r, 0x1.3b29b2p-7f);
  p = __fmaf_rn(p, r, 0x1.c6b08ep-5f);
  p = __fmaf_rn(p, r, 0x1.ebfbep-3f);
  p = __fmaf_rn(p, r, 0x1.62e43p-1f);
  p = __fmaf_rn(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const int32_t n1 = ni / 2, n2 = ni - n1;
  const float s1 = __uint_as_float((uint32_t)(n1 + 127) << 23), s2 = __uint_as_float((uint32_t)(n2 + 127) << 23);
  return (p * s1) * s2;
}

}  // namespace
