// n2v_logistic.h -- the spelled logistic functions n2v_logreg.hip and n2v_edge_logreg.hip share: every caller gets
// the same bits from the same fmaf sequences (DESIGN.md "Node classification"; tests/cpu_logreg/n2v_logreg_cpu.c
// restates them).
//
// Per point, y the label bit:  e = exp(-|z|);  p = (z >= 0 ? 1 : e) / (1 + e);  res = p - y;
//   l = (m > 0 ? m : 0) + log1p(e) with m = y ? -z : z.  exp and log1p are the fmaf sequences spelled below.
#pragma once

#include "n2v_common.h"

namespace {

// exp(t) for t <= 0 (NaN: NaN; t < -104: 0).  n = rintf(t log2 e); r = t - n ln 2 in two fmaf (n times the high
// part is exact); a degree-6 Horner chain; 2^n as two powers of two: exact while the result is normal
__device__ inline float exp_neg(float t) {
  if (!(t >= -104.0f)) return t != t ? t : 0.0f;
  const float n = rintf(t * 0x1.715476p+0f);
  float r = __fmaf_rn(n, -0x1.62e4p-1f, t);
  r = __fmaf_rn(n, -0x1.7f7d1cp-20f, r);
  float p = 0x1.6d7544p-10f;
  p = __fmaf_rn(p, r, 0x1.126fb8p-7f);
  p = __fmaf_rn(p, r, 0x1.5554acp-5f);
  p = __fmaf_rn(p, r, 0x1.555404p-3f);
  p = __fmaf_rn(p, r, 0x1.0p-1f);
  p = __fmaf_rn(p, r, 1.0f);
  p = __fmaf_rn(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const int32_t n1 = ni / 2, n2 = ni - n1;
  const float s1 = __uint_as_float((uint32_t)(n1 + 127) << 23), s2 = __uint_as_float((uint32_t)(n2 + 127) << 23);
  return (p * s1) * s2;
}

// log1p(e) for e in [0, 1] (NaN: NaN): e + e^2 g(e), g a degree-13 Horner chain
__device__ inline float log1p01(float e) {
  float g = 0x1.e52a08p-12f;
  g = __fmaf_rn(g, e, -0x1.eb08aap-9f);
  g = __fmaf_rn(g, e, 0x1.d275c6p-7f);
  g = __fmaf_rn(g, e, -0x1.18da6ep-5f);
  g = __fmaf_rn(g, e, 0x1.ed6386p-5f);
  g = __fmaf_rn(g, e, -0x1.5d27a2p-4f);
  g = __fmaf_rn(g, e, 0x1.b16db6p-4f);
  g = __fmaf_rn(g, e, -0x1.fa5fep-4f);
  g = __fmaf_rn(g, e, 0x1.241036p-3f);
  g = __fmaf_rn(g, e, -0x1.5545d4p-3f);
  g = __fmaf_rn(g, e, 0x1.99987ap-3f);
  g = __fmaf_rn(g, e, -0x1.fffff6p-3f);
  g = __fmaf_rn(g, e, 0x1.555556p-2f);
  g = __fmaf_rn(g, e, -0x1.0p-1f);
  const float u = e * g;
  return __fmaf_rn(e, u, e);
}

// one point: the residual res = p - y and the loss l of the score z under the label bit y
__device__ __forceinline__ void logistic_point(float z, uint32_t y, float &res, float &l) {
  const float e = exp_neg(-fabsf(z));
  const float num = z >= 0.0f ? 1.0f : e;
  const float den = 1.0f + e;
  const float p = num / den;
  const float m = y ? -z : z;
  res = p - (y ? 1.0f : 0.0f);
  l = (m > 0.0f ? m : 0.0f) + log1p01(e);
}

}  // namespace
