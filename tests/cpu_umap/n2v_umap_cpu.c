/* The CPU restatement of csrc/n2v_umap.hip and csrc/n2v_powb.h: the same fp32 operations in the same order, one
 * rounding per spelled operation (compiled by tests/cpu_build.py without contraction), one thread, rows ascending,
 * no grouping of rows: the law alone. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float as_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static int32_t as_int(float f) {
  int32_t i;
  memcpy(&i, &f, 4);
  return i;
}

float n2v_umap_cpu_powb1(float x, float b) {
  if (!(x <= 0x1.fffffep+127f)) return x;
  int32_t adj = 0;
  if (x < 0x1.0p-126f) {
    x = x * 0x1.0p+24f;
    adj = -24;
  }
  const int32_t ix = as_int(x);
  const int32_t d = ix - 0x3f3504f3;
  const int32_t k = d >= 0 ? d / 0x00800000 : -((-d + 0x007fffff) / 0x00800000); /* d >> 23, arithmetic */
  const float m = as_float((uint32_t)(ix - k * 0x00800000));
  const float e = (float)(k + adj);
  const float f = m - 1.0f;
  float g = 0x1.84705ap-4f;
  g = fmaf(g, f, -0x1.5766fep-3f);
  g = fmaf(g, f, 0x1.60f96ep-3f);
  g = fmaf(g, f, -0x1.6efbc4p-3f);
  g = fmaf(g, f, 0x1.a3eb38p-3f);
  g = fmaf(g, f, -0x1.ec6fd6p-3f);
  g = fmaf(g, f, 0x1.278062p-2f);
  g = fmaf(g, f, -0x1.7154b2p-2f);
  g = fmaf(g, f, 0x1.ec708p-2f);
  g = fmaf(g, f, -0x1.715476p-1f);
  g = fmaf(g, f, 0x1.715476p+0f);
  const float lg = g * f;
  const float u = b * lg;
  const float y = fmaf(b, e, u);
  if (!(y >= -151.0f)) return 0.0f;
  if (y > 129.0f) return INFINITY;
  const float n = rintf(y);
  float r = fmaf(b, e, -n);
  r = r + u;
  float p = 0x1.00d2c8p-16f;
  p = fmaf(p, r, 0x1.448988p-13f);
  p = fmaf(p, r, 0x1.5d875ep-10f);
  p = fmaf(p, r, 0x1.3b29b2p-7f);
  p = fmaf(p, r, 0x1.c6b08ep-5f);
  p = fmaf(p, r, 0x1.ebfbep-3f);
  p = fmaf(p, r, 0x1.62e43p-1f);
  p = fmaf(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const int32_t n1 = ni / 2, n2 = ni - n1;
  const float s1 = as_float((uint32_t)(n1 + 127) << 23), s2 = as_float((uint32_t)(n2 + 127) << 23);
  const float q = p * s1;
  return q * s2;
}

/* n2v_umap_powb: the epoch's pw over an array */
void n2v_umap_cpu_powb(const float *x, int64_t n, float b, float *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = x[i] > 0.0f ? (b == 1.0f ? x[i] : n2v_umap_cpu_powb1(x[i], b)) : 0.0f;
}

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

typedef struct {
  float a, b, m2ab, g2b, alpha, alpha4;
} scalars_t;

static float clamp4(float v) { return v > 4.0f ? 4.0f : (v < -4.0f ? -4.0f : v); }

static void move(float *y, float c, float dx, float dy, float alpha) {
  const float px = c * dx, py = c * dy;
  const float gx = clamp4(px), gy = clamp4(py);
  const float sx = alpha * gx, sy = alpha * gy;
  y[0] = y[0] + sx;
  y[1] = y[1] + sy;
}

static void attract(float *y, const float *o, const scalars_t *S) {
  const float dx = y[0] - o[0], dy = y[1] - o[1];
  const float sq = dx * dx;
  const float d2 = fmaf(dy, dy, sq);
  float c = 0.0f;
  if (d2 > 0.0f) {
    const float pw = S->b == 1.0f ? d2 : n2v_umap_cpu_powb1(d2, S->b);
    const float t = S->m2ab * pw;
    const float num = t / d2;
    const float den = fmaf(S->a, pw, 1.0f);
    c = num / den;
  }
  move(y, c, dx, dy, S->alpha);
}

static void repel(float *y, const float *o, const scalars_t *S) {
  const float dx = y[0] - o[0], dy = y[1] - o[1];
  const float sq = dx * dx;
  const float d2 = fmaf(dy, dy, sq);
  if (d2 > 0.0f) {
    const float pw = S->b == 1.0f ? d2 : n2v_umap_cpu_powb1(d2, S->b);
    const float d1 = 0.001f + d2;
    const float dd = fmaf(S->a, pw, 1.0f);
    const float den = d1 * dd;
    const float c = S->g2b / den;
    move(y, c, dx, dy, S->alpha);
  } else if (d2 == 0.0f) {
    y[0] = y[0] + S->alpha4;
    y[1] = y[1] + S->alpha4;
  }
}

/* one epoch; self_hits (may be NULL) counts the draws that hit their own row */
void n2v_umap_cpu_epoch(const int64_t *rowptr, const int32_t *col, const float *eps, int64_t nnz, const float *Y,
                        float *Y_next, int64_t n, int32_t epoch, float a, float b, float gamma, float alpha,
                        int32_t negative, uint64_t seed, int64_t *self_hits) {
  scalars_t S;
  S.a = a;
  S.b = b;
  const float ab = a * b, g2 = 2.0f * gamma;
  S.m2ab = -2.0f * ab;
  S.g2b = g2 * b;
  S.alpha = alpha;
  S.alpha4 = alpha * 4.0f;
  const float ep0 = (float)epoch, ep1 = (float)(epoch + 1);
  const uint64_t he = mix64(seed ^ mix64((uint64_t)epoch + 0x9E3779B97F4A7C15ULL));
  int64_t hits = 0;
  for (int64_t i = 0; i < n; ++i) {
    float y[2] = {Y[2 * i], Y[2 * i + 1]};
    int64_t lo = rowptr[i], hi = rowptr[i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > nnz ? nnz : hi;
    for (int64_t t = lo; t < hi; ++t) {
      const float e = eps[t];
      if (!(e >= 1.0f && e <= 0x1.fffffep+127f)) continue;
      const float q1 = ep1 / e, q0 = ep0 / e;
      if (!(floorf(q1) > floorf(q0))) continue;
      const int32_t j = col[t];
      if (j < 0 || (int64_t)j >= n) continue;
      attract(y, Y + 2 * (int64_t)j, &S);
      attract(y, Y + 2 * (int64_t)j, &S);
      const uint64_t ht = mix64(he + ((uint64_t)t + 1ULL) * 0xD1B54A32D192ED03ULL);
      for (int32_t s = 0; s < negative; ++s) {
        const uint64_t r = mix64(ht ^ (((uint64_t)s + 1ULL) * 0x8CB92BA72F3D8DD7ULL));
        const int64_t k = (int64_t)(((r >> 32) * (uint64_t)n) >> 32);
        if (k == i) {
          ++hits;
          continue;
        }
        repel(y, Y + 2 * k, &S);
      }
    }
    Y_next[2 * i] = y[0];
    Y_next[2 * i + 1] = y[1];
  }
  if (self_hits) *self_hits = hits;
}
