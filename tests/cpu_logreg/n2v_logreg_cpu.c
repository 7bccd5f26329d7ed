/* CPU restatement of node2vec_amd/csrc/n2v_logreg.hip: the scores, the spelled exp / log1p, the slab chains of the
 * fused loss-and-gradient pass and the fp64 fold.  Built with the flags of tests/cpu_build.py (no contraction), so
 * every line below is the fp32 or fp64 operation it spells.  This text is the contract; the kernels are held to its bits.
 *
 * dot(w, x):  acc = +0; for d0 = 0, 16, .. < round_up(dim, 16), j = 0..3, k = 0..3, d = d0 + 4 k + j:
 *             acc = fmaf(x[d], w[d], acc), both read as 0 at d >= dim (n2v_score_tile.h's chain).
 * z = dot(W_k, x_r) + b[k].
 * slabs:      S = min(2048, 512 MiB / (4 c (dim + 3))); slab_rows = round_up(max(1, ceil(n / S)), 64).
 * GW[s][k][d]: acc = +0; for every row r of the slab, ascending: acc = fmaf(res[r][k], x_r[d], acc); then for
 *             every padding row up to the next multiple of 64 rows (counted from the slab's first row):
 *             acc = fmaf(+0, +0, acc) -- a +0 product added to a -0 accumulator gives +0, so a chain that has
 *             underflowed to -0 leaves a padded slab as +0.  Only the last slab has padding rows.
 * Gb[s][k]:   acc = +0; acc = acc + res[r][k] over the slab's rows ascending (no padding rows; never -0).
 * L[s][k]:    acc = 0.0; acc = acc + (double)l[r][k] over the slab's rows ascending.
 * fold:       gW[k][d] = 0.0 + (double)GW[0][k][d] + (double)GW[1][k][d] + .., likewise gb[k] and Lk[k] (an fp64
 *             chain over the slabs of L[s][k]); loss = 0.0 + Lk[0] + Lk[1] + .. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

/* exp(t) for t <= 0 (NaN: NaN): n = rintf(t log2 e); r = t - n ln 2 in two fmaf (the high part of ln 2 has 16
 * significant bits: n hi is exact); a degree-6 Horner chain; the scale 2^n as two powers of two -- exact while the
 * result is normal, one rounding into the denormals.  t < -104: 0.  exp(-0) == 1 exactly. */
float n2v_logreg_cpu_exp_neg(float t) {
  if (!(t >= -104.0f)) return t != t ? t : 0.0f;
  const float n = rintf(t * 0x1.715476p+0f);
  float r = fmaf(n, -0x1.62e4p-1f, t);
  r = fmaf(n, -0x1.7f7d1cp-20f, r);
  float p = 0x1.6d7544p-10f;
  p = fmaf(p, r, 0x1.126fb8p-7f);
  p = fmaf(p, r, 0x1.5554acp-5f);
  p = fmaf(p, r, 0x1.555404p-3f);
  p = fmaf(p, r, 0x1.0p-1f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const int32_t ni = (int32_t)n;
  const int32_t n1 = ni / 2, n2 = ni - n1;
  const float s1 = from_bits((uint32_t)(n1 + 127) << 23), s2 = from_bits((uint32_t)(n2 + 127) << 23);
  return (p * s1) * s2;
}

/* log1p(e) for e in [0, 1] (NaN: NaN): e + e^2 g(e), g a degree-13 Horner chain */
float n2v_logreg_cpu_log1p01(float e) {
  float g = 0x1.e52a08p-12f;
  g = fmaf(g, e, -0x1.eb08aap-9f);
  g = fmaf(g, e, 0x1.d275c6p-7f);
  g = fmaf(g, e, -0x1.18da6ep-5f);
  g = fmaf(g, e, 0x1.ed6386p-5f);
  g = fmaf(g, e, -0x1.5d27a2p-4f);
  g = fmaf(g, e, 0x1.b16db6p-4f);
  g = fmaf(g, e, -0x1.fa5fep-4f);
  g = fmaf(g, e, 0x1.241036p-3f);
  g = fmaf(g, e, -0x1.5545d4p-3f);
  g = fmaf(g, e, 0x1.99987ap-3f);
  g = fmaf(g, e, -0x1.fffff6p-3f);
  g = fmaf(g, e, 0x1.555556p-2f);
  g = fmaf(g, e, -0x1.0p-1f);
  const float u = e * g;
  return fmaf(e, u, e);
}

/* one (row, class): e, p = sigmoid(z), res = p - y, l = the logistic loss; out = {e, p, res, l} */
void n2v_logreg_cpu_point(float z, int32_t y, float *out) {
  const float e = n2v_logreg_cpu_exp_neg(-fabsf(z));
  const float num = z >= 0.0f ? 1.0f : e;
  const float den = 1.0f + e;
  const float p = num / den;
  const float yf = y ? 1.0f : 0.0f;
  const float m = y ? -z : z;
  const float hinge = m > 0.0f ? m : 0.0f;
  out[0] = e;
  out[1] = p;
  out[2] = p - yf;
  out[3] = hinge + n2v_logreg_cpu_log1p01(e);
}

void n2v_logreg_cpu_points(const float *z, int64_t count, int32_t y, float *out) {
  for (int64_t i = 0; i < count; ++i) n2v_logreg_cpu_point(z[i], y, out + 4 * i);
}

float n2v_logreg_cpu_dot(const float *w, const float *x, int32_t dim) {
  const int32_t dp = (dim + 15) / 16 * 16;
  float acc = 0.0f;
  for (int32_t d0 = 0; d0 < dp; d0 += 16)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) {
        const int32_t d = d0 + 4 * k + j;
        acc = fmaf(d < dim ? x[d] : 0.0f, d < dim ? w[d] : 0.0f, acc);
      }
  return acc;
}

int64_t n2v_logreg_cpu_slab_rows(int64_t n, int32_t dim, int32_t c) {
  int64_t most = (512ll << 20) / (4 * (int64_t)c * (dim + 3));
  if (most > 2048) most = 2048;
  int64_t share = (n + most - 1) / most;
  if (share < 1) share = 1;
  return (share + 63) / 64 * 64;
}

void n2v_logreg_cpu_scores(const float *X, int64_t n, int32_t dim, const float *W, const float *b, int32_t c,
                           float *Z) {
  for (int64_t r = 0; r < n; ++r)
    for (int32_t k = 0; k < c; ++k) Z[r * c + k] = n2v_logreg_cpu_dot(W + (int64_t)k * dim, X + r * dim, dim) + b[k];
}

/* y_bits: uint32 [n][ceil(c / 32)]; part: scratch of c * dim floats; res: scratch of c floats.
 * Out: loss[1], gW[c * dim], gb[c] doubles. */
void n2v_logreg_cpu_loss_grad(const float *X, const uint32_t *y_bits, int64_t n, int32_t dim, const float *W,
                              const float *b, int32_t c, double *loss, double *gW, double *gb, float *part,
                              float *res) {
  const int64_t slab = n2v_logreg_cpu_slab_rows(n, dim, c);
  const int64_t cd = (int64_t)c * dim;
  const int32_t words = (c + 31) / 32;
  double Lk[1024];
  for (int64_t i = 0; i < cd; ++i) gW[i] = 0.0;
  for (int32_t k = 0; k < c; ++k) gb[k] = 0.0, Lk[k] = 0.0;
  for (int64_t lo = 0; lo < n; lo += slab) {
    const int64_t hi = lo + slab < n ? lo + slab : n;
    const int64_t hi_pad = lo + (hi - lo + 63) / 64 * 64;
    float Gb[1024];
    double L[1024];
    for (int64_t i = 0; i < cd; ++i) part[i] = 0.0f;
    for (int32_t k = 0; k < c; ++k) Gb[k] = 0.0f, L[k] = 0.0;
    for (int64_t r = lo; r < hi; ++r) {
      const float *x = X + r * dim;
      for (int32_t k = 0; k < c; ++k) {
        float o[4];
        const float z = n2v_logreg_cpu_dot(W + (int64_t)k * dim, x, dim) + b[k];
        n2v_logreg_cpu_point(z, (int32_t)((y_bits[r * words + (k >> 5)] >> (k & 31)) & 1u), o);
        res[k] = o[2];
        Gb[k] = Gb[k] + o[2];
        L[k] = L[k] + (double)o[3];
      }
      for (int32_t k = 0; k < c; ++k)
        for (int32_t d = 0; d < dim; ++d) part[(int64_t)k * dim + d] = fmaf(res[k], x[d], part[(int64_t)k * dim + d]);
    }
    for (int64_t r = hi; r < hi_pad; ++r)
      for (int64_t i = 0; i < cd; ++i) part[i] = fmaf(0.0f, 0.0f, part[i]);
    for (int64_t i = 0; i < cd; ++i) gW[i] = gW[i] + (double)part[i];
    for (int32_t k = 0; k < c; ++k) gb[k] = gb[k] + (double)Gb[k], Lk[k] = Lk[k] + L[k];
  }
  double total = 0.0;
  for (int32_t k = 0; k < c; ++k) total = total + Lk[k];
  loss[0] = total;
}
