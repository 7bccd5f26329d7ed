/* CPU restatement of node2vec_amd/csrc/n2v_silhouette.hip: the silhouette of every scored row in the kernel's fixed
 * order.  Built with the flags of tests/cpu_build.py (no contraction), so every line below is the fp32 or fp64
 * operation it spells.  This text is the contract; the kernels are held to its bits.
 *
 * dot(i, j):  acc = +0; for d0 = 0, 16, .. < round_up(dim, 16), e = 0..3, q = 0..3, d = d0 + 4 q + e:
 *             acc = fmaf(x_j[d], x_i[d], acc), both read as 0 at d >= dim.
 * sumsq(v):   s[l] = +0 for l in [0, 64); for d = l, l + 64, .. < dim: s[l] = fmaf(v[d], v[d], s[l]);
 *             for off = 1, 2, 4, .. 32: every s[l] becomes s[l] + s[l ^ off] at once; the result is s[0].
 * the list:   the rows of label 0 ascending, dead entries (-1) up to a multiple of 16, the rows of label 1, ...
 *             A label outside [0, k) is no label: the row is in no segment and in no count.
 * S(i, c):    four fp64 chains p[0..3] from 0 over the tiles (16 entries) of segment c in ascending order; chain g
 *             adds (double)d(i, j) of the tile's entries 4 g + e, e = 0..3, in that order, skipping dead entries
 *             and j == i (by index).  S = (p[0] + p[1]) + (p[2] + p[3]).
 * Nothing depends on which rows are scored together, or in which order. */
#include <math.h>
#include <stdint.h>

#define EUCLIDEAN 0
#define COSINE 1

static float dot_chain(const float *xj, const float *xi, int32_t dim) {
  const int32_t dp = (dim + 15) / 16 * 16;
  float acc = 0.0f;
  for (int32_t d0 = 0; d0 < dp; d0 += 16)
    for (int e = 0; e < 4; ++e)
      for (int q = 0; q < 4; ++q) {
        const int32_t d = d0 + 4 * q + e;
        acc = fmaf(d < dim ? xj[d] : 0.0f, d < dim ? xi[d] : 0.0f, acc);
      }
  return acc;
}

static float sumsq(const float *v, int32_t dim) {
  float s[64], t[64];
  for (int l = 0; l < 64; ++l) {
    s[l] = 0.0f;
    for (int32_t d = l; d < dim; d += 64) s[l] = fmaf(v[d], v[d], s[l]);
  }
  for (int off = 1; off < 64; off <<= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    for (int l = 0; l < 64; ++l) s[l] = t[l];
  }
  return s[0];
}

float n2v_silhouette_cpu_dot(const float *xj, const float *xi, int32_t dim) { return dot_chain(xj, xi, dim); }

/* inv_norm as n2v_knn_inv_norms writes it */
void n2v_silhouette_cpu_inv_norms(const float *X, int64_t n, int32_t dim, float *out) {
  for (int64_t r = 0; r < n; ++r) {
    const float s = sumsq(X + r * dim, dim);
    out[r] = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
  }
}

/* fp32 d(i, j); aux = xn (Euclidean) or inv_norm (cosine) */
float n2v_silhouette_cpu_dist(const float *X, const float *aux, int32_t dim, int32_t metric, int64_t i, int64_t j) {
  const float dot = dot_chain(X + j * dim, X + i * dim, dim);
  if (metric == COSINE) {
    const float scaled = dot * aux[j];
    const float both = scaled * aux[i];
    return 1.0f - both;
  }
  const float t = fmaf(-2.0f, dot, aux[i]);
  const float sum = t + aux[j];
  return sqrtf(fmaxf(sum, 0.0f));
}

/* counts [k]; seg_off [k + 1]; list [n + 16 k] (the entries past seg_off[k] are not written); returns seg_off[k] */
int64_t n2v_silhouette_cpu_list(const int32_t *labels, int64_t n, int32_t k, int64_t *counts, int64_t *seg_off,
                                int32_t *list) {
  for (int32_t c = 0; c < k; ++c) counts[c] = 0;
  for (int64_t r = 0; r < n; ++r)
    if (labels[r] >= 0 && labels[r] < k) counts[labels[r]] += 1;
  seg_off[0] = 0;
  for (int32_t c = 0; c < k; ++c) seg_off[c + 1] = seg_off[c] + (counts[c] + 15) / 16 * 16;
  for (int64_t at = 0; at < seg_off[k]; ++at) list[at] = -1;
  for (int32_t c = 0; c < k; ++c) {
    int64_t at = seg_off[c];
    for (int64_t r = 0; r < n; ++r)
      if (labels[r] == c) list[at++] = (int32_t)r;
  }
  return seg_off[k];
}

/* rows: NULL (every row, m == n) or [m]; xn_scratch [n] floats, seg_off [k + 1], list [n + 16 k];
 * sums_out: NULL or [m][k], S(i, c) of every scored row (0 for a row that is not scored) */
void n2v_silhouette_cpu(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int32_t *labels,
                        int32_t k, int32_t metric, const int64_t *rows, int64_t m, double *a_out, double *b_out,
                        double *s_out, int32_t *nearest_out, int64_t *counts, float *xn_scratch, int64_t *seg_off,
                        int32_t *list, double *sums_out) {
  n2v_silhouette_cpu_list(labels, n, k, counts, seg_off, list);
  const float *aux = inv_norm;
  if (metric == EUCLIDEAN) {
    for (int64_t r = 0; r < n; ++r) xn_scratch[r] = sumsq(X + r * dim, dim);
    aux = xn_scratch;
  }
  for (int64_t q = 0; q < m; ++q) {
    int64_t i = rows ? rows[q] : q;
    if (i < 0 || i >= n) i = -1; /* not a row: as a row of label -1 */
    int32_t L = -1;
    if (i >= 0 && labels[i] >= 0 && labels[i] < k) L = labels[i];
    if (sums_out)
      for (int32_t c = 0; c < k; ++c) sums_out[q * k + c] = 0.0;
    if (L < 0) {
      a_out[q] = b_out[q] = s_out[q] = NAN;
      nearest_out[q] = -1;
      continue;
    }
    double a = 0.0, b = INFINITY;
    int32_t nearest = -1;
    for (int32_t c = 0; c < k; ++c) {
      if (counts[c] == 0) continue;
      double p[4] = {0.0, 0.0, 0.0, 0.0};
      for (int64_t tile = seg_off[c]; tile < seg_off[c + 1]; tile += 16)
        for (int g = 0; g < 4; ++g)
          for (int e = 0; e < 4; ++e) {
            const int32_t j = list[tile + 4 * g + e];
            if (j < 0 || j == i) continue;
            const float d = n2v_silhouette_cpu_dist(X, aux, dim, metric, i, j);
            p[g] = p[g] + (double)d;
          }
      const double lo = p[0] + p[1];
      const double hi = p[2] + p[3];
      const double S = lo + hi;
      if (sums_out) sums_out[q * k + c] = S;
      if (c == L) {
        a = counts[c] > 1 ? S / (double)(counts[c] - 1) : 0.0;
      } else {
        const double mean = S / (double)counts[c];
        if (mean < b) b = mean, nearest = c;
      }
    }
    double s;
    if (counts[L] == 1 || nearest < 0) {
      s = 0.0;
    } else {
      const double mx = a > b ? a : b;
      s = mx == 0.0 ? 0.0 : (b - a) / mx;
    }
    a_out[q] = a;
    b_out[q] = b;
    s_out[q] = s;
    nearest_out[q] = nearest;
  }
}
