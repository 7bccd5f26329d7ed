/* CPU restatement of node2vec_amd/csrc/n2v_pairs.hip: the pair score in the kernel's fixed order and the
 * four edge features.  Built with the flags of tests/cpu_build.py (no contraction), so every line below is
 * the fp32 operation it spells.
 *
 * The order of a dot product of `dim` elements (it depends on dim alone):
 *   G = 16 for dim <= 128, 32 for dim <= 256, 64 beyond
 *   s[l] = +0 for l in [0, G);  for c = l, l + G, ... while 4 c < dim, j = 0 .. 3 while 4 c + j < dim:
 *       s[l] = fmaf(a[4 c + j], b[4 c + j], s[l])
 *   for off = 1, 2, 4, ... < G:  every s[l] becomes s[l] + s[l ^ off] at once
 *   the dot is s[0]. */
#include <math.h>
#include <stdint.h>

float n2v_pairs_cpu_dot(const float *a, const float *b, int32_t dim) {
  const int G = dim <= 128 ? 16 : dim <= 256 ? 32 : 64;
  float s[64], t[64];
  for (int l = 0; l < G; ++l) {
    s[l] = 0.0f;
    for (int c = l; 4 * c < dim; c += G)
      for (int j = 0; j < 4 && 4 * c + j < dim; ++j) s[l] = fmaf(a[4 * c + j], b[4 * c + j], s[l]);
  }
  for (int off = 1; off < G; off <<= 1) {
    for (int l = 0; l < G; ++l) t[l] = s[l] + s[l ^ off];
    for (int l = 0; l < G; ++l) s[l] = t[l];
  }
  return s[0];
}

/* metric 0: dot; 1: dot * (inv_norm[a] * inv_norm[b]).  An index outside [0, n) scores NaN. */
void n2v_pairs_cpu_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *a,
                          const int64_t *b, int64_t n_pairs, int32_t metric, float *out) {
  for (int64_t i = 0; i < n_pairs; ++i) {
    if (a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n) {
      out[i] = NAN;
      continue;
    }
    const float d = n2v_pairs_cpu_dot(X + a[i] * dim, X + b[i] * dim, dim);
    out[i] = metric == 1 ? d * (inv_norm[a[i]] * inv_norm[b[i]]) : d;
  }
}

/* op 0: (x + y) * 0.5f, 1: x * y, 2: fabsf(x - y), 3: (x - y) * (x - y) */
void n2v_pairs_cpu_features(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                            int64_t n_pairs, int32_t op, float *out) {
  for (int64_t i = 0; i < n_pairs; ++i) {
    float *o = out + i * dim;
    const int dead = a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n;
    for (int32_t d = 0; d < dim; ++d) {
      if (dead) {
        o[d] = NAN;
        continue;
      }
      const float x = X[a[i] * dim + d], y = X[b[i] * dim + d];
      if (op == 0) {
        const float sum = x + y;
        o[d] = sum * 0.5f;
      } else if (op == 1) {
        o[d] = x * y;
      } else if (op == 2) {
        o[d] = fabsf(x - y);
      } else {
        const float diff = x - y;
        o[d] = diff * diff;
      }
    }
  }
}
