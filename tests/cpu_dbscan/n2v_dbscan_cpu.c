/* CPU restatement of node2vec_amd/csrc/n2v_dbscan.hip: the pair test in the kernel's fixed order, the neighbour
 * counts, the components of the core rows by sequential union towards the lowest index, the clusters' ranks and the
 * border rule.  Built with the flags of tests/cpu_build.py (no contraction), so every line below is the fp32
 * operation it spells.  This text is the contract; the kernels are held to its labels and counts exactly.
 *
 * dot(i, j):  acc = +0; for d0 = 0, 16, .. < round_up(dim, 16), e = 0..3, q = 0..3, d = d0 + 4 q + e:
 *             acc = fmaf(x_i[d], x_j[d], acc), both read as 0 at d >= dim.
 * sumsq(v):   s[l] = +0 for l in [0, 64); for d = l, l + 64, .. < dim: s[l] = fmaf(v[d], v[d], s[l]);
 *             for off = 1, 2, 4, .. 32: every s[l] becomes s[l] + s[l ^ off] at once; the result is s[0].
 * within(i, j), i != j:
 *   Euclidean  both = xn_i + xn_j; t = fmaf(-2, dot, both); d2 = fmaxf(t, 0); d2 <= eps2, eps2 = eps * eps
 *   cosine     inv2 = inv_i * inv_j; c = dot * inv2; d = 1 - c; d <= eps
 * Both are symmetric in (i, j) bit for bit (tests/test_dbscan_host.py holds n2v_dbscan_cpu_within to that), so
 * n2v_dbscan_cpu evaluates a pair once.  A row is always within eps of itself: counted by hand, never computed.
 * The hardware's fused multiply-add, where the build finds one, is the same correctly rounded operation as fmaf. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define EUCLIDEAN 0
#define COSINE 1

#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
#define FMA_CLONES __attribute__((target_clones("fma", "default")))
#else
#define FMA_CLONES
#endif

/* dot(i, j0 + k) for k = 0..W-1 at once: W independent chains, each in the order above */
#define W 4
FMA_CLONES static void dot_chains(const float *xi, const float *xj, int32_t dim, float *out) {
  const int32_t dp = (dim + 15) / 16 * 16;
  float acc[W];
  for (int k = 0; k < W; ++k) acc[k] = 0.0f;
  for (int32_t d0 = 0; d0 < dp; d0 += 16) {
    if (d0 + 16 <= dim) {
      for (int e = 0; e < 4; ++e)
        for (int q = 0; q < 4; ++q) {
          const int32_t d = d0 + 4 * q + e;
          for (int k = 0; k < W; ++k) acc[k] = fmaf(xi[d], xj[(int64_t)k * dim + d], acc[k]);
        }
    } else {
      for (int e = 0; e < 4; ++e)
        for (int q = 0; q < 4; ++q) {
          const int32_t d = d0 + 4 * q + e;
          for (int k = 0; k < W; ++k)
            acc[k] = fmaf(d < dim ? xi[d] : 0.0f, d < dim ? xj[(int64_t)k * dim + d] : 0.0f, acc[k]);
        }
    }
  }
  for (int k = 0; k < W; ++k) out[k] = acc[k];
}

static float dot_chain(const float *xi, const float *xj, int32_t dim) {
  const int32_t dp = (dim + 15) / 16 * 16;
  float acc = 0.0f;
  for (int32_t d0 = 0; d0 < dp; d0 += 16)
    for (int e = 0; e < 4; ++e)
      for (int q = 0; q < 4; ++q) {
        const int32_t d = d0 + 4 * q + e;
        acc = fmaf(d < dim ? xi[d] : 0.0f, d < dim ? xj[d] : 0.0f, acc);
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

static int within(int32_t metric, float dot, float ai, float aj, float thr) {
  if (metric == COSINE) {
    const float inv2 = ai * aj;
    const float c = dot * inv2;
    const float d = 1.0f - c;
    return d <= thr;
  }
  const float both = ai + aj;
  const float t = fmaf(-2.0f, dot, both);
  const float d2 = fmaxf(t, 0.0f);
  return d2 <= thr;
}

static float threshold(int32_t metric, float eps) {
  if (metric == COSINE) return eps;
  const float eps2 = eps * eps;
  return eps2;
}

float n2v_dbscan_cpu_dot(const float *xi, const float *xj, int32_t dim) { return dot_chain(xi, xj, dim); }

void n2v_dbscan_cpu_sumsq(const float *X, int64_t n, int32_t dim, float *out) {
  for (int64_t r = 0; r < n; ++r) out[r] = sumsq(X + r * dim, dim);
}

/* inv_norm as n2v_knn_inv_norms writes it */
void n2v_dbscan_cpu_inv_norms(const float *X, int64_t n, int32_t dim, float *out) {
  for (int64_t r = 0; r < n; ++r) {
    const float s = sumsq(X + r * dim, dim);
    out[r] = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
  }
}

/* the pair test with row i on the left: aux = xn (Euclidean) or inv_norm (cosine) */
int32_t n2v_dbscan_cpu_within(const float *X, const float *aux, int32_t dim, int32_t metric, float eps, int64_t i,
                              int64_t j) {
  return within(metric, dot_chain(X + i * dim, X + j * dim, dim), aux[i], aux[j], threshold(metric, eps));
}

static int32_t find(const int32_t *parent, int32_t x) {
  while (parent[x] != x) x = parent[x];
  return x;
}

/* counts [n], core [n] (0 / 1), labels [n] (-1: noise); returns the number of clusters, or -1 without memory.
 * inv_norm: cosine only.  labels may be NULL: the counts alone. */
int32_t n2v_dbscan_cpu(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                       int32_t min_samples, int32_t *counts, uint8_t *core, int32_t *labels) {
  const float thr = threshold(metric, eps);
  float *xn = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
  uint8_t *hit = (uint8_t *)calloc((size_t)(n > 0 ? n * n : 1), 1); /* hit[i n + j], i < j */
  int32_t *parent = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
  if (!xn || !hit || !parent) {
    free(xn), free(hit), free(parent);
    return -1;
  }
  const float *aux = inv_norm;
  if (metric == EUCLIDEAN) {
    for (int64_t r = 0; r < n; ++r) xn[r] = sumsq(X + r * dim, dim);
    aux = xn;
  }
  for (int64_t i = 0; i < n; ++i) {
    int64_t j = i + 1;
    for (; j + W <= n; j += W) {
      float dot[W];
      dot_chains(X + i * dim, X + j * dim, dim, dot);
      for (int k = 0; k < W; ++k) hit[i * n + j + k] = (uint8_t)within(metric, dot[k], aux[i], aux[j + k], thr);
    }
    for (; j < n; ++j)
      hit[i * n + j] = (uint8_t)within(metric, dot_chain(X + i * dim, X + j * dim, dim), aux[i], aux[j], thr);
  }
  /* counts: the self-pair by hand */
  for (int64_t i = 0; i < n; ++i) counts[i] = 1;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j)
      if (hit[i * n + j]) counts[i] += 1, counts[j] += 1;
  for (int64_t i = 0; i < n; ++i) core[i] = counts[i] >= min_samples ? 1 : 0;
  int32_t n_clusters = 0;
  if (labels) {
    /* components of the core rows: the larger root goes under the smaller, so a root is its component's lowest row */
    for (int64_t i = 0; i < n; ++i) parent[i] = (int32_t)i;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = i + 1; j < n; ++j)
        if (core[i] && core[j] && hit[i * n + j]) {
          const int32_t a = find(parent, (int32_t)i), b = find(parent, (int32_t)j);
          if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        }
    /* a cluster's id: the rank of its root among the roots */
    for (int64_t i = 0; i < n; ++i) labels[i] = -1;
    for (int64_t i = 0; i < n; ++i)
      if (core[i] && parent[i] == i) labels[i] = n_clusters++;
    for (int64_t i = 0; i < n; ++i)
      if (core[i]) labels[i] = labels[find(parent, (int32_t)i)];
    /* a row that is not core: the lowest cluster id among the core rows within eps of it */
    for (int64_t b = 0; b < n; ++b) {
      if (core[b]) continue;
      int32_t best = -1;
      for (int64_t c = 0; c < n; ++c) {
        if (!core[c] || !(c < b ? hit[c * n + b] : hit[b * n + c])) continue;
        if (best < 0 || labels[c] < best) best = labels[c];
      }
      labels[b] = best;
    }
  }
  free(xn), free(hit), free(parent);
  return n_clusters;
}
