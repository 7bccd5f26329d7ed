/*
 * n2v_oracle_knn.c -- CPU restatement of the nearest-neighbour kernels (node2vec_amd/csrc/n2v_knn.hip).
 *
 * TEST INFRASTRUCTURE ONLY (see n2v_oracle.h).
 *
 * Every fp32 operation of the kernels, in their order, so that the GPU results can be compared bit for bit
 * (DESIGN.md "Nearest neighbours"):
 *   - sum of squares: 64 partial sums, lane l accumulates s[l] = fmaf(x[d], x[d], s[l]) for
 *     d = l, l + 64, ...; then the xor butterfly s[l] = s[l] + s[l ^ off] for off = 1, 2, ..., 32, all lanes
 *     at once; the result is s[0].  inv = s > 0 ? 1 / sqrtf(s) : 0 (both correctly rounded on gfx950 too);
 *   - the normalised query: q_hat[d] = v[d] * inv for d < dim, 0 up to dp = round_up(dim, 16); a query given
 *     as row r uses inv_norm[r];
 *   - the dot product: acc = 0; for d0 = 0, 16, ... < dp: for j in 0..3: for k in 0..3: d = d0 + 4 k + j,
 *     acc = fmaf(x[d] (0 past dim), q_hat[d], acc) -- the v_mfma_f32_16x16x4_f32 chain of score_tile (an f32
 *     MFMA is a k-ordered fmaf chain), padded terms included; score = acc * inv_norm[r];
 *   - top k: score descending, then row ascending; a NaN score is never selected; the tail is (-1, -inf).
 * Compiled with -ffp-contract=off: every * and + below is one rounded fp32 operation.
 */
#include <math.h>
#include <stdlib.h>

#include "n2v_oracle.h"

static float sumsq(const float *v, int32_t dim) {
  float s[64];
  for (int l = 0; l < 64; ++l) {
    s[l] = 0.f;
    for (int32_t d = l; d < dim; d += 64) s[l] = fmaf(v[d], v[d], s[l]);
  }
  for (int off = 1; off < 64; off <<= 1) {
    float t[64];
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    for (int l = 0; l < 64; ++l) s[l] = t[l];
  }
  return s[0];
}

static float inv_sqrt_or_zero(float s) { return s > 0.f ? 1.f / sqrtf(s) : 0.f; }

static int32_t dim_pad(int32_t dim) { return (dim + 15) / 16 * 16; }

static int args_ok(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                   const int64_t *query_rows, int64_t nq) {
  if (!X || !inv_norm || dim < 1 || dim > 1024 || n < 0 || nq < 0) return 0;
  if ((queries == NULL) == (query_rows == NULL)) return 0;
  if (query_rows)
    for (int64_t q = 0; q < nq; ++q)
      if (query_rows[q] < 0 || query_rows[q] >= n) return 0;
  return 1;
}

int n2v_oracle_knn_inv_norms(const float *X, int64_t n, int32_t dim, float *inv_norm) {
  if (!X || !inv_norm || dim < 1 || dim > 1024 || n < 0) return N2V_ORACLE_EINVAL;
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < n; ++r) inv_norm[r] = inv_sqrt_or_zero(sumsq(X + r * dim, dim));
  return N2V_ORACLE_OK;
}

/* q_hat [dp] of query q */
static void query_hat(const float *X, const float *inv_norm, int32_t dim, const float *queries,
                      const int64_t *query_rows, int64_t q, float *qh) {
  const float *v;
  float inv;
  if (query_rows) {
    v = X + query_rows[q] * dim;
    inv = inv_norm[query_rows[q]];
  } else {
    v = queries + q * dim;
    inv = inv_sqrt_or_zero(sumsq(v, dim));
  }
  for (int32_t d = 0; d < dim_pad(dim); ++d) qh[d] = d < dim ? v[d] * inv : 0.f;
}

/* every score of one query; order 0: the kernel's, 1: plain sequential d (for the specificity test only) */
static void score_row(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *qh, int order,
                      float *out) {
  const int32_t dp = dim_pad(dim);
  for (int64_t r = 0; r < n; ++r) {
    const float *x = X + r * dim;
    float acc = 0.f;
    if (order == 0) {
      for (int32_t d0 = 0; d0 < dp; d0 += 16)
        for (int j = 0; j < 4; ++j)
          for (int k = 0; k < 4; ++k) {
            const int32_t d = d0 + 4 * k + j;
            acc = fmaf(d < dim ? x[d] : 0.f, qh[d], acc);
          }
    } else {
      for (int32_t d = 0; d < dim; ++d) acc = fmaf(x[d], qh[d], acc);
    }
    out[r] = acc * inv_norm[r];
  }
}

int n2v_oracle_knn_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                          const int64_t *query_rows, int64_t nq, int32_t order, float *out) {
  if (!args_ok(X, inv_norm, n, dim, queries, query_rows, nq) || !out || order < 0 || order > 1)
    return N2V_ORACLE_EINVAL;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t q = 0; q < nq; ++q) {
    float qh[1024];
    query_hat(X, inv_norm, dim, queries, query_rows, q, qh);
    score_row(X, inv_norm, n, dim, qh, order, out + q * n);
  }
  return N2V_ORACLE_OK;
}

typedef struct {
  float s;
  int64_t r;
} cand;

/* score descending, then row ascending */
static int cand_cmp(const void *pa, const void *pb) {
  const cand *a = (const cand *)pa, *b = (const cand *)pb;
  if (a->s != b->s) return a->s > b->s ? -1 : 1;
  return a->r < b->r ? -1 : (a->r > b->r);
}

int n2v_oracle_knn_topk(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                        const int64_t *query_rows, int64_t nq, int32_t k, const int64_t *exclude_rows,
                        int64_t *out_rows, float *out_scores) {
  if (!args_ok(X, inv_norm, n, dim, queries, query_rows, nq) || k < 1 || !out_rows || !out_scores)
    return N2V_ORACLE_EINVAL;
  int bad = 0;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t q = 0; q < nq; ++q) {
    float qh[1024];
    float *s = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    cand *c = (cand *)malloc(sizeof(cand) * (size_t)(n > 0 ? n : 1));
    if (!s || !c) {
#pragma omp atomic write
      bad = 1;
    } else {
      query_hat(X, inv_norm, dim, queries, query_rows, q, qh);
      score_row(X, inv_norm, n, dim, qh, 0, s);
      int64_t m = 0;
      for (int64_t r = 0; r < n; ++r) {
        if (isnan(s[r]) || (exclude_rows && exclude_rows[q] == r)) continue;
        c[m].s = s[r];
        c[m].r = r;
        ++m;
      }
      qsort(c, (size_t)m, sizeof(cand), cand_cmp);
      for (int32_t i = 0; i < k; ++i) {
        out_rows[q * k + i] = i < m ? c[i].r : -1;
        out_scores[q * k + i] = i < m ? c[i].s : -INFINITY;
      }
    }
    free(s);
    free(c);
  }
  return bad ? N2V_ORACLE_ENOMEM : N2V_ORACLE_OK;
}
