/* CPU restatement of node2vec_amd/csrc/n2v_pca.hip: which rows are used, the fp64 column means and the scatter
 * matrix of the centred rows.  Built with the flags of tests/cpu_build.py (no contraction), so every line below is
 * the fp32 or fp64 operation it spells.  This text is the contract; the kernels are held to its bits.
 *
 * xh[r][d]:  x[r][d] (inv_norm null) or x[r][d] * inv_norm[r], one fp32 multiply.  Row r is USED when all dim
 *            values of xh[r] are finite; every other row is skipped by both passes and not counted.
 * slabs:     S = min(2048, 512 MiB / (4 round_up(dim, 16)^2)); slab_rows = round_up(max(1, ceil(n / S)), 64).
 *            Both passes also take explicit slab bounds (`bounds`: n_slabs + 1 ascending row numbers), so that a
 *            matrix whose skipped rows were deleted can be cut where the full matrix was.
 * mean:      a step is 64 rows counted from the slab's first row; rows 16 w .. 16 w + 15 of every step belong to
 *            wave w = 0..3.  Per slab s, column d and wave w: c_w = 0.0; c_w = c_w + (double)xh[r][d] over the
 *            wave's used rows ascending; M[s][d] = ((c_0 + c_1) + c_2) + c_3.
 *            mean[d] = (0.0 + M[0][d] + M[1][d] + ..) / (double)n_used; zeros when n_used == 0.
 * scatter:   xc[r][d] = xh[r][d] - center[d], one fp32 subtraction (center null: xc = xh).  Per slab and a <= b:
 *            acc = +0; over the slab's rows ascending acc = fmaf(xc[r][a], xc[r][b], acc) for a used row and
 *            acc = fmaf(+0, +0, acc) for a skipped one, then the same for every row that pads the slab to a
 *            multiple of 64 rows (a -0 accumulator becomes +0).
 *            S[a][b] = S[b][a] = 0.0 + (double)acc_0 + (double)acc_1 + .. over the slabs ascending. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

int64_t n2v_pca_cpu_slab_rows(int64_t n, int32_t dim) {
  const int64_t dp = (dim + 15) / 16 * 16;
  int64_t most = (512ll << 20) / (4 * dp * dp);
  if (most > 2048) most = 2048;
  int64_t share = (n + most - 1) / most;
  if (share < 1) share = 1;
  return (share + 63) / 64 * 64;
}

/* xh of row r into out[dim]; returns whether the row is used */
static int scaled_row(const float *X, const float *inv_norm, int64_t r, int32_t dim, float *out) {
  int used = 1;
  for (int32_t d = 0; d < dim; ++d) {
    float x = X[r * dim + d];
    if (inv_norm) x = x * inv_norm[r];
    out[d] = x;
    if (!isfinite(x)) used = 0;
  }
  return used;
}

void n2v_pca_cpu_mean_slabs(const float *X, const float *inv_norm, int32_t dim, const int64_t *bounds,
                            int32_t n_slabs, double *mean, int64_t *n_used) {
  float *xh = malloc(sizeof(float) * (size_t)dim);
  double *c = malloc(sizeof(double) * 4 * (size_t)dim);
  int64_t used_rows = 0;
  for (int32_t d = 0; d < dim; ++d) mean[d] = 0.0;
  for (int32_t s = 0; s < n_slabs; ++s) {
    for (int32_t i = 0; i < 4 * dim; ++i) c[i] = 0.0;
    for (int64_t r = bounds[s]; r < bounds[s + 1]; ++r) {
      if (!scaled_row(X, inv_norm, r, dim, xh)) continue;
      ++used_rows;
      double *cw = c + (size_t)(((r - bounds[s]) >> 4) & 3) * dim;
      for (int32_t d = 0; d < dim; ++d) cw[d] = cw[d] + (double)xh[d];
    }
    for (int32_t d = 0; d < dim; ++d) {
      const double m = ((c[d] + c[dim + d]) + c[2 * dim + d]) + c[3 * dim + d];
      mean[d] = mean[d] + m;
    }
  }
  for (int32_t d = 0; d < dim; ++d) mean[d] = used_rows > 0 ? mean[d] / (double)used_rows : 0.0;
  n_used[0] = used_rows;
  free(xh);
  free(c);
}

void n2v_pca_cpu_scatter_slabs(const float *X, const float *inv_norm, int32_t dim, const float *center,
                               const int64_t *bounds, int32_t n_slabs, double *S, int64_t *n_used) {
  float *xc = malloc(sizeof(float) * (size_t)dim);
  float *acc = malloc(sizeof(float) * (size_t)dim * dim);
  int64_t used_rows = 0;
  for (int64_t i = 0; i < (int64_t)dim * dim; ++i) S[i] = 0.0;
  for (int32_t s = 0; s < n_slabs; ++s) {
    const int64_t lo = bounds[s], hi = bounds[s + 1];
    const int64_t hi_pad = lo + (hi - lo + 63) / 64 * 64;
    for (int64_t i = 0; i < (int64_t)dim * dim; ++i) acc[i] = 0.0f;
    for (int64_t r = lo; r < hi_pad; ++r) {
      int used = r < hi && scaled_row(X, inv_norm, r, dim, xc);
      if (used) {
        ++used_rows;
        if (center)
          for (int32_t d = 0; d < dim; ++d) xc[d] = xc[d] - center[d];
      } else {
        for (int32_t d = 0; d < dim; ++d) xc[d] = 0.0f;
      }
      for (int32_t a = 0; a < dim; ++a)
        for (int32_t b = a; b < dim; ++b) acc[(int64_t)a * dim + b] = fmaf(xc[a], xc[b], acc[(int64_t)a * dim + b]);
    }
    for (int32_t a = 0; a < dim; ++a)
      for (int32_t b = a; b < dim; ++b) {
        const double v = S[(int64_t)a * dim + b] + (double)acc[(int64_t)a * dim + b];
        S[(int64_t)a * dim + b] = v;
        S[(int64_t)b * dim + a] = v;
      }
  }
  n_used[0] = used_rows;
  free(xc);
  free(acc);
}

static int64_t *plain_bounds(int64_t n, int32_t dim, int32_t *n_slabs) {
  const int64_t slab = n2v_pca_cpu_slab_rows(n, dim);
  *n_slabs = (int32_t)((n + slab - 1) / slab);
  int64_t *b = malloc(sizeof(int64_t) * ((size_t)*n_slabs + 1));
  for (int32_t s = 0; s <= *n_slabs; ++s) b[s] = s * slab < n ? s * slab : n;
  return b;
}

void n2v_pca_cpu_mean(const float *X, const float *inv_norm, int64_t n, int32_t dim, double *mean, int64_t *n_used) {
  int32_t n_slabs;
  int64_t *b = plain_bounds(n, dim, &n_slabs);
  n2v_pca_cpu_mean_slabs(X, inv_norm, dim, b, n_slabs, mean, n_used);
  free(b);
}

void n2v_pca_cpu_scatter(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *center,
                         double *S, int64_t *n_used) {
  int32_t n_slabs;
  int64_t *b = plain_bounds(n, dim, &n_slabs);
  n2v_pca_cpu_scatter_slabs(X, inv_norm, dim, center, b, n_slabs, S, n_used);
  free(b);
}
