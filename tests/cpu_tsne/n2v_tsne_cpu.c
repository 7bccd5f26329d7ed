/* The CPU restatement of csrc/n2v_tsne.hip: the same fp32 / fp64 operations in the same order, one rounding per
 * spelled operation (compiled by tests/cpu_build.py without contraction).  The plan (tile, slab_cols, n_slabs) is an
 * argument: the tests pass what n2v_tsne_plan gives, or numbers of their own. */
#include <math.h>
#include <stdint.h>

typedef struct {
  float dx, dy, w;
} pair_t;

static pair_t pair_of(const float *yi, const float *yj) {
  pair_t p;
  p.dx = yi[0] - yj[0];
  p.dy = yi[1] - yj[1];
  const float sq = p.dx * p.dx;
  const float d2 = fmaf(p.dy, p.dy, sq);
  const float den = 1.0f + d2;
  p.w = 1.0f / den;
  return p;
}

/* the rows `rows[0 .. m)` (NULL: every row, m == n): rep_out [m][2], zrow_out [m] */
void n2v_tsne_cpu_repulse(const float *Y, int64_t n, int32_t tile, int64_t slab_cols, int32_t n_slabs,
                          const int64_t *rows, int64_t m, double *rep_out, double *zrow_out) {
  for (int64_t k = 0; k < m; ++k) {
    const int64_t i = rows ? rows[k] : k;
    const float *yi = Y + 2 * i;
    double X = 0.0, Yy = 0.0, W = 0.0;
    for (int32_t s = 0; s < n_slabs; ++s) {
      const int64_t lo = (int64_t)s * slab_cols;
      const int64_t hi = lo + slab_cols < n ? lo + slab_cols : n;
      double ax = 0.0, ay = 0.0, aw = 0.0;
      for (int64_t t0 = lo; t0 < hi; t0 += tile) {
        const int64_t t1 = t0 + tile < hi ? t0 + tile : hi;
        float sw = 0.f, sx = 0.f, sy = 0.f;
        for (int64_t j = t0; j < t1; ++j) {
          if (j == i) continue;
          const pair_t p = pair_of(yi, Y + 2 * j);
          sw = sw + p.w;
          const float w2 = p.w * p.w;
          sx = fmaf(w2, p.dx, sx);
          sy = fmaf(w2, p.dy, sy);
        }
        ax = ax + (double)sx;
        ay = ay + (double)sy;
        aw = aw + (double)sw;
      }
      X = X + ax;
      Yy = Yy + ay;
      W = W + aw;
    }
    rep_out[2 * k] = X;
    rep_out[2 * k + 1] = Yy;
    zrow_out[k] = W;
  }
}

/* Z of zrow [n]: blocks of 256 rows, rows ascending, then blocks ascending */
double n2v_tsne_cpu_z(const double *zrow, int64_t n) {
  double z = 0.0;
  for (int64_t b0 = 0; b0 < n; b0 += 256) {
    const int64_t b1 = b0 + 256 < n ? b0 + 256 : n;
    double b = 0.0;
    for (int64_t i = b0; i < b1; ++i) b = b + zrow[i];
    z = z + b;
  }
  return z;
}

static float butterfly16(float *v) {
  for (int msk = 8; msk > 0; msk >>= 1) {
    float t[16];
    for (int l = 0; l < 16; ++l) t[l] = v[l] + v[l ^ msk];
    for (int l = 0; l < 16; ++l) v[l] = t[l];
  }
  return v[0];
}

static void update(float a, double rep, double z, float exaggeration, float learning_rate, float momentum,
                   float min_gain, float y, float *vel, float *gain, float *y_next, float *grad) {
  const float r = (float)(rep / z);
  const float t = exaggeration * a;
  const float u = t - r;
  const float g = 4.0f * u;
  float gn;
  if ((g > 0.f) != (*vel > 0.f)) gn = *gain + 0.2f;
  else gn = *gain * 0.8f;
  gn = fmaxf(gn, min_gain);
  const float p1 = momentum * *vel;
  const float p2 = gn * g;
  const float p3 = learning_rate * p2;
  const float v = p1 - p3;
  *grad = g;
  *gain = gn;
  *vel = v;
  *y_next = y + v;
}

void n2v_tsne_cpu_step(const int64_t *rowptr, const int32_t *col, const float *val, int64_t nnz, const float *Y,
                       const double *rep, double z, int64_t n, float exaggeration, float learning_rate,
                       float momentum, float min_gain, float *vel, float *gain, float *Y_next, float *grad) {
  for (int64_t i = 0; i < n; ++i) {
    float ax[16], ay[16];
    int64_t lo = rowptr[i], hi = rowptr[i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > nnz ? nnz : hi;
    for (int l = 0; l < 16; ++l) {
      ax[l] = ay[l] = 0.f;
      for (int64_t e = lo + l; e < hi; e += 16) {
        const int32_t j = col[e];
        if (j < 0 || j >= n) continue;
        const pair_t p = pair_of(Y + 2 * i, Y + 2 * (int64_t)j);
        const float a = val[e] * p.w;
        ax[l] = fmaf(a, p.dx, ax[l]);
        ay[l] = fmaf(a, p.dy, ay[l]);
      }
    }
    const float sx = butterfly16(ax), sy = butterfly16(ay);
    for (int c = 0; c < 2; ++c)
      update(c ? sy : sx, rep[2 * i + c], z, exaggeration, learning_rate, momentum, min_gain, Y[2 * i + c],
             vel + 2 * i + c, gain + 2 * i + c, Y_next + 2 * i + c, grad + 2 * i + c);
  }
}
