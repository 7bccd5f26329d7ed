/* CPU restatement of node2vec_amd/csrc/n2v_edge_logreg.hip: the score of a pair's edge feature against one weight
 * vector, and the slab chains of the fused loss-and-gradient pass with their fp64 fold.  Built with the flags of
 * tests/cpu_build.py (no contraction), so every line below is the fp32 or fp64 operation it spells.  This text is the
 * contract; the kernels are held to its bits.  The pieces it shares with the two older restatements are those
 * restatements themselves: the feature and the dot of tests/cpu_pairs, the logistic point and the slab rule of
 * tests/cpu_logreg.
 *
 * f[d] = op(x_a[d], x_b[d]) (n2v_pairs_cpu_features);  z = n2v_pairs_cpu_dot(w, f) + b0;  a pair with an index outside
 * [0, n) has z = NaN.  res, l = n2v_logreg_cpu_point(z, y != 0).
 * S = n2v_logreg_cpu_slab_rows(n_pairs, dim, 1) pairs per slab; P = 64 / G lane groups, G the lane group of the dot.
 * Slab s, group t (64 pairs), place q of the group: chain (v, g) = (t mod 4, q mod P).
 *   chain:   acc[d] = +0, cb = +0, cl = 0.0; over its pairs, t then q ascending: acc[d] = fmaf(res, f[d], acc[d]);
 *            cb = cb + res; cl = cl + (double)l.  The places past the slab's last pair belong to no chain.
 *   groups:  for off = 1, 2, .. < P, every g at once: chain (v, g) = chain (v, g) + chain (v, g xor off).
 *   waves:   GW[s][d] = ((c(0, 0) + c(1, 0)) + c(2, 0)) + c(3, 0) in fp32, likewise Gb[s]; L[s] the same in fp64.
 *   slabs:   gw[d] = 0.0 + (double)GW[0][d] + (double)GW[1][d] + .., likewise gb; loss = 0.0 + L[0] + L[1] + ..
 * A chain without pairs is +0, so a chain that has underflowed to -0 survives only where every chain it meets is -0
 * as well, and the fp64 fold from 0.0 never returns -0. */
#include "../cpu_logreg/n2v_logreg_cpu.c"
#include "../cpu_pairs/n2v_pairs_cpu.c"

int64_t n2v_edge_logreg_cpu_slab_pairs(int64_t n_pairs, int32_t dim) {
  return n2v_logreg_cpu_slab_rows(n_pairs, dim, 1);
}

/* f: dim floats of scratch per call; returns z */
static float edge_score(const float *X, int64_t n, int32_t dim, int64_t ia, int64_t ib, int32_t op, const float *w,
                        float b0, float *f) {
  n2v_pairs_cpu_features(X, n, dim, &ia, &ib, 1, op, f);
  if (ia < 0 || ia >= n || ib < 0 || ib >= n) return NAN;
  return n2v_pairs_cpu_dot(w, f, dim) + b0;
}

void n2v_edge_logreg_cpu_scores(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                                int64_t n_pairs, int32_t op, const float *w, float b0, float *z) {
  float f[1024];
  for (int64_t i = 0; i < n_pairs; ++i) z[i] = edge_score(X, n, dim, a[i], b[i], op, w, b0, f);
}

/* Out: loss[1], gw[dim], gb[1] doubles. */
void n2v_edge_logreg_cpu_loss_grad(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                                   const uint8_t *y, int64_t n_pairs, int32_t op, const float *w, float b0,
                                   double *loss, double *gw, double *gb) {
  static float acc[4][4][1024], tmp[4][1024];
  const int G = dim <= 128 ? 16 : dim <= 256 ? 32 : 64;
  const int P = 64 / G;
  const int64_t slab = n2v_edge_logreg_cpu_slab_pairs(n_pairs, dim);
  float f[1024];
  for (int32_t d = 0; d < dim; ++d) gw[d] = 0.0;
  gb[0] = 0.0;
  loss[0] = 0.0;
  for (int64_t lo = 0; lo < n_pairs; lo += slab) {
    const int64_t hi = lo + slab < n_pairs ? lo + slab : n_pairs;
    float cb[4][4], tb[4];
    double cl[4][4], tl[4];
    for (int v = 0; v < 4; ++v)
      for (int g = 0; g < P; ++g) {
        cb[v][g] = 0.0f, cl[v][g] = 0.0;
        for (int32_t d = 0; d < dim; ++d) acc[v][g][d] = 0.0f;
      }
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t t = (i - lo) / 64;
      const int v = (int)(t % 4), g = (int)((i - lo) % 64 % P);
      float o[4];
      const float z = edge_score(X, n, dim, a[i], b[i], op, w, b0, f);
      n2v_logreg_cpu_point(z, y[i] != 0, o);
      for (int32_t d = 0; d < dim; ++d) acc[v][g][d] = fmaf(o[2], f[d], acc[v][g][d]);
      cb[v][g] = cb[v][g] + o[2];
      cl[v][g] = cl[v][g] + (double)o[3];
    }
    for (int v = 0; v < 4; ++v)
      for (int off = 1; off < P; off <<= 1) {
        for (int g = 0; g < P; ++g) {
          for (int32_t d = 0; d < dim; ++d) tmp[g][d] = acc[v][g][d] + acc[v][g ^ off][d];
          tb[g] = cb[v][g] + cb[v][g ^ off];
          tl[g] = cl[v][g] + cl[v][g ^ off];
        }
        for (int g = 0; g < P; ++g) {
          for (int32_t d = 0; d < dim; ++d) acc[v][g][d] = tmp[g][d];
          cb[v][g] = tb[g];
          cl[v][g] = tl[g];
        }
      }
    for (int32_t d = 0; d < dim; ++d) {
      float p = acc[0][0][d] + acc[1][0][d];
      p = p + acc[2][0][d];
      p = p + acc[3][0][d];
      gw[d] = gw[d] + (double)p;
    }
    float p = cb[0][0] + cb[1][0];
    p = p + cb[2][0];
    p = p + cb[3][0];
    gb[0] = gb[0] + (double)p;
    double q = cl[0][0] + cl[1][0];
    q = q + cl[2][0];
    q = q + cl[3][0];
    loss[0] = loss[0] + q;
  }
}
