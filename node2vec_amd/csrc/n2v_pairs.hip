// n2v_pairs.hip -- link prediction over trained vectors (the node2vec paper's section 4.4): for a list of
// vertex pairs (a[i], b[i]) the score of every pair, the paper's four edge features (its Table 1), and
// whether the pair is an edge of a CSR graph.  Read-only on X and on the graph; nothing is allocated, no
// atomics, no LDS, no grid cap: a wave owns 64 consecutive pairs, a block of four waves 256, and the grid is
// ceil(n_pairs / 256).
//
// The score's fixed order (DESIGN.md "Link prediction"; tests/cpu_pairs/n2v_pairs_cpu.c restates it).  It
// depends on dim alone:
//   G = 16 for dim <= 128, 32 for dim <= 256, 64 beyond           (the lanes that share one pair)
//   lane l of the G:  s_l = +0;  for c = l, l + G, l + 2 G, ... while 4 c < dim:
//                       for j = 0 .. 3 while 4 c + j < dim:  s_l = fmaf(x_a[4 c + j], x_b[4 c + j], s_l)
//   then for off = 1, 2, 4, ... < G, in every lane at once:       s_l = s_l + s_(l xor off)
//   dot = s_0 (every lane holds the same bits: fp32 addition commutes)
// fmaf and + commute in their two operands, so dot(a, b) and dot(b, a) are the same bits, and the cosine is
// written dot * (inv_norm[a] * inv_norm[b]) for the same reason.  A pair's place in the list, the number of
// pairs and the launch geometry do not enter.
//
// Shape: the gather is the cost (2 * 4 * dim bytes of randomly placed rows per pair), so a lane group of G
// lanes reads a row in 16-byte pieces, 64 / G pairs side by side in a wave and U of those steps unrolled:
// eight 16-byte loads per lane are issued before the first is used.  Pair indices are loaded one lane per
// pair and broadcast by lane shuffles; scores leave as one contiguous 256-byte run per wave; feature rows
// leave as 16-byte non-temporal stores (they are written once and not read here).  dim % 4 != 0 or a
// pointer that is not 16-byte aligned goes element by element through the same guards (VEC = false).
#include <math.h>

#include "n2v_pair_load.h"

namespace {

template <int G, int K, bool VEC>
__global__ __launch_bounds__(256) void pair_scores_kernel(const float *__restrict__ X,
                                                          const float *__restrict__ inv_norm, int64_t n, int32_t dim,
                                                          const int64_t *__restrict__ a,
                                                          const int64_t *__restrict__ b, int64_t n_pairs,
                                                          float *__restrict__ out) {
  constexpr int GP = 64 / G, U = Unroll<K>::U;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kWavePairs;
  if (p0 >= n_pairs) return;
  const int cnt = n_pairs - p0 < kWavePairs ? (int)(n_pairs - p0) : kWavePairs;
  int32_t ra, rb;
  load_pair(a, b, p0, cnt, n, lane, ra, rb);
  float scale = 1.f;
  if (inv_norm && ra >= 0) scale = inv_norm[ra] * inv_norm[rb];
  const int l = lane % G;
  float res = 0.f;
  for (int base = 0; base < cnt; base += GP * U) {
    f32x4 va[U][K], vb[U][K];
    bool live[U];
    load_step<G, K, VEC>(X, dim, ra, rb, base, lane, va, vb, live);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int c = l + k * G;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * c + j < dim) s = __fmaf_rn(va[u][k][j], vb[u][k][j], s);
      }
#pragma unroll
      for (int off = 1; off < G; off <<= 1) s += __shfl_xor(s, off, 64);
      // the GP dots of this step go to the lanes that own those pairs
      const int d = lane - (base + u * GP);
      const float t = __shfl(s, (d & (GP - 1)) * G, 64);
      if (d >= 0 && d < GP) res = t;
    }
  }
  if (lane < cnt) out[p0 + lane] = ra < 0 ? NAN : inv_norm ? res * scale : res;
}

template <int G, int K, bool VEC>
__global__ __launch_bounds__(256) void pair_features_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                            const int64_t *__restrict__ a,
                                                            const int64_t *__restrict__ b, int64_t n_pairs,
                                                            int32_t op, float *__restrict__ out) {
  constexpr int GP = 64 / G, U = Unroll<K>::U;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kWavePairs;
  if (p0 >= n_pairs) return;
  const int cnt = n_pairs - p0 < kWavePairs ? (int)(n_pairs - p0) : kWavePairs;
  int32_t ra, rb;
  load_pair(a, b, p0, cnt, n, lane, ra, rb);
  const int g = lane / G, l = lane % G;
  for (int base = 0; base < cnt; base += GP * U) {
    f32x4 va[U][K], vb[U][K];
    bool live[U];
    load_step<G, K, VEC>(X, dim, ra, rb, base, lane, va, vb, live);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = base + u * GP + g;
      if (q >= cnt) continue;
      float *o = out + (p0 + q) * (int64_t)dim;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int c = l + k * G;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = live[u] ? feature(op, va[u][k][j], vb[u][k][j]) : NAN;
        if (VEC) {
          if (4 * c < dim) __builtin_nontemporal_store(r, reinterpret_cast<f32x4 *>(o + 4 * c));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * c + j < dim) o[4 * c + j] = r[j];
        }
      }
    }
  }
}

// out_mask[i] = row a[i] of the CSR holds b[i]: one lane per pair, a binary search in the row (col ascends
// within a row, multi-edges adjacent)
__global__ __launch_bounds__(256) void pairs_in_graph_kernel(const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ col, int64_t n_vertices,
                                                             const int64_t *__restrict__ a,
                                                             const int64_t *__restrict__ b, int64_t n_pairs,
                                                             uint8_t *__restrict__ out_mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs) return;
  const int64_t u = a[i], v = b[i];
  uint8_t hit = 0;
  if (u >= 0 && u < n_vertices && v >= 0 && v < n_vertices) {
    int64_t lo = rowptr[u];
    const int64_t end = rowptr[u + 1];
    int64_t hi = end;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)col[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    hit = lo < end && (int64_t)col[lo] == v;
  }
  out_mask[i] = hit;
}

bool grid_of(int64_t n_pairs, unsigned &blocks) {
  const int64_t g = (n_pairs + kBlockPairs - 1) / kBlockPairs;
  if (g > 0x7fffffffLL) return false;
  blocks = (unsigned)g;
  return true;
}

bool sizes_ok(int64_t n, int32_t dim, int64_t n_pairs) { return matrix_ok(n, dim) && n_pairs >= 0; }

}  // namespace

extern "C" {

int n2v_pair_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *a,
                    const int64_t *b, int64_t n_pairs, int32_t metric, float *out_scores, void *stream) {
  if (!sizes_ok(n, dim, n_pairs)) return N2V_EINVAL;
  if (metric != N2V_PAIR_DOT && metric != N2V_PAIR_COSINE) return N2V_EINVAL;
  if (metric == N2V_PAIR_COSINE && !inv_norm) return N2V_EINVAL;
  unsigned blocks = 0;
  if (!grid_of(n_pairs, blocks)) return N2V_EINVAL;
  if (n_pairs == 0) return N2V_OK;
  if (!X || !a || !b || !out_scores) return N2V_EINVAL;
  if (metric == N2V_PAIR_DOT) inv_norm = nullptr;  // ignored
  with_shape(dim, vec_ok(dim, X), [&](auto G, auto K, auto VEC) {
    hipLaunchKernelGGL((pair_scores_kernel<G, K, VEC>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, X, inv_norm,
                       n, dim, a, b, n_pairs, out_scores);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_pair_features(const float *X, int64_t n, int32_t dim, const int64_t *a, const int64_t *b, int64_t n_pairs,
                      int32_t op, float *out, void *stream) {
  if (!sizes_ok(n, dim, n_pairs)) return N2V_EINVAL;
  if (op != N2V_PAIR_AVERAGE && op != N2V_PAIR_HADAMARD && op != N2V_PAIR_L1 && op != N2V_PAIR_L2) return N2V_EINVAL;
  unsigned blocks = 0;
  if (!grid_of(n_pairs, blocks)) return N2V_EINVAL;
  if (n_pairs == 0) return N2V_OK;
  if (!X || !a || !b || !out) return N2V_EINVAL;
  with_shape(dim, vec_ok(dim, X, out), [&](auto G, auto K, auto VEC) {
    hipLaunchKernelGGL((pair_features_kernel<G, K, VEC>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, X, n, dim,
                       a, b, n_pairs, op, out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_pairs_in_graph(const int64_t *rowptr, const int32_t *col, int64_t n_vertices, const int64_t *a,
                       const int64_t *b, int64_t n_pairs, uint8_t *out_mask, void *stream) {
  if (n_vertices < 0 || n_vertices >= ((int64_t)1 << 31) || n_pairs < 0) return N2V_EINVAL;
  unsigned blocks = 0;
  if (!grid_of(n_pairs, blocks)) return N2V_EINVAL;
  if (n_pairs == 0) return N2V_OK;
  if (!rowptr || !a || !b || !out_mask) return N2V_EINVAL;  // (col may be NULL: a graph without edges)
  hipLaunchKernelGGL(pairs_in_graph_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col,
                     n_vertices, a, b, n_pairs, out_mask);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
