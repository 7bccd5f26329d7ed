// n2v_silhouette.hip -- silhouette coefficients of a clustering of the rows of X[n, dim]: for a scored row i of
// label L the mean distance a(i) to the other rows of its cluster, the smallest mean distance b(i) to another
// cluster, that cluster nearest(i), and s(i) = (b - a) / max(a, b).  Every (scored row, row) distance is computed:
// 2 m n dim FLOPs on the MFMA chain of n2v_score_tile.h, the sums folded in registers, nothing of size m x n
// stored.  No float atomics; every result is a function of the arguments alone (DESIGN.md "Cluster quality";
// tests/cpu_silhouette/n2v_silhouette_cpu.c restates it, and the kernels are held to its bits).
//
// Rows of a label outside [0, k) belong to no cluster: never counted, never scored (asked for: a = b = s = NaN,
// nearest = -1; so is an entry of `rows` outside [0, n), which is never used as an index).
//
// The list.  The rows of label c, ascending, are segment c of a row list; every segment is padded with dead entries
// (-1) to a multiple of 16, so a tile of 16 list entries belongs to one cluster.  Built on the device: the rows are
// cut into slabs, a block counts its slab's labels (integer atomics in LDS), one block turns the counts into every
// (slab, cluster)'s place (exclusive sums over the slabs, then over the padded clusters), and a block places its
// slab's rows in ascending order (a row's rank among the equal labels of its step of 256 is counted, not raced).
//
// dot(i, j) = score_rows' chain: acc = +0; for d0 = 0, 16, .. < dim_pad, e = 0..3, q = 0..3, d = d0 + 4 q + e:
//   acc = fmaf(x_j[d] (0 past dim), x_i[d] (0 past dim), acc); row j is operand A (read in place through the list),
//   the scored row operand B (from the padded copy Q[m_pad][dim_pad]).
// d(i, j), fp32, one rounding per spelled operation:
//   Euclidean: sqrtf(fmaxf(fmaf(-2, dot, xn_i) + xn_j, 0)), xn = wave_sumsq
//   cosine:    1 - (dot * inv_norm[j]) * inv_norm[i]
// S(i, c), fp64: the lane that holds (i, g = lane >> 4) runs a chain p_g from 0 over the tiles of segment c in
//   ascending order, adding (double)d of the tile's entries 4 g + e, e = 0..3, in that order; dead entries and
//   j == i are skipped.  S = (p_0 + p_1) + (p_2 + p_3).
// a = S(i, L) / (n_L - 1) (0 when n_L == 1); b = the smallest S(i, c) / n_c over c != L with n_c > 0, found by
// `mean < b` from b = +inf over ascending c (ties: the lowest c; NaN never wins), nearest = that c (-1: none);
// s = 0 when n_L == 1, nearest == -1 or max(a, b) == 0, else (b - a) / (a > b ? a : b).  All fp64.
#include <math.h>

#include "n2v_score_tile.h"

namespace {

constexpr int kMaxClusters = 1024;     // cluster.MAX_K
constexpr int kPlaceStep = 256;        // rows per block step of the count and place kernels
constexpr int kPlaceSlabRows = 1024;   // a slab is a multiple of this: four steps
constexpr int kMaxPlaceSlabs = 2048;   // blocks of those kernels at most: the (slab, cluster) table is <= 8 MiB

// the slabs of the list build and the workspace `ws` laid out (ws null: only `bytes` means anything)
struct SilPlan {
  int64_t slab_rows, m_pad, list_len, bytes;
  int32_t n_slabs;
  float *q, *xn;
  int32_t *slab_cnt, *cnt, *list;
  int64_t *seg_off;
};

SilPlan plan_sil(int64_t n, int32_t dim, int32_t k, int64_t m, void *ws) {
  SilPlan p{};
  const int64_t share = (n + kMaxPlaceSlabs - 1) / kMaxPlaceSlabs;
  p.slab_rows = round_up(share < 1 ? 1 : share, kPlaceSlabRows);
  p.n_slabs = (int32_t)((n + p.slab_rows - 1) / p.slab_rows);
  p.m_pad = round_up(m, 64);
  p.list_len = n + 16 * (int64_t)k;  // >= the sum of the padded segments, n + 15 k at most
  Carver carve(ws);
  p.q = carve.take<float>(p.m_pad * dim_pad_of(dim) * 4);
  p.xn = carve.take<float>(n * 4);
  p.slab_cnt = carve.take<int32_t>((int64_t)p.n_slabs * k * 4);
  p.cnt = carve.take<int32_t>((int64_t)k * 4);
  p.seg_off = carve.take<int64_t>(((int64_t)k + 1) * 8);
  p.list = carve.take<int32_t>(p.list_len * 4);
  p.bytes = carve.used;
  return p;
}

// a label is a cluster number or nothing: never an index unless it is one
__device__ inline int32_t label_or_none(int32_t c, int32_t k) { return (c >= 0 && c < k) ? c : -1; }

// xn[r] = wave_sumsq(x_r); one wave per row
__global__ __launch_bounds__(256) void sil_sumsq_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                        float *__restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float s = wave_sumsq(X + r * dim, dim, lane);
  if (lane == 0) xn[r] = s;
}

// pad_rows_kernel over a gathered set of rows: q[i] = x_rows[i] padded with zeros (a zero row where rows[i] is
// outside [0, n) or i >= m); one wave per padded row
__global__ __launch_bounds__(256) void sil_gather_rows_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                              const int64_t *__restrict__ rows, int64_t m,
                                                              int64_t m_pad, float *__restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int32_t dp = dim_pad_of(dim);
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m_pad) return;
  const int64_t r = i < m ? rows[i] : -1;
  const bool live = r >= 0 && r < n;
  const float *v = X + (live ? r : 0) * dim;
  for (int d = lane; d < dp; d += 64) q[i * dp + d] = (live && d < dim) ? v[d] : 0.f;
}

// block s: slab_cnt[s][c] = the rows of slab s with label c
__global__ __launch_bounds__(kPlaceStep) void sil_count_kernel(const int32_t *__restrict__ labels, int64_t n,
                                                               int32_t k, int64_t slab_rows,
                                                               int32_t *__restrict__ slab_cnt) {
  __shared__ int32_t lcnt[kMaxClusters];
  const int tid = threadIdx.x;
  for (int c = tid; c < k; c += kPlaceStep) lcnt[c] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  for (int64_t r = lo + tid; r < hi; r += kPlaceStep) {
    const int32_t c = label_or_none(labels[r], k);
    if (c >= 0) atomicAdd(&lcnt[c], 1);
  }
  __syncthreads();
  for (int c = tid; c < k; c += kPlaceStep) slab_cnt[(int64_t)blockIdx.x * k + c] = lcnt[c];
}

// One block, thread c: slab_cnt[.][c] becomes its exclusive sum over the slabs, cnt[c] the total; then seg_off =
// the exclusive sum over the clusters of round_up(cnt, 16)
__global__ __launch_bounds__(kMaxClusters) void sil_scan_kernel(int32_t *__restrict__ slab_cnt, int32_t n_slabs,
                                                                int32_t k, int32_t *__restrict__ cnt,
                                                                int64_t *__restrict__ seg_off,
                                                                int64_t *__restrict__ counts_out) {
  __shared__ int64_t sp[kMaxClusters];
  const int i = threadIdx.x;
  int32_t total = 0;
  if (i < k) {
    for (int32_t s = 0; s < n_slabs; ++s) {
      const int32_t v = slab_cnt[(int64_t)s * k + i];
      slab_cnt[(int64_t)s * k + i] = total;
      total += v;
    }
    cnt[i] = total;
    if (counts_out) counts_out[i] = total;
  }
  int64_t p = round_up(total, 16);
  sp[i] = p;
  __syncthreads();
  for (int off = 1; off < kMaxClusters; off <<= 1) {
    const int64_t ap = i >= off ? sp[i - off] : 0;
    __syncthreads();
    p += ap;
    sp[i] = p;
    __syncthreads();
  }
  if (i == 0) seg_off[0] = 0;
  if (i < k) seg_off[i + 1] = p;
}

// block s places the rows of slab s, ascending, behind those of the slabs before it
__global__ __launch_bounds__(kPlaceStep) void sil_place_kernel(const int32_t *__restrict__ labels, int64_t n,
                                                               int32_t k, int64_t slab_rows,
                                                               const int32_t *__restrict__ slab_cnt,
                                                               const int64_t *__restrict__ seg_off,
                                                               int32_t *__restrict__ list) {
  __shared__ int32_t cursor[kMaxClusters];
  __shared__ int32_t lab[kPlaceStep];
  const int tid = threadIdx.x;
  for (int c = tid; c < k; c += kPlaceStep) cursor[c] = slab_cnt[(int64_t)blockIdx.x * k + c];
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  for (int64_t base = lo; base < hi; base += kPlaceStep) {
    const int64_t r = base + tid;
    const int32_t c = r < hi ? label_or_none(labels[r], k) : -1;
    lab[tid] = c;
    __syncthreads();
    if (c >= 0) {
      int32_t rank = 0;
      for (int t = 0; t < tid; ++t) rank += lab[t] == c;
      const int64_t at = seg_off[c] + cursor[c] + rank;
      if (at < seg_off[c + 1]) list[at] = (int32_t)r;  // (always, unless the labels change under the call)
    }
    __syncthreads();
    if (c >= 0) atomicAdd(&cursor[c], 1);
    __syncthreads();
  }
}

// Wave w of block x owns the scored rows [16 G (4 x + w), + 16 G): lane l holds, for g < G, scored row
// 16 g + (l & 15) against the list entries 4 (l >> 4) + e of the current tile.  The wave streams the whole list
// once; at the end of a segment it folds the cluster's mean into a or into the running (b, nearest).
template <int G, bool VEC>
__global__ __launch_bounds__(256) void sil_kernel(const float *__restrict__ X, const float *__restrict__ aux,
                                                  int64_t n, int32_t dim, const int32_t *__restrict__ labels,
                                                  int32_t k, int32_t metric, const int64_t *__restrict__ rows,
                                                  int64_t m, const float *__restrict__ q,
                                                  const int32_t *__restrict__ list,
                                                  const int64_t *__restrict__ seg_off,
                                                  const int32_t *__restrict__ cnt, double *__restrict__ a_out,
                                                  double *__restrict__ b_out, double *__restrict__ s_out,
                                                  int32_t *__restrict__ nearest_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * G);
  if (q0 >= m) return;
  const int32_t dp = dim_pad_of(dim);
  const bool cosine = metric == N2V_KMEANS_COSINE;

  const float *qrow[G];
  int32_t qi[G], ql[G], nearc[G];
  float qaux[G];
  double run[G], a[G], b[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t i = q0 + 16 * g + (lane & 15);  // < m_pad: a row of q
    qrow[g] = q + i * dp;
    int64_t r = -1;
    if (i < m) r = rows ? rows[i] : i;
    if (r < 0 || r >= n) r = -1;
    qi[g] = (int32_t)r;
    ql[g] = r >= 0 ? label_or_none(labels[r], k) : -1;
    qaux[g] = r >= 0 ? aux[r] : 0.f;
    run[g] = 0.0, a[g] = 0.0, b[g] = INFINITY, nearc[g] = -1;
  }

  // the end of cluster c: its mean goes into a (the row's own cluster) or competes for b
  auto fold = [&](int32_t c) {
    const int32_t nc = cnt[c];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double t = run[g];
      t = t + __shfl_xor(t, 16, 64);  // (p0 + p1), (p2 + p3)
      t = t + __shfl_xor(t, 32, 64);  // (p0 + p1) + (p2 + p3)
      run[g] = 0.0;
      if (nc <= 0) continue;
      if (c == ql[g]) {
        a[g] = nc > 1 ? t / (double)(nc - 1) : 0.0;
      } else {
        const double mean = t / (double)nc;
        if (mean < b[g]) b[g] = mean, nearc[g] = c;
      }
    }
  };

  const int64_t tiles = seg_off[k] / 16;
  int32_t c = 0;
  int64_t seg_end = seg_off[1];
  auto entry = [&](int64_t at) {  // a list entry: a row of X, or dead
    const int32_t r = list[at];
    return r < n ? r : -1;
  };
  int32_t rid = tiles > 0 ? entry(lane & 15) : -1;
  for (int64_t t = 0; t < tiles; ++t) {
    while (16 * t >= seg_end) {  // c < k - 1 here: 16 t < seg_off[k]
      fold(c);
      ++c;
      seg_end = seg_off[c + 1];
    }
    const int32_t rid_next = t + 1 < tiles ? entry(16 * (t + 1) + (lane & 15)) : -1;
    const bool live = rid >= 0;
    const float raux = live ? aux[rid] : 0.f;
    f32x4 acc[G];
    score_rows<G, VEC>(X + (live ? rid : 0) * (int64_t)dim, live, dim, qrow, lane, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int32_t j = __shfl(rid, 4 * (lane >> 4) + e, 64);
      const float jaux = __shfl(raux, 4 * (lane >> 4) + e, 64);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float dot = acc[g][e];
        float d;
        if (cosine) {
          const float scaled = dot * jaux;
          d = 1.0f - scaled * qaux[g];
        } else {
          const float t2 = __fmaf_rn(-2.0f, dot, qaux[g]);
          d = sqrtf(fmaxf(t2 + jaux, 0.0f));
        }
        // a skipped entry adds +0 to a sum that is never -0: the same bits as not adding
        const bool skip = j < 0 || j == qi[g];
        run[g] = run[g] + (skip ? 0.0 : (double)d);
      }
    }
    rid = rid_next;
  }
  for (; c < k; ++c) fold(c);

  if (lane >= 16) return;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t i = q0 + 16 * g + lane;
    if (i >= m) continue;
    double av = a[g], bv = b[g], sv;
    int32_t nv = nearc[g];
    if (ql[g] < 0) {
      av = bv = sv = NAN;
      nv = -1;
    } else if (cnt[ql[g]] == 1 || nv < 0) {
      sv = 0.0;
    } else {
      const double mx = av > bv ? av : bv;
      sv = mx == 0.0 ? 0.0 : (bv - av) / mx;
    }
    a_out[i] = av;
    b_out[i] = bv;
    s_out[i] = sv;
    nearest_out[i] = nv;
  }
}

bool sizes_ok(int64_t n, int32_t dim, int32_t k, int64_t m) {
  return matrix_ok(n, dim) && k >= 1 && k <= kMaxClusters && m >= 0 && m < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

int64_t n2v_silhouette_workspace_bytes(int64_t n, int32_t dim, int32_t k, int64_t m) {
  if (!sizes_ok(n, dim, k, m)) return -1;
  return (n == 0 || m == 0) ? 0 : plan_sil(n, dim, k, m, nullptr).bytes;
}

int n2v_silhouette(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int32_t *labels, int32_t k,
                   int32_t metric, const int64_t *rows, int64_t m, double *a_out, double *b_out, double *s_out,
                   int32_t *nearest_out, int64_t *counts_out, void *workspace, int64_t workspace_bytes,
                   void *stream) {
  if (!sizes_ok(n, dim, k, m)) return N2V_EINVAL;
  if (metric != N2V_KMEANS_EUCLIDEAN && metric != N2V_KMEANS_COSINE) return N2V_EINVAL;
  if (metric == N2V_KMEANS_COSINE && !inv_norm) return N2V_EINVAL;
  if (!rows && m != n) return N2V_EINVAL;
  if (n == 0 || m == 0) return N2V_OK;
  if (!X || !labels || !a_out || !b_out || !s_out || !nearest_out) return N2V_EINVAL;
  const SilPlan p = plan_sil(n, dim, k, m, workspace);
  if (!workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;

  // the row list
  N2V_HIP_CHECK(hipMemsetAsync(p.list, 0xff, (size_t)p.list_len * 4, st));  // every entry dead (-1)
  hipLaunchKernelGGL(sil_count_kernel, dim3((unsigned)p.n_slabs), dim3(kPlaceStep), 0, st, labels, n, k, p.slab_rows,
                     p.slab_cnt);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sil_scan_kernel, dim3(1), dim3(kMaxClusters), 0, st, p.slab_cnt, p.n_slabs, k, p.cnt, p.seg_off,
                     counts_out);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sil_place_kernel, dim3((unsigned)p.n_slabs), dim3(kPlaceStep), 0, st, labels, n, k, p.slab_rows,
                     p.slab_cnt, p.seg_off, p.list);
  N2V_HIP_CHECK(hipGetLastError());

  // operand B and the per-row factor of the distance
  if (rows)
    hipLaunchKernelGGL(sil_gather_rows_kernel, dim3((unsigned)((p.m_pad + 3) / 4)), dim3(256), 0, st, X, n, dim, rows,
                       m, p.m_pad, p.q);
  else
    launch_pad_rows(st, X, (int32_t)n, p.m_pad, dim, p.q, nullptr);
  N2V_HIP_CHECK(hipGetLastError());
  const float *aux = inv_norm;
  if (metric == N2V_KMEANS_EUCLIDEAN) {
    hipLaunchKernelGGL(sil_sumsq_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X, n, dim, p.xn);
    N2V_HIP_CHECK(hipGetLastError());
    aux = p.xn;
  }

  with_tile(m > 16 ? 64 : 16, vec_ok(dim, X), [&](auto G, auto VEC) {
    const int64_t per_block = 64 * (int64_t) decltype(G)::value;
    hipLaunchKernelGGL((sil_kernel<G, VEC>), dim3((unsigned)((m + per_block - 1) / per_block)), dim3(256), 0, st, X,
                       aux, n, dim, labels, k, metric, rows, m, p.q, p.list, p.seg_off, p.cnt, a_out, b_out, s_out,
                       nearest_out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
