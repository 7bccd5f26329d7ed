// n2v_kmeans.hip -- k-means (Lloyd) over a row-major fp32 matrix X[n, dim]: for every row the nearest of k
// centroids (Euclidean, or cosine = spherical k-means), and the new centroids from the rows of every cluster.
// One launch reads X once per iteration: a block scores 64 rows against every centroid with the MFMA chain
// of n2v_score_tile.h, writes their labels and distances, and adds those same rows (still in L1 / L2) to the
// sums of its slab; a finishing kernel folds the slabs.  No float atomics; every result is a function of
// (X, centroids) alone (DESIGN.md "Clustering"; tests/cpu_kmeans/n2v_kmeans_cpu.c restates it).
//
// Assignment.  dot(c, r) = score_tile's chain: acc = +0; for d0 = 0, 16, .. < dim_pad, j = 0..3, k = 0..3,
// d = d0 + 4 k + j: acc = fmaf(x_r[d] (0 past dim), c[d] (0 past dim), acc).
//   Euclidean: t(c, r) = fmaf(-2, dot(c, r), cn[c]), cn[c] = wave_sumsq(c);  dist = fmaxf(t_min + xn[r], 0)
//   cosine:    t(c, r) = -dot(c, r) (unit centroids);                        dist = 1 - dot_best * inv_norm[r]
//   label = the lowest c with the smallest t (NaN and +inf never win; none left: label -1, dist NaN).
// Update.  Rows are cut into slabs of slab_rows(n, dim, k) (a multiple of 64).  P[s][c][d] is an fp32 chain
// from +0 over the slab's rows of label c in ascending row order, P = P + v with v = x_r[d] (Euclidean) or the
// rounded product x_r[d] * inv_norm[r] (cosine).  sum[c][d] is an fp64 chain from 0 over s ascending of
// (double)P[s][c][d]; counts are integers.  New centroid: (float)(sum / (double)count), or for cosine
// f = (float)sum, f * inv_sqrt_or_zero(wave_sumsq(f)); an empty cluster, or a cosine one whose factor is 0,
// keeps the previous centroid's bits.
#include <math.h>

#include "n2v_score_tile.h"

namespace {

constexpr int kStepRows = kSlabStepRows;
constexpr int kModeAssign = 1, kModeUpdate = 2;

// the slabs, and the workspace `ws` laid out (ws null: only `bytes` means anything): the centroids padded to
// [k_pad][dim_pad], their sums of squares, the slabs' partial sums
struct Plan {
  SlabPlan slabs;
  int64_t k_pad, bytes;
  float *cpad, *cn, *part;
};

Plan plan_of(int64_t n, int32_t dim, int32_t k, void *ws) {
  Plan p{};
  const int64_t per_slab = (int64_t)k * dim * 4;
  p.slabs = slab_plan(n, per_slab);
  p.k_pad = round_up(k, 64);
  Carver carve(ws);
  p.cpad = carve.take<float>(p.k_pad * dim_pad_of(dim) * 4);
  p.cn = carve.take<float>(p.k_pad * 4);
  p.part = carve.take<float>(p.slabs.n_slabs * per_slab);
  p.bytes = carve.used;
  return p;
}

// Block s owns slab s: rows [s slab_rows, ..).  mode: kModeAssign scores and writes labels / dist (and, with
// stats, counts the labels that change and the rows left unassigned), kModeUpdate adds the rows to the slab's
// partial sums (labels as just written, or as given); both: the fused Lloyd step.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void lloyd_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                    int64_t n, int32_t dim, const float *__restrict__ cpad,
                                                    const float *__restrict__ cn, int32_t k, int32_t metric,
                                                    int32_t mode, int32_t *__restrict__ labels,
                                                    float *__restrict__ dist, float *__restrict__ part,
                                                    unsigned long long *__restrict__ counts,
                                                    unsigned long long *__restrict__ stats, int64_t slab_rows) {
  __shared__ int32_t lab[kStepRows];
  __shared__ float sinv[kStepRows];
  __shared__ int32_t lcnt[1024];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t dp = dim_pad_of(dim);
  const bool assign = mode & kModeAssign, update = mode & kModeUpdate, cosine = metric == N2V_KMEANS_COSINE;
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  float *mine = part + (int64_t)blockIdx.x * k * dim;
  if (update) {
    // a thread zeroes exactly the elements it later adds to
    for (int c = 0; c < k; ++c)
      for (int d = tid; d < dim; d += 256) mine[(int64_t)c * dim + d] = 0.f;
    for (int c = tid; c < k; c += 256) lcnt[c] = 0;
  }
  unsigned changed = 0, unassigned = 0;
  __syncthreads();

  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int cnt = hi - base < kStepRows ? (int)(hi - base) : kStepRows;
    const int64_t row0 = base + 16 * wave;
    if (assign && row0 < hi) {
      float best[4];
      int32_t bc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) best[i] = INFINITY, bc[i] = -1;
      for (int32_t c0 = 0; c0 < k; c0 += 16 * G) {
        f32x4 acc[G];
        score_tile<G, VEC>(X, dim, row0, hi, cpad + (int64_t)c0 * dp, lane, acc);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int32_t c = c0 + 16 * g + (lane & 15);
          if (c >= k) continue;
          const float cnc = cn[c];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float t = cosine ? -acc[g][i] : __fmaf_rn(-2.0f, acc[g][i], cnc);
            if (t < best[i]) best[i] = t, bc[i] = c;
          }
        }
      }
      // the best of the 16 lanes that hold one row: smaller t, then lower c (a lane's own c ascend)
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float to = __shfl_xor(best[i], off, 64);
          const int32_t co = __shfl_xor(bc[i], off, 64);
          if (to < best[i] || (to == best[i] && co < bc[i])) best[i] = to, bc[i] = co;
        }
      }
      float xn[4] = {0.f, 0.f, 0.f, 0.f};
      if (dist && !cosine) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int64_t r = row0 + j;
          const float s = wave_sumsq(X + (r < hi ? r : row0) * (int64_t)dim, dim, lane);
          if (lane == 16 * (j >> 2)) xn[j & 3] = s;
        }
      }
      if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t r = row0 + 4 * (lane >> 4) + i;
          if (r >= hi) continue;
          const int32_t c = bc[i];
          if (dist) dist[r] = c < 0 ? NAN : cosine ? 1.f - (-best[i]) * inv_norm[r] : fmaxf(best[i] + xn[i], 0.f);
          if (stats) {
            changed += labels[r] != c;
            unassigned += c < 0;
          }
          labels[r] = c;
          lab[r - base] = c;
        }
      }
    }
    if (!assign && tid < cnt) {
      const int32_t c = labels[base + tid];
      lab[tid] = (c >= 0 && c < k) ? c : -1;  // never an index unless it is one
    }
    if (update && cosine && tid < cnt) sinv[tid] = inv_norm[base + tid];
    __syncthreads();
    if (update) {
      if (tid < cnt && lab[tid] >= 0) atomicAdd(&lcnt[lab[tid]], 1);
      // a thread owns its dimensions; the rows of the step in ascending order.  The running sum of a run of
      // equal labels stays in a register: the same chain of additions as adding to memory row by row.
      for (int d = tid; d < dim; d += 256) {
        int32_t cur = -1;
        float a = 0.f;
        for (int i = 0; i < cnt; ++i) {
          const int32_t c = lab[i];
          if (c < 0) continue;
          float v = X[(base + i) * (int64_t)dim + d];
          if (cosine) v = v * sinv[i];
          if (c != cur) {
            if (cur >= 0) mine[(int64_t)cur * dim + d] = a;
            a = mine[(int64_t)c * dim + d];
            cur = c;
          }
          a = a + v;
        }
        if (cur >= 0) mine[(int64_t)cur * dim + d] = a;
      }
    }
    __syncthreads();
  }
  if (update)
    for (int c = tid; c < k; c += 256)
      if (lcnt[c]) atomicAdd(&counts[c], (unsigned long long)lcnt[c]);
  if (stats) {
    if (changed) atomicAdd(&stats[0], (unsigned long long)changed);
    if (unassigned) atomicAdd(&stats[1], (unsigned long long)unassigned);
  }
}

// One wave per cluster: the slab partials folded in ascending slab order in fp64, then the new centroid
__global__ __launch_bounds__(64) void finish_kernel(const float *__restrict__ part, int32_t n_slabs, int32_t k,
                                                    int32_t dim, int32_t metric,
                                                    const unsigned long long *__restrict__ counts,
                                                    const float *__restrict__ prev, float *__restrict__ out) {
  __shared__ float f[1024];
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x;
  const unsigned long long cnt = counts[c];
  const int64_t stride = (int64_t)k * dim;
  for (int d = lane; d < dim; d += 64) {
    double s = 0.0;
    const float *p = part + c * dim + d;
    for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + (double)p[sl * stride];
    if (metric == N2V_KMEANS_COSINE) f[d] = (float)s;
    else out[c * dim + d] = cnt ? (float)(s / (double)cnt) : prev[c * dim + d];
  }
  if (metric != N2V_KMEANS_COSINE) return;
  __syncthreads();
  const float inv = inv_sqrt_or_zero(wave_sumsq(f, dim, lane));
  const bool keep = cnt == 0 || !(inv > 0.f);
  for (int d = lane; d < dim; d += 64) out[c * dim + d] = keep ? prev[c * dim + d] : f[d] * inv;
}

bool sizes_ok(int64_t n, int32_t dim, int32_t k, int32_t metric) {
  return matrix_ok(n, dim) && k >= 1 && k <= 1024 && (metric == N2V_KMEANS_EUCLIDEAN || metric == N2V_KMEANS_COSINE);
}

// prep (when assigning), the slab launch, finish (when updating); the workspace is checked here, everything else
// was validated by the caller
int run(int32_t mode, const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *centroids_in,
        int32_t k, int32_t metric, int32_t *labels, float *dist, const float *prev, float *centroids_out,
        int64_t *counts_out, int64_t *stats_out, void *ws, int64_t ws_bytes, hipStream_t st) {
  const Plan p = plan_of(n, dim, k, ws);
  if (!workspace_ok(ws, ws_bytes, p.bytes)) return N2V_EINVAL;
  if (mode & kModeAssign) {
    launch_pad_rows(st, centroids_in, k, p.k_pad, dim, p.cpad, p.cn);
    N2V_HIP_CHECK(hipGetLastError());
  }
  if (mode & kModeUpdate) N2V_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)k * 8, st));
  if (stats_out) N2V_HIP_CHECK(hipMemsetAsync(stats_out, 0, 16, st));
  with_tile(k, vec_ok(dim, X), [&](auto G, auto VEC) {
    hipLaunchKernelGGL((lloyd_kernel<G, VEC>), dim3((unsigned)p.slabs.n_slabs), dim3(256), 0, st, X, inv_norm, n, dim,
                       p.cpad, p.cn, k, metric, mode, labels, dist, p.part, (unsigned long long *)counts_out,
                       (unsigned long long *)stats_out, p.slabs.slab_rows);
  });
  N2V_HIP_CHECK(hipGetLastError());
  if (mode & kModeUpdate) {
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)k), dim3(64), 0, st, p.part, p.slabs.n_slabs, k, dim, metric,
                       (const unsigned long long *)counts_out, prev, centroids_out);
    N2V_HIP_CHECK(hipGetLastError());
  }
  return N2V_OK;
}

}  // namespace

extern "C" {

int64_t n2v_kmeans_slab_rows(int64_t n, int32_t dim, int32_t k) {
  if (!sizes_ok(n, dim, k, N2V_KMEANS_EUCLIDEAN)) return -1;
  return plan_of(n, dim, k, nullptr).slabs.slab_rows;
}

int64_t n2v_kmeans_workspace_bytes(int64_t n, int32_t dim, int32_t k) {
  if (!sizes_ok(n, dim, k, N2V_KMEANS_EUCLIDEAN)) return -1;
  return n == 0 ? 0 : plan_of(n, dim, k, nullptr).bytes;
}

int n2v_kmeans_assign(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *centroids,
                      int32_t k, int32_t metric, int32_t *labels_out, float *dist_out, void *workspace,
                      int64_t workspace_bytes, void *stream) {
  if (!sizes_ok(n, dim, k, metric)) return N2V_EINVAL;
  if (metric == N2V_KMEANS_COSINE && !inv_norm) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!X || !centroids || !labels_out) return N2V_EINVAL;
  return run(kModeAssign, X, inv_norm, n, dim, centroids, k, metric, labels_out, dist_out, nullptr, nullptr,
             nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int n2v_kmeans_update(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int32_t *labels,
                      int32_t k, int32_t metric, const float *prev_centroids, float *centroids_out,
                      int64_t *counts_out, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!sizes_ok(n, dim, k, metric)) return N2V_EINVAL;
  if (metric == N2V_KMEANS_COSINE && !inv_norm) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!X || !labels || !prev_centroids || !centroids_out || !counts_out || centroids_out == prev_centroids)
    return N2V_EINVAL;
  return run(kModeUpdate, X, inv_norm, n, dim, nullptr, k, metric, const_cast<int32_t *>(labels), nullptr,
             prev_centroids, centroids_out, counts_out, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int n2v_kmeans_step(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *centroids_in,
                    int32_t k, int32_t metric, int32_t *labels_inout, float *dist_out, float *centroids_out,
                    int64_t *counts_out, int64_t *stats_out, void *workspace, int64_t workspace_bytes,
                    void *stream) {
  if (!sizes_ok(n, dim, k, metric)) return N2V_EINVAL;
  if (metric == N2V_KMEANS_COSINE && !inv_norm) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!X || !centroids_in || !labels_inout || !centroids_out || !counts_out || !stats_out ||
      centroids_out == centroids_in)
    return N2V_EINVAL;
  return run(kModeAssign | kModeUpdate, X, inv_norm, n, dim, centroids_in, k, metric, labels_inout, dist_out,
             centroids_in, centroids_out, counts_out, stats_out, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
