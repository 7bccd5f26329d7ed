// n2v_topk_select.h -- what the two top-k scans over score_tile's scores share (n2v_knn.hip: every row; n2v_ivf.hip:
// the rows of the probed lists): the padded q_hat matrix and the kernel that fills it, the order of results, the
// per-query candidate buffers a block keeps in LDS, and the pairwise merge of the blocks' sorted lists.  Both
// files run the same code, so a (query, row) pair gets the same score, and equal candidate sets the same result,
// from either (DESIGN.md "Nearest neighbours", "Approximate nearest neighbours").
#pragma once

#include <float.h>

#include "n2v_score_tile.h"

namespace {

constexpr int kWaves = 8;              // waves per block of a top-k scan
constexpr int kStepRows = kWaves * 16; // rows scored per block step (16 per wave)
constexpr int kSentinelRow = 0x7fffffff;

// the padded query matrix q_hat [nq_pad][dim_pad] at the start of the workspace (zeros in the padding):
// a tile of G x 16 queries starting at any multiple of its 8, 16, 32 or 64 kept queries stays inside
inline int64_t nq_pad_of(int64_t nq) { return round_up(nq, 64) + 16; }

// q_hat of every query into the workspace; a query given as row r uses inv_norm[r] itself
__global__ __launch_bounds__(256) void queries_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                      int32_t dim, const float *__restrict__ queries,
                                                      const int64_t *__restrict__ query_rows, int64_t nq,
                                                      int64_t nq_pad, float *__restrict__ qhat) {
  const int lane = threadIdx.x & 63;
  const int32_t dp = dim_pad_of(dim);
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq_pad) return;
  float *out = qhat + q * dp;
  if (q >= nq) {
    for (int d = lane; d < dp; d += 64) out[d] = 0.f;
    return;
  }
  const float *v;
  float inv;
  if (query_rows) {
    const int64_t r = query_rows[q];
    v = X + r * dim;
    inv = inv_norm[r];
  } else {
    v = queries + q * dim;
    inv = inv_sqrt_or_zero(wave_sumsq(v, dim, lane));
  }
  for (int d = lane; d < dp; d += 64) out[d] = d < dim ? v[d] * inv : 0.f;
}

// q_hat, the first piece of every workspace
inline float *take_qhat(Carver &carve, int32_t dim, int64_t nq) {
  return carve.take<float>(nq_pad_of(nq) * dim_pad_of(dim) * 4);
}

inline int launch_queries(const float *X, const float *inv_norm, int32_t dim, const float *queries,
                          const int64_t *query_rows, int64_t nq, float *qhat, hipStream_t st) {
  const int64_t nq_pad = nq_pad_of(nq);
  hipLaunchKernelGGL(queries_kernel, dim3((unsigned)((nq_pad + 3) / 4)), dim3(256), 0, st, X, inv_norm, dim,
                     queries, query_rows, nq, nq_pad, qhat);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

// what every entry point that takes queries checks first
inline bool query_args_ok(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                          const int64_t *query_rows, int64_t nq) {
  if (!matrix_ok(n, dim) || nq < 0) return false;
  if ((queries == nullptr) == (query_rows == nullptr)) return false;
  if (!X || !inv_norm) return false;
  return true;
}

// the order of results: score descending, then row ascending (empty slots: -inf, kSentinelRow)
__device__ inline bool better(float sa, int ra, float sb, int rb) { return sa > sb || (sa == sb && ra < rb); }

// A block's candidate buffers: for each of its QACT queries the best candidates seen so far, CAP entries.  A
// score below the query's threshold (the k-th best kept so far) costs one compare; the others are appended.
// When a buffer could overflow in the next block step (kStepRows candidates per query at most) every buffer is
// sorted (bitonic, by `better`) and cut to k: k <= CAP - kStepRows.
template <int QACT, int CAP>
struct TopkBuffers {
  float s[QACT][CAP];
  int32_t r[QACT][CAP];
  int32_t cnt[QACT];
  float thr[QACT];
  int32_t need_sort;
};

// every buffer empty; the whole block calls it (it ends in a barrier)
template <int QACT, int CAP>
__device__ inline void topk_reset(TopkBuffers<QACT, CAP> &b, int tid) {
  for (int i = tid; i < QACT * CAP; i += kWaves * 64) {
    b.s[i / CAP][i % CAP] = -INFINITY;
    b.r[i / CAP][i % CAP] = kSentinelRow;
  }
  for (int i = tid; i < QACT; i += kWaves * 64) {
    b.cnt[i] = 0;
    b.thr[i] = -INFINITY;
  }
  if (tid == 0) b.need_sort = 0;
  __syncthreads();
}

// every buffer sorted best first and cut to k; the whole block calls it after a barrier (it ends in one)
template <int QACT, int CAP>
__device__ inline void topk_sort_cut(TopkBuffers<QACT, CAP> &b, int32_t k, int tid) {
  // bitonic sort of every buffer, best first; slots past cnt hold (-inf, sentinel)
  for (int size = 2; size <= CAP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = tid; p < QACT * (CAP / 2); p += kWaves * 64) {
        const int q = p / (CAP / 2), j = p % (CAP / 2);
        const int a = 2 * j - (j & (stride - 1)), c = a + stride;
        const bool up = (a & size) == 0;  // this half sorted best first
        const float sa = b.s[q][a], sc = b.s[q][c];
        const int ra = b.r[q][a], rc = b.r[q][c];
        if (better(sc, rc, sa, ra) == up) {
          b.s[q][a] = sc, b.s[q][c] = sa;
          b.r[q][a] = rc, b.r[q][c] = ra;
        }
      }
      __syncthreads();
    }
  }
  // keep k: the rest becomes empty again; the k-th kept score is the new threshold
  for (int i = tid; i < QACT * CAP; i += kWaves * 64) {
    const int q = i / CAP, j = i % CAP;
    if (j >= k && j < b.cnt[q]) {
      b.s[q][j] = -INFINITY;
      b.r[q][j] = kSentinelRow;
    }
  }
  __syncthreads();
  for (int q = tid; q < QACT; q += kWaves * 64) {
    if (b.cnt[q] >= k) b.thr[q] = b.s[q][k - 1];
    b.cnt[q] = b.cnt[q] < k ? b.cnt[q] : k;
  }
  if (tid == 0) b.need_sort = 0;
  __syncthreads();
}

// One wave offers the scores of its score_tile / score_rows call: acc[g][i] * inv[i] is the score of query
// 16 g + (lane & 15) of the block (the first q_live are kept) against the row whose number is row[i] and whose
// inv_norm is inv[i] (row[i] < 0: no such row).  A tie with the threshold is kept too, so the order in which
// rows arrive does not matter; NaN fails the compare.
template <int G, int QACT, int CAP>
__device__ inline void topk_offer(TopkBuffers<QACT, CAP> &b, const f32x4 (&acc)[G], const float (&inv)[4],
                                  const int32_t (&row)[4], int q_live, int lane) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int q = 16 * g + (lane & 15);
    if (q >= q_live) continue;
    const float t = b.thr[q];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = acc[g][i] * inv[i];
      if (row[i] >= 0 && s >= t) {
        const int pos = atomicAdd(&b.cnt[q], 1);
        b.s[q][pos] = s;
        b.r[q][pos] = row[i];
        if (pos >= CAP - kStepRows) b.need_sort = 1;
      }
    }
  }
}

// rank of (s, r) among the k sorted entries of a list: how many are better
__device__ inline int rank_in(const float *__restrict__ ls, const int32_t *__restrict__ lr, int k, float s, int r) {
  int a = 0, b = k;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (better(ls[m], lr[m], s, r)) a = m + 1;
    else b = m;
  }
  return a;
}

// One block per query: the n_lists sorted lists of k are merged pairwise (log2 rounds, ping-pong
// between the two halves of the workspace); an entry's place in a merged pair is its own index plus its
// rank in the other list (rows are unique, the empty slots identical).  The winner goes to out.
__global__ __launch_bounds__(256) void merge_kernel(float *__restrict__ s0, int32_t *__restrict__ r0,
                                                    float *__restrict__ s1, int32_t *__restrict__ r1,
                                                    int32_t n_lists, int32_t k, int64_t *__restrict__ out_rows,
                                                    float *__restrict__ out_scores) {
  const int64_t q = blockIdx.x;
  const int64_t span = (int64_t)n_lists * k;
  float *src_s = s0 + q * span, *dst_s = s1 + q * span;
  int32_t *src_r = r0 + q * span, *dst_r = r1 + q * span;
  for (int32_t lists = n_lists; lists > 1; lists = (lists + 1) / 2) {
    const int32_t pairs = lists / 2;
    for (int64_t e = threadIdx.x; e < (int64_t)lists * k; e += blockDim.x) {
      const int32_t l = (int32_t)(e / k), i = (int32_t)(e % k);
      const float s = src_s[e];
      const int32_t r = src_r[e];
      int32_t pos = i, dst_list = l / 2;
      if (l < 2 * pairs) {
        const int32_t other = l ^ 1;
        pos += rank_in(src_s + (int64_t)other * k, src_r + (int64_t)other * k, k, s, r);
      }
      if (pos < k) {
        dst_s[(int64_t)dst_list * k + pos] = s;
        dst_r[(int64_t)dst_list * k + pos] = r;
      }
    }
    __syncthreads();
    float *ts = src_s; src_s = dst_s; dst_s = ts;
    int32_t *tr = src_r; src_r = dst_r; dst_r = tr;
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const int32_t r = src_r[i];
    out_rows[q * k + i] = r == kSentinelRow ? -1 : r;
    out_scores[q * k + i] = r == kSentinelRow ? -INFINITY : src_s[i];
  }
}

}  // namespace
