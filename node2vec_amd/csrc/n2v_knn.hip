// n2v_knn.hip -- exact fp32 cosine nearest neighbours over a row-major matrix X[n, dim]
// (gensim 3.8 KeyedVectors.init_sims / most_similar, which the reference reaches through the
// Word2Vec model of embedding.py:126).  Brute force: every score is computed, none is approximated.
//
// Score of a query q against row r (DESIGN.md "Nearest neighbours"):
//   q_hat = q * (1 / sqrtf(sum q^2))                  (or x_r' * inv_norm[r'] for a query given as a row)
//   score = dot(q_hat, x_r) * inv_norm[r],  inv_norm[r] = 1 / sqrtf(sum x_r^2), 0 for a zero row
// Both sums run in one fixed order (wave_sumsq: lane l sums d = l, l + 64, ... by fmaf, then a fixed
// butterfly), and the dot product is ONE v_mfma_f32_16x16x4_f32 chain over d in a fixed order
// (score_tile: a k-ordered fmaf chain, element by element).  Nothing depends on the number of queries,
// the tile a row or a query lands in, or the entry point: the fused top-k kernel and the full-score
// kernel call the same score_tile, so n2v_knn_topk's scores equal n2v_knn_scores' bit for bit.
#include <float.h>

#include "n2v_score_tile.h"

namespace {

constexpr int kWaves = 8;              // waves per block of the top-k kernel
constexpr int kStepRows = kWaves * 16; // rows scored per block step (16 per wave)
constexpr int kMaxK = 1024;            // the fused path's k limit
constexpr int kSentinelRow = 0x7fffffff;

// the padded query matrix q_hat [nq_pad][dim_pad] at the start of the workspace (zeros in the padding):
// a tile of G x 16 queries starting at any multiple of its 8, 16, 32 or 64 kept queries stays inside
inline int64_t nq_pad_of(int64_t nq) { return round_up(nq, 64) + 16; }

__global__ __launch_bounds__(256) void inv_norm_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                       float *__restrict__ inv_norm) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += waves) {
    const float s = wave_sumsq(X + r * dim, dim, lane);
    if (lane == 0) inv_norm[r] = inv_sqrt_or_zero(s);
  }
}

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

// the order of results: score descending, then row ascending (empty slots: -inf, kSentinelRow)
__device__ inline bool better(float sa, int ra, float sb, int rb) { return sa > sb || (sa == sb && ra < rb); }

// Every score of 16 queries against 16 rows per wave (grid: x = row tiles of 64, y = query tiles of 16)
template <bool VEC>
__global__ __launch_bounds__(256) void scores_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                     int64_t n, int32_t dim, const float *__restrict__ qhat,
                                                     int64_t nq, float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (row0 >= n) return;
  const int64_t q0 = (int64_t)blockIdx.y * 16;
  f32x4 acc[1];
  score_tile<1, VEC>(X, dim, row0, n, qhat + q0 * dim_pad_of(dim), lane, acc);
  const int64_t q = q0 + (lane & 15);
  if (q >= nq) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + 4 * (lane >> 4) + i;
    if (r < n) out[q * n + r] = acc[0][i] * inv_norm[r];
  }
}

// Fused scan: block (x = query tile, y = chunk of rows) keeps, for each of its QACT queries, the best
// candidates of its chunk in an LDS buffer of CAP entries.  A score below the query's threshold (the
// k-th best kept so far) costs one compare; the others are appended.  When a buffer could overflow in
// the next step every buffer is sorted (bitonic, by `better`) and cut to k.  At the end the sorted
// top k of the chunk go to part[q][chunk][0..k).  G groups of 16 queries are scored, the first QACT kept.
template <int G, int QACT, int CAP, bool VEC>
__global__ __launch_bounds__(kWaves * 64) void topk_chunk_kernel(
    const float *__restrict__ X, const float *__restrict__ inv_norm, int64_t n, int32_t dim,
    const float *__restrict__ qhat, int64_t nq, int32_t k, int64_t chunk_rows, int32_t n_chunks,
    float *__restrict__ part_s, int32_t *__restrict__ part_r) {
  __shared__ float buf_s[QACT][CAP];
  __shared__ int32_t buf_r[QACT][CAP];
  __shared__ int32_t cnt[QACT];
  __shared__ float thr[QACT];
  __shared__ int32_t need_sort;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QACT;
  const int32_t chunk = blockIdx.y;
  const int64_t lo = (int64_t)chunk * chunk_rows;
  const int64_t hi = lo + chunk_rows < n ? lo + chunk_rows : n;
  for (int i = tid; i < QACT * CAP; i += kWaves * 64) {
    buf_s[i / CAP][i % CAP] = -INFINITY;
    buf_r[i / CAP][i % CAP] = kSentinelRow;
  }
  for (int i = tid; i < QACT; i += kWaves * 64) {
    cnt[i] = 0;
    thr[i] = -INFINITY;
  }
  if (tid == 0) need_sort = 0;
  __syncthreads();

  auto sort_all = [&]() {
    // bitonic sort of every buffer, best first; slots past cnt hold (-inf, sentinel)
    for (int size = 2; size <= CAP; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int p = tid; p < QACT * (CAP / 2); p += kWaves * 64) {
          const int q = p / (CAP / 2), j = p % (CAP / 2);
          const int a = 2 * j - (j & (stride - 1)), b = a + stride;
          const bool up = (a & size) == 0;  // this half sorted best first
          const float sa = buf_s[q][a], sb = buf_s[q][b];
          const int ra = buf_r[q][a], rb = buf_r[q][b];
          if (better(sb, rb, sa, ra) == up) {
            buf_s[q][a] = sb, buf_s[q][b] = sa;
            buf_r[q][a] = rb, buf_r[q][b] = ra;
          }
        }
        __syncthreads();
      }
    }
    // keep k: the rest becomes empty again; the k-th kept score is the new threshold
    for (int i = tid; i < QACT * CAP; i += kWaves * 64) {
      const int q = i / CAP, j = i % CAP;
      if (j >= k && j < cnt[q]) {
        buf_s[q][j] = -INFINITY;
        buf_r[q][j] = kSentinelRow;
      }
    }
    __syncthreads();
    for (int q = tid; q < QACT; q += kWaves * 64) {
      if (cnt[q] >= k) thr[q] = buf_s[q][k - 1];
      cnt[q] = cnt[q] < k ? cnt[q] : k;
    }
    if (tid == 0) need_sort = 0;
    __syncthreads();
  };

  const float *qtile = qhat + q0 * dim_pad_of(dim);
  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t row0 = base + 16 * wave;
    if (row0 < hi) {
      f32x4 acc[G];
      score_tile<G, VEC>(X, dim, row0, hi, qtile, lane, acc);
      float inv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = row0 + 4 * (lane >> 4) + i;
        inv[i] = r < hi ? inv_norm[r] : 0.f;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int q = 16 * g + (lane & 15);
        if (q >= QACT || q0 + q >= nq) continue;
        const float t = thr[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t r = row0 + 4 * (lane >> 4) + i;
          const float s = acc[g][i] * inv[i];
          // a tie with the threshold cannot win (its row is above every kept row: rows arrive in ascending
          // order within a chunk), so s >= t keeps nothing s > t would not need; NaN fails both
          if (r < hi && s >= t) {
            const int pos = atomicAdd(&cnt[q], 1);
            buf_s[q][pos] = s;
            buf_r[q][pos] = (int32_t)r;
            if (pos >= CAP - kStepRows) need_sort = 1;
          }
        }
      }
    }
    __syncthreads();
    if (need_sort) sort_all();
  }
  sort_all();
  for (int i = tid; i < QACT * k; i += kWaves * 64) {
    const int q = i / k, j = i % k;
    if (q0 + q >= nq) continue;
    const int64_t o = ((q0 + q) * n_chunks + chunk) * (int64_t)k + j;
    part_s[o] = buf_s[q][j];
    part_r[o] = buf_r[q][j];
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

// One block per query: the n_chunks sorted lists of k are merged pairwise (log2 rounds, ping-pong
// between the two halves of the workspace); an entry's place in a merged pair is its own index plus its
// rank in the other list (rows are unique, the empty slots identical).  The winner goes to out.
__global__ __launch_bounds__(256) void merge_kernel(float *__restrict__ s0, int32_t *__restrict__ r0,
                                                    float *__restrict__ s1, int32_t *__restrict__ r1,
                                                    int32_t n_chunks, int32_t k, int64_t *__restrict__ out_rows,
                                                    float *__restrict__ out_scores) {
  const int64_t q = blockIdx.x;
  const int64_t span = (int64_t)n_chunks * k;
  float *src_s = s0 + q * span, *dst_s = s1 + q * span;
  int32_t *src_r = r0 + q * span, *dst_r = r1 + q * span;
  for (int32_t lists = n_chunks; lists > 1; lists = (lists + 1) / 2) {
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

// q_hat, the first piece of every workspace
float *take_qhat(Carver &carve, int32_t dim, int64_t nq) {
  return carve.take<float>(nq_pad_of(nq) * dim_pad_of(dim) * 4);
}

// the launch shape of n2v_knn_topk: query tile, LDS buffer, chunks; and the workspace `ws` laid out (ws null: only
// `bytes` means anything): q_hat, then the two halves (scores, rows) of the chunk lists that the merge ping-pongs
struct TopkPlan {
  int variant;  // 0: G 4 / CAP 256, 1: G 2 / CAP 512, 2: G 1 / CAP 1024, 3: G 1 (8 queries kept) / CAP 2048
  int qt;       // queries per block
  int32_t n_chunks;
  int64_t chunk_rows, bytes;
  float *qhat, *s0, *s1;
  int32_t *r0, *r1;
};

TopkPlan plan_topk(int64_t n, int32_t dim, int64_t nq, int32_t k, void *ws) {
  TopkPlan p{};
  if (k <= 128 && nq > 32) p.variant = 0, p.qt = 64;
  else if (k <= 384 && nq > 16) p.variant = 1, p.qt = 32;
  else if (k <= 896) p.variant = 2, p.qt = 16;
  else p.variant = 3, p.qt = 8;
  const int64_t tiles = (nq + p.qt - 1) / p.qt;
  // about 512 blocks in all (one block of 128 KiB LDS per CU, 256 CUs), never a chunk of less than
  // 16 steps
  int64_t chunks = (512 + tiles - 1) / tiles;
  const int64_t most = (n + 16 * kStepRows - 1) / (16 * kStepRows);
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  p.chunk_rows = round_up((n + chunks - 1) / chunks, kStepRows);
  p.n_chunks = (int32_t)((n + p.chunk_rows - 1) / p.chunk_rows);
  if (p.n_chunks < 1) p.n_chunks = 1;
  const int64_t part = nq * (int64_t)p.n_chunks * k * 4;
  Carver carve(ws);
  p.qhat = take_qhat(carve, dim, nq);
  p.s0 = carve.take<float>(part);
  p.r0 = carve.take<int32_t>(part);
  p.s1 = carve.take<float>(part);
  p.r1 = carve.take<int32_t>(part);
  p.bytes = carve.used;
  return p;
}

bool args_ok(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
             const int64_t *query_rows, int64_t nq) {
  if (!matrix_ok(n, dim) || nq < 0) return false;
  if ((queries == nullptr) == (query_rows == nullptr)) return false;
  if (!X || !inv_norm) return false;
  return true;
}

int launch_queries(const float *X, const float *inv_norm, int32_t dim, const float *queries,
                   const int64_t *query_rows, int64_t nq, float *qhat, hipStream_t st) {
  const int64_t nq_pad = nq_pad_of(nq);
  hipLaunchKernelGGL(queries_kernel, dim3((unsigned)((nq_pad + 3) / 4)), dim3(256), 0, st, X, inv_norm, dim,
                     queries, query_rows, nq, nq_pad, qhat);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

template <int G, int QACT, int CAP>
void launch_topk(const TopkPlan &p, const float *X, const float *inv_norm, int64_t n, int32_t dim, int64_t nq,
                 int32_t k, hipStream_t st) {
  const dim3 grid((unsigned)((nq + QACT - 1) / QACT), (unsigned)p.n_chunks);
  with_bool(vec_ok(dim, X), [&](auto VEC) {
    hipLaunchKernelGGL((topk_chunk_kernel<G, QACT, CAP, VEC>), grid, dim3(kWaves * 64), 0, st, X, inv_norm, n, dim,
                       p.qhat, nq, k, p.chunk_rows, p.n_chunks, p.s0, p.r0);
  });
}

}  // namespace

extern "C" {

int n2v_knn_inv_norms(const float *X, int64_t n, int32_t dim, float *inv_norm, void *stream) {
  if (!matrix_ok(n, dim)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!X || !inv_norm) return N2V_EINVAL;
  const int64_t blocks = (n + 3) / 4 < 65536 ? (n + 3) / 4 : 65536;
  hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X, n, dim,
                     inv_norm);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int64_t n2v_knn_workspace_bytes(int64_t n, int32_t dim, int64_t n_queries, int32_t k) {
  if (!matrix_ok(n, dim) || n_queries < 0 || k < 0 || k > kMaxK) return -1;
  if (n == 0 || n_queries == 0) return 0;
  if (k > 0) return plan_topk(n, dim, n_queries, k, nullptr).bytes;
  Carver carve(nullptr);  // n2v_knn_scores: q_hat alone
  take_qhat(carve, dim, n_queries);
  return carve.used;
}

int n2v_knn_topk(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                 const int64_t *query_rows, int64_t n_queries, int32_t k, int64_t *out_rows, float *out_scores,
                 void *workspace, int64_t workspace_bytes, void *stream) {
  if (!args_ok(X, inv_norm, n, dim, queries, query_rows, n_queries)) return N2V_EINVAL;
  if (k < 1 || k > kMaxK) return N2V_EINVAL;
  if (n == 0 || n_queries == 0) return N2V_OK;
  const TopkPlan p = plan_topk(n, dim, n_queries, k, workspace);
  if (!out_rows || !out_scores || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_queries(X, inv_norm, dim, queries, query_rows, n_queries, p.qhat, st);
  if (rc != N2V_OK) return rc;
  switch (p.variant) {
    case 0: launch_topk<4, 64, 256>(p, X, inv_norm, n, dim, n_queries, k, st); break;
    case 1: launch_topk<2, 32, 512>(p, X, inv_norm, n, dim, n_queries, k, st); break;
    case 2: launch_topk<1, 16, 1024>(p, X, inv_norm, n, dim, n_queries, k, st); break;
    default: launch_topk<1, 8, 2048>(p, X, inv_norm, n, dim, n_queries, k, st); break;
  }
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n_queries), dim3(256), 0, st, p.s0, p.r0, p.s1, p.r1, p.n_chunks,
                     k, out_rows, out_scores);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_knn_scores(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                   const int64_t *query_rows, int64_t n_queries, float *out_scores, void *workspace,
                   int64_t workspace_bytes, void *stream) {
  if (!args_ok(X, inv_norm, n, dim, queries, query_rows, n_queries)) return N2V_EINVAL;
  if (n == 0 || n_queries == 0) return N2V_OK;
  Carver carve(workspace);
  float *qhat = take_qhat(carve, dim, n_queries);
  if (!out_scores || !workspace_ok(workspace, workspace_bytes, carve.used)) return N2V_EINVAL;
  if ((n_queries + 15) / 16 > 65535) return N2V_EINVAL;  // grid y; callers split larger batches
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_queries(X, inv_norm, dim, queries, query_rows, n_queries, qhat, st);
  if (rc != N2V_OK) return rc;
  const dim3 grid((unsigned)((n + 63) / 64), (unsigned)((n_queries + 15) / 16));
  with_bool(vec_ok(dim, X), [&](auto VEC) {
    hipLaunchKernelGGL(scores_kernel<VEC>, grid, dim3(256), 0, st, X, inv_norm, n, dim, qhat, n_queries, out_scores);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
