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
#include "n2v_topk_select.h"

namespace {

constexpr int kMaxK = 1024;  // the fused path's k limit

__global__ __launch_bounds__(256) void inv_norm_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                       float *__restrict__ inv_norm) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += waves) {
    const float s = wave_sumsq(X + r * dim, dim, lane);
    if (lane == 0) inv_norm[r] = inv_sqrt_or_zero(s);
  }
}

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
// candidates of its chunk in an LDS buffer of CAP entries (TopkBuffers, n2v_topk_select.h).  At the end the sorted
// top k of the chunk go to part[q][chunk][0..k).  G groups of 16 queries are scored, the first QACT kept.
template <int G, int QACT, int CAP, bool VEC>
__global__ __launch_bounds__(kWaves * 64) void topk_chunk_kernel(
    const float *__restrict__ X, const float *__restrict__ inv_norm, int64_t n, int32_t dim,
    const float *__restrict__ qhat, int64_t nq, int32_t k, int64_t chunk_rows, int32_t n_chunks,
    float *__restrict__ part_s, int32_t *__restrict__ part_r) {
  __shared__ TopkBuffers<QACT, CAP> buf;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QACT;
  const int32_t chunk = blockIdx.y;
  const int64_t lo = (int64_t)chunk * chunk_rows;
  const int64_t hi = lo + chunk_rows < n ? lo + chunk_rows : n;
  const int q_live = nq - q0 < QACT ? (int)(nq - q0) : QACT;
  topk_reset(buf, tid);

  const float *qtile = qhat + q0 * dim_pad_of(dim);
  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t row0 = base + 16 * wave;
    if (row0 < hi) {
      f32x4 acc[G];
      score_tile<G, VEC>(X, dim, row0, hi, qtile, lane, acc);
      float inv[4];
      int32_t row[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = row0 + 4 * (lane >> 4) + i;
        row[i] = r < hi ? (int32_t)r : -1;
        inv[i] = r < hi ? inv_norm[r] : 0.f;
      }
      topk_offer<G>(buf, acc, inv, row, q_live, lane);
    }
    __syncthreads();
    if (buf.need_sort) topk_sort_cut(buf, k, tid);
  }
  topk_sort_cut(buf, k, tid);
  for (int i = tid; i < QACT * k; i += kWaves * 64) {
    const int q = i / k, j = i % k;
    if (q0 + q >= nq) continue;
    const int64_t o = ((q0 + q) * n_chunks + chunk) * (int64_t)k + j;
    part_s[o] = buf.s[q][j];
    part_r[o] = buf.r[q][j];
  }
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
  if (!query_args_ok(X, inv_norm, n, dim, queries, query_rows, n_queries)) return N2V_EINVAL;
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
  if (!query_args_ok(X, inv_norm, n, dim, queries, query_rows, n_queries)) return N2V_EINVAL;
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
