// n2v_linkrank.hip -- filtered link-prediction ranks over trained vectors: for Q queries (u_q, v_q) of rows of
// X[n, dim], where v_q stands among ALL rows w scored against u_q once the known neighbours of u_q are removed
// (DESIGN.md "Link ranking").  The statistic behind filtered MRR, mean rank and Hits@K.
//
//   s(u, w)    = dot(q_hat_u, x_w) * inv_norm[w],  q_hat_u = x_u * inv_norm[u]: n2v_knn_scores' score of query row
//                u against row w, on the one MFMA chain of n2v_score_tile.h (the dot product: inv_norm all ones)
//   thr_q      = s(u_q, v_q)
//   F(u)       = the distinct columns of row u of the filter CSR (none without a filter)
//   greater[q] = #{ w in [0, n) : w != u_q, w != v_q, w not in F(u_q), s(u_q, w) >  thr_q }
//   equal[q]   = the same with ==
// A NaN on either side of a comparison counts in neither, so a NaN thr_q gives (0, 0).
//
// Two passes, both over score_rows' bits, so that what the second takes away is what the first put in:
//   scan  block (x = tile of 16 G queries, y = chunk of rows), as n2v_knn.hip's fused top-k scan is laid out: every
//         wave scores 16 rows against the tile, compares with the tile's thresholds and counts in registers; the
//         waves' counts meet in LDS and go to the [Q, 2] counters by integer atomic adds (their order cannot show).
//         Nothing of size Q x n is written.
//   list  a wave per query walks the members of {u, v} + F(u) sixteen at a time, rows gathered through `col`, scores
//         them with the same score_rows against the same q_hat row and takes their comparisons away again.  A
//         multi-edge is an entry equal to its predecessor (the columns of a row ascend) and is skipped, as is an entry
//         equal to u or v: those two lead the list once.  15 of the 16 MFMA columns of such a tile are idle; the lists
//         hold sum deg(u) rows, small beside Q n.
// Before both, thr_q comes from a wave per 16 queries that scores v_q against q_hat_q on the tile's diagonal.
//
// A query whose u or v lies outside [0, n) is never dereferenced: its threshold is NaN and its counts (0, 0).  A
// column outside [0, n) is skipped.
#include <math.h>

// q_hat, its kernel and the scan's block shape come from the top-k scans' header; its merge kernel is not used here
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "n2v_topk_select.h"
#pragma clang diagnostic pop

namespace {

// ua[q] = u_q, va[q] = v_q; a query with a row outside [0, n): ua 0, va -1 (dead)
__global__ __launch_bounds__(256) void rank_rows_kernel(const int64_t *__restrict__ a, const int64_t *__restrict__ b,
                                                        int64_t nq, int64_t n, int64_t *__restrict__ ua,
                                                        int64_t *__restrict__ va) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t u = a[q], v = b[q];
  const bool ok = u >= 0 && u < n && v >= 0 && v < n;
  ua[q] = ok ? u : 0;
  va[q] = ok ? v : -1;
}

// thr[q] = s(u_q, v_q) for the 16 queries of a wave: row j of the tile is v of query j, so the tile's diagonal holds
// the thresholds.  thr is written up to nq_pad (NaN past nq and for a dead query): the scan reads whole tiles.
template <bool VEC>
__global__ __launch_bounds__(256) void rank_thr_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                       int32_t dim, const float *__restrict__ qhat,
                                                       const int64_t *__restrict__ va, int64_t nq, int64_t nq_pad,
                                                       float *__restrict__ thr, float *__restrict__ thr_out) {
  const int lane = threadIdx.x & 63;
  const int64_t q0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (q0 >= nq_pad) return;
  const int j = lane & 15;
  const int64_t q = q0 + j;
  const int64_t v = q < nq ? va[q] : -1;
  const bool live = v >= 0;
  const float *qrow[1] = {qhat + q * dim_pad_of(dim)};
  f32x4 acc[1];
  score_rows<1, VEC>(X + (live ? v : 0) * (int64_t)dim, live, dim, qrow, lane, acc);
  const int i = j - 4 * (lane >> 4);  // acc[0][i] is (query j, row 4 (lane >> 4) + i)
  if (i < 0 || i > 3) return;
  const float dot = i == 0 ? acc[0][0] : i == 1 ? acc[0][1] : i == 2 ? acc[0][2] : acc[0][3];
  const float t = live ? dot * inv_norm[v] : NAN;
  thr[q] = t;
  if (thr_out && q < nq) thr_out[q] = t;
}

// the scan: counts[q] += (#{s > thr_q}, #{s == thr_q}) over the rows of the block's chunk
template <int G, bool VEC>
__global__ __launch_bounds__(kWaves * 64) void rank_scan_kernel(const float *__restrict__ X,
                                                                const float *__restrict__ inv_norm, int64_t n,
                                                                int32_t dim, const float *__restrict__ qhat,
                                                                const float *__restrict__ thr, int64_t nq,
                                                                int64_t chunk_rows,
                                                                unsigned long long *__restrict__ counts) {
  __shared__ int32_t sum[16 * G][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * (16 * G);
  const int64_t lo = (int64_t)blockIdx.y * chunk_rows;
  const int64_t hi = lo + chunk_rows < n ? lo + chunk_rows : n;
  for (int i = tid; i < 16 * G * 2; i += kWaves * 64) sum[i >> 1][i & 1] = 0;
  __syncthreads();

  float t[G];
  int32_t gt[G], eq[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    t[g] = thr[q0 + 16 * g + (lane & 15)];  // (inside thr's nq_pad entries)
    gt[g] = eq[g] = 0;
  }
  const float *qtile = qhat + q0 * dim_pad_of(dim);
  for (int64_t row0 = lo + 16 * wave; row0 < hi; row0 += kStepRows) {
    f32x4 acc[G];
    score_tile<G, VEC>(X, dim, row0, hi, qtile, lane, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = row0 + 4 * (lane >> 4) + i;
      if (r >= hi) continue;
      const float inv = inv_norm[r];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float s = acc[g][i] * inv;
        gt[g] += s > t[g];
        eq[g] += s == t[g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // the four lanes that share a query (lane & 15), then the waves
    gt[g] += __shfl_xor(gt[g], 16, 64);
    gt[g] += __shfl_xor(gt[g], 32, 64);
    eq[g] += __shfl_xor(eq[g], 16, 64);
    eq[g] += __shfl_xor(eq[g], 32, 64);
    if (lane < 16) {
      if (gt[g]) atomicAdd(&sum[16 * g + lane][0], gt[g]);
      if (eq[g]) atomicAdd(&sum[16 * g + lane][1], eq[g]);
    }
  }
  __syncthreads();
  for (int i = tid; i < 16 * G * 2; i += kWaves * 64) {
    const int64_t q = q0 + (i >> 1);
    const int32_t c = sum[i >> 1][i & 1];
    if (q < nq && c) atomicAdd(&counts[2 * q + (i & 1)], (unsigned long long)c);
  }
}

// the list pass: a wave per query takes the comparisons of {u, v} + F(u) out of counts[q] again.  It runs after the
// scan on the same stream and owns its query's two counters, so the update is a plain one.
template <bool VEC>
__global__ __launch_bounds__(256) void rank_list_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                        int64_t n, int32_t dim, const float *__restrict__ qhat,
                                                        const float *__restrict__ thr,
                                                        const int64_t *__restrict__ ua, const int64_t *__restrict__ va,
                                                        int64_t nq, const int64_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col,
                                                        int64_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const int64_t v = va[q];
  const float t = thr[q];
  if (v < 0 || t != t) return;  // dead, or nothing was counted
  const int64_t u = ua[q];
  const int64_t beg = rowptr ? rowptr[u] : 0;
  const int64_t len = 2 + (rowptr ? rowptr[u + 1] - beg : 0);  // u, v, then the row's columns
  const float *qrow[1] = {qhat + q * dim_pad_of(dim)};
  int32_t gt = 0, eq = 0;
  for (int64_t e0 = 0; e0 < len; e0 += 16) {
    const int64_t e = e0 + (lane & 15);
    int64_t r = -1;
    if (e == 0) {
      r = u;
    } else if (e == 1) {
      r = v != u ? v : -1;
    } else if (e < len) {
      const int64_t c = col[beg + e - 2];
      const bool repeat = e > 2 && col[beg + e - 3] == (int32_t)c;
      if (!repeat && c != u && c != v && c >= 0 && c < n) r = c;
    }
    const bool live = r >= 0;
    f32x4 acc[1];
    score_rows<1, VEC>(X + (live ? r : 0) * (int64_t)dim, live, dim, qrow, lane, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // every column of the tile is this query: the lanes of column 0 count rows 4 (lane >> 4) + i
      const int64_t ri = __shfl(r, 4 * (lane >> 4) + i, 64);
      if ((lane & 15) == 0 && ri >= 0) {
        const float s = acc[0][i] * inv_norm[ri];
        gt += s > t;
        eq += s == t;
      }
    }
  }
  for (int off = 16; off < 64; off <<= 1) {
    gt += __shfl_xor(gt, off, 64);
    eq += __shfl_xor(eq, off, 64);
  }
  if (lane == 0) {
    counts[2 * q] -= gt;
    counts[2 * q + 1] -= eq;
  }
}

// the launch shape of n2v_link_rank and its workspace laid out (ws null: only `bytes` means anything)
struct RankPlan {
  int32_t n_chunks;
  int64_t chunk_rows, bytes;
  float *qhat, *thr;
  int64_t *ua, *va;
};

RankPlan plan_rank(int64_t n, int32_t dim, int64_t nq, void *ws) {
  RankPlan p{};
  const int64_t qt = nq <= 16 ? 16 : 64;  // with_tile's G
  const int64_t tiles = (nq + qt - 1) / qt;
  // about 2048 blocks in all (no LDS to speak of: 4 blocks of 8 waves per CU, 256 CUs, twice over), never a chunk of
  // less than 16 steps
  int64_t chunks = (2048 + tiles - 1) / tiles;
  const int64_t most = (n + 16 * kStepRows - 1) / (16 * kStepRows);
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  p.chunk_rows = round_up((n + chunks - 1) / chunks, kStepRows);
  p.n_chunks = (int32_t)((n + p.chunk_rows - 1) / p.chunk_rows);
  if (p.n_chunks < 1) p.n_chunks = 1;
  Carver carve(ws);
  p.qhat = take_qhat(carve, dim, nq);
  p.thr = carve.take<float>(nq_pad_of(nq) * 4);
  p.ua = carve.take<int64_t>(nq * 8);
  p.va = carve.take<int64_t>(nq * 8);
  p.bytes = carve.used;
  return p;
}

bool rank_sizes_ok(int64_t n, int32_t dim, int64_t nq) {
  return matrix_ok(n, dim) && nq >= 0 && nq < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

int64_t n2v_link_rank_workspace_bytes(int64_t n, int32_t dim, int64_t n_queries) {
  if (!rank_sizes_ok(n, dim, n_queries)) return -1;
  if (n == 0 || n_queries == 0) return 0;
  return plan_rank(n, dim, n_queries, nullptr).bytes;
}

int n2v_link_rank_plan(int64_t n, int32_t dim, int64_t n_queries, int64_t *chunk_rows_out, int32_t *n_chunks_out) {
  if (!rank_sizes_ok(n, dim, n_queries) || !chunk_rows_out || !n_chunks_out) return N2V_EINVAL;
  const RankPlan p = plan_rank(n, dim, n_queries, nullptr);
  *chunk_rows_out = p.chunk_rows;
  *n_chunks_out = p.n_chunks;
  return N2V_OK;
}

int n2v_link_rank(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *a, const int64_t *b,
                  int64_t n_queries, const int64_t *rowptr, const int32_t *col, float *thr_out, int64_t *counts_out,
                  void *workspace, int64_t workspace_bytes, void *stream) {
  if (!rank_sizes_ok(n, dim, n_queries)) return N2V_EINVAL;
  if ((rowptr == nullptr) != (col == nullptr)) return N2V_EINVAL;
  if (n == 0 || n_queries == 0) return N2V_OK;
  const RankPlan p = plan_rank(n, dim, n_queries, workspace);
  if (!X || !inv_norm || !a || !b || !counts_out || !workspace_ok(workspace, workspace_bytes, p.bytes))
    return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nq = n_queries, nq_pad = nq_pad_of(nq);
  N2V_HIP_CHECK(hipMemsetAsync(counts_out, 0, (size_t)nq * 16, st));
  hipLaunchKernelGGL(rank_rows_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, a, b, nq, n, p.ua, p.va);
  N2V_HIP_CHECK(hipGetLastError());
  const int rc = launch_queries(X, inv_norm, dim, nullptr, p.ua, nq, p.qhat, st);
  if (rc != N2V_OK) return rc;
  const bool vec = vec_ok(dim, X);
  with_bool(vec, [&](auto VEC) {
    hipLaunchKernelGGL(rank_thr_kernel<VEC>, dim3((unsigned)((nq_pad / 16 + 3) / 4)), dim3(256), 0, st, X, inv_norm,
                       dim, p.qhat, p.va, nq, nq_pad, p.thr, thr_out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  with_tile((int32_t)(nq <= 16 ? nq : 17), vec, [&](auto G, auto VEC) {
    const dim3 grid((unsigned)((nq + 16 * G - 1) / (16 * G)), (unsigned)p.n_chunks);
    hipLaunchKernelGGL((rank_scan_kernel<G, VEC>), grid, dim3(kWaves * 64), 0, st, X, inv_norm, n, dim, p.qhat, p.thr,
                       nq, p.chunk_rows, reinterpret_cast<unsigned long long *>(counts_out));
  });
  N2V_HIP_CHECK(hipGetLastError());
  with_bool(vec, [&](auto VEC) {
    hipLaunchKernelGGL(rank_list_kernel<VEC>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, X, inv_norm, n, dim,
                       p.qhat, p.thr, p.ua, p.va, nq, rowptr, col, counts_out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
