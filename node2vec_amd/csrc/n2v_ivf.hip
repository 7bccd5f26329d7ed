// n2v_ivf.hip -- approximate nearest neighbours over an inverted-file (IVF-flat) index of X[n, dim]: the rows are
// cut into nlist lists (spherical k-means cells, node2vec_amd/ann.py) and a query scans only the lists it probes
// (DESIGN.md "Approximate nearest neighbours").
//
// "Approximate" is which lists are probed and nothing else.  A (query, row) score is n2v_knn.hip's, bit for bit:
// the same q_hat (queries_kernel), the same MFMA chain (score_rows, the core of score_tile, which does not depend on
// the tile a row or a query lands in) and the same `* inv_norm[row]`; the selection is n2v_knn.hip's too
// (n2v_topk_select.h: score descending, then ORIGINAL row number ascending, NaN never kept).  So the result is the
// exact top k of the probed lists' rows, and with every list probed it is n2v_knn_topk's.
//
// The index is list_off [nlist + 1] and row_ids (the rows of X in list order); X is read in place through row_ids,
// whole rows at a time.  One launch sequence, no device-to-host read:
//   1. q_hat of every query; the partial lists emptied; the lists' lengths checked against max_list_rows
//   2. the (query, probe) pairs grouped by list (n2v_ivf_group.h, shared with n2v_ivfpq.hip): count (integer
//      atomics), scan, fill -- the order inside a group is whatever the atomics give, and no result depends on it
//   3. block (x = tile of qt pairs of one list, y = chunk of chunk_rows rows of that list): 16 rows x 16 G pairs per
//      wave step, the candidates in LDS, the sorted k best to the slot (pair, chunk); the grid is sized from an
//      upper bound on the tiles and the blocks past the real count exit
//   4. per query the nprobe x chunks slots merged pairwise (merge_kernel)
// There are no float atomics.
#include "n2v_ivf_group.h"

namespace {

constexpr int kMaxK = 128;       // k <= CAP - kStepRows
constexpr int kCap = 256;        // candidates per pair in LDS
constexpr int kChunkSteps = 16;  // block steps per chunk of a list, about

// the launch shape and the workspace `ws` laid out (ws null: only the sizes mean anything): q_hat, the grouping
// tables, the pair list, then the two halves (scores, rows) of the slots that the merge ping-pongs
struct IvfPlan {
  bool ok;
  int qt;              // pairs per tile: 64 (G 4) or 16 (G 1)
  int32_t chunks;      // chunks per list (grid y): ceil(max_list_rows / chunk_rows)
  int64_t chunk_rows;  // a multiple of kStepRows
  int64_t pairs, tiles_max, bytes;
  float *qhat, *s0, *s1;
  IvfGroups g;
  int32_t *r0, *r1;
};

bool sizes_ok(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t nq, int32_t nprobe, int32_t k) {
  if (!matrix_ok(n, dim) || nq < 0 || nq >= ((int64_t)1 << 20)) return false;
  if (nlist < 1 || nlist > kMaxLists || nprobe < 1 || nprobe > nlist || k < 1 || k > kMaxK) return false;
  if (max_list_rows < 1 || (n > 0 && max_list_rows > n)) return false;
  return true;
}

IvfPlan plan_ivf(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t nq, int32_t nprobe, int32_t k,
                 void *ws) {
  IvfPlan p{};
  p.pairs = nq * nprobe;
  // groups of 16 pairs or fewer on average: the narrow tile (a quarter of the MFMA work per row read)
  p.qt = p.pairs <= 16 * (int64_t)nlist ? 16 : 64;
  // a list is cut into even chunks of about kChunkSteps block steps.  The cut depends on max_list_rows alone, so
  // the workspace grows with every other size (callers split a batch of queries until it fits)
  const int64_t chunks = (max_list_rows + kChunkSteps * kStepRows - 1) / (kChunkSteps * kStepRows);
  p.chunk_rows = round_up((max_list_rows + chunks - 1) / chunks, kStepRows);
  p.chunks = (int32_t)((max_list_rows + p.chunk_rows - 1) / p.chunk_rows);
  // every non-empty group ends in one tile that may not be full
  p.tiles_max = p.pairs / p.qt + (p.pairs < nlist ? p.pairs : nlist);
  p.ok = p.tiles_max * p.chunks <= kMaxBlocks;
  const int64_t part = p.pairs * p.chunks * k * 4;
  Carver carve(ws);
  p.qhat = take_qhat(carve, dim, nq);
  p.g = take_groups(carve, nlist, p.pairs);
  p.s0 = carve.take<float>(part);
  p.r0 = carve.take<int32_t>(part);
  p.s1 = carve.take<float>(part);
  p.r1 = carve.take<int32_t>(part);
  p.bytes = carve.used;
  return p;
}

// Block (x = tile, y = chunk): the tile's list is found in tile_off, its pairs in pair_list; the chunk's rows are
// row_ids[list_off[l] + lo .. + hi).  Pair p is query p / nprobe; its sorted k best of the chunk go to slot
// (p, chunk).  A slot no block writes (an unused probe, a list that ends before the chunk) stays empty.
template <int G, int QACT, bool VEC>
__global__ __launch_bounds__(kWaves * 64) void ivf_topk_kernel(
    const float *__restrict__ X, const float *__restrict__ inv_norm, int64_t n, int32_t dim,
    const int64_t *__restrict__ list_off, const int32_t *__restrict__ row_ids, int32_t nlist, int64_t max_list_rows,
    const float *__restrict__ qhat, int64_t zero_query, int32_t nprobe, int32_t k, int64_t chunk_rows, int32_t chunks,
    const int32_t *__restrict__ pair_off, const int32_t *__restrict__ tile_off,
    const int32_t *__restrict__ pair_list, float *__restrict__ part_s, int32_t *__restrict__ part_r,
    uint32_t *__restrict__ status) {
  __shared__ TopkBuffers<QACT, kCap> buf;
  __shared__ int32_t pair_of[QACT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t tile = blockIdx.x, chunk = blockIdx.y;
  if (tile >= tile_off[nlist]) return;
  const int32_t l = list_of_tile(tile_off, nlist, tile);
  const int64_t begin = list_off[l];
  int64_t len = list_off[l + 1] - begin;
  if (len > max_list_rows) len = max_list_rows;
  if (begin < 0) len = 0;
  const int64_t lo = (int64_t)chunk * chunk_rows;
  if (lo >= len) return;
  const int64_t hi = lo + chunk_rows < len ? lo + chunk_rows : len;
  const int32_t first = pair_off[l] + (tile - tile_off[l]) * QACT;
  const int q_live = pair_off[l + 1] - first < QACT ? pair_off[l + 1] - first : QACT;
  for (int i = tid; i < QACT; i += kWaves * 64) pair_of[i] = i < q_live ? pair_list[first + i] : -1;
  topk_reset(buf, tid);

  const int32_t dp = dim_pad_of(dim);
  const float *qrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int32_t p = pair_of[16 * g + (lane & 15)];
    qrow[g] = qhat + (p >= 0 ? (int64_t)(p / nprobe) : zero_query) * dp;
  }
  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t at0 = base + 16 * wave;
    if (at0 < hi) {
      const int64_t at = at0 + (lane & 15);
      int32_t rid = at < hi ? row_ids[begin + at] : -1;
      if (at < hi && (rid < 0 || rid >= n)) {  // not a row of X: never read
        atomicOr(status, N2V_ST_RANGE);
        rid = -1;
      }
      const bool live = rid >= 0;
      const float rinv = live ? inv_norm[rid] : 0.f;
      f32x4 acc[G];
      score_rows<G, VEC>(X + (live ? rid : 0) * (int64_t)dim, live, dim, qrow, lane, acc);
      float inv[4];
      int32_t row[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        row[i] = __shfl(rid, 4 * (lane >> 4) + i, 64);
        inv[i] = __shfl(rinv, 4 * (lane >> 4) + i, 64);
      }
      topk_offer<G>(buf, acc, inv, row, q_live, lane);
    }
    __syncthreads();
    if (buf.need_sort) topk_sort_cut(buf, k, tid);
  }
  topk_sort_cut(buf, k, tid);
  for (int i = tid; i < q_live * k; i += kWaves * 64) {
    const int q = i / k, j = i % k;
    const int64_t o = ((int64_t)pair_of[q] * chunks + chunk) * k + j;
    part_s[o] = buf.s[q][j];
    part_r[o] = buf.r[q][j];
  }
}

template <int G, int QACT>
void launch_scan(const IvfPlan &p, const float *X, const float *inv_norm, int64_t n, int32_t dim,
                 const int64_t *list_off, const int32_t *row_ids, int32_t nlist, int64_t max_list_rows, int64_t nq,
                 int32_t nprobe, int32_t k, uint32_t *status, hipStream_t st) {
  const dim3 grid((unsigned)p.tiles_max, (unsigned)p.chunks);
  with_bool(vec_ok(dim, X), [&](auto VEC) {
    hipLaunchKernelGGL((ivf_topk_kernel<G, QACT, VEC>), grid, dim3(kWaves * 64), 0, st, X, inv_norm, n, dim, list_off,
                       row_ids, nlist, max_list_rows, p.qhat, nq_pad_of(nq) - 1, nprobe, k, p.chunk_rows, p.chunks,
                       p.g.pair_off, p.g.tile_off, p.g.pair_list, p.s0, p.r0, status);
  });
}

}  // namespace

extern "C" {

int64_t n2v_ivf_workspace_bytes(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t n_queries,
                                int32_t nprobe, int32_t k) {
  if (!sizes_ok(n, dim, nlist, max_list_rows, n_queries, nprobe, k)) return -1;
  if (n == 0 || n_queries == 0) return 0;
  const IvfPlan p = plan_ivf(n, dim, nlist, max_list_rows, n_queries, nprobe, k, nullptr);
  return p.ok ? p.bytes : -1;
}

int n2v_ivf_plan(int64_t n, int32_t dim, int32_t nlist, int64_t max_list_rows, int64_t n_queries, int32_t nprobe,
                 int32_t k, int64_t *plan3) {
  if (!plan3 || !sizes_ok(n, dim, nlist, max_list_rows, n_queries, nprobe, k)) return N2V_EINVAL;
  const IvfPlan p = plan_ivf(n, dim, nlist, max_list_rows, n_queries, nprobe, k, nullptr);
  if (!p.ok) return N2V_EINVAL;
  plan3[0] = p.qt;
  plan3[1] = p.chunk_rows;
  plan3[2] = p.chunks;
  return N2V_OK;
}

int n2v_ivf_topk(const float *X, const float *inv_norm, int64_t n, int32_t dim, const int64_t *list_off,
                 const int32_t *row_ids, int32_t nlist, int64_t max_list_rows, const float *queries,
                 const int64_t *query_rows, int64_t n_queries, const int32_t *probes, int32_t nprobe, int32_t k,
                 int64_t *out_rows, float *out_scores, uint32_t *status, void *workspace, int64_t workspace_bytes,
                 void *stream) {
  if (!query_args_ok(X, inv_norm, n, dim, queries, query_rows, n_queries)) return N2V_EINVAL;
  if (!sizes_ok(n, dim, nlist, max_list_rows, n_queries, nprobe, k)) return N2V_EINVAL;
  if (!list_off || !row_ids || !probes || !status) return N2V_EINVAL;
  if (n == 0 || n_queries == 0) return N2V_OK;
  const IvfPlan p = plan_ivf(n, dim, nlist, max_list_rows, n_queries, nprobe, k, workspace);
  if (!p.ok || !out_rows || !out_scores || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_queries(X, inv_norm, dim, queries, query_rows, n_queries, p.qhat, st);
  if (rc != N2V_OK) return rc;
  const int rg = launch_groups(p.g, list_off, nlist, max_list_rows, probes, p.pairs, nprobe, p.qt,
                              p.pairs * p.chunks * k, p.s0, p.r0, status, st);
  if (rg != N2V_OK) return rg;
  if (p.qt == 64)
    launch_scan<4, 64>(p, X, inv_norm, n, dim, list_off, row_ids, nlist, max_list_rows, n_queries, nprobe, k, status, st);
  else
    launch_scan<1, 16>(p, X, inv_norm, n, dim, list_off, row_ids, nlist, max_list_rows, n_queries, nprobe, k, status, st);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n_queries), dim3(256), 0, st, p.s0, p.r0, p.s1, p.r1,
                     nprobe * p.chunks, k, out_rows, out_scores);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
