// n2v_ivfpq.hip -- approximate nearest neighbours over product-quantised codes of an inverted-file index (IVF-PQ,
// node2vec_amd/ann.py build_pq / search_pq; DESIGN.md "Product-quantised codes").
//
// A listed row x of list l is stored as m bytes: code_j names one of 256 codewords w_j[c] (dsub = ceil(dim / m)
// floats each) of sub-space j, chosen nearest to the residual x_hat - c_hat_l.  Inner products are linear, so
//   q_hat . x_hat  ~  q_hat . c_hat_l  +  sum_j q_hat_j . w_j[code_j]
// and the second term is m look-ups in a table that depends on the query alone.  X is not read (only a query given
// as a row of X is).
//
// The arithmetic, in ONE fixed order that no tile, chunk, group or launch size enters:
//   lut[q][j][c] = (..((+0 + q_hat[j dsub] * w_j[c][0]) + q_hat[j dsub + 1] * w_j[c][1]) + ..), t ascending over the
//                  dims j dsub + t < dim; every product and every sum rounded once (__fmul_rn, __fadd_rn);
//                  q_hat is n2v_knn.hip's (queries_kernel)
//   score(q, position p of probe ordinal o) = (..((coarse[q][o] + lut[q][0][code_0]) + lut[q][1][code_1]) + ..),
//                  j ascending, every sum rounded once
// The selection is n2v_knn.hip's (n2v_topk_select.h): score descending, then ORIGINAL row number ascending, NaN
// never kept, the tail (-1, -inf).
//
// One launch sequence, no device-to-host read, no float atomics:
//   1. q_hat of every query, then every query's table into the workspace (lut_kernel)
//   2. the (query, probe) pairs grouped by list (n2v_ivf_group.h)
//   3. block (x = tile of T pairs of one list, y = chunk of chunk_rows positions of that list): the tile's T tables
//      copied to LDS; per block step 128 positions, lane = (position, pair group of 4): the four lanes of a position
//      load its code row with ONE aligned vector load (the same address, so the codes are read once per tile) and
//      each sums m LDS look-ups for its T / 4 pairs; candidates to the LDS buffers, the sorted k best to slot
//      (pair, chunk)
//   4. per query the nprobe x chunks slots merged pairwise (merge_kernel)
#include "n2v_ivf_group.h"

namespace {

constexpr int kPqMaxM = 64;        // sub-quantisers at most
constexpr int kPqCodewords = 256;  // 8-bit codes
constexpr int kPqMaxK = 128;       // k <= CAP - kStepRows
constexpr int kPqCap = 256;        // candidates per pair in LDS
constexpr int kPqChunkSteps = 32;  // block steps per chunk of a list, about
constexpr int kLutQueries = 8;     // queries per block of lut_kernel

// bytes from one code row to the next: m rounded up to 4, 8, 16, 32 or 64, so that a row is one aligned load of
// 4, 8 or 16 bytes, or 2 or 4 of 16
__host__ __device__ inline int32_t code_stride_of(int32_t m) { return m <= 4 ? 4 : m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64; }

// pairs per tile: as many tables (m KiB each) as fit in LDS beside the candidate buffers (2 KiB a pair)
inline int tile_pairs_of(int32_t m) { return m <= 7 ? 16 : m <= 16 ? 8 : m <= 32 ? 4 : 2; }

// what a scan block keeps in LDS: 112 KiB of tables for T = 16 (m <= 7), 128 KiB otherwise
template <int T>
struct ScanLds {
  static constexpr int kTables = T == 16 ? 16 * 7 : 128;
  alignas(16) float lut[kTables * kPqCodewords];
  TopkBuffers<T, kPqCap> buf;
  int32_t pair_of[T];
  float coarse[T];
};

inline int64_t scan_lds_bytes(int T) {
  return T == 16 ? sizeof(ScanLds<16>) : T == 8 ? sizeof(ScanLds<8>) : T == 4 ? sizeof(ScanLds<4>) : sizeof(ScanLds<2>);
}
static_assert(sizeof(ScanLds<16>) <= 160 * 1024 && sizeof(ScanLds<8>) <= 160 * 1024 &&
              sizeof(ScanLds<4>) <= 160 * 1024 && sizeof(ScanLds<2>) <= 160 * 1024, "a scan block's LDS");

struct PqPlan {
  bool ok;
  int qt;              // pairs per tile
  int32_t chunks;      // chunks per list (grid y): ceil(max_list_rows / chunk_rows)
  int64_t chunk_rows;  // a multiple of kStepRows
  int64_t pairs, tiles_max, bytes;
  float *qhat, *lut, *s0, *s1;
  IvfGroups g;
  int32_t *r0, *r1;
};

bool pq_shape_ok(int32_t dim, int32_t m) { return matrix_ok(0, dim) && m >= 1 && m <= kPqMaxM && m <= dim; }

bool pq_sizes_ok(int64_t n, int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows, int64_t nq, int32_t nprobe,
                 int32_t k) {
  if (!matrix_ok(n, dim) || !pq_shape_ok(dim, m) || nq < 0 || nq >= ((int64_t)1 << 20)) return false;
  if (nlist < 1 || nlist > kMaxLists || nprobe < 1 || nprobe > nlist || k < 1 || k > kPqMaxK) return false;
  if (max_list_rows < 1 || (n > 0 && max_list_rows > n)) return false;
  return true;
}

PqPlan plan_pq(int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows, int64_t nq, int32_t nprobe, int32_t k,
               void *ws) {
  PqPlan p{};
  p.pairs = nq * nprobe;
  p.qt = tile_pairs_of(m);
  // a list is cut into even chunks of about kPqChunkSteps block steps; the cut depends on max_list_rows alone
  const int64_t chunks = (max_list_rows + kPqChunkSteps * kStepRows - 1) / (kPqChunkSteps * kStepRows);
  p.chunk_rows = round_up((max_list_rows + chunks - 1) / chunks, kStepRows);
  p.chunks = (int32_t)((max_list_rows + p.chunk_rows - 1) / p.chunk_rows);
  p.tiles_max = p.pairs / p.qt + (p.pairs < nlist ? p.pairs : nlist);
  p.ok = p.tiles_max * p.chunks <= kMaxBlocks;
  const int64_t part = p.pairs * p.chunks * k * 4;
  Carver carve(ws);
  p.qhat = take_qhat(carve, dim, nq);
  p.lut = carve.take<float>(nq * m * kPqCodewords * 4);
  p.g = take_groups(carve, nlist, p.pairs);
  p.s0 = carve.take<float>(part);
  p.r0 = carve.take<int32_t>(part);
  p.s1 = carve.take<float>(part);
  p.r1 = carve.take<int32_t>(part);
  p.bytes = carve.used;
  return p;
}

// Block (x = kLutQueries queries, y = sub-space j), thread c: lut[q][j][c] for the block's queries, t ascending.
// q_hat has zero rows up to nq_pad_of(nq), so a block's 8 queries are always readable.
__global__ __launch_bounds__(kPqCodewords) void lut_kernel(const float *__restrict__ qhat, int64_t nq, int32_t dim,
                                                           const float *__restrict__ codebooks, int32_t m,
                                                           float *__restrict__ lut) {
  const int c = threadIdx.x, j = blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * kLutQueries;
  const int32_t dsub = (dim + m - 1) / m, dp = dim_pad_of(dim);
  const float *w = codebooks + ((int64_t)j * kPqCodewords + c) * dsub;
  const float *qh = qhat + q0 * dp + (int64_t)j * dsub;
  float acc[kLutQueries];
#pragma unroll
  for (int i = 0; i < kLutQueries; ++i) acc[i] = 0.f;
  for (int32_t t = 0; t < dsub && j * dsub + t < dim; ++t) {
    const float wt = w[t];
#pragma unroll
    for (int i = 0; i < kLutQueries; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(qh[(int64_t)i * dp + t], wt));
  }
#pragma unroll
  for (int i = 0; i < kLutQueries; ++i)
    if (q0 + i < nq) lut[((q0 + i) * m + j) * kPqCodewords + c] = acc[i];
}

// the code row at `p`, W 4-byte words, by the widest aligned loads
template <int W>
__device__ inline void load_code_row(const uint8_t *__restrict__ p, uint32_t (&w)[W]) {
  if constexpr (W == 1) {
    w[0] = *reinterpret_cast<const uint32_t *>(p);
  } else if constexpr (W == 2) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    w[0] = v.x, w[1] = v.y;
  } else {
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
      w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
    }
  }
}

// Block (x = tile, y = chunk): the tile's list is found in tile_off, its pairs in pair_list; the chunk's positions
// are list_off[l] + lo .. + hi.  Pair p is query p / nprobe and coarse[p] its first term; its sorted k best of the
// chunk go to slot (p, chunk).  A slot no block writes stays empty.  W = code_stride / 4.
template <int T, int W>
__global__ __launch_bounds__(kWaves * 64) void ivfpq_scan_kernel(
    const uint8_t *__restrict__ codes, int32_t m, int64_t n, const int64_t *__restrict__ list_off,
    const int32_t *__restrict__ row_ids, int32_t nlist, int64_t max_list_rows, const float *__restrict__ lut,
    const float *__restrict__ coarse, int32_t nprobe, int32_t k, int64_t chunk_rows, int32_t chunks,
    const int32_t *__restrict__ pair_off, const int32_t *__restrict__ tile_off,
    const int32_t *__restrict__ pair_list, float *__restrict__ part_s, int32_t *__restrict__ part_r,
    uint32_t *__restrict__ status) {
  __shared__ ScanLds<T> sm;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t tile = blockIdx.x, chunk = blockIdx.y;
  if (tile >= tile_off[nlist]) return;
  const int32_t l = list_of_tile(tile_off, nlist, tile);
  const int64_t begin = list_off[l], total = list_off[nlist];
  int64_t len = list_off[l + 1] - begin;
  if (len > max_list_rows) len = max_list_rows;
  if (begin < 0) len = 0;
  if (begin + len > total) {  // offsets that descend somewhere: nothing past the last one is read
    len = total > begin ? total - begin : 0;
    if (tid == 0) atomicOr(status, N2V_ST_RANGE);
  }
  const int64_t lo = (int64_t)chunk * chunk_rows;
  if (lo >= len) return;
  const int64_t hi = lo + chunk_rows < len ? lo + chunk_rows : len;
  const int32_t first = pair_off[l] + (tile - tile_off[l]) * T;
  const int q_live = pair_off[l + 1] - first < T ? pair_off[l + 1] - first : T;
  for (int i = tid; i < T; i += kWaves * 64) {
    const int32_t p = i < q_live ? pair_list[first + i] : -1;
    sm.pair_of[i] = p;
    sm.coarse[i] = p >= 0 ? coarse[p] : 0.f;
  }
  topk_reset(sm.buf, tid);

  // the tile's tables: pair i's m x 256 floats at sm.lut[i m 256 ..], 16 bytes a thread
  const int per_pair = m * (kPqCodewords / 4);
  for (int i = tid; i < q_live * per_pair; i += kWaves * 64) {
    const int t = i / per_pair, at = i % per_pair;
    const int64_t q = sm.pair_of[t] / nprobe;
    reinterpret_cast<f32x4 *>(sm.lut)[i] = reinterpret_cast<const f32x4 *>(lut + q * m * kPqCodewords)[at];
  }
  __syncthreads();

  const int group = lane & 3, sub = 16 * wave + (lane >> 2);
  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t at = base + sub;
    int32_t rid = at < hi ? row_ids[begin + at] : -1;
    if (at < hi && (rid < 0 || rid >= n)) {  // not a row of the matrix: never a candidate
      atomicOr(status, N2V_ST_RANGE);
      rid = -1;
    }
    if (rid >= 0) {
      uint32_t w[W];
      load_code_row<W>(codes + (begin + at) * (int64_t)(4 * W), w);
#pragma unroll
      for (int t0 = 0; t0 < T; t0 += 4) {
        const int t = t0 + group;
        if (t >= q_live) continue;
        const float *table = sm.lut + t * m * kPqCodewords;
        float s = sm.coarse[t];
#pragma unroll
        for (int j = 0; j < 4 * W; ++j)
          if (j < m) s = __fadd_rn(s, table[j * kPqCodewords + ((w[j >> 2] >> (8 * (j & 3))) & 255u)]);
        if (s >= sm.buf.thr[t]) {  // a tie with the threshold is kept too; NaN fails the compare
          const int pos = atomicAdd(&sm.buf.cnt[t], 1);
          sm.buf.s[t][pos] = s;
          sm.buf.r[t][pos] = rid;
          if (pos >= kPqCap - kStepRows) sm.buf.need_sort = 1;
        }
      }
    }
    __syncthreads();
    if (sm.buf.need_sort) topk_sort_cut(sm.buf, k, tid);
  }
  topk_sort_cut(sm.buf, k, tid);
  for (int i = tid; i < q_live * k; i += kWaves * 64) {
    const int q = i / k, j = i % k;
    const int64_t o = ((int64_t)sm.pair_of[q] * chunks + chunk) * k + j;
    part_s[o] = sm.buf.s[q][j];
    part_r[o] = sm.buf.r[q][j];
  }
}

template <int T, int W>
void launch_pq_scan(const PqPlan &p, const uint8_t *codes, int32_t m, int64_t n, const int64_t *list_off,
                    const int32_t *row_ids, int32_t nlist, int64_t max_list_rows, const float *coarse, int32_t nprobe,
                    int32_t k, uint32_t *status, hipStream_t st) {
  const dim3 grid((unsigned)p.tiles_max, (unsigned)p.chunks);
  hipLaunchKernelGGL((ivfpq_scan_kernel<T, W>), grid, dim3(kWaves * 64), 0, st, codes, m, n, list_off, row_ids, nlist,
                     max_list_rows, p.lut, coarse, nprobe, k, p.chunk_rows, p.chunks, p.g.pair_off, p.g.tile_off,
                     p.g.pair_list, p.s0, p.r0, status);
}

// a query given as a row needs X and inv_norm; one given as a vector does not (the index holds no X)
bool pq_query_args_ok(const float *X, const float *inv_norm, const float *queries, const int64_t *query_rows) {
  if ((queries == nullptr) == (query_rows == nullptr)) return false;
  return queries || (X && inv_norm);
}

int launch_lut(const float *qhat, int64_t nq, int32_t dim, const float *codebooks, int32_t m, float *lut,
               hipStream_t st) {
  const dim3 grid((unsigned)((nq + kLutQueries - 1) / kLutQueries), (unsigned)m);
  hipLaunchKernelGGL(lut_kernel, grid, dim3(kPqCodewords), 0, st, qhat, nq, dim, codebooks, m, lut);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // namespace

extern "C" {

int64_t n2v_ivfpq_workspace_bytes(int64_t n, int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows,
                                  int64_t n_queries, int32_t nprobe, int32_t k) {
  if (k == 0) {  // n2v_ivfpq_lut: q_hat alone
    if (!pq_shape_ok(dim, m) || n_queries < 0 || n_queries >= ((int64_t)1 << 20)) return -1;
    if (n_queries == 0) return 0;
    Carver carve(nullptr);
    take_qhat(carve, dim, n_queries);
    return carve.used;
  }
  if (!pq_sizes_ok(n, dim, m, nlist, max_list_rows, n_queries, nprobe, k)) return -1;
  if (n == 0 || n_queries == 0) return 0;
  const PqPlan p = plan_pq(dim, m, nlist, max_list_rows, n_queries, nprobe, k, nullptr);
  return p.ok ? p.bytes : -1;
}

int n2v_ivfpq_plan(int64_t n, int32_t dim, int32_t m, int32_t nlist, int64_t max_list_rows, int64_t n_queries,
                   int32_t nprobe, int32_t k, int64_t *plan5) {
  if (!plan5 || !pq_sizes_ok(n, dim, m, nlist, max_list_rows, n_queries, nprobe, k)) return N2V_EINVAL;
  const PqPlan p = plan_pq(dim, m, nlist, max_list_rows, n_queries, nprobe, k, nullptr);
  if (!p.ok) return N2V_EINVAL;
  plan5[0] = p.qt;
  plan5[1] = p.chunk_rows;
  plan5[2] = p.chunks;
  plan5[3] = scan_lds_bytes(p.qt);
  plan5[4] = code_stride_of(m);
  return N2V_OK;
}

int n2v_ivfpq_lut(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *queries,
                  const int64_t *query_rows, int64_t n_queries, const float *codebooks, int32_t m, float *lut_out,
                  void *workspace, int64_t workspace_bytes, void *stream) {
  if (!matrix_ok(n, dim) || !pq_shape_ok(dim, m) || n_queries < 0 || n_queries >= ((int64_t)1 << 20))
    return N2V_EINVAL;
  if (!pq_query_args_ok(X, inv_norm, queries, query_rows)) return N2V_EINVAL;
  if (n_queries == 0) return N2V_OK;
  Carver carve(workspace);
  float *qhat = take_qhat(carve, dim, n_queries);
  if (!codebooks || !lut_out || !workspace_ok(workspace, workspace_bytes, carve.used)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_queries(X, inv_norm, dim, queries, query_rows, n_queries, qhat, st);
  if (rc != N2V_OK) return rc;
  return launch_lut(qhat, n_queries, dim, codebooks, m, lut_out, st);
}

int n2v_ivfpq_topk(const uint8_t *codes, const float *codebooks, int32_t m, const float *X, const float *inv_norm,
                   int64_t n, int32_t dim, const int64_t *list_off, const int32_t *row_ids, int32_t nlist,
                   int64_t max_list_rows, const float *queries, const int64_t *query_rows, int64_t n_queries,
                   const int32_t *probes, const float *coarse, int32_t nprobe, int32_t k, int64_t *out_rows,
                   float *out_scores, uint32_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!pq_sizes_ok(n, dim, m, nlist, max_list_rows, n_queries, nprobe, k)) return N2V_EINVAL;
  if (!pq_query_args_ok(X, inv_norm, queries, query_rows)) return N2V_EINVAL;
  if (!codes || !codebooks || !list_off || !row_ids || !probes || !coarse || !status) return N2V_EINVAL;
  if (((uintptr_t)codes & 15) != 0) return N2V_EINVAL;
  if (n == 0 || n_queries == 0) return N2V_OK;
  const PqPlan p = plan_pq(dim, m, nlist, max_list_rows, n_queries, nprobe, k, workspace);
  if (!p.ok || !out_rows || !out_scores || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_queries(X, inv_norm, dim, queries, query_rows, n_queries, p.qhat, st);
  if (rc != N2V_OK) return rc;
  rc = launch_lut(p.qhat, n_queries, dim, codebooks, m, p.lut, st);
  if (rc != N2V_OK) return rc;
  rc = launch_groups(p.g, list_off, nlist, max_list_rows, probes, p.pairs, nprobe, p.qt, p.pairs * p.chunks * k, p.s0,
                     p.r0, status, st);
  if (rc != N2V_OK) return rc;
#define N2V_PQ_SCAN(T, W) \
  launch_pq_scan<T, W>(p, codes, m, n, list_off, row_ids, nlist, max_list_rows, coarse, nprobe, k, status, st)
  switch (code_stride_of(m)) {
    case 4: N2V_PQ_SCAN(16, 1); break;
    case 8: if (p.qt == 16) N2V_PQ_SCAN(16, 2); else N2V_PQ_SCAN(8, 2); break;
    case 16: N2V_PQ_SCAN(8, 4); break;
    case 32: N2V_PQ_SCAN(4, 8); break;
    default: N2V_PQ_SCAN(2, 16); break;
  }
#undef N2V_PQ_SCAN
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n_queries), dim3(256), 0, st, p.s0, p.r0, p.s1, p.r1,
                     nprobe * p.chunks, k, out_rows, out_scores);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
