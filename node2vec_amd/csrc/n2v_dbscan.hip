// n2v_dbscan.hip -- DBSCAN of the rows of X[n, dim] (DESIGN.md "Density clustering"): three scans over (tile of
// columns x chunk of rows), all on score_rows' MFMA chain (n2v_score_tile.h).  Nothing of size n x n and no
// neighbour list is stored: the memory beyond X is the padded operand and O(n) integers.
//
// The canonical result.  Row i is CORE when at least min_samples rows, itself included, are within eps of it.  A
// cluster is a connected component of the core rows under "within eps"; clusters are numbered by their lowest core
// row; a row that is not core takes the lowest-numbered cluster that has a core row within eps of it, or -1.  This
// depends on the SET of pairs within eps alone, and the pair test has fixed bits, so the labels are the same on every
// launch geometry although integer atomics carry them (tests/cpu_dbscan/n2v_dbscan_cpu.c restates all of it).
//
// The pair test, spelled once (within()), symmetric in (i, j) bit for bit; fp32, one rounding per spelled operation:
//   dot(i, j)  score_rows' chain: acc = +0; for d0 = 0, 16, .. < dim_pad, e = 0..3, q = 0..3, d = d0 + 4 q + e:
//              acc = fmaf(x_i[d], x_j[d], acc), both 0 past dim -- the same products in the same order whichever
//              row is operand A
//   Euclidean  d2 = fmaxf(fmaf(-2, dot, xn_i + xn_j), 0) <= eps2, xn = wave_sumsq, eps2 = eps * eps in fp32 (no
//              square root; the sum of the two norms comes first, or the expression would not be symmetric)
//   cosine     1 - dot * (inv_i * inv_j) <= eps (a zero row has inv = 0: at distance 1 from everything)
// A row always counts itself: the self-pair is added by hand and i == j is skipped in the scans, so nothing rests on
// d2(i, i) == 0.
//
// A scan: the columns are operand B, gathered and padded to q[cols_pad][dim_pad]; the rows are operand A, read in
// place through a per-lane pointer.  Work item (tile of 16 G columns, chunk of rows); a block takes items blockIdx.x,
// + gridDim.x, ..: any number of blocks gives the same result.  Each of its 4 waves scores 16 rows a step.
//   count   rows and columns: all of X.  Every lane counts its hits in an integer register; the lanes and waves of
//           a block meet in LDS and go to counts[] by integer atomic adds (counts[] starts at 1, the self-pair).
//           A row is shared by many blocks: atomics, not ownership.
//   union   rows and columns: the compact list of core rows.  A pair is taken when the row's list position is below
//           the column's: only tiles on or above the diagonal are scanned.  Every pair within eps is united in the
//           lock-free union-find of n2v_unionfind.h (its rules are written there) over parent[n], parent[i] = i at
//           first.  dbscan_flatten_kernel then sets parent[i] = find(i) for the core rows: the component's lowest
//           core row.
//   border  columns: the rows that are not core; rows: the core rows, whose labels are their cluster ids.
//           labels[column] = the minimum over the core rows within eps of their labels, by unsigned atomicMin (-1,
//           no cluster, is the largest unsigned value).
// A list entry outside [0, n) is dead: never dereferenced, never an index.
#include <math.h>

#include "n2v_score_tile.h"

#define N2V_UF_FN __device__ inline
#define N2V_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define N2V_UF_CAS(p, e, v) atomicCAS((p), (e), (v))
#define N2V_UF_MIN(p, v) atomicMin((p), (v))
#include "n2v_unionfind.h"

namespace {

constexpr int kCount = 0, kUnion = 1, kBorder = 2;
constexpr int kScanWaves = 4;                        // waves per block
constexpr int kScanStepRows = 16 * kScanWaves;       // rows per block step
constexpr int64_t kScanItems = 2048;                 // work items aimed at when the tiles alone are fewer
constexpr int64_t kMinChunkRows = 16 * kScanStepRows;
constexpr uint32_t kNoLabel = 0xffffffffu;           // -1

// are rows i and j within eps?  ai, aj: xn (Euclidean, thr = eps2) or inv_norm (cosine, thr = eps)
__device__ inline bool within(bool cosine, float dot, float ai, float aj, float thr) {
  if (cosine) {
    const float inv2 = ai * aj;
    const float c = dot * inv2;
    return 1.f - c <= thr;
  }
  const float both = ai + aj;
  const float d2 = fmaxf(__fmaf_rn(-2.f, dot, both), 0.f);
  return d2 <= thr;
}

struct Scan {
  const float *X, *aux, *q;   // q: the columns padded, [round_up(n_cols, 64)][dim_pad]
  const int32_t *rows, *cols; // the lists (null: every row of X in order)
  int32_t *out;               // counts / parent / labels, [n]
  int64_t n, n_rows, n_cols, chunk_rows, n_tiles, n_items;
  int32_t dim, cosine;
  float thr;
};

// entry `pos` of a list of `len`: a row of X, or -1 (dead)
__device__ inline int32_t list_row(const int32_t *list, int64_t pos, int64_t len, int64_t n) {
  if (pos >= len) return -1;
  const int64_t r = list ? (int64_t)list[pos] : pos;
  return (r >= 0 && r < n) ? (int32_t)r : -1;
}

template <int MODE, int G, bool VEC>
__global__ __launch_bounds__(kScanWaves * 64) void dbscan_scan_kernel(Scan a) {
  __shared__ uint32_t fold[16 * G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t dp = dim_pad_of(a.dim);
  const bool cosine = a.cosine != 0;
  const uint32_t none = MODE == kBorder ? kNoLabel : 0u;  // the identity of the fold

  for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int64_t q0 = (item % a.n_tiles) * (16 * G);
    const int64_t lo = (item / a.n_tiles) * a.chunk_rows;
    int64_t hi = lo + a.chunk_rows < a.n_rows ? lo + a.chunk_rows : a.n_rows;
    if (MODE == kUnion && hi > q0 + 16 * G) hi = q0 + 16 * G;  // positions at or past the tile's end: never below it
    if (lo >= hi) continue;  // (the whole block)
    if (MODE != kUnion) {
      for (int i = tid; i < 16 * G; i += kScanWaves * 64) fold[i] = none;
      __syncthreads();
    }

    const float *qrow[G];
    int32_t qid[G];
    float qaux[G];
    uint32_t mine[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int64_t cpos = q0 + 16 * g + (lane & 15);  // < round_up(n_cols, 64): a row of q
      qrow[g] = a.q + cpos * dp;
      qid[g] = list_row(a.cols, cpos, a.n_cols, a.n);
      qaux[g] = qid[g] >= 0 ? a.aux[qid[g]] : 0.f;
      mine[g] = none;
    }

    for (int64_t row0 = lo + 16 * wave; row0 < hi; row0 += kScanStepRows) {
      const int32_t r = list_row(a.rows, row0 + (lane & 15), hi, a.n);
      const bool live = r >= 0;
      const float raux = live ? a.aux[r] : 0.f;
      const uint32_t rlab = (MODE == kBorder && live) ? (uint32_t)a.out[r] : kNoLabel;
      f32x4 acc[G];
      score_rows<G, VEC>(a.X + (live ? r : 0) * (int64_t)a.dim, live, a.dim, qrow, lane, acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int src = 4 * (lane >> 4) + e;  // acc[g][e] is (column 16 g + (lane & 15), row `src` of the step)
        const int32_t j = __shfl(r, src, 64);
        const float jaux = __shfl(raux, src, 64);
        const uint32_t jlab = __shfl(rlab, src, 64);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          bool hit = j >= 0 && qid[g] >= 0 && j != qid[g] && within(cosine, acc[g][e], qaux[g], jaux, a.thr);
          if (MODE == kCount) {
            mine[g] += hit ? 1u : 0u;
          } else if (MODE == kBorder) {
            if (hit && jlab < mine[g]) mine[g] = jlab;
          } else {
            hit = hit && row0 + src < q0 + 16 * g + (lane & 15);
            if (hit) uf_unite(a.out, j, qid[g]);
          }
        }
      }
    }
    if (MODE == kUnion) continue;

#pragma unroll
    for (int g = 0; g < G; ++g) {
      // the four lanes that share a column (lane & 15), then the waves
      uint32_t v = mine[g];
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = MODE == kCount ? v + o : (o < v ? o : v);
      }
      if (lane < 16 && v != none) {
        if (MODE == kCount) atomicAdd(&fold[16 * g + lane], v);
        else atomicMin(&fold[16 * g + lane], v);
      }
    }
    __syncthreads();
    for (int i = tid; i < 16 * G; i += kScanWaves * 64) {
      const uint32_t v = fold[i];
      const int32_t c = list_row(a.cols, q0 + i, a.n_cols, a.n);
      if (c < 0 || v == none) continue;
      if (MODE == kCount) atomicAdd(&a.out[c], (int32_t)v);
      else atomicMin(reinterpret_cast<uint32_t *>(a.out) + c, v);
    }
    __syncthreads();  // fold[] is the next item's as well
  }
}

// q[i] = the row list[i] of X (row i when there is no list) padded with zeros; a zero row for a dead entry and for
// i >= m.  One wave per padded row.
__global__ __launch_bounds__(256) void dbscan_pad_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                         const int32_t *__restrict__ list, int64_t m, int64_t m_pad,
                                                         float *__restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int32_t dp = dim_pad_of(dim);
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m_pad) return;
  const int32_t r = list_row(list, i, m, n);
  const bool live = r >= 0;
  const float *v = X + (live ? r : 0) * (int64_t)dim;
  for (int d = lane; d < dp; d += 64) q[i * dp + d] = (live && d < dim) ? v[d] : 0.f;
}

// xn[r] = wave_sumsq(x_r); one wave per row
__global__ __launch_bounds__(256) void dbscan_sumsq_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                           float *__restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float s = wave_sumsq(X + r * dim, dim, lane);
  if (lane == 0) xn[r] = s;
}

// out[i] = base + step * i: counts start at 1 (the self-pair), parent at i
__global__ __launch_bounds__(256) void dbscan_fill_kernel(int32_t *__restrict__ out, int64_t n, int32_t base,
                                                          int32_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = base + step * (int32_t)i;
}

__global__ __launch_bounds__(256) void dbscan_core_kernel(const int32_t *__restrict__ counts, int64_t n,
                                                          int32_t min_samples, uint8_t *__restrict__ core) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) core[i] = counts[i] >= min_samples ? 1 : 0;
}

// parent[r] = find(r) for the core rows: the root of r's component, its lowest core row.  (Lowered by a minimum
// while other threads still walk through r: rule 5 of n2v_unionfind.h.)
__global__ __launch_bounds__(256) void dbscan_flatten_kernel(int32_t *parent, int64_t n,
                                                             const int32_t *__restrict__ core, int64_t n_core) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t r = list_row(core, c, n_core, n);
  if (r < 0) return;
  const int32_t root = uf_find(parent, r);
  if (root != r) atomicMin(&parent[r], root);
}

// the workspace `ws` laid out (ws null: only `bytes` means anything)
struct DbPlan {
  int64_t bytes;
  float *q, *xn;
};

DbPlan plan_db(int64_t n, int32_t dim, void *ws) {
  DbPlan p{};
  Carver carve(ws);
  p.q = carve.take<float>(round_up(n, 64) * dim_pad_of(dim) * 4);
  p.xn = carve.take<float>(n * 4);
  p.bytes = carve.used;
  return p;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// what the three entry points refuse before they look at n == 0
bool args_ok(int64_t n, int32_t dim, int32_t metric, const float *inv_norm, float eps, int32_t max_blocks) {
  if (!matrix_ok(n, dim) || max_blocks < 0) return false;
  if (metric != N2V_KMEANS_EUCLIDEAN && metric != N2V_KMEANS_COSINE) return false;
  if (metric == N2V_KMEANS_COSINE && !inv_norm) return false;
  return isfinite(eps) && eps >= 0.f;
}

// One scan: the columns `cols` (n_cols of them; null: all n rows) against the rows `rows` (likewise), on stream st.
// p.q and, for the Euclidean metric, p.xn are written here.
template <int MODE>
int run_scan(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
             const int32_t *rows, int64_t n_rows, const int32_t *cols, int64_t n_cols, int32_t *out,
             const DbPlan &p, int32_t max_blocks, hipStream_t st) {
  const bool cosine = metric == N2V_KMEANS_COSINE;
  if (!cosine) {
    hipLaunchKernelGGL(dbscan_sumsq_kernel, dim3(blocks_of(n, 4)), dim3(256), 0, st, X, n, dim, p.xn);
    N2V_HIP_CHECK(hipGetLastError());
  }
  const int64_t cols_pad = round_up(n_cols, 64);
  hipLaunchKernelGGL(dbscan_pad_kernel, dim3(blocks_of(cols_pad, 4)), dim3(256), 0, st, X, n, dim, cols, n_cols,
                     cols_pad, p.q);
  N2V_HIP_CHECK(hipGetLastError());

  Scan a{};
  a.X = X, a.aux = cosine ? inv_norm : p.xn, a.q = p.q, a.rows = rows, a.cols = cols, a.out = out;
  a.n = n, a.n_rows = n_rows, a.n_cols = n_cols, a.dim = dim, a.cosine = cosine ? 1 : 0;
  a.thr = cosine ? eps : eps * eps;
  const int64_t tile = n_cols <= 16 ? 16 : 64;  // with_tile's G
  a.n_tiles = (n_cols + tile - 1) / tile;
  int64_t chunks = (kScanItems + a.n_tiles - 1) / a.n_tiles;
  const int64_t most = (n_rows + kMinChunkRows - 1) / kMinChunkRows;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  a.chunk_rows = round_up((n_rows + chunks - 1) / chunks, kScanStepRows);
  a.n_items = a.n_tiles * ((n_rows + a.chunk_rows - 1) / a.chunk_rows);
  int64_t blocks = a.n_items;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  hipError_t err = hipSuccess;
  with_tile((int32_t)(n_cols <= 16 ? n_cols : 17), vec_ok(dim, X), [&](auto G, auto VEC) {
    err = n2v::launch_resident<2>(dbscan_scan_kernel<MODE, G, VEC>, kScanWaves * 64, 0, blocks, st, a);
  });
  N2V_HIP_CHECK(err);
  return N2V_OK;
}

}  // namespace

extern "C" {

int64_t n2v_dbscan_workspace_bytes(int64_t n, int32_t dim) {
  if (!matrix_ok(n, dim)) return -1;
  return n == 0 ? 0 : plan_db(n, dim, nullptr).bytes;
}

int n2v_dbscan_count(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                     int32_t min_samples, int32_t *counts_out, uint8_t *core_out, void *workspace,
                     int64_t workspace_bytes, int32_t max_blocks, void *stream) {
  if (!args_ok(n, dim, metric, inv_norm, eps, max_blocks) || min_samples < 1) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const DbPlan p = plan_db(n, dim, workspace);
  if (!X || !counts_out || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dbscan_fill_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, counts_out, n, 1, 0);
  N2V_HIP_CHECK(hipGetLastError());
  const int rc = run_scan<kCount>(X, inv_norm, n, dim, metric, eps, nullptr, n, nullptr, n, counts_out, p, max_blocks,
                                  st);
  if (rc != N2V_OK || !core_out) return rc;
  hipLaunchKernelGGL(dbscan_core_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, counts_out, n, min_samples,
                     core_out);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_dbscan_union(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                     const int32_t *core, int64_t n_core, int32_t *root_out, void *workspace,
                     int64_t workspace_bytes, int32_t max_blocks, void *stream) {
  if (!args_ok(n, dim, metric, inv_norm, eps, max_blocks) || n_core < 0 || n_core > n) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const DbPlan p = plan_db(n, dim, workspace);
  if (!X || !root_out || (n_core > 0 && !core) || !workspace_ok(workspace, workspace_bytes, p.bytes))
    return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dbscan_fill_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, root_out, n, 0, 1);
  N2V_HIP_CHECK(hipGetLastError());
  if (n_core == 0) return N2V_OK;
  const int rc = run_scan<kUnion>(X, inv_norm, n, dim, metric, eps, core, n_core, core, n_core, root_out, p,
                                  max_blocks, st);
  if (rc != N2V_OK) return rc;
  hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(blocks_of(n_core, 256)), dim3(256), 0, st, root_out, n, core,
                     n_core);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_dbscan_border(const float *X, const float *inv_norm, int64_t n, int32_t dim, int32_t metric, float eps,
                      const int32_t *core, int64_t n_core, const int32_t *border, int64_t n_border, int32_t *labels,
                      void *workspace, int64_t workspace_bytes, int32_t max_blocks, void *stream) {
  if (!args_ok(n, dim, metric, inv_norm, eps, max_blocks) || n_core < 0 || n_border < 0 || n_core > n ||
      n_border > n)
    return N2V_EINVAL;
  if (n == 0 || n_core == 0 || n_border == 0) return N2V_OK;
  const DbPlan p = plan_db(n, dim, workspace);
  if (!X || !core || !border || !labels || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  return run_scan<kBorder>(X, inv_norm, n, dim, metric, eps, core, n_core, border, n_border, labels, p, max_blocks,
                           (hipStream_t)stream);
}

}  // extern "C"
