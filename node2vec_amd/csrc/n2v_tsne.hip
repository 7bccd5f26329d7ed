// n2v_tsne.hip -- the inner loop of exact t-SNE over 2-D points Y[n, 2]: the all-pairs Student-t repulsion with its
// normaliser Z (n2v_tsne_repulse) and the sparse attraction, gradient and gain / momentum update of one iteration
// (n2v_tsne_step).  No float atomics; every result is a function of the arguments alone, bit for bit (DESIGN.md
// "t-SNE"; tests/cpu_tsne/n2v_tsne_cpu.c restates both).
//
// A pair (i, j), in fp32, every operation rounded once:
//   dx = yi.x - yj.x;  dy = yi.y - yj.y;  d2 = fmaf(dy, dy, dx * dx);  w = 1.0f / (1.0f + d2)  (correctly rounded)
// Repulsion of row i over a tile of kTile columns, j ascending, j == i skipped by index, from sw = sx = sy = +0:
//   sw = sw + w;  w2 = w * w;  sx = fmaf(w2, dx, sx);  sy = fmaf(w2, dy, sy)
// The columns are cut into slabs of slab_cols (whole tiles, n2v_tsne_plan).  Per (row, slab) three fp64 sums start at
// 0.0 and take (double)sx, (double)sy, (double)sw at the end of every tile, tiles ascending; they are the slab's
// partials.  The fold adds a row's partials to 0.0 over the slabs ascending: rep[i] = {X, Y}, zrow[i] = W.
// Z: per block of 256 rows b = 0.0 + zrow[256 k] + zrow[256 k + 1] + .. ascending; Z = 0.0 + b_0 + b_1 + .. ascending.
//
// Mapping of the repulsion: a block of 256 lanes owns 256 rows (a lane per row) and one column slab; the y_j of a
// tile are staged in LDS and read at ONE address by all lanes of a wave (a broadcast: no bank conflict).  The fold
// is a lane per row; the block that finishes last (an integer ticket) adds the blocks' sums in block order, so the
// order of the additions does not depend on which block that is.
//
// Step, per row i: a group of 16 lanes, lane l takes the CSR entries rowptr[i] + l, + 16, .. ascending; per entry
// (column j, value p): the pair as above, a = p * w;  ax = fmaf(a, dx, ax);  ay = fmaf(a, dy, ay) from +0.  The 16
// lane sums fold by the butterfly v[l] = v[l] + v[l ^ m], m = 8, 4, 2, 1.  Then per coordinate c:
//   r = (float)(rep[i][c] / Z[0])  (fp64 division, one rounding to fp32)
//   g = 4.0f * (exaggeration * a_c - r)  (product, difference, product)
//   gain = ((g > 0) != (vel > 0)) ? gain + 0.2f : gain * 0.8f;  gain = fmaxf(gain, min_gain)
//   vel = momentum * vel - learning_rate * (gain * g)  (three products and the difference, each rounded)
//   y_next = y + vel
// An entry whose column is outside [0, n) contributes nothing and is never an index; the entries of a row are
// clamped to [0, nnz).
#include "n2v_dense_host.h"

namespace {

constexpr int kTile = 1024;          // columns per tile: 8 KiB of LDS
constexpr int kRows = 256;           // rows per block: a lane per row
constexpr int kTargetBlocks = 2048;  // blocks of the repulsion launch the plan aims at (8 per CU)
constexpr int kGroup = 16;           // lanes per row of the step
constexpr int kStepRows = 256 / kGroup;

struct Plan {
  int64_t slab_cols;
  int32_t n_slabs;
  int64_t row_blocks;
  int64_t bytes;
  double *part;        // [n_slabs][n][3]
  double *block_sum;   // [row_blocks]
  unsigned *ticket;    // [1]
};

Plan plan_of(int64_t n, void *ws) {
  Plan p{};
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  p.row_blocks = (n + kRows - 1) / kRows;
  int64_t want = p.row_blocks > 0 ? kTargetBlocks / p.row_blocks : 1;
  if (want < 1) want = 1;
  if (want > n_tiles) want = n_tiles;
  const int64_t tiles_per_slab = want > 0 ? (n_tiles + want - 1) / want : 1;
  p.slab_cols = tiles_per_slab * kTile;
  p.n_slabs = (int32_t)(n_tiles > 0 ? (n_tiles + tiles_per_slab - 1) / tiles_per_slab : 0);
  Carver carve(ws);
  p.part = carve.take<double>((int64_t)p.n_slabs * n * 24);
  p.block_sum = carve.take<double>(p.row_blocks * 8);
  p.ticket = carve.take<unsigned>(4);
  p.bytes = carve.used;
  return p;
}

struct Pair {
  float dx, dy, w;
};

__device__ __forceinline__ Pair pair_of(float2 yi, float2 yj) {
  Pair p;
  p.dx = yi.x - yj.x;
  p.dy = yi.y - yj.y;
  const float d2 = fmaf(p.dy, p.dy, p.dx * p.dx);
  p.w = 1.0f / (1.0f + d2);
  return p;
}

// the tile's `cnt` columns against the lane's row; DIAG: the tile holds the block's own rows, `self` is the lane's
// own column within it (skipped by index)
template <bool DIAG>
__device__ __forceinline__ void tile_loop(const float2 *__restrict__ tile, int cnt, float2 yi, int self, float &sw,
                                          float &sx, float &sy) {
#pragma unroll 8
  for (int jj = 0; jj < cnt; ++jj) {
    const Pair p = pair_of(yi, tile[jj]);
    if (DIAG && jj == self) continue;
    sw = sw + p.w;
    const float w2 = p.w * p.w;
    sx = fmaf(w2, p.dx, sx);
    sy = fmaf(w2, p.dy, sy);
  }
}

__global__ __launch_bounds__(kRows) void repulse_kernel(const float2 *__restrict__ Y, int64_t n, int64_t slab_cols,
                                                        double *__restrict__ part, unsigned *__restrict__ ticket) {
  __shared__ float2 tile[kTile];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) ticket[0] = 0u;  // the fold's ticket starts at 0
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int64_t i = row0 + tid;
  const float2 yi = i < n ? Y[i] : float2{0.f, 0.f};
  const int64_t lo = (int64_t)blockIdx.y * slab_cols;
  const int64_t hi = lo + slab_cols < n ? lo + slab_cols : n;
  double ax = 0.0, ay = 0.0, aw = 0.0;
  for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
    const int cnt = (int)(hi - t0 < kTile ? hi - t0 : kTile);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTile / kRows; ++k) {
      const int jj = tid + kRows * k;
      tile[jj] = jj < cnt ? Y[t0 + jj] : float2{0.f, 0.f};
    }
    __syncthreads();
    float sw = 0.f, sx = 0.f, sy = 0.f;
    if (row0 >= t0 && row0 < t0 + kTile) tile_loop<true>(tile, cnt, yi, (int)(i - t0), sw, sx, sy);
    else tile_loop<false>(tile, cnt, yi, -1, sw, sx, sy);
    ax = ax + (double)sx;
    ay = ay + (double)sy;
    aw = aw + (double)sw;
  }
  if (i < n) {
    double *mine = part + ((int64_t)blockIdx.y * n + i) * 3;
    mine[0] = ax;
    mine[1] = ay;
    mine[2] = aw;
  }
}

// a lane per row: the slabs' partials added in slab order; lane 0 adds the block's zrow in row order; the block that
// takes the last ticket adds the blocks' sums in block order
__global__ __launch_bounds__(kRows) void fold_kernel(const double *__restrict__ part, int64_t n, int32_t n_slabs,
                                                     double *__restrict__ rep, double *__restrict__ zrow,
                                                     double *block_sum, unsigned *ticket, double *__restrict__ Z) {
  __shared__ double sz[kRows];
  __shared__ bool last;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int64_t i = row0 + tid;
  double x = 0.0, y = 0.0, w = 0.0;
  if (i < n) {
    for (int32_t s = 0; s < n_slabs; ++s) {
      const double *p = part + ((int64_t)s * n + i) * 3;
      x = x + p[0];
      y = y + p[1];
      w = w + p[2];
    }
    rep[2 * i] = x;
    rep[2 * i + 1] = y;
    zrow[i] = w;
  }
  sz[tid] = w;
  __syncthreads();
  if (tid == 0) {
    const int rows = (int)(n - row0 < kRows ? n - row0 : kRows);
    double b = 0.0;
    for (int k = 0; k < rows; ++k) b = b + sz[k];
    __hip_atomic_store(&block_sum[blockIdx.x], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  double z = 0.0;
  for (int64_t base = 0; base < (int64_t)gridDim.x; base += kRows) {
    const int64_t b = base + tid;
    __syncthreads();
    sz[tid] = b < (int64_t)gridDim.x
                  ? __hip_atomic_load(&block_sum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : 0.0;
    __syncthreads();
    if (tid == 0) {
      const int cnt = (int)((int64_t)gridDim.x - base < kRows ? (int64_t)gridDim.x - base : kRows);
      for (int k = 0; k < cnt; ++k) z = z + sz[k];
    }
  }
  if (tid == 0) Z[0] = z;
}

__device__ __forceinline__ float butterfly16(float v) {
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

struct StepScalars {
  float exaggeration, learning_rate, momentum, min_gain;
};

__device__ __forceinline__ void update(float a, double rep, double z, const StepScalars &s, float y, float &vel,
                                       float &gain, float &y_next, float &grad) {
  const float r = (float)(rep / z);
  const float t = s.exaggeration * a;
  const float u = t - r;
  const float g = 4.0f * u;
  float gn = ((g > 0.f) != (vel > 0.f)) ? gain + 0.2f : gain * 0.8f;
  gn = fmaxf(gn, s.min_gain);
  const float p1 = s.momentum * vel;
  const float p2 = gn * g;
  const float p3 = s.learning_rate * p2;
  const float v = p1 - p3;
  grad = g;
  gain = gn;
  vel = v;
  y_next = y + v;
}

__global__ __launch_bounds__(256) void step_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const float *__restrict__ val, int64_t nnz,
                                                   const float2 *__restrict__ Y, const double *__restrict__ rep,
                                                   const double *__restrict__ Z, int64_t n, StepScalars s,
                                                   float2 *__restrict__ vel, float2 *__restrict__ gain,
                                                   float2 *__restrict__ Y_next, float2 *__restrict__ grad) {
  const int l = threadIdx.x & (kGroup - 1);
  const int64_t i = (int64_t)blockIdx.x * kStepRows + (threadIdx.x / kGroup);
  const bool live = i < n;  // (no early return: the butterfly runs on whole waves)
  float ax = 0.f, ay = 0.f;
  float2 yi = float2{0.f, 0.f};
  if (live) {
    yi = Y[i];
    int64_t lo = rowptr[i], hi = rowptr[i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > nnz ? nnz : hi;
    for (int64_t e = lo + l; e < hi; e += kGroup) {
      const int32_t j = col[e];
      if ((uint32_t)j >= (uint64_t)n) continue;
      const Pair p = pair_of(yi, Y[j]);
      const float a = val[e] * p.w;
      ax = fmaf(a, p.dx, ax);
      ay = fmaf(a, p.dy, ay);
    }
  }
  ax = butterfly16(ax);
  ay = butterfly16(ay);
  if (!live || l != 0) return;
  const double z = Z[0];
  float2 v = vel[i], gn = gain[i], yn, g;
  update(ax, rep[2 * i], z, s, yi.x, v.x, gn.x, yn.x, g.x);
  update(ay, rep[2 * i + 1], z, s, yi.y, v.y, gn.y, yn.y, g.y);
  vel[i] = v;
  gain[i] = gn;
  Y_next[i] = yn;
  grad[i] = g;
}

inline bool rows_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

int n2v_tsne_plan(int64_t n, int32_t *tile, int64_t *slab_cols, int32_t *n_slabs) {
  if (!rows_ok(n) || !tile || !slab_cols || !n_slabs) return N2V_EINVAL;
  const Plan p = plan_of(n, nullptr);
  *tile = kTile;
  *slab_cols = p.slab_cols;
  *n_slabs = p.n_slabs;
  return N2V_OK;
}

int64_t n2v_tsne_workspace_bytes(int64_t n) {
  if (!rows_ok(n)) return -1;
  return n == 0 ? 0 : plan_of(n, nullptr).bytes;
}

int n2v_tsne_repulse(const float *Y, int64_t n, double *rep_out, double *zrow_out, double *z_out, void *workspace,
                     int64_t workspace_bytes, void *stream) {
  if (!rows_ok(n)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const Plan p = plan_of(n, workspace);
  if (!Y || !rep_out || !zrow_out || !z_out || ((uintptr_t)Y & 7) != 0 ||
      !workspace_ok(workspace, workspace_bytes, p.bytes))
    return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(repulse_kernel, dim3((unsigned)p.row_blocks, (unsigned)p.n_slabs), dim3(kRows), 0, st,
                     reinterpret_cast<const float2 *>(Y), n, p.slab_cols, p.part, p.ticket);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)p.row_blocks), dim3(kRows), 0, st, p.part, n, p.n_slabs, rep_out,
                     zrow_out, p.block_sum, p.ticket, z_out);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_tsne_step(const int64_t *rowptr, const int32_t *col, const float *val, int64_t nnz, const float *Y,
                  const double *rep, const double *Z, int64_t n, float exaggeration, float learning_rate,
                  float momentum, float min_gain, float *vel, float *gain, float *Y_next, float *grad_out,
                  void *stream) {
  if (!rows_ok(n) || nnz < 0) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  if (!rowptr || (nnz > 0 && (!col || !val)) || !Y || !rep || !Z || !vel || !gain || !Y_next || !grad_out ||
      Y == Y_next || (((uintptr_t)Y | (uintptr_t)Y_next | (uintptr_t)vel | (uintptr_t)gain | (uintptr_t)grad_out) & 7))
    return N2V_EINVAL;
  const StepScalars s{exaggeration, learning_rate, momentum, min_gain};
  hipLaunchKernelGGL(step_kernel, dim3((unsigned)((n + kStepRows - 1) / kStepRows)), dim3(256), 0, (hipStream_t)stream,
                     rowptr, col, val, nnz, reinterpret_cast<const float2 *>(Y), rep, Z, n, s,
                     reinterpret_cast<float2 *>(vel), reinterpret_cast<float2 *>(gain),
                     reinterpret_cast<float2 *>(Y_next), reinterpret_cast<float2 *>(grad_out));
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
