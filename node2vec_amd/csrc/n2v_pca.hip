// n2v_pca.hip -- the moments of a row-major fp32 matrix X[n, dim] that principal components need: the fp64 column
// means and the symmetric dim x dim scatter matrix of the centred rows, each in one pass that reads X once (for
// dim <= 128) and leaves it in HBM.  The scatter is an MFMA chain whose k axis is the rows: a block owns a slab of
// rows, stages 64 centred rows at a time in LDS and keeps its share of the upper-triangle 16 x 16 tiles in
// registers for the whole slab; a finishing kernel folds the slabs in fp64 and writes both halves.  No float
// atomics; every result is a function of (X, inv_norm, center) alone (DESIGN.md "Principal components";
// tests/cpu_pca/n2v_pca_cpu.c restates it).
//
// Row r enters as xh[d] = x[d] (inv_norm null) or x[d] * inv_norm[r] (one fp32 multiply).  It is USED when all dim
// values xh[d] are finite; every other row is skipped by both passes and not counted in n_used.
// Rows are cut into slabs of slab_rows(n, dim) (a multiple of 64); a step is 64 rows counted from the slab's first
// row, wave w of the block (0..3) owning rows 16 w .. 16 w + 15 of every step.
//   mean:    per slab s, column d and wave w: c_w = 0.0; c_w = c_w + (double)xh[r][d] over the wave's used rows
//            ascending;  M[s][d] = ((c_0 + c_1) + c_2) + c_3;  mean[d] = (0.0 + M[0][d] + M[1][d] + ..) / n_used,
//            zeros when n_used == 0.
//   scatter: xc[r][d] = xh[r][d] - center[d] (one fp32 subtraction; center null: xc = xh).  Per slab s and a <= b:
//            acc = +0; over the rows of the slab's steps ascending, acc = fmaf(xc[r][a], xc[r][b], acc) for a used
//            row and acc = fmaf(+0, +0, acc) for a skipped row or one that pads the last step (a -0 accumulator
//            becomes +0);  S[a][b] = S[b][a] = 0.0 + (double)acc_0 + (double)acc_1 + .. over the slabs ascending.
// The chain runs on v_mfma_f32_16x16x4_f32, four rows per instruction, ascending.
//
// Tiles and groups.  T = round_up(dim, 16) / 16 tile columns, cut into super-columns of 8 (128 columns).  A block
// of the diagonal launch (grid y = I) stages columns [128 I, 128 I + 128) and holds the <= 36 tiles (ti <= tj) of
// that super-column, 9 per wave; a block of the off-diagonal launch (grid y = 2 pair(I < J) + half) stages
// super-column I and the 64 columns [128 J + 64 half, ..) and holds their <= 32 tiles, 8 per wave.  dim <= 128
// is the one diagonal group: X is read once.  Beyond, every group reads whole rows again (the used flag needs
// them) and stages only its columns: correct at any dim <= 1024, not fast.
#include "n2v_score_tile.h"

namespace {

constexpr int kStepRows = kSlabStepRows;
constexpr int kSuper = 128;  // columns of operand range A: a super-column of 8 tile columns
constexpr int kHalf = 64;    // columns of operand range B of an off-diagonal group
// floats per LDS row, 16 mod 32: an operand read (ds_read_b32: 32 lanes per pass, 2 rows x 16 columns) finds its
// two rows 16 banks apart; 16-byte aligned rows for the staging stores
constexpr int kStrideA = kSuper + 16, kStrideB = kHalf + 16;

// how a wave holds a row: lane l owns the units j = 0 .. NJ - 1 at columns W (l + 64 j) .. + W - 1 -- one 16-byte
// load each when VEC, one float otherwise; BIG: rows too long for the short form; RB rows are in flight at a time
template <bool VEC, bool BIG>
struct RowShape {
  static constexpr int W = VEC ? 4 : 1;
  static constexpr int NJ = VEC ? (BIG ? 4 : 1) : (BIG ? 16 : 2);
  static constexpr int N = W * NJ;
  static constexpr int RB = BIG ? 2 : 8;
};
inline bool big_row(int32_t dim, bool vec) { return dim > (vec ? 256 : 128); }

// the lane's values of a row (xr null: a row that pads the step); columns at or beyond dim read as 0
template <bool VEC, bool BIG>
__device__ inline void load_row(const float *__restrict__ xr, int32_t dim, int lane, float *v) {
  using Sh = RowShape<VEC, BIG>;
#pragma unroll
  for (int j = 0; j < Sh::NJ; ++j) {
    const int d = Sh::W * (lane + 64 * j);
    const bool in = xr && d < dim;
    if constexpr (VEC) {
      const f32x4 t = in ? *reinterpret_cast<const f32x4 *>(xr + d) : f32x4{0.f, 0.f, 0.f, 0.f};
      v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
    } else {
      v[j] = in ? xr[d] : 0.f;
    }
  }
}

// v becomes xh (scaled by s when `scaled`); true when the row is live and all its dim values are finite
template <bool VEC, bool BIG>
__device__ inline bool scale_and_flag(float *v, float s, bool scaled, bool live, int32_t dim, int lane) {
  using Sh = RowShape<VEC, BIG>;
  bool fin = true;
#pragma unroll
  for (int j = 0; j < Sh::NJ; ++j) {
    const int d = Sh::W * (lane + 64 * j);
#pragma unroll
    for (int e = 0; e < Sh::W; ++e) {
      float &x = v[Sh::W * j + e];
      if (scaled) x = x * s;
      if (d < dim) fin = fin && (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    }
  }
  return live && __all(fin);
}

// the slabs, and the workspace `ws` laid out (ws null: only `bytes` means anything): the slabs' partial scatter
// [dp][dp] (tiles on and above the diagonal), partial column sums and used-row counts
struct Plan {
  SlabPlan slabs;
  int32_t dp;
  int64_t bytes;
  float *P;
  double *M;
  int64_t *cnt;
};

Plan plan_of(int64_t n, int32_t dim, void *ws) {
  Plan p{};
  p.dp = dim_pad_of(dim);
  p.slabs = slab_plan(n, (int64_t)p.dp * p.dp * 4);
  Carver carve(ws);
  p.P = carve.take<float>((int64_t)p.slabs.n_slabs * p.dp * p.dp * 4);
  p.M = carve.take<double>((int64_t)p.slabs.n_slabs * dim * 8);
  p.cnt = carve.take<int64_t>((int64_t)p.slabs.n_slabs * 8);
  p.bytes = carve.used;
  return p;
}

// Block s owns slab s.  A wave sums its rows of every step into fp64 accumulators (a lane owns its columns); the
// four waves' sums are added in wave order.
template <bool VEC, bool BIG>
__global__ __launch_bounds__(256) void mean_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                   int64_t n, int32_t dim, int64_t slab_rows,
                                                   double *__restrict__ M, int64_t *__restrict__ cnt) {
  using Sh = RowShape<VEC, BIG>;
  __shared__ double swave[3][1024];
  __shared__ int scnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  double acc[Sh::N];
#pragma unroll
  for (int i = 0; i < Sh::N; ++i) acc[i] = 0.0;
  int used_rows = 0;
  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t row0 = base + 16 * wave;
    for (int i0 = 0; i0 < 16; i0 += Sh::RB) {
      float v[Sh::RB][Sh::N], s[Sh::RB];
#pragma unroll
      for (int b = 0; b < Sh::RB; ++b) {
        const int64_t r = row0 + i0 + b;
        load_row<VEC, BIG>(r < hi ? X + r * (int64_t)dim : nullptr, dim, lane, v[b]);
        s[b] = (inv_norm && r < hi) ? inv_norm[r] : 1.f;
      }
#pragma unroll
      for (int b = 0; b < Sh::RB; ++b) {
        const bool used = scale_and_flag<VEC, BIG>(v[b], s[b], inv_norm != nullptr, row0 + i0 + b < hi, dim, lane);
        if (!used) continue;
        ++used_rows;
#pragma unroll
        for (int i = 0; i < Sh::N; ++i) acc[i] = acc[i] + (double)v[b][i];
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < Sh::NJ; ++j)
#pragma unroll
      for (int e = 0; e < Sh::W; ++e) {
        const int d = Sh::W * (lane + 64 * j) + e;
        if (d < dim) swave[wave - 1][d] = acc[Sh::W * j + e];
      }
  }
  if (lane == 0) scnt[wave] = used_rows;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < Sh::NJ; ++j)
#pragma unroll
      for (int e = 0; e < Sh::W; ++e) {
        const int d = Sh::W * (lane + 64 * j) + e;
        if (d < dim)
          M[(int64_t)blockIdx.x * dim + d] = ((acc[Sh::W * j + e] + swave[0][d]) + swave[1][d]) + swave[2][d];
      }
    if (lane == 0) cnt[blockIdx.x] = (int64_t)scnt[0] + scnt[1] + scnt[2] + scnt[3];
  }
}

// Block (s, g) owns slab s and tile group g.  Per step of 64 rows a wave stages its 16 rows' centred values of the
// group's columns in LDS (a row that is not used as +0, never as 0 - center); after the barrier every wave runs
// the step's 16 MFMAs into each of its tiles, both operands read from LDS (lane l: column l & 15 of the tile's
// column block, row 4 q + (l >> 4)).  The accumulators leave the registers once, after the slab's last step.
template <bool VEC, bool BIG, bool OFF>
__global__ __launch_bounds__(256) void scatter_kernel(const float *__restrict__ X, const float *__restrict__ inv_norm,
                                                      int64_t n, int32_t dim, const float *__restrict__ center,
                                                      int64_t slab_rows, float *__restrict__ P,
                                                      int64_t *__restrict__ cnt) {
  using Sh = RowShape<VEC, BIG>;
  constexpr int kSlots = OFF ? 8 : 9;
  constexpr int kBaseB = kStepRows * kStrideA;  // range B follows range A
  constexpr int kLds = kBaseB + (OFF ? kStepRows * kStrideB : 0);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  __shared__ int scnt[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t dp = dim_pad_of(dim);
  const int T = dp / 16;
  // the group: range A = super-column I, range B (OFF) = half a super-column J > I
  int a0, b0, ta, tb, ntiles;
  if constexpr (OFF) {
    int pr = (int)blockIdx.y >> 1, J = 1;
    while (pr >= J) pr -= J, ++J;
    a0 = kSuper * pr;
    b0 = kSuper * J + kHalf * ((int)blockIdx.y & 1);
    ta = 8;
    tb = T - b0 / 16 < 4 ? T - b0 / 16 : 4;
    if (tb <= 0) return;  // the last super-column has no second half
    ntiles = ta * tb;
  } else {
    a0 = b0 = kSuper * (int)blockIdx.y;
    ta = tb = T - a0 / 16 < 8 ? T - a0 / 16 : 8;
    ntiles = ta * (ta + 1) / 2;
  }
  // slot s of wave w is tile 4 s + w of the group (row-major over ti, tj; the diagonal group's tj >= ti)
  int ti[kSlots], tj[kSlots], oa[kSlots], ob[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int t = 4 * s + wave;
    int i = 0, j = 0;
    if (t < ntiles) {
      if constexpr (OFF) {
        i = t / tb, j = t % tb;
      } else {
        int rem = t;
        while (rem >= ta - i) rem -= ta - i, ++i;
        j = i + rem;
      }
    }
    ti[s] = i, tj[s] = j;
    oa[s] = (lane >> 4) * kStrideA + 16 * i + (lane & 15);
    ob[s] = OFF ? kBaseB + (lane >> 4) * kStrideB + 16 * j + (lane & 15)
                : (lane >> 4) * kStrideA + 16 * j + (lane & 15);
  }
  // columns of a tile beyond dim are never staged: they stay +0
  for (int i = tid; i < kLds; i += 256) lds[i] = 0.f;
  float cen[Sh::N];
#pragma unroll
  for (int j = 0; j < Sh::NJ; ++j)
#pragma unroll
    for (int e = 0; e < Sh::W; ++e) {
      const int d = Sh::W * (lane + 64 * j) + e;
      cen[Sh::W * j + e] = (center && d < dim) ? center[d] : 0.f;
    }
  f32x4 acc[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  int used_rows = 0;
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  __syncthreads();

  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int64_t row0 = base + 16 * wave;
    for (int i0 = 0; i0 < 16; i0 += Sh::RB) {
      float v[Sh::RB][Sh::N], sc[Sh::RB];
#pragma unroll
      for (int b = 0; b < Sh::RB; ++b) {
        const int64_t r = row0 + i0 + b;
        load_row<VEC, BIG>(r < hi ? X + r * (int64_t)dim : nullptr, dim, lane, v[b]);
        sc[b] = (inv_norm && r < hi) ? inv_norm[r] : 1.f;
      }
#pragma unroll
      for (int b = 0; b < Sh::RB; ++b) {
        const bool used = scale_and_flag<VEC, BIG>(v[b], sc[b], inv_norm != nullptr, row0 + i0 + b < hi, dim, lane);
        used_rows += used ? 1 : 0;
        const int rl = 16 * wave + i0 + b;  // the row within the step
#pragma unroll
        for (int j = 0; j < Sh::NJ; ++j) {
          const int d = Sh::W * (lane + 64 * j);
          if (d >= dim) continue;
          float xc[Sh::W];
#pragma unroll
          for (int e = 0; e < Sh::W; ++e) {
            const float x = v[b][Sh::W * j + e];
            xc[e] = used ? (center ? x - cen[Sh::W * j + e] : x) : 0.f;
          }
          if ((unsigned)(d - a0) < (unsigned)kSuper) {
            float *at = lds + rl * kStrideA + (d - a0);
            if constexpr (VEC) *reinterpret_cast<f32x4 *>(at) = f32x4{xc[0], xc[1], xc[2], xc[3]};
            else at[0] = xc[0];
          }
          if constexpr (OFF) {
            if ((unsigned)(d - b0) < (unsigned)kHalf) {
              float *at = lds + kBaseB + rl * kStrideB + (d - b0);
              if constexpr (VEC) *reinterpret_cast<f32x4 *>(at) = f32x4{xc[0], xc[1], xc[2], xc[3]};
              else at[0] = xc[0];
            }
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kStepRows / 4; ++q) {
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        const float a = lds[oa[s] + 4 * q * kStrideA];
        const float b = lds[ob[s] + 4 * q * (OFF ? kStrideB : kStrideA)];
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[s], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  float *mine = P + (int64_t)blockIdx.x * dp * dp;
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (4 * s + wave >= ntiles) continue;
    const int col = b0 + 16 * tj[s] + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) mine[(int64_t)(a0 + 16 * ti[s] + 4 * (lane >> 4) + i) * dp + col] = acc[s][i];
  }
  if (!OFF && blockIdx.y == 0) {
    if (lane == 0) scnt[wave] = used_rows;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = (int64_t)scnt[0] + scnt[1] + scnt[2] + scnt[3];
  }
}

__device__ inline int64_t used_total(const int64_t *__restrict__ cnt, int32_t n_slabs) {
  int64_t t = 0;
  for (int32_t sl = 0; sl < n_slabs; ++sl) t += cnt[sl];
  return t;
}

// a thread per column: the slabs' sums folded in ascending slab order, divided by the number of used rows
__global__ __launch_bounds__(256) void fold_mean_kernel(const double *__restrict__ M, const int64_t *__restrict__ cnt,
                                                        int32_t n_slabs, int32_t dim, double *__restrict__ mean,
                                                        int64_t *__restrict__ n_used) {
  const int32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= dim) return;
  const int64_t used = used_total(cnt, n_slabs);
  double s = 0.0;
  for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + M[(int64_t)sl * dim + d];
  mean[d] = used > 0 ? s / (double)used : 0.0;
  if (d == 0) n_used[0] = used;
}

// a thread per element on or above the diagonal: the slab partials folded in ascending slab order in fp64, written
// to both halves
__global__ __launch_bounds__(256) void fold_scatter_kernel(const float *__restrict__ P, const int64_t *__restrict__ cnt,
                                                           int32_t n_slabs, int32_t dim, int32_t dp,
                                                           double *__restrict__ S, int64_t *__restrict__ n_used) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) n_used[0] = used_total(cnt, n_slabs);
  if (i >= (int64_t)dim * dim) return;
  const int32_t a = (int32_t)(i / dim), b = (int32_t)(i % dim);
  if (a > b) return;
  const float *p = P + (int64_t)a * dp + b;
  double s = 0.0;
  for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + (double)p[(int64_t)sl * dp * dp];
  S[(int64_t)a * dim + b] = s;
  S[(int64_t)b * dim + a] = s;
}

// f(VEC, BIG): the two runtime choices of the row shape as template arguments
template <typename F>
inline void with_row_shape(int32_t dim, bool vec, F &&f) {
  with_bool(vec, [&](auto v) { with_bool(big_row(dim, vec), [&](auto big) { f(v, big); }); });
}

}  // namespace

extern "C" {

int64_t n2v_pca_slab_rows(int64_t n, int32_t dim) {
  if (!matrix_ok(n, dim)) return -1;
  return plan_of(n, dim, nullptr).slabs.slab_rows;
}

int64_t n2v_pca_workspace_bytes(int64_t n, int32_t dim) {
  if (!matrix_ok(n, dim)) return -1;
  return n == 0 ? 0 : plan_of(n, dim, nullptr).bytes;
}

int n2v_pca_mean(const float *X, const float *inv_norm, int64_t n, int32_t dim, double *mean, int64_t *n_used,
                 void *workspace, int64_t workspace_bytes, void *stream) {
  if (!matrix_ok(n, dim)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const Plan p = plan_of(n, dim, workspace);
  if (!X || !mean || !n_used || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  with_row_shape(dim, vec_ok(dim, X), [&](auto VEC, auto BIG) {
    hipLaunchKernelGGL((mean_kernel<VEC, BIG>), dim3((unsigned)p.slabs.n_slabs), dim3(256), 0, st, X, inv_norm, n, dim,
                       p.slabs.slab_rows, p.M, p.cnt);
  });
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold_mean_kernel, dim3((unsigned)((dim + 255) / 256)), dim3(256), 0, st, p.M, p.cnt,
                     p.slabs.n_slabs, dim, mean, n_used);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_pca_scatter(const float *X, const float *inv_norm, int64_t n, int32_t dim, const float *center, double *S,
                    int64_t *n_used, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!matrix_ok(n, dim)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const Plan p = plan_of(n, dim, workspace);
  if (!X || !S || !n_used || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned supers = (unsigned)((p.dp + kSuper - 1) / kSuper);
  with_row_shape(dim, vec_ok(dim, X), [&](auto VEC, auto BIG) {
    hipLaunchKernelGGL((scatter_kernel<VEC, BIG, false>), dim3((unsigned)p.slabs.n_slabs, supers), dim3(256), 0, st, X,
                       inv_norm, n, dim, center, p.slabs.slab_rows, p.P, p.cnt);
    if (supers > 1)
      hipLaunchKernelGGL((scatter_kernel<VEC, BIG, true>), dim3((unsigned)p.slabs.n_slabs, supers * (supers - 1)),
                         dim3(256), 0, st, X, inv_norm, n, dim, center, p.slabs.slab_rows, p.P, p.cnt);
  });
  N2V_HIP_CHECK(hipGetLastError());
  const int64_t elems = (int64_t)dim * dim;
  hipLaunchKernelGGL(fold_scatter_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, p.P, p.cnt,
                     p.slabs.n_slabs, dim, p.dp, S, n_used);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
