// n2v_logreg.hip -- one-vs-rest logistic regression over a row-major fp32 matrix X[n, dim]: the scores
// z[r][k] = dot(W_k, x_r) + b[k] of c classes, and in one launch that reads X once the summed logistic loss and its
// gradient by W and b.  A block scores 64 rows against 16 or 64 classes at a time with the MFMA chain of
// n2v_score_tile.h, turns the scores into residuals that stay in LDS, and multiplies them with the same rows
// (still in L1 / L2) into the slab's partial gradient with a second MFMA chain whose k axis is the rows; a
// finishing kernel folds the slabs in fp64.  No float atomics; every result is a function of (X, y, W, b) alone
// (DESIGN.md "Node classification"; tests/cpu_logreg/n2v_logreg_cpu.c restates it).
//
// Per (row, class), y the label bit, res = p - y and the loss l are the spelled functions of n2v_logistic.h.
// Rows are cut into slabs of slab_rows(n, dim, c) (a multiple of 64).  Per slab s:
//   GW[s][k][d]: acc = +0; acc = fmaf(res[r][k], x_r[d], acc) over the slab's rows ascending, then over the rows
//                that pad the slab to a multiple of 64 acc = fmaf(+0, +0, acc): a -0 accumulator becomes +0.
//   Gb[s][k]:    acc = +0; acc = acc + res[r][k] over the slab's rows ascending.
//   L[s][k]:     acc = 0.0; acc = acc + (double)l[r][k] over the slab's rows ascending.
// gW, gb and Lk are fp64 chains from 0.0 over s ascending of the (double) partials; loss = 0.0 + Lk[0] + Lk[1] ..
#include <math.h>

#include "n2v_logistic.h"
#include "n2v_score_tile.h"

namespace {

constexpr int kStepRows = kSlabStepRows;
constexpr int kMaxClasses = 1024;

// the slabs, and the workspace `ws` laid out (ws null: only `bytes` means anything): W padded to [c_pad][dim_pad],
// the slabs' partial GW, Gb and L, and the folded Lk
struct Plan {
  SlabPlan slabs;
  int64_t c_pad, bytes;
  float *wpad, *GW, *Gb;
  double *L, *Lk;
};

Plan plan_of(int64_t n, int32_t dim, int32_t c, void *ws) {
  Plan p{};
  p.slabs = slab_plan(n, 4 * (int64_t)c * (dim + 3));  // GW and Gb in fp32, L in fp64
  p.c_pad = round_up(c, 64);
  const int64_t sc = (int64_t)p.slabs.n_slabs * c;
  Carver carve(ws);
  p.wpad = carve.take<float>(p.c_pad * dim_pad_of(dim) * 4);
  p.GW = carve.take<float>(sc * dim * 4);
  p.Gb = carve.take<float>(sc * 4);
  p.L = carve.take<double>(sc * 8);
  p.Lk = carve.take<double>((int64_t)c * 8);
  p.bytes = carve.used;
  return p;
}

// a wave scores 16 rows per step against every class; the steps of 64 rows go round the grid
template <int G, bool VEC>
__global__ __launch_bounds__(256) void scores_kernel(const float *__restrict__ X, int64_t n, int32_t dim,
                                                     const float *__restrict__ wpad, const float *__restrict__ b,
                                                     int32_t c, float *__restrict__ Z) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t dp = dim_pad_of(dim);
  for (int64_t base = (int64_t)blockIdx.x * kStepRows; base < n; base += (int64_t)gridDim.x * kStepRows) {
    const int64_t row0 = base + 16 * wave;
    if (row0 >= n) continue;
    for (int32_t c0 = 0; c0 < c; c0 += 16 * G) {
      f32x4 acc[G];
      score_tile<G, VEC>(X, dim, row0, n, wpad + (int64_t)c0 * dp, lane, acc);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int32_t k = c0 + 16 * g + (lane & 15);
        if (k >= c) continue;
        const float bk = b[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t r = row0 + 4 * (lane >> 4) + i;
          if (r < n) Z[r * c + k] = acc[g][i] + bk;
        }
      }
    }
  }
}

// Block s owns slab s: rows [s slab_rows, ..).  Per step of 64 rows and per chunk of 16 G classes: the scoring
// half leaves res and l of the step in LDS; the gradient half adds res^T x to the slab's partial (a lane owns its
// accumulator elements for the whole slab: it stores them after a step and loads them before the next).
template <int G, bool VEC>
__global__ __launch_bounds__(256) void loss_grad_kernel(const float *__restrict__ X,
                                                        const uint32_t *__restrict__ y_bits, int64_t n, int32_t dim,
                                                        const float *__restrict__ wpad, const float *__restrict__ b,
                                                        int32_t c, float *__restrict__ GW, float *__restrict__ Gb,
                                                        double *__restrict__ L, int64_t slab_rows) {
  constexpr int kChunk = 16 * G;      // classes per chunk
  // floats per LDS row, 16 mod 32: the two rows that the 32 lanes of one LDS pass read for operand A sit 16 banks
  // apart (no conflict); the scoring half's writes, rows 4 apart, are 2-way conflicts
  constexpr int kStride = G == 1 ? 48 : 80;
  __shared__ float sres[kStepRows * kStride];
  __shared__ float sl[kStepRows * kStride];
  __shared__ float sgb[kMaxClasses];
  __shared__ double sloss[kMaxClasses];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t dp = dim_pad_of(dim);
  const int32_t words = (c + 31) >> 5;
  const int64_t lo = (int64_t)blockIdx.x * slab_rows;
  const int64_t hi = lo + slab_rows < n ? lo + slab_rows : n;
  float *mine = GW + (int64_t)blockIdx.x * c * dim;
  // thread tid < kChunk owns class c0 + tid of every chunk, here and below
  if (tid < kChunk)
    for (int32_t k = tid; k < c; k += kChunk) sgb[k] = 0.f, sloss[k] = 0.0;

  for (int64_t base = lo; base < hi; base += kStepRows) {
    const int cnt = hi - base < kStepRows ? (int)(hi - base) : kStepRows;
    const int64_t row0 = base + 16 * wave;
    const bool first = base == lo;
    for (int32_t c0 = 0; c0 < c; c0 += kChunk) {
      {
        f32x4 acc[G];
        score_tile<G, VEC>(X, dim, row0, hi, wpad + (int64_t)c0 * dp, lane, acc);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int32_t k = c0 + 16 * g + (lane & 15);
          const float bk = k < c ? b[k] : 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            sres[(16 * wave + 4 * (lane >> 4) + i) * kStride + 16 * g + (lane & 15)] = acc[g][i] + bk;
        }
      }
      // a lane turns the scores it has just written into residuals, one at a time (a rolled loop: few registers)
#pragma unroll 1
      for (int j = 0; j < 4 * G; ++j) {
        const int g = j >> 2, i = j & 3;
        const int32_t k = c0 + 16 * g + (lane & 15);
        const int rl = 16 * wave + 4 * (lane >> 4) + i;
        const int64_t r = base + rl;
        float res = 0.f, l = 0.f;
        if (r < hi && k < c) {
          const uint32_t y = (y_bits[r * words + (k >> 5)] >> (k & 31)) & 1u;
          const float z = sres[rl * kStride + 16 * g + (lane & 15)];
          logistic_point(z, y, res, l);
        }
        sres[rl * kStride + 16 * g + (lane & 15)] = res;
        sl[rl * kStride + 16 * g + (lane & 15)] = l;
      }
      __syncthreads();
      if (tid < kChunk && c0 + tid < c) {
        float gb = sgb[c0 + tid];
        double ls = sloss[c0 + tid];
        for (int i = 0; i < cnt; ++i) {
          gb = gb + sres[i * kStride + tid];
          ls = ls + (double)sl[i * kStride + tid];
        }
        sgb[c0 + tid] = gb;
        sloss[c0 + tid] = ls;
      }
      // gradient: D[class][d] += sum over the step's rows of res[row][class] x[row][d]; operand A is res (lane l:
      // class l & 15, row l >> 4), operand B is x (d l & 15, row l >> 4); four rows per MFMA, ascending
      for (int32_t d0 = 16 * wave; d0 < dp; d0 += 64) {
        const int32_t d = d0 + (lane & 15);
        float xb[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t r = base + 4 * q + (lane >> 4);
          xb[q] = (r < hi && d < dim) ? X[r * (int64_t)dim + d] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int32_t k0 = c0 + 16 * g + 4 * (lane >> 4);
          if (c0 + 16 * g >= c) break;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if (!first && d < dim) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (k0 + i < c) acc[i] = mine[(int64_t)(k0 + i) * dim + d];
          }
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float a = sres[(4 * q + (lane >> 4)) * kStride + 16 * g + (lane & 15)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[q], acc, 0, 0, 0);
          }
          if (d < dim) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (k0 + i < c) mine[(int64_t)(k0 + i) * dim + d] = acc[i];
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid < kChunk)
    for (int32_t k = tid; k < c; k += kChunk) {
      Gb[(int64_t)blockIdx.x * c + k] = sgb[k];
      L[(int64_t)blockIdx.x * c + k] = sloss[k];
    }
}

// the slab partials folded in ascending slab order in fp64: a thread per element of gW, then of gb and Lk
__global__ __launch_bounds__(256) void fold_kernel(const float *__restrict__ GW, const float *__restrict__ Gb,
                                                   const double *__restrict__ L, int32_t n_slabs, int32_t c,
                                                   int32_t dim, double *__restrict__ gW, double *__restrict__ gb,
                                                   double *__restrict__ Lk) {
  const int64_t cd = (int64_t)c * dim;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cd) {
    double s = 0.0;
    for (int32_t sl = 0; sl < n_slabs; ++sl) s = s + (double)GW[sl * cd + i];
    gW[i] = s;
  } else if (i < cd + c) {
    const int64_t k = i - cd;
    double s = 0.0, l = 0.0;
    for (int32_t sl = 0; sl < n_slabs; ++sl) {
      s = s + (double)Gb[(int64_t)sl * c + k];
      l = l + L[(int64_t)sl * c + k];
    }
    gb[k] = s;
    Lk[k] = l;
  }
}

__global__ void loss_kernel(const double *__restrict__ Lk, int32_t c, double *__restrict__ loss) {
  double s = 0.0;
  for (int32_t k = 0; k < c; ++k) s = s + Lk[k];
  loss[0] = s;
}

bool sizes_ok(int64_t n, int32_t dim, int32_t c) { return matrix_ok(n, dim) && c >= 1 && c <= kMaxClasses; }

}  // namespace

extern "C" {

int64_t n2v_logreg_slab_rows(int64_t n, int32_t dim, int32_t c) {
  if (!sizes_ok(n, dim, c)) return -1;
  return plan_of(n, dim, c, nullptr).slabs.slab_rows;
}

int64_t n2v_logreg_workspace_bytes(int64_t n, int32_t dim, int32_t c) {
  if (!sizes_ok(n, dim, c)) return -1;
  return n == 0 ? 0 : plan_of(n, dim, c, nullptr).bytes;
}

int n2v_logreg_scores(const float *X, int64_t n, int32_t dim, const float *W, const float *b, int32_t c,
                      float *scores_out, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!sizes_ok(n, dim, c)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const Plan p = plan_of(n, dim, c, workspace);
  if (!X || !W || !b || !scores_out || !workspace_ok(workspace, workspace_bytes, p.bytes)) return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  launch_pad_rows(st, W, c, p.c_pad, dim, p.wpad, nullptr);
  N2V_HIP_CHECK(hipGetLastError());
  const int64_t steps = (n + kStepRows - 1) / kStepRows;
  const unsigned blocks = (unsigned)(steps < 4096 ? steps : 4096);
  with_tile(c, vec_ok(dim, X), [&](auto G, auto VEC) {
    hipLaunchKernelGGL((scores_kernel<G, VEC>), dim3(blocks), dim3(256), 0, st, X, n, dim, p.wpad, b, c, scores_out);
  });
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

int n2v_logreg_loss_grad(const float *X, const uint32_t *y_bits, int64_t n, int32_t dim, const float *W,
                         const float *b, int32_t c, double *loss_out, double *grad_w_out, double *grad_b_out,
                         void *workspace, int64_t workspace_bytes, void *stream) {
  if (!sizes_ok(n, dim, c)) return N2V_EINVAL;
  if (n == 0) return N2V_OK;
  const Plan p = plan_of(n, dim, c, workspace);
  if (!X || !y_bits || !W || !b || !loss_out || !grad_w_out || !grad_b_out ||
      !workspace_ok(workspace, workspace_bytes, p.bytes))
    return N2V_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  launch_pad_rows(st, W, c, p.c_pad, dim, p.wpad, nullptr);
  N2V_HIP_CHECK(hipGetLastError());
  with_tile(c, vec_ok(dim, X), [&](auto G, auto VEC) {
    hipLaunchKernelGGL((loss_grad_kernel<G, VEC>), dim3((unsigned)p.slabs.n_slabs), dim3(256), 0, st, X, y_bits, n,
                       dim, p.wpad, b, c, p.GW, p.Gb, p.L, p.slabs.slab_rows);
  });
  N2V_HIP_CHECK(hipGetLastError());
  const int64_t elems = (int64_t)c * dim + c;
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, p.GW, p.Gb, p.L,
                     p.slabs.n_slabs, c, dim, grad_w_out, grad_b_out, p.Lk);
  N2V_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(1), 0, st, p.Lk, c, loss_out);
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

}  // extern "C"
