// n2v_score_tile.h -- the fixed-order fp32 pieces n2v_knn.hip, n2v_ivf.hip, n2v_kmeans.hip and n2v_logreg.hip share:
// the sum of squares of a row (wave_sumsq), 1 / sqrt or 0, the 16 x 16 MFMA dot chain (score_rows, and score_tile
// over contiguous operands) and the kernel that pads its operand B (pad_rows_kernel).  Every caller gets the same
// bits from the same code (DESIGN.md "Nearest neighbours", "Clustering", "Node classification"); what surrounds the
// kernels on the host is n2v_dense_host.h.
#pragma once

#include "n2v_dense_host.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows of the padded operand matrix [rows_pad][dim_pad] are dim_pad floats long (zeros in the padding)
__host__ __device__ inline int32_t dim_pad_of(int32_t dim) { return (int32_t)round_up(dim, 16); }

// sum of squares of v[0..dim) in one fixed order: lane l sums d = l, l + 64, ... by fmaf, then a fixed
// butterfly; the whole wave calls it
__device__ inline float wave_sumsq(const float *__restrict__ v, int32_t dim, int lane) {
  float s = 0.f;
  for (int d = lane; d < dim; d += 64) s = __fmaf_rn(v[d], v[d], s);
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  return s;
}

__device__ inline float inv_sqrt_or_zero(float s) { return s > 0.f ? 1.f / sqrtf(s) : 0.f; }

// The rows of src[n_rows][dim] padded with zeros to dst[rows_pad][dim_pad], score_tile's operand B, and with
// `sumsq` (may be null) wave_sumsq of every row, 0 for a padding row; one wave per padded row.  (Kernel and
// launcher are templates so that only the files that launch it carry the kernel.)
template <typename = void>
__global__ __launch_bounds__(256) void pad_rows_kernel(const float *__restrict__ src, int32_t n_rows,
                                                       int64_t rows_pad, int32_t dim, float *__restrict__ dst,
                                                       float *__restrict__ sumsq) {
  const int lane = threadIdx.x & 63;
  const int32_t dp = dim_pad_of(dim);
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows_pad) return;
  const bool live = r < n_rows;
  const float *v = src + (live ? r : 0) * dim;
  for (int d = lane; d < dp; d += 64) dst[r * dp + d] = (live && d < dim) ? v[d] : 0.f;
  if (!sumsq) return;
  const float s = wave_sumsq(v, dim, lane);
  if (lane == 0) sumsq[r] = live ? s : 0.f;
}

template <typename T = void>
void launch_pad_rows(hipStream_t st, const float *src, int32_t n_rows, int64_t rows_pad, int32_t dim,
                            float *dst, float *sumsq) {
  hipLaunchKernelGGL(pad_rows_kernel<T>, dim3((unsigned)((rows_pad + 3) / 4)), dim3(256), 0, st, src, n_rows, rows_pad,
                     dim, dst, sumsq);
}

// Dot products of 16 rows with G groups of 16 queries, one wave: acc[g][i] is dot(query 16 g + (lane & 15),
// row 4 (lane >> 4) + i of the tile).  The X tile is operand A (lane l: row l & 15, k = l >> 4), q_hat operand B
// (query l & 15, k = l >> 4); a lane loads d0 + 4 k .. + 3 and feeds them to four MFMAs, so d is summed in the
// order d0 + 4 k + j over (d0, j, k) -- fixed.  Both sides are given per lane, so either may be gathered: `xr`
// the lane's row of X (read as 0 when not `live`, and at dims at or beyond `dim`; it must still be a readable
// address), qrow[g] the padded q_hat row (dim_pad floats, 16-byte aligned) of the lane's query in group g.
template <int G, bool VEC>
__device__ inline void score_rows(const float *__restrict__ xr, bool live, int32_t dim,
                                  const float *(&qrow)[G], int lane, f32x4 (&acc)[G]) {
  const int32_t dp = dim_pad_of(dim);
  const int k4 = 4 * (lane >> 4);
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int kBatch = 8;  // X loads in flight per lane: 8 x 16 B
  for (int db = 0; db < dp; db += 16 * kBatch) {
    f32x4 xa[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int d = db + 16 * b + k4;
      if (VEC) {
        xa[b] = (live && d < dim) ? *reinterpret_cast<const f32x4 *>(xr + d) : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[b][j] = (live && d + j < dim) ? xr[d + j] : 0.f;
      }
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int d0 = db + 16 * b;
      if (d0 >= dp) break;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const f32x4 q4 = *reinterpret_cast<const f32x4 *>(qrow[g] + k4 + d0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].x, q4.x, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].y, q4.y, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].z, q4.z, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].w, q4.w, acc[g], 0, 0, 0);
      }
    }
  }
}

// score_rows over a contiguous run of rows (row0 .., rows at or beyond `row_end` read as 0) and a contiguous
// q_hat tile [16 G][dim_pad]: acc[g][i] is dot(q_hat[16 g + (lane & 15)], x[row0 + 4 (lane >> 4) + i]).
template <int G, bool VEC>
__device__ inline void score_tile(const float *__restrict__ X, int32_t dim, int64_t row0, int64_t row_end,
                                  const float *__restrict__ qhat_tile, int lane, f32x4 (&acc)[G]) {
  const int32_t dp = dim_pad_of(dim);
  const int64_t row = row0 + (lane & 15);
  const bool live = row < row_end;
  const float *qrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) qrow[g] = qhat_tile + (int64_t)(16 * g + (lane & 15)) * dp;
  score_rows<G, VEC>(X + (live ? row : 0) * (int64_t)dim, live, dim, qrow, lane, acc);
}

}  // namespace
