// n2v_pair_load.h -- what the kernels over a list of vertex pairs share (n2v_pairs.hip, n2v_edge_logreg.hip): the
// guarded 16-byte loads of the two rows of a pair, the layout of a wave's 64 pairs (G lanes per pair, 64 / G pairs
// side by side, U steps unrolled: eight 16-byte loads per lane in flight) and the four edge features.  Every caller
// gets the same bits from the same code (DESIGN.md "Link prediction", "Link-prediction classifier").
#pragma once

#include "n2v_dense_host.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWavePairs = 64;
constexpr int kBlockPairs = 256;  // 4 waves

// chunk c of a row: elements 4 c .. 4 c + 3; what lies at or beyond dim (or in a dead pair's row) reads as 0
template <bool VEC>
__device__ __forceinline__ f32x4 load_chunk(const float *__restrict__ row, int c, int32_t dim, bool live) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (live && 4 * c < dim) v = *reinterpret_cast<const f32x4 *>(row + 4 * c);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (live && 4 * c + j < dim) v[j] = row[4 * c + j];
  }
  return v;
}

// Row numbers of the wave's pairs, one lane per pair: -1 in both for a pair beyond the list or with an index
// outside [0, n) -- such a row is never dereferenced.
__device__ __forceinline__ void load_pair(const int64_t *__restrict__ a, const int64_t *__restrict__ b, int64_t p0,
                                          int cnt, int64_t n, int lane, int32_t &ra, int32_t &rb) {
  ra = rb = -1;
  if (lane < cnt) {
    const int64_t ia = a[p0 + lane], ib = b[p0 + lane];
    if (ia >= 0 && ia < n && ib >= 0 && ib < n) ra = (int32_t)ia, rb = (int32_t)ib;
  }
}

// pairs per step of a wave: 64 / G side by side, U steps unrolled
template <int K>
struct Unroll { static constexpr int U = K == 1 ? 4 : K == 2 ? 2 : 1; };

// The U x K chunks of both rows of this lane's pairs of the step starting at pair `base` of the wave; all
// loads are issued before any is used.  live[u]: the pair exists and both indices are rows.
template <int G, int K, bool VEC>
__device__ __forceinline__ void load_step(const float *__restrict__ X, int32_t dim, int32_t ra, int32_t rb, int base,
                                          int lane, f32x4 (&va)[Unroll<K>::U][K], f32x4 (&vb)[Unroll<K>::U][K],
                                          bool (&live)[Unroll<K>::U]) {
  constexpr int GP = 64 / G, U = Unroll<K>::U;
  const int g = lane / G, l = lane % G;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = base + u * GP + g;  // < 64: the step divides the wave's pairs
    const int32_t xa = __shfl(ra, q, 64), xb = __shfl(rb, q, 64);
    live[u] = xa >= 0;
    const float *pa = X + (int64_t)(live[u] ? xa : 0) * dim;
    const float *pb = X + (int64_t)(live[u] ? xb : 0) * dim;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      va[u][k] = load_chunk<VEC>(pa, l + k * G, dim, live[u]);
      vb[u][k] = load_chunk<VEC>(pb, l + k * G, dim, live[u]);
    }
  }
}

// one element of an edge feature: one or two correctly rounded fp32 operations (the library is built with
// -ffp-contract=off)
__device__ __forceinline__ float feature(int32_t op, float x, float y) {
  switch (op) {
    case N2V_PAIR_AVERAGE: return (x + y) * 0.5f;
    case N2V_PAIR_HADAMARD: return x * y;
    case N2V_PAIR_L1: return fabsf(x - y);
    default: { const float d = x - y; return d * d; }
  }
}

// f(G, K, VEC) as template arguments: the lane group of a dimension (G = 16 for dim <= 128, 32 for dim <= 256, 64
// beyond), K = ceil(dim / 4 G) chunks per lane, and the load path
template <typename F>
void with_shape(int32_t dim, bool vec, F &&f) {
  with_bool(vec, [&](auto v) {
    if (dim <= 64) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{}, v);
    else if (dim <= 128) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 2>{}, v);
    else if (dim <= 256) f(std::integral_constant<int, 32>{}, std::integral_constant<int, 2>{}, v);
    else if (dim <= 512) f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{}, v);
    else if (dim <= 768) f(std::integral_constant<int, 64>{}, std::integral_constant<int, 3>{}, v);
    else f(std::integral_constant<int, 64>{}, std::integral_constant<int, 4>{}, v);
  });
}

}  // namespace
