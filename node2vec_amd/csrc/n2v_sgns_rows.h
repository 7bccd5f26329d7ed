// n2v_sgns_rows.h -- what the word2vec trainers that keep a row across a wave share: the counter-based
// draws of a sentence, row loads / stores (lane l owns elements l*VEC .. l*VEC+VEC-1), the wave64 dot
// product and the bisect over the cumulative table.  Included by n2v_sgns.hip (skip-gram) and
// n2v_cbow.hip (CBOW): one definition, so that both are pinned to the same summation order.
#pragma once

#include "n2v_common.h"

namespace n2v {

constexpr int kSgnsWaves = 4;      // waves per block
constexpr int kExpTable = 1000;    // EXP_TABLE_SIZE
constexpr int kBuckets = 1024;     // coarse index of cum_table: bucket b covers values [b<<21, (b+1)<<21)

__host__ __device__ inline uint64_t sentence_stream(uint64_t seed, uint64_t sentence_id) {
  return mix64(seed ^ mix64(sentence_id + 0xA0761D6478BD642FULL));
}
__host__ __device__ inline uint64_t sgns_draw(uint64_t hs, uint64_t idx) {
  return mix64(hs + (idx + 1ULL) * 0xE7037ED1A0B428DBULL);
}

template <int VEC>
struct Row {
  float v[VEC];
};

// Rows are read and written with AGENT-SCOPE (`sc1`) accesses (rounds 1 - 5 used plain
// accesses).  The XCDs' L2s are not coherent with each other and a CU's L1 is never refreshed by another
// CU's stores: with plain accesses a row trained by waves on two XCDs keeps the updates of ONE of them for as long
// as a line stays cached -- a window of micro- to milliseconds where gensim's threads on a coherent CPU race over
// nanoseconds.  Measured (round 6, profiles/r10m_sgns_coherent.log): of the rows a block of 768 sentences trains on a
// 10^7 x 128 model, 4.5 % end a whole update away from the ordered run with plain accesses, 0.95 % with these; cfg 2
// link AUC 0.8983 -> 0.9016 (hub_rows = 0) and 0.9085 -> 0.9107 (default), the rate on a 10^8 x 128 model unchanged
// (813.6 / 813.7 M pairs/s: a random 512-byte row misses every cache anyway).  Values are the same bits: the
// deterministic mode is untouched.  Rows of up to 128 floats only (4- and 8-byte accesses per lane: dim <= 128, the
// dims of BASELINE cfgs 2 - 4): the 16-byte form (buffer loads / stores with aux = sc1 through a descriptor per row)
// was built and measured too and costs 3.4 % at dim 256 and 31 % at dim 512 (profiles/r10n_sgns_coherent_rates.log),
// so wider rows keep plain accesses.
__device__ __forceinline__ float row_ld1(const float *p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned int *>(p), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void row_st1(float *p, float x) {
  __hip_atomic_store(reinterpret_cast<unsigned int *>(p), __float_as_uint(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int VEC>
__device__ __forceinline__ void load_row(const float *base, int dim, int lane, bool full,
                                         Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      r.v[0] = row_ld1(base + lane);
    } else if constexpr (VEC == 2) {
      const unsigned long long u = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(base + lane * 2),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.v[0] = __uint_as_float((unsigned int)u);
      r.v[1] = __uint_as_float((unsigned int)(u >> 32));
    } else {
      // (16-byte accesses stay plain: see above row_ld1)
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        float4 t = *reinterpret_cast<const float4 *>(base + lane * VEC + q * 4);
        r.v[4 * q + 0] = t.x;
        r.v[4 * q + 1] = t.y;
        r.v[4 * q + 2] = t.z;
        r.v[4 * q + 3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      int e = lane * VEC + v;
      r.v[v] = e < dim ? row_ld1(base + e) : 0.0f;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_row(float *base, int dim, int lane, bool full,
                                          const Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      row_st1(base + lane, r.v[0]);
    } else if constexpr (VEC == 2) {
      const unsigned long long u = (unsigned long long)__float_as_uint(r.v[0]) |
                                   ((unsigned long long)__float_as_uint(r.v[1]) << 32);
      __hip_atomic_store(reinterpret_cast<unsigned long long *>(base + lane * 2), u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q)
        *reinterpret_cast<float4 *>(base + lane * VEC + q * 4) =
            make_float4(r.v[4 * q], r.v[4 * q + 1], r.v[4 * q + 2], r.v[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      int e = lane * VEC + v;
      if (e < dim) row_st1(base + e, r.v[v]);
    }
  }
}

// one DPP step: value of the lane selected by `kCtrl` (no LDS round trip)
template <int kCtrl>
__device__ __forceinline__ float dpp_move(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xF, 0xF, true));
}

// Dot product across the wave.  Per-lane FMA chain over its VEC elements, then a balanced
// tree over adjacent lanes (butterfly distances 1, 2, 4, 8, 16, 32 -- the order the oracle
// restates).  Distances 1..8 are DPP modifiers on the adds (quad_perm, row_half_mirror,
// row_mirror: values are already uniform inside the mirrored groups, so mirror == xor);
// the four row sums are read with v_readlane and combined as (R0 + R1) + (R2 + R3).
// No LDS crossbar (ds_bpermute cost six dependent LDS round trips per dot), and the
// result is a scalar to the compiler, so the branches on it are scalar branches.
template <int VEC>
__device__ __forceinline__ float wave_dot(const Row<VEC> &a, const Row<VEC> &b) {
  float acc = 0.0f;
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc = __fmaf_rn(a.v[v], b.v[v], acc);
  acc = acc + dpp_move<0xB1>(acc);   // quad_perm [1,0,3,2]  : lane ^ 1
  acc = acc + dpp_move<0x4E>(acc);   // quad_perm [2,3,0,1]  : lane ^ 2
  acc = acc + dpp_move<0x141>(acc);  // row_half_mirror      : the other quad  (== lane ^ 4)
  acc = acc + dpp_move<0x140>(acc);  // row_mirror           : the other half-row (== lane ^ 8)
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 48));
  return (r0 + r1) + (r2 + r3);      // lane ^ 16, then lane ^ 32
}

__device__ __forceinline__ int bisect_left_u32(const uint32_t *a, int64_t n, uint32_t x,
                                               int iters) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < iters; ++it) {
    int64_t mid = (lo + hi) >> 1;
    uint32_t val = a[mid < n ? mid : n - 1];
    bool act = lo < hi;
    bool less = val < x;
    lo = (act && less) ? mid + 1 : lo;
    hi = (act && !less) ? mid : hi;
  }
  return (int)lo;
}

}  // namespace n2v
