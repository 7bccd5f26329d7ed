// n2v_w2v_core.h -- what the four word2vec trainers share (DESIGN.md "The trainers' shared core").
// Device side: the counter-based draws of a sentence, rows across a wave (lane l owns elements
// l*VEC .. l*VEC+VEC-1: loads, stores, atomic adds, the wave64 dot product), the row
// counter and the bisects over the cumulative table.  Host side: the common parameter checks,
// the hogwild launch geometry and the launch itself.  Included by n2v_sgns.hip (skip-gram), n2v_cbow.hip
// (CBOW), n2v_hs.hip (hierarchical softmax) and n2v_sgns_batched.hip (batched skip-gram, which keeps its
// own row tiles): one definition, so that all are pinned to the same streams and summation order.
#pragma once

#include <type_traits>

#include "n2v_common.h"

namespace n2v {

constexpr int kSgnsWaves = 4;      // waves per block
constexpr int kExpTable = 1000;    // EXP_TABLE_SIZE
constexpr int kBuckets = 1024;     // coarse index of cum_table: bucket b covers values [b<<21, (b+1)<<21)

__host__ __device__ inline uint64_t sentence_stream(uint64_t seed, uint64_t sentence_id) {
  return mix64(seed ^ mix64(sentence_id + 0xA0761D6478BD642FULL));
}
__host__ __device__ inline uint64_t sentence_draw(uint64_t hs, uint64_t idx) {
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

// kWideRaggedPlain: how a ragged row (dim != 64 * VEC) of more than 128 floats (VEC > 2) is accessed, element
// by element.  false (skip-gram, CBOW): agent-scope, like the narrow rows -- CBOW relies on it to read hub
// rows of wide models past a stale L1 line (its full_at).  true (HS): plain, like the 16-byte accesses of a
// full wide row.  HS was written with the plain form and has no atomically updated rows to read back (it
// refuses hot_nodes); the two forms were never measured against each other there, so the difference is
// inherited, not chosen.
template <int VEC, bool kWideRaggedPlain = false>
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
      r.v[v] = e < dim ? ((kWideRaggedPlain && VEC > 2) ? base[e] : row_ld1(base + e)) : 0.0f;
    }
  }
}

template <int VEC, bool kWideRaggedPlain = false>
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
      if (e < dim) {
        if (kWideRaggedPlain && VEC > 2)
          base[e] = r.v[v];
        else
          row_st1(base + e, r.v[v]);
      }
    }
  }
}

// no-return f32 atomic add of a lane's elements (global_atomic_add_f32)
template <int VEC>
__device__ __forceinline__ void add_row(float *base, int dim, int lane, const Row<VEC> &d) {
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (lane * VEC + v < dim) unsafeAtomicAdd(base + lane * VEC + v, d.v[v]);
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
// Independent calls on different rows are interleaved by the compiler (several reductions
// per DPP chain).
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

// ---- the row loop: which sentence a wave trains next ----
// Rows are taken from a shared counter (pairs_out[1], reset by the launcher) rather than by a fixed
// stride: a few per cent of tail at dim 128-256; a single wave (deterministic mode) still sees them in
// order.  The counter is 32 bits wide, so every kernel takes this path only for n_walks < 0xfffffff0 (and
// with pairs_out) and deals rows by stride otherwise.  Returns the claimed row, wave-uniform.
__device__ __forceinline__ int64_t claim_row(unsigned int *counter, int lane) {
  unsigned int t = 0;
  if (lane == 0) t = atomicAdd(counter, 1u);
  return (int64_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)t);
}

// ---- negative draws: bisect_left over the cumulative count^0.75 table ----
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
// bisect_left confined to [lo, hi], by one lane (data-dependent trip count)
__device__ __forceinline__ int bisect_range_u32(const uint32_t *a, int lo, int hi, uint32_t x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// bucket[b] = bisect_left(cum_table, b << 21), b = 0 .. kBuckets, by the whole block: a draw x lies in
// bucket x >> 21 and its bisect_left is confined to [bucket[b], bucket[b + 1]] -- same index, half the
// probes.  Only needed (and only allocated) without the caller's fine index (n2v_sgns_params.cum_index).
__device__ __forceinline__ void bucket_table_build(int32_t *bucket, const uint32_t *cum_table, int64_t n_vocab) {
  const int bis_iters = 64 - __clzll((long long)n_vocab);
  for (int b = threadIdx.x; b <= kBuckets; b += blockDim.x)
    bucket[b] = bisect_left_u32(cum_table, n_vocab, (uint32_t)b << 21, bis_iters);
}

// ---- host side: what every trainer's launcher checks, derives and does ----
// the parameter ranges all four share (tokens are int32: a vocabulary of 2^31 words cannot be named)
inline bool check_common(int64_t n_vocab, int dim, int window, int64_t n_walks, int32_t walk_len) {
  return n_walks >= 0 && walk_len >= 1 && walk_len <= N2V_SGNS_MAX_SENTENCE && n_vocab >= 1 &&
         n_vocab < (1ll << 31) && dim >= 1 && dim <= 1024 && window >= 1 && window <= 32;
}
// floats per lane of a row across the wave: the power of two with 64 * VEC >= dim
inline int vec_of(int dim) {
  int vec = 1;
  while (64 * vec < dim) vec *= 2;
  return vec;
}
inline int sent_cap_of(int32_t walk_len) { return (walk_len + 3) & ~3; }

// Hogwild concurrency is scaled to the model: unsynchronised waves are harmless while collisions on a
// row are rare (gensim runs <= 16 threads); on a tiny vocabulary thousands of racing waves would
// overwrite each other's updates.  One wave per 32 vocabulary rows, up to the whole chip (8192 waves >=
// 256 K rows), at most one per sentence and at most max_waves (> 0); fewer waves than a block holds run
// as one smaller block; deterministic mode is one wave.
struct LaunchGeometry {
  int64_t blocks;
  int block_threads;
};
inline LaunchGeometry hogwild_geometry(int64_t n_vocab, int64_t n_walks, int64_t max_waves, bool deterministic,
                                       int waves_per_block) {
  int64_t waves = n_vocab / 32;
  if (waves < 1) waves = 1;
  if (waves > n_walks) waves = n_walks;
  if (max_waves > 0 && waves > max_waves) waves = max_waves;
  if (deterministic) return {1, 64};
  if (waves < waves_per_block) return {1, (int)waves * 64};
  return {(waves + waves_per_block - 1) / waves_per_block, waves_per_block * 64};
}

// Launches `kernel` on geometry `g` with `lds` bytes of dynamic LDS, or (dry_waves != NULL) launches
// nothing and writes the waves the launch would keep in flight.  Above 64 KB the dynamic-LDS limit of the
// kernel is raised first (the skip-gram ring, the HS path cache, the batched tiles; CBOW's LDS never
// exceeds ~17 KB at walk_len <= 256, so the condition is never true there).  Unless deterministic, the
// blocks are capped by those resident at once.  pairs_out[1] is the kernels' row counter (claim_row):
// it is started at zero on the same stream.  `args` are the kernel's arguments, converted to its
// parameter types.
template <typename... KArgs>
inline int launch_trainer(void (*kernel)(KArgs...), LaunchGeometry g, size_t lds, bool deterministic,
                          unsigned long long *pairs_out, void *stream, int64_t *dry_waves,
                          std::common_type_t<KArgs>... args) {
  const void *fn = (const void *)kernel;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return N2V_ELAUNCH;
  if (!deterministic) {
    const int64_t cap = resident_blocks(fn, g.block_threads, lds);
    if (g.blocks > cap) g.blocks = cap;
  }
  if (dry_waves) {
    *dry_waves = g.blocks * (int64_t)(g.block_threads / 64);
    return N2V_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  if (pairs_out && hipMemsetAsync(pairs_out + 1, 0, sizeof(unsigned long long), st) != hipSuccess)
    return N2V_ELAUNCH;
  void *argv[] = {(void *)&args...};
  N2V_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)g.blocks), dim3((unsigned)g.block_threads), argv, lds, st));
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}

// the batched skip-gram trainer (n2v_sgns_batched.hip), checked and launched for n2v_sgns_train (n2v_sgns.hip) when
// P->batched is set; dry_waves as launch_trainer's
int launch_sgns_batched(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1neg,
                        const uint32_t *cum_table, const uint32_t *sample_int, const float *exp_table,
                        const n2v_sgns_params *P, unsigned long long *pairs_out, void *stream, int64_t *dry_waves);

}  // namespace n2v
