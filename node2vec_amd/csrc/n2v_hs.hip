// n2v_hs.hip -- skip-gram hierarchical-softmax SGD for gfx950 (what Spark ML's Word2Vec trains
// behind the reference's Node2VecSpark, embedding.py:182-285; the algorithm is word2vec.c's
// CreateBinaryTree + skip-gram HS, restated in tests/cpu_hs/n2v_hs_cpu.c, DESIGN.md
// "Hierarchical softmax").
//
// n2v_hs_tree_build: the Huffman tree on the host (a sequential O(V) pass; the vocabulary is
// already sorted).  Paths are stored as a CSR of int32 syn1 rows, root first, and the code bits
// as one uint64 per word, so a kernel fetches a whole path with one vector load instead of a
// chain of dependent parent-pointer loads.
//
// hs_kernel: one wave64 per sentence, lane l owns VEC elements of a row, dot products closed by
// the same DPP tree as the SGNS kernel.  All contexts of one centre position walk the same path:
// the top `cache_rows` path rows are read into LDS once per position, updated across its
// contexts, and written back once (exact: the updates are applied in the sequential order).
// Within one pair every node's dot product depends only on syn0[context] and that node's row,
// so the path is trained in groups of NB nodes whose loads and reductions are in flight
// together.  Deterministic mode (one wave) is bit-identical to the restatement; hogwild mode uses
// plain stores (atomic adds on the top inner nodes, n2v_hs_params.hot_nodes, measured slower and
// worse: the library refuses them, DESIGN.md "Hierarchical softmax").
#include <cstdlib>
#include <cstring>
#include <vector>

#include "n2v_common.h"

namespace n2v {
namespace hs {

constexpr int kWaves = 4;        // waves per block
constexpr int kExpTable = 1000;  // EXP_TABLE_SIZE
constexpr int kMaxCode = 64;     // code bits per word (one uint64)

__host__ __device__ inline uint64_t sentence_stream(uint64_t seed, uint64_t sentence_id) {
  return mix64(seed ^ mix64(sentence_id + 0xA0761D6478BD642FULL));
}
__host__ __device__ inline uint64_t hs_draw(uint64_t hs, uint64_t idx) {
  return mix64(hs + (idx + 1ULL) * 0xE7037ED1A0B428DBULL);
}

template <int VEC>
struct Row {
  float v[VEC];
};

// Agent-scope accesses for rows of up to 128 floats (the XCDs' L2s are not coherent; the same
// rule and measurements as row_ld1 in n2v_sgns_rows.h).  Wider rows stay plain.
__device__ __forceinline__ float ld1(const float *p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned int *>(p), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st1(float *p, float x) {
  __hip_atomic_store(reinterpret_cast<unsigned int *>(p), __float_as_uint(x), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

template <int VEC>
__device__ __forceinline__ void load_row(const float *base, int dim, int lane, bool full, Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      r.v[0] = ld1(base + lane);
    } else if constexpr (VEC == 2) {
      const unsigned long long u = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(base + lane * 2),
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r.v[0] = __uint_as_float((unsigned int)u);
      r.v[1] = __uint_as_float((unsigned int)(u >> 32));
    } else {
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
      const int e = lane * VEC + v;
      r.v[v] = e < dim ? (VEC <= 2 ? ld1(base + e) : base[e]) : 0.0f;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_row(float *base, int dim, int lane, bool full, const Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      st1(base + lane, r.v[0]);
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
      const int e = lane * VEC + v;
      if (e < dim) {
        if (VEC <= 2)
          st1(base + e, r.v[v]);
        else
          base[e] = r.v[v];
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

template <int kCtrl>
__device__ __forceinline__ float dpp_move(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xF, 0xF, true));
}

// The SGNS kernel's wave dot product (n2v_sgns.hip wave_dot): per-lane fmaf chain, then lane
// distances 1, 2, 4, 8 by DPP and the four row sums as (R0 + R1) + (R2 + R3).  Independent calls
// on different rows are interleaved by the compiler (several reductions per DPP chain).
template <int VEC>
__device__ __forceinline__ float wave_dot(const Row<VEC> &a, const Row<VEC> &b) {
  float acc = 0.0f;
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc = __fmaf_rn(a.v[v], b.v[v], acc);
  acc = acc + dpp_move<0xB1>(acc);
  acc = acc + dpp_move<0x4E>(acc);
  acc = acc + dpp_move<0x141>(acc);
  acc = acc + dpp_move<0x140>(acc);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 48));
  return (r0 + r1) + (r2 + r3);
}

// path nodes trained together per group: 16 floats of rows per lane, and at least two nodes, so that
// the loads of a group are issued together.  (syn1 is not restrict: the store of a group's last
// uncached row precedes the loads of the next group, so groups are dependent round trips.)
template <int VEC>
constexpr int group_nodes() {
  return VEC >= 16 ? 2 : (16 / VEC > 8 ? 8 : 16 / VEC);
}

template <int VEC>
__global__ __launch_bounds__(kWaves * 64) void hs_kernel(
    const int32_t *__restrict__ walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1,
    const int64_t *__restrict__ path_off, const int32_t *__restrict__ points,
    const uint64_t *__restrict__ codes, const float *__restrict__ exp_table_g, n2v_hs_params P,
    unsigned long long *pairs_out, int32_t sent_cap, int32_t cache_rows) {
  constexpr int NB = group_nodes<VEC>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *exp_lds = reinterpret_cast<float *>(smem);
  const int hogwild = P.deterministic ? 0 : 1;
  const int row_floats = 64 * VEC;
  // per wave: sent[sent_cap], red[sent_cap], then cache_rows current rows (+ as loaded, hogwild)
  const int per_wave = 2 * sent_cap + cache_rows * row_floats * (1 + hogwild);
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  int32_t *sent = reinterpret_cast<int32_t *>(smem + kExpTable * sizeof(float)) + wave_in_block * per_wave;
  int32_t *red = sent + sent_cap;
  float *cache = reinterpret_cast<float *>(red + sent_cap);  // [cache_rows][64 * VEC], lane-owned
  float *orig = cache + cache_rows * row_floats;             // hogwild: the rows as loaded
  for (int i = threadIdx.x; i < kExpTable; i += blockDim.x) exp_lds[i] = exp_table_g[i];
  __syncthreads();

  const int dim = P.dim, window = P.window;
  const int64_t V = P.n_vocab;
  const bool full = dim == 64 * VEC;
  // hogwild only: syn1 rows [hot_lo, V - 1) -- the top hot_nodes inner nodes -- take atomic adds
  const int64_t hot_lo = hogwild ? (V - 1) - (int64_t)P.hot_nodes : (int64_t)1 << 62;
  float alpha = P.alpha;
  const int waves_per_block = blockDim.x >> 6;
  unsigned long long pairs = 0;
  const bool dynamic = pairs_out != nullptr;
  unsigned int *row_counter = reinterpret_cast<unsigned int *>(pairs_out + 1);
  int64_t rr = (int64_t)blockIdx.x * waves_per_block + wave_in_block;
  const int64_t n_waves = (int64_t)gridDim.x * waves_per_block;
  auto lds_row = [&](float *base, int slot) { return base + slot * row_floats + lane * VEC; };

  for (;;) {
    if (dynamic) {
      unsigned int t = 0;
      if (lane == 0) t = atomicAdd(row_counter, 1u);
      rr = (int64_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)t);
    }
    if (rr >= n_walks) break;
    const int64_t r = readfirstlane_i64(rr);
    if (!dynamic) rr += n_waves;
    const uint64_t hsd = sentence_stream(P.seed, (uint64_t)(P.sentence_base + r));
    if (P.row_alpha) alpha = P.row_alpha[r];
    // ---- sentence: in-vocabulary tokens in order, a reduced window per kept position ----
    int nf = 0;
    for (int base = 0; base < walk_len; base += 64) {
      const int t = base + lane;
      const int32_t tok = t < walk_len ? walks[r * walk_len + t] : -1;
      const bool keep = tok >= 0 && (int64_t)tok < V;
      const uint64_t mask = ballot64(keep);
      const int pos = nf + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep) {
        sent[pos] = tok;
        red[pos] = (int32_t)((uint32_t)(hs_draw(hsd, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
      }
      nf += __popcll(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (int i = 0; i < nf; ++i) {
      const int32_t centre = __builtin_amdgcn_readfirstlane(sent[i]);
      const int b = __builtin_amdgcn_readfirstlane(red[i]);
      const int lo = max(0, i - window + b);
      const int hi = min(nf, i + window + 1 - b);
      const int64_t o = readfirstlane_i64(path_off[centre]);
      const int len = __builtin_amdgcn_readfirstlane((int)(path_off[centre + 1] - o));
      const uint64_t code = readfirstlane_u64(codes[centre]);
      // the whole path in one load: lane d holds point d (len <= 64)
      const int32_t my_point = lane < len ? points[o + lane] : 0;
      const int nc = min(len, cache_rows);
      // ---- the top nc path rows into LDS, once per position ----
      for (int d = 0; d < nc; ++d) {
        const int32_t p = __builtin_amdgcn_readlane(my_point, d);
        Row<VEC> t;
        load_row<VEC>(syn1 + (int64_t)p * dim, dim, lane, full, t);
        float *q = lds_row(cache, d);
#pragma unroll
        for (int v = 0; v < VEC; ++v) q[v] = t.v[v];
        if (hogwild) {
          float *q0 = lds_row(orig, d);
#pragma unroll
          for (int v = 0; v < VEC; ++v) q0[v] = t.v[v];
        }
      }
      for (int j = lo; j < hi; ++j) {
        if (j == i) continue;
        ++pairs;
        if (len == 0) continue;
        // the context row is read here, after the previous pair's write-back: a context word
        // repeated inside the window sees its own update
        float *p0 = syn0 + (int64_t)__builtin_amdgcn_readfirstlane(sent[j]) * dim;
        Row<VEC> x, neu;
        load_row<VEC>(p0, dim, lane, full, x);
#pragma unroll
        for (int v = 0; v < VEC; ++v) neu.v[v] = 0.0f;
        for (int d0 = 0; d0 < len; d0 += NB) {
          Row<VEC> rows[NB];
          int32_t pt[NB];
          float f[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const int d = d0 + k;
            pt[k] = __builtin_amdgcn_readlane(my_point, d < len ? d : 0);
            if (d < len) {
              if (d < nc) {
                const float *q = lds_row(cache, d);
#pragma unroll
                for (int v = 0; v < VEC; ++v) rows[k].v[v] = q[v];
              } else {
                load_row<VEC>(syn1 + (int64_t)pt[k] * dim, dim, lane, full, rows[k]);
              }
            }
          }
#pragma unroll
          for (int k = 0; k < NB; ++k) f[k] = d0 + k < len ? wave_dot<VEC>(x, rows[k]) : 0.0f;
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const int d = d0 + k;
            if (d >= len) break;
            if (f[k] <= -6.0f || f[k] >= 6.0f) continue;
            const int bit = (int)((code >> d) & 1ull);
            const float g = ((float)(1 - bit) - exp_lds[(int)((f[k] + 6.0f) * 83.0f)]) * alpha;
            Row<VEC> delta;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              neu.v[v] = __fmaf_rn(g, rows[k].v[v], neu.v[v]);
              delta.v[v] = g * x.v[v];
              rows[k].v[v] = __fmaf_rn(g, x.v[v], rows[k].v[v]);
            }
            if (d < nc) {
              float *q = lds_row(cache, d);
#pragma unroll
              for (int v = 0; v < VEC; ++v) q[v] = rows[k].v[v];
            } else if ((int64_t)pt[k] >= hot_lo) {
              add_row<VEC>(syn1 + (int64_t)pt[k] * dim, dim, lane, delta);
            } else {
              store_row<VEC>(syn1 + (int64_t)pt[k] * dim, dim, lane, full, rows[k]);
            }
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) x.v[v] = x.v[v] + neu.v[v];
        store_row<VEC>(p0, dim, lane, full, x);
      }
      // ---- write the cached path rows back, once per position ----
      for (int d = 0; d < nc; ++d) {
        const int32_t p = __builtin_amdgcn_readlane(my_point, d);
        Row<VEC> t;
        const float *q = lds_row(cache, d);
#pragma unroll
        for (int v = 0; v < VEC; ++v) t.v[v] = q[v];
        float *dst = syn1 + (int64_t)p * dim;
        if ((int64_t)p >= hot_lo) {
          const float *q0 = lds_row(orig, d);
#pragma unroll
          for (int v = 0; v < VEC; ++v) t.v[v] = t.v[v] - q0[v];
          add_row<VEC>(dst, dim, lane, t);
        } else {
          store_row<VEC>(dst, dim, lane, full, t);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (pairs_out && lane == 0 && pairs) atomicAdd(pairs_out, pairs);
}

}  // namespace hs
}  // namespace n2v

extern "C" int n2v_hs_tree_build(const int64_t *counts, int64_t n_vocab, int64_t *path_off_out,
                                 uint64_t *codes_out, int32_t *points_out, int64_t points_capacity) {
  if (!counts || !path_off_out || !codes_out || n_vocab < 1 || n_vocab >= (1ll << 31)) return N2V_EINVAL;
  const int64_t V = n_vocab;
  int64_t total = 0;
  for (int64_t a = 0; a < V; ++a) {
    if (counts[a] < 0 || (a > 0 && counts[a] > counts[a - 1])) return N2V_EINVAL;  // descending
    if (counts[a] > (INT64_MAX / 4) - total) return N2V_EINVAL;                     // sums stay below the sentinel
    total += counts[a];
  }
  // word2vec.c CreateBinaryTree: two queues, pos1 descending over the leaves, pos2 ascending over
  // the merged nodes; strict `<`, so a tie takes the merged node; binary[min2i] = 1
  std::vector<int64_t> count((size_t)(2 * V + 1));
  std::vector<int64_t> parent((size_t)(2 * V), 0);
  std::vector<uint8_t> binary((size_t)(2 * V), 0);
  for (int64_t a = 0; a < V; ++a) count[a] = counts[a];
  for (int64_t a = V; a < 2 * V + 1; ++a) count[a] = INT64_MAX;  // unmerged slot: above any sum
  int64_t pos1 = V - 1, pos2 = V;
  for (int64_t a = 0; a < V - 1; ++a) {
    int64_t m1, m2;
    if (pos1 >= 0 && count[pos1] < count[pos2]) m1 = pos1--; else m1 = pos2++;
    if (pos1 >= 0 && count[pos1] < count[pos2]) m2 = pos1--; else m2 = pos2++;
    count[V + a] = count[m1] + count[m2];
    parent[m1] = V + a;
    parent[m2] = V + a;
    binary[m2] = 1;
  }
  // depth and code prefix top-down: a node's parent is created after it, so descending node
  // numbers visit parents first.  Root 2V - 2 has depth 0.
  std::vector<uint8_t> depth((size_t)(2 * V - 1), 0);
  std::vector<uint64_t> prefix((size_t)(2 * V - 1), 0);
  for (int64_t x = 2 * V - 3; x >= 0; --x) {
    const int64_t p = parent[x];
    const int dp = depth[p];
    if (dp >= n2v::hs::kMaxCode) return N2V_EINVAL;  // a code longer than 64 bits
    depth[x] = (uint8_t)(dp + 1);
    prefix[x] = prefix[p] | ((uint64_t)binary[x] << dp);
  }
  path_off_out[0] = 0;
  for (int64_t w = 0; w < V; ++w) {
    const int len = V > 1 ? depth[w] : 0;
    path_off_out[w + 1] = path_off_out[w] + len;
    codes_out[w] = V > 1 ? prefix[w] : 0;
  }
  if (!points_out) return N2V_OK;
  if (points_capacity < path_off_out[V]) return N2V_EINVAL;
  // points root first: walk up from the leaf, filling from the end; inner node V + a is syn1 row a
  for (int64_t w = 0; w < V; ++w) {
    int64_t d = path_off_out[w + 1] - path_off_out[w];
    int64_t b = w;
    while (d > 0) {
      b = parent[b];
      points_out[path_off_out[w] + --d] = (int32_t)(b - V);
    }
  }
  return N2V_OK;
}

namespace {
// The LDS path cache of a hogwild wave: bytes for its rows, both copies (deterministic mode runs one
// wave and takes four times as many rows).  Not tuned by measurement: the budget keeps a block of 4
// waves at ~44 KB of LDS (3 blocks = 12 waves per CU) and caches the top 16 / 8 / 4 / 2 / 1 levels at
// VEC 1 / 2 / 4 / 8 / 16; the levels below are read and written per pair.
constexpr int kCacheBytesPerWave = 8192;

int hs_cache_rows(const n2v_hs_params *P, int vec) {
  if (!P->path_cache) return 0;
  int rows = P->deterministic ? 4 * kCacheBytesPerWave / (256 * vec) : kCacheBytesPerWave / (2 * 256 * vec);
  return rows > 64 ? 64 : rows;
}

int hs_train_impl(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1,
                  const int64_t *path_off, const int32_t *points, const uint64_t *codes, const float *exp_table,
                  const n2v_hs_params *P, unsigned long long *pairs_out, void *stream, int64_t *dry_waves) {
  if (!P) return N2V_EINVAL;
  if (!dry_waves && (!walks || !syn0 || !syn1 || !path_off || !points || !codes || !exp_table)) return N2V_EINVAL;
  if (n_walks < 0 || walk_len < 1 || walk_len > N2V_SGNS_MAX_SENTENCE) return N2V_EINVAL;
  if (P->n_vocab < 1 || P->n_vocab >= (1ll << 31) || P->dim < 1 || P->dim > 1024 || P->window < 1 ||
      P->window > 32)
    return N2V_EINVAL;
  if (P->deterministic != 0 && P->deterministic != 1) return N2V_EINVAL;
  if (P->path_cache != 0 && P->path_cache != 1) return N2V_EINVAL;
  // hot_nodes > 0 (atomic adds on the top inner nodes) measured slower and worse than plain stores, and
  // its atomic write-backs are not read back consistently by the same wave: refused
  if (P->hot_nodes != 0 || P->max_waves < 0) return N2V_EINVAL;
  if (dry_waves) *dry_waves = 0;
  if (n_walks == 0) return N2V_OK;
  using namespace n2v;
  using namespace n2v::hs;
  int vec = 1;
  while (64 * vec < P->dim) vec *= 2;
  const int cache_rows = hs_cache_rows(P, vec);
  const int sent_cap = (walk_len + 3) & ~3;
  const size_t per_wave = (size_t)2 * sent_cap + (size_t)cache_rows * 64 * vec * (P->deterministic ? 1 : 2);
  const size_t lds = kExpTable * sizeof(float) + (size_t)(P->deterministic ? 1 : kWaves) * per_wave * 4;
  // hogwild concurrency: one wave per 32 vocabulary rows, up to the whole chip (the SGNS rule)
  int64_t waves = P->n_vocab / 32;
  if (waves < 1) waves = 1;
  if (waves > n_walks) waves = n_walks;
  if (P->max_waves > 0 && waves > P->max_waves) waves = P->max_waves;
  int64_t blocks = (waves + kWaves - 1) / kWaves;
  dim3 block(kWaves * 64);
  if (waves < kWaves) block = dim3((unsigned)waves * 64);
  if (P->deterministic) {
    blocks = 1;
    block = dim3(64);
  }
  hipStream_t st = (hipStream_t)stream;
  if (!dry_waves && pairs_out && hipMemsetAsync(pairs_out + 1, 0, sizeof(unsigned long long), st) != hipSuccess)
    return N2V_ELAUNCH;
#define N2V_HS_LAUNCH(VV)                                                                              \
  do {                                                                                                 \
    const void *fn = (const void *)hs_kernel<VV>;                                                      \
    if (lds > 64 * 1024 &&                                                                             \
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)   \
      return N2V_ELAUNCH;                                                                              \
    if (!P->deterministic) {                                                                           \
      const int64_t cap = resident_blocks(fn, (int)block.x, lds);                                      \
      if (blocks > cap) blocks = cap;                                                                  \
    }                                                                                                  \
    if (dry_waves) {                                                                                   \
      *dry_waves = blocks * (int64_t)(block.x / 64);                                                   \
      break;                                                                                           \
    }                                                                                                  \
    hipLaunchKernelGGL((hs_kernel<VV>), dim3((unsigned)blocks), block, lds, st, walks, n_walks, walk_len, \
                       syn0, syn1, path_off, points, codes, exp_table, *P, pairs_out, sent_cap, cache_rows); \
  } while (0)
  switch (vec) {
    case 1: N2V_HS_LAUNCH(1); break;
    case 2: N2V_HS_LAUNCH(2); break;
    case 4: N2V_HS_LAUNCH(4); break;
    case 8: N2V_HS_LAUNCH(8); break;
    default: N2V_HS_LAUNCH(16); break;
  }
#undef N2V_HS_LAUNCH
  if (dry_waves) return N2V_OK;
  N2V_HIP_CHECK(hipGetLastError());
  return N2V_OK;
}
}  // namespace

extern "C" int n2v_hs_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1,
                            const int64_t *path_off, const int32_t *points, const uint64_t *codes,
                            const float *exp_table, const n2v_hs_params *P, unsigned long long *pairs_out,
                            void *stream) {
  return hs_train_impl(walks, n_walks, walk_len, syn0, syn1, path_off, points, codes, exp_table, P, pairs_out,
                       stream, nullptr);
}

extern "C" int64_t n2v_hs_hogwild_waves(const n2v_hs_params *P, int64_t n_walks, int32_t walk_len) {
  int64_t waves = 0;
  const int rc = hs_train_impl(nullptr, n_walks, walk_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, P,
                               nullptr, nullptr, &waves);
  return rc == N2V_OK ? waves : (int64_t)rc;
}
