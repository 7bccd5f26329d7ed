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
// the DPP tree of wave_dot (n2v_w2v_core.h).  All contexts of one centre position walk the same path:
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
#include "n2v_w2v_core.h"

namespace n2v {
namespace hs {

constexpr int kWaves = 4;        // waves per block
constexpr int kMaxCode = 64;     // code bits per word (one uint64)

// ragged rows of more than 128 floats are accessed plainly here (load_row in n2v_w2v_core.h)
constexpr bool kWideRaggedPlain = true;

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
  unsigned long long pairs = 0;
  auto lds_row = [&](float *base, int slot) { return base + slot * row_floats + lane * VEC; };

  const int waves_per_block = blockDim.x >> 6;
  const bool dynamic = pairs_out != nullptr && n_walks < 0xfffffff0ll;
  unsigned int *row_counter = reinterpret_cast<unsigned int *>(pairs_out + 1);
  int64_t rr = (int64_t)blockIdx.x * waves_per_block + wave_in_block;
  const int64_t n_waves = (int64_t)gridDim.x * waves_per_block;
  for (;;) {
    if (dynamic) rr = claim_row(row_counter, lane);
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
        red[pos] = (int32_t)((uint32_t)(sentence_draw(hsd, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
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
        load_row<VEC, kWideRaggedPlain>(syn1 + (int64_t)p * dim, dim, lane, full, t);
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
        load_row<VEC, kWideRaggedPlain>(p0, dim, lane, full, x);
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
                load_row<VEC, kWideRaggedPlain>(syn1 + (int64_t)pt[k] * dim, dim, lane, full, rows[k]);
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
              store_row<VEC, kWideRaggedPlain>(syn1 + (int64_t)pt[k] * dim, dim, lane, full, rows[k]);
            }
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) x.v[v] = x.v[v] + neu.v[v];
        store_row<VEC, kWideRaggedPlain>(p0, dim, lane, full, x);
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
          store_row<VEC, kWideRaggedPlain>(dst, dim, lane, full, t);
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
  if (!n2v::check_common(P->n_vocab, P->dim, P->window, n_walks, walk_len)) return N2V_EINVAL;
  if (P->deterministic != 0 && P->deterministic != 1) return N2V_EINVAL;
  if (P->path_cache != 0 && P->path_cache != 1) return N2V_EINVAL;
  // hot_nodes > 0 (atomic adds on the top inner nodes) measured slower and worse than plain stores, and
  // its atomic write-backs are not read back consistently by the same wave: refused
  if (P->hot_nodes != 0 || P->max_waves < 0) return N2V_EINVAL;
  if (dry_waves) *dry_waves = 0;
  if (n_walks == 0) return N2V_OK;
  using namespace n2v;
  using namespace n2v::hs;
  const int vec = vec_of(P->dim);
  const int cache_rows = hs_cache_rows(P, vec);
  const int sent_cap = sent_cap_of(walk_len);
  const size_t per_wave = (size_t)2 * sent_cap + (size_t)cache_rows * 64 * vec * (P->deterministic ? 1 : 2);
  const size_t lds = kExpTable * sizeof(float) + (size_t)(P->deterministic ? 1 : kWaves) * per_wave * 4;
  const LaunchGeometry geo = hogwild_geometry(P->n_vocab, n_walks, P->max_waves, P->deterministic, kWaves);
  auto launch = [&](auto kernel) {
    return launch_trainer(kernel, geo, lds, P->deterministic, pairs_out, stream, dry_waves, walks, n_walks, walk_len,
                          syn0, syn1, path_off, points, codes, exp_table, *P, pairs_out, sent_cap, cache_rows);
  };
  switch (vec) {
    case 1: return launch(hs_kernel<1>);
    case 2: return launch(hs_kernel<2>);
    case 4: return launch(hs_kernel<4>);
    case 8: return launch(hs_kernel<8>);
    default: return launch(hs_kernel<16>);
  }
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
