// n2v_cbow.hip -- CBOW (sg = 0) negative-sampling SGD for gfx950.
//
// What gensim.models.Word2Vec trains at the reference's call site embedding.py:126 when the caller
// sets `negative` and leaves `sg` at gensim's default 0: gensim 3.8 train_batch_cbow +
// fast_sentence_cbow_neg, restated in tests/cpu_cbow/n2v_cbow_cpu.c (DESIGN.md "CBOW").  For
// position i of a prepared sentence (centre c, reduced window [lo, hi), count = hi - lo - 1 > 0):
//   neu1 = sum of syn0[sent[m]], m = lo .. hi - 1, m != i, ascending (a repeated word twice);
//   cbow_mean: neu1 *= 1 / count;
//   targets d = 0 .. negative: c with label 1, then the draws (one set per POSITION: draw index
//   2 * walk_len + i * negative + d - 1), a draw equal to c skipped; f = wave_dot(neu1, syn1neg[t]);
//   |f| >= 6 skipped; g = (label - EXP_TABLE[(int)((f + 6) * 83)]) * alpha;
//   work = fmaf(g, syn1neg[t], work); syn1neg[t] = fmaf(g, neu1, syn1neg[t]);
//   not cbow_mean: work *= 1 / count;  then syn0[sent[m]] += work for the same m, ascending (a
//   repeated word receives it twice).  The counter grows by one per trained position.
// Deviations from gensim, those of the skip-gram kernel: counter-based draws -- sentence_stream(seed,
// sentence id), draw 2t for subsampling and 2t + 1 for the reduced window of raw position t -- where
// gensim runs one linear congruential generator per thread; dot products summed in the wave64 order
// (lane l owns elements l*VEC .., then the butterfly over lane distances 1 .. 32) where BLAS sdot
// leaves the order open; FMAs where the skip-gram kernel spells them; the seeded initialisation.
//
// Design: one wave64 per sentence, sentence preparation a copy of sgns_kernel's.  Every row of a position is
// known before any arithmetic -- up to 2 * window context rows and 1 + negative target rows -- and the
// target rows do not depend on neu1, so the first kTG target rows are requested BEFORE the context
// rows are summed: one round trip to memory covers both.  Context rows are summed in groups of kCG
// as they land (step order kept), the dot products of a group of targets are reduced together, and
// the updates are applied in target order; only a target equal to an earlier one of the same group is
// read back after that one's store.  The negative draws of 64 / negative positions are made at once,
// lane-parallel, so the dependent probes of a bisect are paid once per ~12 positions.  The second
// pass over the context rows reads each row again and stores row + work (read-modify-write, the
// agent-scope accesses of n2v_w2v_core.h at dim <= 128); rows below hub_rows (hogwild only) take
// atomic adds of this wave's contribution instead.
#include <cstdlib>

#include "n2v_common.h"
#include "n2v_w2v_core.h"

namespace n2v {
namespace cbow {

constexpr int kWaves = 4;      // waves per block
constexpr int kNegSlots = 64;  // negative draws made at once (64 / negative positions)

// context rows summed per group / target rows in flight: registers per lane are VEC * (2 + kCG + kTG)
template <int VEC>
constexpr int ctx_group() {
  return VEC <= 2 ? 8 : (VEC == 4 ? 4 : (VEC == 8 ? 2 : 1));
}
template <int VEC>
constexpr int tgt_group() {
  return VEC <= 4 ? 6 : (VEC == 8 ? 3 : 2);
}

template <int VEC>
__global__ __launch_bounds__(kWaves * 64) void cbow_kernel(
    const int32_t *__restrict__ walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1neg,
    const uint32_t *__restrict__ cum_table, const uint32_t *__restrict__ sample_int,
    const float *__restrict__ exp_table_g, n2v_sgns_params P, int32_t cbow_mean, unsigned long long *pairs_out,
    int32_t sent_cap) {
  constexpr int kCG = ctx_group<VEC>();
  constexpr int kTG = tgt_group<VEC>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *exp_lds = reinterpret_cast<float *>(smem);
  int32_t *bucket = reinterpret_cast<int32_t *>(smem + kExpTable * sizeof(float));
  // per wave: sent[sent_cap], red[sent_cap], neg[kNegSlots]
  const int per_wave = 2 * sent_cap + kNegSlots;
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int bucket_words = P.cum_index ? 0 : (kBuckets + 1 + 3);  // + 3: 16-byte alignment
  int32_t *sent = reinterpret_cast<int32_t *>(smem + kExpTable * sizeof(float)) + bucket_words +
                  wave_in_block * per_wave;
  int32_t *red = sent + sent_cap;
  int32_t *neg = red + sent_cap;
  for (int i = threadIdx.x; i < kExpTable; i += blockDim.x) exp_lds[i] = exp_table_g[i];
  if (!P.cum_index) bucket_table_build(bucket, cum_table, P.n_vocab);
  __syncthreads();

  const int dim = P.dim, window = P.window, K = P.negative;
  // hogwild only: rows [0, hub_rows) are updated by atomic adds
  const int hub_rows = P.deterministic ? 0 : P.hub_rows;
  const bool full = dim == 64 * VEC;
  // A hub row is updated by atomic adds, which execute in L2: a later plain 16-byte load of the same
  // wave could be served from a stale L1 line, so hub rows of wide models are read element by element
  // with the agent-scope loads of the ragged path (rows of <= 128 floats are read that way anyway).
  auto full_at = [&](int32_t row) { return full && (VEC <= 2 || row >= hub_rows); };
  float alpha = P.alpha;
  const uint32_t domain = cum_table[P.n_vocab - 1];
  const int waves_per_block = blockDim.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * waves_per_block;
  const int ppb = kNegSlots / K;  // positions per batch of draws (negative <= 32: at least 2)
  unsigned long long trained = 0;

  const bool dynamic = pairs_out != nullptr && n_walks < 0xfffffff0ll;
  unsigned int *row_counter = reinterpret_cast<unsigned int *>(pairs_out + 1);
  int64_t rr = (int64_t)blockIdx.x * waves_per_block + wave_in_block;
  for (;;) {
    if (dynamic) rr = claim_row(row_counter, lane);
    if (rr >= n_walks) break;
    const int64_t r = readfirstlane_i64(rr);
    if (!dynamic) rr += n_waves;
    const uint64_t hs = sentence_stream(P.seed, (uint64_t)(P.sentence_base + r));
    if (P.row_alpha) alpha = P.row_alpha[r];
    // ---- sentence preparation: a copy of sgns_kernel's (shared as a function it changes the assembly) ----
    int nf = 0;
    for (int base = 0; base < walk_len; base += 64) {
      const int t = base + lane;
      int32_t tok = t < walk_len ? walks[r * walk_len + t] : -1;
      bool keep = tok >= 0 && (int64_t)tok < P.n_vocab;
      if (keep && sample_int) {
        uint32_t rnd = (uint32_t)(sentence_draw(hs, 2ULL * (uint64_t)t) >> 32);
        keep = !(sample_int[tok] < rnd);
      }
      const uint64_t mask = ballot64(keep);
      const int pos = nf + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep) {
        sent[pos] = tok;
        red[pos] = (int32_t)((uint32_t)(sentence_draw(hs, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
      }
      nf += __popcll(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (int i = 0; i < nf; ++i) {
      // ---- the negative draws of positions i .. i + ppb - 1, lane-parallel ----
      const int ib = i % ppb;
      if (ib == 0) {
        __builtin_amdgcn_wave_barrier();
        const int jj = lane / K, d = lane - jj * K;
        if (jj < ppb && i + jj < nf) {
          const uint64_t idx = 2ULL * (uint64_t)walk_len + (uint64_t)(i + jj) * (uint64_t)K + (uint64_t)d;
          const uint32_t x = (uint32_t)((sentence_draw(hs, idx) >> 16) % (uint64_t)domain);
          int blo, bhi;
          if (P.cum_index) {
            const uint32_t bk = x >> (31 - P.cum_index_bits);
            blo = P.cum_index[bk];
            bhi = P.cum_index[bk + 1];
          } else {
            blo = bucket[x >> 21];
            bhi = bucket[(x >> 21) + 1];
          }
          while (blo < bhi) {  // bisect_left inside the bucket
            const int mid = (blo + bhi) >> 1;
            if (cum_table[mid] < x)
              blo = mid + 1;
            else
              bhi = mid;
          }
          neg[lane] = blo;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      const int32_t centre = __builtin_amdgcn_readfirstlane(sent[i]);
      const int b = __builtin_amdgcn_readfirstlane(red[i]);
      const int lo = max(0, i - window + b);
      const int hi = min(nf, i + window + 1 - b);
      const int count = hi - lo - 1;
      if (count == 0) continue;
      const int32_t *ng = neg + ib * K;
      // target e of the position: the centre word (e == 0), draw e - 1, or -1 = nothing to train
      // (past `negative`, or a draw equal to the centre word)
      auto target = [&](int e) -> int32_t {
        if (e == 0) return centre;
        if (e > K) return -1;
        const int32_t t = __builtin_amdgcn_readfirstlane(ng[e - 1]);
        return t == centre ? -1 : t;
      };
      // ---- the first kTG target rows are requested before the context rows ----
      int32_t tg[kTG];
      Row<VEC> trow[kTG];
#pragma unroll
      for (int e = 0; e < kTG; ++e) {
        tg[e] = target(e);
        bool dup = false;
#pragma unroll
        for (int e2 = 0; e2 < e; ++e2) dup = dup || tg[e2] == tg[e];
        if (tg[e] >= 0 && !dup) load_row<VEC>(syn1neg + (int64_t)tg[e] * dim, dim, lane, full_at(tg[e]), trow[e]);
      }
      // ---- neu1: the context rows in groups of kCG, added in position order ----
      Row<VEC> neu1, work;
#pragma unroll
      for (int v = 0; v < VEC; ++v) neu1.v[v] = work.v[v] = 0.0f;
      // the m-th context position (m = 0 .. count - 1) is sentence position lo + m, + 1 past the centre
      const int before = i - lo;
      for (int m0 = 0; m0 < count; m0 += kCG) {
        Row<VEC> crow[kCG];
#pragma unroll
        for (int e = 0; e < kCG; ++e) {
          const int m = m0 + e;
          if (m < count) {
            const int32_t w = __builtin_amdgcn_readfirstlane(sent[lo + m + (m >= before ? 1 : 0)]);
            load_row<VEC>(syn0 + (int64_t)w * dim, dim, lane, full_at(w), crow[e]);
          }
        }
#pragma unroll
        for (int e = 0; e < kCG; ++e) {
          if (m0 + e < count) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) neu1.v[v] = neu1.v[v] + crow[e].v[v];
          }
        }
      }
      const float inv = 1.0f / (float)count;
      if (cbow_mean) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) neu1.v[v] = neu1.v[v] * inv;
      }
      // ---- the targets, in order ----
      auto train_target = [&](int32_t t, float label, float f, Row<VEC> &row) {
        if (f <= -6.0f || f >= 6.0f) return;
        const float g = (label - exp_lds[(int)((f + 6.0f) * 83.0f)]) * alpha;
        float *p = syn1neg + (int64_t)t * dim;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          work.v[v] = __fmaf_rn(g, row.v[v], work.v[v]);
          row.v[v] = __fmaf_rn(g, neu1.v[v], row.v[v]);
        }
        if (t < hub_rows) {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            if (lane * VEC + v < dim) unsafeAtomicAdd(p + lane * VEC + v, g * neu1.v[v]);
        } else {
          store_row<VEC>(p, dim, lane, full, row);
        }
      };
      {
        float f[kTG];
        bool dupf[kTG];
#pragma unroll
        for (int e = 0; e < kTG; ++e) {
          dupf[e] = false;
#pragma unroll
          for (int e2 = 0; e2 < e; ++e2) dupf[e] = dupf[e] || tg[e2] == tg[e];
          f[e] = (tg[e] >= 0 && !dupf[e]) ? wave_dot<VEC>(neu1, trow[e]) : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < kTG; ++e) {
          if (tg[e] < 0) continue;
          if (dupf[e]) {  // drawn twice: it sees its first update
            load_row<VEC>(syn1neg + (int64_t)tg[e] * dim, dim, lane, full_at(tg[e]), trow[e]);
            f[e] = wave_dot<VEC>(neu1, trow[e]);
          }
          train_target(tg[e], e == 0 ? 1.0f : 0.0f, f[e], trow[e]);
        }
      }
      for (int d0 = kTG; d0 <= K; d0 += kTG) {  // further groups (1 + negative > kTG): after the stores above
        int32_t tgn[kTG];
        Row<VEC> rown[kTG];
        float f[kTG];
        bool dupf[kTG];
#pragma unroll
        for (int e = 0; e < kTG; ++e) {
          tgn[e] = target(d0 + e);
          dupf[e] = false;
#pragma unroll
          for (int e2 = 0; e2 < e; ++e2) dupf[e] = dupf[e] || tgn[e2] == tgn[e];
          if (tgn[e] >= 0 && !dupf[e]) load_row<VEC>(syn1neg + (int64_t)tgn[e] * dim, dim, lane, full_at(tgn[e]), rown[e]);
        }
#pragma unroll
        for (int e = 0; e < kTG; ++e) f[e] = (tgn[e] >= 0 && !dupf[e]) ? wave_dot<VEC>(neu1, rown[e]) : 0.0f;
#pragma unroll
        for (int e = 0; e < kTG; ++e) {
          if (tgn[e] < 0) continue;
          if (dupf[e]) {
            load_row<VEC>(syn1neg + (int64_t)tgn[e] * dim, dim, lane, full_at(tgn[e]), rown[e]);
            f[e] = wave_dot<VEC>(neu1, rown[e]);
          }
          train_target(tgn[e], 0.0f, f[e], rown[e]);
        }
      }
      if (!cbow_mean) {  // gensim divides the error over the summed window
#pragma unroll
        for (int v = 0; v < VEC; ++v) work.v[v] = work.v[v] * inv;
      }
      // ---- syn0[context] += work, in position order ----
      for (int m0 = 0; m0 < count; m0 += kCG) {
        Row<VEC> crow[kCG];
        int32_t cw[kCG];
#pragma unroll
        for (int e = 0; e < kCG; ++e) {
          const int m = m0 + e;
          cw[e] = m < count ? __builtin_amdgcn_readfirstlane(sent[lo + m + (m >= before ? 1 : 0)]) : -1;
          bool dup = false;
#pragma unroll
          for (int e2 = 0; e2 < e; ++e2) dup = dup || cw[e2] == cw[e];
          if (cw[e] >= hub_rows && !dup) load_row<VEC>(syn0 + (int64_t)cw[e] * dim, dim, lane, full, crow[e]);
        }
#pragma unroll
        for (int e = 0; e < kCG; ++e) {
          if (cw[e] < 0) continue;
          float *p = syn0 + (int64_t)cw[e] * dim;
          if (cw[e] < hub_rows) {
            add_row<VEC>(p, dim, lane, work);
            continue;
          }
          bool dup = false;
#pragma unroll
          for (int e2 = 0; e2 < e; ++e2) dup = dup || cw[e2] == cw[e];
          if (dup) load_row<VEC>(p, dim, lane, full, crow[e]);  // a repeated word: on top of its first update
#pragma unroll
          for (int v = 0; v < VEC; ++v) crow[e].v[v] = crow[e].v[v] + work.v[v];
          store_row<VEC>(p, dim, lane, full, crow[e]);
        }
      }
      ++trained;
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (pairs_out && lane == 0 && trained) atomicAdd(pairs_out, trained);
}

// n2v_cbow_train, or (dry_waves != NULL) only its launch geometry
static int train_impl(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1neg,
                      const uint32_t *cum_table, const uint32_t *sample_int, const float *exp_table,
                      const n2v_sgns_params *P, int32_t cbow_mean, unsigned long long *pairs_out, void *stream,
                      int64_t *dry_waves) {
  if (!P) return N2V_EINVAL;
  if (!dry_waves && (!walks || !syn0 || !syn1neg || !cum_table || !exp_table)) return N2V_EINVAL;
  if (!check_common(P->n_vocab, P->dim, P->window, n_walks, walk_len) || P->negative < 1 || P->negative > 32)
    return N2V_EINVAL;
  if (P->batched != 0 || P->window_cache != 0) return N2V_EINVAL;  // skip-gram variants
  if (cbow_mean != 0 && cbow_mean != 1) return N2V_EINVAL;
  if (P->hub_rows < 0 || P->max_waves < 0) return N2V_EINVAL;
  if (P->cum_index && (P->cum_index_bits < 1 || P->cum_index_bits > 30)) return N2V_EINVAL;
  if (dry_waves) *dry_waves = 0;
  if (n_walks == 0) return N2V_OK;
  const int V = vec_of(P->dim);
  const int sent_cap = sent_cap_of(walk_len);
  const size_t lds = kExpTable * sizeof(float) + (P->cum_index ? 0 : (kBuckets + 1 + 3) * sizeof(int32_t)) +
                     (size_t)kWaves * (size_t)(2 * sent_cap + kNegSlots) * 4;
  const LaunchGeometry geo = hogwild_geometry(P->n_vocab, n_walks, P->max_waves, P->deterministic, kWaves);
  auto launch = [&](auto kernel) {
    return launch_trainer(kernel, geo, lds, P->deterministic, pairs_out, stream, dry_waves, walks, n_walks, walk_len,
                          syn0, syn1neg, cum_table, sample_int, exp_table, *P, cbow_mean, pairs_out, sent_cap);
  };
  switch (V) {
    case 1: return launch(cbow_kernel<1>);
    case 2: return launch(cbow_kernel<2>);
    case 4: return launch(cbow_kernel<4>);
    case 8: return launch(cbow_kernel<8>);
    default: return launch(cbow_kernel<16>);
  }
}

}  // namespace cbow
}  // namespace n2v

extern "C" int n2v_cbow_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0,
                              float *syn1neg, const uint32_t *cum_table, const uint32_t *sample_int,
                              const float *exp_table, const n2v_sgns_params *P, int32_t cbow_mean,
                              unsigned long long *pairs_out, void *stream) {
  return n2v::cbow::train_impl(walks, n_walks, walk_len, syn0, syn1neg, cum_table, sample_int, exp_table, P,
                               cbow_mean, pairs_out, stream, nullptr);
}

extern "C" int64_t n2v_cbow_hogwild_waves(const n2v_sgns_params *P, int64_t n_walks, int32_t walk_len) {
  int64_t waves = 0;
  const int rc = n2v::cbow::train_impl(nullptr, n_walks, walk_len, nullptr, nullptr, nullptr, nullptr, nullptr, P, 1,
                                       nullptr, nullptr, &waves);
  return rc == N2V_OK ? waves : (int64_t)rc;
}
