// n2v_foldin.hip -- fold-in: rows for NEW vertices against a frozen skip-gram negative-sampling model
// (DESIGN.md "Fold-in").
//
// syn1neg and the rows of every known word are frozen.  A pair (centre position i, context position j) of
// sgns_kernel (n2v_sgns.hip) then writes nothing but row1 = the row of sent[j], so the whole training of a new
// vertex u is ONE sequential chain over the pairs whose context word is u, independent of every other new vertex:
// no races, no atomics, and the same bits for any launch geometry.
//
//   foldin_pairs_kernel  one wave per walk: the trainer's sentence preparation (restated below; a new token is
//                        always kept), then one 16-byte record per trainable pair -- sent[j] new, sent[i] known --
//                        in (row, i, j) order.  Run twice: a count pass, the caller's prefix over rows, a fill
//                        pass; no atomic decides an order.
//   foldin_kernel<VEC>   one wave per new vertex: the row is loaded once, trained over the vertex's record list
//                        (the caller grouped the records by vertex with a STABLE sort) and stored once.
//
// Per pair the chain reads 4 * dim * (1 + K) bytes and writes nothing (the trainer moves 8 * dim * (2 + K)).
// Every address of the chain is known before it starts -- centres from the records, negatives from the
// counter-based draws -- so the rows of the next two pairs are requested while a pair is trained.
#include "n2v_common.h"
#include "n2v_w2v_core.h"

namespace n2v {

constexpr int kFoldWaves = 4;  // waves per block, as the trainers

// ---- pair listing ----
// records == NULL: the count pass (row_count[r] = records of walk r); else the fill pass, walk r writing from
// records[row_off[r]].  A record is {new index, row, i | rel << 16, centre word}.
__global__ __launch_bounds__(kFoldWaves * 64) void foldin_pairs_kernel(
    const int32_t *__restrict__ walks, int64_t n_walks, int32_t walk_len, int64_t n_vocab, int64_t n_new,
    const uint32_t *__restrict__ sample_int, uint64_t seed, int64_t sentence_base, int32_t window,
    const int64_t *__restrict__ row_off, int64_t *__restrict__ row_count, int4 *__restrict__ records) {
  __shared__ int32_t sent_s[kFoldWaves][N2V_SGNS_MAX_SENTENCE];
  __shared__ int32_t red_s[kFoldWaves][N2V_SGNS_MAX_SENTENCE];
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  int32_t *sent = sent_s[wave_in_block];
  int32_t *red = red_s[wave_in_block];
  const int64_t n_waves = (int64_t)gridDim.x * kFoldWaves;
  const int64_t n_all = n_vocab + n_new;
  for (int64_t rr = (int64_t)blockIdx.x * kFoldWaves + wave_in_block; rr < n_walks; rr += n_waves) {
    const int64_t r = readfirstlane_i64(rr);
    const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
    // ---- sentence preparation: sgns_kernel's, restated (its object code stays as it is).  The one difference:
    // a new token is always kept -- sample_int has no entry for it; the draws are keyed on t, nothing shifts ----
    int nf = 0;
    for (int base = 0; base < walk_len; base += 64) {
      const int t = base + lane;
      int32_t tok = t < walk_len ? walks[r * walk_len + t] : -1;
      bool keep = tok >= 0 && (int64_t)tok < n_all;
      if (keep && sample_int && (int64_t)tok < n_vocab) {
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

    // ---- the pairs of every known centre: lane `rel` is the trainer's window slot of context position j ----
    const int64_t out = records ? row_off[r] : 0;
    int64_t cnt = 0;
    for (int i = 0; i < nf; ++i) {
      const int32_t centre = __builtin_amdgcn_readfirstlane(sent[i]);
      if ((int64_t)centre >= n_vocab) continue;  // a new vertex has no output row
      const int b = __builtin_amdgcn_readfirstlane(red[i]);
      const int lo = max(0, i - window + b);
      const int hi = min(nf, i + window + 1 - b);
      const int rel = lane;  // rel = j - i + window - (j > i): below `window` before the centre, from it on after
      const int j = i - window + rel + (rel >= window ? 1 : 0);
      bool emit = rel < 2 * window && j >= lo && j < hi;
      const int32_t cj = emit ? sent[j] : 0;
      emit = emit && (int64_t)cj >= n_vocab;  // a known context word is frozen
      const uint64_t mask = ballot64(emit);
      if (records && emit)
        records[out + cnt + __popcll(mask & ((1ull << lane) - 1ull))] =
            make_int4((int32_t)((int64_t)cj - n_vocab), (int32_t)r, i | (rel << 16), centre);
      cnt += __popcll(mask);
    }
    if (!records && lane == 0) row_count[r] = cnt;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the next walk overwrites sent / red
  }
}

// ---- chain training ----
// Rows are read with PLAIN loads: nothing this kernel reads is written while it runs (syn1neg and the tables are
// frozen, a new row belongs to one wave), so the agent-scope loads of row_ld1 / load_row, which exist to read
// past another CU's stale cache line, are not needed.
template <int VEC>
__device__ __forceinline__ void load_plain(const float *base, int dim, int lane, bool full, Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      r.v[0] = base[lane];
    } else if constexpr (VEC == 2) {
      const float2 t = *reinterpret_cast<const float2 *>(base + lane * 2);
      r.v[0] = t.x;
      r.v[1] = t.y;
    } else {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const float4 t = *reinterpret_cast<const float4 *>(base + lane * VEC + q * 4);
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
      r.v[v] = e < dim ? base[e] : 0.0f;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_plain(float *base, int dim, int lane, bool full, const Row<VEC> &r) {
  if (full) {
    if constexpr (VEC == 1) {
      base[lane] = r.v[0];
    } else if constexpr (VEC == 2) {
      *reinterpret_cast<float2 *>(base + lane * 2) = make_float2(r.v[0], r.v[1]);
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
      if (e < dim) base[e] = r.v[v];
    }
  }
}

// negative rows of a pair that are requested ahead, as sgns_kernel's KP; with three pairs' buffers live
// (one trained, two in flight) that is 3 * (1 + KP) * VEC row registers per lane
template <int VEC>
constexpr int fold_kp() {
  return VEC <= 4 ? 5 : (VEC == 8 ? 3 : 1);
}

template <int VEC>
// Occupancy aimed for: the chain is latency-bound like the trainer.  dim <= 64 (VEC 1: 18 row registers in the
// three buffers) holds the full 8 waves per SIMD in 61 VGPRs.  dim <= 128 (VEC 2: 36 row registers) spills 16
// VGPRs when held to 64, so it is asked for 6 waves per SIMD (80 VGPRs, 8 bytes of scratch per lane): 6 waves
// x 12 rows in flight.  Wider rows take the registers they need: 131 VGPRs at VEC 4, 167 at VEC 8, 175 at
// VEC 16 -- 3 to 2 waves per SIMD, each with 2 * (1 + KP) rows of 1 to 4 KB in flight.  (Compiler figures;
// other choices have not been measured on the GPU.)
__global__ __launch_bounds__(kFoldWaves * 64, (VEC == 1 ? 8 : (VEC == 2 ? 6 : 1))) void foldin_kernel(
    const int4 *__restrict__ records, const int64_t *__restrict__ vertex_off, int64_t n_new, int64_t n_walks,
    int32_t walk_len, float *__restrict__ new_rows, const float *__restrict__ syn1neg,
    const uint32_t *__restrict__ cum_table, const float *__restrict__ exp_table_g, n2v_sgns_params P) {
  constexpr int KP = fold_kp<VEC>();
  __shared__ float exp_lds[kExpTable];
  __shared__ int32_t bucket[kBuckets + 1];
  // two batches of draws per wave: one being trained, one being requested ahead
  __shared__ int32_t neg_s[kFoldWaves][2][64];
  __shared__ int32_t cen_s[kFoldWaves][2][64];
  __shared__ float alp_s[kFoldWaves][2][64];
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < kExpTable; i += blockDim.x) exp_lds[i] = exp_table_g[i];
  if (!P.cum_index) bucket_table_build(bucket, cum_table, P.n_vocab);
  __syncthreads();

  const int dim = P.dim, window = P.window, K = P.negative;
  const bool full = dim == 64 * VEC;
  const int32_t n_vocab = (int32_t)P.n_vocab;
  const uint32_t domain = cum_table[P.n_vocab - 1];
  const int B = 64 / K;  // records per batch of draws: one lane per (record, d) slot; K <= 32, so B >= 2
  const int64_t n_waves = (int64_t)gridDim.x * kFoldWaves;
  int32_t(*neg)[64] = neg_s[wave_in_block];
  int32_t(*cen)[64] = cen_s[wave_in_block];
  float(*alp)[64] = alp_s[wave_in_block];

  struct PairBuf {
    Row<VEC> crow;
    Row<VEC> rows[KP];
    int32_t tg[KP];  // < 0: skipped (the draw hit the centre word, or past K)
    int32_t centre;  // < 0: a record this kernel refuses to follow (not the listing's)
    float alpha;
    int half, rec;   // where the pair's draws stand in LDS (the groups past KP are read when it is trained)
  };

  // a grid larger than n_new: the surplus waves find no vertex
  for (int64_t uu = (int64_t)blockIdx.x * kFoldWaves + wave_in_block; uu < n_new; uu += n_waves) {
    const int64_t u = readfirstlane_i64(uu);
    const int64_t beg = vertex_off[u], end = vertex_off[u + 1];
    if (beg >= end) continue;  // the vertex never occurs: its row stays as it is
    float *prow = new_rows + u * dim;
    Row<VEC> row1;
    load_plain<VEC>(prow, dim, lane, full, row1);

    int64_t pi = beg;     // next record to request
    int ib = 0, ih = 0;   // its place in its batch, and the batch's half of the LDS buffers

    // ---- negative draws of records [p0, p0 + B), lane-parallel: sgns_kernel's draws for those pairs ----
    auto draw_batch = [&](int64_t p0, int half) {
      const int nb = (int)(end - p0 < (int64_t)B ? end - p0 : (int64_t)B);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the pairs that read this half are trained
      const int rec = lane / K, d = lane - rec * K;
      if (rec < nb) {
        const int4 R = records[p0 + rec];
        const int32_t row = R.y, i = R.z & 0xffff, rel = R.z >> 16, centre = R.w;
        const bool ok = row >= 0 && (int64_t)row < n_walks && centre >= 0 && centre < n_vocab && i < walk_len &&
                        rel >= 0 && rel < 2 * window;
        int32_t tg = -1;
        if (ok) {
          const uint64_t hs = sentence_stream(P.seed, (uint64_t)(P.sentence_base + (int64_t)row));
          const uint64_t idx = 2ULL * (uint64_t)walk_len +
                               ((uint64_t)i * 2ULL * (uint64_t)window + (uint64_t)rel) * (uint64_t)K + (uint64_t)d;
          const uint32_t x = (uint32_t)((sentence_draw(hs, idx) >> 16) % (uint64_t)domain);
          int blo, bhi;  // bisect_left(cum_table, x) inside the bucket of x, as the trainer does
          if (P.cum_index) {
            const uint32_t bk = x >> (31 - P.cum_index_bits);
            blo = P.cum_index[bk];
            bhi = P.cum_index[bk + 1];
          } else {
            blo = bucket[x >> 21];
            bhi = bucket[(x >> 21) + 1];
          }
          blo = bisect_range_u32(cum_table, blo, bhi, x);
          blo = blo < n_vocab ? blo : n_vocab - 1;  // (a table that ends at its domain never gets here)
          tg = blo == centre ? -1 : blo;            // a negative equal to the centre is skipped
        }
        neg[half][lane] = tg;
        if (d == 0) {
          cen[half][rec] = ok ? centre : -1;
          alp[half][rec] = (ok && P.row_alpha) ? P.row_alpha[row] : P.alpha;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    };
    // start every row load of record pi: the centre's syn1neg row and the first KP negatives.  Nothing the
    // chain reads is ever written, so there is no `late` row: a request may run any distance ahead.
    auto issue = [&](PairBuf &Q) {
      if (pi >= end) return;
      if (ib == 0) draw_batch(pi, ih);
      // LDS loads at a uniform address are lane-varying to the compiler: mark them scalar
      Q.centre = __builtin_amdgcn_readfirstlane(cen[ih][ib]);
      Q.alpha = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(alp[ih][ib])));
      Q.half = ih;
      Q.rec = ib;
      if (Q.centre >= 0) load_plain<VEC>(syn1neg + (int64_t)Q.centre * dim, dim, lane, full, Q.crow);
#pragma unroll
      for (int e = 0; e < KP; ++e) {
        Q.tg[e] = (e < K && Q.centre >= 0) ? __builtin_amdgcn_readfirstlane(neg[ih][ib * K + e]) : -1;
        if (Q.tg[e] >= 0) load_plain<VEC>(syn1neg + (int64_t)Q.tg[e] * dim, dim, lane, full, Q.rows[e]);
      }
      ++pi;
      if (++ib == B) {
        ib = 0;
        ih ^= 1;
      }
    };
    // one pair: sgns_kernel's process with the stores to syn1neg removed
    auto process = [&](PairBuf &A) {
      if (A.centre < 0) return;
      const float alpha = A.alpha;
      Row<VEC> work;
#pragma unroll
      for (int v = 0; v < VEC; ++v) work.v[v] = 0.0f;
      {  // the centre word, label 1
        const float f = wave_dot<VEC>(row1, A.crow);
        if (!(f <= -6.0f || f >= 6.0f)) {
          const float g = (1.0f - exp_lds[(int)((f + 6.0f) * 83.0f)]) * alpha;
#pragma unroll
          for (int v = 0; v < VEC; ++v) work.v[v] = __fmaf_rn(g, A.crow.v[v], work.v[v]);
        }
      }
      auto train_negative = [&](const Row<VEC> &row2) {
        const float f = wave_dot<VEC>(row1, row2);
        if (f <= -6.0f || f >= 6.0f) return;
        const float g = (0.0f - exp_lds[(int)((f + 6.0f) * 83.0f)]) * alpha;
#pragma unroll
        for (int v = 0; v < VEC; ++v) work.v[v] = __fmaf_rn(g, row2.v[v], work.v[v]);
      };
#pragma unroll
      for (int e = 0; e < KP; ++e) {  // first group: rows already in flight
        if (A.tg[e] < 0) continue;
        train_negative(A.rows[e]);
      }
      const int32_t *ng = neg[A.half] + A.rec * K;
      for (int d0 = KP; d0 < K; d0 += KP) {  // further groups (negative > KP): requested here
        int32_t tg[KP];
        Row<VEC> rows[KP];
#pragma unroll
        for (int e = 0; e < KP; ++e) {
          tg[e] = (d0 + e < K) ? __builtin_amdgcn_readfirstlane(ng[d0 + e]) : -1;
          if (tg[e] >= 0) load_plain<VEC>(syn1neg + (int64_t)tg[e] * dim, dim, lane, full, rows[e]);
        }
#pragma unroll
        for (int e = 0; e < KP; ++e) {
          if (tg[e] < 0) continue;
          train_negative(rows[e]);
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) row1.v[v] = row1.v[v] + work.v[v];
    };

    // Three buffers in rotation, spelled out so that no buffer is ever copied (a copy would wait for its loads):
    // while pair p is trained the rows of p + 1 and p + 2 are in flight.  A batch of draws is made when the
    // requests reach its first record; by then training stands in the batch before it (B >= 2), so the half it
    // overwrites is no longer read.
    PairBuf bufA, bufB, bufC;
    issue(bufA);
    issue(bufB);
    for (int64_t pp = beg; pp < end;) {
      issue(bufC);
      process(bufA);
      if (++pp >= end) break;
      issue(bufA);
      process(bufB);
      if (++pp >= end) break;
      issue(bufB);
      process(bufC);
      ++pp;
    }
    store_plain<VEC>(prow, dim, lane, full, row1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the next vertex overwrites the draw buffers
  }
}

// what n2v_sgns_train refuses of these parameters, and what fold-in adds to that
static bool foldin_check(const n2v_sgns_params *P, int64_t n_walks, int32_t walk_len, int64_t n_new) {
  if (!P) return false;
  if (!check_common(P->n_vocab, P->dim, P->window, n_walks, walk_len) || P->negative < 1 || P->negative > 32)
    return false;
  if (P->batched != 0 || P->window_cache != 0 || P->hub_rows < 0) return false;
  if (P->cum_index && (P->cum_index_bits < 1 || P->cum_index_bits > 30)) return false;
  if (n_walks >= (1ll << 31)) return false;  // a record names its row in 32 bits
  // tokens are int32: the last new vertex is token n_vocab + n_new - 1
  return n_new >= 0 && n_new <= (1ll << 31) && P->n_vocab + n_new <= (1ll << 31);
}

static int foldin_pairs_launch(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_new,
                               const uint32_t *sample_int, const n2v_sgns_params *P, const int64_t *row_off,
                               int64_t *row_count, int4 *records, void *stream) {
  const int64_t blocks = (n_walks + kFoldWaves - 1) / kFoldWaves;
  N2V_HIP_CHECK(launch_resident(foldin_pairs_kernel, kFoldWaves * 64, 0, blocks, (hipStream_t)stream, walks, n_walks,
                                walk_len, P->n_vocab, n_new, sample_int, P->seed, P->sentence_base, P->window,
                                row_off, row_count, records));
  return N2V_OK;
}

}  // namespace n2v

extern "C" int n2v_foldin_pair_counts(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_new,
                                      const uint32_t *sample_int, const n2v_sgns_params *P, int64_t *row_count_out,
                                      void *stream) {
  if (!n2v::foldin_check(P, n_walks, walk_len, n_new) || !walks || !row_count_out) return N2V_EINVAL;
  if (n_walks == 0) return N2V_OK;
  return n2v::foldin_pairs_launch(walks, n_walks, walk_len, n_new, sample_int, P, nullptr, row_count_out, nullptr,
                                  stream);
}

extern "C" int n2v_foldin_pair_records(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_new,
                                       const uint32_t *sample_int, const n2v_sgns_params *P, const int64_t *row_off,
                                       n2v_foldin_record *records_out, void *stream) {
  if (!n2v::foldin_check(P, n_walks, walk_len, n_new) || !walks || !row_off || !records_out) return N2V_EINVAL;
  if (n_walks == 0) return N2V_OK;
  static_assert(sizeof(n2v_foldin_record) == sizeof(int4), "a record is one 16-byte store");
  return n2v::foldin_pairs_launch(walks, n_walks, walk_len, n_new, sample_int, P, row_off, nullptr,
                                  reinterpret_cast<int4 *>(records_out), stream);
}

extern "C" int n2v_foldin_train(const n2v_foldin_record *records, const int64_t *vertex_off, int64_t n_new,
                                int64_t n_walks, int32_t walk_len, float *new_rows, const float *syn1neg,
                                const uint32_t *cum_table, const float *exp_table, const n2v_sgns_params *P,
                                void *stream) {
  using namespace n2v;
  if (!foldin_check(P, n_walks, walk_len, n_new) || !syn1neg || !cum_table || !exp_table) return N2V_EINVAL;
  if (n_new > 0 && !new_rows) return N2V_EINVAL;
  if (n_new == 0 || n_walks == 0) return N2V_OK;
  if (!records || !vertex_off) return N2V_EINVAL;
  // one wave per new vertex, at most max_waves (> 0; whole blocks) and at most those resident at once
  int64_t waves = n_new;
  if (P->max_waves > 0 && waves > P->max_waves) waves = P->max_waves;
  const int64_t blocks = (waves + kFoldWaves - 1) / kFoldWaves;
  const int4 *rec = reinterpret_cast<const int4 *>(records);
  auto launch = [&](auto kernel) {
    N2V_HIP_CHECK(launch_resident(kernel, kFoldWaves * 64, 0, blocks, (hipStream_t)stream, rec, vertex_off, n_new,
                                  n_walks, walk_len, new_rows, syn1neg, cum_table, exp_table, *P));
    return (int)N2V_OK;
  };
  // the VEC set of sgns_kernel: dim 1 .. 1024, full and ragged
  switch (vec_of(P->dim)) {
    case 1: return launch(foldin_kernel<1>);
    case 2: return launch(foldin_kernel<2>);
    case 4: return launch(foldin_kernel<4>);
    case 8: return launch(foldin_kernel<8>);
    default: return launch(foldin_kernel<16>);
  }
}
