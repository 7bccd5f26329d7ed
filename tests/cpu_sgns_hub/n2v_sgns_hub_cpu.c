/*
 * n2v_sgns_hub_cpu.c -- single-thread CPU restatement of the HUB FORM of the two skip-gram trainers:
 * what node2vec_amd/csrc/n2v_sgns.hip and n2v_sgns_batched.hip compute in hogwild mode, where rows
 * below hub_rows (and every row that leaves an LDS ring) go back to memory as fp32 atomic adds
 * instead of stores.
 *
 * TEST INFRASTRUCTURE ONLY: tests/test_hub_form_*.py build it with the flags of tests/cpu_build.py (no
 * contraction, no fast-math) and pin the kernels to it bit for bit on one wave and on the
 * conflict-free corpora of tests/conflict_free.py.  It is a SECOND statement of the in-order
 * training: written from the kernels' comments and from what oracle/n2v_oracle_sgns.c documents, it
 * calls nothing of the oracle, and with hub_rows = 0 (and stores for the ring) the tests hold it to
 * the oracle's bits.
 *
 * An atomic add is ONE fp32 addition onto the value memory holds at that moment, in program order
 * (hub_add below).  On one wave, or where no two waves touch a row, that is what the hardware add
 * computes whatever the schedule -- provided no operand is subnormal (a hardware fp32 atomic need
 * not honour the denormal mode): compiled with -DN2V_HUB_CHECK every add counts such operands, and
 * the tests assert the count is zero on every case they take to the GPU.
 *
 * The default trainer (n2v_sgns_hub_cpu_train), per position i of the prepared sentence:
 *   crow = syn1neg[centre] as loaded, crow0 = crow;
 *   per pair (i, j), j ascending: row1 = syn0[sent[j]] (window cache: the ring's copy), work = 0;
 *     label 1: f = dot(row1, crow); |f| < 6: g = (1 - sigma) * alpha; work = fma(g, crow, work);
 *              crow = fma(g, row1, crow)                       (registers: memory is not touched)
 *     every negative t != centre, in draw order: row2 = syn1neg[t] as memory holds it NOW;
 *              f = dot(row1, row2); |f| < 6: g = (0 - sigma) * alpha; work = fma(g, row2, work);
 *              t <  hub_rows: syn1neg[t][e] = syn1neg[t][e] + fl(g * row1[e])      (atomic add)
 *              t >= hub_rows: syn1neg[t][e] = fma(g, row1[e], row2[e])              (store)
 *     then the context row: window cache: ring copy = row1 + work;
 *              else sent[j] <  hub_rows: syn0[.][e] = syn0[.][e] + work[e]          (atomic add)
 *                   sent[j] >= hub_rows: syn0[.][e] = row1[e] + work[e]             (store)
 *   after the pairs: centre < hub_rows: syn1neg[centre][e] += crow[e] - crow0[e]    (atomic add)
 *                    else syn1neg[centre] = crow                                    (store)
 * The window cache holds one copy per distinct word of positions i - window .. i + 1 + window,
 * loaded when the first of them enters (position i + 1 + window enters BEFORE position i trains)
 * and written back when the last leaves (position i - window, AFTER position i trained):
 * syn0[w][e] += copy[e] - loaded[e] (atomic add, whatever hub_rows is).
 *
 * The batched trainer (n2v_sgns_hub_cpu_train_batched) is documented at its function.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* test-only mutations: each is one way a kernel could be subtly wrong that a norm ratio survives */
enum {
  MUT_NONE = 0,
  MUT_CENTRE_TWICE = 1, /* the centre delta added twice */
  MUT_NEG_FMA = 2,      /* the negative add uses fma(g, row1, mem) instead of mem + fl(g * row1) */
  MUT_BOUNDARY = 3,     /* row hub_rows itself is treated as a hub */
  MUT_LAST_LANE = 4     /* the last lane that owns elements of a ragged row skips its adds */
};

static int64_t subnormal_operands = 0;

/* operands of atomic adds that were nonzero subnormals since the last call; -1 without N2V_HUB_CHECK */
int64_t n2v_sgns_hub_cpu_subnormals(void) {
#ifdef N2V_HUB_CHECK
  const int64_t n = subnormal_operands;
  subnormal_operands = 0;
  return n;
#else
  (void)subnormal_operands;
  return -1;
#endif
}

static inline void hub_add(float *mem, float x) {
  const float sum = *mem + x;
#ifdef N2V_HUB_CHECK
  subnormal_operands += (x != 0.0f && fabsf(x) < FLT_MIN) + (*mem != 0.0f && fabsf(*mem) < FLT_MIN) +
                        (sum != 0.0f && fabsf(sum) < FLT_MIN);
#endif
  *mem = sum;
}

static inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static inline uint64_t sentence_stream(uint64_t seed, uint64_t sentence_id) {
  return mix64(seed ^ mix64(sentence_id + 0xA0761D6478BD642FULL));
}

static inline uint64_t draw(uint64_t hs, uint64_t idx) { return mix64(hs + (idx + 1ULL) * 0xE7037ED1A0B428DBULL); }

static int vec_width(int dim) {
  int v = 1;
  while (64 * v < dim) v *= 2;
  return v;
}

/* wave64 order: lane l owns elements l*V .. l*V+V-1 (an fma chain), then the butterfly over lane
 * distances 1, 2, 4, 8, 16, 32 */
static float wave_dot(const float *a, const float *b, int dim, int V) {
  float p[64], t[64];
  for (int l = 0; l < 64; ++l) {
    float acc = 0.0f;
    for (int v = 0; v < V; ++v) {
      const int e = l * V + v;
      if (e < dim) acc = fmaf(a[e], b[e], acc);
    }
    p[l] = acc;
  }
  for (int off = 1; off < 64; off <<= 1) {
    for (int l = 0; l < 64; ++l) t[l] = p[l] + p[l ^ off];
    memcpy(p, t, sizeof(p));
  }
  return p[0];
}

static int32_t bisect_left(const uint32_t *a, int64_t n, uint32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (int32_t)lo;
}

/* vocabulary filter, subsampling (draw 2t), reduced windows (draw 2t + 1) of raw position t */
static int prepare(const int32_t *row, int walk_len, int64_t n_vocab, const uint32_t *sample_int, uint64_t hs,
                   int window, int32_t *sent, int32_t *red) {
  int nf = 0;
  for (int t = 0; t < walk_len; ++t) {
    const int32_t tok = row[t];
    if (tok < 0 || tok >= n_vocab) continue;
    if (sample_int && sample_int[tok] < (uint32_t)(draw(hs, 2ULL * (uint64_t)t) >> 32)) continue;
    sent[nf] = tok;
    red[nf] = (int32_t)((uint32_t)(draw(hs, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
    ++nf;
  }
  return nf;
}

/* elements of a row that take an atomic add: all of them, or (MUT_LAST_LANE) all but those of the
 * last lane that owns any, where the row does not fill the wave */
static int add_end(int dim, int V, int mutation) {
  if (mutation == MUT_LAST_LANE && dim != 64 * V) return (dim - 1) / V * V;
  return dim;
}

/* the window cache: one copy per distinct word in the window */
typedef struct {
  int32_t word[16];
  int ref[16];
  float *cur, *loaded; /* [16][dim] */
} Ring;

static int ring_enter(Ring *R, int32_t word, const float *syn0, int dim) {
  int k = 0;
  while (k < 16 && !(R->ref[k] > 0 && R->word[k] == word)) ++k;
  if (k == 16) {
    k = 0;
    while (R->ref[k] != 0) ++k; /* 2 * window + 2 <= 16 positions are in the ring at most */
    R->word[k] = word;
    memcpy(R->cur + (size_t)k * dim, syn0 + (int64_t)word * dim, sizeof(float) * (size_t)dim);
    memcpy(R->loaded + (size_t)k * dim, syn0 + (int64_t)word * dim, sizeof(float) * (size_t)dim);
  }
  ++R->ref[k];
  return k;
}

/* the row goes back with its last position: as the delta it collected (add), or as it stands (store) */
static void ring_leave(Ring *R, int k, float *syn0, int dim, int store) {
  if (--R->ref[k] != 0) return;
  float *dst = syn0 + (int64_t)R->word[k] * dim;
  for (int e = 0; e < dim; ++e) {
    if (store)
      dst[e] = R->cur[(size_t)k * dim + e];
    else
      hub_add(dst + e, R->cur[(size_t)k * dim + e] - R->loaded[(size_t)k * dim + e]);
  }
}

/* The default trainer, rows [0, n_walks) in order.  window_cache 1 needs dim 64 or 128 and window <= 7
 * (what the kernel accepts).  roles (or NULL): int64 [3][n_vocab], += 1 per position a word is the
 * centre of, per pair it is the context of, per negative target update it receives.  Returns the
 * pairs trained, -1 for arguments the kernel refuses. */
int64_t n2v_sgns_hub_cpu_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1neg,
                               const uint32_t *cum_table, const uint32_t *sample_int, const float *exp_table,
                               int64_t n_vocab, int64_t sentence_base, uint64_t seed, int32_t dim, int32_t window,
                               int32_t negative, float alpha, int32_t hub_rows, int32_t window_cache, int32_t mutation,
                               int64_t *roles) {
  if (walk_len < 1 || walk_len > 256 || dim < 1 || dim > 1024 || window < 1 || window > 32 || negative < 1 ||
      negative > 32 || n_vocab < 1 || hub_rows < 0 || (window_cache != 0 && window_cache != 1))
    return -1;
  const int V = vec_width(dim);
  if (window_cache && (dim != 64 * V || V > 2 || 2 * window + 2 > 16)) return -1;
  const int hub_end = mutation == MUT_BOUNDARY ? hub_rows + 1 : hub_rows; /* rows below it are hubs */
  const int aend = add_end(dim, V, mutation);
  const uint32_t domain = cum_table[n_vocab - 1];
  int32_t sent[256], red[256];
  int pos_row[256];
  float *work = (float *)malloc(sizeof(float) * (size_t)dim);
  float *crow = (float *)malloc(sizeof(float) * (size_t)dim);
  float *crow0 = (float *)malloc(sizeof(float) * (size_t)dim);
  Ring R;
  R.cur = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  R.loaded = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  int64_t pairs = 0;
  for (int64_t r = 0; r < n_walks; ++r) {
    const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
    const int nf = prepare(walks + r * walk_len, walk_len, n_vocab, sample_int, hs, window, sent, red);
    for (int k = 0; k < 16; ++k) R.ref[k] = 0;
    if (window_cache)
      for (int j = 0; j <= window && j < nf; ++j) pos_row[j] = ring_enter(&R, sent[j], syn0, dim);
    for (int i = 0; i < nf; ++i) {
      if (window_cache && i + 1 + window < nf)
        pos_row[i + 1 + window] = ring_enter(&R, sent[i + 1 + window], syn0, dim);
      const int32_t centre = sent[i];
      int lo = i - window + red[i];
      if (lo < 0) lo = 0;
      int hi = i + window + 1 - red[i];
      if (hi > nf) hi = nf;
      float *pc = syn1neg + (int64_t)centre * dim;
      memcpy(crow, pc, sizeof(float) * (size_t)dim);
      memcpy(crow0, pc, sizeof(float) * (size_t)dim);
      if (roles && hi - lo > 1) ++roles[centre];
      for (int j = lo; j < hi; ++j) {
        if (j == i) continue;
        const int32_t cj = sent[j];
        float *mem1 = syn0 + (int64_t)cj * dim;
        float *row1 = window_cache ? R.cur + (size_t)pos_row[j] * dim : mem1;
        const int rel = j - i + window - (j > i ? 1 : 0);
        if (roles) ++roles[n_vocab + cj];
        for (int e = 0; e < dim; ++e) work[e] = 0.0f;
        { /* the centre word, label 1: in registers */
          const float f = wave_dot(row1, crow, dim, V);
          if (!(f <= -6.0f || f >= 6.0f)) {
            const float g = (1.0f - exp_table[(int)((f + 6.0f) * 83.0f)]) * alpha;
            for (int e = 0; e < dim; ++e) {
              work[e] = fmaf(g, crow[e], work[e]);
              crow[e] = fmaf(g, row1[e], crow[e]);
            }
          }
        }
        for (int d = 0; d < negative; ++d) {
          const uint64_t idx = 2ULL * (uint64_t)walk_len +
                               ((uint64_t)i * 2ULL * (uint64_t)window + (uint64_t)rel) * (uint64_t)negative + (uint64_t)d;
          const int32_t t = bisect_left(cum_table, n_vocab, (uint32_t)((draw(hs, idx) >> 16) % (uint64_t)domain));
          if (t == centre) continue;
          float *row2 = syn1neg + (int64_t)t * dim;
          const float f = wave_dot(row1, row2, dim, V);
          if (f <= -6.0f || f >= 6.0f) continue;
          const float g = (0.0f - exp_table[(int)((f + 6.0f) * 83.0f)]) * alpha;
          if (roles) ++roles[2 * n_vocab + t];
          const int hub = t < hub_end;
          for (int e = 0; e < dim; ++e) {
            const float r2 = row2[e];
            work[e] = fmaf(g, r2, work[e]);
            if (!hub) {
              row2[e] = fmaf(g, row1[e], r2);
            } else if (e < aend) {
              if (mutation == MUT_NEG_FMA)
                row2[e] = fmaf(g, row1[e], r2);
              else
                hub_add(row2 + e, g * row1[e]);
            }
          }
        }
        if (!window_cache && cj < hub_end) {
          for (int e = 0; e < aend; ++e) hub_add(mem1 + e, work[e]);
        } else {
          for (int e = 0; e < dim; ++e) row1[e] = row1[e] + work[e]; /* the ring's copy, or memory */
        }
        ++pairs;
      }
      if (centre < hub_end) {
        for (int e = 0; e < aend; ++e) {
          hub_add(pc + e, crow[e] - crow0[e]);
          if (mutation == MUT_CENTRE_TWICE) hub_add(pc + e, crow[e] - crow0[e]);
        }
      } else {
        memcpy(pc, crow, sizeof(float) * (size_t)dim);
      }
      if (window_cache && i - window >= 0) ring_leave(&R, pos_row[i - window], syn0, dim, 0);
    }
    if (window_cache)
      for (int j = nf - window > 0 ? nf - window : 0; j < nf; ++j) ring_leave(&R, pos_row[j], syn0, dim, 0);
  }
  free(work);
  free(crow);
  free(crow0);
  free(R.cur);
  free(R.loaded);
  return pairs;
}

/* The batched trainer in hogwild mode (n2v_sgns_batched.hip).  The negatives of a position are drawn
 * once (the draw indices of relative position 0) and shared by its pairs; the position is trained from
 * one snapshot of its rows.  Sentences of fewer than 2 kept tokens train nothing.
 *   The context ring: 12 physical rows (2 * window + 2 <= 12) or 16, one per distinct word of positions
 *   i - window .. i + 1 + window, the lowest free row first.  Positions 0 .. window enter before
 *   position 0; position i + 1 + window enters before position i trains, position i - window leaves
 *   after it.  A row is loaded from syn0 when the first of its positions enters and goes back when the
 *   last leaves: syn0[w][e] += copy[e] - loaded[e] (atomic add; ctx_store = 1: syn0[w] = copy, the
 *   deterministic form, with which and hub_rows = 0 this function states what the oracle states).
 *   Per position: context rows = the physical rows with a position in the reduced window, ascending,
 *   multiplicity mu_c; target rows = the centre (label 1), then the distinct negatives != centre in draw
 *   order, multiplicity mu_t; C_old = the ring copies, T_old = the syn1neg rows as memory holds them.
 *   F[c][t] = four fma chains over d (k-step s = d mod (dim / 4) goes to chain s mod 4, within a step
 *             the planes d / (dim / 4) = 0 .. 3 in order), summed (c0 + c1) + (c2 + c3);
 *   G[c][t] = 0 if |F| >= 6, else ((label - sigma) * alpha) * (float)(mu_c * mu_t);
 *   target t:  acc = (t < hub_rows ? 0 : T_old[t][e]); acc = fma(G[c][t], C_old[c][e], acc) over the
 *              context rows in the order of the matrix cores' k-steps (step s, then group g: row 3g + s
 *              with 12 ring rows, 4g + s with 16); t < hub_rows: syn1neg[t][e] += acc (atomic add),
 *              else syn1neg[t][e] = acc;
 *   context c: copy[e] = fma chain from C_old[c][e] over the targets (step s, group g: target 2g + s
 *              when 1 + negative <= 8, else 4g + s) of G[c][t] * T_old[t][e].
 * mutation: MUT_BOUNDARY only.  Returns the pairs trained, -1 for arguments the kernel refuses. */
int64_t n2v_sgns_hub_cpu_train_batched(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0,
                                       float *syn1neg, const uint32_t *cum_table, const uint32_t *sample_int,
                                       const float *exp_table, int64_t n_vocab, int64_t sentence_base, uint64_t seed,
                                       int32_t dim, int32_t window, int32_t negative, float alpha, int32_t hub_rows,
                                       int32_t ctx_store, int32_t mutation) {
  if (walk_len < 1 || walk_len > 256 || (dim != 64 && dim != 128 && dim != 256) || window < 1 ||
      2 * window + 2 > 16 || negative < 1 || negative > 15 || n_vocab < 1 || hub_rows < 0)
    return -1;
  const int Q = dim / 4;
  const int rrows = 2 * window + 2 <= 12 ? 12 : 16;
  const int KC = rrows == 12 ? 3 : 4;
  const int KT = 1 + negative <= 8 ? 2 : 4;
  const int hub_end = mutation == MUT_BOUNDARY ? hub_rows + 1 : hub_rows;
  const uint32_t domain = cum_table[n_vocab - 1];
  int32_t sent[256], red[256];
  int pos_row[256];
  Ring R;
  R.cur = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  R.loaded = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  float *cold = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  float *told = (float *)malloc(sizeof(float) * (size_t)dim * 16);
  int64_t pairs = 0;
  for (int64_t r = 0; r < n_walks; ++r) {
    const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
    const int nf = prepare(walks + r * walk_len, walk_len, n_vocab, sample_int, hs, window, sent, red);
    if (nf < 2) continue;
    for (int k = 0; k < 16; ++k) R.ref[k] = 0;
    for (int j = 0; j <= window && j < nf; ++j) pos_row[j] = ring_enter(&R, sent[j], syn0, dim);
    for (int i = 0; i < nf; ++i) {
      const int32_t centre = sent[i];
      int lo = i - window + red[i];
      if (lo < 0) lo = 0;
      int hi = i + window + 1 - red[i];
      if (hi > nf) hi = nf;
      if (i + 1 + window < nf) pos_row[i + 1 + window] = ring_enter(&R, sent[i + 1 + window], syn0, dim);
      /* context rows: physical rows in ascending order */
      int mult[16], urow[16], umult[16], nu = 0, npairs = 0;
      for (int k = 0; k < 16; ++k) mult[k] = 0;
      for (int j = lo; j < hi; ++j)
        if (j != i) {
          ++mult[pos_row[j]];
          ++npairs;
        }
      for (int k = 0; k < 16; ++k)
        if (mult[k] > 0) {
          urow[nu] = k;
          umult[nu++] = mult[k];
        }
      if (nu > 0) {
        int32_t tword[16];
        int tmult[16], nt = 1;
        tword[0] = centre;
        tmult[0] = 1;
        for (int d = 0; d < negative; ++d) {
          const uint64_t idx = 2ULL * (uint64_t)walk_len + ((uint64_t)i * 2ULL * (uint64_t)window) * (uint64_t)negative +
                               (uint64_t)d;
          const int32_t t = bisect_left(cum_table, n_vocab, (uint32_t)((draw(hs, idx) >> 16) % (uint64_t)domain));
          if (t == centre) continue;
          int k = 1;
          while (k < nt && tword[k] != t) ++k;
          if (k < nt) {
            ++tmult[k];
          } else {
            tword[nt] = t;
            tmult[nt++] = 1;
          }
        }
        /* the snapshot */
        for (int u = 0; u < nu; ++u) memcpy(cold + (size_t)u * dim, R.cur + (size_t)urow[u] * dim, sizeof(float) * (size_t)dim);
        for (int t = 0; t < nt; ++t) memcpy(told + (size_t)t * dim, syn1neg + (int64_t)tword[t] * dim, sizeof(float) * (size_t)dim);
        float G[16][16];
        for (int u = 0; u < nu; ++u)
          for (int t = 0; t < nt; ++t) {
            const float *a = cold + (size_t)u * dim, *b = told + (size_t)t * dim;
            float ch[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int s = 0; s < Q; ++s)
              for (int p = 0; p < 4; ++p) ch[s & 3] = fmaf(a[p * Q + s], b[p * Q + s], ch[s & 3]);
            const float f = (ch[0] + ch[1]) + (ch[2] + ch[3]);
            float g = 0.0f;
            if (!(f <= -6.0f || f >= 6.0f))
              g = (((t == 0 ? 1.0f : 0.0f) - exp_table[(int)((f + 6.0f) * 83.0f)]) * alpha) * (float)(umult[u] * tmult[t]);
            G[u][t] = g;
          }
        for (int t = 0; t < nt; ++t) {
          float *row = syn1neg + (int64_t)tword[t] * dim;
          const int hub = tword[t] < hub_end;
          for (int e = 0; e < dim; ++e) {
            float acc = hub ? 0.0f : told[(size_t)t * dim + e];
            for (int s = 0; s < KC; ++s)
              for (int g = 0; g < 4; ++g) {
                const int u = KC * g + s;
                if (u < nu) acc = fmaf(G[u][t], cold[(size_t)u * dim + e], acc);
              }
            if (hub)
              hub_add(row + e, acc);
            else
              row[e] = acc;
          }
        }
        for (int u = 0; u < nu; ++u) {
          float *row = R.cur + (size_t)urow[u] * dim;
          for (int e = 0; e < dim; ++e) {
            float acc = cold[(size_t)u * dim + e];
            for (int s = 0; s < KT; ++s)
              for (int g = 0; g < 4; ++g) {
                const int t = KT * g + s;
                if (t < nt) acc = fmaf(G[u][t], told[(size_t)t * dim + e], acc);
              }
            row[e] = acc;
          }
        }
        pairs += npairs;
      }
      if (i - window >= 0) ring_leave(&R, pos_row[i - window], syn0, dim, ctx_store);
    }
    for (int j = nf - window > 0 ? nf - window : 0; j < nf; ++j) ring_leave(&R, pos_row[j], syn0, dim, ctx_store);
  }
  free(R.cur);
  free(R.loaded);
  free(cold);
  free(told);
  return pairs;
}
