/*
 * n2v_cbow_cpu.c -- single-thread CPU restatement of CBOW with negative sampling.
 *
 * TEST INFRASTRUCTURE ONLY: tests/test_cbow_*.py build it once per session with
 * the flags of tests/cpu_build.py (no contraction, no fast-math) and pin
 * node2vec_amd/csrc/n2v_cbow.hip to it bit for bit in deterministic mode.
 *
 * The algorithm is gensim 3.8 train_batch_cbow / fast_sentence_cbow_neg (gensim cannot run here;
 * this file is the pin).  Sentence preparation is that of the skip-gram kernel: tokens < 0 or
 * >= n_vocab dropped, subsampling with draw 2t, reduced window b = (draw(2t + 1) >> 32) % window for
 * raw position t.  For position i of the kept sentence (nf tokens, centre c = sent[i]):
 *   1. lo = max(0, i - window + b), hi = min(nf, i + window + 1 - b), count = hi - lo - 1;
 *      count == 0: nothing trained, nothing counted;
 *   2. neu1 = sum over m = lo .. hi - 1, m != i, ascending, of syn0[sent[m]] (fp32 adds in that
 *      order; a word that stands twice in the window is added twice);
 *   3. inv = 1.0f / (float)count; cbow_mean: neu1 *= inv;
 *   4. work = 0; d = 0 is target c with label 1, d >= 1 is target
 *      bisect_left(cum_table, (draw(2 * walk_len + i * negative + d - 1) >> 16) % cum_table[n_vocab - 1])
 *      with label 0, skipped when it equals c (one set of draws per position);
 *      f = wave_dot(neu1, syn1neg[target]); f <= -6 or f >= 6 skips;
 *      g = (label - exp_table[(int)((f + 6) * 83)]) * alpha;
 *      work = fmaf(g, syn1neg[target], work); syn1neg[target] = fmaf(g, neu1, syn1neg[target]);
 *   5. not cbow_mean: work *= inv;
 *   6. syn0[sent[m]] += work for the same m, ascending (a repeated word receives it twice);
 *   7. the count of trained positions grows by one.
 * hub_rows > 0 states the kernel's hogwild HUB FORM instead (0: the above, what deterministic mode runs):
 *   4'. a target below hub_rows takes an atomic add of the ROUNDED product,
 *       syn1neg[target][e] = syn1neg[target][e] + fl(g * neu1[e]), where the store form has one fmaf;
 *       work is computed from the row as it was read, as above;
 *   6'. a context word below hub_rows takes syn0[.][e] = syn0[.][e] + work[e] as an atomic add: one fp32
 *       addition onto what memory holds, which in order is the same value as the store.
 * An atomic add is one fp32 addition in program order (hub_add).  Compiled with -DN2V_HUB_CHECK it counts
 * operands that are nonzero subnormals, which a hardware fp32 atomic need not honour
 * (n2v_cbow_cpu_subnormals); tests/test_hub_form_host.py asserts there are none.  `mutation` is test-only:
 * 2 replaces the rounded product by fmaf, 3 treats row hub_rows itself as a hub, 4 lets the last lane
 * that owns elements of a ragged row skip its adds (the numbering of tests/cpu_sgns_hub/n2v_sgns_hub_cpu.c).
 * Deviations from gensim, deliberate and documented (DESIGN.md "CBOW"): the draws come from the
 * project's counter-based stream where gensim runs a linear congruential generator per thread; the
 * dot product is summed in the order of the wave64 kernel (lane l owns elements l*V .. l*V+V-1,
 * then a butterfly over lane distances 1 .. 32) where BLAS sdot leaves it unspecified; the seeded
 * initialisation.  The helpers below are copied from tests/cpu_hs/n2v_hs_cpu.c.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static inline uint64_t sentence_stream(uint64_t seed, uint64_t sentence_id) {
  return mix64(seed ^ mix64(sentence_id + 0xA0761D6478BD642FULL));
}

static inline uint64_t draw(uint64_t hs, uint64_t idx) {
  return mix64(hs + (idx + 1ULL) * 0xE7037ED1A0B428DBULL);
}

static int64_t subnormal_operands = 0;

/* operands of atomic adds that were nonzero subnormals since the last call; -1 without N2V_HUB_CHECK */
int64_t n2v_cbow_cpu_subnormals(void) {
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

static int vec_width(int dim) {
  int v = 1;
  while (64 * v < dim) v *= 2;
  return v;
}

static float wave_dot(const float *a, const float *b, int dim, int V) {
  float p[64], t[64];
  for (int l = 0; l < 64; ++l) {
    float acc = 0.0f;
    for (int v = 0; v < V; ++v) {
      int e = l * V + v;
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

static int64_t bisect_left(const uint32_t *a, int64_t n, uint32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* Trains rows [0, n_walks) in order, single thread: the contract of n2v_cbow_train on host
 * pointers.  Returns the trained positions, or -1 for arguments the kernel refuses.
 * stats (or NULL): [0] += windows that hold a word twice, [1] += negative draws equal to their
 * centre word -- what the tests assert about their own cases. */
int64_t n2v_cbow_cpu_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1neg,
                           const uint32_t *cum_table, const uint32_t *sample_int, const float *exp_table,
                           int64_t n_vocab, int64_t sentence_base, uint64_t seed, int32_t dim, int32_t window,
                           int32_t negative, float alpha, const float *row_alpha, int32_t cbow_mean,
                           int64_t *stats, int32_t hub_rows, int32_t mutation) {
  if (walk_len < 1 || walk_len > 256 || dim < 1 || dim > 1024 || window < 1 || window > 32 || negative < 1 ||
      negative > 32 || n_vocab < 1 || (cbow_mean != 0 && cbow_mean != 1) || hub_rows < 0)
    return -1;
  const int V = vec_width(dim);
  const int hub_end = mutation == 3 ? hub_rows + 1 : hub_rows; /* rows below it are hubs */
  const int add_end = (mutation == 4 && dim != 64 * V) ? (dim - 1) / V * V : dim;
  const uint32_t domain = cum_table[n_vocab - 1];
  int32_t sent[256], red[256];
  float *neu1 = (float *)malloc(sizeof(float) * (size_t)dim);
  float *work = (float *)malloc(sizeof(float) * (size_t)dim);
  int64_t trained = 0;
  for (int64_t r = 0; r < n_walks; ++r) {
    const float a = row_alpha ? row_alpha[r] : alpha;
    const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
    int nf = 0;
    for (int t = 0; t < walk_len; ++t) {
      const int32_t tok = walks[r * walk_len + t];
      if (tok < 0 || tok >= n_vocab) continue;
      if (sample_int && sample_int[tok] < (uint32_t)(draw(hs, 2ULL * (uint64_t)t) >> 32)) continue;
      sent[nf] = tok;
      red[nf] = (int32_t)((uint32_t)(draw(hs, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
      ++nf;
    }
    for (int i = 0; i < nf; ++i) {
      const int32_t c = sent[i];
      int lo = i - window + red[i];
      if (lo < 0) lo = 0;
      int hi = i + window + 1 - red[i];
      if (hi > nf) hi = nf;
      const int count = hi - lo - 1;
      if (count == 0) continue;
      memset(neu1, 0, sizeof(float) * (size_t)dim);
      memset(work, 0, sizeof(float) * (size_t)dim);
      int twice = 0;
      for (int m = lo; m < hi; ++m) {
        if (m == i) continue;
        const float *row = syn0 + (int64_t)sent[m] * dim;
        for (int e = 0; e < dim; ++e) neu1[e] = neu1[e] + row[e];
        for (int m2 = lo; m2 < m; ++m2)
          if (m2 != i && sent[m2] == sent[m]) twice = 1;
      }
      if (stats) stats[0] += twice;
      const float inv = 1.0f / (float)count;
      if (cbow_mean)
        for (int e = 0; e < dim; ++e) neu1[e] = neu1[e] * inv;
      for (int d = 0; d <= negative; ++d) {
        int32_t target;
        float label;
        if (d == 0) {
          target = c;
          label = 1.0f;
        } else {
          const uint64_t idx = 2ULL * (uint64_t)walk_len + (uint64_t)i * (uint64_t)negative + (uint64_t)(d - 1);
          target = (int32_t)bisect_left(cum_table, n_vocab, (uint32_t)((draw(hs, idx) >> 16) % (uint64_t)domain));
          if (target == c) {
            if (stats) stats[1] += 1;
            continue;
          }
          label = 0.0f;
        }
        float *row2 = syn1neg + (int64_t)target * dim;
        const float f = wave_dot(neu1, row2, dim, V);
        if (f <= -6.0f || f >= 6.0f) continue;
        const float g = (label - exp_table[(int)((f + 6.0f) * 83.0f)]) * a;
        const int hub = target < hub_end;
        for (int e = 0; e < dim; ++e) {
          const float r2 = row2[e];
          work[e] = fmaf(g, r2, work[e]);
          if (!hub || mutation == 2) {
            if (!hub || e < add_end) row2[e] = fmaf(g, neu1[e], r2);
          } else if (e < add_end) {
            hub_add(row2 + e, g * neu1[e]);
          }
        }
      }
      if (!cbow_mean)
        for (int e = 0; e < dim; ++e) work[e] = work[e] * inv;
      for (int m = lo; m < hi; ++m) {
        if (m == i) continue;
        float *row = syn0 + (int64_t)sent[m] * dim;
        if (sent[m] < hub_end) {
          for (int e = 0; e < add_end; ++e) hub_add(row + e, work[e]);
        } else {
          for (int e = 0; e < dim; ++e) row[e] = row[e] + work[e];
        }
      }
      ++trained;
    }
  }
  free(neu1);
  free(work);
  return trained;
}
