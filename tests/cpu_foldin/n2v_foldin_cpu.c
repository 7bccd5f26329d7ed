/*
 * n2v_foldin_cpu.c -- single-thread CPU restatement of fold-in (DESIGN.md "Fold-in").
 *
 * TEST INFRASTRUCTURE ONLY: tests/test_foldin_*.py build it once per session with the flags of
 * tests/cpu_build.py (no contraction, no fast-math) and pin node2vec_amd/csrc/n2v_foldin.hip to it bit for bit.
 *
 * The contract.  A trained skip-gram negative-sampling model is frozen: syn1neg, the tables and the rows of every
 * known word are only read.  Tokens in [0, n_vocab) are known words, tokens in [n_vocab, n_vocab + n_new) are new
 * vertices (new index tok - n_vocab), any other token is dropped.  For walk r:
 *   1. the stream is sentence_stream(seed, sentence_base + r); a known token at raw position t is kept unless
 *      sample_int[tok] < draw(2t) >> 32 (a NEW token is always kept: sample_int has no entry for it); a kept token
 *      has the reduced window b = (draw(2t + 1) >> 32) % window; compaction preserves order (nf tokens);
 *   2. for centre position i and context position j != i with lo <= j < hi (lo = max(0, i - window + b_i),
 *      hi = min(nf, i + window + 1 - b_i)) the pair is trained when sent[j] is new AND sent[i] is known;
 *   3. one pair, on row1 = new_rows[sent[j] - n_vocab] with centre c = sent[i]:  work = 0;
 *      f = wave_dot(row1, syn1neg[c]); unless f <= -6 or f >= 6: g = (1 - exp[(int)((f + 6) * 83)]) * alpha,
 *      work = fmaf(g, syn1neg[c], work);  then for d = 0 .. K - 1 the target
 *      bisect_left(cum_table, (draw(2 * len + (i * 2 * window + rel) * K + d) >> 16) % cum_table[n_vocab - 1]),
 *      rel = j - i + window - (j > i), skipped when it equals c, with g = (0 - exp[...]) * alpha;
 *      finally row1 = row1 + work.  Nothing else is written.
 *   4. order: for one new vertex, (r, i, j) ascending.  Two new vertices never read each other's rows, so walking
 *      all pairs in (r, i, j) order -- what this file does -- is every vertex's own chain.
 * The dot product is summed in the order of the wave64 kernels (lane l owns elements l*V .. l*V+V-1, then a
 * butterfly over lane distances 1 .. 32).  The helpers are copied from tests/cpu_cbow/n2v_cbow_cpu.c.
 */
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

/* One pass over rows [0, n_walks) in order.  new_rows == NULL: only the listing.  records_out (or NULL): one
 * {new index, row, i | rel << 16, centre} per trainable pair, in (row, i, j) order.  Returns the trainable pairs, or
 * -1 for arguments the kernels refuse.  stats (or NULL): [0] += negative draws equal to their centre word,
 * [1] += targets skipped at the sigmoid cut (|f| >= 6), [2] += targets that read exp_table[0], [3] += targets
 * that read exp_table[995], the last entry any f below 6 reaches ((f + 6) * 83 < 996: entries 996 .. 999 of
 * word2vec's table are never read) -- what the tests assert about their own cases. */
int64_t n2v_foldin_cpu_pass(const int32_t *walks, int64_t n_walks, int32_t walk_len, int64_t n_vocab, int64_t n_new,
                            float *new_rows, const float *syn1neg, const uint32_t *cum_table,
                            const uint32_t *sample_int, const float *exp_table, int64_t sentence_base, uint64_t seed,
                            int32_t dim, int32_t window, int32_t negative, float alpha, const float *row_alpha,
                            int32_t *records_out, int64_t *stats) {
  if (walk_len < 1 || walk_len > 256 || dim < 1 || dim > 1024 || window < 1 || window > 32 || negative < 1 ||
      negative > 32 || n_vocab < 1 || n_new < 0 || n_vocab + n_new > (1ll << 31) || n_walks < 0)
    return -1;
  const int V = vec_width(dim);
  const uint32_t domain = cum_table ? cum_table[n_vocab - 1] : 1;
  int32_t sent[256], red[256];
  float *work = (float *)malloc(sizeof(float) * (size_t)dim);
  int64_t pairs = 0;
  for (int64_t r = 0; r < n_walks; ++r) {
    const float a = row_alpha ? row_alpha[r] : alpha;
    const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
    int nf = 0;
    for (int t = 0; t < walk_len; ++t) {
      const int32_t tok = walks[r * walk_len + t];
      if (tok < 0 || tok >= n_vocab + n_new) continue;
      if (tok < n_vocab && sample_int && sample_int[tok] < (uint32_t)(draw(hs, 2ULL * (uint64_t)t) >> 32)) continue;
      sent[nf] = tok;
      red[nf] = (int32_t)((uint32_t)(draw(hs, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
      ++nf;
    }
    for (int i = 0; i < nf; ++i) {
      const int32_t c = sent[i];
      if (c >= n_vocab) continue; /* a new vertex has no output row */
      int lo = i - window + red[i];
      if (lo < 0) lo = 0;
      int hi = i + window + 1 - red[i];
      if (hi > nf) hi = nf;
      for (int j = lo; j < hi; ++j) {
        if (j == i || sent[j] < n_vocab) continue; /* a known context word is frozen */
        const int rel = j - i + window - (j > i ? 1 : 0);
        if (records_out) {
          int32_t *rec = records_out + 4 * pairs;
          rec[0] = (int32_t)(sent[j] - n_vocab);
          rec[1] = (int32_t)r;
          rec[2] = i | (rel << 16);
          rec[3] = c;
        }
        ++pairs;
        if (!new_rows) continue;
        float *row1 = new_rows + (int64_t)(sent[j] - n_vocab) * dim;
        memset(work, 0, sizeof(float) * (size_t)dim);
        for (int d = -1; d < negative; ++d) {
          int32_t target;
          float label;
          if (d < 0) {
            target = c;
            label = 1.0f;
          } else {
            const uint64_t idx = 2ULL * (uint64_t)walk_len +
                                 ((uint64_t)i * 2ULL * (uint64_t)window + (uint64_t)rel) * (uint64_t)negative +
                                 (uint64_t)d;
            target = (int32_t)bisect_left(cum_table, n_vocab, (uint32_t)((draw(hs, idx) >> 16) % (uint64_t)domain));
            if (target == c) {
              if (stats) stats[0] += 1;
              continue;
            }
            label = 0.0f;
          }
          const float *row2 = syn1neg + (int64_t)target * dim;
          const float f = wave_dot(row1, row2, dim, V);
          if (f <= -6.0f || f >= 6.0f) {
            if (stats) stats[1] += 1;
            continue;
          }
          const int at = (int)((f + 6.0f) * 83.0f);
          if (stats) stats[2] += at == 0, stats[3] += at == 995;
          const float g = (label - exp_table[at]) * a;
          for (int e = 0; e < dim; ++e) work[e] = fmaf(g, row2[e], work[e]);
        }
        for (int e = 0; e < dim; ++e) row1[e] = row1[e] + work[e];
      }
    }
  }
  free(work);
  return pairs;
}
