/*
 * n2v_hs_cpu.c -- single-thread CPU restatement of skip-gram hierarchical softmax.
 *
 * TEST INFRASTRUCTURE ONLY: tests/test_hs_*.py build it once per session with the flags of
 * tests/cpu_build.py (no contraction, no fast-math: the oracle's flags) and pin
 * node2vec_amd/csrc/n2v_hs.hip to it bit for bit in deterministic mode.
 *
 * The algorithm is word2vec.c / Spark MLlib Word2Vec skip-gram with hierarchical softmax, as
 * published (Spark cannot run here; this file is the pin):
 *   - vocabulary: sgns.build_vocab (descending count, ties by ascending id); tokens < 0 or
 *     >= n_vocab are dropped from a row before windowing (the host has already cut sentences
 *     into rows of at most maxSentenceLength in-vocabulary tokens);
 *   - Huffman tree: word2vec.c CreateBinaryTree (n2v_hs_tree_build): two queues, pos1 descending
 *     over the leaves, pos2 ascending over the merged nodes, strict `<` (a tie takes the merged
 *     node), binary[min2i] = 1, inner node V + a is syn1 row a, point[0] = V - 2 is the root,
 *     codes stored root first (bit d of codes[w]); the unmerged-slot sentinel exceeds any count;
 *     V = 1 gives code length 0 and no training (word2vec.c would index syn1 row -1);
 *   - pairs: per centre position i a reduced window b in [0, window) is drawn; the contexts are
 *     j in [i - window + b, i + window - b], j != i; for each context the CENTRE word's path is
 *     run against the CONTEXT row: f = dot(syn0[ctx], syn1[point[d]]); |f| >= 6 skips the node;
 *     g = (1 - code[d] - EXP_TABLE[(int)((f + 6) * 83)]) * alpha; neu1e += g * syn1[point[d]];
 *     syn1[point[d]] += g * syn0[ctx]; after the path syn0[ctx] += neu1e.  No subsampling, no
 *     negatives, all fp32;
 *   - learning rate: one fp32 value per row (row_alpha, computed by the host: hs.spark_row_alpha),
 *     or `alpha` for every row.
 * Deviations, deliberate and documented (DESIGN.md "Hierarchical softmax"): the window draws come
 * from the project's counter-based stream -- sentence_stream(seed, sentence id), draw index
 * 2 t + 1 for raw position t, as the SGNS kernel draws them -- where Spark uses one XORShift
 * generator per partition; the dot product is summed in the order of the wave64 kernel (lane l
 * owns elements l*V .. l*V+V-1, then a butterfly over lane distances 1 .. 32) where BLAS sdot
 * leaves it unspecified.  The helpers below are copied from oracle/n2v_oracle_sgns.c.
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

/* The reduced window of every in-vocabulary position of row r (what the kernel draws), for the
 * tests' float64 restatement: red_out[k] for the k-th kept token; returns the number kept. */
int n2v_hs_cpu_windows(const int32_t *walks, int64_t r, int32_t walk_len, int64_t n_vocab, int64_t sentence_base,
                       uint64_t seed, int32_t window, int32_t *red_out) {
  const uint64_t hs = sentence_stream(seed, (uint64_t)(sentence_base + r));
  int nf = 0;
  for (int t = 0; t < walk_len; ++t) {
    int32_t tok = walks[r * walk_len + t];
    if (tok < 0 || tok >= n_vocab) continue;
    red_out[nf++] = (int32_t)((uint32_t)(draw(hs, 2ULL * (uint64_t)t + 1ULL) >> 32) % (uint32_t)window);
  }
  return nf;
}

/* Trains rows [0, n_walks) in order, single thread: the contract of n2v_hs_train on host
 * pointers.  Returns the pairs formed, or -1 for arguments the kernel refuses. */
int64_t n2v_hs_cpu_train(const int32_t *walks, int64_t n_walks, int32_t walk_len, float *syn0, float *syn1,
                         const int64_t *path_off, const int32_t *points, const uint64_t *codes,
                         const float *exp_table, int64_t n_vocab, int64_t sentence_base, uint64_t seed,
                         int32_t dim, int32_t window, float alpha, const float *row_alpha) {
  if (walk_len < 1 || walk_len > 256 || dim < 1 || dim > 1024 || window < 1 || window > 32 || n_vocab < 1)
    return -1;
  const int V = vec_width(dim);
  int32_t sent[256], red[256];
  float *neu1e = (float *)malloc(sizeof(float) * (size_t)dim);
  int64_t pairs = 0;
  for (int64_t r = 0; r < n_walks; ++r) {
    const float a = row_alpha ? row_alpha[r] : alpha;
    const int nf = n2v_hs_cpu_windows(walks, r, walk_len, n_vocab, sentence_base, seed, window, red);
    int k = 0;
    for (int t = 0; t < walk_len; ++t) {
      int32_t tok = walks[r * walk_len + t];
      if (tok >= 0 && tok < n_vocab) sent[k++] = tok;
    }
    for (int i = 0; i < nf; ++i) {
      const int32_t centre = sent[i];
      const int64_t o = path_off[centre];
      const int len = (int)(path_off[centre + 1] - o);
      const uint64_t code = codes[centre];
      int lo = i - window + red[i];
      if (lo < 0) lo = 0;
      int hi = i + window + 1 - red[i];
      if (hi > nf) hi = nf;
      for (int j = lo; j < hi; ++j) {
        if (j == i) continue;
        ++pairs;
        float *row1 = syn0 + (int64_t)sent[j] * dim;
        memset(neu1e, 0, sizeof(float) * (size_t)dim);
        for (int d = 0; d < len; ++d) {
          float *row2 = syn1 + (int64_t)points[o + d] * dim;
          const float f = wave_dot(row1, row2, dim, V);
          if (f <= -6.0f || f >= 6.0f) continue;
          const int bit = (int)((code >> d) & 1ULL);
          const float g = ((float)(1 - bit) - exp_table[(int)((f + 6.0f) * 83.0f)]) * a;
          for (int e = 0; e < dim; ++e) {
            const float r2 = row2[e];
            neu1e[e] = fmaf(g, r2, neu1e[e]);
            row2[e] = fmaf(g, row1[e], r2);
          }
        }
        for (int e = 0; e < dim; ++e) row1[e] = row1[e] + neu1e[e];
      }
    }
  }
  free(neu1e);
  return pairs;
}
