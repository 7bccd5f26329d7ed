"""The precondition of tests/test_train_geometry_gpu.py, with no GPU: every corpus that file trains in
hogwild mode really is conflict-free under the CPU restatement alone (tests/conflict_free.py: the
shared rows keep their bits, no row is changed by two sentences, the per-sentence runs merged are the
joint run bit for bit), and the proof notices a case that is not."""
import numpy as np
import pytest

import conflict_free as cf
from test_cbow_host import cbow_cpu  # noqa: F401  (session fixture: the CBOW restatement)
from test_hs_host import hs_cpu, lib  # noqa: F401  (session fixtures: the restatement, the built library)

HS_DIMS = [64, 128, 256, 300, 1024]
SGNS_DIMS = [64, 128, 200, 512]
# CBOW: a full and a ragged dimension among them for every VEC of interest (1: 64; 2: 100, 128; 4: 256;
# 8: 300; 16: 1024)
CBOW_DIMS = [64, 100, 128, 256, 300, 1024]
# (sentences = waves, out-of-vocabulary tokens): the plain case, more sentences than waves, -1 tokens
# HS: the depth whose nodes head the sentences.  Depth 3 (8 sentences of 128 words, 8 waves) puts a row that
# trains among the 4 rows a hogwild wave caches at dim 256; at dim 300 / 1024 it caches 2 / 1 rows, which any two
# sentences share, so there the cached rows can only be saturated ones
HS_VARIANTS = [(5, False), (6, False), (5, True), (3, False)]
SGNS_VARIANTS = [(32, False), (64, False), (32, True)]
# CBOW: and 8 sentences, which the GPU test runs on one short block of 3 waves
CBOW_VARIANTS = [(32, False), (64, False), (32, True), (8, False)]
# negative = 32: the only setting at which a wave writes all 64 words of its `neg` region in LDS, the last
# words of its share (at negative = 5 the draws of 12 positions fill 60)
CBOW_ALL_LANES = [(64, 32, False), (64, 8, False)]


@pytest.mark.parametrize("depth,oov", HS_VARIANTS)
@pytest.mark.parametrize("dim", HS_DIMS)
def test_hs_corpus_is_conflict_free(lib, hs_cpu, dim, depth, oov):
    case = cf.hs_case(hs_cpu, dim, depth, oov)
    assert case.walks.shape == (2 ** depth, cf.TOKENS) and bool((case.walks < 0).any()) == oov
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() > 0.8  # f >= 6.4 at the top nodes throughout
    print(case.name, "pairs", pairs, "min syn0[:, 0]", float(j0[:, 0].min()))


@pytest.mark.parametrize("sentences,oov", SGNS_VARIANTS)
@pytest.mark.parametrize("dim", SGNS_DIMS)
def test_sgns_corpus_is_conflict_free(oracle, dim, sentences, oov):
    case = cf.sgns_case(oracle, dim, sentences, oov)
    assert case.walks.shape == (sentences, cf.TOKENS) and bool((case.walks < 0).any()) == oov
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() >= 1.0  # label-1 updates only raise it: f >= 8 at the sink
    # no element moves by half of itself: the window cache's atomic write-back is then exact (sgns_case)
    move = np.abs(j0 - case.m0) / np.abs(case.m0)
    assert move.max() < 0.5, float(move.max())
    # the sink took every negative draw: no other row of syn1neg moved unless a sentence holds its word
    in_corpus = np.zeros(cf.V_WORDS + 1, bool)
    in_corpus[case.walks[case.walks >= 0]] = True
    moved = (j1 != case.m1).any(1)
    assert not moved[~in_corpus].any() and moved[in_corpus].all()
    print(case.name, "pairs", pairs)


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("sentences,oov", CBOW_VARIANTS)
@pytest.mark.parametrize("dim", CBOW_DIMS)
def test_cbow_corpus_is_conflict_free(cbow_cpu, dim, sentences, oov, cbow_mean):
    case = cf.cbow_case(cbow_cpu, dim, sentences, oov, cbow_mean)
    assert case.walks.shape == (sentences, cf.TOKENS) and bool((case.walks < 0).any()) == oov
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() >= 1.0  # only raised: the mean (or sum) of the context stays >= 1, f >= 8 at the sink
    # the sink took every draw: no other row of syn1neg moved unless a sentence holds its word
    in_corpus = np.zeros(cf.V_WORDS + 1, bool)
    in_corpus[case.walks[case.walks >= 0]] = True
    moved = (j1 != case.m1).any(1)
    assert not moved[~in_corpus].any() and moved[in_corpus].all()
    print(case.name, "positions", pairs, "max |syn0|", float(np.abs(j0).max()))


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("dim,sentences,oov", CBOW_ALL_LANES)
def test_cbow_corpus_with_32_negatives_is_conflict_free(cbow_cpu, dim, sentences, oov, cbow_mean):
    case = cf.cbow_case(cbow_cpu, dim, sentences, oov, cbow_mean, negative=32)
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() >= 1.0
    in_corpus = np.zeros(cf.V_WORDS + 1, bool)
    in_corpus[case.walks[case.walks >= 0]] = True
    moved = (j1 != case.m1).any(1)
    assert not moved[~in_corpus].any() and moved[in_corpus].all()


def test_the_proof_notices_unsaturated_shared_rows(lib, hs_cpu, oracle, cbow_cpu):
    """top HS rows of 5 instead of 8 (f = 5: trained by every sentence), and likewise the SGNS sink and
    the CBOW sink (f = 5 * count under cbow_mean 0, 5 at count 1; f = 5 under cbow_mean 1)"""
    with pytest.raises(AssertionError):
        cf.prove(cf.hs_case(hs_cpu, 64, 5, False, saturated=5.0))
    with pytest.raises(AssertionError):
        cf.prove(cf.sgns_case(oracle, 64, 32, False, saturated=5.0))
    for cbow_mean in (0, 1):
        with pytest.raises(AssertionError):
            cf.prove(cf.cbow_case(cbow_cpu, 64, 32, False, cbow_mean, saturated=5.0))


def test_the_proof_notices_a_shared_word(lib, hs_cpu, oracle, cbow_cpu):
    """one word of sentence 0 put into sentence 1: two sentences change its rows"""
    for case in (cf.hs_case(hs_cpu, 64, 5, False), cf.sgns_case(oracle, 64, 32, False),
                 cf.cbow_case(cbow_cpu, 64, 32, False, 0), cf.cbow_case(cbow_cpu, 64, 32, False, 1)):
        case.walks[1, 7] = case.walks[0, 3]
        with pytest.raises(AssertionError):
            cf.prove(case)
