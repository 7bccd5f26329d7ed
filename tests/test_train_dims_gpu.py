"""The trainers in deterministic mode, bit for bit against their CPU restatements, at the dimensions
the other files leave out: the per-element tail of load_row / store_row in every VEC instance (129 ..
255, 257 .. 511, 513 .. 1023; in HS these use plain accesses, below 128 the agent-scope ones), the sizes people pick
for word2vec (200, 300), the smallest rows, and SGNS at 1024.  In SGNS these ranges also change the
negatives in flight (KP = 5 up to dim 256, 3 up to 512, 1 above: sgns_kernel) and switch the lookahead
off above 512; `negative` > KP runs the further groups of negatives and their `dup` reload.

Small-vocabulary corpora (60 to 300 tokens, as in test_sgns_gpu.py and test_hs_gpu.py): words repeat
inside a window all the time.
"""
import numpy as np
import pytest
import torch

from test_hs_gpu import _check_bits, _corpus, _model
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)
from test_sgns_gpu import _setup

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 3, 5, 15, 17, 33, 65, 127, 129, 200, 255, 257, 300, 511, 513, 768, 1000, 1023, 1024]


def _sgns_bits(oracle, dim, sample, window=5, negative=5):
    sgns, m, idx = _setup(60, 40, 21, dim, seed=5 + dim, sample=sample)
    m.window, m.negative = window, negative
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1neg.cpu().numpy().copy()
    n = 0
    for blk, alpha in ((0, 0.025), (1, 0.02)):  # two launches: sentence_base moves on
        m.train_block(idx, alpha, blk * idx.shape[0], deterministic=True)
        n += oracle.sgns_train(idx.cpu().numpy(), s0, s1, m.cum_table.cpu().numpy(),
                               None if m.sample_int is None else m.sample_int.cpu().numpy(),
                               sgns.exp_table(), len(m.vocab), blk * idx.shape[0], m.seed, dim, window, negative,
                               alpha)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n > 0
    g0, g1 = m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(g1).all()
    assert np.array_equal(g0.view(np.uint32), s0.view(np.uint32)), float(np.abs(g0 - s0).max())
    assert np.array_equal(g1.view(np.uint32), s1.view(np.uint32)), float(np.abs(g1 - s1).max())
    assert np.abs(s1).max() > 0


@pytest.mark.parametrize("sample", [0.0, 1e-2])
@pytest.mark.parametrize("dim", DIMS)
def test_sgns_deterministic_dimension_sweep(oracle, dim, sample):
    _sgns_bits(oracle, dim, sample)


@pytest.mark.parametrize("window,negative", [(5, 5), (2, 7), (7, 11)])
@pytest.mark.parametrize("dim", [200, 300, 1000])
def test_sgns_deterministic_more_negatives_than_in_flight(oracle, dim, window, negative):
    """negative > KP in each VEC class (KP = 5 at dim 200, 3 at 300, 1 at 1000): further groups of
    negatives, a negative repeated inside a group read back after its own update"""
    _sgns_bits(oracle, dim, 1e-2, window, negative)


@pytest.mark.parametrize("path_cache", [True, False])
@pytest.mark.parametrize("dim", DIMS)
def test_hs_deterministic_dimension_sweep(hs_cpu, dim, path_cache):
    walks = _corpus(300, 12, 40, 7 * dim + 1)
    m, idx = _model(walks, dim, 5, seed=dim + 5)
    launches = ((0, 0.025, None), (idx.shape[0], 0.02, None))
    assert _check_bits(hs_cpu, m, idx, launches, path_cache=path_cache) > 0
    assert np.abs(m.syn1.cpu().numpy()).max() > 0


@pytest.mark.parametrize("dim", [200, 300])
def test_hs_deterministic_per_row_rates(hs_cpu, dim):
    """row_alpha (Spark's schedule: a rate per row) at the word2vec sizes"""
    from node2vec_amd import hs

    walks = _corpus(200, 10, 30, dim)
    walks[0, ::4] = -1
    m, idx = _model(walks, dim, 5, seed=dim)
    words = (idx >= 0).sum(1).cpu().numpy()
    launches = [(ep * idx.shape[0], 0.025, hs.spark_row_alpha(words * 1500, ep, 2, 0.025)) for ep in range(2)]
    assert len({float(a) for _, _, ra in launches for a in ra}) > 2  # the rates really differ by row
    _check_bits(hs_cpu, m, idx, launches)
