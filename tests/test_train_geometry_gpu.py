"""The hogwild launch of the trainers, bit for bit: many waves, several blocks, every wave_in_block.

Deterministic mode runs one wave in one block, so the bit-identity tests of test_hs_gpu.py,
test_sgns_gpu.py and test_cbow_gpu.py never touch the per-wave LDS carve-up (sent + wave_in_block *
per_wave; in HS the `orig` copy behind `cache` and the (1 + hogwild) factor that the kernel and the
host's LDS size must agree on; in CBOW the bucket table in front of the waves' regions, there without
a cum_index and absent with one), blocks of 4 waves, a short block of fewer (CBOW: waves < 4), the
sentence counter in pairs_out[1] or the resident_blocks cap.  CBOW runs here with plain stores
everywhere (hub_rows = 0).  The
corpora of tests/conflict_free.py make the racy mode schedule-independent: no two sentences write the
same row and the rows they share are saturated (never written), so ANY schedule computes what the CPU
restatement computes in order.  Each test first proves that under the restatement alone
(conflict_free.prove, also run without a GPU by test_train_geometry_cpu.py), then runs the same
launches with deterministic=False and the library's own wave rule and asks for the same bits.  One
run each: the argument does not depend on scheduling.

Rows updated by atomic deltas -- SGNS and CBOW hub_rows, the window cache's write-back, and the batched
trainer (n2v_sgns_batched.hip), whose hogwild mode returns context rows as atomic adds of (row - row as
loaded) and hub target rows as atomic adds of their deltas -- round differently from the store form these
restatements state.  tests/test_hub_form_gpu.py pins them bit for bit against restatements of the hub
form: every trainer on one wave, and SGNS and CBOW hub_rows on many waves over the corpora used here.
(The default kernel's window cache also writes back by atomic add; conflict_free.sgns_case keeps that
add exact, so this file's store-form oracle holds for it.)

The batched trainer's hogwild mode on many waves has a file of its own, tests/test_batched_geometry_gpu.py:
its kernel rewrites the saturated sink rows at every position, so it runs under the weaker precondition
that a shared row only ever receives the bits it holds (tests/conflict_free.py).

Not covered: real races (two waves on one row), which stay a statistical claim.
"""
import numpy as np
import pytest
import torch

import conflict_free as cf
from same_bits import same_bits as _same_bits
from test_cbow_host import cbow_cpu  # noqa: F401  (the session fixture that builds the CBOW restatement)
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)
from test_train_geometry_cpu import CBOW_ALL_LANES, CBOW_DIMS, CBOW_VARIANTS, HS_DIMS, HS_VARIANTS, SGNS_VARIANTS

pytestmark = pytest.mark.gpu

MIN_WAVES = 8  # at least two blocks of 4 waves: every wave_in_block, blockIdx > 0


def _identity_vocab(n):
    from node2vec_amd import sgns

    return sgns.Vocab(torch.arange(n).cuda(), torch.full((n,), 7, dtype=torch.int64).cuda(),
                      torch.arange(n, dtype=torch.int32).cuda())


def _compare(case, want, got0, got1, pairs, waves, exact_waves=None):
    w0, w1, n = want
    print(case.name, "waves", waves, "pairs", pairs)
    if exact_waves is None:
        assert waves >= MIN_WAVES, waves
    else:
        assert waves == exact_waves, waves
    assert pairs == n
    _same_bits("syn0", got0, w0)
    _same_bits("syn1", got1, w1)


@pytest.mark.parametrize("path_cache", [True, False])
@pytest.mark.parametrize("depth,oov", HS_VARIANTS)
@pytest.mark.parametrize("dim", HS_DIMS)
def test_hs_hogwild_bit_identical_on_conflict_free_corpus(hs_cpu, dim, depth, oov, path_cache):
    """dims 64 / 128 / 256 / 300 / 1024: hogwild path caches of 16 / 8 / 4 / 2 / 1 rows against paths of
    10 nodes.  depth 6: 64 sentences on 16 waves, so every wave takes several through the counter.
    depth 3: 8 sentences on 8 waves, and a row that trains among the cached ones up to dim 256 (at 300 and
    1024 the 2 / 1 cached rows are shared by any two sentences, so there they are saturated rows: what
    is pinned is that they come back from LDS unharmed)."""
    from node2vec_amd import hs

    case = cf.hs_case(hs_cpu, dim, depth, oov)
    want = cf.prove(case)
    m = hs.HsModel(_identity_vocab(cf.V_WORDS), dim, cf.WINDOW, seed=cf.SEED)
    t = case.extra["tree"]
    assert np.array_equal(m.tree.points, t.points) and np.array_equal(m.tree.codes, t.codes)
    m.syn0.copy_(torch.from_numpy(case.m0))
    m.syn1.copy_(torch.from_numpy(case.m1))
    m.path_cache = path_cache
    if depth == 6:
        m.max_waves = 16
    idx = torch.from_numpy(case.walks).cuda()
    for base, alpha in case.launches():
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    assert m.hogwild_waves_used <= (16 if depth == 6 else 32)  # depth 6: four sentences per wave
    _compare(case, want, m.syn0.cpu().numpy(), m.syn1.cpu().numpy(), int(m.pairs.item()), m.hogwild_waves_used)


# (dim, window cache): the default kernel; the LDS ring of the window's syn0 rows where it fits
SGNS_CONFIGS = [(64, 0), (128, 0), (200, 0), (512, 0), (64, 1), (128, 1)]


@pytest.mark.parametrize("sentences,oov", SGNS_VARIANTS)
@pytest.mark.parametrize("dim,window_cache", SGNS_CONFIGS)
def test_sgns_hogwild_bit_identical_on_conflict_free_corpus(oracle, dim, window_cache, sentences, oov):
    """the default kernel, plain stores everywhere (hub_rows = 0, sample = 0).  64 sentences run on 16
    waves.  The batched trainer: tests/test_batched_geometry_gpu.py (see the module docstring)."""
    from node2vec_amd import _lib, sgns

    case = cf.sgns_case(oracle, dim, sentences, oov)
    want = cf.prove(case)
    n_vocab = cf.V_WORDS + 1
    m = sgns.SgnsModel(_identity_vocab(n_vocab), dim, cf.WINDOW, cf.NEGATIVE, seed=cf.SEED, sample=0.0)
    m.syn0.copy_(torch.from_numpy(case.m0))
    m.syn1neg.copy_(torch.from_numpy(case.m1))
    # the noise distribution of the case, and the bucket index rebuilt over it
    m.cum_table.copy_(torch.from_numpy(cf.sgns_cum_table()))
    _lib.check(_lib.load().n2v_cum_index_build(m.cum_table.data_ptr(), n_vocab, m.cum_index_bits,
                                               m.cum_index.data_ptr(), _lib.current_stream_ptr()),
               "n2v_cum_index_build")
    m.hub_rows = 0
    m.window_cache = window_cache
    if sentences == 64:
        m.max_waves = 16
    idx = torch.from_numpy(case.walks).cuda()
    waves = m.hogwild_waves(idx.shape[0], idx.shape[1])
    assert waves <= (16 if sentences == 64 else 32)  # 64 sentences: four per wave
    for base, alpha in case.launches():
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    _compare(case, want, m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy(), int(m.pairs.item()), waves)


# (dim, use_cum_index): with a cum_index the waves' LDS regions follow the sigmoid table directly, without
# one the bucket table lies between -- both layouts at a full and at a ragged dimension
CBOW_CONFIGS = [(64, True), (64, False), (100, False), (128, True), (256, False), (300, True), (300, False),
                (1024, True)]


def test_cbow_configs_cover_what_they_claim():
    assert [d for d, _ in CBOW_CONFIGS if d not in CBOW_DIMS] == [] and {d for d, _ in CBOW_CONFIGS} == set(CBOW_DIMS)
    for dim in (64, 300):
        assert {u for d, u in CBOW_CONFIGS if d == dim} == {True, False}
    full = {u for d, u in CBOW_CONFIGS if d in (64, 128, 256, 1024)}
    assert full == {True, False} == {u for d, u in CBOW_CONFIGS if d in (100, 300)}


def _cbow_hogwild(case, dim, use_cum_index, sentences, cbow_mean, negative):
    from node2vec_amd import _lib, sgns

    want = cf.prove(case)
    n_vocab = cf.V_WORDS + 1
    m = sgns.SgnsModel(_identity_vocab(n_vocab), dim, cf.WINDOW, negative, seed=cf.SEED, sample=0.0, sg=0,
                       cbow_mean=cbow_mean, use_cum_index=use_cum_index)
    assert (m.cum_index is not None) == use_cum_index
    m.syn0.copy_(torch.from_numpy(case.m0))
    m.syn1neg.copy_(torch.from_numpy(case.m1))
    # the noise distribution of the case, and the bucket index rebuilt over it
    m.cum_table.copy_(torch.from_numpy(cf.sgns_cum_table()))
    if use_cum_index:
        _lib.check(_lib.load().n2v_cum_index_build(m.cum_table.data_ptr(), n_vocab, m.cum_index_bits,
                                                   m.cum_index.data_ptr(), _lib.current_stream_ptr()),
                   "n2v_cum_index_build")
    m.hub_rows = 0
    exact = None
    if sentences == 64:
        m.max_waves = exact = 16
    elif sentences == 8:
        m.max_waves = exact = 3
    idx = torch.from_numpy(case.walks).cuda()
    waves = m.hogwild_waves(idx.shape[0], idx.shape[1])  # read back: max_waves, whole blocks, the occupancy cap
    assert waves <= 32
    for base, alpha in case.launches():
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    _compare(case, want, m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy(), int(m.pairs.item()), waves, exact)


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("sentences,oov", CBOW_VARIANTS)
@pytest.mark.parametrize("dim,use_cum_index", CBOW_CONFIGS)
def test_cbow_hogwild_bit_identical_on_conflict_free_corpus(cbow_cpu, dim, use_cum_index, sentences, oov, cbow_mean):
    """n2v_cbow.hip with plain stores everywhere (hub_rows = 0, sample = 0).  32 sentences run under the
    library's own rule (at least 8 waves: two blocks of 4), 64 sentences on 16 waves, so every wave takes
    several through the counter, and 8 sentences on ONE block of 3 waves (max_waves = 3: the launch
    whose block is shorter than 4 waves while the LDS is sized for 4)."""
    case = cf.cbow_case(cbow_cpu, dim, sentences, oov, cbow_mean)
    _cbow_hogwild(case, dim, use_cum_index, sentences, cbow_mean, cf.NEGATIVE)


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("use_cum_index", [True, False])
@pytest.mark.parametrize("dim,sentences,oov", CBOW_ALL_LANES)
def test_cbow_hogwild_with_32_negatives(cbow_cpu, dim, sentences, oov, use_cum_index, cbow_mean):
    """negative = 32: every batch of draws writes all 64 words of the wave's `neg` region, so the END of a
    wave's share of the LDS is in use (at negative = 5 its last 4 words are never touched, and a share
    4 words short would go unnoticed): a neighbour's tokens there, or the sink where a token was, change
    the rows trained"""
    case = cf.cbow_case(cbow_cpu, dim, sentences, oov, cbow_mean, negative=32)
    _cbow_hogwild(case, dim, use_cum_index, sentences, cbow_mean, 32)
