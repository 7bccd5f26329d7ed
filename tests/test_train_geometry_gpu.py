"""The hogwild launch of the trainers, bit for bit: many waves, several blocks, every wave_in_block.

Deterministic mode runs one wave in one block, so the bit-identity tests of test_hs_gpu.py and
test_sgns_gpu.py never touch the per-wave LDS carve-up (sent + wave_in_block * per_wave; in HS the
`orig` copy behind `cache` and the (1 + hogwild) factor that the kernel and the host's LDS size must
agree on), blocks of 4 waves, the sentence counter in pairs_out[1] or the resident_blocks cap.  The
corpora of tests/conflict_free.py make the racy mode schedule-independent: no two sentences write the
same row and the rows they share are saturated (never written), so ANY schedule computes what the CPU
restatement computes in order.  Each test first proves that under the restatement alone
(conflict_free.prove, also run without a GPU by test_train_geometry_cpu.py), then runs the same
launches with deterministic=False and the library's own wave rule and asks for the same bits.  One
run each: the argument does not depend on scheduling.

Not covered: real races (two waves on one row), and rows updated by atomic deltas -- SGNS hub_rows,
and the batched trainer (n2v_sgns_batched.hip), whose hogwild mode returns context rows as atomic adds
of (row - row as loaded) and target rows as atomic adds of their deltas: their rounding differs from
the fmaf chain of its oracle, so it has no exact many-wave test here.  The default kernel's window
cache also writes back by atomic add; conflict_free.sgns_case keeps that add exact.
"""
import numpy as np
import pytest
import torch

import conflict_free as cf
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)
from test_train_geometry_cpu import HS_DIMS, HS_VARIANTS, SGNS_VARIANTS

pytestmark = pytest.mark.gpu

MIN_WAVES = 8  # at least two blocks of 4 waves: every wave_in_block, blockIdx > 0


def _identity_vocab(n):
    from node2vec_amd import sgns

    return sgns.Vocab(torch.arange(n).cuda(), torch.full((n,), 7, dtype=torch.int64).cuda(),
                      torch.arange(n, dtype=torch.int32).cuda())


def _same_bits(name, got, want):
    """bit equality, and on a failure which rows and elements differ: what a fault is located from"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        rows = np.unique(bad[:, 0])
        pytest.fail(f"{name}: {len(bad)} elements in {len(rows)} rows differ; rows {rows[:16].tolist()}, "
                    f"elements of the first {bad[bad[:, 0] == rows[0], 1][:16].tolist()}, "
                    f"largest difference {float(np.abs(got - want).max())}", pytrace=False)


def _compare(case, want, got0, got1, pairs, waves):
    w0, w1, n = want
    print(case.name, "waves", waves, "pairs", pairs)
    assert waves >= MIN_WAVES, waves
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
    waves.  The batched trainer is left out: see the module docstring."""
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
