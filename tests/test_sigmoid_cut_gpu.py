"""The sigmoid-table cut that the HS, SGNS, batched SGNS and CBOW trainers share, at its edges.

Every trainer skips a node or target when f <= -6 or f >= 6 and otherwise reads
exp_table[(int)((f + 6) * 83)].  The other bit-for-bit tests start from small random rows, so |f| stays
far from 6 and nothing tells `<=` from `<` or pins the table index at its first and last used entries.

Construction: every syn0 row is [1, 0, ..., 0] and every output row (syn1, syn1neg) is [x, 0, ..., 0], so
the first dot product of a launch is EXACTLY x for every dim and reduction order (all other terms are
0 * 0).  One sentence of two tokens per launch, window 1, deterministic mode.  The whole state is
compared bit for bit with the trainer's CPU witness, and the witness alone shows that the case hit what
it names: no output row changes exactly when |x| >= 6, and the two sides of a table-bin edge differ by
far more than their inputs do.
"""
import numpy as np
import pytest
import torch

from test_cbow_host import cbow_cpu, cpu_train as cbow_cpu_train  # noqa: F401  (session fixture, its caller)
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)

pytestmark = pytest.mark.gpu

F32 = np.float32
ALPHA = 0.025
SEED = 5
NEGATIVE = 3
N_WORDS = 4
SIX = F32(6.0)
X_VALUES = {"-6": -SIX, "-6 toward 0": np.nextafter(-SIX, F32(0)), "0": F32(0.0),
            "6 toward 0": np.nextafter(SIX, F32(0)), "6": SIX}


def table_index(x):
    """(int)((f + 6.0f) * 83.0f) in fp32, as the trainers compute it"""
    return int((F32(x) + F32(6.0)) * F32(83.0))


def bin_edge(k=581):
    """adjacent fp32 values (lo, hi) with table_index(lo) = k - 1 and table_index(hi) = k; k = 581 is near
    x = 1, where neighbouring table entries differ by ~2.4e-3"""
    x = F32(k / 83.0 - 6.0)
    while table_index(x) >= k:
        x = np.nextafter(x, F32(-np.inf))
    while table_index(x) < k:
        x = np.nextafter(x, F32(np.inf))
    lo, hi = np.nextafter(x, F32(-np.inf)), x
    assert lo < hi and np.nextafter(lo, F32(np.inf)) == hi
    assert table_index(lo) == k - 1 and table_index(hi) == k
    return lo, hi


def test_the_values_are_what_they_are_called():
    from node2vec_amd import sgns

    x = X_VALUES
    assert x["-6"] == -6 and x["6"] == 6 and x["-6"].dtype == x["6 toward 0"].dtype == np.float32
    assert -6 < x["-6 toward 0"] < F32(-5.999999) and F32(5.999999) < x["6 toward 0"] < 6
    # the first and the last table entry any trainer can read; both inside the table
    assert table_index(x["-6 toward 0"]) == 0 and table_index(x["0"]) == 498
    assert table_index(x["6 toward 0"]) == 996 < sgns.EXP_TABLE_SIZE
    lo, hi = bin_edge()
    t = sgns.exp_table()
    assert 0.9 < lo < hi < 1.1 and t[table_index(hi)] - t[table_index(lo)] > 2e-3


def _rows(n, dim, first):
    m = np.zeros((n, dim), np.float32)
    m[:, 0] = first
    return m


def _identity_vocab(n):
    from node2vec_amd import sgns

    return sgns.Vocab(torch.arange(n).cuda(), torch.arange(n + 6, 6, -1, dtype=torch.int64).cuda(),
                      torch.arange(n, dtype=torch.int32).cuda())


def _same_state(got0, got1, w0, w1):
    assert np.array_equal(got0.view(np.uint32), w0.view(np.uint32)), (got0[:, 0], w0[:, 0])
    assert np.array_equal(got1.view(np.uint32), w1.view(np.uint32)), (got1[:, 0], w1[:, 0])


def _hs(hs_cpu, dim, x, sentence):
    """words 0 / 1 / 2 of counts 9 / 8 / 7 have the codes 0, 11 and 10: the first pair's centre decides
    which code bits meet f = x"""
    from node2vec_amd import hs, sgns

    m = hs.HsModel(_identity_vocab(3), dim, 1, seed=SEED)
    assert m.tree.lengths.tolist() == [1, 2, 2]
    s0, s1 = _rows(3, dim, 1.0), _rows(2, dim, x)
    m.syn0.copy_(torch.from_numpy(s0))
    m.syn1.copy_(torch.from_numpy(s1))
    walks = np.array([sentence], np.int32)
    m.train_block(torch.from_numpy(walks).cuda(), ALPHA, 0, deterministic=True)
    t, exp = m.tree, sgns.exp_table()
    n = hs_cpu.n2v_hs_cpu_train(walks.ctypes.data, 1, 2, s0.ctypes.data, s1.ctypes.data, t.path_off.ctypes.data,
                                t.points.ctypes.data, t.codes.ctypes.data, exp.ctypes.data, 3, 0, m.seed, dim, 1,
                                ALPHA, None)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n == 2
    _same_state(m.syn0.cpu().numpy(), m.syn1.cpu().numpy(), s0, s1)
    return s0, s1


def _ns_model(dim, x, **kw):
    from node2vec_amd import sgns

    m = sgns.SgnsModel(_identity_vocab(N_WORDS), dim, 1, NEGATIVE, seed=SEED, sample=0.0, **kw)
    m.hub_rows = 0
    s0, s1 = _rows(N_WORDS, dim, 1.0), _rows(N_WORDS, dim, x)
    m.syn0.copy_(torch.from_numpy(s0))
    m.syn1neg.copy_(torch.from_numpy(s1))
    return m, s0, s1


def _sgns(oracle, dim, x, sentence, batched=False):
    from node2vec_amd import sgns

    m, s0, s1 = _ns_model(dim, x)
    m.batched = batched
    walks = np.array([sentence], np.int32)
    m.train_block(torch.from_numpy(walks).cuda(), ALPHA, 0, deterministic=True)
    n = oracle.sgns_train(walks, s0, s1, m.cum_table.cpu().numpy(), None, sgns.exp_table(), N_WORDS, 0, m.seed, dim,
                          1, NEGATIVE, ALPHA, batched=batched)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n == 2
    _same_state(m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy(), s0, s1)
    return s0, s1


def _sgns_batched(oracle, dim, x, sentence):
    return _sgns(oracle, dim, x, sentence, batched=True)


def _cbow(cbow_cpu, dim, x, sentence, cbow_mean=1):
    """one context word: its row is the mean and the sum"""
    m, s0, s1 = _ns_model(dim, x, sg=0, cbow_mean=cbow_mean)
    walks = np.array([sentence], np.int32)
    m.train_block(torch.from_numpy(walks).cuda(), ALPHA, 0, deterministic=True)
    n = cbow_cpu_train(cbow_cpu, walks, s0, s1, m.cum_table.cpu().numpy(), None, N_WORDS, 0, m.seed, dim, 1,
                       NEGATIVE, ALPHA, cbow_mean)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n == 2
    _same_state(m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy(), s0, s1)
    return s0, s1


def _cbow_sum(cbow_cpu, dim, x, sentence):
    return _cbow(cbow_cpu, dim, x, sentence, cbow_mean=0)


# trainer -> (its run, the fixture of its witness, sentences: the first pair's centre word varies)
HS_SENTENCES = ([0, 1], [1, 2], [2, 1])  # the first pair trains nodes of code bits 0 / 1, 1 / 1, 0
NS_SENTENCES = ([1, 2], [3, 0])
TRAINERS = {"hs": (_hs, "hs_cpu", HS_SENTENCES), "sgns": (_sgns, "oracle", NS_SENTENCES),
            "sgns_batched": (_sgns_batched, "oracle", NS_SENTENCES), "cbow": (_cbow, "cbow_cpu", NS_SENTENCES),
            "cbow_sum": (_cbow_sum, "cbow_cpu", NS_SENTENCES)}
# (the batched trainer's tiles hold dims 64, 128 and 256 only: it refuses 100)
CASES = [(t, dim) for t in TRAINERS for dim in ((64, 128) if t == "sgns_batched" else (64, 100))]


@pytest.mark.parametrize("name", list(X_VALUES))
@pytest.mark.parametrize("trainer,dim", CASES)
def test_cut_at_plus_and_minus_six(request, trainer, dim, name):
    run, fixture, sentences = TRAINERS[trainer]
    witness = request.getfixturevalue(fixture)
    x = X_VALUES[name]
    for sentence in sentences:
        w0, w1 = run(witness, dim, x, sentence)
        unchanged = bool((w1.view(np.uint32) == _rows(len(w1), dim, x).view(np.uint32)).all())
        print(trainer, dim, name, sentence, "output rows", w1[:, 0].tolist(), "syn0", w0[:, 0].tolist())
        assert unchanged == (abs(float(x)) >= 6.0), "the witness: output rows are skipped exactly when |x| >= 6"
        if unchanged:  # nothing trained, so nothing came back to syn0 either
            assert (w0.view(np.uint32) == _rows(len(w0), dim, 1.0).view(np.uint32)).all()
        elif x != 0:  # (from x = 0 the first pair sends g * 0 back)
            assert not np.array_equal(w0, _rows(len(w0), dim, 1.0))


@pytest.mark.parametrize("trainer,dim", CASES)
def test_both_sides_of_a_table_bin_edge(request, trainer, dim):
    """lo and hi are one ulp apart.  Read from the same table entry, every value they lead to would stay
    within a few ulps of each other; the entries k - 1 and k differ by 2.4e-3, which moves the first
    update by alpha * 2.4e-3 = 6e-5, five hundred ulps"""
    run, fixture, sentences = TRAINERS[trainer]
    witness = request.getfixturevalue(fixture)
    lo, hi = bin_edge()
    for sentence in sentences:
        (l0, l1), (h0, h1) = run(witness, dim, lo, sentence), run(witness, dim, hi, sentence)
        d = float(np.abs(h1.astype(np.float64) - l1).max())
        print(trainer, dim, sentence, "lo", float(lo), "hi", float(hi), "largest difference of the output rows", d)
        assert d > 100 * (float(hi) - float(lo)), "the witness: both sides read the same table entry"
