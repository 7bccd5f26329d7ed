"""Fold-in (DESIGN.md "Fold-in"), the parts that need no GPU: the CPU restatement tests/cpu_foldin/n2v_foldin_cpu.c
against a second statement of the definition in numpy float64 with ordinary dot products (records equal, rows inside
a measured tolerance), the properties of the definition on the restatement, the refusals of the Python layer and
KeyedVectors.with_rows."""
import ctypes as C
from bisect import bisect_left

import numpy as np
import pandas as pd
import pytest

import foldin_cases as fc

M64 = fc.M64

# TOLERANCE, measured here over the case list (test_rows_agree_with_float64 prints the figure of every case): the
# largest |fp32 restatement - float64 numpy| is 1.341e-04, in case many_vertices_dim64 (rows of magnitude ~2).  Eight
# of the ten cases stay between 3.6e-08 and 1.05e-06, a few ulp of fp32 carried through a chain; the two above that
# (8.17e-06 in dim128_window32_row_alpha is the other) each hold a target whose f lies within fp32 rounding of a
# boundary of the 1000-entry sigmoid table, so that the two precisions read neighbouring entries: a step of about
# alpha * 0.003 * |syn1neg|, which belongs to the definition (it is word2vec's table).  A factor 4 over the largest
# covers rounding growth on longer chains; a missing or misdrawn target moves a row by 1e-2 and more.
F64_GAP_MEASURED = 1.341e-04
F64_TOL = 4 * F64_GAP_MEASURED


@pytest.fixture(scope="session")
def foldin_cpu(tmp_path_factory):
    """the CPU restatement, built once per session by cpu_build"""
    return fc.build_cpu(tmp_path_factory.mktemp("foldin_cpu"))


@pytest.fixture(scope="session")
def cases():
    """every case of the list, made once and never written to"""
    out = {name: fc.make(name) for name in fc.NAMES}
    for c in out.values():
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def reference_foldin(case, table):
    """float64 statement of one pass, written from the definition: per walk the filter (a new token is always
    kept) and the reduced windows, then every (centre i, context j) with a new context and a known centre, trained
    on the new row with the trainer's draws for that pair and no update of syn1neg.  Shares only mix64 with the C
    file.  Returns (records in (row, i, j) order, rows float64)."""
    walks, n_vocab, n_new = case["walks"], case["n_vocab"], case["n_new"]
    window, K, ln = case["window"], case["negative"], case["walks"].shape[1]
    cum = [int(x) for x in case["cum_table"]]
    si = case["sample_int"]
    s1 = case["syn1neg"].astype(np.float64)
    rows = case["init"].astype(np.float64)
    records = []
    for r in range(walks.shape[0]):
        alpha = float(case["alpha"] if case["row_alpha"] is None else case["row_alpha"][r])
        hs = mix64(case["seed"] ^ mix64(case["sentence_base"] + r + 0xA0761D6478BD642F))
        draw = lambda idx: mix64(hs + (idx + 1) * 0xE7037ED1A0B428DB)  # noqa: E731
        sent, red = [], []
        for t in range(ln):
            tok = int(walks[r, t])
            if tok < 0 or tok >= n_vocab + n_new:
                continue
            if tok < n_vocab and si is not None and int(si[tok]) < (draw(2 * t) >> 32):
                continue
            sent.append(tok)
            red.append((draw(2 * t + 1) >> 32) % window)
        for i, centre in enumerate(sent):
            if centre >= n_vocab:
                continue
            for j in range(max(0, i - window + red[i]), min(len(sent), i + window + 1 - red[i])):
                if j == i or sent[j] < n_vocab:
                    continue
                u = sent[j] - n_vocab
                rel = j - i + window - (1 if j > i else 0)
                records.append((u, r, i | (rel << 16), centre))
                work = np.zeros(rows.shape[1])
                targets = [(centre, 1.0)]
                for d in range(K):
                    tg = bisect_left(cum, (draw(2 * ln + (i * 2 * window + rel) * K + d) >> 16) % cum[-1])
                    if tg != centre:
                        targets.append((tg, 0.0))
                for tg, label in targets:
                    f = float(rows[u] @ s1[tg])
                    if f <= -6.0 or f >= 6.0:
                        continue
                    work += (label - float(table[int((f + 6.0) * 83.0)])) * alpha * s1[tg]
                rows[u] += work
    return np.array(records, np.int32).reshape(-1, 4), rows


@pytest.fixture(scope="session")
def references(cases):
    """the float64 statement of every case, computed once"""
    from node2vec_amd import sgns

    table = sgns.exp_table()
    return {name: reference_foldin(c, table) for name, c in cases.items()}


@pytest.mark.parametrize("name", fc.NAMES)
def test_records_equal_the_float64_statement(foldin_cpu, cases, references, name):
    n, rec = fc.cpu_pass(foldin_cpu, cases[name], records=True)
    ref, _ = references[name]
    assert n == ref.shape[0] > 0
    assert np.array_equal(rec, ref)


def test_rows_agree_with_float64(foldin_cpu, cases, references):
    worst = 0.0
    for name in fc.NAMES:
        rows = cases[name]["init"].copy()
        fc.cpu_pass(foldin_cpu, cases[name], rows)
        gap = float(np.abs(rows.astype(np.float64) - references[name][1]).max())
        moved = float(np.abs(rows - cases[name]["init"]).max())
        print("fold-in fp32 restatement against float64: %-28s max |gap| %.3e (rows moved by up to %.3e, |row| <= %.3e)"
              % (name, gap, moved, float(np.abs(rows).max())))
        assert moved > 1e-4, name  # the case trains
        worst = max(worst, gap)
    print("fold-in: largest gap over the case list %.3e, tolerance %.3e" % (worst, F64_TOL))
    assert worst <= F64_TOL, worst


def test_cases_reach_what_they_claim(foldin_cpu, cases):
    """from the restatement alone: draws that hit the centre word, both sides of the sigmoid cut, a vertex that
    never occurs, vertices at both ends of a sentence, more pairs of one vertex in a walk than one batch of draws"""
    stats = np.zeros(4, np.int64)
    fc.cpu_pass(foldin_cpu, cases["two_word_vocabulary"], cases["two_word_vocabulary"]["init"].copy(), stats=stats)
    assert stats[0] > 0, "no negative draw equals its centre word"
    stats = np.zeros(4, np.int64)
    fc.cpu_pass(foldin_cpu, cases["sigmoid_cut"], cases["sigmoid_cut"]["init"].copy(), stats=stats)
    assert stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats  # skipped at |f| >= 6, entry 0, the last entry read
    c = cases["ragged_dim100_two_passes"]
    _, rec = fc.cpu_pass(foldin_cpu, c, records=True)
    assert c["never"] is not None and not (rec[:, 0] == c["never"]).any()
    assert c["walks"].shape[1] > 128  # two 64-token preparation passes, and a third
    for name in ("ragged_dim100_two_passes", "dim128_window32_row_alpha"):
        w, nv = cases[name]["walks"], cases[name]["n_vocab"]
        assert (w[::2, 0] >= nv).all() and (w[::2, -1] >= nv).all()
    c = cases["hot_vertex_many_batches"]
    _, rec = fc.cpu_pass(foldin_cpu, c, records=True)
    assert int(((rec[:, 0] == 1) & (rec[:, 1] == 1)).sum()) > 4 * (64 // c["negative"])
    big = cases["many_vertices_dim64"]
    assert big["n_new"] > 4 * 64 and big["cum_index"] and big["sample_int"] is not None


def test_vertices_fold_in_together_as_alone(foldin_cpu, cases):
    """{u, v} together == each alone, bit for bit.  Alone: the walks that hold the other vertex are emptied (the
    rows keep their numbers, so every sentence keeps its stream) and its row is absent from the result."""
    c = cases["dim256_window1_two_passes"]
    nv = c["n_vocab"]
    walks = c["walks"].copy()
    walks[walks >= nv] = -1
    walks[0::2, 3::7] = nv        # u in the even rows
    walks[1::2, 2::5] = nv + 1    # v in the odd rows
    both = c["init"][:2].copy()
    n, _ = fc.cpu_pass(foldin_cpu, c, both, walks=walks, n_new=2)
    assert n > 0 and not np.array_equal(both[0], c["init"][0]) and not np.array_equal(both[1], c["init"][1])
    for u, mine in ((0, slice(0, None, 2)), (1, slice(1, None, 2))):
        own = np.full_like(walks, -1)
        own[mine] = walks[mine]
        alone = c["init"][:2].copy()
        fc.cpu_pass(foldin_cpu, c, alone, walks=own, n_new=2)
        assert np.array_equal(alone[u], both[u]) and np.array_equal(alone[1 - u], c["init"][1 - u])


def test_a_chain_never_reads_another_new_row(foldin_cpu, cases):
    """in walks where new vertices meet, the row of u after a pass is the same bits whatever the rows of the other
    new vertices hold: they are set to 100 here"""
    c = cases["ragged_dim100_two_passes"]
    both = c["init"].copy()
    fc.cpu_pass(foldin_cpu, c, both)
    for u in (0, 5, 13):
        rows = np.full_like(both, 100.0)
        rows[u] = c["init"][u]
        fc.cpu_pass(foldin_cpu, c, rows)
        assert np.isfinite(rows[u]).all() and np.array_equal(rows[u], both[u]), u
        assert not np.array_equal(both[u], c["init"][u])


def _hand(walk, n_vocab, n_new, dim=8, window=2, K=3):
    """a hand-made one-walk case over a tiny frozen model"""
    rng = np.random.default_rng(9)
    cum, _ = fc._tables(np.arange(n_vocab, 0, -1, dtype=np.int64) * 7, 0.0)
    return {"n_vocab": n_vocab, "n_new": n_new, "dim": dim, "negative": K, "window": window,
            "walks": np.array([walk], np.int32), "cum_table": cum, "sample_int": None,
            "syn1neg": rng.standard_normal((n_vocab, dim)).astype(np.float32),
            "init": rng.standard_normal((n_new, dim)).astype(np.float32), "row_alpha": None, "alpha": 0.05,
            "seed": 11, "sentence_base": 0}


def test_a_new_centre_trains_nothing(foldin_cpu):
    """a walk of new vertices only, and one whose only known word is out of every window: no pair at all"""
    c = _hand([5, 6, 5, 7, 6], 5, 3)
    rows = c["init"].copy()
    n, rec = fc.cpu_pass(foldin_cpu, c, rows, records=True)
    assert n == 0 and rec.shape == (0, 4) and np.array_equal(rows, c["init"])


def test_adjacent_new_tokens_train_nothing_between_themselves(foldin_cpu):
    """known a, new u, new v, known b with window 1 (b = 0 always): the pairs are (a, u) and (b, v) only"""
    c = _hand([0, 5, 6, 1], 5, 2, window=1)
    rows = c["init"].copy()
    n, rec = fc.cpu_pass(foldin_cpu, c, rows, records=True)
    # centre i = 0 (word 0) -> j = 1 (u, rel 1); centre i = 3 (word 1) -> j = 2 (v, rel 0)
    assert rec.tolist() == [[0, 0, 0 | (1 << 16), 0], [1, 0, 3 | (0 << 16), 1]] and n == 2
    assert not np.array_equal(rows[0], c["init"][0]) and not np.array_equal(rows[1], c["init"][1])
    # u's row after the pass does not depend on v's row, nor v's on u's
    other = c["init"].copy()
    other[1] = 100.0
    fc.cpu_pass(foldin_cpu, c, other)
    assert np.array_equal(other[0], rows[0])


def test_alpha_zero_leaves_the_rows_as_initialised(foldin_cpu, cases):
    c = cases["dim128_window32_row_alpha"]
    rows = c["init"].copy()
    n, _ = fc.cpu_pass(foldin_cpu, c, rows, alpha=0.0, row_alpha=None)
    assert n > 0 and np.array_equal(rows, c["init"])


def test_restatement_refuses_what_the_kernels_refuse(foldin_cpu, cases):
    c = dict(cases["one_vertex_dim1"])
    for key, bad in (("dim", 0), ("dim", 1025), ("window", 0), ("window", 33), ("negative", 0), ("negative", 33)):
        assert fc.cpu_pass(foldin_cpu, {**c, key: bad})[0] == -1
    assert fc.cpu_pass(foldin_cpu, c, n_new=-1)[0] == -1


# ---- the Python layer ----
def _fitted(params):
    from node2vec_amd.embedding import HipW2V, KeyedVectors, Node2VecHIP

    walks = pd.DataFrame({"walk": [[0, 1, 2], [2, 1, 0]]})
    n2v = Node2VecHIP(walks, dict(params), random_seed=5)
    n2v.model = HipW2V(KeyedVectors(np.arange(3), np.zeros((3, 4), np.float32)), np.zeros((3, 4), np.float32),
                       {**n2v.w2v_params, **params}, 0)
    return n2v


@pytest.mark.parametrize("params", [{"sg": 0, "negative": 5}, {"sg": 1, "negative": 5, "batched": True}])
def test_infer_vertices_refuses_other_objectives(params):
    with pytest.raises(ValueError, match="skip-gram negative sampling only"):
        _fitted(params).infer_vertices(pd.DataFrame({"walk": [[0, 7, 2]]}))


def test_infer_vertices_refuses_the_spark_model():
    from node2vec_amd.embedding import Node2VecSpark

    n2v = Node2VecSpark.__new__(Node2VecSpark)
    with pytest.raises(ValueError, match="skip-gram negative sampling only"):
        n2v.infer_vertices(pd.DataFrame({"walk": [[0, 7, 2]]}))


def test_fold_in_refuses_cbow_and_batched_models():
    import torch
    from types import SimpleNamespace

    from node2vec_amd import foldin

    walks = torch.zeros((2, 4), dtype=torch.int32)
    for extra in ({"sg": 0}, {"batched": True}):
        m = SimpleNamespace(syn1neg=torch.zeros((3, 4)), seed=1, window=2, negative=2, **extra)
        with pytest.raises(ValueError):
            foldin.fold_in(m, walks, 1, 1)
        with pytest.raises(ValueError):
            foldin.pair_records(m, walks, 1)


def test_with_rows_order_and_non_aliasing():
    from node2vec_amd.embedding import KeyedVectors

    old = np.arange(12, dtype=np.float32).reshape(3, 4)
    kv = KeyedVectors(np.array([7, 3, 9]), old.copy())
    new = -np.arange(8, dtype=np.float32).reshape(2, 4)
    ext = kv.with_rows(np.array([20, 4]), new)
    assert len(kv) == 3 and np.array_equal(kv.vectors, old) and "20" not in kv
    assert list(ext.index2word) == ["7", "3", "9", "20", "4"] and len(ext) == 5
    assert np.array_equal(ext.vectors[:3], old) and np.array_equal(ext.vectors[3:], new)
    assert np.array_equal(ext["4"], new[1]) and ext.vocab["20"] == 3 and np.array_equal(ext["3"], old[1])
    ext.vectors[0, 0] = 99.0
    ext.vectors[4, 0] = 99.0
    assert kv.vectors[0, 0] == 0.0 and new[1, 0] == -4.0  # shares memory with neither
    with pytest.raises(ValueError):
        kv.with_rows(np.array([3]), new[:1])  # already in the vocabulary
    with pytest.raises(ValueError):
        kv.with_rows(np.array([20, 4]), new[:, :3])
    # string tokens (a loaded text file)
    kv = KeyedVectors(["a", "b"], old[:2].copy())
    ext = kv.with_rows(["c"], new[:1])
    assert list(ext.index2word) == ["a", "b", "c"] and np.array_equal(ext["c"], new[0])


def test_argument_errors_come_back_before_any_launch():
    """N2V_EINVAL (-1) without a GPU: nothing is launched; nothing to do is N2V_OK"""
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    L = _lib.load()
    buf = (C.c_int64 * 64)()
    p_ = C.addressof(buf)

    def params(**kw):
        a = dict(n_vocab=10, sentence_base=0, seed=1, dim=8, window=2, negative=3, alpha=0.025, deterministic=0,
                 cum_index_bits=0, cum_index=0, max_waves=0, batched=0, window_cache=0, hub_rows=0, row_alpha=0)
        a.update(kw)
        return _lib.SgnsParams(*[a[f[0]] for f in _lib.SgnsParams._fields_])

    def train(P=None, records=p_, off=p_, n_new=2, rows=3, ln=5, new_rows=p_, s1=p_, cum=p_, exp=p_):
        return L.n2v_foldin_train(records, off, n_new, rows, ln, new_rows, s1, cum, exp, P or params(), None)

    def counts(P=None, walks=p_, rows=3, ln=5, n_new=2, out=p_):
        return L.n2v_foldin_pair_counts(walks, rows, ln, n_new, None, P or params(), out, None)

    def fill(P=None, walks=p_, rows=3, ln=5, n_new=2, off=p_, out=p_):
        return L.n2v_foldin_pair_records(walks, rows, ln, n_new, None, P or params(), off, out, None)

    assert train(n_new=0) == 0 and train(rows=0) == 0 and counts(rows=0) == 0 and fill(rows=0) == 0
    assert train(n_new=0, new_rows=0) == 0
    for call in (train, counts, fill):
        assert call(n_new=-1) == -1 and call(n_new=2 ** 31) == -1 and call(P=params(n_vocab=2 ** 31 - 1)) == -1
        assert call(ln=0) == -1 and call(ln=257) == -1 and call(rows=-1) == -1 and call(rows=2 ** 31) == -1
        for bad in (dict(dim=0), dict(dim=1025), dict(window=0), dict(window=33), dict(negative=0), dict(negative=33),
                    dict(n_vocab=0), dict(batched=1), dict(window_cache=1), dict(hub_rows=-1),
                    dict(cum_index=p_, cum_index_bits=0), dict(cum_index=p_, cum_index_bits=31)):
            assert call(P=params(**bad)) == -1, bad
    assert train(new_rows=0) == -1 and train(s1=0) == -1 and train(cum=0) == -1 and train(exp=0) == -1
    assert train(records=0) == -1 and train(off=0) == -1
    assert counts(walks=0) == -1 and counts(out=0) == -1
    assert fill(walks=0) == -1 and fill(off=0) == -1 and fill(out=0) == -1
