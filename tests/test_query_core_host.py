"""The host rules that similarity, ann and the model queries share (node2vec_amd/_dense.py, ann._front, the id / name
helpers of embedding._ModelQueries), each against a literal restatement of the code it replaced.  No GPU and no
library: everything here runs, or raises, before either is needed."""
import re

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

INF = float("inf")


# ---- drop_self ----------------------------------------------------------------------------------------------------

def _drop_self_plain(out_r, out_s, self_rows, k):
    """the epilogue knn, search and search_pq each wrote out: a query's own row goes, or else its last entry"""
    rows, scores = [], []
    for r, s, own in zip(out_r.tolist(), out_s.tolist(), self_rows.tolist()):
        at = [i for i, v in enumerate(r) if v == own] or [len(r) - 1]
        rows.append([v for i, v in enumerate(r) if i not in at])
        scores.append([v for i, v in enumerate(s) if i not in at])
        assert len(rows[-1]) == k
    return rows, scores


@pytest.mark.parametrize("out_r,out_s,own", [
    ([[7, 3, 9, 1], [4, 6, 2, 8]], [[.9, .8, .7, .6], [.5, .4, .3, .2]], [3, 5]),       # in the middle | absent
    ([[7, 3, 9, 1], [6, 4, 2, 8]], [[.9, .8, .7, .6], [.5, .4, .3, .2]], [1, 6]),       # in the last slot | first
    ([[5, 2, -1, -1], [5, -1, -1, -1]], [[.9, .1, -INF, -INF], [.9, -INF, -INF, -INF]], [2, 9]),  # a (-1, -inf) tail
    ([[4, 0], [3, 1]], [[.5, .25], [.5, .25]], [4, 2]),                                # k = 1: own | absent
    ([[1, 0], [0, 1]], [[.5, .25], [.5, .25]], [0, 2]),                                # k = 1: own last | absent
])
def test_drop_self_is_the_epilogue_it_replaced(out_r, out_s, own):
    from node2vec_amd import _dense

    out_r, out_s, own = torch.tensor(out_r), torch.tensor(out_s, dtype=torch.float32), torch.tensor(own)
    k = out_r.shape[1] - 1
    got_r, got_s = _dense.drop_self(out_r, out_s, own, k)
    want_r, want_s = _drop_self_plain(out_r, out_s, own, k)
    assert got_r.dtype == torch.int64 and got_s.dtype == torch.float32 and got_r.shape == got_s.shape == (2, k)
    assert got_r.tolist() == want_r and got_s.tolist() == want_s


# ---- topk_batches -------------------------------------------------------------------------------------------------

def _knn_loop(need, nq, limit):
    """similarity._topk_fused's loop as it was: (i, j, bytes of workspace) per launch"""
    if nq == 0:
        return []
    step = nq
    while step > 1 and need(step) > limit:
        step = (step + 1) // 2
    return [(i, min(nq, i + step), max(int(need(min(nq, i + step) - i)), 16)) for i in range(0, nq, step)]


def _ann_loop(need, nq, limit):
    """ann._topk's and ann._pq_topk's loop as it was"""
    if nq == 0:
        return []
    step = min(nq, (1 << 20) - 1)
    while step > 1 and not 0 <= need(step) <= limit:
        step = (step + 1) // 2
    return [(i, min(nq, i + step), max(int(need(min(nq, i + step) - i)), 16)) for i in range(0, nq, step)]


def _linear(count):
    return 100 + 10 * count


def _refusing(count):  # a library that refuses more than 8 queries a launch
    return -1 if count > 8 else 100 + 10 * count


@pytest.mark.parametrize("need,nq,limit,launches", [
    (_linear, 37, 1 << 30, 1),           # fits at once
    (_linear, 37, 150, 8),               # 37 -> 19 -> 10 -> 5: three halvings, a ragged last launch
    (_linear, 37, 50, 37),               # never fits: one query a launch, whatever it needs
    (_linear, 0, 1 << 30, 0),
    (_linear, 1, 1 << 30, 1),
    (_linear, 1, 50, 1),
    (_refusing, 37, 1 << 30, None),      # the two flavours part here
    (lambda count: 1 + count // 4096, (1 << 20) + 5, 1 << 30, None),  # the cap of 2^20 - 1 queries a launch
])
def test_topk_batches_launches_what_the_three_loops_launched(monkeypatch, need, nq, limit, launches):
    from node2vec_amd import _dense, similarity

    monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", limit)
    for max_step, loop in ((None, _knn_loop), ((1 << 20) - 1, _ann_loop)):
        seen = []

        def launch(i, j, ws, out_r, out_s):
            assert ws.dtype == torch.uint8 and out_r.shape == out_s.shape == (nq, 2)
            seen.append((i, j, ws.numel()))
            out_r[i:j] = 7

        out_r, out_s = _dense.topk_batches(need, launch, nq, 2, "cpu", max_step=max_step)
        assert seen == loop(need, nq, limit)
        assert launches is None or len(seen) == launches
        assert out_r.dtype == torch.int64 and out_s.dtype == torch.float32
        assert (out_r == 7).all() and (out_s == -INF).all()  # every query launched once; scores as allocated
    if need is _refusing:
        assert _knn_loop(need, nq, limit) == [(0, 37, 16)] and len(_ann_loop(need, nq, limit)) == 8
    if nq > 1 << 20:
        assert len(_knn_loop(need, nq, limit)) == 1 and len(_ann_loop(need, nq, limit)) == 2


def test_topk_batches_launches_nothing_on_an_empty_problem():
    from node2vec_amd import _dense

    def launch(*args):
        raise AssertionError("launched")

    out_r, out_s = _dense.topk_batches(_linear, launch, 5, 3, "cpu", empty=True)
    assert out_r.shape == out_s.shape == (5, 3) and (out_r == -1).all() and (out_s == -INF).all()
    out_r, out_s = _dense.topk_batches(_linear, launch, 0, 3, "cpu", max_step=9)
    assert out_r.shape == out_s.shape == (0, 3)


# ---- the id / name frame of the model queries ---------------------------------------------------------------------

def _queries(name_id=None, wv=None):
    from node2vec_amd.embedding import _ModelQueries

    q = _ModelQueries()
    q.name_id = name_id
    if wv is not None:
        q.model = type("Model", (), {"wv": wv})()
    return q


def test_who_maps_ids_through_name_id():
    ids = np.array([2, 7, 1, 5], dtype=np.int64)
    column, who = _queries()._who(ids)
    assert column == "id" and who is ids
    name_id = pd.DataFrame({"id": [1, 2, 1, 5, 7], "name": ["a", "b", "c", "e", "g"]})
    column, who = _queries(name_id)._who(ids)
    assert column == "name" and who.tolist() == ["b", "g", "c", "e"]  # id 1 twice: its last name
    with pytest.raises(KeyError) as err:  # 7 and 5 are missing: the first in vocabulary order
        _queries(name_id[name_id["id"] < 5])._who(ids)
    assert err.value.args == (7,)


def test_vocab_ids_of_string_tokens_are_those_of_the_integer_array():
    from node2vec_amd.embedding import KeyedVectors, _ModelQueries

    ids = np.array([40, 3, 17, 8, 25], dtype=np.int64)
    vectors = np.zeros((5, 4), np.float32)
    by_id, by_token = KeyedVectors(ids, vectors), KeyedVectors([str(i) for i in ids], vectors)
    assert by_id.ids is not None and by_token.ids is None
    for lo, hi in ((0, None), (1, 4), (3, 9)):
        a, b = _ModelQueries._vocab_ids(by_id, lo, hi), _ModelQueries._vocab_ids(by_token, lo, hi)
        assert a.dtype == b.dtype == np.int64 and np.array_equal(a, b) and np.array_equal(a, ids[lo:hi])
    assert _queries(wv=by_token)._wv() is by_token
    with pytest.raises(ValueError, match=re.escape("Model is not available. Please run fit()")):
        _queries()._wv()


# ---- what search and search_pq refuse, and which error wins --------------------------------------------------------

def _indexes():
    from node2vec_amd import ann

    flat = ann.IVFIndex(torch.zeros(4, 8), torch.ones(4), torch.zeros(5, dtype=torch.int64),
                        torch.zeros(0, dtype=torch.int32), 1, 70, 8, 3)
    return flat, ann.IVFPQIndex(flat, torch.zeros(2, 256, 4), torch.zeros((0, 4), dtype=torch.uint8), 2, 4)


X = torch.zeros(70, 8)
Q = torch.zeros(3, 8)
LIMIT = "is above the index's limit of 128: similarity.knn serves larger k exactly"

# (keyword arguments, exception, message) that hold for both; then (function, index, ...) with "flat", "pq" or
# None, which is no index at all
BOTH = [
    (dict(k=0, queries=Q), ValueError, "k must be >= 1"),
    (dict(k=5, queries=Q, exclude_self=True), ValueError, "exclude_self needs rows="),
    (dict(k=129, queries=Q), ValueError, "k = 129 " + LIMIT),
    (dict(k=128, rows=[0], exclude_self=True), ValueError, "k = 128 + 1 (exclude_self) " + LIMIT),
    (dict(k=5, queries=Q, X=torch.zeros(70, 9)), ValueError, "the index was built on a [70, 8] matrix, not [70, 9]"),
    (dict(k=5, queries=Q, X=torch.zeros(8)), ValueError, "X must be a 2-D tensor on a HIP device"),
    # two bad arguments: the earlier check wins
    (dict(k=200, queries=Q, exclude_self=True), ValueError, "exclude_self needs rows="),
    (dict(k=0, queries=Q, X=torch.zeros(70, 9)), ValueError, "k must be >= 1"),
]
CASES = [("search", "flat", {"X": X, **kw}, exc, msg) for kw, exc, msg in BOTH]
CASES += [("search_pq", "pq", kw, exc, msg) for kw, exc, msg in BOTH]
CASES += [
    ("search", None, dict(k=5, X=X, queries=Q), ValueError, "index must be an IVFIndex (ann.build_index)"),
    ("search", "flat", dict(k=5, X=None, queries=Q), ValueError, "X must be a 2-D tensor on a HIP device"),
    ("search", None, dict(k=0, X=X, queries=Q), ValueError, "k must be >= 1"),
    ("search_pq", "flat", dict(k=5, queries=Q), ValueError, "index must be an IVFPQIndex (ann.build_pq)"),
    ("search_pq", "pq", dict(k=5, queries=Q, refine=-1), ValueError, "refine must be >= 0"),
    ("search_pq", "pq", dict(k=5), ValueError, "give exactly one of queries= / rows="),
    ("search_pq", "pq", dict(k=5, queries=Q, rows=[0], X=X), ValueError, "give exactly one of queries= / rows="),
    ("search_pq", "pq", dict(k=5, rows=[0]), ValueError, "rows= needs X"),
    ("search_pq", "pq", dict(k=5, queries=Q, refine=2), ValueError,
     "refine > 0 needs X: the exact scores are computed from its rows"),
    ("search_pq", "pq", dict(k=5, queries=torch.zeros(3, 7)), ValueError, "queries must be [n_queries, 8]"),
    ("search_pq", "pq", dict(k=5, queries=torch.zeros(2, 3, 8)), ValueError, "queries must be [n_queries, 8]"),
    ("search_pq", "pq", dict(k=5, queries=Q, probes=torch.zeros((2, 1), dtype=torch.int32)), ValueError,
     "probes must be [3, 1 .. 4]"),
    ("search_pq", "pq", dict(k=5, queries=Q, probes=torch.zeros((3, 5), dtype=torch.int32)), ValueError,
     "probes must be [3, 1 .. 4]"),
    ("search_pq", "pq", dict(k=5, queries=torch.zeros(8), probes=torch.zeros(1, dtype=torch.int32)), ValueError,
     "probes must be [1, 1 .. 4]"),
    # two bad arguments: the earlier check wins
    ("search_pq", "flat", dict(k=0, queries=Q), ValueError, "k must be >= 1"),
    ("search_pq", "pq", dict(k=0, queries=Q, refine=-1), ValueError, "k must be >= 1"),
    ("search_pq", "pq", dict(k=5, rows=[0], refine=2), ValueError, "rows= needs X"),
    ("search_pq", "pq", dict(k=129, queries=Q, refine=-1), ValueError, "refine must be >= 0"),
    ("search_pq", "flat", dict(k=5), ValueError, "index must be an IVFPQIndex (ann.build_pq)"),
]
# What needs a device before it can be refused stays with the GPU tests: search hands X to similarity._inputs, which
# wants it on the device, before it looks at queries=, rows=, inv_norm= or probes=; so does search_pq given X.


@pytest.mark.parametrize("fn,which,kw,exc,msg", CASES)
def test_search_and_search_pq_refuse_in_their_own_order(fn, which, kw, exc, msg):
    from node2vec_amd import ann

    flat, pq = _indexes()
    index = {"flat": flat, "pq": pq}.get(which, "no index")
    kw = dict(kw)
    with pytest.raises(exc, match="^" + re.escape(msg) + "$"):
        if fn == "search":
            ann.search(kw.pop("X"), index, kw.pop("k"), **kw)
        else:
            ann.search_pq(index, kw.pop("k"), **kw)
