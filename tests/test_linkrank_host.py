"""Link ranking without a GPU: ranking_metrics on hand-written counts, holdout_edges' guarantees, the refusals of the
n2v_link_rank entry points (nothing is launched), and the proof that the cases of tests/linkrank_cases.py pin
something: each can tell a wrong filter, a wrong tie rule and a wrong count apart from the restatement alone, and a
restatement that sums in another order counts differently."""
import ctypes as C

import numpy as np
import pytest
import torch

import linkrank_cases as lc
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


def test_ranking_metrics_on_hand_written_counts():
    from node2vec_amd import linkpred

    greater, equal = [0, 0, 3, 9, 120], [0, 2, 0, 1, 4]
    ks = (1, 2, 5, 10, 100, 1000)
    want = {"mean": [1.0, 2.0, 4.0, 10.5, 123.0], "optimistic": [1.0, 1.0, 4.0, 10.0, 121.0],
            "pessimistic": [1.0, 3.0, 4.0, 11.0, 125.0]}
    for tie, ranks in want.items():
        got = linkpred.ranking_metrics(torch.tensor(greater), np.array(equal), ks=ks, tie=tie)
        ranks = np.array(ranks)
        assert set(got) == {"mrr", "mean_rank", "n"} | {f"hits@{k}" for k in ks}
        assert got["n"] == 5 and isinstance(got["n"], int)
        assert got["mean_rank"] == float(ranks.mean())
        assert got["mrr"] == pytest.approx(float((1.0 / ranks).mean()), rel=1e-15) and 0.0 < got["mrr"] <= 1.0
        hits = [got[f"hits@{k}"] for k in ks]
        assert hits == [float((ranks <= k).mean()) for k in ks]
        assert all(x <= y for x, y in zip(hits, hits[1:])) and hits[-1] == 1.0
    assert linkpred.ranking_metrics([0], [0])["mrr"] == 1.0
    one = linkpred.ranking_metrics(greater, equal)
    assert set(one) == {"mrr", "mean_rank", "hits@1", "hits@10", "hits@50", "hits@100", "n"}  # the default ks
    assert one == linkpred.ranking_metrics(greater, equal, tie="mean")
    for bad in (dict(tie="median"), dict(ks=(0,))):
        with pytest.raises(ValueError):
            linkpred.ranking_metrics(greater, equal, **bad)
    with pytest.raises(ValueError):
        linkpred.ranking_metrics([], [])
    with pytest.raises(ValueError):
        linkpred.ranking_metrics([1, 2], [1])
    with pytest.raises(ValueError):
        linkpred.ranking_metrics([-1], [0])


def _undirected(rng, n, m, loops=0, copies=0):
    from node2vec_amd.graph import DeviceGraph

    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    a, b = a[a != b], b[a != b]
    a, b = np.concatenate([a, a[:copies]]), np.concatenate([b, b[:copies]])  # multi-edges
    loop = rng.integers(0, n, loops)
    src, dst = np.concatenate([a, b, loop]), np.concatenate([b, a, loop])
    return DeviceGraph.from_edges(src, dst, n_vertices=n)


def _arcs(g):
    src = np.repeat(np.arange(g.n_vertices), g.degrees().numpy())
    return set(zip(src.tolist(), g.col.numpy().tolist()))


@pytest.mark.parametrize("undirected", [True, False])
def test_holdout_edges_keeps_every_vertex_an_out_edge(undirected):
    from node2vec_amd import linkpred

    rng = np.random.default_rng(11)
    g = _undirected(rng, 60, 150, loops=4, copies=10)
    train, ta, tb = linkpred.holdout_edges(g, 0.25, seed=3, undirected=undirected)
    again = linkpred.holdout_edges(g, 0.25, seed=3, undirected=undirected)
    assert torch.equal(ta, again[1]) and torch.equal(tb, again[2])
    assert torch.equal(train.rowptr, again[0].rowptr) and torch.equal(train.col, again[0].col)
    other = linkpred.holdout_edges(g, 0.25, seed=4, undirected=undirected)
    assert not (torch.equal(ta, other[1]) and torch.equal(tb, other[2]))
    before, after = _arcs(g), _arcs(train)
    pairs = list(zip(ta.tolist(), tb.tolist()))
    assert ta.dtype == tb.dtype == torch.int64 and len(pairs) == len(set(pairs)) > 0
    edges = {(min(s, d), max(s, d)) for s, d in before if s != d} if undirected else {e for e in before if e[0] != e[1]}
    assert len(pairs) == round(0.25 * len(edges))  # this graph has enough edges that may leave
    for a, b in pairs:
        assert a != b and (a, b) in before and (a, b) not in after
        if undirected:
            assert a < b and (b, a) in before and (b, a) not in after
    gone = set(pairs) | ({(b, a) for a, b in pairs} if undirected else set())
    assert after == before - gone  # nothing else left, self-loops and the other multi-edges stay
    assert train.n_edges == sum(1 for s, d in zip(np.repeat(np.arange(60), g.degrees().numpy()).tolist(),
                                                  g.col.tolist()) if (s, d) not in gone)
    had, has = g.degrees() > 0, train.degrees() > 0
    assert bool((has == had).all()), "a vertex lost its last out-edge"
    nothing = linkpred.holdout_edges(g, 0.0, seed=3, undirected=undirected)
    assert nothing[1].numel() == 0 and torch.equal(nothing[0].col, g.col)
    with pytest.raises(ValueError):
        linkpred.holdout_edges(g, 1.0, seed=3)


def test_holdout_edges_takes_nothing_from_a_star_and_keeps_weights():
    from node2vec_amd import linkpred
    from node2vec_amd.graph import DeviceGraph

    leaves = np.arange(1, 12)
    hub = np.zeros_like(leaves)
    star = DeviceGraph.from_edges(np.concatenate([hub, leaves]), np.concatenate([leaves, hub]), n_vertices=12)
    train, ta, tb = linkpred.holdout_edges(star, 0.5, seed=1)
    assert ta.numel() == 0 and tb.numel() == 0  # every edge is some leaf's last
    assert torch.equal(train.rowptr, star.rowptr) and torch.equal(train.col, star.col)
    # a triangle with a tail, weighted: one edge of the triangle may leave, its weights leave with it
    src, dst = np.array([0, 1, 1, 2, 2, 0, 2, 3]), np.array([1, 0, 2, 1, 0, 2, 3, 2])
    w = np.array([1.5, 1.5, 2.5, 2.5, 3.5, 3.5, 4.5, 4.5], np.float32)
    g = DeviceGraph.from_edges(src, dst, w, n_vertices=4)
    train, ta, tb = linkpred.holdout_edges(g, 0.3, seed=2)
    assert ta.numel() == 1 and (int(ta[0]), int(tb[0])) in {(0, 1), (0, 2), (1, 2)}
    left = {(s, d): x for s, d, x in zip(np.repeat(np.arange(4), train.degrees().numpy()).tolist(),
                                         train.col.tolist(), train.w.tolist())}
    assert left == {(s, d): x for s, d, x in zip(src.tolist(), dst.tolist(), w.tolist())
                    if {s, d} != {int(ta[0]), int(tb[0])}}


def test_link_rank_abi_refuses_bad_arguments_without_a_gpu(lib):
    from node2vec_amd import _lib

    L = lib
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf) & ~15  # (16-byte aligned; never dereferenced)

    def need(n=1000, dim=64, nq=10):
        return L.n2v_link_rank_workspace_bytes(n, dim, nq)

    def rank(n=1000, dim=64, nq=10, X=p, inv=p, a=p, b=p, rowptr=p, col=p, thr=p, counts=p, ws=p, ws_bytes=None):
        ws_bytes = need(n, dim, nq) if ws_bytes is None else ws_bytes
        return L.n2v_link_rank(X, inv, n, dim, a, b, nq, rowptr, col, thr, counts, ws, ws_bytes, None)

    assert need() > 0 and need() % 256 == 0 and need(nq=0) == 0 and need(n=0) == 0
    assert need(nq=100) > need(nq=10) and need(dim=128) > need(dim=64)
    for kw in (dict(dim=0), dict(dim=1025), dict(n=-1), dict(n=1 << 31), dict(nq=-1), dict(nq=1 << 31)):
        assert need(**kw) == -1, kw
        assert rank(ws_bytes=1 << 20, **kw) == _lib.EINVAL, kw
    assert rank(nq=0) == _lib.OK and rank(n=0) == _lib.OK  # nothing to do: nothing launched
    assert rank(nq=0, rowptr=None) == _lib.EINVAL  # (refused before the empty batch returns)
    for kw in (dict(X=None), dict(inv=None), dict(a=None), dict(b=None), dict(counts=None), dict(ws=None),
               dict(rowptr=None), dict(col=None), dict(ws=p + 8), dict(ws_bytes=need() - 1), dict(ws_bytes=0)):
        assert rank(**kw) == _lib.EINVAL, kw
    rows, chunks = C.c_int64(), C.c_int32()
    assert L.n2v_link_rank_plan(1000, 64, 10, None, C.byref(chunks)) == _lib.EINVAL
    assert L.n2v_link_rank_plan(1000, 64, 10, C.byref(rows), None) == _lib.EINVAL
    assert L.n2v_link_rank_plan(1000, 0, 10, C.byref(rows), C.byref(chunks)) == _lib.EINVAL
    assert L.n2v_link_rank_plan(1000, 64, 10, C.byref(rows), C.byref(chunks)) == _lib.OK
    assert (rows.value, chunks.value) == (1024, 1)
    from node2vec_amd import linkpred

    n = lc.chunked_n(lambda n: linkpred.link_rank_plan(n, 128, 65))
    rows, chunks = linkpred.link_rank_plan(n, 128, 65)
    assert chunks >= 2 and rows % 128 == 0 and (chunks - 1) * rows < n < chunks * rows
    rows, chunks = linkpred.link_rank_plan(1 << 20, 128, 4096)
    assert chunks * ((4096 + 63) // 64) == 2048 and rows * chunks >= 1 << 20


def test_target_ranks_checks_its_arguments_before_the_gpu():
    from node2vec_amd import linkpred

    with pytest.raises(ValueError):
        linkpred.target_ranks(torch.zeros(4, 3), [0], [1], metric="euclidean")
    with pytest.raises(ValueError):
        linkpred.target_ranks(torch.zeros(4, 3), [0], [1])  # not on a device


@pytest.mark.parametrize("n,dim,nq,metric", [c for c in lc.shape_cases() if lc.rich(c[0], c[2])]
                         + [(2049, 128, 65, m) for m in lc.METRICS])
def test_cases_are_meaningful(oracle, n, dim, nq, metric):
    """the conditions tests/test_linkrank_gpu.py asserts before it compares, here for every such case at once"""
    case = lc.make_case(n, dim, nq, metric)
    lc.assert_meaningful(case, *lc.expected(oracle, case))
    if n >= 24:  # the graph's special rows and the queries on them
        deg = np.diff(case.rowptr)
        row = lambda u: case.col[case.rowptr[u]:case.rowptr[u + 1]]  # noqa: E731
        assert deg[0] == 0 and deg[1] == 1 and len(set(row(2))) >= 17 and len(set(row(2))) < deg[2]
        assert 3 in row(3) and len(set(row(3))) < deg[3]
        assert case.a[0] == 0 and case.a[1] == 1 and case.b[1] in row(1) and case.a[2] == 2
        assert case.a[3] == case.b[3] == 3 and (case.a[5], case.b[5]) == (case.a[2], case.b[2])


@pytest.mark.parametrize("metric", lc.METRICS)
def test_another_summation_order_counts_differently(oracle, metric):
    """specificity: on the case without equal rows, the restatement that sums d sequentially (order 1) gives other
    counts on some query -- so equality with order 0 pins the kernel's order, not just any correct dot product"""
    case = lc.make_case(1000, 128, 65, metric, kind="near")
    assert len(np.unique(case.X, axis=0)) == 1000
    c0, t0, _ = lc.expected(oracle, case, order=0)
    c1, t1, _ = lc.expected(oracle, case, order=1)
    assert (c0 != c1).any(axis=1).sum() >= 1
    assert np.allclose(t0, t1, rtol=1e-5, atol=1e-6)  # (the same numbers up to rounding)
