"""Link ranking on the GPU (node2vec_amd/linkpred.py, csrc/n2v_linkrank.hip) against the CPU restatement of the score
chain (n2v_oracle.knn_scores, through tests/linkrank_cases.py): the counts equal as integers, the thresholds as bit
patterns.  The cases walk the tile edges (n, dim, queries per tile, the unaligned path, a scan of several chunks), the
filter lists (no list, one entry, more than one list tile, multi-edges, a self-loop, v in F(u), u == v, a repeated
query), zero and NaN rows and the query batches; then the public interface end to end on the karate club.

karate (34 vertices, 78 edges, 16 of them held out, 10 walks of length 10 per vertex, dim 16, 3 epochs, deterministic):
the first run on an MI355X printed  MRR 0.2874  Hits@10 0.5938  mean rank 9.78  (32 queries; no threshold is asserted)."""
import numpy as np
import pandas as pd
import pytest
import torch

import linkrank_cases as lc
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _unaligned(X):
    """X on the device with its base 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(X, np.float32))
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _graph(case):
    from node2vec_amd.graph import DeviceGraph

    if case.rowptr is None:
        return None
    return DeviceGraph(_t(case.rowptr), _t(case.col), None)


def _run(case, Xd=None):
    from node2vec_amd import linkpred

    greater, equal, thr = linkpred.target_ranks(_t(case.X) if Xd is None else Xd, _t(case.a), _t(case.b),
                                                graph=_graph(case), metric=case.metric)
    assert greater.is_cuda and greater.dtype == equal.dtype == torch.int64 and thr.dtype == torch.float32
    return torch.stack((greater, equal), dim=1).cpu().numpy(), thr.cpu().numpy()


def _same(got, want, what=""):
    (gc, gt), (wc, wt) = got, want
    bad = np.nonzero((gc != wc).any(axis=1) | (gt.view(np.uint32) != wt.view(np.uint32)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} queries differ, first {bad[0]}: counts {gc[bad[0]]} want " \
                          f"{wc[bad[0]]}, thr {gt[bad[0]]!r} want {wt[bad[0]]!r}"


def _check(oracle, case, what, Xd=None, rich=True):
    counts, thr, S = lc.expected(oracle, case)
    if rich:
        lc.assert_meaningful(case, counts, thr, S)  # before the GPU is compared
    _same(_run(case, Xd), (counts, thr), what)


@pytest.mark.parametrize("n,dim,nq,metric", lc.shape_cases())
def test_counts_and_thresholds_at_the_tile_edges(oracle, n, dim, nq, metric):
    _check(oracle, lc.make_case(n, dim, nq, metric), (n, dim, nq, metric), rich=lc.rich(n, nq))


@pytest.mark.parametrize("metric", lc.METRICS)
def test_a_scan_of_several_chunks_with_a_ragged_last_one(oracle, metric):
    from node2vec_amd import linkpred

    n = lc.chunked_n(lambda n: linkpred.link_rank_plan(n, 128, 65))
    chunk_rows, n_chunks = linkpred.link_rank_plan(n, 128, 65)
    assert n_chunks >= 2 and n % chunk_rows != 0
    _check(oracle, lc.make_case(n, 128, 65, metric), (n, metric))


@pytest.mark.parametrize("metric", lc.METRICS)
def test_rows_that_are_not_16_byte_aligned(oracle, metric):
    case = lc.make_case(65, 128, 17, metric)
    _check(oracle, case, ("unaligned", metric), Xd=_unaligned(case.X))


@pytest.mark.parametrize("metric", lc.METRICS)
def test_without_a_filter(oracle, metric):
    case = lc.make_case(1000, 16, 65, metric, filtered=False)
    _check(oracle, case, ("no filter", metric))


@pytest.mark.parametrize("metric", lc.METRICS)
def test_the_summation_order_is_pinned(oracle, metric):
    """the case without equal rows, on which tests/test_linkrank_host.py shows that another order counts differently"""
    case = lc.make_case(1000, 128, 65, metric, kind="near")
    _check(oracle, case, ("near", metric))


def test_zero_and_nan_rows(oracle):
    """a zero row under cosine scores 0 against everything (inv_norm 0); a NaN row gives its own query (0, 0) and a NaN
    threshold, and is counted for no other query"""
    case = lc.make_case(200, 16, 40, "cosine")
    X = case.X.copy()
    zero, nan = 7, 11
    X[zero] = 0.0
    X[nan, 3] = np.nan
    a, b = case.a.copy(), case.b.copy()
    a[6:12] = (zero, 20, nan, 21, zero, 22)
    b[6:12] = (20, zero, 21, nan, zero, 22)
    case = case._replace(X=X, a=a, b=b)
    counts, thr, S = lc.expected(oracle, case)
    assert (S[:, zero][~np.isnan(S[:, zero])] == 0).all() and thr[7] == 0 and thr[6] == 0
    assert np.isnan(thr[8]) and np.isnan(thr[9]) and (counts[8] == 0).all() and (counts[9] == 0).all()
    assert counts[6, 1] > 0  # the zero query ties with every candidate
    got = _run(case)
    _same(got, (counts, thr), "zero / NaN")
    # the NaN row is never counted: the counts are those of the matrix without it, whatever it held
    live = [q for q in range(40) if nan not in (a[q], b[q])]
    other = X.copy()
    other[nan] = 1e30
    other[nan, 0] = -np.inf
    got_other = _run(case._replace(X=other))
    assert np.array_equal(got[0][live], got_other[0][live])
    with np.errstate(invalid="ignore"):
        for q in live:
            cand = S[q][~lc.excluded(case, q) & (np.arange(200) != nan)]
            assert (counts[q] == ((cand > thr[q]).sum(), (cand == thr[q]).sum())).all()


def test_query_batches_give_the_single_batch_result(oracle, monkeypatch):
    from node2vec_amd import _lib, linkpred, similarity

    case = lc.make_case(300, 16, 200, "cosine")
    want = lc.expected(oracle, case)[:2]
    whole = _run(case)
    _same(whole, want, "one batch")
    L = _lib.load()
    limit = L.n2v_link_rank_workspace_bytes(300, 16, 64)
    assert L.n2v_link_rank_workspace_bytes(300, 16, 65) > limit
    monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", limit)  # 200 -> 100 -> 50 queries a batch: 4 batches
    calls = []
    real = linkpred._dense.workspace
    monkeypatch.setattr(linkpred._dense, "workspace", lambda *a, **k: calls.append(a[-1]) or real(*a, **k))
    _same(_run(case), want, "batches")
    assert len(calls) >= 3 and sum(calls) == 200, calls


def test_empty_and_out_of_range_queries():
    from node2vec_amd import linkpred

    X = torch.randn(50, 16, device="cuda")
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    greater, equal, thr = linkpred.target_ranks(X, empty, empty)
    assert greater.shape == equal.shape == thr.shape == (0,)
    for a, b in (([0, 50], [1, 2]), ([0, 1], [-1, 2])):
        with pytest.raises(IndexError):
            linkpred.target_ranks(X, a, b)
    with pytest.raises(ValueError):
        from node2vec_amd.graph import DeviceGraph

        linkpred.target_ranks(X, [0], [1], graph=DeviceGraph(torch.zeros(4, dtype=torch.int64, device="cuda"),
                                                             torch.zeros(0, dtype=torch.int32, device="cuda"), None))


def test_end_to_end_on_the_karate_club():
    """no quality threshold: nobody has measured one (the first run's figures are in the module's docstring)"""
    from node2vec_amd import linkpred
    from node2vec_amd.embedding import Node2VecHIP
    from node2vec_amd.fugue import random_walk
    from node2vec_amd.graph import DeviceGraph

    e = np.array(load_golden("karate_edges.json"))
    g = DeviceGraph.from_edges(e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), n_vertices=34, device="cuda")
    train, ta, tb = linkpred.holdout_edges(g, 0.2, seed=5)
    n_test = int(ta.numel())
    assert n_test == round(0.2 * 78) and train.n_edges == g.n_edges - 2 * n_test
    assert not bool(linkpred.has_edge(train, ta, tb).any()) and not bool(linkpred.has_edge(train, tb, ta).any())
    assert bool(linkpred.has_edge(g, ta, tb).all()) and bool((train.degrees() > 0).all())
    src = torch.repeat_interleave(torch.arange(34, device="cuda"), train.degrees()).cpu().numpy()
    df_train = pd.DataFrame({"src": src, "dst": train.col.cpu().numpy(), "weight": 1.0})
    params = {"num_walks": 10, "walk_length": 10, "return_param": 1.0, "inout_param": 1.0}
    walks = random_walk("hip", df_train, params, random_seed=42)
    n2v = Node2VecHIP(walks, {"min_count": 0, "iter": 3, "size": 16, "negative": 5, "deterministic": True},
                      random_seed=1000)
    n2v.fit()
    wv = n2v.model.wv
    assert len(wv) == 34
    df_test = pd.DataFrame({"src": ta.cpu().numpy(), "dst": tb.cpu().numpy()})
    ks = (1, 3, 10)
    out = n2v.link_ranking(df_test, df_train[["src", "dst"]], ks=ks)
    assert list(out.columns) == ["mrr", "mean_rank", "hits@1", "hits@3", "hits@10", "n", "dropped"] and len(out) == 1
    row = out.iloc[0]
    print("karate link ranking: MRR %.4f Hits@10 %.4f mean rank %.2f" % (row["mrr"], row["hits@10"], row["mean_rank"]))
    assert row["n"] == 2 * n_test and row["dropped"] == 0
    assert 0.0 < row["mrr"] <= 1.0 and 1.0 <= row["mean_rank"] <= 34 and row["hits@1"] <= row["hits@3"] <= row["hits@10"]
    # the same numbers from the counts of KeyedVectors.target_ranks, both directions pooled
    a, b = ta.cpu().numpy(), tb.cpu().numpy()
    gr, eq, thr = wv.target_ranks(np.concatenate([a, b]), np.concatenate([b, a]), graph=train)
    assert gr.dtype == eq.dtype == np.int64 and thr.dtype == np.float32 and gr.shape == (2 * n_test,)
    again = linkpred.ranking_metrics(gr, eq, ks=ks)
    assert {k: row[k] for k in again} == again
    assert linkpred.link_ranking(train, wv, ta, tb, ks=ks) == dict(again, dropped=0)
    # thr is the pair's cosine as similarity.scores gives it, and the filter took train's neighbours out
    from node2vec_amd import similarity

    ra = torch.from_numpy(wv._rows_of_tokens(np.concatenate([a, b]))).cuda()
    rb = torch.from_numpy(wv._rows_of_tokens(np.concatenate([b, a]))).cuda()
    S = similarity.scores(wv._device_vectors(), rows=ra)
    assert torch.equal(S[torch.arange(2 * n_test, device="cuda"), rb].cpu().view(torch.int32), torch.from_numpy(thr).view(torch.int32))
    unfiltered = wv.target_ranks(np.concatenate([a, b]), np.concatenate([b, a]))
    assert (unfiltered[0] >= gr).all() and (unfiltered[0] > gr).any()
    one_way = n2v.link_ranking(df_test, df_train[["src", "dst"]], ks=ks, both=False)
    assert one_way.iloc[0]["n"] == n_test
    with pytest.raises(ValueError):
        n2v.link_ranking(df_test[["src"]])
