"""Link prediction on the GPU (node2vec_amd/linkpred.py, csrc/n2v_pairs.hip): scores and edge features bit for
bit against the CPU restatement (tests/cpu_pairs/n2v_pairs_cpu.c) and numpy float32 at every lane-group
instance and on the ragged path, 64-bit offsets, has_edge against a Python set, the samplers, and the public
interface end to end on the karate club."""
import numpy as np
import pandas as pd
import pytest
import torch

import pairs_cases as pc
from conftest import load_golden

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 63, 64, 65, 100, 128, 129, 256, 300, 512, 1024)
N_PAIRS = (1, 63, 64, 65, 257, 10007)  # 10 007: no multiple of the pairs of a step, a wave or a block
ROWS = 300
ZERO_ROW, NAN_ROW = 5, 7


@pytest.fixture(scope="module")
def pairs_cpu(tmp_path_factory):
    return pc.build(tmp_path_factory.mktemp("pairs_cpu"))


def _matrix(dim):
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((ROWS, dim)).astype(np.float32)
    X[ZERO_ROW] = 0.0
    X[NAN_ROW, dim // 2] = np.nan
    return X


def _pair_list():
    """10 007 pairs over the 300 rows: a == b, the zero row, the NaN row on either side, a repeated pair, then
    random ones (with more repeats); every prefix of length >= 7 holds the special ones"""
    rng = np.random.default_rng(99)
    a, b = rng.integers(0, ROWS, N_PAIRS[-1]), rng.integers(0, ROWS, N_PAIRS[-1])
    head = [(3, 3), (ZERO_ROW, 9), (NAN_ROW, 2), (2, NAN_ROW), (ZERO_ROW, ZERO_ROW), (11, 12), (11, 12)]
    a[:len(head)], b[:len(head)] = zip(*head)
    a[5000:5100], b[5000:5100] = a[100:200], b[100:200]
    return a.astype(np.int64), b.astype(np.int64)


@pytest.fixture(scope="module")
def wanted(pairs_cpu):
    """per dim, computed once and shared: the matrix (host and device), the device's inverse norms, and the
    restatement's scores of the whole pair list for both metrics"""
    from node2vec_amd import similarity

    a, b = _pair_list()
    cache = {}

    def get(dim):
        if dim not in cache:
            X = _matrix(dim)
            Xd = torch.from_numpy(X).cuda()
            inv = similarity.inv_norms(Xd)
            want = {m: pc.scores(pairs_cpu, X, inv.cpu().numpy(), a, b, m) for m in ("dot", "cosine")}
            cache[dim] = (X, Xd, inv, want)
        return cache[dim]

    return a, b, get


@pytest.mark.parametrize("dim", DIMS)
def test_scores_equal_the_restatement_bit_for_bit(wanted, dim):
    from node2vec_amd import linkpred

    a, b, get = wanted
    X, Xd, inv, want = get(dim)
    for metric in ("dot", "cosine"):
        for n in N_PAIRS:
            got = linkpred.pair_scores(Xd, torch.from_numpy(a[:n]), torch.from_numpy(b[:n]), metric,
                                       inv_norm=inv if metric == "cosine" else None)
            assert got.dtype == torch.float32 and got.shape == (n,)
            assert pc.same_bits(got.cpu().numpy(), want[metric][:n]), (dim, metric, n)
    full = want["cosine"]
    assert full[1] == 0.0 and full[4] == 0.0  # a zero row scores 0
    assert np.isnan(full[2]) and np.isnan(full[3]) and np.isnan(want["dot"][2])  # a NaN row scores NaN
    assert full[5] == full[6] and not np.isnan(full[0])
    # the norms default to similarity.inv_norms(X); lists and numpy arrays are taken as indices
    got = linkpred.pair_scores(Xd, a[:65].tolist(), b[:65])
    assert pc.same_bits(got.cpu().numpy(), full[:65])
    assert linkpred.pair_scores(Xd, [], []).shape == (0,)


@pytest.mark.parametrize("dim", DIMS)
def test_scores_do_not_depend_on_place_batch_or_side(wanted, dim):
    from node2vec_amd import linkpred

    a, b, get = wanted
    _, Xd, inv, want = get(dim)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for metric in ("dot", "cosine"):
        rev = linkpred.pair_scores(Xd, ta.flip(0), tb.flip(0), metric, inv_norm=inv).flip(0)
        assert pc.same_bits(rev.cpu().numpy(), want[metric])
        swapped = linkpred.pair_scores(Xd, tb, ta, metric, inv_norm=inv)
        assert pc.same_bits(swapped.cpu().numpy(), want[metric])
        tail = linkpred.pair_scores(Xd, ta[4001:4500], tb[4001:4500], metric, inv_norm=inv)  # an unaligned slice
        assert pc.same_bits(tail.cpu().numpy(), want[metric][4001:4500])


@pytest.mark.parametrize("dim", DIMS)
def test_features_equal_numpy_float32_bit_for_bit(wanted, dim):
    from node2vec_amd import linkpred

    a, b, get = wanted
    X, Xd, _, _ = get(dim)
    for op in pc.OPS:
        want = pc.numpy_features(X, a, b, op)
        for n in N_PAIRS:
            got = linkpred.pair_features(Xd, torch.from_numpy(a[:n]), torch.from_numpy(b[:n]), op)
            assert got.dtype == torch.float32 and got.shape == (n, dim)
            assert pc.same_bits(got.cpu().numpy(), want[:n]), (dim, op, n)
    out = torch.full((257, dim), -7.0, device="cuda")
    ret = linkpred.pair_features(Xd, a[:257], b[:257], "l1", out=out)
    assert ret is out and pc.same_bits(out.cpu().numpy(), pc.numpy_features(X, a[:257], b[:257], "l1"))
    for bad in (torch.empty((256, dim), device="cuda"), torch.empty((257, dim)),
                torch.empty((257, dim), dtype=torch.float64, device="cuda"),
                torch.empty((dim, 257), device="cuda").t() if dim > 1 else torch.empty((257, 2), device="cuda")):
        with pytest.raises(ValueError):
            linkpred.pair_features(Xd, a[:257], b[:257], "l1", out=bad)
    assert linkpred.pair_features(Xd, [], [], "l2").shape == (0, dim)


def test_special_values_pass_through_the_operators(pairs_cpu):
    """-0.0, denormals, inf and NaN elements, at a full and a ragged dimension"""
    from node2vec_amd import linkpred

    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 1.0, -1.0],
                       np.float32)
    for dim in (64, 67):
        rng = np.random.default_rng(dim)
        X = special[rng.integers(0, special.size, (24, dim))]
        X[12] = -X[13]
        a, b = np.repeat(np.arange(24), 24), np.tile(np.arange(24), 24)
        Xd = torch.from_numpy(X).cuda()
        for op in pc.OPS:
            got = linkpred.pair_features(Xd, a, b, op).cpu().numpy()
            assert pc.same_bits(got, pc.numpy_features(X, a, b, op)), (dim, op)
            assert pc.same_bits(got, pc.features(pairs_cpu, X, a, b, op)), (dim, op)
        got = linkpred.pair_scores(Xd, a, b, "dot").cpu().numpy()
        assert pc.same_bits(got, pc.scores(pairs_cpu, X, None, a, b, "dot")), dim


def test_a_base_off_the_16_byte_grid_takes_the_element_path(wanted):
    """dim % 4 == 0, but X, or the features' out alone, starts 4 bytes past a 16-byte boundary: the same bits"""
    from node2vec_amd import linkpred

    def shifted(shape):
        out = torch.empty(shape[0] * shape[1] + 1, device="cuda")[1:].view(shape)
        assert out.data_ptr() % 16 == 4
        return out

    a, b, get = wanted
    X, Xd, inv, want = get(64)
    Xs = shifted(X.shape).copy_(Xd)
    for metric in ("dot", "cosine"):
        got = linkpred.pair_scores(Xs, a[:257], b[:257], metric, inv_norm=inv)
        assert pc.same_bits(got.cpu().numpy(), want[metric][:257]), metric
    feat = pc.numpy_features(X, a[:257], b[:257], "l2")
    for M, out in ((Xs, None), (Xd, shifted((257, 64)))):
        got = linkpred.pair_features(M, a[:257], b[:257], "l2", out=out)
        assert pc.same_bits(got.cpu().numpy(), feat), out is None


def test_offsets_past_2_31_elements(pairs_cpu):
    """rows whose first element lies beyond 2^31 floats of X (and of nothing else: X is never filled)"""
    from node2vec_amd import linkpred, similarity

    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"needs 12 GiB of free device memory for an 8 GiB matrix, {free >> 30} GiB are free")
    n, dim = 2 ** 21 + 3, 1024
    rows = np.array([0, n - 3, n - 2, n - 1], np.int64)
    assert (n - 3) * dim >= 2 ** 31
    small = np.random.default_rng(21).standard_normal((4, dim)).astype(np.float32)
    X = torch.empty((n, dim), device="cuda")
    X[torch.from_numpy(rows).cuda()] = torch.from_numpy(small).cuda()
    rng = np.random.default_rng(22)
    ia, ib = rng.integers(0, 4, 200), rng.integers(0, 4, 200)
    ia[:16], ib[:16] = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    inv_small = similarity.inv_norms(torch.from_numpy(small).cuda())
    inv = torch.zeros(n, device="cuda")
    inv[torch.from_numpy(rows).cuda()] = inv_small
    for metric in ("dot", "cosine"):
        got = linkpred.pair_scores(X, rows[ia], rows[ib], metric, inv_norm=inv).cpu().numpy()
        assert pc.same_bits(got, pc.scores(pairs_cpu, small, inv_small.cpu().numpy(), ia, ib, metric)), metric
    for op in pc.OPS:
        got = linkpred.pair_features(X, rows[ia], rows[ib], op).cpu().numpy()
        assert pc.same_bits(got, pc.numpy_features(small, ia, ib, op)), op
    with pytest.raises(MemoryError, match="chunks"):
        linkpred.pair_features(X, torch.zeros(2 ** 21, dtype=torch.int64), torch.zeros(2 ** 21, dtype=torch.int64))
    del X
    torch.cuda.empty_cache()


def _test_graph():
    """rows of 0, 1, 2, 3, 64, 65 and 5 000 entries; a self-loop (row 2), multi-edges (rows 3 and 6)"""
    from node2vec_amd.graph import DeviceGraph

    nv = 6000
    rng = np.random.default_rng(4)
    long_row = np.sort(rng.choice(np.arange(1, nv - 1), 4990, replace=False))
    rows = {1: [10], 2: [2, 50], 3: [7, 7, 9], 4: np.sort(rng.choice(np.arange(1, nv - 1), 64, replace=False)),
            5: np.sort(rng.choice(np.arange(1, nv - 1), 65, replace=False)),
            6: np.concatenate([long_row, long_row[:10]]), 5999: [5998]}
    src = np.concatenate([np.full(len(v), k) for k, v in rows.items()])
    dst = np.concatenate([np.asarray(v) for v in rows.values()])
    order = rng.permutation(src.size)  # from_edges sorts
    g = DeviceGraph.from_edges(src[order], dst[order], n_vertices=nv, device="cuda")
    assert g.n_edges == src.size and int(g.degrees()[6]) == 5000 and int(g.degrees()[0]) == 0
    return g, rows, set(zip(src.tolist(), dst.tolist())), nv


def test_has_edge_equals_the_edge_set():
    from node2vec_amd import linkpred

    g, rows, edges, nv = _test_graph()
    qa, qb = [], []
    for r, cols in rows.items():
        first, last = int(min(cols)), int(max(cols))
        for c in (first, last, first - 1, last + 1):
            qa.append(r)
            qb.append(c)
    for r in (0, 7, nv - 2):  # empty rows
        for c in (0, r, nv - 1):
            qa.append(r)
            qb.append(c)
    rng = np.random.default_rng(5)
    qa = np.concatenate([qa, rng.integers(0, 8, 10000), rng.integers(0, nv, 10000)])
    qb = np.concatenate([qb, rng.integers(0, nv, 20000)])
    assert qb.min() >= 0 and qb.max() < nv
    got = linkpred.has_edge(g, qa, qb)
    assert got.dtype == torch.bool and got.shape == (qa.size,)
    want = np.array([(int(u), int(v)) in edges for u, v in zip(qa, qb)])
    assert want.sum() > 500 and (~want).sum() > 5000
    assert np.array_equal(got.cpu().numpy(), want)
    assert linkpred.has_edge(g, [], []).shape == (0,)


def test_an_index_outside_the_rows_is_an_indexerror_before_any_launch():
    from node2vec_amd import linkpred

    X = torch.ones((10, 8), device="cuda")
    g, _, _, nv = _test_graph()
    for bad, n in ((-1, 10), (10, 10)):
        for a, b in (([0, bad], [1, 2]), ([0, 1], [bad, 2])):
            with pytest.raises(IndexError):
                linkpred.pair_scores(X, a, b)
            with pytest.raises(IndexError):
                linkpred.pair_features(X, a, b)
    for bad in (-1, nv):
        with pytest.raises(IndexError):
            linkpred.has_edge(g, [0, bad], [1, 2])
        with pytest.raises(IndexError):
            linkpred.has_edge(g, [0, 1], [bad, 2])
    with pytest.raises(ValueError):
        linkpred.pair_scores(X, [0, 1], [1])


def test_samplers_return_edges_and_non_edges():
    from node2vec_amd import linkpred, synthetic
    from node2vec_amd.graph import DeviceGraph

    g = synthetic.rmat(11, 6000, device="cuda")  # 2 048 vertex ids
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    src = np.repeat(np.arange(g.n_vertices), np.diff(rowptr))
    edges = set(zip(src.tolist(), col.tolist()))
    deg = np.diff(rowptr)
    n = 5000
    a, b = linkpred.sample_edges(g, n, seed=3)
    assert a.dtype == b.dtype == torch.int64 and a.shape == b.shape == (n,)
    pairs = list(zip(a.tolist(), b.tolist()))
    assert all(p in edges for p in pairs) and len(set(pairs)) > n // 4
    na, nb = linkpred.sample_non_edges(g, n, seed=3)
    assert na.dtype == nb.dtype == torch.int64 and na.shape == nb.shape == (n,)
    for u, v in zip(na.tolist(), nb.tolist()):
        assert u != v and (u, v) not in edges and (v, u) not in edges and deg[u] > 0 and deg[v] > 0
    for sampler in (linkpred.sample_edges, linkpred.sample_non_edges):
        again, other = sampler(g, n, seed=3), sampler(g, n, seed=4)
        first = sampler(g, n, seed=3)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        assert not (torch.equal(first[0], other[0]) and torch.equal(first[1], other[1]))
    # K8: no non-edge exists; the bounded number of rounds ends in an error
    u, v = np.nonzero(~np.eye(8, dtype=bool))
    k8 = DeviceGraph.from_edges(u, v, n_vertices=8, device="cuda")
    with pytest.raises(RuntimeError, match="graph too dense"):
        linkpred.sample_non_edges(k8, 10, seed=1)
    assert linkpred.sample_edges(k8, 10, seed=1)[0].shape == (10,)


@pytest.fixture(scope="module")
def karate():
    from node2vec_amd.fugue import random_walk
    from node2vec_amd.graph import DeviceGraph

    e = load_golden("karate_edges.json")
    df = pd.DataFrame(e, columns=["src", "dst", "weight"])
    params = {"num_walks": 10, "walk_length": 10, "return_param": 1.0, "inout_param": 1.0}
    walks = random_walk("hip", df, params, random_seed=42)  # the cfg 1 walks of tests/test_api_gpu.py
    g = DeviceGraph.from_edges(df["src"].to_numpy(), df["dst"].to_numpy(), n_vertices=34, device="cuda")
    return df[["src", "dst"]], walks, g


def _fit(kind, walks):
    from node2vec_amd.embedding import Node2VecHIP, Node2VecSpark

    if kind == "hip":
        n2v = Node2VecHIP(walks, {"min_count": 0, "iter": 3, "size": 16, "negative": 5, "deterministic": True},
                          random_seed=1000)
    else:
        n2v = Node2VecSpark(walks, {"minCount": 0, "maxIter": 2, "vectorSize": 16, "windowSize": 5,
                                    "deterministic": True}, random_seed=1000)
    n2v.fit()
    return n2v


@pytest.mark.parametrize("kind", ["hip", "spark"])
def test_end_to_end_on_the_karate_club(karate, pairs_cpu, kind):
    from node2vec_amd import linkpred, similarity

    df_edges, walks, g = karate
    n2v = _fit(kind, walks)
    wv = n2v.model.wv
    src, dst = df_edges["src"].to_numpy(), df_edges["dst"].to_numpy()
    rows_a = np.array([wv.vocab[str(v)] for v in src])
    rows_b = np.array([wv.vocab[str(v)] for v in dst])
    X = wv.vectors
    inv = similarity.inv_norms(torch.from_numpy(X).cuda()).cpu().numpy()
    # 1. link_scores == wv.pair_scores on the same ids (== the restatement)
    for metric in ("cosine", "dot"):
        out = n2v.link_scores(df_edges, metric)
        assert list(out.columns) == ["src", "dst", "score"] and len(out) == len(df_edges)
        assert np.array_equal(out["src"].to_numpy(), src) and np.array_equal(out["dst"].to_numpy(), dst)
        direct = wv.pair_scores(src, dst, metric)
        assert direct.dtype == np.float32
        assert pc.same_bits(out["score"].to_numpy(), direct)
        assert pc.same_bits(direct, wv.pair_scores([str(v) for v in src], [str(v) for v in dst], metric))
        assert pc.same_bits(direct, pc.scores(pairs_cpu, X, inv, rows_a, rows_b, metric))
    # 2. link_auc == the O(P N) count over the scores of the same samples
    n = 200
    pos, neg = linkpred.sample_edges(g, n, 5), linkpred.sample_non_edges(g, n, 6)
    res = linkpred.link_auc(g, wv, n, seed=5, center=False)
    s_pos = wv.pair_scores(pos[0].tolist(), pos[1].tolist())
    s_neg = wv.pair_scores(neg[0].tolist(), neg[1].tolist())
    assert set(res) == {"auc", "pairs_pos", "pairs_neg", "dropped"}
    assert res["auc"] == pc.auc_quadratic(s_pos, s_neg) == linkpred.auc(s_pos, s_neg)
    assert (res["pairs_pos"], res["pairs_neg"], res["dropped"]) == (n, n, 0)
    res = linkpred.link_auc(g, wv, n, seed=5)  # centred, as the quality scripts score
    Xc = wv._device_vectors() - wv._device_vectors().mean(dim=0, keepdim=True)
    row = lambda t: torch.tensor([wv.vocab[str(v)] for v in t.tolist()])  # noqa: E731
    s_pos = linkpred.pair_scores(Xc, row(pos[0]), row(pos[1])).cpu().numpy()
    s_neg = linkpred.pair_scores(Xc, row(neg[0]), row(neg[1])).cpu().numpy()
    assert res["auc"] == pc.auc_quadratic(s_pos, s_neg) and 0.0 <= res["auc"] <= 1.0
    # 3. edge_embedding == the numpy product of the vertices' vectors
    for op in pc.OPS:
        emb = n2v.edge_embedding(df_edges, op)
        assert list(emb.columns) == ["src", "dst", "vector"] and len(emb) == len(df_edges)
        got = np.array(emb["vector"].tolist(), dtype=np.float32)
        va = np.stack([wv[str(v)] for v in src]).astype(np.float32)
        vb = np.stack([wv[str(v)] for v in dst]).astype(np.float32)
        both = np.concatenate([va, vb])
        k = len(src)
        assert pc.same_bits(got, pc.numpy_features(both, np.arange(k), np.arange(k) + k, op)), op
    assert pc.same_bits(np.array(n2v.edge_embedding(df_edges)["vector"].tolist(), dtype=np.float32), va * vb)
    with pytest.raises(KeyError):
        n2v.link_scores(pd.DataFrame({"src": [0, 99], "dst": [1, 2]}))
