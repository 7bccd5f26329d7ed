"""UMAP on the GPU (csrc/n2v_umap.hip through node2vec_amd.umap) against the CPU restatement,
tests/cpu_umap/n2v_umap_cpu.c, bit for bit: x^b over the sweeps, one epoch over the graph and parameter cases on any
launch geometry, and the loop of fit.  The graph cases put rows on both sides of the lane / wave split (LONG entries),
on no entries, on entries that never fire, on columns out of range and on coincident points.  Then the fit end to end
and the public surface."""
import numpy as np
import pandas as pd
import pytest
import torch

import umap_cases as uc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return uc.build(tmp_path_factory.mktemp("umap_cpu"))


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def test_powb_bitwise_over_the_sweeps(cpu):
    """2^-40 .. 2^40, the subnormal arguments, both ends of the normal range, the mantissa's split and 1, and what is
    not positive; b == 1 gives the argument itself"""
    from node2vec_amd import umap

    x = np.concatenate([uc.powb_sweep(), uc.powb_edges()])
    assert (x[x > 0] < 2.0 ** -126).any() and (x == np.float32(2.0 ** -126)).any() and np.isinf(x).any()
    xd = _dev(x)
    for b in uc.BS + (1.0,):
        got = umap.powb(xd, b).cpu().numpy()
        assert uc.same_bits(got, uc.powb(cpu, x, b)), b
    assert torch.equal(umap.powb(xd, 1.0)[xd > 0], xd[xd > 0])


def _gpu_epoch(csr, Y, e, a, b, gamma, alpha, negative, seed, max_blocks):
    from node2vec_amd import umap

    Yd = _dev(Y, np.float32)
    keep = Yd.clone()
    out = torch.full_like(Yd, float("nan"))
    umap.epoch(csr[0], csr[1], csr[2], Yd, out, e, a, b, gamma, alpha, negative, seed, max_blocks)
    assert torch.equal(Yd, keep)  # Y is read only
    return out.cpu().numpy()


PARAMS = [(negative, ab, e) for negative in (0, 1, 5) for ab in ((1.0, 1.0), uc.AB) for e in (0, 7)]


@pytest.mark.parametrize("n", [1, 2, 63, 257, 1000])
def test_epoch_bitwise_on_any_launch_geometry(cpu, n):
    """negative in {0, 1, 5} x (a, b) in {(1, 1), umap-learn's} x epoch in {0, 7}, each with max_blocks in {0, 1, 3};
    the seed is one for which a draw hits its own row (n >= 2)"""
    csr, Y = uc.graph_case(n, 100 + n)
    lengths = np.diff(csr[0])
    if n == 1000:
        assert {0, 70, 300, uc.LONG, uc.LONG + 1} <= set(lengths.tolist())
    dcsr = (_dev(csr[0], np.int64), _dev(csr[1], np.int32), _dev(csr[2], np.float32))
    for negative, (a, b), e in PARAMS:
        seed = uc.self_draw_seed(cpu, csr, Y, e, negative) if negative and n > 1 else 3
        want, hits = uc.epoch(cpu, csr, Y, e, a, b, 1.0, 0.75, negative, seed)
        assert hits > 0 or negative == 0 or n == 1
        for max_blocks in (0, 1, 3):
            got = _gpu_epoch(dcsr, Y, e, a, b, 1.0, 0.75, negative, seed, max_blocks)
            assert uc.same_bits(got, want), (n, negative, a, b, e, max_blocks, np.abs(got - want).max())
    if n > 5:
        assert not uc.same_bits(want, Y) and uc.same_bits(want[0], Y[0])  # row 0 has no entries: it copies


def test_epoch_on_a_self_loop_and_on_far_points(cpu):
    """n = 1 with an entry on itself: every draw hits the row; points 1e20 apart: d2 overflows, the moves are what
    the restatement gives (NaN included)"""
    one = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([1.0], np.float32))
    Y = np.array([[0.5, -2.0]], np.float32)
    dcsr = (_dev(one[0]), _dev(one[1]), _dev(one[2]))
    want, hits = uc.epoch(cpu, one, Y, 0, *uc.AB, 1.0, 1.0, 5, 9)
    assert hits == 5 and uc.same_bits(_gpu_epoch(dcsr, Y, 0, *uc.AB, 1.0, 1.0, 5, 9, 0), want)
    csr, Y = uc.graph_case(63, 7)
    Y[3] = [1e20, -1e20]
    Y[9] = [3e38, 3e38]
    dcsr = (_dev(csr[0], np.int64), _dev(csr[1], np.int32), _dev(csr[2], np.float32))
    want, _ = uc.epoch(cpu, csr, Y, 2, *uc.AB, 1.0, 0.5, 5, 1)
    assert uc.same_bits(_gpu_epoch(dcsr, Y, 2, *uc.AB, 1.0, 0.5, 5, 1, 0), want)


def test_fit_is_the_restated_loop_bit_for_bit(cpu):
    """5 epochs on n = 257 with check_every = 2 from a given layout: the alternation of the two layout buffers and the
    step-size schedule; two calls give the same bits, another seed other bits"""
    from node2vec_amd import umap

    n = 257
    X = _dev(np.random.default_rng(31).standard_normal((n, 8)).astype(np.float32))
    g = umap.fuzzy_graph(X, 10)
    assert g.n_neighbors == 10 and int((g.rowptr[1:] - g.rowptr[:-1]).min()) >= 10
    Y0 = (np.random.default_rng(32).uniform(-10, 10, (n, 2))).astype(np.float32)
    kw = dict(n_epochs=5, a=uc.AB[0], b=uc.AB[1], learning_rate=1.0, check_every=2, init=_dev(Y0))
    res = umap.fit(g, seed=4, **kw)
    csr = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), umap.epochs_per_sample(g.val).cpu().numpy())
    want = uc.fit_loop(cpu, csr, Y0, 5, uc.AB[0], uc.AB[1], seed=4)
    assert res.n_epochs == 5 and (res.a, res.b) == uc.AB and uc.same_bits(res.embedding.cpu().numpy(), want)
    assert not np.array_equal(want, Y0)
    assert torch.equal(umap.fit(g, seed=4, **kw).embedding, res.embedding)
    assert not torch.equal(umap.fit(g, seed=5, **kw).embedding, res.embedding)
    with pytest.raises(ValueError, match="pca"):
        umap.fit(g, n_epochs=1)
    with pytest.raises(ValueError, match="non-finite"):
        umap.fit(g, n_epochs=4, check_every=2, init=torch.full((n, 2), float("nan"), device="cuda"))


def test_fuzzy_graph_on_the_device():
    from node2vec_amd import similarity, umap

    n, k = 200, 12
    X = _dev(np.random.default_rng(51).standard_normal((n, 12)).astype(np.float32))
    g = umap.fuzzy_graph(X, k)
    idx, score = similarity.knn(X, k, rows=torch.arange(n, device="cuda"), exclude_self=True)
    own = umap.fuzzy_graph(X, neighbours=(idx, (1.0 - score.double()).clamp(min=0.0)))
    assert all(torch.equal(p, q) for p, q in zip(g[:3], own[:3])) and g.col.is_cuda
    dense = torch.zeros((n, n), device="cuda")
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), g.rowptr[1:] - g.rowptr[:-1])
    dense[rows, g.col.long()] = g.val
    member = torch.zeros((n, n), dtype=torch.bool, device="cuda")
    member[torch.arange(n, device="cuda")[:, None].expand_as(idx), idx] = True
    assert torch.equal(dense > 0, member | member.T) and torch.equal(dense, dense.T)
    assert 1.0 - 2.0 ** -23 <= float(dense.max()) <= 1.0  # every row's nearest neighbour is a full member


def test_fit_end_to_end_on_three_blobs():
    """three Gaussian blobs at umap_cases.BLOB_SEPARATION, where the restated loop leaves no point with a foreign
    nearest neighbour (test_umap_host): none here either, from the device's own neighbours and PCA layout"""
    from node2vec_amd import umap

    X, labels = uc.blobs(separation=uc.BLOB_SEPARATION)
    res = umap.fit(_dev(X), n_epochs=200)
    Y = res.embedding
    assert res.n_epochs == 200 and tuple(Y.shape) == (300, 2) and Y.dtype == torch.float32 and Y.is_cuda
    assert bool(torch.isfinite(Y).all()) and res.graph.n_neighbors == 15
    assert abs(res.a - uc.AB[0]) <= 1e-3 and abs(res.b - uc.AB[1]) <= 1e-3
    print(f"foreign nearest neighbours: {uc.foreign_nearest(Y.cpu().numpy(), labels)}")
    assert uc.foreign_nearest(Y.cpu().numpy(), labels) == 0
    start = umap.fit(_dev(X), n_epochs=0).embedding
    assert float(start.min()) == 0.0 and float(start.max()) == 10.0 and not torch.equal(start, Y)
    a = umap.fit(res.graph, n_epochs=10, init="random", seed=1).embedding
    b = umap.fit(res.graph, n_epochs=10, init="random", seed=1).embedding
    c = umap.fit(res.graph, n_epochs=10, init="random", seed=2).embedding
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_keyedvectors_umap():
    from node2vec_amd import similarity, umap
    from node2vec_amd.embedding import KeyedVectors

    X, _ = uc.blobs(per=40, seed=6)
    ids = np.arange(1000, 1120)
    kw = dict(n_epochs=20)
    Xd = _dev(X)
    want = umap.fit(Xd, n_neighbors=9, inv_norm=similarity.inv_norms(Xd), **kw)
    for kv in (KeyedVectors(ids, X), KeyedVectors(ids, Xd)):
        res = kv.umap(n_neighbors=9, **kw)
        assert torch.equal(res.embedding, want.embedding) and torch.equal(res.graph.val, want.graph.val)
        part = kv.umap(n_neighbors=9, restrict_vocab=50, **kw)
        assert tuple(part.embedding.shape) == (50, 2)
        assert torch.equal(part.embedding, umap.fit(Xd[:50], n_neighbors=9, **kw).embedding)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_model_classes_map_their_vocabulary():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    X, _ = uc.blobs(per=20, dim=8, seed=8)
    ids = np.arange(60)[::-1] + 100  # vocabulary order is not id order
    names = pd.DataFrame({"id": list(ids), "name": [f"v{i}" for i in ids]})
    kw = dict(n_neighbors=6, n_epochs=10)
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((60, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((59, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        assert n2v.umap_result is None
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.umap()
        n2v.model = model(KeyedVectors(ids, X))
        df = n2v.umap(**kw)
        assert list(df.columns) == ["id", "x0", "x1"] and df["id"].tolist() == ids.tolist()
        want = n2v.model.wv.umap(**kw).embedding.cpu().numpy()
        assert np.array_equal(df[["x0", "x1"]].to_numpy(), want)
        assert np.array_equal(n2v.umap_result.embedding.cpu().numpy(), want)
        part = n2v.umap(restrict_vocab=30, **kw)
        assert part["id"].tolist() == ids[:30].tolist()
        n2v.name_id = names
        named = n2v.umap(**kw)
        assert list(named.columns) == ["name", "x0", "x1"]
        assert named["name"].tolist()[:2] == [f"v{ids[0]}", f"v{ids[1]}"]
        assert named["x0"].tolist() == df["x0"].tolist()
