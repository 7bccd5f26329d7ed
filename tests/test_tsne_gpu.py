"""t-SNE on the GPU (csrc/n2v_tsne.hip through node2vec_amd.tsne) against the CPU restatement,
tests/cpu_tsne/n2v_tsne_cpu.c, bit for bit: the repulsion (rep, zrow, Z), the step (grad, Y_next, vel, gain) and the
loop of fit.  The sizes sit on the kernels' edges: a ragged wave, the tile, the first second column slab, a ragged
row block and tile at once, slabs of several tiles and more than 256 row blocks (Z's second pass).  Then the gradient
against the float64 definition within the host test's bounds, the affinities, the fit end to end and the public
surface."""
import numpy as np
import pandas as pd
import pytest
import torch

import tsne_cases as tc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return tc.build(tmp_path_factory.mktemp("tsne_cpu"))


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _check_repulse(cpu, Y, rows=None):
    """tsne.repulse on the device == the restatement by the library's plan, bit for bit (rows: only those rows of
    rep and zrow are restated; Z is then the restated order over the device's zrow)"""
    from node2vec_amd import tsne

    n = Y.shape[0]
    rep, zrow, Z = (t.cpu().numpy() for t in tsne.repulse(_dev(Y, np.float32)))
    w_rep, w_zrow = tc.repulse(cpu, Y, tsne.plan(n), rows)
    pick = slice(None) if rows is None else rows
    assert tc.same_bits(rep[pick], w_rep), ("rep", n, np.abs(rep[pick] - w_rep).max())
    assert tc.same_bits(zrow[pick], w_zrow), ("zrow", n)
    assert tc.same_bits(Z, np.array([tc.z_of(cpu, zrow)])), ("Z", n)
    return rep, zrow, Z


def _two_slabs():
    """the smallest n with two column slabs, read from the library's plan"""
    from node2vec_amd import tsne

    tile = tsne.plan(1)[0]
    n = tile + 1
    assert tsne.plan(tile)[2] == 1 and tsne.plan(n)[2] == 2
    return n, tsne.plan(n)[1]


def test_repulse_bitwise_over_the_sizes(cpu):
    from node2vec_amd import tsne

    tile = tsne.plan(1)[0]
    n2, slab_cols = _two_slabs()
    ragged = 2 * tile + 256 + 77  # a ragged row block and a ragged tile at once
    for n in (1, 2, 63, 64, 65, tile - 1, tile, tile + 1, n2, n2 + slab_cols + 1, ragged):
        _check_repulse(cpu, tc.normal_points(n, n, scale=3.0))
    assert tsne.plan(n2 + slab_cols + 1)[2] >= 3


def test_repulse_bitwise_on_long_slabs_and_past_256_row_blocks(cpu):
    """n = 66 001: 258 row blocks (Z's sum of the block sums takes a second pass of 256), slabs of several tiles;
    64 rows spread over the row blocks are restated"""
    from node2vec_amd import tsne

    n = 66001
    tile, slab_cols, n_slabs = tsne.plan(n)
    assert -(-n // 256) > 256 and slab_cols >= 2 * tile and n_slabs >= 2
    rows = np.unique(np.r_[0, 255, 256, n - 1, n - 2, 65536, np.random.default_rng(1).integers(0, n, 58)])
    _check_repulse(cpu, tc.normal_points(n, 9, scale=30.0), rows.astype(np.int64))


def test_repulse_special_values_and_the_same_bits_twice(cpu):
    Y = tc.normal_points(300, 5)
    Y[7] = Y[3]                                    # coincident: 1 in Z, nothing in the force
    Y[11] = [1e20, -1e20]                          # d2 overflows: w = 0
    Y[20] = np.nextafter(Y[19], np.float32(np.inf))  # one ulp apart: dx * dx underflows
    first = _check_repulse(cpu, Y)
    again = _check_repulse(cpu, Y)
    assert all(tc.same_bits(a, b) for a, b in zip(first, again))
    assert np.isfinite(first[0]).all() and first[1][11] == 0.0
    rep, zrow, Z = _check_repulse(cpu, np.array([[0.5, -1.0], [0.5, -1.0]], np.float32))
    assert rep.tolist() == [[0.0, 0.0], [0.0, 0.0]] and zrow.tolist() == [1.0, 1.0] and Z.tolist() == [2.0]
    rep, zrow, Z = _check_repulse(cpu, np.array([[3.0, 4.0]], np.float32))
    assert rep.tolist() == [[0.0, 0.0]] and Z.tolist() == [0.0]


def _gpu_step(csr, Y, rep, Z, ex, lr, mom, min_gain, vel, gain):
    from node2vec_amd import _lib

    rowptr, col, val = _dev(csr[0], np.int64), _dev(csr[1], np.int32), _dev(csr[2], np.float32)
    Yd, repd, Zd = _dev(Y, np.float32), _dev(rep, np.float64), _dev(np.array([Z]), np.float64)
    vel, gain = _dev(vel, np.float32), _dev(gain, np.float32)
    Y_next, grad = torch.zeros_like(Yd), torch.zeros_like(Yd)
    _lib.check(_lib.load().n2v_tsne_step(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), col.numel(),
                                         Yd.data_ptr(), repd.data_ptr(), Zd.data_ptr(), Y.shape[0], ex, lr, mom,
                                         min_gain, vel.data_ptr(), gain.data_ptr(), Y_next.data_ptr(), grad.data_ptr(),
                                         _lib.current_stream_ptr()), "n2v_tsne_step")
    assert torch.equal(Yd, _dev(Y, np.float32))  # Y is read only
    return tuple(t.cpu().numpy() for t in (Y_next, grad, vel, gain))


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_step_bitwise(cpu, exaggeration):
    """rows of 0, 1, 15, 16, 17, 33 and 200 entries, n = 203 (not a multiple of 4); velocities of both signs and
    zero, a row whose gradient is exactly zero (no entries, rep = 0), gains that the rule drives to min_gain"""
    n = 203
    lengths = [0, 1, 15, 16, 17, 33, 200]
    Y = tc.normal_points(n, 21, scale=2.0)
    csr = tc.random_csr(n, lengths, 22)
    assert sorted(set(np.diff(csr[0]).tolist())) == lengths
    rep, zrow = tc.repulse(cpu, Y, tc.host_plan(n))
    Z = tc.z_of(cpu, zrow)
    rep[0] = 0.0  # row 0 has no entries: g == 0 exactly
    rng = np.random.default_rng(23)
    vel = rng.standard_normal((n, 2)).astype(np.float32)
    vel[rng.random((n, 2)) < 0.2] = 0.0
    gain = (rng.random((n, 2)) * 2.0 + 0.5).astype(np.float32)
    gain[rng.random((n, 2)) < 0.3] = 0.011  # times 0.8 falls below min_gain
    args = (exaggeration, 37.5, 0.8, 0.01)
    want = tc.step(cpu, csr, Y, rep, Z, *args, vel, gain)
    got = _gpu_step(csr, Y, rep, Z, *args, vel, gain)
    for name, g, w in zip(("Y_next", "grad", "vel", "gain"), got, want):
        assert tc.same_bits(g, w), (name, np.abs(g - w).max())
    grad, new_gain = want[1], want[3]
    assert grad[0].tolist() == [0.0, 0.0]
    combos = {(bool(a), bool(b)) for a, b in zip((grad > 0).reshape(-1), (vel > 0).reshape(-1))}
    assert len(combos) == 4 and (vel[grad != 0] == 0).any()
    assert (new_gain == np.float32(0.01)).any() and (new_gain > np.float32(0.01)).any()


def test_fit_is_the_restated_loop_bit_for_bit(cpu):
    """6 iterations with exaggeration_iter = 2 and check_every = 3 from a given layout: the schedule's switches of
    exaggeration and momentum and the alternation of the two layout buffers"""
    from node2vec_amd import tsne

    n = 130
    X = torch.from_numpy(np.random.default_rng(31).standard_normal((n, 8)).astype(np.float32)).cuda()
    aff = tsne.affinities(X, 8.0)
    Y0 = tc.normal_points(n, 32, scale=1e-4)
    res = tsne.fit(aff, n_iter=6, exaggeration_iter=2, check_every=3, init=_dev(Y0))
    csr = tuple(t.cpu().numpy() for t in (aff.rowptr, aff.col, aff.val))
    Y, vel, gain, grad = tc.fit_loop(cpu, csr, Y0, tsne.plan(n), 6, 2, 12.0, max(n / 12.0 / 4.0, 50.0), (0.5, 0.8),
                                     0.01)
    assert res.n_iter == 6 and tc.same_bits(res.embedding.cpu().numpy(), Y)
    assert res.grad_norm == pytest.approx(float(np.sqrt((grad.astype(np.float64) ** 2).sum())), rel=1e-12)
    assert not np.array_equal(Y, Y0)


def test_gradient_against_float64_within_the_derived_bound():
    """n = 300 points at least 0.5 apart, P from affinities on random unit rows in dim 16: |grad - gradient64| <=
    tsne_cases.gradient_bound, the bound of the host test"""
    from node2vec_amd import tsne

    n = 300
    X = np.random.default_rng(41).standard_normal((n, 16)).astype(np.float32)
    aff = tsne.affinities(_dev(X), 12.0)
    Y = tc.lattice_points(n, 42)
    Pd = tc.dense_of(tuple(t.cpu().numpy() for t in (aff.rowptr, aff.col, aff.val)), n)
    assert np.array_equal(Pd, Pd.T)
    for ex in (1.0, 12.0):
        grad, Z = tsne.gradient(aff, _dev(Y), ex)
        err, bound = np.abs(grad.cpu().numpy() - tc.gradient64(Pd, Y, ex)), tc.gradient_bound(Pd, Y, ex)
        print(f"exaggeration {ex}: max error / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert abs(Z - tc.repulse64(Y)[2]) <= tc.repulse_bounds(Y)[2]
    kl = tsne.kl_divergence(aff, _dev(Y))
    assert kl == pytest.approx(tc.kl64(Pd, Y), rel=1e-6)


def test_affinities_on_the_device():
    from node2vec_amd import similarity, tsne

    n, perplexity = 200, 9.0
    X = _dev(np.random.default_rng(51).standard_normal((n, 12)).astype(np.float32))
    aff = tsne.affinities(X, perplexity)
    k = aff.k
    assert k == 27 and aff.perplexity == perplexity and aff.col.dtype == torch.int32 and aff.val.dtype == torch.float32
    idx, score = similarity.knn(X, k, rows=torch.arange(n, device="cuda"), exclude_self=True)
    Pd = tc.dense_of(tuple(t.cpu().numpy() for t in (aff.rowptr, aff.col, aff.val)), n)
    member = np.zeros((n, n), bool)
    member[np.repeat(np.arange(n), k), idx.cpu().numpy().reshape(-1)] = True
    assert np.array_equal(Pd > 0, member | member.T)  # the neighbour sets are knn's
    assert abs(Pd.sum() - 1.0) <= aff.col.numel() * 2.0 ** -24
    d2 = (2.0 * (1.0 - score.double())).clamp(min=0.0)
    p = tsne.calibrate(d2, perplexity)
    assert p.is_cuda
    got = tc.entropy_perplexity(p.cpu().numpy())
    assert (np.abs(got - perplexity) <= 1e-4 * perplexity).all()
    r, c, v = tsne.symmetrise(idx, p, n)
    assert torch.equal(r, aff.rowptr) and torch.equal(c, aff.col) and torch.equal(v, aff.val)
    # lists of the caller's own; -1 entries are dropped
    idx2 = idx.clone()
    idx2[:, -4:] = -1
    own = tsne.affinities(X, perplexity, neighbours=(idx2, d2))
    assert own.k == k
    Po = tc.dense_of(tuple(t.cpu().numpy() for t in (own.rowptr, own.col, own.val)), n)
    member[:] = False
    member[np.repeat(np.arange(n), k - 4), idx[:, :-4].cpu().numpy().reshape(-1)] = True
    assert np.array_equal(Po > 0, member | member.T)
    for bad in (n - 1, n, 0.5):
        with pytest.raises(ValueError, match="perplexity"):
            tsne.affinities(X, bad)
    with pytest.raises(ValueError, match="neighbours="):
        tsne.affinities(X, perplexity, metric="euclidean")


def test_fit_end_to_end_on_three_blobs():
    """three Gaussian blobs at tsne_cases.BLOB_SEPARATION, where the float64 reference optimiser leaves no point with
    a foreign nearest neighbour (test_tsne_host): at most 3 of 300 here"""
    from node2vec_amd import tsne

    X, labels = tc.blobs()
    Xd = _dev(X)
    kw = dict(perplexity=10.0, n_iter=300, exaggeration_iter=100)
    res = tsne.fit(Xd, **kw)
    Y = res.embedding
    assert res.n_iter == 300 and tuple(Y.shape) == (300, 2) and Y.dtype == torch.float32 and Y.is_cuda
    assert bool(torch.isfinite(Y).all()) and np.isfinite(res.grad_norm)
    first = tsne.fit(res.affinities, n_iter=0, init=Y)  # (the divergence of a layout, through fit)
    assert first.kl_divergence == res.kl_divergence == tsne.kl_divergence(res.affinities, Y)
    start = tsne.fit(Xd, n_iter=0, perplexity=10.0)
    print(f"KL {start.kl_divergence:.4f} -> {res.kl_divergence:.4f}; foreign nearest neighbours: "
          f"{tc.foreign_nearest(Y.cpu().numpy(), labels)}")
    assert res.kl_divergence < start.kl_divergence
    assert tc.foreign_nearest(Y.cpu().numpy(), labels) <= 3
    again = tsne.fit(Xd, **kw)
    assert torch.equal(again.embedding, Y) and again.kl_divergence == res.kl_divergence
    a = tsne.fit(res.affinities, n_iter=20, init="random", seed=1).embedding
    b = tsne.fit(res.affinities, n_iter=20, init="random", seed=1).embedding
    c = tsne.fit(res.affinities, n_iter=20, init="random", seed=2).embedding
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError, match="pca"):
        tsne.fit(res.affinities, n_iter=1)
    with pytest.raises(ValueError, match="non-finite"):
        tsne.fit(res.affinities, n_iter=4, check_every=2, init=torch.full((300, 2), float("nan"), device="cuda"))


def test_keyedvectors_tsne():
    from node2vec_amd import similarity, tsne
    from node2vec_amd.embedding import KeyedVectors

    X, _ = tc.blobs(per=40, seed=6)
    ids = np.arange(1000, 1120)
    kw = dict(n_iter=30, exaggeration_iter=10)
    Xd = _dev(X)
    want = tsne.fit(Xd, perplexity=7.0, inv_norm=similarity.inv_norms(Xd), **kw)
    for kv in (KeyedVectors(ids, X), KeyedVectors(ids, Xd)):
        res = kv.tsne(perplexity=7.0, **kw)
        assert torch.equal(res.embedding, want.embedding) and res.kl_divergence == want.kl_divergence
        part = kv.tsne(perplexity=7.0, restrict_vocab=50, **kw)
        assert tuple(part.embedding.shape) == (50, 2)
        assert torch.equal(part.embedding, tsne.fit(Xd[:50], perplexity=7.0, **kw).embedding)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_model_classes_map_their_vocabulary():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecGensim, Node2VecHIP, Node2VecSpark

    X, _ = tc.blobs(per=20, dim=8, seed=8)
    ids = np.arange(60)[::-1] + 100  # vocabulary order is not id order
    names = pd.DataFrame({"id": list(ids) + [159, 500], "name": [f"v{i}" for i in ids] + ["last", "unused"]})
    kw = dict(perplexity=5.0, n_iter=20, exaggeration_iter=10)
    assert Node2VecGensim is Node2VecHIP
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((60, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((59, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.tsne()
        n2v.model = model(KeyedVectors(ids, X))
        df = n2v.tsne(**kw)
        assert list(df.columns) == ["id", "x0", "x1"] and df["id"].tolist() == ids.tolist()
        want = n2v.model.wv.tsne(**kw).embedding.cpu().numpy()
        assert np.array_equal(df[["x0", "x1"]].to_numpy(), want)
        assert np.array_equal(n2v.tsne_result.embedding.cpu().numpy(), want)
        part = n2v.tsne(restrict_vocab=30, **kw)
        assert part["id"].tolist() == ids[:30].tolist()
        n2v.name_id = names
        named = n2v.tsne(**kw)
        assert list(named.columns) == ["name", "x0", "x1"]
        assert named["name"].tolist()[:2] == ["last", f"v{ids[1]}"]  # id 159 keeps its last name
        assert named["x0"].tolist() == df["x0"].tolist()
        n2v.name_id = names[names["id"] != 105]
        with pytest.raises(KeyError):
            n2v.tsne(**kw)
