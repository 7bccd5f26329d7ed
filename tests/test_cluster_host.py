"""k-means (node2vec_amd/cluster.py, csrc/n2v_kmeans.hip), the parts that need no GPU: the CPU restatement
(tests/cpu_kmeans/n2v_kmeans_cpu.c) against float64 numpy and on the contract's rules, the C ABI's argument
checks, the header and the binding, the argument checks of the Python layer and the k-means++ draw."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import kmeans_cases as kc
from conftest import ROOT

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def cpu(tmp_path_factory):
    return kc.build(tmp_path_factory.mktemp("kmeans_cpu"))


CASES = [(300, 32, 2), (300, 64, 7), (200, 100, 16), (200, 129, 33), (150, 256, 64)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("n,dim,k", CASES)
def test_restated_labels_are_the_float64_argmin_outside_the_rounding_bound(cpu, n, dim, k, metric):
    """t(c, r) as computed differs from the exact value by at most B = gamma_(dim_pad + 2) (2 sum |x_i c_i| +
    sum c_i^2): a dot chain of dim_pad fmaf (Higham 3.1: gamma_dim_pad sum |x_i c_i|, doubled by the factor
    -2, which is exact), a sum of squares of dim terms in some order (gamma_dim sum c_i^2), and the one rounding
    of the final fmaf, all within gamma_(dim_pad + 2) of the magnitudes.  For cosine t = -dot and B =
    gamma_dim_pad sum |x_i c_i|.  Where the float64 gap between the best and the second best t exceeds the two
    bounds, the label is the float64 argmin; the rows inside the bound are skipped and are at most 1 %."""
    X, Cm = kc.normal_case(n, dim, k, 17 * dim + k)
    inv = kc.inv_norms(cpu, X)
    if metric == "cosine":
        Cm = kc.unit(cpu, Cm)
    labels, dist = kc.assign(cpu, X, inv, Cm, metric)
    X64, C64 = X.astype(np.float64), Cm.astype(np.float64)
    dp = (dim + 15) // 16 * 16
    mag = np.abs(X64) @ np.abs(C64).T
    if metric == "euclidean":
        t = (C64 ** 2).sum(1)[None, :] - 2.0 * (X64 @ C64.T)
        bound = gamma(dp + 2) * (2.0 * mag + (C64 ** 2).sum(1)[None, :])
        want_dist = t.min(1) + (X64 ** 2).sum(1)
        dist_tol = bound.max(1) + gamma(dim + 2) * (X64 ** 2).sum(1) + U * np.abs(want_dist)
    else:
        t = -(X64 @ C64.T)
        bound = gamma(dp) * mag
        norm = np.sqrt((X64 ** 2).sum(1))
        want_dist = 1.0 + t.min(1) / norm
        dist_tol = bound.max(1) / norm + gamma(dim + 6) + 2 * U
    order = np.sort(t, axis=1)
    decided = np.ones(n, bool) if k == 1 else (order[:, 1] - order[:, 0]) > 2.0 * bound.max(1)
    assert (~decided).sum() <= 0.01 * n, (~decided).sum()
    assert np.array_equal(labels[decided], t.argmin(1)[decided])
    assert (np.abs(dist.astype(np.float64) - np.maximum(want_dist, 0.0)) <= dist_tol).all()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("n,dim,k", CASES)
def test_restated_centroids_are_the_float64_means_within_the_rounding_bound(cpu, n, dim, k, metric):
    """a cluster's sum is m fp32 additions per slab and one fp64 addition per slab (exact to far below fp32), so
    |sum - exact| <= gamma_m sum |v_r[d]|; the division and the rounding to fp32 add two roundings.  For cosine
    the summand x * inv_norm carries gamma_(dim + 4) of its own, and the normalisation the relative error of the
    norm of the sum: gamma_(m + 2 dim + 16) (A_d / |s| + |want_d| (1 + |A| / |s|)), A_d = sum |v_r[d]|."""
    X, _ = kc.normal_case(n, dim, k, 5 * dim + k)
    rng = np.random.default_rng(dim)
    labels = rng.integers(0, k, n).astype(np.int32)
    prev = rng.standard_normal((k, dim)).astype(np.float32)
    inv = kc.inv_norms(cpu, X)
    got, counts = kc.update(cpu, X, inv, labels, k, metric, prev)
    assert np.array_equal(counts, np.bincount(labels, minlength=k))
    X64 = X.astype(np.float64)
    for c in range(k):
        rows = X64[labels == c]
        m = len(rows)
        if m == 0:
            assert np.array_equal(got[c].view(np.uint32), prev[c].view(np.uint32))
            continue
        if metric == "euclidean":
            want = rows.mean(0)
            tol = gamma(m + 2) * np.abs(rows).sum(0) / m + U * np.abs(want)
        else:
            unit = rows / np.sqrt((rows ** 2).sum(1))[:, None]
            s, A = unit.sum(0), np.abs(unit).sum(0)
            ns = np.sqrt((s ** 2).sum())
            want = s / ns
            tol = gamma(m + 2 * dim + 16) * (A / ns + np.abs(want) * (1.0 + np.sqrt((A ** 2).sum()) / ns))
        assert (np.abs(got[c].astype(np.float64) - want) <= tol).all(), (c, m)


def test_restated_dot_is_the_chain_the_contract_spells(cpu):
    """the order (d0, j, k) with d = d0 + 4 k + j against a replay in exact arithmetic, rounded once per step"""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    for dim in (1, 3, 16, 17, 100):
        c, x = rng.standard_normal(dim).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
        acc = np.float32(0.0)
        for d0 in range(0, (dim + 15) // 16 * 16, 16):
            for j in range(4):
                for k in range(4):
                    d = d0 + 4 * k + j
                    if d < dim:  # a padded term adds +0 * +0 and changes nothing but the sign of a zero sum
                        exact = Fraction(float(x[d])) * Fraction(float(c[d])) + Fraction(float(acc))
                        acc = _round_f32(exact)  # ONE rounding of the exact fused result
        assert kc.dot(cpu, c, x) == acc, dim


def _round_f32(exact):
    """the float32 nearest to an exact rational (ties to even)"""
    from fractions import Fraction

    if exact == 0:
        return np.float32(0.0)
    lo = np.float32(float(exact))
    best = lo
    for cand in (np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))):
        d_best, d_cand = abs(Fraction(float(best)) - exact), abs(Fraction(float(cand)) - exact)
        if d_cand < d_best or (d_cand == d_best and (cand.view(np.uint32) & 1) == 0 and (best.view(np.uint32) & 1)):
            best = cand
    return best


def test_ties_go_to_the_lowest_index(cpu):
    X, Cm = kc.normal_case(50, 32, 6, 1)
    Cm[4] = Cm[1]  # duplicates: never the later one
    Cm[5] = Cm[0]
    for metric in ("euclidean", "cosine"):
        Cu = kc.unit(cpu, Cm) if metric == "cosine" else Cm
        labels, _ = kc.assign(cpu, X, kc.inv_norms(cpu, X), Cu, metric)
        assert not np.isin(labels, (4, 5)).any() and np.isin(labels, (0, 1)).any()
    # integer rows on the middle plane of two integer centres: every t is exact, the tie is exact
    Cm = np.zeros((3, 4), np.float32)
    Cm[0, 0], Cm[1, 0], Cm[2, 1] = 2.0, -2.0, 50.0
    X = np.array([[0, 1, 2, 3], [0, -4, 1, 0], [1, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
    labels, dist = kc.assign(cpu, X, None, Cm, "euclidean")
    assert labels.tolist() == [0, 0, 0, 1]
    assert dist.tolist() == [18.0, 21.0, 1.0, 1.0]


def test_empty_clusters_nan_rows_and_labels_that_are_none(cpu):
    X, Cm = kc.normal_case(200, 16, 4, 2)
    X[7] = np.nan
    X[9, 3] = np.nan
    Cm[3] = 1e3  # far from every row: stays empty
    for metric in ("euclidean", "cosine"):
        Cu = kc.unit(cpu, Cm) if metric == "cosine" else Cm
        if metric == "cosine":
            Cu[3] = -Cu[0]  # the opposite of a centre no row prefers to its own
            Cu[0] = kc.unit(cpu, X[:1])[0]
        inv = kc.inv_norms(cpu, X)
        labels, dist, out, counts, stats = kc.step(cpu, X, inv, Cu, metric, np.full(200, -1))
        assert labels[7] == labels[9] == -1 and np.isnan(dist[[7, 9]]).all() and stats[1] == 2
        assert stats[0] == 198 and counts.sum() == 198
        empty = np.nonzero(counts == 0)[0]
        for c in empty:
            assert np.array_equal(out[c].view(np.uint32), Cu[c].view(np.uint32))
        assert not np.isnan(out).any()  # the NaN rows joined no sum
        # labels outside [-1, k) are treated as -1
        wild = labels.copy()
        wild[:5] = [4, 1 << 20, -2, -(1 << 31), 1000]
        tame = wild.copy()
        tame[:5] = -1
        a, ca = kc.update(cpu, X, inv, wild, 4, metric, Cu)
        b, cb = kc.update(cpu, X, inv, tame, 4, metric, Cu)
        assert kc.same_bits(a, b) and np.array_equal(ca, cb)
        # step == assign, then update
        l2, d2 = kc.assign(cpu, X, inv, Cu, metric)
        o2, c2 = kc.update(cpu, X, inv, l2, 4, metric, Cu)
        assert np.array_equal(l2, labels) and kc.same_bits(d2, dist) and kc.same_bits(o2, out)
        assert np.array_equal(c2, counts)


def test_cosine_zero_rows_and_zero_sums(cpu):
    X, Cm = kc.normal_case(40, 8, 3, 4)
    X[3] = 0.0
    X[4] = -0.0
    Cu = kc.unit(cpu, Cm)
    inv = kc.inv_norms(cpu, X)
    labels, dist = kc.assign(cpu, X, inv, Cu, "cosine")
    assert labels[3] == labels[4] == 0 and dist[3] == dist[4] == 1.0
    # a cluster whose unit rows cancel keeps its centroid
    X[10], X[11] = X[12], -X[12]
    lab = np.full(40, -1, np.int32)
    lab[[10, 11]] = 2
    out, counts = kc.update(cpu, X, kc.inv_norms(cpu, X), lab, 3, "cosine", Cu)
    assert counts.tolist() == [0, 0, 2] and kc.same_bits(out, Cu)


def test_slab_size_is_the_documented_function(cpu, lib):
    for n, dim, k in ((1, 1, 1), (257, 64, 8), (10 ** 7, 128, 64), (10 ** 8, 1024, 1024), (2 ** 31 - 1, 64, 1024)):
        s = kc.slab_rows(cpu, n, dim, k)
        most = min(2048, (512 << 20) // (4 * k * dim))
        assert s == (max(1, -(-n // most)) + 63) // 64 * 64 == lib.n2v_kmeans_slab_rows(n, dim, k)
        assert lib.n2v_kmeans_workspace_bytes(n, dim, k) <= (512 << 20) + 4 * 1024 * 1025 + 1024
    assert lib.n2v_kmeans_workspace_bytes(0, 64, 8) == 0
    assert lib.n2v_kmeans_workspace_bytes(10, 0, 8) == -1 and lib.n2v_kmeans_slab_rows(10, 64, 1025) == -1


def test_kmeans_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; n == 0 is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    q = p + 1024
    big = 1 << 40

    def assign(X=p, inv=p, n=10, dim=16, cen=p, k=4, metric=1, labels=p, dist=p, ws=p, ws_bytes=big):
        return lib.n2v_kmeans_assign(X, inv, n, dim, cen, k, metric, labels, dist, ws, ws_bytes, None)

    def update(X=p, inv=p, n=10, dim=16, labels=p, k=4, metric=1, cen=p, out=q, counts=p, ws=p, ws_bytes=big):
        return lib.n2v_kmeans_update(X, inv, n, dim, labels, k, metric, cen, out, counts, ws, ws_bytes, None)

    def step(X=p, inv=p, n=10, dim=16, cen=p, k=4, metric=1, labels=p, dist=p, out=q, counts=p, stats=p, ws=p,
             ws_bytes=big):
        return lib.n2v_kmeans_step(X, inv, n, dim, cen, k, metric, labels, dist, out, counts, stats, ws, ws_bytes,
                                   None)

    for call in (assign, update, step):
        assert call(n=0) == _lib.OK and call(n=0, dim=1, k=1) == _lib.OK and call(n=0, dim=1024, k=1024) == _lib.OK
        assert call(n=0, metric=0, inv=None) == _lib.OK
        for kw in (dict(dim=0), dict(dim=1025), dict(k=0), dict(k=1025), dict(n=-1), dict(n=1 << 31),
                   dict(metric=-1), dict(metric=2), dict(inv=None), dict(X=None), dict(cen=None), dict(labels=None),
                   dict(ws=None), dict(ws=p + 4), dict(ws_bytes=0),
                   dict(ws_bytes=lib.n2v_kmeans_workspace_bytes(10, 16, 4) - 1)):
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
        for kw in (dict(dim=0), dict(k=1025), dict(metric=2), dict(inv=None)):
            assert call(n=0, **kw) == _lib.EINVAL, (call.__name__, kw)  # refused before the empty input returns
    for call in (update, step):
        for kw in (dict(out=None), dict(counts=None), dict(out=p)):  # out == the input centroids
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
    assert step(stats=None) == _lib.EINVAL


def test_header_and_binding_name_the_kmeans_entry_points(lib):
    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("n2v_kmeans_workspace_bytes", "n2v_kmeans_assign", "n2v_kmeans_update", "n2v_kmeans_step",
                 "n2v_kmeans_slab_rows"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code) and hasattr(lib, name)
    for name, value in (("EUCLIDEAN", 0), ("COSINE", 1)):
        assert re.search(r"#define\s+N2V_KMEANS_%s\s+%d\b" % (name, value), code)
        assert getattr(_lib, "KMEANS_" + name) == value
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15


def test_kmeans_and_init_centroids_check_their_arguments_before_the_gpu():
    """on a host tensor: the message names the bad argument, so it was found before the device check"""
    from node2vec_amd import cluster

    X = torch.zeros((10, 8))
    for call in (cluster.kmeans, cluster.init_centroids):
        with pytest.raises(ValueError, match="metric"):
            call(X, 3, metric="manhattan")
        with pytest.raises(ValueError, match="init"):
            call(X, 3, init="kmeans||")
        for k in (0, -1, 1025):
            with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
                call(X, k)
        with pytest.raises(ValueError, match="clusters of n = 10 rows"):
            call(X, 11)
        for bad in (torch.zeros((3, 7)), torch.zeros((2, 8)), torch.zeros(8)):
            with pytest.raises(ValueError, match="centroids must be"):
                call(X, 3, init=bad)
        with pytest.raises(ValueError, match="HIP device"):  # everything else was fine: no CPU path
            call(X, 3)
    with pytest.raises(ValueError, match="n_init"):
        cluster.kmeans(X, 3, n_init=0)
    with pytest.raises(ValueError, match="metric"):
        cluster.assign(X, torch.zeros((3, 8)), metric="l1")
    with pytest.raises(ValueError, match="centroids must be"):
        cluster.assign(X, torch.zeros((3, 9)))
    with pytest.raises(ValueError, match="HIP device"):
        cluster.assign(X, torch.zeros((3, 8)))
    with pytest.raises(ValueError, match="centroids must be"):
        cluster.update(X, torch.zeros(10, dtype=torch.int32), 3, "euclidean", torch.zeros((4, 8)))


def test_kmeans_pp_draw_is_a_pure_function_of_d_and_the_seed():
    from node2vec_amd import cluster

    D = torch.tensor([0.0, 3.0, 0.0, 1.0, 0.0, 4.0], dtype=torch.float32)
    draws = [[cluster.draw_next(D, rng, [0]) for _ in range(200)] for rng in
             (np.random.default_rng(5), np.random.default_rng(5))]
    assert draws[0] == draws[1]
    assert set(draws[0]) == {1, 3, 5}  # a row of D = 0 is never drawn
    rng = np.random.default_rng(5)
    want = [int(np.searchsorted(np.cumsum(D.double().numpy()), rng.random() * 8.0, side="right")) for _ in range(200)]
    assert draws[0] == want
    zero = torch.zeros(5)
    rng = np.random.default_rng(1)
    state = rng.bit_generator.state
    assert cluster.draw_next(zero, rng, [0, 1, 3]) == 2  # total 0: the lowest unchosen row, no random number
    assert rng.bit_generator.state == state


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_plugin_classes_refuse_cluster_before_fit_and_check_names_and_k_first():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    wv = KeyedVectors(np.array([0, 1, 2, 3, 4]), np.ones((5, 4), np.float32))
    names = pd.DataFrame({"id": [0, 1, 2, 3], "name": list("abcd")})
    for cls, model in ((Node2VecHIP, HipW2V(wv, np.zeros((5, 4), np.float32), {}, 0)),
                       (Node2VecSpark, HsW2VModel(wv, np.zeros((4, 4), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {}, name_id=names)
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.cluster(2)
        n2v.model = model
        with pytest.raises(KeyError):  # vertex 4 has no name
            n2v.cluster(2)
        n2v.name_id = None
        with pytest.raises(ValueError, match="metric"):
            n2v.cluster(2, metric="l2")
        with pytest.raises(ValueError, match="clusters of n = 5 rows"):
            n2v.cluster(6)
        with pytest.raises(ValueError, match="clusters of n = 3 rows"):
            n2v.cluster(4, restrict_vocab=3)
        assert n2v.clusters is None
