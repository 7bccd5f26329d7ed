"""The host side of principal components (csrc/n2v_pca.hip, node2vec_amd.pca): the size entry points, the argument
checks that come back before anything is launched, the CPU restatement against float64 with a derived bound, the
input checks of pca.fit / pca.transform and the sign rule.  No GPU is needed."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import pca_cases as pc
from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

NS = [0, 1, 63, 64, 65, 131072, 131073, 2 ** 31 - 1, 2 ** 31, -1]
DIMS = [0, 1, 16, 17, 128, 129, 1024, 1025, -1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return pc.build(tmp_path_factory.mktemp("pca_cpu"))


def test_size_entry_points(lib, cpu):
    for n, dim in itertools.product(NS, DIMS):
        slab, need = lib.n2v_pca_slab_rows(n, dim), lib.n2v_pca_workspace_bytes(n, dim)
        if not (1 <= dim <= 1024 and 0 <= n < 2 ** 31):
            assert slab == -1 and need == -1, (n, dim)
            continue
        assert slab > 0 and slab % 64 == 0 and (n + slab - 1) // slab <= 2048, (n, dim, slab)
        assert slab == pc.slab_rows(cpu, n, dim), (n, dim)
        dp = (dim + 15) // 16 * 16
        assert (n + slab - 1) // slab * dp * dp * 4 <= 512 << 20, (n, dim)  # the partials stay under the cap
        assert (need == 0) if n == 0 else (need >= (n + slab - 1) // slab * (dp * dp * 4 + dim * 8 + 8)), (n, dim)


def test_entry_points_validate_their_arguments(lib):
    """argument errors come back as N2V_EINVAL (-1) before anything is launched (no GPU needed); n == 0 is N2V_OK"""
    n, dim = 100, 20
    need = lib.n2v_pca_workspace_bytes(n, dim)
    buf = (ctypes.c_char * (need + 64))()
    p_ = (ctypes.addressof(buf) + 15) & ~15  # 16-byte aligned, never dereferenced

    def mean(**kw):
        a = dict(X=p_, inv=0, n=n, dim=dim, mean=p_, used=p_, ws=p_, bytes=need)
        a.update(kw)
        return lib.n2v_pca_mean(a["X"], a["inv"], a["n"], a["dim"], a["mean"], a["used"], a["ws"], a["bytes"], None)

    def scatter(**kw):
        a = dict(X=p_, inv=0, n=n, dim=dim, center=0, S=p_, used=p_, ws=p_, bytes=need)
        a.update(kw)
        return lib.n2v_pca_scatter(a["X"], a["inv"], a["n"], a["dim"], a["center"], a["S"], a["used"], a["ws"],
                                   a["bytes"], None)

    for call in (mean, scatter):
        assert call(X=0) == -1 and call(used=0) == -1 and call(ws=0) == -1
        assert call(ws=p_ + 4) == -1 and call(ws=p_ + 8) == -1  # not 16-byte aligned
        assert call(bytes=need - 1) == -1 and call(bytes=0) == -1
        assert call(n=-1) == -1 and call(n=2 ** 31) == -1 and call(dim=0) == -1 and call(dim=1025) == -1
        assert call(n=0) == 0 and call(n=0, X=0, ws=0, used=0, bytes=0) == 0  # nothing to do
        assert call(n=0, dim=0) == -1  # (refused before the empty matrix returns)
    assert mean(mean=0) == -1 and scatter(S=0) == -1


@pytest.mark.parametrize("n,dim,unit,centered", [(81, 20, False, True), (300, 17, True, True), (1000, 8, False, False),
                                                 (200, 130, True, True), (64, 1, False, True)])
def test_restatement_against_float64_with_the_derived_bound(cpu, n, dim, unit, centered):
    """|S_cpu - S64| <= (slab_rows + 4) 2^-24 sum_r |xc_a| |xc_b| for every element (pca_cases.element_bound says
    where the terms come from), S64 and the sum in float64 around the same fp32 centre"""
    X, inv = pc.normal_case(n, dim, 11 * n + dim, with_norms=unit)
    m, S, used = pc.moments(cpu, X, inv, centered)
    assert used == n
    S64, A = pc.ref_scatter(X, inv, m.astype(np.float32) if centered else None)
    err, bound = np.abs(S - S64), pc.element_bound(A, pc.slab_rows(cpu, n, dim))
    assert (err <= bound).all(), (err / bound).max()
    assert np.array_equal(S, S.T)


def test_restatement_mean_is_the_float64_mean(cpu):
    """positive data, so that `relative` has one meaning: |mean - sum(float64) / n| <= n 2^-53 |mean|"""
    rng = np.random.default_rng(3)
    for n, dim in ((81, 20), (5000, 7), (129, 130)):
        X = rng.random((n, dim)).astype(np.float32) + np.float32(0.25)
        m, used = pc.mean(cpu, X)
        want = X.sum(0, dtype=np.float64) / n
        assert used == n and (np.abs(m - want) <= n * 2.0 ** -53 * np.abs(want)).all()


def test_restatement_skips_rows_and_counts_them(cpu):
    X, inv = pc.normal_case(200, 6, 2, with_norms=True)
    X[0, 1], X[63, 0], X[64, 5], X[199, 2] = np.nan, np.inf, -np.inf, np.nan
    inv[10] = np.inf  # a finite row whose scaled values are not
    keep = np.ones(200, bool)
    keep[[0, 63, 64, 199]] = False
    m, S, used = pc.moments(cpu, X, None)
    assert used == 196 and np.isfinite(S).all() and np.isfinite(m).all()
    S64, A = pc.ref_scatter(X[keep], None, m.astype(np.float32))
    assert (np.abs(S - S64) <= pc.element_bound(A, 64)).all()
    assert pc.moments(cpu, X, inv)[2] == 195
    m, used = pc.mean(cpu, np.full((3, 2), np.nan, np.float32))  # no used row: zeros
    assert used == 0 and m.tolist() == [0.0, 0.0]


def test_fit_and_transform_check_their_inputs_before_any_gpu_call(monkeypatch):
    from node2vec_amd import _lib, pca

    def no_gpu(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    X = torch.zeros((10, 4))
    for bad in (X, X.double(), X.numpy(), torch.zeros(4), None):
        with pytest.raises(ValueError):
            pca.fit(bad)
        with pytest.raises(ValueError):
            pca.moments(bad)
    for k in (0, 5, -1):
        with pytest.raises(ValueError, match="n_components"):
            pca.fit(X, k)
    with pytest.raises(ValueError, match="inv_norm"):
        pca.fit(X, 2, unit=True, inv_norm=torch.ones(9))
    with pytest.raises(ValueError, match="inv_norm"):
        pca.fit(X, 2, unit=True, inv_norm=torch.ones((10, 1)))
    res = pca.PCAResult(torch.eye(4)[:2], torch.zeros(4), torch.ones(2, dtype=torch.float64),
                        torch.ones(2, dtype=torch.float64) / 2, torch.ones(2, dtype=torch.float64), 2.0, 10, False,
                        False)
    for bad in (X, X.double(), torch.zeros((10, 5)), None):
        with pytest.raises(ValueError):
            pca.transform(bad, res)
    with pytest.raises(ValueError):
        pca.transform(X, "not a result")
    with pytest.raises(ValueError, match="inv_norm"):
        pca.transform(X, res._replace(unit=True), inv_norm=torch.ones(3))


def test_projection_of_a_result():
    """W = components, b = -float32(mean . V in float64); whiten scales both by 1 / sqrt(lambda), 0 for lambda = 0"""
    from node2vec_amd import pca

    V = torch.tensor([[0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    mean = torch.tensor([1.0, 2.0, 3.0])
    lam = torch.tensor([4.0, 0.0], dtype=torch.float64)
    res = pca.PCAResult(V, mean, lam, lam / 4, lam.sqrt(), 4.0, 10, False, False)
    W, b = pca.projection(res)
    want_b = np.float32(-(np.float64(np.float32(0.6)) * 1.0 + np.float64(np.float32(0.8)) * 2.0))
    assert torch.equal(W, V) and b.tolist() == [float(want_b), -3.0]
    W, b = pca.projection(res._replace(whiten=True))
    assert torch.equal(W, torch.stack([V[0].double() * 0.5, V[1].double() * 0.0]).float())
    assert b.tolist() == [float(np.float32(np.float64(want_b) * 0.5)), 0.0]


def test_the_sign_rule():
    from node2vec_amd import pca

    V = np.array([[0.1, -0.9, 0.4],      # the largest entry is negative: flipped
                  [0.2, 0.3, -0.1],      # positive: kept
                  [-0.6, 0.6, 0.5],      # a tie: the LOWEST index decides, and it is negative: flipped
                  [0.6, -0.6, 0.5],      # a tie whose lowest index is positive: kept
                  [0.0, 0.0, 0.0]])
    got = pca.fix_signs(V)
    assert np.array_equal(got, np.array([[-0.1, 0.9, -0.4], [0.2, 0.3, -0.1], [0.6, -0.6, -0.5], [0.6, -0.6, 0.5],
                                         [0.0, 0.0, 0.0]]))
    assert np.array_equal(V[0], [0.1, -0.9, 0.4])  # the argument is not changed
