"""The host side of UMAP (csrc/n2v_umap.hip, node2vec_amd.umap): the curve fit, the smoothing and the fuzzy union on
CPU tensors against their definitions, the CPU restatement of x^b and of one epoch against float64, the argument
checks that come back before anything is launched, and the restated loop on the blobs of the GPU end-to-end test.
No GPU is needed."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import umap_cases as uc
from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

# Measured here, on the CPU, over the sweeps and cases below (the figures are in DESIGN.md "UMAP"); each test asserts
# four times its figure, the margin being for arguments the sweeps do not hit.
POWB_MEASURED = 1.0e-7    # largest relative error of the restated x^b against float64 pow: 9.99e-8, at b = 1.3
EPOCH_MEASURED = 9.2e-5   # largest coordinate difference of one restated epoch against float64: 9.12e-5
EPOCH_ALPHA = 0.25


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return uc.build(tmp_path_factory.mktemp("umap_cpu"))


def _curve(x, a, b):
    return 1.0 / (1.0 + a * x ** (2.0 * b))


def test_find_ab_is_umap_learns_fit():
    from node2vec_amd import umap

    a, b = umap.find_ab(1.0, 0.1)
    print(f"find_ab(1.0, 0.1) = ({a:.6f}, {b:.6f})")
    assert abs(a - uc.AB[0]) <= 1e-3 and abs(b - uc.AB[1]) <= 1e-3
    for spread, min_dist in ((1.0, 0.1), (1.0, 0.5), (2.0, 0.25), (0.5, 0.0)):
        a, b = umap.find_ab(spread, min_dist)
        x = np.linspace(0.0, 3.0 * spread, 300)
        target = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
        fitted = ((_curve(x, a, b) - target) ** 2).sum()
        assert a > 0 and b > 0 and fitted < ((_curve(x, 1.0, 1.0) - target) ** 2).sum()
    for bad in ((0.0, 0.1), (1.0, -0.1), (1.0, 3.0)):
        with pytest.raises(ValueError):
            umap.find_ab(*bad)


def _membership_sums(dist, rho, sigma):
    return np.exp(-np.maximum(0.0, dist - rho[:, None]) / sigma[:, None]).sum(1)


def test_smooth_knn_reaches_log2_k():
    """Every row whose target can be reached -- fewer than log2(k) entries at or below rho -- sums to log2(k) within
    the stopping rule's 1e-5: random rows, rows with repeated distances, rows with zero distances, rows on very
    different scales.  A row of equal distances sums to k whatever sigma is: its sigma is the floor, not a division
    by zero."""
    from node2vec_amd import umap

    rng = np.random.default_rng(3)
    n, k = 120, 15
    dist = np.sort(rng.random((n, k)), axis=1)
    dist[1, 4:9] = dist[1, 4]          # repeated distances
    dist[2, :2] = 0.0                  # two zeros (exact duplicates of the point): rho is the third
    dist[3] = np.sort(np.repeat(dist[3, :5], 3))  # every distance three times: 3 entries at rho, log2(15) = 3.9
    dist[4] *= 1e-6
    dist[5] *= 1e4
    dist[6] = 0.37                     # all equal
    dist[7] = 0.0                      # all zero: rho = 0
    rho, sigma = umap.smooth_knn(torch.from_numpy(dist), k)
    assert rho.dtype == sigma.dtype == torch.float64 and tuple(rho.shape) == tuple(sigma.shape) == (n,)
    rho, sigma = rho.numpy(), sigma.numpy()
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    positive = np.where(dist > 0, dist, np.inf).min(1)
    assert np.array_equal(rho, np.where(np.isfinite(positive), positive, 0.0))
    assert rho[2] == dist[2, 2] and rho[7] == 0.0
    reachable = np.ones(n, bool)
    reachable[[6, 7]] = False
    err = np.abs(_membership_sums(dist, rho, sigma) - np.log2(k))
    print(f"largest |sum - log2(k)| over the reachable rows: {err[reachable].max():.3e}")
    assert (err[reachable] <= 1e-5).all()
    assert sigma[6] == pytest.approx(1e-3 * 0.37, rel=1e-12) and _membership_sums(dist, rho, sigma)[6] == k
    assert sigma[7] == pytest.approx(1e-3 * dist.mean(), rel=1e-12)
    # a non-finite distance is an absent entry
    absent = dist.copy()
    absent[:, -3:] = np.inf
    rho2, sigma2 = (t.numpy() for t in umap.smooth_knn(torch.from_numpy(absent), k))
    rows = np.arange(n) >= 8
    assert (np.abs(_membership_sums(absent[:, :-3], rho2, sigma2)[rows] - np.log2(k)) <= 1e-5).all()


def test_fuzzy_graph_from_the_callers_neighbours_is_the_dense_union():
    from node2vec_amd import umap

    n, k = 60, 7
    rng = np.random.default_rng(4)
    idx = np.stack([rng.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)])
    dist = np.sort(rng.random((n, k)), axis=1)
    g = umap.fuzzy_graph(None, neighbours=(torch.from_numpy(idx), torch.from_numpy(dist)))
    assert g.n_neighbors == k and g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32
    assert g.val.dtype == torch.float32
    rho, sigma = (t.numpy() for t in umap.smooth_knn(torch.from_numpy(dist), k))
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), k), idx.reshape(-1)] = np.exp(-np.maximum(0.0, dist - rho[:, None]) /
                                                            sigma[:, None]).reshape(-1)
    want = (A + A.T) - A * A.T
    rowptr, col, val = g.rowptr.numpy(), g.col.numpy(), g.val.numpy()
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == int((want > 0).sum())
    dense = np.zeros((n, n), np.float32)
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and np.array_equal(c, np.nonzero(want[i])[0])  # the pattern, ascending
        dense[i, c] = val[rowptr[i]:rowptr[i + 1]]
    assert np.array_equal(dense, want.astype(np.float32))  # one fp32 rounding
    assert np.array_equal(dense, dense.T) and (dense.diagonal() == 0).all() and dense.max() == 1.0
    # an index of -1, or a row's own, is an absent entry
    idx2 = idx.copy()
    idx2[:, -1] = -1
    idx2[::2, -2] = np.arange(n)[::2]
    g2 = umap.fuzzy_graph(None, neighbours=(torch.from_numpy(idx2), torch.from_numpy(dist)))
    cols2 = [set(g2.col.numpy()[g2.rowptr[i]:g2.rowptr[i + 1]].tolist()) for i in range(n)]
    assert all(i not in cols2[i] for i in range(n))
    kept = [set(idx2[i][(idx2[i] >= 0) & (idx2[i] != i)].tolist()) for i in range(n)]
    assert all(cols2[i] == kept[i] | {j for j in range(n) if i in kept[j]} for i in range(n))
    eps = umap.epochs_per_sample(g.val)
    assert eps.dtype == torch.float32 and float(eps.min()) == 1.0
    assert torch.equal(eps, g.val.max() / g.val)
    assert umap.epochs_per_sample(torch.tensor([0.5, 0.0, 0.25])).tolist() == [1.0, float("inf"), 2.0]


def test_restated_powb_against_float64_pow(cpu):
    """d2 from 2^-40 to 2^40, 64 per octave and 20 000 random, b in {0.5, 0.7, 0.8951, 1.3}: the largest relative error
    measured is 9.99e-8 (POWB_MEASURED); four times that is asserted"""
    x = uc.powb_sweep()
    assert x.min() == np.float32(2.0 ** -40) and x.max() == np.float32(2.0 ** 40)
    worst = 0.0
    for b in uc.BS:
        got = uc.powb(cpu, x, b).astype(np.float64)
        want = x.astype(np.float64) ** float(np.float32(b))
        rel = float(np.abs(got / want - 1.0).max())
        print(f"b = {b}: largest relative error {rel:.3e}")
        worst = max(worst, rel)
    print(f"powb: largest relative error {worst:.3e}")
    assert worst <= 4.0 * POWB_MEASURED
    # the ends: what is not positive gives 0, 1 gives 1, b == 1 gives x itself, overflow and underflow saturate
    e = uc.powb_edges()
    for b in (0.5, 1.0, 1.3):
        got = uc.powb(cpu, e, b)
        assert (got[~(e > 0)] == 0).all() and (got[e == 1.0] == 1.0).all()
        if b == 1.0:
            assert uc.same_bits(got[e > 0], e[e > 0])
        fin = (e > 0) & np.isfinite(e)
        want = e[fin].astype(np.float64) ** float(np.float32(b))
        normal = (want >= 2.0 ** -126) & (want < 2.0 ** 128)
        assert np.abs(got[fin][normal] / want[normal] - 1.0).max() <= 4.0 * POWB_MEASURED
        assert (got[fin][want >= 2.0 ** 129] == np.inf).all() and (got[fin][want < 2.0 ** -151] == 0).all()
        assert (got[e == np.inf] == np.inf).all()


CASE_NS = (1, 2, 63, 257, 1000)
PARAMS = tuple(itertools.product((0, 1, 5), ((1.0, 1.0), uc.AB), (0, 7)))  # negative, (a, b), epoch


def test_one_restated_epoch_against_float64(cpu):
    """The graph and parameter cases of the GPU test at alpha = 0.25, against the same law with the same draws in
    float64 numpy with float64 pow.  The largest coordinate difference measured is 9.12e-5 (EPOCH_MEASURED; the
    median row differs by 3e-7: next to a coincident point the repulsion's slope is 2 gamma b / 0.001 per unit, so
    a rounding there grows by hundreds per step along a chain of up to 300 entries); four times that is asserted."""
    worst, met_all = 0.0, dict(self_draws=0, coincident_neighbours=0, coincident_negatives=0, fired=0)
    for n in CASE_NS:
        csr, Y = uc.graph_case(n, 100 + n)
        for negative, (a, b), e in PARAMS:
            got, hits = uc.epoch(cpu, csr, Y, e, a, b, 1.0, EPOCH_ALPHA, negative, 3)
            want, met = uc.epoch64(csr, Y, e, a, b, 1.0, EPOCH_ALPHA, negative, 3)
            assert hits == met["self_draws"]
            worst = max(worst, float(np.abs(got - want).max()))
            for key in met_all:
                met_all[key] += met[key]
        print(f"n = {n}: largest coordinate difference so far {worst:.3e}")
    print(f"epoch: largest coordinate difference {worst:.3e}; met {met_all}")
    assert all(v > 0 for v in met_all.values()), met_all  # the cases meet what they were built to meet
    assert worst <= 4.0 * EPOCH_MEASURED


def test_restated_epoch_exact_values(cpu):
    """what can be said exactly: a row without a firing entry copies; entries that never fire and columns out of range
    move nothing; eps = 2 fires in the odd epochs only; a draw that hits the row itself is skipped (n = 1: all of
    them); a coincident negative moves both coordinates by 4 alpha"""
    Y = np.array([[1.0, 2.0], [4.0, 6.0], [4.0, 6.0]], np.float32)
    rowptr = np.array([0, 6, 6, 6], np.int64)
    col = np.array([1, 1, 1, 1, -1, 3], np.int32)
    dead = (rowptr, col, np.array([0.5, np.inf, np.nan, -1.0, 1.0, 1.0], np.float32))
    for e in (0, 7):
        got, _ = uc.epoch(cpu, dead, Y, e, 1.0, 1.0, 1.0, 1.0, 5, 0)
        assert uc.same_bits(got, Y)
    two = (np.array([0, 1, 1, 1], np.int64), np.array([1], np.int32), np.array([2.0], np.float32))
    moved = [not uc.same_bits(uc.epoch(cpu, two, Y, e, 1.0, 1.0, 1.0, 1.0, 0, 0)[0], Y) for e in range(6)]
    assert moved == [False, True, False, True, False, True]
    got, _ = uc.epoch(cpu, two, Y, 1, 1.0, 1.0, 1.0, 0.5, 0, 0)
    # d = (-3, -4), d2 = 25, c = -2 / 26: both attractions stay inside the clamp
    y = Y[0].astype(np.float64)
    for _ in range(2):
        d = y - Y[1]
        y = y + 0.5 * (-2.0 / (1.0 + d @ d)) * d
    assert np.abs(got[0] - y).max() <= 1e-6 and uc.same_bits(got[1:], Y[1:])
    one = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([1.0], np.float32))
    got, hits = uc.epoch(cpu, one, Y[:1], 0, *uc.AB, 1.0, 1.0, 5, 9)
    assert hits == 5 and uc.same_bits(got, Y[:1])
    # rows 1 and 2 coincide; row 1's neighbour is row 2: no attraction, and every draw of 2 is a coincident negative
    pair = (np.array([0, 0, 1, 1], np.int64), np.array([2], np.int32), np.array([1.0], np.float32))
    ks = uc.draws(5, 0, np.array([0]), 5, 3)[0]
    got, hits = uc.epoch(cpu, pair, Y, 0, 1.0, 1.0, 0.0, 0.125, 5, 5)
    assert hits == int((ks == 1).sum())
    first = list(ks).index(2) if 2 in ks else None
    if first is not None and 0 not in ks[:first]:  # gamma = 0: point 0 moves nothing; then y has left the spot
        assert got[1].tolist() == [4.5, 6.5]


def test_entry_points_validate_their_arguments(lib):
    """argument errors come back as N2V_EINVAL (-1) before anything is launched (no GPU needed); n == 0 is N2V_OK"""
    buf = (ctypes.c_char * 8192)()
    p_ = (ctypes.addressof(buf) + 15) & ~15  # aligned, never dereferenced
    q_ = p_ + 1024

    def epoch(**kw):
        v = dict(rowptr=p_, col=p_, eps=p_, nnz=10, Y=p_, Y_next=q_, n=100, epoch=0, a=1.5, b=0.9, gamma=1.0,
                 alpha=1.0, negative=5, seed=1, max_blocks=0)
        v.update(kw)
        return lib.n2v_umap_epoch(v["rowptr"], v["col"], v["eps"], v["nnz"], v["Y"], v["Y_next"], v["n"], v["epoch"],
                                  v["a"], v["b"], v["gamma"], v["alpha"], v["negative"], v["seed"], v["max_blocks"],
                                  None)

    for name in ("rowptr", "col", "eps", "Y", "Y_next"):
        assert epoch(**{name: 0}) == -1, name
    assert epoch(Y_next=p_) == -1  # Y_next == Y
    assert epoch(Y=p_ + 4) == -1 and epoch(Y_next=q_ + 4) == -1  # float2 accesses
    assert epoch(n=-1) == -1 and epoch(n=2 ** 31) == -1 and epoch(nnz=-1) == -1
    assert epoch(negative=-1) == -1 and epoch(negative=65) == -1
    assert epoch(epoch=-1) == -1 and epoch(epoch=2 ** 31 - 1) == -1 and epoch(max_blocks=-1) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert epoch(a=bad) == -1 and epoch(b=bad) == -1, bad
    for bad in (float("inf"), float("nan")):
        assert epoch(gamma=bad) == -1 and epoch(alpha=bad) == -1
    assert epoch(n=0) == 0 and epoch(n=0, rowptr=0, col=0, eps=0, Y=0, Y_next=0, nnz=0) == 0
    assert epoch(n=0, a=0.0) == -1  # (refused before the empty layout returns)

    def powb(x=p_, n=10, b=0.9, out=q_):
        return lib.n2v_umap_powb(x, n, b, out, None)

    assert powb(x=0) == -1 and powb(out=0) == -1 and powb(n=-1) == -1 and powb(n=2 ** 40) == -1
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert powb(b=bad) == -1
    assert powb(n=0) == 0 and powb(n=0, x=0, out=0) == 0


def test_fit_checks_its_inputs_before_any_gpu_call(monkeypatch):
    from node2vec_amd import _lib, umap

    def no_gpu(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    X = torch.zeros((40, 4))
    for bad in (X.numpy(), torch.zeros(4), None):
        with pytest.raises(ValueError):
            umap.fit(bad)
    for k in (1, 40, 100):
        with pytest.raises(ValueError, match="n_neighbors"):
            umap.fit(X, n_neighbors=k)
    with pytest.raises(ValueError, match="negative_sample_rate"):
        umap.fit(X, negative_sample_rate=65)
    with pytest.raises(ValueError, match="both a and b"):
        umap.fit(X, a=1.0)
    with pytest.raises(ValueError, match="finite and positive"):
        umap.fit(X, a=1.0, b=0.0)
    with pytest.raises(ValueError, match="init"):
        umap.fit(X, init="spectral")
    assert umap.default_epochs(10000) == 500 and umap.default_epochs(10001) == 200
    assert umap.alpha_of(0, 200) == 1.0 and umap.alpha_of(50, 200, 2.0) == 1.5


def blob_graph():
    """the fuzzy graph of the blobs from float64 numpy neighbours, on CPU tensors -> (X, labels, csr with eps)"""
    from node2vec_amd import umap

    X, labels = uc.blobs(separation=uc.BLOB_SEPARATION)
    idx, dist = uc.blob_neighbours(X)
    g = umap.fuzzy_graph(None, neighbours=(torch.from_numpy(idx), torch.from_numpy(dist)))
    return X, labels, (g.rowptr.numpy(), g.col.numpy(), umap.epochs_per_sample(g.val).numpy())


def test_the_restated_loop_separates_the_blobs(cpu):
    """three Gaussian blobs of 100 rows in 16-D at umap_cases.BLOB_SEPARATION, 200 epochs of the restated loop from
    the PCA layout with find_ab's curve: every point's nearest layout neighbour carries its own label -- the condition
    the GPU end-to-end test asks of the device"""
    from node2vec_amd import umap

    X, labels, csr = blob_graph()
    a, b = umap.find_ab()
    Y0 = uc.pca_init64(X)
    assert Y0.min() == 0.0 and Y0.max() == 10.0
    Y = uc.fit_loop(cpu, csr, Y0, 200, a, b)
    assert np.isfinite(Y).all() and not np.array_equal(Y, Y0)
    print(f"foreign nearest neighbours: {uc.foreign_nearest(Y, labels)} (from the PCA layout: "
          f"{uc.foreign_nearest(Y0, labels)})")
    assert uc.foreign_nearest(Y, labels) == 0
