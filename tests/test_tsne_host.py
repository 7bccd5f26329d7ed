"""The host side of t-SNE (csrc/n2v_tsne.hip, node2vec_amd.tsne): the float64 definitions against each other, the
CPU restatement against them within bounds derived from the unit roundoff, the calibration and the symmetrisation
on CPU tensors, the argument checks that come back before anything is launched, and the reference optimiser on the
blobs of the GPU end-to-end test.  No GPU is needed."""
import ctypes

import numpy as np
import pytest
import torch

import tsne_cases as tc
from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return tc.build(tmp_path_factory.mktemp("tsne_cpu"))


def test_the_float64_gradient_is_the_gradient_of_the_float64_kl():
    """central differences at n = 12 with a random P: a step of 1e-5 in float64 leaves a truncation error of h^2
    (1e-10) times a third derivative of order one and a rounding error of 2^-53 / h = 1e-11, both relative to
    values of order 1e-2..1: below 1e-8, and the bound is 1e-6 of the largest gradient entry"""
    n, h = 12, 1e-5
    Pd = tc.random_symmetric_p(n, 1)
    Y = np.random.default_rng(2).standard_normal((n, 2))
    g = tc.gradient64(Pd, Y)
    num = np.zeros_like(g)
    for i in range(n):
        for c in range(2):
            up, dn = Y.copy(), Y.copy()
            up[i, c] += h
            dn[i, c] -= h
            num[i, c] = (tc.kl64(Pd, up) - tc.kl64(Pd, dn)) / (2 * h)
    rel = np.abs(num - g).max() / np.abs(g).max()
    print(f"central differences: relative error {rel:.3e}")
    assert rel <= 1e-6


@pytest.mark.parametrize("n,plan", [(1, None), (2, None), (300, None), (1500, None), (1500, (64, 128, 12)),
                                    (700, (256, 256, 3))])
def test_restatement_against_float64_with_the_derived_bounds(cpu, n, plan):
    """|restatement - float64| <= tsne_cases.repulse_bounds (the derivation is in pair_bound and repulse_bounds:
    gamma_(6 + tile) on zrow's terms, gamma_(14 + tile) on rep's, a factor 1 + 2^-40 for the fp64 folds), on points at
    least 0.5 apart, by the library-shaped plan and by plans of the test's own with many tiles and slabs"""
    Y = tc.lattice_points(n, 7 * n + 1)
    if n > 1:
        w, _ = tc.w64(Y)
        assert (1.0 / w[~np.eye(n, dtype=bool)] - 1.0).min() >= 0.25  # at least 0.5 apart
    plan = plan or tc.host_plan(n)
    assert plan[1] % plan[0] == 0 and plan[1] * plan[2] >= n
    rep, zrow = tc.repulse(cpu, Y, plan)
    Z = tc.z_of(cpu, zrow)
    rep64, zrow64, Z64 = tc.repulse64(Y)
    rb, zb, Zb = tc.repulse_bounds(Y, plan[0])
    assert (np.abs(rep - rep64) <= rb).all(), (np.abs(rep - rep64) / np.maximum(rb, 1e-300)).max()
    assert (np.abs(zrow - zrow64) <= zb).all(), (np.abs(zrow - zrow64) / np.maximum(zb, 1e-300)).max()
    assert abs(Z - Z64) <= Zb
    some = np.array([n - 1, 0, n // 2], np.int64)  # a row list gives the rows' own values
    rep_s, zrow_s = tc.repulse(cpu, Y, plan, rows=some)
    assert tc.same_bits(rep_s, rep[some]) and tc.same_bits(zrow_s, zrow[some])


def test_restatement_on_coincident_and_far_points(cpu):
    """exact values: two coincident points count 1 each in Z and nothing in the force; a point at 1e20 overflows d2,
    so w = 0 and it counts nowhere; j == i is skipped by index"""
    Y = np.array([[0.5, -1.0], [0.5, -1.0]], np.float32)
    rep, zrow = tc.repulse(cpu, Y, tc.host_plan(2))
    assert rep.tolist() == [[0.0, 0.0], [0.0, 0.0]] and zrow.tolist() == [1.0, 1.0] and tc.z_of(cpu, zrow) == 2.0
    Y = np.array([[0.0, 0.0], [1e20, 0.0], [0.0, 1.0]], np.float32)
    rep, zrow = tc.repulse(cpu, Y, tc.host_plan(3))
    assert zrow.tolist() == [0.5, 0.0, 0.5] and rep.tolist() == [[0.0, -0.25], [0.0, 0.0], [0.0, 0.25]]
    rep, zrow = tc.repulse(cpu, Y[:1], tc.host_plan(1))
    assert zrow.tolist() == [0.0] and rep.tolist() == [[0.0, 0.0]]


def test_restated_step_against_the_float64_gradient(cpu):
    """the restated step's gradient within tsne_cases.gradient_bound of the float64 definition, exaggeration 1 and 12,
    with rows of 0 to 200 entries"""
    n = 260
    Y = tc.lattice_points(n, 3)
    csr = tc.random_csr(n, [0, 1, 15, 16, 17, 33, 200], 4)
    Pd = tc.dense_of(csr, n)
    rep, zrow = tc.repulse(cpu, Y, tc.host_plan(n))
    Z = tc.z_of(cpu, zrow)
    for ex in (1.0, 12.0):
        _, grad, _, _ = tc.step(cpu, csr, Y, rep, Z, ex, 0.0, 0.0, 0.0, np.zeros_like(Y), np.ones_like(Y))
        err, bound = np.abs(grad - tc.gradient64(Pd, Y, ex)), tc.gradient_bound(Pd, Y, ex)
        assert (err <= bound).all(), (err / bound).max()


def test_calibrate_on_cpu_tensors():
    """rows with at least two distinct distances reach the perplexity: the stopping rule's 1e-5 in H is under 1.1e-5
    relative in exp(H), and 1e-4 is asked; a row of equal distances is uniform; rows sum to 1"""
    from node2vec_amd import tsne

    rng = np.random.default_rng(11)
    n, k = 200, 40
    d2 = rng.random((n, k)) * 2.0
    d2[3] = 0.7            # all equal: uniform
    d2[4, :] = 0.3
    d2[4, 5] = 0.2         # two distinct distances: one nearest entry, the rest equal
    d2[5] *= 1e-6          # needs a large beta
    d2[6] *= 1e3           # a small one
    for perplexity in (5.0, 12.5, 30.0):
        p = tsne.calibrate(torch.from_numpy(d2), perplexity)
        assert p.dtype == torch.float64 and tuple(p.shape) == (n, k)
        p = p.numpy()
        assert np.abs(p.sum(1) - 1.0).max() <= 1e-12
        got = tc.entropy_perplexity(p)
        distinct = np.array([len(np.unique(r)) >= 2 for r in d2])
        assert distinct.sum() == n - 1
        assert (np.abs(got[distinct] - perplexity) <= 1e-4 * perplexity).all(), np.abs(got - perplexity).max()
        assert np.array_equal(p[3], np.full(k, p[3, 0])) and abs(p[3, 0] - 1.0 / k) <= 1e-15
        want = tc.calibrate64(d2, perplexity)
        assert np.abs(p - want).max() <= 1e-12  # the same bisection, row by row
    absent = d2.copy()
    absent[:, -3:] = np.inf  # absent entries: p = 0, the rest calibrated
    p = tsne.calibrate(torch.from_numpy(absent), 10.0).numpy()
    assert (p[:, -3:] == 0).all() and np.abs(p.sum(1) - 1.0).max() <= 1e-12
    rows = np.arange(n) != 3
    assert (np.abs(tc.entropy_perplexity(p)[rows] - 10.0) <= 1e-3).all()


def test_symmetrisation_against_the_dense_definition():
    from node2vec_amd import tsne

    n, k = 50, 7
    rng = np.random.default_rng(12)
    idx = np.stack([rng.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)])
    p_cond = rng.random((n, k))
    p_cond /= p_cond.sum(1, keepdims=True)
    rowptr, col, val = tsne.symmetrise(torch.from_numpy(idx), torch.from_numpy(p_cond), n)
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    rowptr, col, val = rowptr.numpy(), col.numpy(), val.numpy()
    want = tc.dense_affinities64(idx, p_cond, n)
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == int((want > 0).sum())
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and np.array_equal(c, np.nonzero(want[i])[0])  # the pattern, ascending
        assert np.array_equal(val[rowptr[i]:rowptr[i + 1]], want[i, c].astype(np.float32))  # one fp32 rounding
    assert abs(float(val.astype(np.float64).sum()) - 1.0) <= len(col) * 2.0 ** -24
    # an index of -1 is an absent entry
    idx2 = idx.copy()
    idx2[:, 0] = -1
    r2, c2, v2 = tsne.symmetrise(torch.from_numpy(idx2), torch.from_numpy(p_cond), n)
    p2 = p_cond.copy()
    p2[:, 0] = 0.0
    idx3 = idx.copy()
    want2 = tc.dense_affinities64(idx3, p2, n)
    assert int(r2[-1]) == int((want2 > 0).sum())
    assert np.array_equal(tc.dense_of((r2.numpy(), c2.numpy(), v2.numpy()), n), want2.astype(np.float32).astype(np.float64))


def test_entry_points_validate_their_arguments(lib):
    """argument errors come back as N2V_EINVAL (-1) before anything is launched (no GPU needed); n == 0 is N2V_OK"""
    n = 100
    need = lib.n2v_tsne_workspace_bytes(n)
    assert need > 0 and lib.n2v_tsne_workspace_bytes(0) == 0
    assert lib.n2v_tsne_workspace_bytes(-1) == -1 and lib.n2v_tsne_workspace_bytes(2 ** 31) == -1
    buf = (ctypes.c_char * (need + 4096))()
    p_ = (ctypes.addressof(buf) + 15) & ~15  # 16-byte aligned, never dereferenced
    q_ = p_ + 1024

    def repulse(**kw):
        a = dict(Y=p_, n=n, rep=p_, zrow=p_, Z=p_, ws=p_, bytes=need)
        a.update(kw)
        return lib.n2v_tsne_repulse(a["Y"], a["n"], a["rep"], a["zrow"], a["Z"], a["ws"], a["bytes"], None)

    def step(**kw):
        a = dict(rowptr=p_, col=p_, val=p_, nnz=10, Y=p_, rep=p_, Z=p_, n=n, vel=p_, gain=p_, Y_next=q_, grad=p_)
        a.update(kw)
        return lib.n2v_tsne_step(a["rowptr"], a["col"], a["val"], a["nnz"], a["Y"], a["rep"], a["Z"], a["n"], 1.0,
                                 0.0, 0.5, 0.01, a["vel"], a["gain"], a["Y_next"], a["grad"], None)

    for name in ("Y", "rep", "zrow", "Z", "ws"):
        assert repulse(**{name: 0}) == -1, name
    assert repulse(ws=p_ + 8) == -1 and repulse(ws=p_ + 4) == -1  # not 16-byte aligned
    assert repulse(bytes=need - 1) == -1 and repulse(bytes=0) == -1
    assert repulse(n=-1) == -1 and repulse(n=2 ** 31) == -1
    assert repulse(n=0) == 0 and repulse(n=0, Y=0, rep=0, zrow=0, Z=0, ws=0, bytes=0) == 0
    for name in ("rowptr", "col", "val", "Y", "rep", "Z", "vel", "gain", "Y_next", "grad"):
        assert step(**{name: 0}) == -1, name
    assert step(Y_next=p_) == -1  # Y == Y_next
    assert step(n=-1) == -1 and step(n=2 ** 31) == -1 and step(nnz=-1) == -1
    assert step(n=0) == 0 and step(n=0, rowptr=0, Y=0, Y_next=0) == 0


@pytest.mark.parametrize("n", [1, 1000, 10 ** 5, 2 ** 31 - 1])
def test_the_plan_covers_the_range(lib, n):
    tile, slab, slabs = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
    assert lib.n2v_tsne_plan(n, ctypes.byref(tile), ctypes.byref(slab), ctypes.byref(slabs)) == 0
    assert tile.value == tc.TILE and slab.value % tile.value == 0 and slabs.value >= 1
    assert slabs.value * slab.value >= n and (slabs.value - 1) * slab.value < n
    assert (tile.value, slab.value, slabs.value) == tc.host_plan(n)
    assert lib.n2v_tsne_workspace_bytes(n) >= slabs.value * n * 24
    assert lib.n2v_tsne_plan(-1, ctypes.byref(tile), ctypes.byref(slab), ctypes.byref(slabs)) == -1
    assert lib.n2v_tsne_plan(2 ** 31, ctypes.byref(tile), ctypes.byref(slab), ctypes.byref(slabs)) == -1


def test_fit_checks_its_inputs_before_any_gpu_call(monkeypatch):
    from node2vec_amd import _lib, tsne

    def no_gpu(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    X = torch.zeros((40, 4))
    for bad in (X.numpy(), torch.zeros(4), None):
        with pytest.raises(ValueError):
            tsne.fit(bad)
    for perplexity in (0.5, 39.0, 100.0):
        with pytest.raises(ValueError, match="perplexity"):
            tsne.affinities(X, perplexity)
        with pytest.raises(ValueError, match="perplexity"):
            tsne.fit(X, perplexity=perplexity)
    with pytest.raises(ValueError, match="neighbours="):
        tsne.affinities(X, 5.0, metric="euclidean")
    assert tsne.default_k(40, 5.0) == 15 and tsne.default_k(40, 30.0) == 39


def test_the_reference_optimiser_separates_the_blobs():
    """the float64 numpy optimiser, on the case and the schedule of the GPU end-to-end test, leaves no point whose
    nearest neighbour in the plane carries another label: the condition under which that test's cap of 3 in 300
    means something.  tsne_cases.BLOB_SEPARATION is the separation at which this holds."""
    X, labels = tc.blobs()
    Pd = tc.blob_affinities64(X, 10.0)
    assert abs(Pd.sum() - 1.0) <= 1e-12
    Y0 = tc.pca_init64(X)
    Y = tc.optimise64(Pd, Y0, 300, 100)
    assert np.isfinite(Y).all() and tc.kl64(Pd, Y) < tc.kl64(Pd, Y0)
    assert tc.foreign_nearest(Y, labels) == 0
