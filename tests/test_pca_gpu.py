"""Principal components on the GPU (csrc/n2v_pca.hip through node2vec_amd.pca) against the CPU restatement,
tests/cpu_pca/n2v_pca_cpu.c, bit for bit: the float64 means and scatter matrix by their bit patterns.  The shapes sit
on the kernel's edges: both load paths (dim % 4, base alignment), the 16-column tile, the register-resident limit
(128), the first column of a second super-column (129), of its second half (193) and of a third (257), a ragged
wave, step and slab (n).  Then the fit end to end against numpy.linalg.eigh in float64 with derived bounds, and
the public surface."""
import numpy as np
import pandas as pd
import pytest
import torch

import pca_cases as pc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return pc.build(tmp_path_factory.mktemp("pca_cpu"))


def _device(a, aligned=True):
    """a float32 numpy array on the device; aligned=False: its base 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if aligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _check(cpu, X, inv=None, centered=True, aligned=True):
    """pca.moments on the device == the restatement, bit for bit; S symmetric to the bit"""
    from node2vec_amd import pca

    what = (X.shape, inv is not None, centered, aligned)
    mean, S, used = pca.moments(_device(X, aligned), centered, unit=inv is not None,
                                inv_norm=None if inv is None else torch.from_numpy(inv).cuda())
    mean, S = mean.cpu().numpy(), S.cpu().numpy()
    w_mean, w_S, w_used = pc.moments(cpu, X, inv, centered)
    assert used == w_used, what
    assert pc.same_bits(mean, w_mean), ("mean",) + what
    assert pc.same_bits(S, w_S), ("S",) + what + (np.abs(S - w_S).max(),)
    assert pc.same_bits(S, np.ascontiguousarray(S.T)), ("symmetry",) + what
    return mean, S, used


@pytest.mark.parametrize("dim", [1, 3, 4, 15, 16, 17, 64, 100, 128, 129, 144, 193, 256, 257, 272, 1000, 1024])
def test_bitwise_over_the_dimensions(cpu, dim):
    X, inv = pc.normal_case(81, dim, 31 * dim, with_norms=True)
    for centered in (True, False):
        for norms in (None, inv):
            for aligned in (True, False):
                _check(cpu, X, norms, centered, aligned)


def _three_slabs_and_a_tail(dim):
    from node2vec_amd import pca

    slab = pca.slab_rows(300, dim)  # read from the library
    n = 3 * slab + 37
    assert pca.slab_rows(n, dim) == slab and n // slab == 3 and n % slab
    return n, slab


def test_bitwise_over_the_row_counts(cpu):
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 255, 257, _three_slabs_and_a_tail(20)[0]):
        X, inv = pc.normal_case(n, 20, n, with_norms=True)
        _check(cpu, X)
        _check(cpu, X, inv, aligned=False)


def test_bitwise_on_slabs_longer_than_one_step_and_the_same_twice(cpu):
    from node2vec_amd import pca

    n, dim = 150001, 8
    assert pca.slab_rows(n, dim) > 64 and n // pca.slab_rows(n, dim) >= 3
    X, inv = pc.normal_case(n, dim, 3, with_norms=True)
    first = _check(cpu, X, inv)
    again = _check(cpu, X, inv)
    assert pc.same_bits(first[0], again[0]) and pc.same_bits(first[1], again[1])
    _check(cpu, X, None, aligned=False)


def test_skipped_rows_are_not_counted_and_leave_the_scatter_of_the_rest(cpu):
    """NaN, +inf and -inf in one column of rows at the first step, at a step edge and in the last slab: n_used drops
    by exactly those rows, and S is the scatter of the matrix without them, cut into slabs where the full matrix is"""
    from node2vec_amd import pca

    n, slab = _three_slabs_and_a_tail(20)
    X, _ = pc.normal_case(n, 20, 21)
    bad = [0, 63, 64, n - 2]
    X[0, 3], X[63, 3], X[64, 3], X[n - 2, 3] = np.nan, np.inf, -np.inf, np.nan
    for aligned in (True, False):
        mean, S, used = _check(cpu, X, aligned=aligned)
        assert used == n - 4 and np.isfinite(S).all() and np.isfinite(mean).all()
    Xd = _device(X)
    L, ws = pca._lib.load(), pca.alloc_workspace(n, 20, "cuda")
    out = torch.zeros(20 * 20 + 20, dtype=torch.float64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.n2v_pca_mean(Xd.data_ptr(), None, n, 20, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                          pca._lib.current_stream_ptr()) == 0
    assert L.n2v_pca_scatter(Xd.data_ptr(), None, n, 20, None, out[20:].data_ptr(), counts[1:].data_ptr(),
                             ws.data_ptr(), ws.numel(), pca._lib.current_stream_ptr()) == 0
    assert counts.tolist() == [n - 4, n - 4]  # both entry points
    keep = np.ones(n, bool)
    keep[bad] = False
    bounds = [int(keep[:min(s * slab, n)].sum()) for s in range(5)]
    centre = mean.astype(np.float32)
    want, w_used = pc.scatter(cpu, X[keep], None, centre, bounds=bounds)
    assert w_used == n - 4 and pc.same_bits(S, want)


def test_an_all_skipped_slab_contributes_nothing(cpu):
    n, slab = _three_slabs_and_a_tail(20)
    X, _ = pc.normal_case(n, 20, 22)
    X[slab:2 * slab, 7] = np.nan
    mean, S, used = _check(cpu, X)
    assert used == n - slab and np.isfinite(S).all()
    keep = np.r_[0:slab, 2 * slab:n]
    want, _ = pc.scatter(cpu, X[keep], None, mean.astype(np.float32), bounds=[0, slab, slab, 2 * slab, n - slab])
    assert pc.same_bits(S, want)


def test_signed_zeros_and_denormals(cpu):
    """uncentred, so that the values reach the products as they are: products that underflow to -0 (an accumulator
    of -0 that a padding row turns into +0), denormal factors and denormal sums"""
    rng = np.random.default_rng(5)
    tiny = np.float32(1e-40)
    for dim in (4, 5, 20):
        X = np.zeros((70, dim), np.float32)
        X[0, :2] = [1e-30, -1e-30]          # the product underflows to -0
        X[1] = -0.0
        X[2, :] = tiny                       # denormal factors
        X[3, :2] = [1e-20, -3e-20]           # a denormal product
        X[4:, :] = (rng.standard_normal((66, dim)) * 1e-19).astype(np.float32)  # sums among the denormals
        X[10, 1] = -0.0
        for aligned in (True, False):
            mean, S, used = _check(cpu, X[:1], centered=False, aligned=aligned)  # one row, 63 that pad the step
            assert used == 1 and S[0, 1] == 0.0 and not np.signbit(S[0, 1])
            _check(cpu, X[:5], centered=False, aligned=aligned)
            _check(cpu, X, centered=False, aligned=aligned)
            _check(cpu, X, centered=True, aligned=aligned)


def test_a_product_overflow_makes_fit_raise():
    from node2vec_amd import pca

    X = np.ones((50, 6), np.float32)
    X[::2, 2] = 3e30
    X[1::2, 2] = -3e30
    with pytest.raises(ValueError, match="non-finite"):
        pca.fit(_device(X), 2)
    X[:, 0] = np.nan
    with pytest.raises(ValueError, match="at least 2"):
        pca.fit(_device(X), 2)
    with pytest.raises(ValueError, match="n_components"):
        pca.fit(_device(pc.normal_case(3, 6, 1)[0]), 3)  # min(dim, n_used - 1) = 2


@pytest.fixture(scope="module")
def planted():
    """(X, the fit, the float64 eigenpairs of the float64 sample covariance, ||E||_F).  E = C_gpu - C64.  The scatter
    pass centres on c = float32(mean), the float64 covariance on the float64 mean m: S_c = S_m + n (m - c)(m - c)^T
    exactly, and |S_gpu - S_c| is under pca_cases.element_bound.  So |E_ab| <= ((slab_rows + 4) 2^-24 A_ab + n |m_a
    - c_a| |m_b - c_b|) / (n - 1), A in float64 around c."""
    from node2vec_amd import pca

    X = pc.planted()
    n, dim = X.shape
    res = pca.fit(_device(X), 3)
    X64 = X.astype(np.float64)
    lam64, vec64 = np.linalg.eigh(np.cov(X64.T))
    lam64, vec64 = lam64[::-1], vec64[:, ::-1].T
    c = res.mean.cpu().numpy()
    _, A = pc.ref_scatter(X, None, c)
    delta = np.abs(X64.mean(0) - c.astype(np.float64))
    E = (pc.element_bound(A, pca.slab_rows(n, dim)) + n * np.outer(delta, delta)) / (n - 1)
    return X, res, lam64, vec64, float(np.linalg.norm(E))


def test_planted_directions_against_float64_eigh(planted):
    X, res, lam64, vec64, e_norm = planted
    dim = X.shape[1]
    V = res.components.cpu().numpy().astype(np.float64)
    lam = res.explained_variance.numpy()
    assert res.n_used == 4000 and V.shape == (3, dim) and res.components.is_cuda
    assert np.allclose(np.sqrt(lam64[:3]), [3, 2, 1], rtol=0.1)  # the planted spectrum
    for j in range(3):
        gap = np.abs(np.delete(lam64, j) - lam64[j]).min()
        # the angle of the fitted direction; the rounding of the stored fp32 component changes its length, not
        # (to first order) its direction, so the cosine is taken of the normalised vector
        cos = abs(V[j] @ vec64[j]) / np.linalg.norm(V[j])
        print(f"component {j}: 1 - cos = {1 - cos:.3e} <= {(2 * e_norm / gap) ** 2:.3e}; "
              f"|lambda - lambda64| = {abs(lam[j] - lam64[j]):.3e} <= {e_norm:.3e}")
        assert 1.0 - cos <= (2 * e_norm / gap) ** 2  # Davis-Kahan
        assert abs(lam[j] - lam64[j]) <= e_norm        # Weyl
        at = np.argmax(np.abs(V[j]))
        assert V[j, at] > 0  # the sign rule
    assert np.abs(V @ V.T - np.eye(3)).max() <= dim * 2.0 ** -23
    assert res.total_variance == pytest.approx(lam64.sum(), rel=1e-5)
    assert np.allclose(res.explained_variance_ratio.numpy(), lam / res.total_variance, rtol=1e-12)
    assert np.allclose(res.singular_values.numpy(), np.sqrt(lam * 3999), rtol=1e-12)


@pytest.mark.parametrize("whiten", [False, True])
def test_transform_is_the_pinned_projection_with_the_fitted_variances(planted, whiten):
    """transform == classify.decision_function(X, W, b) bit for bit.  The column variances: with Z64 the float64
    projection by the same fp32 (W, b), var(Z64_j) = w_j^T C64 w_j, and w_j = s (u_j + e), u_j the unit eigenvector
    of C_gpu, |e| <= 2^-24 from the fp32 storage, s the whitening scale with one more fp32 rounding; so
    |var(Z64_j) - s^2 lambda_j| <= s^2 (||E||_F + 3 2^-24 lambda_0) + 4 2^-24 s^2 lambda_j (the same bound,
    scaled).  The fp32 scores differ from Z64 by at most (dim + 2) 2^-24 (sum_d |x_d| |w_d| + |b|) a row
    (an fmaf chain of dim terms and one addition), which moves the variance by at most 2 sqrt(var msq) + msq, msq the
    mean square of that row bound times n / (n - 1)."""
    from node2vec_amd import classify, pca

    X, res, lam64, vec64, e_norm = planted
    n, dim = X.shape
    res = res._replace(whiten=whiten)
    Xd = _device(X)
    W, b = pca.projection(res)
    Z = pca.transform(Xd, res)
    assert Z.dtype == torch.float32 and tuple(Z.shape) == (n, 3)
    assert torch.equal(Z, classify.decision_function(Xd, W, b))
    lam = res.explained_variance.numpy()
    W64, b64 = W.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    var = Z.cpu().numpy().astype(np.float64).var(0, ddof=1)
    row = (dim + 2) * pc.U24 * (np.abs(X.astype(np.float64)) @ np.abs(W64).T + np.abs(b64))
    msq = (row ** 2).sum(0) / (n - 1)
    for j in range(3):
        s2 = 1.0 / lam[j] if whiten else 1.0
        target = 1.0 if whiten else lam[j]
        bound = s2 * (e_norm + 3 * pc.U24 * lam[0]) + 4 * pc.U24 * target + 2 * np.sqrt(target * msq[j]) + msq[j]
        print(f"column {j}: |var - {target:.6g}| = {abs(var[j] - target):.3e} <= {bound:.3e}")
        assert abs(var[j] - target) <= bound


def test_unit_rows_and_skipped_rows_in_the_projection(cpu):
    """unit=True fits x / |x| over the given norms, and transform scores with b = 0 and applies the norms and b to the
    [n, k] scores; a row the fit skipped projects to NaN"""
    from node2vec_amd import classify, pca, similarity

    X = pc.planted(n=500, dim=12, seed=9)
    X[17, 4] = np.nan
    Xd = _device(X)
    inv = similarity.inv_norms(Xd)
    res = pca.fit(Xd, 2, unit=True)
    assert res.unit and res.n_used == 499
    _, S, used = pc.moments(cpu, X, inv.cpu().numpy())
    assert used == 499 and pc.same_bits(pca.moments(Xd, unit=True, inv_norm=inv)[1].cpu().numpy(), S)
    W, b = pca.projection(res)
    Z = pca.transform(Xd, res)
    assert torch.equal(Z[:17], (classify.decision_function(Xd, W, torch.zeros_like(b)) * inv[:, None] + b)[:17])
    assert torch.isnan(Z[17]).all() and torch.isfinite(Z[18:]).all()
    assert torch.equal(pca.transform(Xd, res, inv_norm=inv)[18:], Z[18:])


def test_keyedvectors_pca_and_project():
    from node2vec_amd import pca
    from node2vec_amd.embedding import KeyedVectors

    X = pc.planted(n=300, dim=10, seed=4)
    ids = np.arange(1000, 1300)
    for kv in (KeyedVectors(ids, X), KeyedVectors(ids, _device(X))):
        res = kv.pca(2)
        want = pca.fit(_device(X), 2, unit=True)
        assert res.unit and torch.equal(res.components, want.components) and torch.equal(res.mean, want.mean)
        assert torch.equal(kv.project(res), pca.transform(_device(X), want))
        plain = kv.pca(3, metric="euclidean", whiten=True)
        want = pca.fit(_device(X), 3, whiten=True)
        assert not plain.unit and plain.whiten and torch.equal(plain.components, want.components)
        assert torch.equal(kv.project(plain), pca.transform(_device(X), want))
        part = kv.pca(2, restrict_vocab=100)
        assert part.n_used == 100 and torch.equal(part.components, pca.fit(_device(X[:100]), 2, unit=True).components)
        assert tuple(kv.project(part, restrict_vocab=50).shape) == (50, 2)
    with pytest.raises(ValueError):
        KeyedVectors(ids, X).pca(2, metric="manhattan")
    with pytest.raises(ValueError, match="n_components"):
        KeyedVectors(ids, X).pca(11)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_model_classes_project_their_vocabulary():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    X = pc.planted(n=60, dim=8, seed=6)
    ids = np.arange(60)[::-1] + 100  # vocabulary order is not id order
    names = pd.DataFrame({"id": list(ids) + [159, 500], "name": [f"v{i}" for i in ids] + ["last", "unused"]})
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((60, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((59, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.project(2)
        n2v.model = model(KeyedVectors(ids, X))
        df = n2v.project(2)
        assert list(df.columns) == ["id", "x0", "x1"] and df["id"].tolist() == ids.tolist()
        want = n2v.model.wv.project(n2v.model.wv.pca(2)).cpu().numpy()
        assert n2v.pca_result.unit and np.array_equal(df[["x0", "x1"]].to_numpy(), want)
        assert list(n2v.project(3, metric="euclidean").columns) == ["id", "x0", "x1", "x2"]
        assert not n2v.pca_result.unit
        n2v.name_id = names
        clusters = n2v.cluster(3, seed=1)
        named = n2v.project(2)
        assert list(named.columns) == ["name", "x0", "x1"]
        assert named["name"].tolist() == clusters["name"].tolist()  # cluster()'s rule: id 159 keeps its last name
        assert named["name"].tolist()[:2] == ["last", f"v{ids[1]}"]
        assert named["x0"].tolist() == df["x0"].tolist()
        n2v.name_id = names[names["id"] != 105]
        with pytest.raises(KeyError):
            n2v.project(2)
