"""The link-prediction classifier without a GPU: tests/cpu_edge_logreg/n2v_edge_logreg_cpu.c (the restatement
csrc/n2v_edge_logreg.hip is held to) against numpy float32 features, the pairs restatement's dot and float64 numpy
inside a derived bound; its slab edges; the whole fit_edges() on the restatement against a float64 Newton solution;
and the argument checks of the four entry points and of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_logreg_cases as ec
import logreg_cases as lc
import pairs_cases as pc
from conftest import ROOT  # noqa: F401
from test_classify_host import MEASURED_ULPS, U

NAMES = ("n2v_edge_logreg_slab_pairs", "n2v_edge_logreg_workspace_bytes", "n2v_edge_logreg_scores",
         "n2v_edge_logreg_loss_grad")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return ec.build(tmp_path_factory.mktemp("edge_logreg_cpu"))


@pytest.fixture(scope="module")
def pairs_cpu(tmp_path_factory):
    return pc.build(tmp_path_factory.mktemp("edge_pairs_cpu"))


@pytest.fixture(scope="module")
def lib():
    from node2vec_amd import _lib

    return _lib.load()


def _gamma(m):
    return m * U / (1 - m * U)


def _score_roundings(dim):
    """roundings on the longest path of a score: a lane's fmaf chain, the xor tree, the add of b0"""
    G = 16 if dim <= 128 else 32 if dim <= 256 else 64
    return 4 * -(-dim // (4 * G)) + int(np.log2(G)) + 1


def _chain_roundings(n_pairs, dim, slab):
    """roundings on the longest path of a slab's fp32 sums: the longest chain (the pairs of ceil(groups / 4) groups
    that fall to one lane group), the tree over the lane groups, the three adds over the waves"""
    P = ec.lane_groups(dim)
    groups = -(-min(n_pairs, slab) // 64)
    return -(-groups // 4) * (64 // P) + int(np.log2(P)) + 3


@pytest.mark.parametrize("dim", [1, 3, 17, 64, 130, 300])
def test_restated_features_equal_numpy_float32(cpu, dim):
    X, a, b, _, _, _ = ec.normal_case(40, dim, 150, dim)
    X[5] = 0.0
    X[6, dim // 2] = -0.0
    for op in ec.OPS:
        assert pc.same_bits(ec.features(cpu, X, a, b, op), pc.numpy_features(X, a, b, op)), (dim, op)


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 128, 129, 256, 300, 1024])
def test_restated_scores_are_the_pairs_dot_of_w_and_f_plus_one_add(cpu, pairs_cpu, dim):
    X, a, b, _, w, b0 = ec.normal_case(30, dim, 70, 100 + dim)
    for op in ec.OPS:
        F = pc.numpy_features(X, a, b, op)
        want = np.array([pc.dot(pairs_cpu, w, f) + b0 for f in F], np.float32)  # float32 + float32: one fp32 add
        assert want.dtype == np.float32
        got = ec.scores(cpu, X, a, b, w, b0, op)
        assert pc.same_bits(got, want), (dim, op)
        assert pc.same_bits(ec.scores(cpu, X, b, a, w, b0, op), got)  # the operators commute bitwise
    a[4], b[9] = -1, 30  # outside [0, n): NaN, never read
    z = ec.scores(cpu, X, a, b, w, b0, "l2")
    assert np.isnan(z[4]) and np.isnan(z[9]) and np.isfinite(np.delete(z, [4, 9])).all()


# (rows, dim, n_pairs): a slab is 64 pairs up to 131 072 pairs, so the first three hold 4, 6 and 3 slabs; 17 and 130
# are ragged; 131 073 pairs make slabs of 128 (two waves of a block at work), 524 289 slabs of 320 (a wave's chains
# run over two groups)
@pytest.mark.parametrize("rows,dim,n_pairs", [(50, 8, 200), (70, 17, 333), (40, 130, 150), (40, 4, 131073),
                                              (40, 4, 524289)])
def test_restated_loss_and_gradient_against_float64_numpy(cpu, rows, dim, n_pairs):
    """The bound, derived as tests/test_classify_host.py derives its own.  The reference takes the fp32 feature rows
    as given (they are exact inputs to both sides).  A score is _score_roundings(dim) = m_z roundings deep:
    |dz| <= g(m_z) (|f| . |w| + |b0|) with g(m) = m U / (1 - m U).  sigmoid' <= 1/4, the spelled p is within 2
    MEASURED p ulps of sigmoid(z) and p - y rounds once more: |dres| <= |dz| / 4 + (2 ulps_p + 1) U.  A slab's fp32
    sums are m = _chain_roundings deep (chain length times unit roundoff times the sum of the absolute terms):
    g(m) sum |res f|.  |dl| <= |dz| + (2 ulps_l + 1) U |l|; the fp64 sums add at most n 2^-53 relative."""
    X, a, b, y, w, b0 = ec.normal_case(rows, dim, n_pairs, rows + dim)
    for op in ("hadamard", "l1"):
        F = ec.features(cpu, X, a, b, op)
        loss, gw, gb = ec.loss_grad(cpu, X, a, b, y, w, b0, op)
        want_loss, want_gw, want_gb, Z, R = ec.ref_loss_grad(F, y, w, b0)
        aF = np.abs(F.astype(np.float64))
        dz = _gamma(_score_roundings(dim)) * (aF @ np.abs(w.astype(np.float64)) + abs(float(b0)))[:, None]
        dres = dz / 4 + (2 * MEASURED_ULPS["p"] + 1) * U
        slab = ec.slab_pairs(cpu, n_pairs, dim)
        m = _chain_roundings(n_pairs, dim, slab)
        aR = np.abs(R) + dres
        bound_gw = (dres.T @ aF + _gamma(m) * (aR.T @ aF) + 1e-15 * np.abs(want_gw)).reshape(-1)
        bound_gb = dres.sum() + _gamma(m) * aR.sum() + 1e-15
        ell = np.logaddexp(0.0, np.where(np.asarray(y).reshape(-1, 1), -Z, Z))
        bound_loss = (dz + (2 * MEASURED_ULPS["l"] + 1) * U * ell).sum() + 1e-13 * ell.sum()
        err = np.abs(gw - want_gw.reshape(-1))
        print(op, "gw err", err.max(), "bound", bound_gw.max(), "loss err", abs(loss[0] - want_loss), bound_loss)
        assert (err <= bound_gw).all(), err.max()
        assert abs(gb[0] - want_gb[0]) <= bound_gb
        assert abs(loss[0] - want_loss) <= bound_loss
        # not vacuous: the bounds are small against the values they bound
        assert bound_gw.max() < 1e-3 * np.abs(want_gw).max() and bound_loss < 1e-4 * want_loss


def test_restated_slabs_and_their_edges(cpu):
    sp = lambda n, dim: ec.slab_pairs(cpu, n, dim)  # noqa: E731
    assert sp(1, 8) == sp(64, 8) == sp(65, 8) == sp(2048 * 64, 64) == 64
    assert sp(2048 * 64 + 1, 64) == 128 and sp(2048 * 256 + 1, 64) == 320 and sp(4 * 10 ** 7, 128) == 19584
    assert sp((1 << 31) - 1, 1024) == 1 << 20
    for dim in (1, 17, 1024):
        assert sp(10 ** 6, dim) == lc.slab_rows(cpu, 10 ** 6, dim, 1)
    # The slabs are folded in fp64 from 0.0, ascending: while a slab is 64 pairs, the sums of a list are the fp64 sums
    # of its slabs' own -- one whole slab, one pair more than a slab, a last slab of 37 pairs, two whole slabs
    X, a, b, y, w, b0 = ec.normal_case(50, 20, 128, 9)
    for op in ("average", "l2"):
        first = ec.loss_grad(cpu, X, a[:64], b[:64], y[:64], w, b0, op)
        for n in (65, 101, 128):
            rest = ec.loss_grad(cpu, X, a[64:n], b[64:n], y[64:n], w, b0, op)
            whole = ec.loss_grad(cpu, X, a[:n], b[:n], y[:n], w, b0, op)
            for got, p, q in zip(whole, first, rest):
                assert ec.same_bits(got, p + q), (op, n)
    # and within a slab a pair's place decides its chain: the sums change when two pairs of one group trade places
    # only by rounding (the set of chains differs), never by more than the bound above allows -- but the SCORES do not
    # depend on the place at all
    z = ec.scores(cpu, X, a, b, w, b0, "l2")
    assert pc.same_bits(ec.scores(cpu, X, a[::-1], b[::-1], w, b0, "l2")[::-1], z)


def test_a_chain_that_underflows_to_minus_zero_never_reaches_the_result(cpu):
    """res f = 1e-30 * -1e-30 rounds to -0: the pair's chain holds -0.  With one pair the other chains are +0 and the
    lane-group tree already gives +0; with whole slabs of such pairs (393 217 pairs: slabs of 256, every chain of a
    full slab -0) the slab's partial is -0 and the fp64 fold from 0.0 gives +0."""
    X = np.array([[-1e-30]], np.float32)
    w, b0 = np.zeros(1, np.float32), np.float32(-69.0)
    assert np.signbit(np.float32(-1e-30) * np.float32(1e-30))
    for n in (1, 2048 * 192 + 1):
        assert n == 1 or ec.slab_pairs(cpu, n, 1) == 256
        idx = np.zeros(n, np.int64)
        loss, gw, gb = ec.loss_grad(cpu, X, idx, idx, np.zeros(n), w, b0, "average")
        assert gw[0] == 0.0 and not np.signbit(gw[0]) and gb[0] > 0.0 and loss[0] > 0.0


def _planted_fit(cpu, op):
    from node2vec_amd import linkpred

    X, a, b, y = ec.planted(op=op)
    res = linkpred.fit_edges(torch.from_numpy(X), torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(y),
                             op=op, C=1.0, tol=1e-4, loss_grad_fn=ec.torch_loss_grad_fn(cpu, X, a, b, y, op))
    return X, a, b, y, res


def test_fit_edges_on_the_restatement_reaches_the_newton_solution(cpu):
    op, tol = "hadamard", 1e-4
    X, a, b, y, res = _planted_fit(cpu, op)
    n, dim = a.shape[0], X.shape[1]
    assert (n, dim) == (400, 8) and 0.2 < y.mean() < 0.8
    assert res.converged and res.reason == "gradient" and res.n_evals >= res.n_iter + 1 and res.op == op
    assert res.w.dtype == torch.float32 and tuple(res.w.shape) == (dim,) and tuple(res.b.shape) == (1,)
    w, b0 = res.w.numpy(), float(res.b[0])
    F = ec.features(cpu, X, a, b, op)
    # the float64 gradient at the returned fp32 parameters
    _, gw, gb, Z, R = ec.ref_loss_grad(F, y, w, b0)
    gw = gw + w.astype(np.float64)
    aF = np.abs(F.astype(np.float64))
    dz = _gamma(_score_roundings(dim)) * (aF @ np.abs(w.astype(np.float64)) + abs(b0))[:, None]
    dres = dz / 4 + (2 * MEASURED_ULPS["p"] + 1) * U
    aR = np.abs(R) + dres
    bound = max((dres.T @ aF + _gamma(n) * (aR.T @ aF)).max(), dres.sum() + _gamma(n) * aR.sum())
    gmax = max(np.abs(gw).max(), np.abs(gb).max())
    print("max|grad| / n", gmax / n, "bound / n", bound / n)
    assert gmax / n <= tol + bound / n
    # Against Newton's solution.  The objective is strongly convex: with mu the smallest eigenvalue of its Hessian,
    # |theta - theta*| <= |grad f(theta)| / mu.  mu is taken at theta* and halved for the Hessian's change on the way
    # (sigmoid' moves by less than a tenth over the |dz| this allows); the score of pair i moves by at most
    # margin[i] = |[f_i, 1]| |dtheta|, so a pair whose Newton score lies further than that from 0 keeps its side.
    Wn, bn = lc.newton(F, y.reshape(-1, 1), C=1.0)
    A = np.hstack([F.astype(np.float64), np.ones((n, 1))])
    Zn = A @ np.r_[Wn[0], bn[0]]
    pn = np.exp(-np.logaddexp(0.0, -Zn))
    H = (A * (pn * (1 - pn))[:, None]).T @ A + np.diag(np.r_[np.ones(dim), 0.0])
    mu = np.linalg.eigvalsh(H)[0] / 2
    margin = np.linalg.norm(np.r_[gw.reshape(-1), gb.reshape(-1)]) / mu * np.linalg.norm(A, axis=1)
    diff = np.abs(Z.reshape(-1) - Zn)
    print("largest |z_fit - z_ref|", diff.max(), "largest margin", margin.max(), "mu", mu)
    assert (diff <= margin).all()
    decided = np.abs(Zn) > margin
    print("undecided share", 1.0 - decided.mean())
    assert 1.0 - decided.mean() <= 0.02  # not vacuous: the margins leave nearly every pair decided
    assert np.array_equal((Z.reshape(-1) > 0)[decided], (Zn > 0)[decided])
    # the same call again: the same bits
    again = _planted_fit(cpu, op)[4]
    assert torch.equal(again.w, res.w) and torch.equal(again.b, res.b) and again.n_evals == res.n_evals


def test_plan_matches_the_restatement(cpu, lib):
    for n, dim in ((1, 1), (300, 20), (2048 * 64, 64), (2048 * 64 + 1, 64), (10 ** 7, 256), ((1 << 31) - 1, 1024),
                   (4 * 10 ** 7, 128), (150001, 3)):
        slab = lib.n2v_edge_logreg_slab_pairs(n, dim)
        assert slab == ec.slab_pairs(cpu, n, dim) == lib.n2v_logreg_slab_rows(n, dim, 1) and slab % 64 == 0
        slabs = -(-n // slab)
        assert slabs <= 2048
        need = lib.n2v_edge_logreg_workspace_bytes(n, dim)
        assert slabs * 4 * (dim + 3) <= need <= slabs * 4 * (dim + 3) + 3 * 256
    assert lib.n2v_edge_logreg_workspace_bytes(0, 64) == 0 and lib.n2v_edge_logreg_slab_pairs(0, 64) == 64
    for n, dim in ((10, 0), (10, 1025), (-1, 64), (1 << 31, 64)):
        assert lib.n2v_edge_logreg_workspace_bytes(n, dim) == -1 and lib.n2v_edge_logreg_slab_pairs(n, dim) == -1


def test_edge_logreg_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; n_pairs == 0 is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    need = lib.n2v_edge_logreg_workspace_bytes(10, 16)
    assert 0 < need <= 4096 * 8 - 16

    def scores(n=5, dim=16, n_pairs=10, op=1, X=p, a=p, b=p, w=p, b0=p, out=p):
        return lib.n2v_edge_logreg_scores(X, n, dim, a, b, n_pairs, op, w, b0, out, None)

    def loss_grad(n=5, dim=16, n_pairs=10, op=1, X=p, a=p, b=p, y=p, w=p, b0=p, loss=p, gw=p, gb=p, ws=p,
                  ws_bytes=need):
        return lib.n2v_edge_logreg_loss_grad(X, n, dim, a, b, y, n_pairs, op, w, b0, loss, gw, gb, ws, ws_bytes, None)

    for call in (scores, loss_grad):
        assert call(n_pairs=0) == _lib.OK and call(n_pairs=0, X=None, a=None, b=None, w=None, b0=None) == _lib.OK
        for kw in (dict(dim=0), dict(dim=1025), dict(n=-1), dict(n=1 << 31), dict(n_pairs=-1), dict(n_pairs=1 << 31),
                   dict(op=-1), dict(op=4), dict(X=None), dict(a=None), dict(b=None), dict(w=None), dict(b0=None)):
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
        for kw in (dict(dim=0), dict(n=-1), dict(op=4)):
            assert call(n_pairs=0, **kw) == _lib.EINVAL, (call.__name__, kw)  # refused before the empty list returns
    assert scores(out=None) == _lib.EINVAL
    assert loss_grad(n_pairs=0, ws=None, ws_bytes=0) == _lib.OK
    for kw in (dict(y=None), dict(loss=None), dict(gw=None), dict(gb=None), dict(ws=None), dict(ws=p + 4),
               dict(ws_bytes=0), dict(ws_bytes=need - 1)):
        assert loss_grad(**kw) == _lib.EINVAL, kw


def test_header_binding_and_docstrings_name_the_entry_points(lib):
    from node2vec_amd import _lib, linkpred

    header = open(ROOT + "/include/n2v_hip.h").read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert "n2v_edge_logreg_scores" in linkpred.edge_scores.__doc__
    assert "n2v_edge_logreg_loss_grad" in linkpred.edge_loss_grad.__doc__
    assert "n2v_edge_logreg_slab_pairs" in linkpred.edge_slab_pairs.__doc__
    assert "trained on" in " ".join(linkpred.link_classifier_auc.__doc__.split())  # says which graph it samples
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15


def test_python_argument_checks(cpu):
    from node2vec_amd import linkpred

    X, a, b, y = ec.planted()
    fn = ec.torch_loss_grad_fn(cpu, X, a, b, y, "hadamard")
    T = torch.from_numpy
    for bad in (-1, X.shape[0]):
        for aa, bb in ((np.r_[a[:-1], bad], b), (a, np.r_[bad, b[1:]])):
            with pytest.raises(IndexError):
                linkpred.fit_edges(T(X), T(aa), T(bb), T(y), loss_grad_fn=fn)
    for value in (np.inf, np.nan):
        Xb = X.copy()
        Xb[3, 1] = value
        with pytest.raises(ValueError, match="non-finite"):
            linkpred.fit_edges(T(Xb), T(a), T(b), T(y), loss_grad_fn=fn)
    for kw in (dict(C=0.0), dict(max_iter=0), dict(tol=-1.0), dict(history=0), dict(op="cosine")):
        with pytest.raises(ValueError):
            linkpred.fit_edges(T(X), T(a), T(b), T(y), loss_grad_fn=fn, **kw)
    with pytest.raises(ValueError):
        linkpred.fit_edges(T(X), T(a), T(b), T(y[:-1]), loss_grad_fn=fn)
    with pytest.raises(ValueError):
        linkpred.fit_edges(T(X), T(a[:0]), T(b[:0]), T(y[:0]), loss_grad_fn=fn)
    res = linkpred.fit_edges(T(X), T(a), T(b), T(y), max_iter=2, tol=0.0, loss_grad_fn=fn)
    assert res.reason == "max_iter" and res.n_iter == 2 and not res.converged
    for fraction in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="train_fraction"):
            linkpred.link_classifier_auc(None, None, 10, 1, train_fraction=fraction)
    with pytest.raises(ValueError, match="operator"):
        linkpred.link_classifier_auc(None, None, 10, 1, op="dot")
