"""Node classification without a GPU: the spelled exp / log1p of tests/cpu_logreg/n2v_logreg_cpu.c (the restatement
csrc/n2v_logreg.hip is held to) against float64 libm, the restated loss and gradient against float64 numpy inside a
derived bound, the host-side pieces of node2vec_amd.classify, the whole fit() on the restatement, and the argument
checks of the four entry points."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

import logreg_cases as lc
from conftest import ROOT  # noqa: F401

U = 2.0 ** -24  # unit roundoff of fp32
# The largest errors of the spelled functions against float64 libm, in fp32 ulps of the true value, measured by
# test_spelled_functions_against_float64_libm on the cases it builds (DESIGN.md "Node classification").
MEASURED_ULPS = {"e": 1.06, "p": 2.24, "l": 1.75}


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return lc.build(tmp_path_factory.mktemp("logreg_cpu"))


@pytest.fixture(scope="module")
def lib():
    from node2vec_amd import _lib

    return _lib.load()


def _ulps(got, want):
    """|got - want| in fp32 ulps of want (float64); the ulp of a value below 2^-126 is 2^-149"""
    want = np.asarray(want, np.float64)
    expo = np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126)))
    return np.abs(np.asarray(got, np.float64) - want) / 2.0 ** (expo - 23)


def _neighbours(x, k=64):
    """every fp32 within k ulps of x"""
    base = np.float32(x).view(np.int32)
    return (base + np.arange(-k, k + 1, dtype=np.int32)).view(np.float32)


def _spelled_cases():
    ln2 = np.log(2.0)
    cuts = [(m + 0.5) * ln2 for m in range(0, 151)]  # where rintf(t log2 e) steps
    z = [_neighbours(v) for v in cuts] + [_neighbours(-v) for v in cuts]
    z += [_neighbours(104.0), _neighbours(-104.0), _neighbours(103.97), _neighbours(87.33), _neighbours(88.72)]
    z.append(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754944e-38, 1.0, -1.0, 103.9, 104.5, 150.0, -150.0,
                       1e30, -1e30], np.float32))
    rng = np.random.default_rng(1)
    z.append((rng.standard_normal(500000) * 4.0).astype(np.float32))
    z.append(rng.uniform(-110.0, 110.0, 500000).astype(np.float32))
    return np.concatenate(z)


def test_spelled_functions_against_float64_libm(cpu):
    z = _spelled_cases()
    z64 = z.astype(np.float64)
    worst = {"e": 0.0, "p": 0.0, "l": 0.0}
    for y in (0, 1):
        got = lc.points(cpu, z, y)
        e = np.exp(-np.abs(z64))
        p = np.exp(-np.logaddexp(0.0, -z64))
        ell = np.logaddexp(0.0, -z64 if y else z64)
        worst["e"] = max(worst["e"], _ulps(got[:, 0], e).max())
        worst["p"] = max(worst["p"], _ulps(got[:, 1], p).max())
        worst["l"] = max(worst["l"], _ulps(got[:, 3], ell).max())
        assert np.array_equal(got[:, 2], got[:, 1] - np.float32(y))  # res = p - y, one rounding
    print("largest errors in ulps:", worst)
    for name, ulps in worst.items():
        assert ulps <= 2.0 * MEASURED_ULPS[name], (name, ulps)
        assert ulps >= 0.25 * MEASURED_ULPS[name], (name, ulps, "MEASURED_ULPS is stale")


def test_exp_of_minus_zero_is_one_and_the_ends_saturate(cpu):
    one = np.float32(1.0)
    assert cpu.n2v_logreg_cpu_exp_neg(-0.0) == one and cpu.n2v_logreg_cpu_exp_neg(0.0) == one
    assert cpu.n2v_logreg_cpu_exp_neg(-104.5) == 0.0 and cpu.n2v_logreg_cpu_exp_neg(-np.inf) == 0.0
    assert np.isnan(cpu.n2v_logreg_cpu_exp_neg(np.nan))
    assert cpu.n2v_logreg_cpu_log1p01(0.0) == 0.0
    got = lc.points(cpu, np.array([0.0, -0.0, 120.0, -120.0, np.inf, -np.inf, np.nan], np.float32), 1)
    assert got[0, 1] == 0.5 and got[1, 1] == 0.5 and got[0, 3] == got[1, 3]
    assert got[2, 1] == 1.0 and got[2, 2] == 0.0 and got[2, 3] == 0.0   # p saturates to exactly 1
    assert got[3, 1] == 0.0 and got[3, 2] == -1.0 and got[3, 3] == 120.0  # and to exactly 0
    assert got[4, 1] == 1.0 and got[5, 1] == 0.0 and got[5, 3] == np.inf
    assert np.isnan(got[6]).all()


@pytest.mark.parametrize("n,dim,c", [(200, 8, 3), (333, 17, 5), (150, 64, 33)])
def test_restated_loss_and_gradient_against_float64_numpy(cpu, n, dim, c):
    """the bound: a score is a chain of dp + 1 roundings (dp = round_up(dim, 16)), |dz| <= g(dp + 1) (|x| . |w| + |b|)
    with g(m) = m U / (1 - m U); sigmoid' <= 1/4, the spelled p is within 2 MEASURED p ulps (<= U each, p <= 1) of
    sigmoid(z) and p - y rounds once more: |dres| <= |dz| / 4 + (2 ulps_p + 1) U; a slab's fp32 chain over m rows adds
    g(m) sum |res x| (chain length times unit roundoff times the sum of the absolute terms); l' is within [-1, 1]:
    |dl| <= |dz| + 2 ulps_l U |l|; the fp64 sums add at most n c 2^-53 relative."""
    X, W, b, Y = lc.normal_case(n, dim, c, n + dim)
    loss, gW, gb = lc.loss_grad(cpu, X, Y, W, b)
    want_loss, want_gW, want_gb, Z, R = lc.ref_loss_grad(X, Y, W, b)
    dp = (dim + 15) // 16 * 16
    g = lambda m: m * U / (1 - m * U)  # noqa: E731
    aX, aW = np.abs(X.astype(np.float64)), np.abs(W.astype(np.float64))
    dz = g(dp + 1) * (aX @ aW.T + np.abs(b.astype(np.float64)))
    dres = dz / 4 + (2 * MEASURED_ULPS["p"] + 1) * U
    m = min(n, lc.slab_rows(cpu, n, dim, c))
    aR = np.abs(R) + dres
    bound_gW = dres.T @ aX + g(m) * (aR.T @ aX) + 1e-15 * np.abs(want_gW)
    bound_gb = dres.sum(0) + g(m) * aR.sum(0) + 1e-15
    ell = np.logaddexp(0.0, np.where(Y, -Z, Z))
    bound_loss = (dz + (2 * MEASURED_ULPS["l"] + 1) * U * ell).sum() + 1e-13 * ell.sum()
    assert (np.abs(gW - want_gW) <= bound_gW).all(), np.abs(gW - want_gW).max()
    assert (np.abs(gb - want_gb) <= bound_gb).all()
    assert abs(loss[0] - want_loss) <= bound_loss
    # not vacuous: the bounds are small against the values they bound
    assert bound_gW.max() < 1e-3 * np.abs(want_gW).max() and bound_loss < 1e-4 * want_loss


def test_same_bits_compares_in_the_arrays_own_precision():
    one = np.array([1.0, -0.0, np.nan])
    assert lc.same_bits(one, one.copy()) and lc.same_bits(one.astype(np.float32), one.astype(np.float32))
    assert not lc.same_bits(one, np.array([1.0 + 2.0 ** -52, -0.0, np.nan]))  # one float64 ulp
    assert not lc.same_bits(one, np.array([1.0, 0.0, np.nan])) and not lc.same_bits(one, one.astype(np.float32))


def test_restated_slabs_and_padding_rows(cpu):
    assert lc.slab_rows(cpu, 300, 20, 18) == 64 and lc.slab_rows(cpu, 10 ** 7, 64, 8) == 4928
    assert lc.slab_rows(cpu, (1 << 23) + 5, 260, 4) * 8 < 1 << 24
    assert lc.slab_rows(cpu, 10 ** 6, 1024, 1024) == (10 ** 6 // 127 // 64 + 1) * 64
    # a chain that underflows to -0 leaves the padded slab as +0: fmaf(+0, +0, -0) = +0
    X = np.array([[-1e-30]], np.float32)
    W, b, Y = np.zeros((1, 1), np.float32), np.array([-69.0], np.float32), np.array([[0]])
    _, gW, _ = lc.loss_grad(cpu, X, Y, W, b)
    assert gW[0, 0] == 0.0 and not np.signbit(gW[0, 0])


@pytest.mark.parametrize("c", [31, 32, 33])
def test_pack_labels_at_the_word_edges(c):
    from node2vec_amd import classify

    rng = np.random.default_rng(c)
    Y = rng.random((9, c)) < 0.5
    Y[0], Y[1] = True, False
    Y[2] = False
    Y[2, c - 1] = True
    got = classify.pack_labels(torch.from_numpy(Y))
    assert got.dtype == torch.int32 and tuple(got.shape) == (9, (c + 31) // 32)
    words = got.numpy().view(np.uint32)
    assert np.array_equal(words, lc.pack(Y))
    for k in range(c):
        assert np.array_equal((words[:, k >> 5] >> np.uint32(k & 31)) & 1, Y[:, k])
    assert np.array_equal(classify.pack_labels(torch.from_numpy(Y.astype(np.float32))).numpy(), got.numpy())
    if c % 32:
        assert not (words[:, -1] >> np.uint32(c % 32)).any()  # no bit past the last class


def test_labels_from_frame():
    from node2vec_amd import classify

    ids = np.array([30, 10, 20, 40])
    df = pd.DataFrame({"id": [10, 30, 10, 20], "label": ["b", "a", "c", "b"]})
    Y, classes = classify.labels_from_frame(df, ids)
    assert classes.tolist() == ["a", "b", "c"]
    assert Y.tolist() == [[True, False, False], [False, True, True], [False, True, False], [False, False, False]]
    with pytest.raises(KeyError):
        classify.labels_from_frame(pd.DataFrame({"id": [10, 99], "label": ["a", "b"]}), ids)
    with pytest.raises(ValueError):
        classify.labels_from_frame(pd.DataFrame({"id": [10]}), ids)


def test_f1_scores_by_hand_with_an_empty_class():
    from node2vec_amd import classify

    truth = torch.tensor([[1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]])
    pred = torch.tensor([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]])
    # class 0: TP 2, FP 1, FN 1 -> 4 / 6; class 1: TP 2, FP 0, FN 1 -> 4 / 5; class 2: nothing -> 0
    got = classify.f1_scores(truth, pred)
    assert got["per_class"].dtype == torch.float64
    assert got["per_class"].tolist() == [4 / 6, 4 / 5, 0.0]
    assert got["macro"] == pytest.approx((4 / 6 + 4 / 5) / 3, abs=1e-15)
    assert got["micro"] == 8 / 11  # TP 4, FP 1, FN 2
    none = classify.f1_scores(torch.zeros(3, 2), torch.zeros(3, 2))
    assert none["micro"] == 0.0 and none["macro"] == 0.0


def test_f1_scores_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    from node2vec_amd import classify

    rng = np.random.default_rng(8)
    truth, pred = rng.random((300, 7)) < 0.3, rng.random((300, 7)) < 0.3
    got = classify.f1_scores(torch.from_numpy(truth), torch.from_numpy(pred))
    assert got["micro"] == pytest.approx(metrics.f1_score(truth, pred, average="micro"), abs=1e-14)
    assert got["macro"] == pytest.approx(metrics.f1_score(truth, pred, average="macro"), abs=1e-14)


def test_predict_top_ties_go_to_the_lower_class():
    from node2vec_amd import classify

    scores = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.5, -1.0, 0.5, 4.0], [1.0, 2.0, 3.0, 4.0]])
    got = classify.predict_top(scores, [1, 2, 2, 0])
    assert got.tolist() == [[False, True, False, False], [True, True, False, False], [True, False, False, True],
                            [False] * 4]
    assert classify.predict(scores[:1], 2.5).tolist() == [[False, True, True, False]]


def test_two_loop_recursion_on_a_dense_quadratic():
    """f = x^T A x / 2 - b^T x: with exact line searches and n pairs L-BFGS's direction is Newton's; here the pairs
    of n conjugate-gradient-like steps span the space, so -H g lands on the minimiser A^-1 b"""
    from node2vec_amd import classify

    rng = np.random.default_rng(2)
    M = rng.standard_normal((6, 6))
    A = torch.from_numpy(M @ M.T + 6 * np.eye(6))
    b = torch.from_numpy(rng.standard_normal(6))
    want = torch.linalg.solve(A, b)
    x = torch.zeros(6, dtype=torch.float64)
    pairs = []
    assert torch.equal(classify.two_loop(A @ x - b, []), -(A @ x - b))
    for _ in range(12):
        g = A @ x - b
        if float(g.abs().max()) < 1e-13:
            break
        d = classify.two_loop(g, pairs)
        assert float((g * d).sum()) < 0.0  # a descent direction
        t = -float((g * d).sum()) / float(d @ A @ d)  # the exact line search
        s = t * d
        pairs = (pairs + [(s, A @ s)])[-6:]
        x = x + s
    assert torch.allclose(x, want, rtol=0, atol=1e-12)


# m: four times the largest |z_fit - z_ref| measured on the planted case (0.0262, printed by the test)
PLANTED_MARGIN = 4 * 0.0262


def test_fit_on_the_restatement_reaches_the_newton_solution(cpu):
    from node2vec_amd import classify

    X, Y = lc.planted()
    n, dim = X.shape
    tol = 1e-4
    res = classify.fit(torch.from_numpy(X), torch.from_numpy(Y), C=1.0, tol=tol,
                       loss_grad_fn=lc.torch_loss_grad_fn(cpu, X, Y))
    assert res.converged and res.reason == "gradient" and res.n_evals >= res.n_iter + 1
    assert res.W.dtype == torch.float32 and tuple(res.W.shape) == (3, dim)
    W, b = res.W.numpy(), res.b.numpy()
    # the float64 gradient at the returned fp32 parameters
    _, gW, gb, Z, R = lc.ref_loss_grad(X, Y, W, b)
    gW = gW + W.astype(np.float64)
    dp = 16
    g = lambda m: m * U / (1 - m * U)  # noqa: E731
    aX = np.abs(X.astype(np.float64))
    dz = g(dp + 1) * (aX @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64)))
    dres = dz / 4 + (2 * MEASURED_ULPS["p"] + 1) * U
    aR = np.abs(R) + dres
    bound = max((dres.T @ aX + g(n) * (aR.T @ aX)).max(), (dres.sum(0) + g(n) * aR.sum(0)).max())
    gmax = max(np.abs(gW).max(), np.abs(gb).max())
    print("max|grad| / n", gmax / n, "bound / n", bound / n)
    assert gmax / n <= tol + bound / n
    # against Newton's solution
    Wn, bn = lc.newton(X, Y, C=1.0)
    Zn = X.astype(np.float64) @ Wn.T + bn
    diff = np.abs(Z - Zn).max()
    print("largest |z_fit - z_ref|", diff)
    assert diff <= PLANTED_MARGIN / 2
    decided = np.abs(Zn) >= PLANTED_MARGIN
    assert 1.0 - decided.mean() <= 0.02
    assert np.array_equal((Z > 0)[decided], (Zn > 0)[decided])
    # the same call again: the same bits
    again = classify.fit(torch.from_numpy(X), torch.from_numpy(Y), C=1.0, tol=tol,
                         loss_grad_fn=lc.torch_loss_grad_fn(cpu, X, Y))
    assert torch.equal(again.W, res.W) and torch.equal(again.b, res.b) and again.n_evals == res.n_evals


def test_fit_stops_at_max_iter_and_refuses_bad_input(cpu):
    from node2vec_amd import classify

    X, Y = lc.planted()
    fn = lc.torch_loss_grad_fn(cpu, X, Y)
    res = classify.fit(torch.from_numpy(X), torch.from_numpy(Y), max_iter=2, tol=0.0, loss_grad_fn=fn)
    assert res.reason == "max_iter" and res.n_iter == 2 and not res.converged
    bad = X.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        classify.fit(torch.from_numpy(bad), torch.from_numpy(Y), loss_grad_fn=fn)
    for kw in (dict(C=0.0), dict(max_iter=0), dict(tol=-1.0), dict(history=0)):
        with pytest.raises(ValueError):
            classify.fit(torch.from_numpy(X), torch.from_numpy(Y), loss_grad_fn=fn, **kw)
    assert sorted(np.concatenate(classify.split_rows(11, 0.5, 3)).tolist()) == list(range(11))
    assert len(classify.split_rows(11, 0.5, 3)[0]) == round(0.5 * 11)


def test_plan_matches_the_restatement(cpu, lib):
    for n, dim, c in ((1, 1, 1), (300, 20, 18), (10 ** 7, 64, 8), (10 ** 7, 256, 1024), ((1 << 31) - 1, 1024, 1024),
                      ((1 << 23) + 5, 260, 4), (150001, 8, 4)):
        slab = lib.n2v_logreg_slab_rows(n, dim, c)
        assert slab == lc.slab_rows(cpu, n, dim, c) and slab % 64 == 0
        slabs = -(-n // slab)
        assert slabs * 4 * c * (dim + 3) <= 512 << 20
        assert lib.n2v_logreg_workspace_bytes(n, dim, c) >= slabs * 4 * c * (dim + 3)
    assert lib.n2v_logreg_workspace_bytes(0, 64, 8) == 0
    assert lib.n2v_logreg_workspace_bytes(10, 0, 8) == -1 and lib.n2v_logreg_slab_rows(10, 64, 1025) == -1
    assert lib.n2v_logreg_slab_rows(-1, 64, 8) == -1 and lib.n2v_logreg_slab_rows(1 << 31, 64, 8) == -1


def test_logreg_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; n == 0 is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    need = lib.n2v_logreg_workspace_bytes(10, 16, 4)
    assert 0 < need <= 4096 * 8 - 16

    def scores(n=10, dim=16, c=4, X=p, W=p, b=p, out=p, ws=p, ws_bytes=need):
        return lib.n2v_logreg_scores(X, n, dim, W, b, c, out, ws, ws_bytes, None)

    def loss_grad(n=10, dim=16, c=4, X=p, y=p, W=p, b=p, loss=p, gW=p, gb=p, ws=p, ws_bytes=need):
        return lib.n2v_logreg_loss_grad(X, y, n, dim, W, b, c, loss, gW, gb, ws, ws_bytes, None)

    for call in (scores, loss_grad):
        assert call(n=0) == _lib.OK and call(n=0, X=None, ws=None, ws_bytes=0) == _lib.OK
        for kw in (dict(dim=0), dict(dim=1025), dict(c=0), dict(c=1025), dict(n=-1), dict(n=1 << 31), dict(X=None),
                   dict(W=None), dict(b=None), dict(ws=None), dict(ws=p + 4), dict(ws_bytes=0),
                   dict(ws_bytes=need - 1)):
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
        for kw in (dict(dim=0), dict(c=1025)):
            assert call(n=0, **kw) == _lib.EINVAL, (call.__name__, kw)  # refused before the empty input returns
    assert scores(out=None) == _lib.EINVAL
    for kw in (dict(y=None), dict(loss=None), dict(gW=None), dict(gb=None)):
        assert loss_grad(**kw) == _lib.EINVAL, kw


def test_header_and_binding_name_the_logreg_entry_points(lib):
    from node2vec_amd import _lib

    names = ("n2v_logreg_slab_rows", "n2v_logreg_workspace_bytes", "n2v_logreg_scores", "n2v_logreg_loss_grad")
    header = open(ROOT + "/include/n2v_hip.h").read()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15
