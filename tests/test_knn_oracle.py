"""The nearest-neighbour oracle (oracle/n2v_oracle_knn.c) and the launch plan of csrc/n2v_knn.hip, on the
CPU.  The GPU kernels are compared with this oracle bit for bit (tests/test_knn_exact_gpu.py), so it has to
be right (float64 agrees within the kernels' old tolerance) and specific (another fmaf order gives other
bits).  The plan restatement (n2v_oracle.knn_plan) is what the GPU tests use to assert that they reach
every launch variant, chunk count and load path: it is checked here against n2v_knn_workspace_bytes,
which is host-only."""
import itertools

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)


def _cos64(X, Q):
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    nx, nq = np.linalg.norm(X64, axis=1), np.linalg.norm(Q64, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (Q64 @ X64.T) / (nq[:, None] * nx[None, :])
    return np.nan_to_num(S, nan=0.0)


@pytest.mark.parametrize("dim", [1, 5, 16, 100, 128, 300, 1024])
def test_oracle_scores_agree_with_float64(oracle, dim):
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((700, dim)).astype(np.float32)
    Q = rng.standard_normal((20, dim)).astype(np.float32)
    X[3] = 0.0
    tol = dim * 2.0 ** -22
    S = oracle.knn_scores(X, queries=Q)
    assert S.dtype == np.float32 and S.shape == (20, 700)
    assert np.abs(S - _cos64(X, Q)).max() <= tol
    assert (S[:, 3] == 0).all()
    inv = oracle.knn_inv_norms(X)
    assert inv[3] == 0 and np.abs(inv.astype(np.float64) * np.linalg.norm(X.astype(np.float64), axis=1)
                                  - np.where(np.arange(700) == 3, 0, 1)).max() <= 2 ** -20
    # a query given as a row normalises with inv_norm[r]: the same bits as the row given as a vector
    rows = np.array([0, 3, 699, 5, 5])
    assert np.array_equal(oracle.knn_scores(X, rows=rows).view(np.int32),
                          oracle.knn_scores(X, queries=X[rows]).view(np.int32))


def test_oracle_order_is_specific():
    """a plain sequential fmaf chain passes the same tolerance but differs in the bits of many scores"""
    import n2v_oracle as oracle

    oracle.build()
    rng = np.random.default_rng(1)
    dim = 128
    X = rng.standard_normal((2000, dim)).astype(np.float32)
    Q = rng.standard_normal((16, dim)).astype(np.float32)
    a = oracle.knn_scores(X, queries=Q, order=0)
    b = oracle.knn_scores(X, queries=Q, order=1)
    ref = _cos64(X, Q)
    assert np.abs(a - ref).max() <= dim * 2.0 ** -22 and np.abs(b - ref).max() <= dim * 2.0 ** -22
    differ = float((a.view(np.int32) != b.view(np.int32)).mean())
    assert differ > 0.2, differ


def test_oracle_topk_rule(oracle):
    """(score descending, row ascending), NaN never selected, (-1, -inf) tail, exclude"""
    rng = np.random.default_rng(2)
    base = rng.standard_normal((3, 8)).astype(np.float32)
    X = base[rng.integers(0, 3, 300)]
    X[10] = np.nan
    X[11, 2] = np.inf
    Q = np.concatenate([rng.standard_normal((4, 8)).astype(np.float32), np.full((1, 8), np.nan, np.float32)])
    S = oracle.knn_scores(X, queries=Q)
    assert np.isnan(S[:, 10]).all() and np.isnan(S[:, 11]).all() and np.isnan(S[4]).all()
    for k in (1, 50, 298, 299, 400):
        r, s = oracle.knn_topk(X, k, queries=Q)
        for q in range(4):
            ok = np.nonzero(~np.isnan(S[q]))[0]
            order = ok[np.lexsort((ok, -S[q, ok].astype(np.float64)))][:k]
            m = len(order)
            assert r[q, :m].tolist() == order.tolist()
            assert np.array_equal(s[q, :m].view(np.int32), S[q, order].view(np.int32))
            assert (r[q, m:] == -1).all() and (s[q, m:] == -np.inf).all()
        assert (r[4] == -1).all() and (s[4] == -np.inf).all()
    r, _ = oracle.knn_topk(X, 5, rows=[0, 1], exclude=[0, -1])
    full, _ = oracle.knn_topk(X, 6, rows=[0, 1])
    assert r[0].tolist() == [x for x in full[0].tolist() if x != 0][:5] and r[1].tolist() == full[1, :5].tolist()


PLAN_GRID = list(itertools.product(
    [1, 15, 127, 128, 129, 2048, 2049, 4096, 6144, 10000, 100003, 1 << 20, (1 << 31) - 1],  # n
    [1, 3, 16, 100, 1024],  # dim
    [1, 8, 9, 16, 17, 32, 33, 64, 65, 200, 4096, 100000],  # nq
    [1, 127, 128, 129, 384, 385, 896, 897, 1024],  # k
))


def test_plan_restatement_matches_workspace_bytes():
    from node2vec_amd import _lib
    import n2v_oracle as oracle

    L = _lib.load()
    for n, dim, nq, k in PLAN_GRID:
        variant, qt, n_chunks, chunk_rows, ws = oracle.knn_plan(n, dim, nq, k)
        assert L.n2v_knn_workspace_bytes(n, dim, nq, k) == ws, (n, dim, nq, k)
        assert 1 <= n_chunks <= 512 and chunk_rows % 128 == 0
        assert (n_chunks - 1) * chunk_rows < n <= n_chunks * chunk_rows
        assert qt == (64, 32, 16, 8)[variant]
    # every variant, one chunk, odd and even counts, and the 512-chunk ceiling occur in the grid
    seen = {(p[0], 1 if p[2] == 1 else 2 + p[2] % 2) for p in (oracle.knn_plan(*c) for c in PLAN_GRID)}
    assert seen == {(v, c) for v in range(4) for c in (1, 2, 3)}
    assert max(oracle.knn_plan(*c)[2] for c in PLAN_GRID) == 512


def test_gpu_cases_cover_every_launch_path():
    """tests/test_knn_exact_gpu.py reaches every variant x {1 chunk, an odd count > 1, an even count} x
    {VEC, scalar loads} with its plan-edge cases alone, and the adversarial shapes every variant"""
    import n2v_oracle as oracle
    from test_knn_exact_gpu import ADVERSARIAL_SHAPES, TOPK_CASES

    def klass(n_chunks):
        return "one" if n_chunks == 1 else ("odd", "even")[n_chunks % 2 == 0]

    seen = set()
    for n, dim, nq, k, aligned in TOPK_CASES:
        variant, _, n_chunks, _, _ = oracle.knn_plan(n, dim, nq, k)
        seen.add((variant, klass(n_chunks), aligned and dim % 4 == 0))
    assert seen == {(v, c, vec) for v in range(4) for c in ("one", "odd", "even") for vec in (False, True)}
    assert {oracle.knn_plan(*s)[0] for s in ADVERSARIAL_SHAPES} == {0, 1, 2, 3}
    assert all(oracle.knn_plan(*s)[2] > 1 for s in ADVERSARIAL_SHAPES)
    assert {n for n, *_ in TOPK_CASES} >= {1, 100} and any(k > n for n, _, _, k, _ in TOPK_CASES)
