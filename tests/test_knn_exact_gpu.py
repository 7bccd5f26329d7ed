"""The nearest-neighbour kernels (csrc/n2v_knn.hip through node2vec_amd.similarity) against their CPU
restatement, oracle/n2v_oracle_knn.c, bit for bit: rows with torch.equal / array_equal, scores by their
int32 bit patterns.  Any other summation order, tie rule or selection slip changes bits that a tolerance
test (tests/test_similarity_gpu.py) lets through.

The cases are chosen on the launch plan (n2v_oracle.knn_plan, checked against n2v_knn_workspace_bytes in
tests/test_knn_oracle.py, which also asserts that TOPK_CASES reach every variant x {1 chunk, odd, even}
x {VEC, scalar}), and the data makes the fused kernel's LDS buffers work: ties that straddle chunks,
scores that rise along the rows (every row passes the threshold, the buffer re-sorts every step), zero
rows and queries, and non-finite values."""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)

pytestmark = pytest.mark.gpu

# n, dim, nq, k, aligned: VEC loads when aligned and dim % 4 == 0, scalar loads otherwise
TOPK_CASES = [
    # variant 0 (64 queries per block, CAP 256)
    (1999, 64, 33, 1, True), (1999, 17, 65, 128, True), (2049, 128, 200, 127, True),
    (2049, 64, 64, 100, False), (6001, 16, 65, 128, True), (6001, 3, 33, 127, True),
    # variant 1 (32, CAP 512)
    (1999, 128, 17, 129, True), (1999, 64, 32, 384, False), (2049, 100, 200, 200, True),
    (2049, 129, 17, 384, True), (6001, 64, 32, 129, True), (6001, 5, 17, 384, True),
    # variant 2 (16, CAP 1024)
    (1999, 16, 1, 385, True), (1999, 63, 9, 128, True), (2049, 64, 16, 896, True),
    (2049, 64, 8, 500, False), (6001, 128, 9, 385, True), (6001, 65, 16, 896, True),
    # variant 3 (8, CAP 2048); n = 2049: the second chunk holds 897 rows, fewer than k
    (1999, 64, 9, 1023, True), (1999, 65, 200, 1024, True), (2049, 128, 65, 897, True),
    (2049, 64, 1, 1024, False), (6001, 64, 200, 1024, True), (6001, 1, 9, 1023, True),
    # n = 1, n < k, 5, 21, 49 and 506 chunks
    (1, 64, 8, 1, True), (1, 3, 33, 10, True), (100, 64, 17, 384, True), (700, 1024, 9, 1024, True),
    (8193, 64, 1, 10, True), (100003, 16, 200, 1024, False), (100003, 128, 1, 10, True),
    (1100000, 64, 1, 128, True),
]


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


def _bits(s):
    s = s.cpu().numpy() if isinstance(s, torch.Tensor) else s
    return np.ascontiguousarray(s, np.float32).view(np.int32)


def _same(got, want, what=""):
    (gr, gs), (wr, ws) = got, want
    gr = gr.cpu().numpy()
    assert gr.shape == wr.shape, what
    bad = np.nonzero((gr != wr).any(axis=1) | (_bits(gs) != _bits(ws)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} queries differ, first {bad[0]}: rows {gr[bad[0]][:8]} want " \
                          f"{wr[bad[0]][:8]}, scores {gs[bad[0]][:8].tolist()} want {ws[bad[0]][:8].tolist()}"


def _expect(oracle, X, k, queries=None, rows=None, restrict=None, exclude_self=False):
    """what similarity.knn must return, from the oracle (restrict and exclude_self as knn defines them)"""
    n = X.shape[0]
    ne = n if restrict is None else min(restrict, n)
    exclude = np.asarray(rows, np.int64) if exclude_self else None
    if rows is not None and ne < n:  # a query row outside the candidates is a vector query
        queries, rows = X[np.asarray(rows)], None
    return oracle.knn_topk(X[:ne], k, queries=queries, rows=rows, exclude=exclude)


def _mixed_rows(rng, n, dim):
    """Gaussian rows; ~5 % copies of three hub rows spread over the whole matrix, ~1 % zero rows"""
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n >= 20:
        hubs = X[:3].copy()
        for i, r in enumerate(rng.choice(n, n // 20, replace=False)):
            X[r] = hubs[i % 3]
        X[rng.choice(n, max(1, n // 100), replace=False)] = 0.0
    return X


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 300, 1023, 1024])
def test_norms_and_scores_bitwise(oracle, dim):
    from node2vec_amd import similarity

    rng = np.random.default_rng(100 + dim)
    n, nq = 300, 37
    X = _mixed_rows(rng, n, dim)
    X[5] = 0.0
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q[3] = 0.0
    Q[4] = X[7]
    R = rng.integers(0, n, nq)
    R[:2] = (5, 7)
    inv = oracle.knn_inv_norms(X)
    want_q = oracle.knn_scores(X, queries=Q)
    want_r = oracle.knn_scores(X, rows=R)
    got = {}
    for aligned in (True, False):
        Xd = _device(X, aligned)
        assert np.array_equal(_bits(similarity.inv_norms(Xd)), _bits(inv)), aligned
        sq = similarity.scores(Xd, queries=_device(Q))
        sr = similarity.scores(Xd, rows=torch.from_numpy(R).cuda())
        assert np.array_equal(_bits(sq), _bits(want_q)), ("queries", aligned)
        assert np.array_equal(_bits(sr), _bits(want_r)), ("rows", aligned)
        got[aligned] = (sq, sr)
    assert torch.equal(got[True][0].view(torch.int32), got[False][0].view(torch.int32))
    assert (got[True][0][3] == 0).all() and (got[True][0][:, 5] == 0).all()


@pytest.mark.parametrize("n,dim,nq,k,aligned", TOPK_CASES)
def test_topk_at_the_plan_edges(oracle, n, dim, nq, k, aligned):
    import n2v_oracle
    from node2vec_amd import similarity

    rng = np.random.default_rng(n * 31 + dim * 7 + nq * 3 + k)
    X = _mixed_rows(rng, n, dim)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    R = rng.integers(0, n, nq)
    if nq > 2:  # a zero query, a copy of a row; the last row and a zero row as query rows
        Q[0], Q[1] = 0.0, X[n // 2]
        zero = np.nonzero(~X.any(axis=1))[0]
        R[0], R[1] = n - 1, zero[0] if len(zero) else 0
    Xd = _device(X, aligned)
    Rd = torch.from_numpy(R).cuda()
    _same(similarity.knn(Xd, k, queries=_device(Q)), _expect(oracle, X, k, queries=Q), "queries")
    _same(similarity.knn(Xd, k, rows=Rd), _expect(oracle, X, k, rows=R), "rows")
    chunk_rows = n2v_oracle.knn_plan(n, dim, nq, k)[3]
    for restrict in sorted({1, k - 1, k, k + 1, chunk_rows, n}):
        if 1 <= restrict <= n:
            _same(similarity.knn(Xd, k, rows=Rd, restrict=restrict),
                  _expect(oracle, X, k, rows=R, restrict=restrict), f"restrict={restrict}")


def _random_plans(count, seed=77):
    """(n, dim, nq, k, aligned) drawn across the plan space, n * nq * dim kept under 1.5e8"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        n, dim, nq = int(rng.integers(1, 20000)), int(rng.integers(1, 301)), int(rng.integers(1, 301))
        if n * nq * dim <= 1.5e8:
            out.append((n, dim, nq, int(rng.integers(1, 1025)), bool(rng.integers(0, 2))))
    return out


@pytest.mark.parametrize("n,dim,nq,k,aligned", _random_plans(24))
def test_topk_random_plans(oracle, n, dim, nq, k, aligned):
    from node2vec_amd import similarity

    rng = np.random.default_rng(n + 7 * dim + 13 * nq + 17 * k)
    X = _mixed_rows(rng, n, dim)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    R = rng.integers(0, n, nq)
    Xd = _device(X, aligned)
    _same(similarity.knn(Xd, k, queries=_device(Q)), _expect(oracle, X, k, queries=Q), "queries")
    _same(similarity.knn(Xd, k, rows=torch.from_numpy(R).cuda()), _expect(oracle, X, k, rows=R), "rows")


ADVERSARIAL_SHAPES = [(6001, 16, 33, 128), (4100, 16, 17, 384), (2049, 16, 16, 896), (6001, 16, 9, 1024)]


def _adversarial(kind, n, dim, nq, rng):
    X = np.zeros((n, dim), np.float32)
    Q = np.zeros((nq, dim), np.float32)
    phi = -0.01 * np.arange(nq)  # queries at or below the first axis: cos(theta - phi) is monotone in theta
    if kind in ("increasing", "decreasing"):
        t = (np.arange(n) if kind == "decreasing" else n - np.arange(n)) * (math.pi / 2 / n)
        X[:, 0], X[:, 1] = np.cos(t), np.sin(t)
        Q[:, 0], Q[:, 1] = np.cos(phi), np.sin(phi)
        return X, Q
    Q[:] = rng.standard_normal((nq, dim))
    if kind == "identical":
        X[:] = rng.standard_normal(dim)
    elif kind == "two":  # alternating rows
        X[:] = rng.standard_normal((2, dim))[np.arange(n) % 2]
    elif kind == "three":  # runs of 700 rows, across chunk boundaries
        X[:] = rng.standard_normal((3, dim))[(np.arange(n) // 700) % 3]
    else:  # "zeros": every third row and every other query zero
        X[:] = rng.standard_normal((n, dim))
        X[::3] = 0.0
        Q[::2] = 0.0
    return X, Q


@pytest.mark.parametrize("kind", ["increasing", "decreasing", "identical", "two", "three", "zeros"])
@pytest.mark.parametrize("n,dim,nq,k", ADVERSARIAL_SHAPES)
def test_topk_adversarial_distributions(oracle, kind, n, dim, nq, k):
    from node2vec_amd import similarity

    rng = np.random.default_rng(sum(map(ord, kind)) * 100003 + n + k)
    X, Q = _adversarial(kind, n, dim, nq, rng)
    Xd = _device(X)
    got = similarity.knn(Xd, k, queries=_device(Q))
    want = _expect(oracle, X, k, queries=Q)
    _same(got, want, kind)
    if kind == "identical":
        assert (got[0] == torch.arange(k, device="cuda")).all()
    if kind == "zeros":  # a zero query scores 0 against every row: rows 0 .. k - 1
        assert (got[0][::2] == torch.arange(k, device="cuda")).all() and (got[1][::2] == 0).all()
    R = np.arange(0, n, max(1, n // nq))[:nq]
    _same(similarity.knn(Xd, k, rows=torch.from_numpy(R).cuda()), _expect(oracle, X, k, rows=R), kind + " rows")


def test_fused_and_sorted_paths_agree_at_the_limit(oracle):
    from node2vec_amd import similarity

    rng = np.random.default_rng(21)
    n, dim = 3000, 32
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[rng.choice(n, 900, replace=False)] = rng.standard_normal((3, dim)).astype(np.float32)[rng.integers(0, 3, 900)]
    X[[100, 500, 2500]] = rng.standard_normal(dim).astype(np.float32)  # a query row (500), copies below and above
    X[7] = 0.0  # a zero-norm query row
    X[2000] = X[1200]  # a query row outside restrict = 1500 with a copy inside
    Xd = _device(X)
    R = np.array([500, 7, 2000, 0, 2999, 1499, 1500])
    Rd = torch.from_numpy(R).cuda()
    Q = _device(rng.standard_normal((9, dim)))
    for kw in (dict(rows=Rd), dict(queries=Q), dict(rows=Rd, restrict=1500)):
        r4, s4 = similarity.knn(Xd, 1024, **kw)
        r5, s5 = similarity.knn(Xd, 1025, **kw)
        assert torch.equal(r4, r5[:, :1024]) and torch.equal(s4.view(torch.int32), s5[:, :1024].view(torch.int32))
    for k in (1023, 1024):  # asks for 1024 (fused) and 1025 (sorted)
        for restrict in (None, 1500):
            got = similarity.knn(Xd, k, rows=Rd, restrict=restrict, exclude_self=True)
            _same(got, _expect(oracle, X, k, rows=R, restrict=restrict, exclude_self=True), f"{k} {restrict}")
            assert not (got[0] == Rd[:, None]).any()
    got = similarity.knn(Xd, 1024, rows=Rd, exclude_self=True)[0].cpu().numpy()
    assert got[0, :2].tolist() == [100, 2500]  # the query row's copies, in row order
    assert got[1, :3].tolist() == [0, 1, 2]  # a zero query row: every score 0, its own row left out


def test_batch_splitting_is_bitwise_invisible(oracle, monkeypatch):
    from node2vec_amd import _lib, similarity

    rng = np.random.default_rng(22)
    n, dim, nq = 3000, 24, 65
    X = _mixed_rows(rng, n, dim)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Xd, Qd = _device(X), _device(Q)
    whole = {k: similarity.knn(Xd, k, queries=Qd) for k in (100, 1024, 1100)}
    full = similarity.scores(Xd, queries=Qd)
    L = _lib.load()
    # the fused path halves 65 -> 33 -> 17 -> 9 queries per launch (with other plans: at k = 100 variant 2,
    # not 0); the sorted path takes 2 queries per launch, scores() 7
    for k, (r, s) in whole.items():
        limit = int(L.n2v_knn_workspace_bytes(n, dim, 9, k)) if k <= 1024 else 16 * n * 2
        assert k > 1024 or L.n2v_knn_workspace_bytes(n, dim, 17, k) > limit
        monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", limit)
        r2, s2 = similarity.knn(Xd, k, queries=Qd)
        assert torch.equal(r, r2) and torch.equal(s.view(torch.int32), s2.view(torch.int32)), k
        _same((r2, s2), _expect(oracle, X, k, queries=Q), f"split k={k}")
    monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", 4 * n * 7)
    assert torch.equal(similarity.scores(Xd, queries=Qd).view(torch.int32), full.view(torch.int32))


def test_non_finite_inputs_are_never_selected(oracle):
    from node2vec_amd import similarity

    rng = np.random.default_rng(23)
    n = 1500
    for dim in (20, 19):
        X = rng.standard_normal((n, dim)).astype(np.float32)
        X[3, 5] = np.nan
        X[900, 1] = np.inf
        X[901] = X[902]  # ties next to the inf row
        Q = rng.standard_normal((6, dim)).astype(np.float32)
        Q[2, 0] = np.nan
        Q[4] = X[902]
        Xd, Qd = _device(X), _device(Q)
        full = similarity.scores(Xd, queries=Qd)
        assert torch.isnan(full[:, 3]).all() and torch.isnan(full[:, 900]).all() and torch.isnan(full[2]).all()
        want = oracle.knn_scores(X, queries=Q)
        nan = np.isnan(want)  # NaN where the oracle has NaN; its sign and payload are not compared
        assert np.array_equal(torch.isnan(full).cpu().numpy(), nan)
        assert np.array_equal(_bits(full)[~nan], _bits(want)[~nan])
        R = np.array([3, 900, 902, 0])
        for k in (5, 1024, 1025, n - 2, n - 1, n, n + 100):
            r, s = similarity.knn(Xd, k, queries=Qd)
            _same((r, s), _expect(oracle, X, k, queries=Q), f"dim {dim} k {k}")
            assert not ((r == 3) | (r == 900)).any() and not torch.isnan(s).any()
            assert (r[2] == -1).all() and (s[2] == float("-inf")).all()  # a NaN query selects nothing
            m = min(k, n - 2)
            assert (r[[0, 1, 3, 4, 5], m:] == -1).all() and (s[[0, 1, 3, 4, 5], m:] == float("-inf")).all()
            assert (r[[0, 1, 3, 4, 5], :m] >= 0).all()
            rr = similarity.knn(Xd, k, rows=torch.from_numpy(R).cuda())
            _same(rr, _expect(oracle, X, k, rows=R), f"rows dim {dim} k {k}")
            assert (rr[0][:2] == -1).all()  # a query row holding NaN or inf


def test_more_queries_than_one_scores_launch_takes():
    """n = 17, k = 1025 (the sorted path): 2^20 - 16 + 9 queries, more than n2v_knn_scores takes at once"""
    from node2vec_amd import similarity

    n, dim, nq = 17, 4, (1 << 20) - 16 + 9
    g = torch.Generator(device="cuda").manual_seed(24)
    X = torch.randn(n, dim, device="cuda", generator=g)
    X[5] = X[11]
    Q = torch.randn(nq, dim, device="cuda", generator=g)
    r, s = similarity.knn(X, 1025, queries=Q)
    h = nq // 2
    for lo, hi in ((0, h), (h, nq)):
        rh, sh = similarity.knn(X, 1025, queries=Q[lo:hi])
        assert torch.equal(rh, r[lo:hi]) and torch.equal(sh.view(torch.int32), s[lo:hi].view(torch.int32))
        del rh, sh
    assert (r[:, n:] == -1).all() and (r[:, :n] >= 0).all()
    # rows 5 and 11 tie: 5 comes first
    assert ((r[:, :n] == 5).int().argmax(dim=1) < (r[:, :n] == 11).int().argmax(dim=1)).all()
    del r, s
    torch.cuda.empty_cache()
