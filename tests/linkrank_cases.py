"""Cases and expected values of the link-ranking tests (tests/test_linkrank_host.py, tests/test_linkrank_gpu.py).

Everything here runs on the CPU.  The expected counts come from the committed CPU restatement of the score chain,
n2v_oracle.knn_scores (oracle/n2v_oracle_knn.c): one full score row per query, a mask built from the CSR, plain numpy
counts.  A case is a matrix X, queries (a, b) and a filter CSR:

  kind "dups"  Gaussian rows, about one in eight a copy of another (equal bits by construction: ties under cosine
               and dot alike), one zero row
  kind "ints"  small-integer rows: dot products are exact in fp32, so they tie exactly whatever the order
  kind "near"  no two rows equal: Gaussian rows, and rows that differ from some query's target in a few coordinates
               by one ulp, so that their scores lie within a rounding of the threshold -- which side they fall on is
               the summation order's doing, and a restatement that sums d sequentially counts differently

The filter graph is a directed multigraph with, when n allows (n >= 24): row 0 without out-edges, row 1 of degree 1,
row 2 of degree >= 17 with a multi-edge in it, row 3 with a self-loop and a multi-edge; every other row has 0 .. 5
random columns (repeats and self-loops as they fall).  The queries begin with (0, *), (1, its neighbour), (2, *),
(3, 3), (3, *), (2, *) again, then random pairs."""
from typing import NamedTuple, Optional

import numpy as np

NS = (1, 2, 15, 16, 17, 63, 64, 65, 1000)
DIMS = (1, 3, 16, 100, 128, 1024)
QS = (1, 16, 17, 65)
METRICS = ("cosine", "dot")


def rich(n, nq):
    """such a case must show a filtered neighbour above a threshold, a tie and 16 rows above a threshold (smaller
    ones cannot: fewer than 18 rows, or a single query, which is the one on the row without out-edges)"""
    return n >= 63 and nq >= 16


class Case(NamedTuple):
    X: np.ndarray                 # fp32 [n, dim]
    a: np.ndarray                 # int64 [nq]
    b: np.ndarray
    rowptr: Optional[np.ndarray]  # int64 [n + 1] | None: no filter
    col: Optional[np.ndarray]     # int32
    metric: str


def filter_graph(rng, n):
    """(rowptr int64 [n + 1], col int32): the multigraph of the module's docstring, columns ascending within a row"""
    rows = [list(rng.integers(0, n, rng.integers(0, min(n, 5) + 1))) for _ in range(n)]
    if n >= 24:
        rows[0] = []
        rows[1] = [int(rng.integers(2, n))]
        many = list(rng.choice(np.arange(3, n), 19, replace=False))
        rows[2] = many + [many[0], many[0], many[5]]
        other = int(rng.integers(4, n))
        rows[3] = [3, other, other, int(rng.integers(4, n))]
    rows = [sorted(int(c) for c in r) for r in rows]
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.array([c for r in rows for c in r], np.int32)


def queries(rng, n, nq, rowptr, col):
    a, b = rng.integers(0, n, nq), rng.integers(0, n, nq)
    if n >= 24 and rowptr is not None:
        head = [(0, int(rng.integers(0, n))), (1, int(col[rowptr[1]])), (2, int(rng.integers(0, n))), (3, 3),
                (3, int(rng.integers(0, n))), None]
        head[5] = head[2]
        for i, (u, v) in enumerate(head[:nq]):
            a[i], b[i] = u, v
    elif nq >= 3:
        a[1], b[1] = a[0], b[0]  # a repeated query
        b[2] = a[2]              # u == v
    return a.astype(np.int64), b.astype(np.int64)


def matrix(rng, n, dim, kind, b):
    if kind == "ints":
        X = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    else:
        X = rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "dups" and n >= 8:
        for r in rng.choice(n, n // 8, replace=False):
            X[r] = X[b[rng.integers(0, len(b))]]  # a copy of some query's target: a tie with its threshold
        X[rng.integers(0, n)] = 0.0
    if kind == "near":
        targets = set(int(v) for v in b)
        free = [r for r in range(n) if r not in targets]
        for r in rng.choice(free, min(len(free), n // 2), replace=False):
            X[r] = X[b[rng.integers(0, len(b))]]
            for d in rng.choice(dim, min(dim, 3), replace=False):
                X[r, d] = np.nextafter(X[r, d], np.float32(np.inf if rng.random() < 0.5 else -np.inf))
        assert len(np.unique(X, axis=0)) == n or dim < 8, "near: two rows are equal"
    return X


def make_case(n, dim, nq, metric, kind=None, seed=0, filtered=True) -> Case:
    rng = np.random.default_rng([n, dim, nq, METRICS.index(metric), seed])
    rowptr, col = filter_graph(rng, n) if filtered else (None, None)
    a, b = queries(rng, n, nq, rowptr, col)
    kind = kind or ("dups" if metric == "cosine" else "ints")
    return Case(matrix(rng, n, dim, kind, b), a, b, rowptr, col, metric)


def inv_norms(oracle, case):
    """cosine: the restated inverse norms; dot: ones (multiplying by 1.0f changes no bit)"""
    if case.metric == "cosine":
        return oracle.knn_inv_norms(case.X)
    return np.ones(case.X.shape[0], np.float32)


def excluded(case, q):
    """bool [n]: the rows that are no candidates of query q -- u, v and the columns of row u"""
    out = np.zeros(case.X.shape[0], bool)
    u = case.a[q]
    out[u] = out[case.b[q]] = True
    if case.rowptr is not None:
        out[case.col[case.rowptr[u]:case.rowptr[u + 1]]] = True
    return out


def expected(oracle, case, order=0):
    """(counts int64 [nq, 2], thr fp32 [nq], scores fp32 [nq, n]) from the restated score rows; order 1: the
    restatement that sums d sequentially"""
    S = oracle.knn_scores(case.X, rows=case.a, inv_norm=inv_norms(oracle, case), order=order)
    nq = len(case.a)
    thr = S[np.arange(nq), case.b].copy()
    counts = np.zeros((nq, 2), np.int64)
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            cand = S[q][~excluded(case, q)]
            counts[q] = ((cand > thr[q]).sum(), (cand == thr[q]).sum())  # a NaN on either side: neither
    return counts, thr, S


def assert_meaningful(case, counts, thr, S):
    """the case can tell a wrong kernel from a right one, from the restatement alone: dropping the filter would
    change some `greater`, some query has ties, some query has at least 16 rows above it"""
    assert (counts[:, 1] > 0).any(), "no query has a tie"
    assert (counts[:, 0] >= 16).any(), "no query has 16 rows above its threshold"
    if case.rowptr is None:
        return
    hit = False
    with np.errstate(invalid="ignore"):
        for q in range(len(case.a)):
            u, v = case.a[q], case.b[q]
            nb = case.col[case.rowptr[u]:case.rowptr[u + 1]]
            nb = nb[(nb != u) & (nb != v)]
            hit = hit or bool((S[q][nb] > thr[q]).any())
    assert hit, "no filtered neighbour scores above its query's threshold"


def shape_cases():
    """(n, dim, nq, metric): every n with every nq, the dimensions and metrics taken in turn; every dimension with
    both metrics at n = 65, nq = 17"""
    out = []
    for i, n in enumerate(NS):
        for j, nq in enumerate(QS):
            out.append((n, DIMS[(i + j) % len(DIMS)], nq, METRICS[(i + 2 * j + j // 2) % 2]))
    for dim in DIMS:
        for metric in METRICS:
            if (65, dim, 17, metric) not in out:
                out.append((65, dim, 17, metric))
    return out


def chunked_n(plan):
    """an n whose scan has at least two chunks, the last one ragged: plan(n) -> (chunk_rows, n_chunks)"""
    n = 2049
    chunk_rows, n_chunks = plan(n)
    assert n_chunks >= 2 and n % chunk_rows != 0, (n, chunk_rows, n_chunks)
    return n
