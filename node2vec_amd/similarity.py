"""Nearest neighbours by cosine over trained vectors, on the GPU (csrc/n2v_knn.hip).

What gensim 3.8 computes in KeyedVectors.init_sims / most_similar on the Word2Vec model the reference
returns (embedding.py:120-127), without the normalised copy of the matrix and without the
n_queries x n score matrix: the top k of every query are selected inside the scan.  Exact fp32, brute
force; every score is computed in one fixed order, so results do not depend on how queries are batched
(DESIGN.md "Nearest neighbours").  A row or query of norm 0 scores 0 (gensim: NaN).  A row or query holding
inf or NaN scores NaN; knn() never selects a NaN score.

Device tensors in and out.  There is no CPU path: a missing GPU or library raises.
"""
from typing import Optional, Tuple

import torch

from node2vec_amd import _dense, _lib

MAX_DIM = _dense.MAX_DIM
MAX_FUSED_K = 1024  # n2v_knn_topk's limit; larger k go through the full scores and a stable sort
WORKSPACE_LIMIT = 1 << 30  # bytes of workspace (or of full scores) per launch: query batches are split to fit


def inv_norms(X: torch.Tensor) -> torch.Tensor:
    """1 / ||x_r|| for every row (0 for a zero row), fp32 [n]: the norms init_sims computes."""
    X = _dense.matrix(X)
    out = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().n2v_knn_inv_norms(X.data_ptr(), X.shape[0], X.shape[1], out.data_ptr(),
                                                  _lib.current_stream_ptr()), "n2v_knn_inv_norms")
    return out


def _inputs(X, queries, rows, restrict, inv_norm):
    """(X', inv_norm', queries, rows): X' the rows [0, restrict); a query row outside them becomes its vector"""
    X = _dense.matrix(X)
    if (queries is None) == (rows is None):
        raise ValueError("give exactly one of queries= / rows=")
    n = X.shape[0]
    if restrict is not None:
        restrict = int(restrict)
        if restrict < 0:
            raise ValueError("restrict must be >= 0")
    n_eff = n if restrict is None else min(restrict, n)
    inv_norm = _dense.norms(X[:n_eff], inv_norm)
    if rows is not None:
        rows = _dense.rows(rows, n, X.device)
    else:
        queries = _dense.queries(queries, X.shape[1], X.device)
    if restrict is not None and restrict < n:
        if rows is not None:  # the same q_hat bit for bit: both forms normalise with the same sum
            queries, rows = X[rows].contiguous(), None
        X = X[:n_eff]
    return X, inv_norm, queries, rows


def _scores(X, inv_norm, queries, rows) -> torch.Tensor:
    L = _lib.load()
    n, dim = X.shape
    nq = (rows if rows is not None else queries).shape[0]
    out = torch.empty((nq, n), dtype=torch.float32, device=X.device)
    if n == 0 or nq == 0:
        return out
    ws = _dense.workspace(L.n2v_knn_workspace_bytes, n, dim, nq, 0, device=X.device)
    _lib.check(L.n2v_knn_scores(X.data_ptr(), inv_norm.data_ptr(), n, dim, _dense.ptr(queries), _dense.ptr(rows), nq,
                                out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
               "n2v_knn_scores")
    return out


def scores(X: torch.Tensor, queries=None, rows=None, restrict: Optional[int] = None,
           inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every score, fp32 [n_queries, n'] (n' = min(n, restrict)): most_similar's `dists` for topn=None.
    Bit for bit the scores knn() selects from."""
    X, inv_norm, queries, rows = _inputs(X, queries, rows, restrict, inv_norm)
    with torch.cuda.device(X.device):
        nq = (rows if rows is not None else queries).shape[0]
        step = max(1, min(WORKSPACE_LIMIT // max(4 * X.shape[0], 1), (1 << 20) - 16))
        parts = [_scores(X, inv_norm, None if queries is None else queries[i:i + step],
                         None if rows is None else rows[i:i + step]) for i in range(0, nq, step)]
    return torch.cat(parts) if len(parts) != 1 else parts[0]


def _topk_fused(X, inv_norm, queries, rows, k):
    L = _lib.load()
    n, dim = X.shape
    nq = (rows if rows is not None else queries).shape[0]

    def launch(i, j, ws, out_r, out_s):
        q = None if queries is None else queries[i:j]
        r = None if rows is None else rows[i:j]
        _lib.check(L.n2v_knn_topk(X.data_ptr(), inv_norm.data_ptr(), n, dim, _dense.ptr(q), _dense.ptr(r), j - i, k,
                                  out_r[i:j].data_ptr(), out_s[i:j].data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.current_stream_ptr()), "n2v_knn_topk")

    return _dense.topk_batches(lambda count: L.n2v_knn_workspace_bytes(n, dim, count, k), launch, nq, k, X.device,
                               empty=n == 0)


def _topk_sorted(X, inv_norm, queries, rows, k):
    """k above the fused limit: full scores in batches, a stable descending sort (ties: row ascending).
    A NaN score is absent, as in the fused kernel: it sorts last and leaves (-1, -inf)."""
    n = X.shape[0]
    nq = (rows if rows is not None else queries).shape[0]
    out_r = torch.full((nq, k), -1, dtype=torch.int64, device=X.device)
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=X.device)
    keep = min(k, n)
    # scores, sorted scores and int64 indices; n2v_knn_scores takes at most 65 535 x 16 queries
    step = max(1, min(WORKSPACE_LIMIT // max(16 * n, 1), (1 << 20) - 16))
    for i in range(0, nq, step):
        j = min(nq, i + step)
        s = _scores(X, inv_norm, None if queries is None else queries[i:j], None if rows is None else rows[i:j])
        # no real score is -inf (a row's norm is finite or its inv_norm 0), so -inf marks the absent
        s = s.masked_fill_(torch.isnan(s), float("-inf"))
        s, idx = torch.sort(s, dim=1, descending=True, stable=True)
        s, idx = s[:, :keep], idx[:, :keep]
        out_r[i:j, :keep] = idx.masked_fill_(s == float("-inf"), -1)
        out_s[i:j, :keep] = s
    return out_r, out_s


def knn(X: torch.Tensor, k: int, queries=None, rows=None, restrict: Optional[int] = None,
        inv_norm: Optional[torch.Tensor] = None, exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k rows of X nearest to every query by cosine: (rows int64 [nq, k], scores fp32 [nq, k]), by score
    descending, then row ascending; where fewer than k rows exist the tail is row -1, score -inf.

    queries: [nq, dim] (or [dim]) vectors, or rows: [nq] row numbers of X -- exactly one.  restrict: only rows
    [0, restrict) are candidates (gensim's restrict_vocab).  inv_norm: inv_norms(X), cached by the caller.
    exclude_self (rows= only): a query's own row is not returned (k + 1 are asked for).

    Non-finite input: a row or query holding inf or NaN scores NaN, and a NaN score is never selected, for
    every k -- such rows are left out like absent ones, so the tail may start early (row -1, score -inf).
    scores() returns the NaN itself."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if exclude_self and rows is None:
        raise ValueError("exclude_self needs rows=")
    X, inv_norm, queries, qrows = _inputs(X, queries, rows, restrict, inv_norm)
    self_rows = None
    if exclude_self:
        self_rows = torch.as_tensor(rows, device=X.device).to(torch.int64).reshape(-1)
    want = k + 1 if exclude_self else k
    with torch.cuda.device(X.device):
        pick = _topk_fused if want <= MAX_FUSED_K else _topk_sorted
        out_r, out_s = pick(X, inv_norm, queries, qrows, want)
    if not exclude_self:
        return out_r, out_s
    return _dense.drop_self(out_r, out_s, self_rows, k)
