"""Approximate nearest neighbours by cosine over trained vectors: an inverted-file (IVF-flat) index on the GPU
(csrc/n2v_ivf.hip).

The rows of X are cut into nlist lists, the cells of a spherical k-means (cluster.kmeans(metric="cosine")), and a
query scans only the nprobe lists whose centroids are nearest to it.  "Approximate" is which lists are probed and
nothing else: every score is similarity.knn's, bit for bit, and the result is the exact top k (score descending,
then row ascending) of the probed lists' rows -- with every list probed it IS similarity.knn's result (DESIGN.md
"Approximate nearest neighbours").  The index holds no copy of X: two integer arrays (list_off, row_ids) and the
centroids.

Device tensors in and out.  There is no CPU path (layout() alone is plain torch): a missing GPU or library raises.
"""
import ctypes as C
import math
from typing import Optional, Tuple

import torch

from node2vec_amd import _dense, _lib, cluster, similarity

MAX_LISTS = cluster.MAX_K
MAX_K = 128  # n2v_ivf_topk's limit; larger k are similarity.knn's


def layout(labels: torch.Tensor, nlist: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(list_off int64 [nlist + 1], row_ids int32): list l is row_ids[list_off[l]:list_off[l + 1]], the rows whose
    label is l in ascending order (a stable sort by label).  A label outside [0, nlist) -- k-means' -1 -- puts its
    row in no list.  Plain torch, on the labels' device."""
    nlist = int(nlist)
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.dtype.is_floating_point:
        raise ValueError("labels must be a 1-D integer tensor")
    if nlist < 1:
        raise ValueError("nlist must be >= 1")
    if labels.shape[0] >= 1 << 31:
        raise ValueError("at most 2^31 - 1 rows")
    labels = labels.to(torch.int64)
    rows = torch.nonzero((labels >= 0) & (labels < nlist)).reshape(-1)
    kept = labels[rows]
    order = torch.sort(kept, stable=True)[1]
    list_off = torch.zeros(nlist + 1, dtype=torch.int64, device=labels.device)
    list_off[1:] = torch.cumsum(torch.bincount(kept, minlength=nlist), 0)
    return list_off, rows[order].to(torch.int32)


class IVFIndex:
    """An inverted-file index over one matrix X [n, dim] (which it does not hold): `centroids` fp32 [nlist, dim]
    (unit vectors) with `centroid_inv_norm`, `list_off` int64 [nlist + 1] and `row_ids` int32 (layout()),
    `max_list_rows` (the longest list, read once when the index is built), `n`, `dim`, and `nprobe`, the number of
    lists a query scans unless the call says otherwise (settable, 1 .. nlist)."""

    def __init__(self, centroids, centroid_inv_norm, list_off, row_ids, max_list_rows: int, n: int, dim: int,
                 nprobe: int):
        self.centroids = centroids
        self.centroid_inv_norm = centroid_inv_norm
        self.list_off = list_off
        self.row_ids = row_ids
        self.max_list_rows = int(max_list_rows)
        self.n = int(n)
        self.dim = int(dim)
        self.nprobe = max(1, min(int(nprobe), self.nlist))

    @property
    def nlist(self) -> int:
        return int(self.centroids.shape[0])


def _index(X, unit_centroids, labels, nprobe) -> IVFIndex:
    n, dim = X.shape
    if int(nprobe) < 1:
        raise ValueError("nprobe must be >= 1")
    list_off, row_ids = layout(labels.to(X.device), unit_centroids.shape[0])
    longest = int((list_off[1:] - list_off[:-1]).max())  # the one read of the build
    return IVFIndex(unit_centroids, similarity.inv_norms(unit_centroids), list_off, row_ids.contiguous(),
                    max(longest, 1), n, dim, nprobe)


def from_labels(X: torch.Tensor, centroids: torch.Tensor, labels: torch.Tensor, nprobe: int = 8) -> IVFIndex:
    """The index of a clustering the caller already has: `centroids` [nlist, dim] (normalised here) and one label per
    row of X (a label outside [0, nlist): the row is in no list and is never found)."""
    X = _dense.matrix(X)
    n, dim = X.shape
    centroids = cluster._centroids(centroids, None, dim).to(device=X.device, dtype=torch.float32).contiguous()
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError(f"labels must be a [{n}] tensor")
    return _index(X, cluster._unit(centroids), labels, nprobe)


def build_index(X: torch.Tensor, nlist: Optional[int] = None, nprobe: int = 8, seed: int = 0,
                inv_norm: Optional[torch.Tensor] = None, **kmeans_kw) -> IVFIndex:
    """The index of X: cluster.kmeans(X, nlist, metric="cosine", seed=seed, **kmeans_kw) as it stands -- its
    centroids and labels, untouched -- then layout().  nlist=None: min(1024, max(1, round(sqrt(n)))); nprobe is
    clipped to nlist.  The same call gives the same index, bit for bit (k-means' own promise).  A row k-means left
    unassigned (a non-finite row) is in no list."""
    X = _dense.matrix(X)
    n = X.shape[0]
    if nlist is None:
        nlist = min(MAX_LISTS, max(1, round(math.sqrt(n))))
    res = cluster.kmeans(X, int(nlist), metric="cosine", seed=seed, inv_norm=inv_norm, **kmeans_kw)
    return _index(X, res.centroids, res.labels, nprobe)


def _nprobe(index: IVFIndex, nprobe) -> int:
    nprobe = index.nprobe if nprobe is None else int(nprobe)
    if nprobe < 1:
        raise ValueError("nprobe must be >= 1")
    return min(nprobe, index.nlist)


def _query_vectors(index, queries, rows, X):
    """unit-free query vectors [nq, dim] for the centroid search (knn normalises them itself)"""
    if (queries is None) == (rows is None):
        raise ValueError("give exactly one of queries= / rows=")
    if rows is not None:
        if X is None:
            raise ValueError("rows= needs X")
        rows = torch.as_tensor(rows, device=X.device).to(torch.int64).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= X.shape[0]):
            raise IndexError("query row outside [0, n)")
        return X[rows].contiguous()
    queries = torch.as_tensor(queries, device=index.centroids.device)
    return queries[None] if queries.ndim == 1 else queries


def probe(index: IVFIndex, queries=None, rows=None, X: Optional[torch.Tensor] = None,
          inv_norm: Optional[torch.Tensor] = None, nprobe: Optional[int] = None) -> torch.Tensor:
    """int32 [nq, nprobe]: for every query the nprobe lists whose centroids are nearest by cosine -- similarity.knn
    over the centroids, so score descending, then list number ascending, and the probes of a smaller nprobe are a
    prefix of those of a larger one.  A query no centroid scores (a NaN query) gets -1.  rows= are rows of X, which
    must then be given; inv_norm is accepted as search() accepts it and not needed: knn normalises the queries."""
    nprobe = _nprobe(index, nprobe)
    q = _query_vectors(index, queries, rows, X)
    lists, _ = similarity.knn(index.centroids, nprobe, queries=q, inv_norm=index.centroid_inv_norm)
    return lists.to(torch.int32)


def plan(n: int, dim: int, nlist: int, max_list_rows: int, n_queries: int, nprobe: int, k: int) -> Tuple[int, int, int]:
    """n2v_ivf_plan: ((query, probe) pairs per tile, rows per chunk of a list, chunks per list); ValueError for
    sizes n2v_ivf_topk refuses"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load().n2v_ivf_plan(n, dim, nlist, max_list_rows, n_queries, nprobe, k, out), "n2v_ivf_plan")
    return int(out[0]), int(out[1]), int(out[2])


def _topk(X, inv_norm, index, queries, rows, probes, k):
    L = _lib.load()
    n, dim = X.shape
    nq, nprobe = probes.shape
    out_r = torch.full((nq, k), -1, dtype=torch.int64, device=X.device)
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=X.device)
    if n == 0 or nq == 0:
        return out_r, out_s
    sizes = (n, dim, index.nlist, index.max_list_rows)

    def need(count):
        return int(L.n2v_ivf_workspace_bytes(*sizes, count, nprobe, k))

    step = min(nq, (1 << 20) - 1)  # queries per launch: the workspace stays under WORKSPACE_LIMIT
    while step > 1 and not 0 <= need(step) <= similarity.WORKSPACE_LIMIT:
        step = (step + 1) // 2
    status = torch.zeros(1, dtype=torch.int32, device=X.device)
    for i in range(0, nq, step):
        j = min(nq, i + step)
        ws = _dense.workspace(L.n2v_ivf_workspace_bytes, *sizes, j - i, nprobe, k, device=X.device)
        q = None if queries is None else queries[i:j]
        r = None if rows is None else rows[i:j]
        _lib.check(L.n2v_ivf_topk(X.data_ptr(), inv_norm.data_ptr(), n, dim, index.list_off.data_ptr(),
                                  index.row_ids.data_ptr(), index.nlist, index.max_list_rows, _dense.ptr(q),
                                  _dense.ptr(r), j - i, probes[i:j].data_ptr(), nprobe, k, out_r[i:j].data_ptr(),
                                  out_s[i:j].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.current_stream_ptr()), "n2v_ivf_topk")
    if int(status) & _lib.ST_RANGE:
        raise ValueError("n2v_ivf_topk: a list longer than max_list_rows, a probe outside [-1, nlist) or a row id "
                         "outside [0, n): the index does not belong to these arguments")
    return out_r, out_s


def search(X: torch.Tensor, index: IVFIndex, k: int, queries=None, rows=None, nprobe: Optional[int] = None,
           probes: Optional[torch.Tensor] = None, inv_norm: Optional[torch.Tensor] = None,
           exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity.knn's contract over the rows of the probed lists: (rows int64 [nq, k], scores fp32 [nq, k]), by
    score descending, then row ascending; where fewer than k candidates exist the tail is row -1, score -inf; a NaN
    score is never selected.  X: the matrix the index was built on.  nprobe: lists per query (default: the index's);
    probes: int32 [nq, nprobe'] of list numbers (-1: unused, a query's entries distinct) instead of probe()'s.
    exclude_self (rows= only): a query's own row is not returned (k + 1 are asked for).  k + exclude_self <= 128."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if exclude_self and rows is None:
        raise ValueError("exclude_self needs rows=")
    want = k + 1 if exclude_self else k
    if want > MAX_K:
        raise ValueError(f"k = {k}{' + 1 (exclude_self)' if exclude_self else ''} is above the index's limit of "
                         f"{MAX_K}: similarity.knn serves larger k exactly")
    if not isinstance(index, IVFIndex):
        raise ValueError("index must be an IVFIndex (ann.build_index)")
    n, dim = _dense.shape(X)
    if (n, dim) != (index.n, index.dim):
        raise ValueError(f"the index was built on a [{index.n}, {index.dim}] matrix, not [{n}, {dim}]")
    X, inv_norm, queries, qrows = similarity._inputs(X, queries, rows, None, inv_norm)
    nq = (qrows if qrows is not None else queries).shape[0]
    with torch.cuda.device(X.device):
        if probes is None:
            probes = probe(index, queries=queries, rows=qrows, X=X, nprobe=nprobe)
        else:
            probes = torch.as_tensor(probes, device=X.device)
            if probes.ndim != 2 or probes.shape[0] != nq or not 1 <= probes.shape[1] <= index.nlist:
                raise ValueError(f"probes must be [{nq}, 1 .. {index.nlist}]")
        probes = probes.to(torch.int32).contiguous()
        out_r, out_s = _topk(X, inv_norm, index, queries, qrows, probes, want)
    if not exclude_self:
        return out_r, out_s
    drop = out_r == qrows[:, None]
    drop[:, -1] |= ~drop.any(dim=1)  # not among the k + 1: the last one goes
    keep = ~drop
    return out_r[keep].view(-1, k), out_s[keep].view(-1, k)
