"""Approximate nearest neighbours by cosine over trained vectors: an inverted-file (IVF-flat) index on the GPU
(csrc/n2v_ivf.hip).

The rows of X are cut into nlist lists, the cells of a spherical k-means (cluster.kmeans(metric="cosine")), and a
query scans only the nprobe lists whose centroids are nearest to it.  "Approximate" is which lists are probed and
nothing else: every score is similarity.knn's, bit for bit, and the result is the exact top k (score descending,
then row ascending) of the probed lists' rows -- with every list probed it IS similarity.knn's result (DESIGN.md
"Approximate nearest neighbours").  The index holds no copy of X: two integer arrays (list_off, row_ids) and the
centroids.

build_pq() adds product-quantised codes to an index (IVF-PQ, csrc/n2v_ivfpq.hip; DESIGN.md "Product-quantised
codes"): m bytes per listed row instead of the row, so that search_pq() needs no X at all -- its scores are
approximations (a table look-up per byte), made exact again for the best few by refine=.

Device tensors in and out.  There is no CPU path (layout() alone is plain torch): a missing GPU or library raises.
"""
import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
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


def probe(index: IVFIndex, queries=None, rows=None, X: Optional[torch.Tensor] = None,
          inv_norm: Optional[torch.Tensor] = None, nprobe: Optional[int] = None) -> torch.Tensor:
    """int32 [nq, nprobe]: for every query the nprobe lists whose centroids are nearest by cosine -- similarity.knn
    over the centroids, so score descending, then list number ascending, and the probes of a smaller nprobe are a
    prefix of those of a larger one.  A query no centroid scores (a NaN query) gets -1.  rows= are rows of X, which
    must then be given; inv_norm is accepted as search() accepts it and not needed: knn normalises the queries."""
    nprobe = _nprobe(index, nprobe)
    if (queries is None) == (rows is None):
        raise ValueError("give exactly one of queries= / rows=")
    if rows is None:  # the vectors as they are: knn normalises them itself
        q = _dense.queries(queries, index.centroids.shape[1], index.centroids.device)
    elif X is None:
        raise ValueError("rows= needs X")
    else:
        q = X[_dense.rows(rows, X.shape[0], X.device)].contiguous()
    lists, _ = similarity.knn(index.centroids, nprobe, queries=q, inv_norm=index.centroid_inv_norm)
    return lists.to(torch.int32)


def plan(n: int, dim: int, nlist: int, max_list_rows: int, n_queries: int, nprobe: int, k: int) -> Tuple[int, int, int]:
    """n2v_ivf_plan: ((query, probe) pairs per tile, rows per chunk of a list, chunks per list); ValueError for
    sizes n2v_ivf_topk refuses"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load().n2v_ivf_plan(n, dim, nlist, max_list_rows, n_queries, nprobe, k, out), "n2v_ivf_plan")
    return int(out[0]), int(out[1]), int(out[2])


def _scan(name, need, launch, nq, k, device, empty):
    """_dense.topk_batches for the two scans of an index: at most 2^20 - 1 queries a launch, and the status word
    launch(i, j, ws, out_r, out_s, status) hands to the library, read once after the last launch"""
    status = []  # made before the first launch: an empty problem has none and reads nothing

    def run(*args):
        if not status:
            status.append(torch.zeros(1, dtype=torch.int32, device=device))
        launch(*args, status[0])

    out = _dense.topk_batches(need, run, nq, k, device, max_step=(1 << 20) - 1, empty=empty)
    if status and int(status[0]) & _lib.ST_RANGE:
        raise ValueError(f"{name}: a list longer than max_list_rows, a probe outside [-1, nlist), a list that a "
                         "query's probes name twice, or a row id outside [0, n): the index does not belong to "
                         "these arguments")
    return out


def _topk(X, inv_norm, index, queries, rows, probes, k):
    L = _lib.load()
    n, dim = X.shape
    nq, nprobe = probes.shape
    sizes = (n, dim, index.nlist, index.max_list_rows)

    def need(count):
        return int(L.n2v_ivf_workspace_bytes(*sizes, count, nprobe, k))

    def launch(i, j, ws, out_r, out_s, status):
        q = None if queries is None else queries[i:j]
        r = None if rows is None else rows[i:j]
        _lib.check(L.n2v_ivf_topk(X.data_ptr(), inv_norm.data_ptr(), n, dim, index.list_off.data_ptr(),
                                  index.row_ids.data_ptr(), index.nlist, index.max_list_rows, _dense.ptr(q),
                                  _dense.ptr(r), j - i, probes[i:j].data_ptr(), nprobe, k, out_r[i:j].data_ptr(),
                                  out_s[i:j].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.current_stream_ptr()), "n2v_ivf_topk")

    return _scan("n2v_ivf_topk", need, launch, nq, k, X.device, n == 0)


def _front(kind, index, k, refine, queries, rows, X, inv_norm, probes, exclude_self):
    """What search (kind IVFIndex) and search_pq (kind IVFPQIndex) check before they scan, in the order they
    promise their errors in: (k, k + exclude_self, X, inv_norm, queries, rows, probes), the last three as the
    library takes them (probes None: the caller finds them).  Only search_pq may go without X."""
    k, refine, pq = int(k), int(refine), kind is IVFPQIndex
    if k < 1:
        raise ValueError("k must be >= 1")
    if refine < 0:
        raise ValueError("refine must be >= 0")
    if exclude_self and rows is None:
        raise ValueError("exclude_self needs rows=")
    want = k + 1 if exclude_self else k
    if want > MAX_K:
        raise ValueError(f"k = {k}{' + 1 (exclude_self)' if exclude_self else ''} is above the index's limit of "
                         f"{MAX_K}: similarity.knn serves larger k exactly")
    if not isinstance(index, kind):
        raise ValueError(f"index must be an {kind.__name__} (ann.{'build_pq' if pq else 'build_index'})")
    if pq:
        if (queries is None) == (rows is None):
            raise ValueError("give exactly one of queries= / rows=")
        if X is None and rows is not None:
            raise ValueError("rows= needs X")
        if X is None and refine > 0:
            raise ValueError("refine > 0 needs X: the exact scores are computed from its rows")
    if X is not None or not pq:
        n, dim = _dense.shape(X)
        if (n, dim) != (index.n, index.dim):
            raise ValueError(f"the index was built on a [{index.n}, {index.dim}] matrix, not [{n}, {dim}]")
        X, inv_norm, queries, rows = similarity._inputs(X, queries, rows, None, inv_norm)
    else:
        queries, rows, inv_norm = _dense.queries(queries, index.dim, index.codes.device), None, None
    if probes is not None:
        nq = (rows if rows is not None else queries).shape[0]
        probes = torch.as_tensor(probes, device=index.codes.device if pq else X.device)
        if probes.ndim != 2 or probes.shape[0] != nq or not 1 <= probes.shape[1] <= index.nlist:
            raise ValueError(f"probes must be [{nq}, 1 .. {index.nlist}]")
        probes = probes.to(torch.int32).contiguous()
    return k, want, X, inv_norm, queries, rows, probes


def search(X: torch.Tensor, index: IVFIndex, k: int, queries=None, rows=None, nprobe: Optional[int] = None,
           probes: Optional[torch.Tensor] = None, inv_norm: Optional[torch.Tensor] = None,
           exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity.knn's contract over the rows of the probed lists: (rows int64 [nq, k], scores fp32 [nq, k]), by
    score descending, then row ascending; where fewer than k candidates exist the tail is row -1, score -inf; a NaN
    score is never selected.  X: the matrix the index was built on.  nprobe: lists per query (default: the index's);
    probes: int32 [nq, nprobe'] of list numbers (-1: unused; a list a query names twice: ValueError, found on the
    device and raised after the scan like a probe out of range) instead of probe()'s.
    exclude_self (rows= only): a query's own row is not returned (k + 1 are asked for).  k + exclude_self <= 128."""
    k, want, X, inv_norm, queries, qrows, probes = _front(IVFIndex, index, k, 0, queries, rows, X, inv_norm, probes,
                                                          exclude_self)
    with torch.cuda.device(X.device):
        if probes is None:
            probes = probe(index, queries=queries, rows=qrows, X=X, nprobe=nprobe)
        out_r, out_s = _topk(X, inv_norm, index, queries, qrows, probes, want)
    return _dense.drop_self(out_r, out_s, qrows, k) if exclude_self else (out_r, out_s)


# ---- product-quantised codes (IVF-PQ) -------------------------------------------------------------------------------

PQ_MAX_M = 64         # sub-quantisers at most
PQ_CODEWORDS = 256    # per sub-space: 8-bit codes
PQ_TRAIN_ROWS = 65536


def code_stride(m: int) -> int:
    """bytes from one row of IVFPQIndex.codes to the next: m rounded up to 4, 8, 16, 32 or 64, so that the scan
    reads a row with aligned 4-, 8- or 16-byte loads (n2v_ivfpq_plan's fifth number)"""
    return next(s for s in (4, 8, 16, 32, 64) if m <= s)


class IVFPQIndex(IVFIndex):
    """An IVFIndex with product-quantised codes: `codebooks` fp32 [m, 256, dsub] (dsub = ceil(dim / m), the last
    sub-space zero-padded), `codes` uint8 [len(row_ids), code_stride(m)] -- row p holds the m codes of row
    row_ids[p], the bytes past m are 0 -- `m`, `dsub`, and `refine`, what KeyedVectors passes to search_pq.  It
    does not hold X: search_pq(refine=0) with queries= runs from the index alone."""

    def __init__(self, base: IVFIndex, codebooks, codes, m: int, dsub: int, refine: int = 0):
        super().__init__(base.centroids, base.centroid_inv_norm, base.list_off, base.row_ids, base.max_list_rows,
                         base.n, base.dim, base.nprobe)
        self.codebooks = codebooks
        self.codes = codes
        self.m = int(m)
        self.dsub = int(dsub)
        self.refine = int(refine)


def _check_m(m, dim: int) -> int:
    m = int(m)
    if not 1 <= m <= min(dim, PQ_MAX_M):
        raise ValueError(f"m = {m} outside [1, min(dim, {PQ_MAX_M})] = [1, {min(dim, PQ_MAX_M)}]")
    return m


def _residuals(X, inv_norm, index: IVFIndex, positions: torch.Tensor, width: int) -> torch.Tensor:
    """fp32 [len(positions), width]: x_hat - c_hat of the rows at these positions of row_ids (x_hat = x * inv_norm,
    c_hat the unit centroid of the position's list), zeros past dim"""
    rows = index.row_ids[positions].long()
    lists = torch.searchsorted(index.list_off, positions, right=True) - 1
    out = torch.zeros((positions.shape[0], width), dtype=torch.float32, device=X.device)
    out[:, :index.dim] = X[rows] * inv_norm[rows][:, None] - index.centroids[lists]
    return out


def _pq_inputs(X, index, m, inv_norm):
    X = _dense.matrix(X)
    n, dim = X.shape
    if not isinstance(index, IVFIndex):
        raise ValueError("index must be an IVFIndex (ann.build_index)")
    if (n, dim) != (index.n, index.dim):
        raise ValueError(f"the index was built on a [{index.n}, {index.dim}] matrix, not [{n}, {dim}]")
    return X, _check_m(m, dim), _dense.norms(X, inv_norm)


def pq_train(X: torch.Tensor, index: IVFIndex, m: int, seed: int = 0, train_rows: Optional[int] = None,
             inv_norm: Optional[torch.Tensor] = None, **kmeans_kw) -> torch.Tensor:
    """build_pq's first half: the codebooks, fp32 [m, 256, ceil(dim / m)]"""
    if train_rows is not None and int(train_rows) < 1:
        raise ValueError("train_rows must be >= 1")
    X, m, inv_norm = _pq_inputs(X, index, m, inv_norm)
    dsub = -(-index.dim // m)
    n_listed = int(index.row_ids.shape[0])
    codebooks = torch.zeros((m, PQ_CODEWORDS, dsub), dtype=torch.float32, device=X.device)
    if n_listed == 0:
        return codebooks
    with torch.cuda.device(X.device):
        take = min(n_listed, PQ_TRAIN_ROWS if train_rows is None else int(train_rows))
        picked = np.sort(np.random.default_rng(seed).choice(n_listed, size=take, replace=False))
        if take < PQ_CODEWORDS:
            picked = np.tile(picked, -(-PQ_CODEWORDS // take))[:PQ_CODEWORDS]
        train = _residuals(X, inv_norm, index, torch.from_numpy(picked).to(X.device), m * dsub)
        for j in range(m):
            sub = train[:, j * dsub:(j + 1) * dsub].contiguous()
            codebooks[j] = cluster.kmeans(sub, PQ_CODEWORDS, metric="euclidean", seed=seed + j, **kmeans_kw).centroids
    return codebooks


def pq_encode(X: torch.Tensor, index: IVFIndex, codebooks: torch.Tensor,
              inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """build_pq's second half: the codes, uint8 [len(row_ids), code_stride(m)], of every listed row under these
    codebooks"""
    X, m, inv_norm = _pq_inputs(X, index, codebooks.shape[0] if codebooks.ndim == 3 else 0, inv_norm)
    dsub = -(-index.dim // m)
    if tuple(codebooks.shape) != (m, PQ_CODEWORDS, dsub):
        raise ValueError(f"codebooks must be [m, {PQ_CODEWORDS}, {dsub}]")
    n_listed = int(index.row_ids.shape[0])
    codes = torch.zeros((n_listed, code_stride(m)), dtype=torch.uint8, device=X.device)
    # a slab: the gathered rows, their residuals and one sub-matrix
    slab = max(1, similarity.WORKSPACE_LIMIT // (4 * (index.dim + m * dsub + dsub)))
    with torch.cuda.device(X.device):
        for lo in range(0, n_listed, slab):
            hi = min(n_listed, lo + slab)
            res = _residuals(X, inv_norm, index, torch.arange(lo, hi, device=X.device), m * dsub)
            for j in range(m):
                labels, _ = cluster.assign(res[:, j * dsub:(j + 1) * dsub].contiguous(), codebooks[j], "euclidean")
                codes[lo:hi, j] = labels.clamp(min=0).to(torch.uint8)
    return codes


def build_pq(X: torch.Tensor, index: IVFIndex, m: int, seed: int = 0, train_rows: Optional[int] = None,
             inv_norm: Optional[torch.Tensor] = None, **kmeans_kw) -> IVFPQIndex:
    """`index` (of X) with product-quantised codes of its listed rows.  The residual of a listed row, x * inv_norm
    minus its list's unit centroid, is cut into m sub-vectors of dsub = ceil(dim / m) dims (the last zero-padded),
    and sub-vector j is stored as the number of its nearest codeword among 256.

    Training (pq_train): min(n_listed, train_rows or 65 536) positions of row_ids drawn without replacement from
    numpy.random.default_rng(seed), ascending; per sub-space cluster.kmeans(residuals[:, j dsub:(j + 1) dsub], 256,
    metric="euclidean", seed=seed + j, **kmeans_kw).  Fewer than 256 training rows are repeated up to 256, so spare
    codewords are copies of used ones: a copy never wins a tie against the lower code.  Encoding (pq_encode): slabs
    of positions bounded by similarity.WORKSPACE_LIMIT, cluster.assign per sub-space; the codes ARE its labels (its
    tie rule: the lowest code).  A row in no list has no code.  A label of -1 (a non-finite sub-vector of a row listed
    by from_labels) is stored as code 0: the row's approximate scores are then finite, whatever the tables give, and
    mean nothing; refine >= 1 drops it again (its exact score is NaN).  The same call gives the same index, bit for
    bit."""
    if train_rows is not None and int(train_rows) < 1:
        raise ValueError("train_rows must be >= 1")
    X, m, inv_norm = _pq_inputs(X, index, m, inv_norm)
    codebooks = pq_train(X, index, m, seed, train_rows, inv_norm, **kmeans_kw)
    return IVFPQIndex(index, codebooks, pq_encode(X, index, codebooks, inv_norm), m, codebooks.shape[2])


def plan_pq(n: int, dim: int, m: int, nlist: int, max_list_rows: int, n_queries: int, nprobe: int,
            k: int) -> Tuple[int, int, int, int, int]:
    """n2v_ivfpq_plan: ((query, probe) pairs per tile, positions per chunk of a list, chunks per list, bytes of LDS
    of a scan block, bytes per row of codes); ValueError for sizes n2v_ivfpq_topk refuses"""
    out = (C.c_int64 * 5)()
    _lib.check(_lib.load().n2v_ivfpq_plan(n, dim, m, nlist, max_list_rows, n_queries, nprobe, k, out),
               "n2v_ivfpq_plan")
    return tuple(int(v) for v in out)


def pq_lut(codebooks: torch.Tensor, dim: int, queries=None, rows=None, X: Optional[torch.Tensor] = None,
           inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """n2v_ivfpq_lut: fp32 [nq, m, 256], lut[q][j][c] = q_hat_j . w_j[c] -- the tables search_pq sums from.
    queries: [nq, dim] vectors, or rows: row numbers of X (then X, and inv_norm unless it is to be computed)."""
    L = _lib.load()
    codebooks = codebooks.to(torch.float32).contiguous()
    m = _check_m(codebooks.shape[0], dim)
    if codebooks.ndim != 3 or tuple(codebooks.shape[1:]) != (PQ_CODEWORDS, -(-dim // m)):
        raise ValueError(f"codebooks must be [m, {PQ_CODEWORDS}, ceil({dim} / m)]")
    if (queries is None) == (rows is None):
        raise ValueError("give exactly one of queries= / rows=")
    n = 0
    if rows is not None:
        if X is None:
            raise ValueError("rows= needs X")
        X, inv_norm, _, rows = similarity._inputs(X, None, rows, None, inv_norm)
        n = X.shape[0]
    else:
        queries = _dense.queries(queries, dim, codebooks.device)
    nq = (rows if rows is not None else queries).shape[0]
    out = torch.empty((nq, m, PQ_CODEWORDS), dtype=torch.float32, device=codebooks.device)
    if nq == 0:
        return out
    with torch.cuda.device(codebooks.device):
        ws = _dense.workspace(L.n2v_ivfpq_workspace_bytes, n, dim, m, 1, 1, nq, 1, 0, device=codebooks.device)
        _lib.check(L.n2v_ivfpq_lut(_dense.ptr(X if rows is not None else None),
                                   _dense.ptr(inv_norm if rows is not None else None), n, dim, _dense.ptr(queries),
                                   _dense.ptr(rows), nq, codebooks.data_ptr(), m, out.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _lib.current_stream_ptr()), "n2v_ivfpq_lut")
    return out


def _pq_topk(index: IVFPQIndex, X, inv_norm, queries, rows, probes, coarse, k):
    L = _lib.load()
    nq, nprobe = probes.shape
    sizes = (index.n, index.dim, index.m, index.nlist, index.max_list_rows)

    def need(count):
        return int(L.n2v_ivfpq_workspace_bytes(*sizes, count, nprobe, k))

    def launch(i, j, ws, out_r, out_s, status):
        q = None if queries is None else queries[i:j]
        r = None if rows is None else rows[i:j]
        _lib.check(L.n2v_ivfpq_topk(index.codes.data_ptr(), index.codebooks.data_ptr(), index.m, _dense.ptr(X),
                                    _dense.ptr(inv_norm), index.n, index.dim, index.list_off.data_ptr(),
                                    index.row_ids.data_ptr(), index.nlist, index.max_list_rows, _dense.ptr(q),
                                    _dense.ptr(r), j - i, probes[i:j].data_ptr(), coarse[i:j].data_ptr(), nprobe, k,
                                    out_r[i:j].data_ptr(), out_s[i:j].data_ptr(), status.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _lib.current_stream_ptr()), "n2v_ivfpq_topk")

    return _scan("n2v_ivfpq_topk", need, launch, nq, k, index.codes.device,
                 index.n == 0 or index.codes.shape[0] == 0)


def _rerank(X, inv_norm, queries, rows, cand: torch.Tensor, k: int):
    """the k best of every query's candidates (int64 [nq, c], -1: none) by similarity.knn's own scores: n2v_ivf_topk
    over one "list" per query, at most 1024 queries (lists) a launch"""
    n, dim = X.shape
    nq = cand.shape[0]
    out_r = torch.full((nq, k), -1, dtype=torch.int64, device=X.device)
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=X.device)
    for i in range(0, nq, MAX_LISTS):
        j = min(nq, i + MAX_LISTS)
        part = cand[i:j]
        have = part >= 0
        list_off = torch.zeros(j - i + 1, dtype=torch.int64, device=X.device)
        list_off[1:] = torch.cumsum(have.sum(dim=1), 0)
        ids = torch.cat([part[have], part.new_zeros(1)]).to(torch.int32)  # never empty: one entry no list holds
        lists = IVFIndex(torch.empty((j - i, 0)), None, list_off, ids, max(1, min(cand.shape[1], n)), n, dim, 1)
        probes = torch.arange(j - i, dtype=torch.int32, device=X.device)[:, None].contiguous()
        out_r[i:j], out_s[i:j] = _topk(X, inv_norm, lists, None if queries is None else queries[i:j],
                                       None if rows is None else rows[i:j], probes, k)
    return out_r, out_s


def search_pq(index: IVFPQIndex, k: int, queries=None, rows=None, X: Optional[torch.Tensor] = None,
              nprobe: Optional[int] = None, probes: Optional[torch.Tensor] = None, refine: int = 0,
              inv_norm: Optional[torch.Tensor] = None, exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rows int64 [nq, k], scores fp32 [nq, k]) over the product-quantised codes of the probed lists, best first, the
    tail (-1, -inf).

    refine = 0: the approximate result.  The score of a listed row is the query's score against its list's
    centroid plus m table entries (n2v_ivfpq_topk), ordered by score descending, then row ascending.  X is needed
    only with rows=, to fetch the query vectors.  The centroid scores are the probe's own (similarity.knn over the
    centroids), or with probes= (int32 [nq, nprobe'], -1: unused; a list a query names twice: ValueError, as in
    search) similarity.scores over the centroids, gathered.
    refine = f >= 1 (X required): the min(128, f * k') best by approximate score (k' = k + exclude_self) are scored
    again with similarity.knn's scores, bit for bit, and the k best by (exact score descending, row ascending)
    returned -- a NaN score is dropped there.  exclude_self (rows= only): a query's own row is not returned.
    k + exclude_self <= 128."""
    k, want, X, inv_norm, queries, qrows, probes = _front(IVFPQIndex, index, k, refine, queries, rows, X, inv_norm,
                                                          probes, exclude_self)
    refine = int(refine)
    with torch.cuda.device(index.codes.device):
        qvec = queries if qrows is None else X[qrows].contiguous()
        if probes is None:
            probes, coarse = similarity.knn(index.centroids, _nprobe(index, nprobe), queries=qvec,
                                            inv_norm=index.centroid_inv_norm)
            probes = probes.to(torch.int32)
        else:
            every = similarity.scores(index.centroids, queries=qvec, inv_norm=index.centroid_inv_norm)
            coarse = torch.gather(every, 1, probes.long().clamp(0, index.nlist - 1))
        coarse = coarse.to(torch.float32).contiguous()
        first = want if refine == 0 else min(MAX_K, max(want, refine * want))
        out_r, out_s = _pq_topk(index, X if qrows is not None else None, inv_norm if qrows is not None else None,
                                queries, qrows, probes, coarse, first)
        if refine > 0:
            out_r, out_s = _rerank(X, inv_norm, queries, qrows, out_r, want)
    return _dense.drop_self(out_r, out_s, qrows, k) if exclude_self else (out_r, out_s)
