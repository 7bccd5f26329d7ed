"""k-means over trained vectors, on the GPU (csrc/n2v_kmeans.hip): the clustering of the node2vec paper's case
study (section 4.1), without copying the matrix to the host.

Lloyd's iteration with one pass over X per iteration (n2v_kmeans_step scores, assigns and sums in one launch).
"euclidean" is what the paper and scikit-learn use and is the default HERE, as in scikit-learn; "cosine" is
spherical k-means (unit centroids, rows weighted by 1 / norm) and is the default on KeyedVectors.kmeans and the
model classes, whose other queries are all cosines.  Every label, distance and centroid is computed in one fixed
order of fp32 / fp64 operations (DESIGN.md "Clustering"): the same call gives the same bits, whatever the launch.
A cluster that loses all its rows keeps its centroid (scikit-learn relocates it).  A row whose distances are all
NaN gets label -1, joins no cluster and is counted in n_unassigned.

silhouette_samples / silhouette_score (csrc/n2v_silhouette.hip; DESIGN.md "Cluster quality") say how good a
clustering is, which inertia cannot: every distance of a scored row to every other row, on the GPU, in one fixed
order as well.

dbscan / neighbor_counts (csrc/n2v_dbscan.hip; DESIGN.md "Density clustering") are the density clustering: no k to
choose, clusters of any shape, stray rows left as noise, and scikit-learn's labels exactly.

Device tensors in and out.  There is no CPU path: a missing GPU or library raises.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from node2vec_amd import _dense, _lib, similarity

METRICS = {"euclidean": _lib.KMEANS_EUCLIDEAN, "cosine": _lib.KMEANS_COSINE}
INITS = ("k-means++", "random")
MAX_K = 1024


class KMeansResult(NamedTuple):
    centroids: torch.Tensor  # fp32 [k, dim] (unit vectors for cosine)
    labels: torch.Tensor     # int32 [n], -1: unassigned
    dist: torch.Tensor       # fp32 [n]: squared Euclidean distance, or 1 - cosine, to the row's centroid
    counts: torch.Tensor     # int64 [k]
    inertia: float           # dist.double().sum() over the assigned rows
    n_iter: int
    converged: bool
    n_unassigned: int


class SilhouetteResult(NamedTuple):
    s: torch.Tensor        # fp64 [m]: (b - a) / max(a, b); NaN for a row of no cluster
    a: torch.Tensor        # fp64 [m]: mean distance to the other rows of the row's cluster
    b: torch.Tensor        # fp64 [m]: the smallest mean distance to the rows of another cluster
    nearest: torch.Tensor  # int32 [m]: that cluster, -1: none
    counts: torch.Tensor   # int64 [k]: rows per cluster


class DBSCANResult(NamedTuple):
    labels: torch.Tensor     # int32 [n]: the cluster of every row, -1: noise
    core_mask: torch.Tensor  # bool [n]: counts >= min_samples
    n_clusters: int
    counts: torch.Tensor     # int32 [n]: rows within eps of the row, itself included
    sizes: torch.Tensor      # int64 [n_clusters]: rows per cluster


def check_metric(metric: str) -> None:
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: " + " | ".join(METRICS))


def check_k(k, n: Optional[int] = None) -> int:
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError(f"k = {k} outside [1, {MAX_K}]")
    if n is not None and k > n:
        raise ValueError(f"k = {k} clusters of n = {n} rows")
    return k


def _norms(X: torch.Tensor, metric: str, inv_norm: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return _dense.norms(X, inv_norm) if metric == "cosine" else None


def _centroids(C, k: Optional[int], dim: int) -> torch.Tensor:
    """the shape of a centroid matrix, checked on the host"""
    if not isinstance(C, torch.Tensor) or C.ndim != 2 or C.shape[1] != dim or (k is not None and C.shape[0] != k):
        raise ValueError(f"centroids must be a [{'k' if k is None else k}, {dim}] tensor")
    if not 1 <= C.shape[0] <= MAX_K:
        raise ValueError(f"k = {C.shape[0]} outside [1, {MAX_K}]")
    return C


def alloc_workspace(n: int, dim: int, k: int, device) -> torch.Tensor:
    return _dense.workspace(_lib.load().n2v_kmeans_workspace_bytes, n, dim, k, device=device)


_workspace = alloc_workspace  # the name callers used before it became public


def _unit(C: torch.Tensor) -> torch.Tensor:
    return C * similarity.inv_norms(C)[:, None]


def slab_rows(n: int, dim: int, k: int) -> int:
    """rows per slab of the update's fixed order of summation (n2v_kmeans_slab_rows)"""
    return int(_lib.load().n2v_kmeans_slab_rows(n, dim, k))


def assign(X: torch.Tensor, centroids: torch.Tensor, metric: str = "euclidean",
           inv_norm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [n], dist fp32 [n]): the nearest centroid of every row (ties: the lowest index) and the
    distance to it -- squared Euclidean, or 1 - cosine against UNIT centroids (init_centroids and update return
    such).  inv_norm: similarity.inv_norms(X) for cosine, computed when not given."""
    check_metric(metric)
    n, dim = _dense.shape(X)
    _centroids(centroids, None, dim)
    X = _dense.matrix(X)
    C = centroids.to(device=X.device, dtype=torch.float32).contiguous()
    k = C.shape[0]
    norms = _norms(X, metric, inv_norm)
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    dist = torch.empty(n, dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        ws = alloc_workspace(n, dim, k, X.device)
        _lib.check(_lib.load().n2v_kmeans_assign(X.data_ptr(), _dense.ptr(norms), n, dim, C.data_ptr(), k,
                                                 METRICS[metric], labels.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _lib.current_stream_ptr()), "n2v_kmeans_assign")
    return labels, dist


def update(X: torch.Tensor, labels: torch.Tensor, k: int, metric: str, prev_centroids: torch.Tensor,
           inv_norm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(centroids fp32 [k, dim], counts int64 [k]): the mean of every cluster's rows (cosine: the unit vector of the
    sum of their unit vectors); an empty cluster keeps its row of prev_centroids.  A label outside [0, k) joins no
    cluster."""
    check_metric(metric)
    n, dim = _dense.shape(X)
    k = check_k(k)
    _centroids(prev_centroids, k, dim)
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError(f"labels must be a [{n}] tensor")
    X = _dense.matrix(X)
    prev = prev_centroids.to(device=X.device, dtype=torch.float32).contiguous()
    labels = labels.to(device=X.device, dtype=torch.int32).contiguous()
    norms = _norms(X, metric, inv_norm)
    out = prev.clone()
    counts = torch.zeros(k, dtype=torch.int64, device=X.device)
    with torch.cuda.device(X.device):
        ws = alloc_workspace(n, dim, k, X.device)
        _lib.check(_lib.load().n2v_kmeans_update(X.data_ptr(), _dense.ptr(norms), n, dim, labels.data_ptr(), k,
                                                 METRICS[metric], prev.data_ptr(), out.data_ptr(), counts.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "n2v_kmeans_update")
    return out, counts


def draw_next(D: torch.Tensor, rng: np.random.Generator, chosen) -> int:
    """k-means++'s draw: a row with probability D[row] / sum(D), by one rng.random() against the float64 running
    sum of D.  A row of D = 0 (every chosen row) cannot be drawn; when the sum is 0 the lowest row not in
    `chosen` is taken (and no random number)."""
    cum = torch.cumsum(D.to(torch.float64), 0)
    total = float(cum[-1])
    if not total > 0.0:
        taken = set(int(c) for c in chosen)
        return next(r for r in range(D.shape[0]) if r not in taken)
    u = rng.random() * total
    at = torch.searchsorted(cum, torch.tensor([u], dtype=torch.float64, device=cum.device), right=True)
    return int(at.clamp(max=D.shape[0] - 1))


def init_centroids(X: torch.Tensor, k: int, metric: str = "euclidean", seed: int = 0, init="k-means++",
                   inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """k initial centroids, fp32 [k, dim] (unit vectors for cosine), from rng = numpy.random.default_rng(seed):
    "random": k distinct rows; "k-means++" (Arthur & Vassilvitskii): the first rng.integers(n), every further one
    drawn with probability proportional to the distance to the nearest centre chosen so far (one assign pass with
    k = 1 per centre); or a [k, dim] tensor, used as it is (normalised for cosine).  The same seed gives the same
    centres."""
    check_metric(metric)
    n, dim = _dense.shape(X)
    k = check_k(k, n)
    if isinstance(init, torch.Tensor):
        _centroids(init, k, dim)
    elif init not in INITS:
        raise ValueError(f"init {init!r}: " + " | ".join(INITS) + " | a [k, dim] tensor")
    X = _dense.matrix(X)
    unit = _unit if metric == "cosine" else (lambda C: C)
    if isinstance(init, torch.Tensor):
        return unit(init.to(device=X.device, dtype=torch.float32).contiguous().clone())
    rng = np.random.default_rng(seed)
    if init == "random":
        rows = np.sort(rng.choice(n, size=k, replace=False))
        return unit(X[torch.from_numpy(rows).to(X.device)].contiguous())
    norms = _norms(X, metric, inv_norm)
    chosen = [int(rng.integers(n))]
    D = None
    for _ in range(1, k):
        centre = unit(X[chosen[-1]:chosen[-1] + 1].contiguous())
        dist = torch.nan_to_num(assign(X, centre, metric, norms)[1], nan=0.0, posinf=0.0)
        D = dist if D is None else torch.minimum(D, dist)
        D[chosen] = 0.0
        chosen.append(draw_next(D, rng, chosen))
    return unit(X[torch.tensor(chosen, device=X.device)].contiguous())


def _lloyd(X, norms, C, metric, max_iter, tol) -> KMeansResult:
    L = _lib.load()
    n, dim = X.shape
    k = C.shape[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device=X.device)
    dist = torch.empty(n, dtype=torch.float32, device=X.device)
    nxt = torch.empty_like(C)
    counts = torch.zeros(k, dtype=torch.int64, device=X.device)
    stats = torch.zeros(2, dtype=torch.int64, device=X.device)
    ws = alloc_workspace(n, dim, k, X.device)
    n_iter, settled, converged = 0, False, False
    for n_iter in range(1, max_iter + 1):
        _lib.check(L.n2v_kmeans_step(X.data_ptr(), _dense.ptr(norms), n, dim, C.data_ptr(), k, METRICS[metric],
                                     labels.data_ptr(), dist.data_ptr(), nxt.data_ptr(), counts.data_ptr(),
                                     stats.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "n2v_kmeans_step")
        shift = ((nxt - C) ** 2).sum() if tol > 0 else None
        C, nxt = nxt, C
        n_changed = int(stats[0])  # the iteration's one synchronisation
        if n_changed == 0:  # the labels of the iteration before: the update repeated itself bit for bit
            settled = converged = True
            break
        if shift is not None and float(shift) <= tol:
            converged = True
            break
    if not settled:  # labels and distances against the centroids that are returned
        _lib.check(L.n2v_kmeans_assign(X.data_ptr(), _dense.ptr(norms), n, dim, C.data_ptr(), k, METRICS[metric],
                                       labels.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.current_stream_ptr()), "n2v_kmeans_assign")
    live = labels >= 0
    counts = torch.bincount(labels[live].long(), minlength=k)
    return KMeansResult(C, labels, dist, counts, float(dist[live].double().sum()), n_iter, converged,
                        int(n - int(live.sum())))


def kmeans(X: torch.Tensor, k: int, metric: str = "euclidean", init="k-means++", n_init: int = 1, max_iter: int = 100,
           tol: float = 0.0, seed: int = 0, inv_norm: Optional[torch.Tensor] = None) -> KMeansResult:
    """Lloyd's k-means of the rows of X.  metric: "euclidean" (the default here, as in scikit-learn) or "cosine"
    (spherical; the default of KeyedVectors.kmeans and of the model classes' cluster()).  An iteration is one
    n2v_kmeans_step; it stops when no label changed (converged), when tol > 0 and the summed squared shift of the
    centres is <= tol (converged), or after max_iter iterations.  Unless it stopped on unchanged labels, one more
    assignment makes labels and dist those of the returned centroids.  n_init > 1: seeds seed, seed + 1, ...; the
    run of lowest inertia is returned (ties: the first).  One host synchronisation per iteration."""
    check_metric(metric)
    n, dim = _dense.shape(X)
    k = check_k(k, n)
    if isinstance(init, torch.Tensor):
        _centroids(init, k, dim)
    elif init not in INITS:
        raise ValueError(f"init {init!r}: " + " | ".join(INITS) + " | a [k, dim] tensor")
    if int(n_init) < 1 or int(max_iter) < 1 or not float(tol) >= 0.0:
        raise ValueError("n_init and max_iter must be >= 1 and tol >= 0")
    X = _dense.matrix(X)
    norms = _norms(X, metric, inv_norm)
    best = None
    with torch.cuda.device(X.device):
        for run in range(int(n_init)):
            C = init_centroids(X, k, metric, int(seed) + run, init, norms)
            res = _lloyd(X, norms, C, metric, int(max_iter), float(tol))
            if best is None or res.inertia < best.inertia:
                best = res
    return best


def _labels(labels, n: int, k: Optional[int]) -> Tuple[torch.Tensor, int]:
    """(labels int32 [n] where they are, k): checked on the host side of the call, before anything needs a device"""
    if isinstance(labels, KMeansResult):
        k = labels.centroids.shape[0] if k is None else k
        labels = labels.labels
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError(f"labels must be a [{n}] tensor")
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f"labels must be integers, not {labels.dtype}")
    # MAX_K is a label of no cluster whatever k is: nothing wraps on the way to int32
    labels = labels.to(torch.int64).clamp(min=-1, max=MAX_K).to(torch.int32)
    if k is None:
        k = max(int(labels.max()) + 1, 1) if n else 1
    return labels, check_k(k)


def sample_rows(labels: torch.Tensor, k: int, sample_size: Optional[int], seed: int = 0) -> Optional[torch.Tensor]:
    """silhouette_score's sample: sample_size of the rows whose label is in [0, k), without replacement, from
    numpy.random.default_rng(seed), ascending (int64, on the host); None when every such row is taken"""
    if sample_size is None:
        return None
    if int(sample_size) < 1:
        raise ValueError("sample_size must be >= 1")
    have = torch.nonzero((labels >= 0) & (labels < k))[:, 0].cpu().numpy()
    if int(sample_size) >= len(have):
        return None
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.sort(have[rng.choice(len(have), size=int(sample_size), replace=False)]))


def silhouette_samples(X: torch.Tensor, labels, metric: str = "euclidean", k: Optional[int] = None, rows=None,
                       inv_norm: Optional[torch.Tensor] = None) -> SilhouetteResult:
    """The silhouette of rows of X under a clustering (csrc/n2v_silhouette.hip): for row i of label L,
    a = the mean distance to the other rows of cluster L, b = the smallest mean distance to the rows of another
    non-empty cluster (ties: the lowest cluster), nearest = that cluster, s = (b - a) / max(a, b); s = 0 for a
    cluster of one row, for a = b = 0 and when no other cluster has rows.  The distance is the true Euclidean
    distance (scikit-learn's default; not the squared one kmeans reports) or 1 - cosine.  labels: int [n] or a
    KMeansResult; a label outside [0, k) is no cluster: the row is never counted, and scores NaN when asked for.
    k: clusters, labels.max() + 1 when not given.  rows: the rows to score (any order, repeats allowed), every row
    when not given; each is scored against ALL rows, so its values are the same bits whichever rows come with it.
    Every distance is computed: 2 m n dim FLOPs, nothing of size m x n stored.  Device tensors out."""
    check_metric(metric)
    n, dim = _dense.shape(X)
    labels, k = _labels(labels, n, k)
    if rows is not None:
        rows = torch.as_tensor(rows)
        if rows.ndim != 1 or rows.dtype.is_floating_point or rows.dtype.is_complex or rows.dtype == torch.bool:
            raise ValueError("rows must be a 1-D tensor of row numbers")
    X = _dense.matrix(X)
    labels = labels.to(X.device).contiguous()
    norms = _norms(X, metric, inv_norm)
    if rows is not None:
        rows = rows.to(device=X.device, dtype=torch.int64).contiguous()
    m = n if rows is None else int(rows.shape[0])
    a = torch.empty(m, dtype=torch.float64, device=X.device)
    b = torch.empty(m, dtype=torch.float64, device=X.device)
    s = torch.empty(m, dtype=torch.float64, device=X.device)
    nearest = torch.empty(m, dtype=torch.int32, device=X.device)
    counts = torch.zeros(k, dtype=torch.int64, device=X.device)
    with torch.cuda.device(X.device):
        ws = _dense.workspace(_lib.load().n2v_silhouette_workspace_bytes, n, dim, k, m, device=X.device)
        _lib.check(_lib.load().n2v_silhouette(X.data_ptr(), _dense.ptr(norms), n, dim, labels.data_ptr(), k,
                                              METRICS[metric], _dense.ptr(rows), m, a.data_ptr(), b.data_ptr(),
                                              s.data_ptr(), nearest.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                              ws.numel(), _lib.current_stream_ptr()), "n2v_silhouette")
    return SilhouetteResult(s, a, b, nearest, counts)


def silhouette_score(X: torch.Tensor, labels, metric: str = "euclidean", sample_size: Optional[int] = None,
                     seed: int = 0, k: Optional[int] = None, inv_norm: Optional[torch.Tensor] = None) -> float:
    """The mean silhouette (float64) over the rows that have a cluster.  sample_size: that many of those rows
    (sample_rows: without replacement, from numpy.random.default_rng(seed); all of them when there are no more),
    each scored against every row -- a sampled value is the row's exact silhouette and the cost is
    sample_size * n distances (scikit-learn scores its sample against the sample alone).  Fewer than two
    clusters with rows is a ValueError."""
    check_metric(metric)
    n, _ = _dense.shape(X)
    labels, k = _labels(labels, n, k)
    member = (labels >= 0) & (labels < k)
    if int(torch.bincount(labels[member].long(), minlength=k).count_nonzero()) < 2:
        raise ValueError("the silhouette needs at least two clusters with rows")
    rows = sample_rows(labels, k, sample_size, seed)
    res = silhouette_samples(X, labels, metric, k, rows, inv_norm)
    s = res.s if rows is not None else res.s[member.to(res.s.device)]
    return float(s.mean())


def _eps(eps) -> float:
    """eps as the kernels take it: rounded to fp32, finite and >= 0"""
    with np.errstate(over="ignore"):
        eps = float(np.float32(eps))
    if not (np.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"eps = {eps} must be finite and >= 0")
    return eps


def _finite(X: torch.Tensor) -> None:
    if not bool(torch.isfinite(X).all()):
        raise ValueError("X holds a value that is not finite")


def _count(X, norms, eps, metric, min_samples, want_core, max_blocks):
    """scan 1 -> (counts int32 [n], core bool [n] or None, the workspace for the scans that follow)"""
    n, dim = X.shape
    counts = torch.empty(n, dtype=torch.int32, device=X.device)
    core = torch.empty(n, dtype=torch.uint8, device=X.device) if want_core else None
    ws = _dense.workspace(_lib.load().n2v_dbscan_workspace_bytes, n, dim, device=X.device)
    _lib.check(_lib.load().n2v_dbscan_count(X.data_ptr(), _dense.ptr(norms), n, dim, METRICS[metric], eps,
                                            min_samples, counts.data_ptr(), _dense.ptr(core), ws.data_ptr(),
                                            ws.numel(), max_blocks, _lib.current_stream_ptr()), "n2v_dbscan_count")
    return counts, None if core is None else core.bool(), ws


def neighbor_counts(X: torch.Tensor, eps: float, metric: str = "euclidean",
                    inv_norm: Optional[torch.Tensor] = None, max_blocks: int = 0) -> torch.Tensor:
    """int32 [n]: how many rows lie within eps of every row, itself included -- dbscan's first scan on its own,
    for choosing eps (a row is core at min_samples <= its count).  Arguments as for dbscan."""
    check_metric(metric)
    eps = _eps(eps)
    if int(max_blocks) < 0:
        raise ValueError("max_blocks must be >= 0")
    _dense.shape(X)
    X = _dense.matrix(X)
    _finite(X)
    norms = _norms(X, metric, inv_norm)
    with torch.cuda.device(X.device):
        return _count(X, norms, eps, metric, 1, False, int(max_blocks))[0]


def dbscan(X: torch.Tensor, eps: float, min_samples: int = 5, metric: str = "euclidean",
           inv_norm: Optional[torch.Tensor] = None, max_blocks: int = 0) -> DBSCANResult:
    """DBSCAN of the rows of X (csrc/n2v_dbscan.hip).  A row is core when at least min_samples rows, itself
    included, lie within eps of it (Euclidean distance <= eps, or 1 - cosine <= eps; eps is rounded to fp32, and the
    Euclidean test compares squared distances: there is no square root).  A cluster is a connected component of
    core rows, numbered by its lowest core row; a row that is not core takes the lowest-numbered cluster with a core
    row within eps of it, and is noise (-1) when there is none.  That is the labelling of
    sklearn.cluster.DBSCAN(algorithm="brute"), label for label, wherever fp32 and fp64 agree on which pairs are
    within eps.  The result depends on the set of those pairs alone: the same call gives the same labels whatever
    the launch (max_blocks > 0 caps the blocks of a scan).  At most three scans of 2 n^2 dim FLOPs, the second over
    the core rows and the third over (other rows x core rows); nothing of size n x n and no neighbour list is
    stored.  Two host synchronisations (the sizes of the two row lists).  The rows must be finite.
    silhouette_samples ignores labels outside [0, k), so result.labels goes straight into it (k = n_clusters):
    noise rows are never counted and score NaN."""
    check_metric(metric)
    eps = _eps(eps)
    if int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError(f"min_samples = {min_samples} must be an integer >= 1")
    if int(max_blocks) < 0:
        raise ValueError("max_blocks must be >= 0")
    n, dim = _dense.shape(X)
    X = _dense.matrix(X)
    _finite(X)
    norms = _norms(X, metric, inv_norm)
    L = _lib.load()
    min_samples, max_blocks = min(int(min_samples), (1 << 31) - 1), int(max_blocks)
    with torch.cuda.device(X.device):
        if n == 0:
            none = torch.empty(0, dtype=torch.int32, device=X.device)
            return DBSCANResult(none, none.bool(), 0, none.clone(), torch.zeros(0, dtype=torch.int64, device=X.device))
        counts, core_mask, ws = _count(X, norms, eps, metric, min_samples, True, max_blocks)
        core = torch.nonzero(core_mask)[:, 0].to(torch.int32)
        root = torch.empty(n, dtype=torch.int32, device=X.device)
        _lib.check(L.n2v_dbscan_union(X.data_ptr(), _dense.ptr(norms), n, dim, METRICS[metric], eps, core.data_ptr(),
                                      core.numel(), root.data_ptr(), ws.data_ptr(), ws.numel(), max_blocks,
                                      _lib.current_stream_ptr()), "n2v_dbscan_union")
        # a cluster's id is the rank of its root among the roots: a mask and an exclusive sum
        is_root = core_mask & (root == torch.arange(n, dtype=torch.int32, device=X.device))
        rank = torch.cumsum(is_root, 0, dtype=torch.int32) - 1  # (at a root: the roots before it)
        n_clusters = int(rank[-1]) + 1
        labels = torch.where(core_mask, rank[root.long()], torch.full_like(rank, -1)).contiguous()
        border = torch.nonzero(~core_mask)[:, 0].to(torch.int32)
        _lib.check(L.n2v_dbscan_border(X.data_ptr(), _dense.ptr(norms), n, dim, METRICS[metric], eps,
                                       core.data_ptr(), core.numel(), border.data_ptr(), border.numel(),
                                       labels.data_ptr(), ws.data_ptr(), ws.numel(), max_blocks,
                                       _lib.current_stream_ptr()), "n2v_dbscan_border")
        sizes = torch.bincount(labels[labels >= 0].long(), minlength=n_clusters)
    return DBSCANResult(labels, core_mask, n_clusters, counts, sizes)
