"""UMAP layouts of trained vectors on the GPU (csrc/n2v_umap.hip): the non-linear 2-D map whose epoch costs
O(n k (1 + negatives)), for the sizes at which tsne.py's exact O(n^2) gradient stops being practical.

The fuzzy graph comes from similarity.knn (cosine neighbours, distance max(0, 1 - score)), smoothed per row in
float64 torch (rho, sigma) and merged with its transpose by the probabilistic union A + A^T - A o A^T into a CSR matrix
whose rows ascend by column.  The optimiser is umap-learn's sampled attraction and repulsion, formulated so that it is
reproducible: every vertex is one sequential chain over its own entries, every other vertex is read from the previous
epoch's layout, and the negative draws are counter-based (DESIGN.md "UMAP").  The same call gives the same bits on any
launch geometry; one launch per epoch (0.08 ms at n = 10^5, 1.0 ms at 10^6 on one MI355X: DESIGN.md "UMAP"); the two
layout buffers alternate.  Two output dimensions only; no transform of
new points, no supervision, set_op_mix_ratio = local_connectivity = 1.

Device tensors in and out.  There is no CPU path for the epoch: a missing GPU or library raises.  find_ab() is numpy;
smooth_knn(), fuzzy_graph() from the caller's neighbours and epochs_per_sample() are plain torch and run on tensors
of any device.
"""
import math
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from node2vec_amd import _dense, _lib, similarity

SMOOTH_TOL = 1e-5       # umap-learn's SMOOTH_K_TOLERANCE
MAX_HALVINGS = 64
MIN_K_DIST_SCALE = 1e-3
MAX_NEGATIVE = 64       # n2v_umap_epoch's bound


class FuzzyGraph(NamedTuple):
    rowptr: torch.Tensor  # int64 [n + 1]
    col: torch.Tensor     # int32 [nnz], ascending within a row
    val: torch.Tensor     # fp32 [nnz]: A + A^T - A o A^T, rounded once; symmetric bit for bit
    n_neighbors: int


class UMAPResult(NamedTuple):
    embedding: torch.Tensor  # fp32 [n, 2]
    a: float
    b: float
    n_epochs: int
    graph: FuzzyGraph


def find_ab(spread: float = 1.0, min_dist: float = 0.1) -> Tuple[float, float]:
    """(a, b) of the curve 1 / (1 + a x^(2 b)) nearest, in least squares on linspace(0, 3 spread, 300), to umap-learn's
    target: 1 below min_dist, exp(-(x - min_dist) / spread) from there on.  Levenberg-Marquardt from (1, 1) in
    float64 numpy; find_ab(1.0, 0.1) is umap-learn's (1.5769, 0.8951)."""
    spread, min_dist = float(spread), float(min_dist)
    if not (spread > 0.0 and 0.0 <= min_dist < 3.0 * spread):
        raise ValueError("find_ab wants spread > 0 and 0 <= min_dist < 3 spread")
    x = np.linspace(0.0, 3.0 * spread, 300)
    target = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    xs, ts = x[1:], target[1:]  # x = 0 gives 1 for every (a, b)
    lx = np.log(xs)

    def residual(p):
        return 1.0 / (1.0 + p[0] * xs ** (2.0 * p[1])) - ts

    p, lam = np.array([1.0, 1.0]), 1e-3
    cost = float((residual(p) ** 2).sum())
    for _ in range(200):
        pw = xs ** (2.0 * p[1])
        f = 1.0 / (1.0 + p[0] * pw)
        J = np.stack([-f * f * pw, -f * f * p[0] * pw * 2.0 * lx], axis=1)
        r = f - ts
        H, g = J.T @ J, J.T @ r
        step = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        trial = p + step
        trial_cost = float((residual(trial) ** 2).sum()) if (trial > 0).all() else float("inf")
        if trial_cost < cost:
            done = cost - trial_cost <= 1e-16 * cost
            p, cost, lam = trial, trial_cost, lam * 0.3
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


def smooth_knn(dist: torch.Tensor, k: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rho fp64 [n], sigma fp64 [n]) of rows of neighbour distances [n, m] (a non-finite distance is an absent
    entry): rho is the row's smallest positive distance (0 if there is none), sigma comes by bisection so that
    sum_j exp(-max(0, d_j - rho) / sigma) = log2(k) within 1e-5 -- umap-learn's bracket rule: from 1, doubling until the
    sum is too large, then halving, 64 steps at most -- and is at least 1e-3 times the row's mean distance (the mean
    of all distances for a row with rho = 0).  All rows at once, in float64, on dist's device."""
    dist = torch.as_tensor(dist).to(torch.float64)
    if dist.ndim != 2:
        raise ValueError("dist must be [n, m]")
    present = torch.isfinite(dist)
    zero = torch.zeros_like(dist)
    inf = torch.full_like(dist, float("inf"))
    rho = torch.where(present & (dist > 0), dist, inf).min(dim=1, keepdim=True).values
    rho = torch.where(torch.isfinite(rho), rho, torch.zeros_like(rho))
    d = torch.where(present, (dist - rho).clamp(min=0.0), zero)
    target = math.log2(float(k))
    sigma = torch.ones_like(rho)
    lo = torch.zeros_like(rho)
    hi = torch.full_like(rho, float("inf"))
    for _ in range(MAX_HALVINGS):
        psum = torch.where(present, torch.exp(-d / sigma), zero).sum(dim=1, keepdim=True)
        todo = (psum - target).abs() >= SMOOTH_TOL
        if not bool(todo.any()):
            break
        down = todo & (psum > target)
        up = todo & ~down
        hi = torch.where(down, sigma, hi)
        lo = torch.where(up, sigma, lo)
        grown = torch.where(torch.isinf(hi), sigma * 2.0, (lo + hi) / 2.0)
        sigma = torch.where(down, (lo + hi) / 2.0, torch.where(up, grown, sigma))
    count = present.sum(dim=1, keepdim=True).clamp(min=1)
    row_mean = torch.where(present, dist, zero).sum(dim=1, keepdim=True) / count
    all_mean = torch.where(present, dist, zero).sum() / present.sum().clamp(min=1)
    floor = MIN_K_DIST_SCALE * torch.where(rho > 0, row_mean, all_mean.expand_as(row_mean))
    return rho[:, 0], torch.maximum(sigma, floor)[:, 0]


def _union(idx: torch.Tensor, member: torch.Tensor, n: int):
    """(rowptr, col, val fp32) of A + A^T - A o A^T, A[i, idx[i, j]] = member[i, j]; an entry with idx outside [0, n)
    or on the diagonal is dropped.  Both halves are merged by a stable sort on (row, col): a row ascends by column; an
    entry present in both halves is (a + b) - a * b in float64, a sum and a product that commute, so val is symmetric
    bit for bit; val is rounded to fp32 once.  The entries of a row of idx must be distinct."""
    dev = idx.device
    rows = torch.arange(n, device=dev, dtype=torch.int64)[:, None].expand_as(idx)
    keep = (idx >= 0) & (idx < n) & (idx != rows)
    r, c, v = rows[keep], idx[keep], member[keep]
    keys, perm = torch.sort(torch.cat([r * n + c, c * n + r]), stable=True)
    vals = torch.cat([v, v])[perm]
    m = keys.shape[0]
    first = torch.ones(m, dtype=torch.bool, device=dev)
    first[1:] = keys[1:] != keys[:-1]
    paired = torch.zeros(m, dtype=torch.bool, device=dev)
    paired[:-1] = ~first[1:]
    other = torch.where(paired, torch.roll(vals, -1), torch.zeros_like(vals))
    val = ((vals + other) - vals * other)[first]
    uniq = keys[first]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(torch.div(uniq, n, rounding_mode="floor"), minlength=n), 0)
    return rowptr, (uniq % n).to(torch.int32), val.to(torch.float32)


def check_neighbors(n: int, n_neighbors) -> int:
    n_neighbors = int(n_neighbors)
    if not 2 <= n_neighbors <= n - 1:
        raise ValueError(f"n_neighbors = {n_neighbors} outside [2, n - 1] for n = {n}")
    return n_neighbors


def fuzzy_graph(X: Optional[torch.Tensor], n_neighbors: int = 15, inv_norm: Optional[torch.Tensor] = None,
                neighbours=None) -> FuzzyGraph:
    """The fuzzy simplicial set of the rows of X as a symmetric CSR.  The neighbours are similarity.knn's n_neighbors
    nearest other rows by cosine, their distance max(0, 1 - score) in float64.  neighbours=(idx int64 [n, k], dist
    [n, k]) brings lists of the caller's own instead (from an IVF index, or another metric; X may then be None): an
    index of -1, or a row's own, is an absent entry.  Memberships are exp(-max(0, d - rho) / sigma) with smooth_knn's
    (rho, sigma) for log2(k); the union is A + A^T - A o A^T."""
    if neighbours is not None:
        idx, dist = neighbours
        idx = torch.as_tensor(idx).to(torch.int64)
        dist = torch.as_tensor(dist, device=idx.device).to(torch.float64)
        if idx.ndim != 2 or dist.shape != idx.shape or (X is not None and idx.shape[0] != _dense.shape(X)[0]):
            raise ValueError("neighbours must be (idx [n, k], dist [n, k])")
        n, k = int(idx.shape[0]), int(idx.shape[1])
    else:
        n, _ = _dense.shape(X)
        k = check_neighbors(n, n_neighbors)
        X = _dense.matrix(X)
        if inv_norm is None:
            inv_norm = similarity.inv_norms(X)
        step = max(1, similarity.WORKSPACE_LIMIT // (16 * (k + 1)))  # the int64 rows and fp32 scores of a batch
        parts = []
        for i in range(0, n, step):
            rows = torch.arange(i, min(n, i + step), device=X.device, dtype=torch.int64)
            r, s = similarity.knn(X, k, rows=rows, exclude_self=True, inv_norm=inv_norm)
            parts.append((r, (1.0 - s.double()).clamp_(min=0.0)))
        idx = torch.cat([p[0] for p in parts])
        dist = torch.cat([p[1] for p in parts])
    rows = torch.arange(n, device=idx.device, dtype=torch.int64)[:, None]
    dist = torch.where((idx >= 0) & (idx < n) & (idx != rows), dist, torch.full_like(dist, float("inf")))
    rho, sigma = smooth_knn(dist, k)
    member = torch.exp(-(dist - rho[:, None]).clamp(min=0.0) / sigma[:, None])
    rowptr, col, val = _union(idx, member, n)
    return FuzzyGraph(rowptr, col, val, k)


def epochs_per_sample(val: torch.Tensor) -> torch.Tensor:
    """fp32 [nnz]: w_max / w, one fp32 division; +inf (never sampled) where w <= 0"""
    val = torch.as_tensor(val).to(torch.float32)
    if val.numel() == 0:
        return val.clone()
    eps = val.max() / val
    return torch.where(val > 0, eps, torch.full_like(eps, float("inf")))


def _layout(Y) -> torch.Tensor:
    if not isinstance(Y, torch.Tensor) or Y.ndim != 2 or Y.shape[1] != 2 or not Y.is_cuda:
        raise ValueError("Y must be an [n, 2] tensor on a HIP device")
    return Y.to(torch.float32).contiguous()


def epoch(rowptr: torch.Tensor, col: torch.Tensor, eps: torch.Tensor, Y: torch.Tensor, Y_next: torch.Tensor,
          e: int, a: float, b: float, gamma: float = 1.0, alpha: float = 1.0, negative: int = 5, seed: int = 0,
          max_blocks: int = 0) -> None:
    """n2v_umap_epoch, the raw call: Y_next = epoch e from Y (fp32 [n, 2] contiguous device tensors, two buffers)
    over the CSR (rowptr int64, col int32, eps fp32) on Y's device.  Enqueues; does not synchronise."""
    n = int(Y.shape[0])
    for t, dtype, name in ((rowptr, torch.int64, "rowptr"), (col, torch.int32, "col"), (eps, torch.float32, "eps"),
                           (Y, torch.float32, "Y"), (Y_next, torch.float32, "Y_next")):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on a HIP device")
    if tuple(Y.shape) != (n, 2) or Y_next.shape != Y.shape or rowptr.shape[0] != n + 1 or col.shape != eps.shape:
        raise ValueError("epoch wants Y, Y_next [n, 2], rowptr [n + 1] and col, eps [nnz]")
    with torch.cuda.device(Y.device):
        _lib.check(_lib.load().n2v_umap_epoch(rowptr.data_ptr(), _dense.ptr(col), _dense.ptr(eps), int(col.shape[0]),
                                              Y.data_ptr(), Y_next.data_ptr(), n, int(e), float(a), float(b),
                                              float(gamma), float(alpha), int(negative), int(seed) & (2 ** 64 - 1),
                                              int(max_blocks), _lib.current_stream_ptr()), "n2v_umap_epoch")


def powb(x: torch.Tensor, b: float) -> torch.Tensor:
    """n2v_umap_powb: the epoch's x^b over an fp32 device tensor (0 where x is not positive)"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("x must be an fp32 tensor on a HIP device")
    x = x.contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().n2v_umap_powb(x.data_ptr(), x.numel(), float(b), out.data_ptr(),
                                             _lib.current_stream_ptr()), "n2v_umap_powb")
    return out


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def alpha_of(e: int, n_epochs: int, learning_rate: float = 1.0) -> float:
    """the step size of epoch e, computed on the host in float64 and passed to the kernel as fp32"""
    return float(learning_rate) * (1.0 - float(e) / float(n_epochs))


def _initial(X, init, seed, n, device, inv_norm) -> torch.Tensor:
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (n, 2):
            raise ValueError(f"init must be [{n}, 2]")
        return init.to(device=device, dtype=torch.float32).contiguous()
    if init == "random":
        Y = np.random.default_rng(seed).uniform(-10.0, 10.0, (n, 2))
        return torch.from_numpy(Y.astype(np.float32)).to(device)
    if init == "pca":
        if X is None:
            raise ValueError('init="pca" needs the vectors: pass X, or an init of your own with the graph')
        from node2vec_amd import pca

        res = pca.fit(X, 2, unit=True, inv_norm=inv_norm)
        Y = pca.transform(X, res, inv_norm=inv_norm).double()
        lo = Y.min(dim=0, keepdim=True).values
        span = Y.max(dim=0, keepdim=True).values - lo
        span = torch.where(span > 0, span, torch.ones_like(span))
        return (10.0 * (Y - lo) / span).float().contiguous()
    raise ValueError('init must be "pca", "random" or an [n, 2] tensor')


def fit(X_or_graph: Union[torch.Tensor, FuzzyGraph], n_epochs: Optional[int] = None, min_dist: float = 0.1,
        spread: float = 1.0, a: Optional[float] = None, b: Optional[float] = None, learning_rate: float = 1.0,
        negative_sample_rate: int = 5, repulsion_strength: float = 1.0, init="pca", seed: int = 0,
        check_every: int = 50, **graph_kw) -> UMAPResult:
    """The UMAP layout of the rows of X (or of a fuzzy graph made before).  n_epochs: 500 for n <= 10 000, else 200.
    a, b: find_ab(spread, min_dist) unless both are given.  Epoch e runs n2v_umap_epoch with the step size
    learning_rate (1 - e / n_epochs), negative_sample_rate draws per firing entry and the draws' key (seed, e).
    init: "pca" (pca.fit(X, 2, unit=True) projected, every coordinate shifted and scaled to span [0, 10]), "random"
    (numpy.random.default_rng(seed) uniform in [-10, 10], made on the host) or an [n, 2] tensor.  The host
    synchronises every check_every epochs only: a non-finite layout raises ValueError.  One launch per epoch; the two
    layout buffers alternate.  The other arguments (n_neighbors, inv_norm, neighbours) go to fuzzy_graph()."""
    if isinstance(X_or_graph, FuzzyGraph):
        X, graph = None, X_or_graph
        if graph_kw:
            raise ValueError(f"{sorted(graph_kw)} go with X, not with a graph made before")
        n = int(graph.rowptr.shape[0]) - 1
        device = graph.rowptr.device
    else:
        n, _ = _dense.shape(X_or_graph)
        if graph_kw.get("neighbours") is None:
            check_neighbors(n, graph_kw.get("n_neighbors", 15))
        X, graph = X_or_graph, None
        device = X.device
    n_epochs = default_epochs(n) if n_epochs is None else int(n_epochs)
    negative, check_every = int(negative_sample_rate), max(1, int(check_every))
    if n_epochs < 0:
        raise ValueError("n_epochs must be >= 0")
    if not 0 <= negative <= MAX_NEGATIVE:
        raise ValueError(f"negative_sample_rate = {negative} outside [0, {MAX_NEGATIVE}]")
    if (a is None) != (b is None):
        raise ValueError("give both a and b, or neither")
    if a is None:
        a, b = find_ab(spread, min_dist)
    a, b = float(a), float(b)
    if not (0.0 < a < float("inf") and 0.0 < b < float("inf")):
        raise ValueError("a and b must be finite and positive")
    if not isinstance(init, torch.Tensor) and init not in ("pca", "random"):
        raise ValueError('init must be "pca", "random" or an [n, 2] tensor')
    if graph is None:
        X = _dense.matrix(X)
    with torch.cuda.device(device):
        if graph is None:
            if graph_kw.get("inv_norm") is None and graph_kw.get("neighbours") is None:
                graph_kw["inv_norm"] = similarity.inv_norms(X)
            graph = fuzzy_graph(X, **graph_kw)
        graph = FuzzyGraph(graph.rowptr.to(device, torch.int64).contiguous(),
                           graph.col.to(device, torch.int32).contiguous(),
                           graph.val.to(device, torch.float32).contiguous(), graph.n_neighbors)
        Y0 = _layout(_initial(X, init, seed, n, device, graph_kw.get("inv_norm")))
        eps = epochs_per_sample(graph.val)
        Y = [Y0.clone(), torch.empty_like(Y0)]
        at = 0
        for e in range(n_epochs):
            epoch(graph.rowptr, graph.col, eps, Y[at], Y[1 - at], e, a, b, repulsion_strength,
                  alpha_of(e, n_epochs, learning_rate), negative, seed)
            at = 1 - at
            if (e + 1) % check_every == 0 or e + 1 == n_epochs:
                if not bool(torch.isfinite(Y[at]).all()):
                    raise ValueError(f"the layout holds a non-finite value after {e + 1} epochs: lower learning_rate")
        return UMAPResult(Y[at], a, b, n_epochs, graph)
