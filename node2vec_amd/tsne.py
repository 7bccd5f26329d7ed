"""t-SNE of trained vectors on the GPU (csrc/n2v_tsne.hip): the two-dimensional map that shows a clustering, without
copying the matrix to the host.

The affinities come from similarity.knn (cosine neighbours), calibrated to a perplexity per row in float64 torch and
symmetrised into a CSR matrix whose rows ascend by column.  The optimiser is van der Maaten's: gains, momentum and
early exaggeration.  Its inner loop is the EXACT gradient: per iteration n2v_tsne_repulse sums the n^2 Student-t
kernels and n2v_tsne_step adds the sparse attraction and updates the layout, three launches in all.  Both run in one
fixed order of fp32 / fp64 operations (DESIGN.md "t-SNE"): the same call gives the same bits.  There is no Barnes-Hut
or interpolation approximation, so an iteration costs O(n^2): 4.7 ms at n = 10^5 on one MI355X (DESIGN.md "t-SNE"),
so 1000 iterations take seconds there and about 8 minutes at n = 10^6, past which the exact gradient stops being
practical -- fit a sample or the first rows instead.  Two output dimensions only.

Device tensors in and out.  There is no CPU path for the gradient: a missing GPU or library raises.  calibrate() and
symmetrise() are plain torch and run on tensors of any device.
"""
import math
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from node2vec_amd import _dense, _lib, similarity

ENTROPY_TOL = 1e-5
MAX_HALVINGS = 100


class Affinities(NamedTuple):
    rowptr: torch.Tensor  # int64 [n + 1]
    col: torch.Tensor     # int32 [nnz], ascending within a row
    val: torch.Tensor     # fp32 [nnz]: P = (P_cond + P_cond^T) / (2 n), rounded once
    perplexity: float
    k: int


class TSNEResult(NamedTuple):
    embedding: torch.Tensor  # fp32 [n, 2]
    kl_divergence: float
    n_iter: int              # iterations run
    grad_norm: float         # of the last gradient measured
    affinities: Affinities


def plan(n: int) -> Tuple[int, int, int]:
    """(tile, slab_cols, n_slabs) of the repulsion's fixed order of summation (n2v_tsne_plan)"""
    import ctypes as C

    tile, slab, slabs = C.c_int32(), C.c_int64(), C.c_int32()
    _lib.check(_lib.load().n2v_tsne_plan(int(n), C.byref(tile), C.byref(slab), C.byref(slabs)), "n2v_tsne_plan")
    return tile.value, slab.value, slabs.value


def calibrate(d2: torch.Tensor, perplexity: float) -> torch.Tensor:
    """P_cond fp64 [n, k]: per row p_j proportional to exp(-beta (d2_j - min d2)) with beta found by bisection so
    that the entropy H = ln(perplexity) within 1e-5 (at most 100 halvings; the bracket doubles and halves until it has
    two ends, as in the original t-SNE).  A non-finite d2 marks an absent entry: p = 0.  Rows sum to 1.  A row whose
    distances are all equal comes out uniform.  All rows at once, in float64, on d2's device."""
    d2 = torch.as_tensor(d2).to(torch.float64)
    if d2.ndim != 2:
        raise ValueError("d2 must be [n, k]")
    present = torch.isfinite(d2)
    big = torch.where(present, d2, torch.full_like(d2, float("inf")))
    dmin = big.min(dim=1, keepdim=True).values
    dmin = torch.where(torch.isfinite(dmin), dmin, torch.zeros_like(dmin))
    d = torch.where(present, d2 - dmin, torch.zeros_like(d2))
    target = math.log(float(perplexity))
    n = d2.shape[0]
    beta = torch.ones((n, 1), dtype=torch.float64, device=d2.device)
    lo = torch.full_like(beta, float("-inf"))
    hi = torch.full_like(beta, float("inf"))

    def probabilities(b):
        p = torch.where(present, torch.exp(-b * d), torch.zeros_like(d))
        s = p.sum(dim=1, keepdim=True).clamp(min=1e-300)
        return p, s

    for _ in range(MAX_HALVINGS):
        p, s = probabilities(beta)
        H = torch.log(s) + beta * (d * p).sum(dim=1, keepdim=True) / s
        diff = H - target
        todo = diff.abs() > ENTROPY_TOL
        if not bool(todo.any()):
            break
        up = todo & (diff > 0)   # too flat: beta grows
        down = todo & (diff <= 0)
        lo = torch.where(up, beta, lo)
        hi = torch.where(down, beta, hi)
        grown = torch.where(torch.isinf(hi), beta * 2.0, (beta + hi) / 2.0)
        shrunk = torch.where(torch.isinf(lo), beta / 2.0, (beta + lo) / 2.0)
        beta = torch.where(up, grown, torch.where(down, shrunk, beta))
    p, s = probabilities(beta)
    return p / s


def symmetrise(idx: torch.Tensor, p_cond: torch.Tensor, n: int):
    """(rowptr int64 [n + 1], col int32, val fp32) of P = (C + C^T) / (2 n), C[i, idx[i, j]] = p_cond[i, j]; an entry
    with idx < 0 is dropped.  The entries of both halves are merged by a sort on (row, col): a row ascends by column,
    an entry present in both halves is their fp64 sum, and val is rounded to fp32 once.  The entries of a row of idx
    must be distinct."""
    idx = torch.as_tensor(idx).to(torch.int64)
    p_cond = torch.as_tensor(p_cond, device=idx.device).to(torch.float64)
    if idx.ndim != 2 or idx.shape != p_cond.shape or idx.shape[0] != n:
        raise ValueError("idx and p_cond must both be [n, k]")
    keep = (idx >= 0) & (idx < n)
    rows = torch.arange(n, device=idx.device, dtype=torch.int64)[:, None].expand_as(idx)[keep]
    cols = idx[keep]
    v = p_cond[keep] / (2.0 * n)
    keys = torch.cat([rows * n + cols, cols * n + rows])
    uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
    val = torch.zeros(uniq.shape[0], dtype=torch.float64, device=idx.device)
    val.index_add_(0, inverse, torch.cat([v, v]))  # at most two terms per entry: the sum has one order
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    rowptr[1:] = torch.cumsum(torch.bincount(torch.div(uniq, n, rounding_mode="floor"), minlength=n), 0)
    return rowptr, (uniq % n).to(torch.int32), val.to(torch.float32)


def default_k(n: int, perplexity: float) -> int:
    return min(n - 1, int(math.floor(3.0 * perplexity)))


def check_perplexity(n: int, perplexity) -> float:
    perplexity = float(perplexity)
    if not (1.0 <= perplexity < n - 1):
        raise ValueError(f"perplexity = {perplexity} outside [1, n - 1) for n = {n}")
    return perplexity


def affinities(X: torch.Tensor, perplexity: float = 30.0, k: Optional[int] = None, metric: str = "cosine",
               inv_norm: Optional[torch.Tensor] = None, neighbours=None) -> Affinities:
    """The symmetric affinities P of the rows of X as CSR.  The neighbours are similarity.knn's k nearest by cosine
    (k: min(n - 1, floor(3 perplexity)) by default), their squared distances those of unit rows, d2 = max(0, 2 (1 -
    score)) in float64.  neighbours=(idx int64 [n, k], d2 [n, k]) brings lists of the caller's own instead (from an
    IVF index, or Euclidean distances); an index of -1 is an absent entry.  Only metric "cosine" is built in."""
    n, _ = _dense.shape(X)
    perplexity = check_perplexity(n, perplexity)
    if metric != "cosine":
        raise ValueError(f'metric {metric!r}: the neighbour search here is cosine; bring other distances through '
                         f'neighbours=(idx, d2)')
    if neighbours is not None:
        idx, d2 = neighbours
        idx = torch.as_tensor(idx).to(torch.int64)
        d2 = torch.as_tensor(d2, device=idx.device).to(torch.float64)
        if idx.ndim != 2 or idx.shape[0] != n or d2.shape != idx.shape:
            raise ValueError("neighbours must be (idx [n, k], d2 [n, k])")
        k = int(idx.shape[1])
    else:
        k = default_k(n, perplexity) if k is None else int(k)
        if not 1 <= k <= n - 1:
            raise ValueError(f"k = {k} outside [1, n - 1]")
        X = _dense.matrix(X)
        if inv_norm is None:
            inv_norm = similarity.inv_norms(X)
        step = max(1, similarity.WORKSPACE_LIMIT // (16 * (k + 1)))  # the int64 rows and fp32 scores of a batch
        parts = []
        for i in range(0, n, step):
            rows = torch.arange(i, min(n, i + step), device=X.device, dtype=torch.int64)
            r, s = similarity.knn(X, k, rows=rows, exclude_self=True, inv_norm=inv_norm)
            parts.append((r, (2.0 * (1.0 - s.double())).clamp_(min=0.0)))
        idx = torch.cat([p[0] for p in parts])
        d2 = torch.cat([p[1] for p in parts])
    d2 = torch.where(idx >= 0, d2, torch.full_like(d2, float("inf")))
    rowptr, col, val = symmetrise(idx, calibrate(d2, perplexity), n)
    return Affinities(rowptr, col, val, perplexity, k)


def _layout(Y) -> torch.Tensor:
    if not isinstance(Y, torch.Tensor) or Y.ndim != 2 or Y.shape[1] != 2 or not Y.is_cuda:
        raise ValueError("Y must be an [n, 2] tensor on a HIP device")
    return Y.to(torch.float32).contiguous()


class _Loop:
    """the buffers of the optimiser's inner loop and its two calls"""

    def __init__(self, aff: Affinities, Y: torch.Tensor):
        self.L = _lib.load()
        self.n = n = int(Y.shape[0])
        if aff.rowptr.shape[0] != n + 1:
            raise ValueError(f"the affinities are of {aff.rowptr.shape[0] - 1} rows, the layout of {n}")
        dev = Y.device
        self.aff = Affinities(aff.rowptr.to(dev, torch.int64).contiguous(), aff.col.to(dev, torch.int32).contiguous(),
                              aff.val.to(dev, torch.float32).contiguous(), aff.perplexity, aff.k)
        self.nnz = int(self.aff.col.shape[0])
        self.Y = [Y.clone(), torch.empty_like(Y)]
        self.rep = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        self.zrow = torch.zeros(n, dtype=torch.float64, device=dev)
        self.Z = torch.zeros(1, dtype=torch.float64, device=dev)
        self.vel = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        self.gain = torch.ones((n, 2), dtype=torch.float32, device=dev)
        self.grad = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        self.ws = _dense.workspace(self.L.n2v_tsne_workspace_bytes, n, device=dev)
        self.at = 0  # which of the two Y buffers is current

    def repulse(self) -> None:
        _lib.check(self.L.n2v_tsne_repulse(self.Y[self.at].data_ptr(), self.n, self.rep.data_ptr(),
                                           self.zrow.data_ptr(), self.Z.data_ptr(), self.ws.data_ptr(),
                                           self.ws.numel(), _lib.current_stream_ptr()), "n2v_tsne_repulse")

    def step(self, exaggeration, learning_rate, momentum, min_gain, vel=None, gain=None) -> None:
        """the current Y's rep and Z must be in place; the other buffer becomes current"""
        a = self.aff
        vel = self.vel if vel is None else vel
        gain = self.gain if gain is None else gain
        _lib.check(self.L.n2v_tsne_step(a.rowptr.data_ptr(), _dense.ptr(a.col), _dense.ptr(a.val), self.nnz,
                                        self.Y[self.at].data_ptr(), self.rep.data_ptr(), self.Z.data_ptr(), self.n,
                                        exaggeration, learning_rate, momentum, min_gain, vel.data_ptr(),
                                        gain.data_ptr(), self.Y[1 - self.at].data_ptr(), self.grad.data_ptr(),
                                        _lib.current_stream_ptr()), "n2v_tsne_step")
        self.at = 1 - self.at


def repulse(Y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rep fp64 [n, 2], zrow fp64 [n], Z fp64 [1]) of a layout: n2v_tsne_repulse"""
    Y = _layout(Y)
    n = int(Y.shape[0])
    L = _lib.load()
    rep = torch.zeros((n, 2), dtype=torch.float64, device=Y.device)
    zrow = torch.zeros(n, dtype=torch.float64, device=Y.device)
    Z = torch.zeros(1, dtype=torch.float64, device=Y.device)
    with torch.cuda.device(Y.device):
        ws = _dense.workspace(L.n2v_tsne_workspace_bytes, n, device=Y.device)
        _lib.check(L.n2v_tsne_repulse(Y.data_ptr(), n, rep.data_ptr(), zrow.data_ptr(), Z.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _lib.current_stream_ptr()), "n2v_tsne_repulse")
    return rep, zrow, Z


def gradient(aff: Affinities, Y: torch.Tensor, exaggeration: float = 1.0) -> Tuple[torch.Tensor, float]:
    """(grad fp32 [n, 2], Z): the gradient of KL(P || Q) at Y, 4 (exaggeration * attraction - repulsion / Z): one
    n2v_tsne_repulse and one n2v_tsne_step with a zero learning rate on a state of its own.  One host
    synchronisation (Z)."""
    Y = _layout(Y)
    with torch.cuda.device(Y.device):
        loop = _Loop(aff, Y)
        loop.repulse()
        loop.step(float(exaggeration), 0.0, 0.0, 0.0)
    return loop.grad, float(loop.Z.item())


def kl_divergence(aff: Affinities, Y: torch.Tensor) -> float:
    """KL(P || Q) = sum p ln(p (1 + d^2) Z) over the entries of P, in float64 torch, Z from n2v_tsne_repulse"""
    Y = _layout(Y)
    n = int(Y.shape[0])
    Z = repulse(Y)[2]
    rowptr = aff.rowptr.to(Y.device)
    rows = torch.repeat_interleave(torch.arange(n, device=Y.device), rowptr[1:] - rowptr[:-1])
    p = aff.val.to(Y.device).double()
    Yd = Y.double()
    d2 = ((Yd[rows] - Yd[aff.col.to(Y.device).long()]) ** 2).sum(1)
    live = p > 0
    return float((p[live] * torch.log(p[live] * (1.0 + d2[live]) * Z)).sum().item())


def _initial(X, init, seed, n, device, inv_norm) -> torch.Tensor:
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (n, 2):
            raise ValueError(f"init must be [{n}, 2]")
        return init.to(device=device, dtype=torch.float32).contiguous()
    if init == "random":
        Y = np.random.default_rng(seed).standard_normal((n, 2)) * 1e-4
        return torch.from_numpy(Y.astype(np.float32)).to(device)
    if init == "pca":
        if X is None:
            raise ValueError('init="pca" needs the vectors: pass X, or an init of your own with the affinities')
        from node2vec_amd import pca

        res = pca.fit(X, 2, unit=True, inv_norm=inv_norm)
        Y = pca.transform(X, res, inv_norm=inv_norm).double()
        return (Y / Y[:, 0].std(unbiased=False) * 1e-4).float().contiguous()
    raise ValueError('init must be "pca", "random" or an [n, 2] tensor')


def fit(X_or_affinities: Union[torch.Tensor, Affinities], n_iter: int = 1000, perplexity: float = 30.0,
        early_exaggeration: float = 12.0, exaggeration_iter: int = 250, learning_rate="auto",
        momentum: Tuple[float, float] = (0.5, 0.8), min_gain: float = 0.01, init="pca", seed: int = 0,
        check_every: int = 50, min_grad_norm: float = 1e-7, **affinity_kw) -> TSNEResult:
    """The t-SNE map of the rows of X (or of affinities made before).  Iterations [0, exaggeration_iter) multiply P
    by early_exaggeration and use momentum[0]; the rest use 1 and momentum[1].  learning_rate "auto":
    max(n / early_exaggeration / 4, 50).  init: "pca" (pca.fit(X, 2, unit=True) projected, the first column scaled
    to a standard deviation of 1e-4), "random" (numpy.random.default_rng(seed) normals times 1e-4, made on the host)
    or an [n, 2] tensor.  The host synchronises every check_every iterations only: a non-finite layout raises
    ValueError, and past the exaggeration a gradient norm below min_grad_norm stops the loop.  Three launches per
    iteration; the two layout buffers alternate.  The other arguments go to affinities()."""
    if isinstance(X_or_affinities, Affinities):
        X, aff = None, X_or_affinities
        if affinity_kw:
            raise ValueError(f"{sorted(affinity_kw)} go with X, not with affinities made before")
        n = int(aff.rowptr.shape[0]) - 1
        device = aff.rowptr.device
    else:
        n, _ = _dense.shape(X_or_affinities)
        check_perplexity(n, perplexity)
        X = _dense.matrix(X_or_affinities)
        device = X.device
        if affinity_kw.get("inv_norm") is None and affinity_kw.get("neighbours") is None:
            affinity_kw["inv_norm"] = similarity.inv_norms(X)
        aff = affinities(X, perplexity, **affinity_kw)
    n_iter, exaggeration_iter, check_every = int(n_iter), int(exaggeration_iter), max(1, int(check_every))
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    if learning_rate == "auto":
        learning_rate = max(n / float(early_exaggeration) / 4.0, 50.0)
    learning_rate, min_gain = float(learning_rate), float(min_gain)
    with torch.cuda.device(device):
        Y0 = _layout(_initial(X, init, seed, n, device, affinity_kw.get("inv_norm")))
        loop = _Loop(aff, Y0)
        done, grad_norm = 0, float("nan")
        for it in range(n_iter):
            early = it < exaggeration_iter
            loop.repulse()
            loop.step(float(early_exaggeration) if early else 1.0, learning_rate,
                      float(momentum[0] if early else momentum[1]), min_gain)
            done = it + 1
            if done % check_every == 0 or done == n_iter:
                grad_norm = float(torch.linalg.vector_norm(loop.grad.double()).item())
                if not bool(torch.isfinite(loop.Y[loop.at]).all()):
                    raise ValueError(f"the layout holds a non-finite value after {done} iterations: lower "
                                     f"learning_rate or early_exaggeration")
                if not early and grad_norm < min_grad_norm:
                    break
        Y = loop.Y[loop.at]
        return TSNEResult(Y, kl_divergence(loop.aff, Y), done, grad_norm, loop.aff)
