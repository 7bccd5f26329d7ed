"""Principal components of trained vectors, on the GPU (csrc/n2v_pca.hip): the projection that plots a clustering,
shrinks dim or whitens, without copying the matrix to the host.

Two passes over X: the fp64 column means (n2v_pca_mean) and the dim x dim scatter matrix of the centred rows
(n2v_pca_scatter, an MFMA chain over the rows).  Only the dim x dim eigenproblem runs on the host
(numpy.linalg.eigh in float64).  The projection is classify.decision_function: X V^T + b with pinned bits.  Every
mean, scatter element and projected value is computed in one fixed order of fp32 / fp64 operations (DESIGN.md
"Principal components"): the same call gives the same bits.  unit=True takes the rows as directions (x / |x|, as
every KeyedVectors query does).  A row holding a non-finite value is skipped by the fit and not counted; its
projection is whatever the arithmetic gives: NaN.

Device tensors in and out.  There is no CPU path: a missing GPU or library raises.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from node2vec_amd import _dense, _lib


class PCAResult(NamedTuple):
    components: torch.Tensor                # fp32 [k, dim], orthonormal rows, largest variance first
    mean: torch.Tensor                      # fp32 [dim]: the centre the scatter pass subtracted (zeros: uncentred)
    explained_variance: torch.Tensor        # fp64 [k]: eigenvalues of S / (n_used - 1), descending
    explained_variance_ratio: torch.Tensor  # fp64 [k]: explained_variance / total_variance
    singular_values: torch.Tensor           # fp64 [k]: sqrt(explained_variance (n_used - 1))
    total_variance: float                   # trace of S / (n_used - 1)
    n_used: int                             # rows whose values are all finite
    unit: bool
    whiten: bool


def alloc_workspace(n: int, dim: int, device) -> torch.Tensor:
    return _dense.workspace(_lib.load().n2v_pca_workspace_bytes, n, dim, device=device)


def slab_rows(n: int, dim: int) -> int:
    """rows per slab of the fixed order of summation of both passes (n2v_pca_slab_rows)"""
    return int(_lib.load().n2v_pca_slab_rows(n, dim))


def moments(X: torch.Tensor, center: bool = True, unit: bool = False,
            inv_norm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(mean fp64 [dim], S fp64 [dim, dim], n_used): the column means of the used rows (computed whether or not
    they are subtracted) and the scatter matrix sum_r xc_r xc_r^T, xc = x - float32(mean) (center=False: xc = x),
    symmetric to the bit.  unit: rows scaled by 1 / norm first (inv_norm: similarity.inv_norms(X), computed when
    not given; passing inv_norm implies nothing without unit=True).  One host synchronisation (n_used)."""
    n, dim = _dense.shape(X)
    _dense.check_inv_norm(n, inv_norm if unit else None)
    X = _dense.matrix(X)
    norms = _dense.norms(X, inv_norm) if unit else None
    mean = torch.zeros(dim, dtype=torch.float64, device=X.device)
    S = torch.zeros((dim, dim), dtype=torch.float64, device=X.device)
    used = torch.zeros(2, dtype=torch.int64, device=X.device)
    L = _lib.load()
    with torch.cuda.device(X.device):
        ws = alloc_workspace(n, dim, X.device)
        _lib.check(L.n2v_pca_mean(X.data_ptr(), _dense.ptr(norms), n, dim, mean.data_ptr(), used.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()), "n2v_pca_mean")
        centre = mean.float() if center else None
        _lib.check(L.n2v_pca_scatter(X.data_ptr(), _dense.ptr(norms), n, dim, _dense.ptr(centre), S.data_ptr(),
                                     used[1:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "n2v_pca_scatter")
    counts = used.cpu()
    assert int(counts[0]) == int(counts[1]), "the two passes disagree on the used rows"
    return mean, S, int(counts[0])


def fix_signs(V: np.ndarray) -> np.ndarray:
    """rows of V with the sign rule applied: a component's entry of largest magnitude is positive, the lowest index
    on ties"""
    V = np.array(V, dtype=np.float64, copy=True)
    if V.size:
        at = np.argmax(np.abs(V), axis=1)  # the first of equal maxima
        V[V[np.arange(V.shape[0]), at] < 0] *= -1.0
    return V


def check_components(n_components, dim: int, n_used: Optional[int] = None) -> Optional[int]:
    if n_components is None:
        return None
    k = int(n_components)
    most = dim if n_used is None else min(dim, n_used - 1)
    if k < 1 or k > most:
        raise ValueError(f"n_components = {k} outside [1, {most}] (min(dim, n_used - 1))")
    return k


def fit(X: torch.Tensor, n_components: Optional[int] = None, center: bool = True, unit: bool = False,
        whiten: bool = False, inv_norm: Optional[torch.Tensor] = None) -> PCAResult:
    """The leading n_components principal components of the rows of X (None: min(dim, n_used - 1)).  The covariance
    is S / (n_used - 1) from moments(); its eigenproblem runs on the host (numpy.linalg.eigh, float64), eigenvalues
    descending, negative ones from rounding clamped to 0; sign rule: fix_signs.  whiten only marks the result:
    transform() then scales every component to unit variance.  ValueError: fewer than two used rows, n_components
    out of range, or a non-finite element of S (an fp32 product or sum of the scatter pass overflowed)."""
    n, dim = _dense.shape(X)
    check_components(n_components, dim)
    _dense.check_inv_norm(n, inv_norm if unit else None)
    mean, S, n_used = moments(X, center, unit, inv_norm)
    if n_used < 2:
        raise ValueError(f"{n_used} rows of X hold only finite values: principal components need at least 2")
    k = check_components(n_components, dim, n_used) or min(dim, n_used - 1)
    S_host = S.cpu().numpy()
    if not np.isfinite(S_host).all():
        raise ValueError("the scatter matrix holds a non-finite value: an fp32 product of two centred values (or "
                         "a slab's sum of them) overflowed; scale X down")
    lam, vec = np.linalg.eigh(S_host / (n_used - 1))
    order = np.argsort(-lam, kind="stable")
    lam = np.maximum(lam[order], 0.0)
    V = fix_signs(vec[:, order].T[:k])
    total = float(lam.sum())
    ev = lam[:k].copy()
    dev = X.device
    centre = mean.float() if center else torch.zeros(dim, dtype=torch.float32, device=dev)
    return PCAResult(torch.from_numpy(V.astype(np.float32)).to(dev), centre, torch.from_numpy(ev),
                     torch.from_numpy(ev / total if total > 0 else np.zeros_like(ev)),
                     torch.from_numpy(np.sqrt(ev * (n_used - 1))), total, n_used, bool(unit), bool(whiten))


def projection(result: PCAResult) -> Tuple[torch.Tensor, torch.Tensor]:
    """(W fp32 [k, dim], b fp32 [k]) of transform(): W = components, b[j] = -float32(sum_d mean[d] V[j][d] in
    float64); whiten: both scaled by 1 / sqrt(explained_variance[j]) in float64, 0 for a zero eigenvalue"""
    V = result.components.double().cpu()
    b = -(V * result.mean.double().cpu()[None, :]).sum(1)
    if result.whiten:
        lam = result.explained_variance.double().cpu()
        scale = torch.where(lam > 0, 1.0 / torch.sqrt(lam.clamp(min=1e-300)), torch.zeros_like(lam))
        V, b = V * scale[:, None], b * scale
    dev = result.components.device
    return V.float().to(dev), b.float().to(dev)


def transform(X: torch.Tensor, result: PCAResult, inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n, k]: the rows of X on the components, classify.decision_function(X, W, b) with projection()'s W and
    b.  A unit result scores with b = 0 and applies `* inv_norm[:, None] + b` to the [n, k] scores in torch
    (inv_norm: computed when not given).  A row the fit skipped comes out as the arithmetic gives: NaN."""
    from node2vec_amd import classify

    n, dim = _dense.shape(X)
    if not isinstance(result, PCAResult) or result.components.ndim != 2 or result.components.shape[1] != dim:
        raise ValueError(f"result must be a PCAResult whose components are [k, {dim}]")
    _dense.check_inv_norm(n, inv_norm if result.unit else None)
    X = _dense.matrix(X)
    W, b = projection(result)
    if not result.unit:
        return classify.decision_function(X, W, b)
    norms = _dense.norms(X, inv_norm)
    return classify.decision_function(X, W, torch.zeros_like(b)) * norms[:, None] + b
