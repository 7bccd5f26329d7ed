"""Shared by tests/test_silhouette_host.py and tests/test_silhouette_gpu.py: the CPU restatement of
csrc/n2v_silhouette.hip (tests/cpu_silhouette/n2v_silhouette_cpu.c) behind numpy, a brute-force float64 silhouette,
the rounding bounds of the fp32 distances, and the case builders."""
import ctypes as C
from typing import NamedTuple

import numpy as np

import cpu_build
from pca_cases import same_bits  # noqa: F401  (bit for bit in fp64, a NaN equals any NaN)

METRICS = {"euclidean": 0, "cosine": 1}
P = C.c_void_p
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


class Sil(NamedTuple):
    s: np.ndarray
    a: np.ndarray
    b: np.ndarray
    nearest: np.ndarray
    counts: np.ndarray
    sums: np.ndarray  # [m, k] S(i, c), or None


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_silhouette/n2v_silhouette_cpu.c", out_dir)
    L.n2v_silhouette_cpu_dot.restype = C.c_float
    L.n2v_silhouette_cpu_dot.argtypes = [P, P, C.c_int32]
    L.n2v_silhouette_cpu_inv_norms.restype = None
    L.n2v_silhouette_cpu_inv_norms.argtypes = [P, C.c_int64, C.c_int32, P]
    L.n2v_silhouette_cpu_dist.restype = C.c_float
    L.n2v_silhouette_cpu_dist.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    L.n2v_silhouette_cpu_list.restype = C.c_int64
    L.n2v_silhouette_cpu_list.argtypes = [P, C.c_int64, C.c_int32, P, P, P]
    L.n2v_silhouette_cpu.restype = None
    L.n2v_silhouette_cpu.argtypes = [P, P, C.c_int64, C.c_int32, P, C.c_int32, C.c_int32, P, C.c_int64, P, P, P, P,
                                     P, P, P, P, P]
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _p(a):
    return None if a is None else a.ctypes.data


def inv_norms(L, X) -> np.ndarray:
    X = _f32(X)
    out = np.empty(X.shape[0], np.float32)
    L.n2v_silhouette_cpu_inv_norms(X.ctypes.data, X.shape[0], X.shape[1], out.ctypes.data)
    return out


def row_list(L, labels, k):
    """-> (counts [k], seg_off [k + 1], list [seg_off[k]])"""
    labels = np.ascontiguousarray(labels, np.int32)
    n = labels.shape[0]
    counts, seg_off, lst = np.empty(k, np.int64), np.empty(k + 1, np.int64), np.empty(n + 16 * k, np.int32)
    end = L.n2v_silhouette_cpu_list(labels.ctypes.data, n, k, counts.ctypes.data, seg_off.ctypes.data,
                                    lst.ctypes.data)
    return counts, seg_off, lst[:end]


def restated(L, X, labels, k, metric, rows=None, inv=None, sums=False) -> Sil:
    X = _f32(X)
    n, dim = X.shape
    labels = np.ascontiguousarray(labels, np.int32)
    if metric == "cosine" and inv is None:
        inv = inv_norms(L, X)
    inv = None if inv is None else _f32(inv)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    m = n if rows is None else rows.shape[0]
    a, b, s = np.empty(m, np.float64), np.empty(m, np.float64), np.empty(m, np.float64)
    nearest, counts = np.empty(m, np.int32), np.empty(k, np.int64)
    xn, seg_off, lst = np.empty(max(n, 1), np.float32), np.empty(k + 1, np.int64), np.empty(n + 16 * k, np.int32)
    S = np.empty((m, k), np.float64) if sums else None
    L.n2v_silhouette_cpu(X.ctypes.data, _p(inv), n, dim, labels.ctypes.data, k, METRICS[metric], _p(rows), m,
                         a.ctypes.data, b.ctypes.data, s.ctypes.data, nearest.ctypes.data, counts.ctypes.data,
                         xn.ctypes.data, seg_off.ctypes.data, lst.ctypes.data, _p(S))
    return Sil(s, a, b, nearest, counts, S)


def distances64(X, metric) -> np.ndarray:
    """float64 [n, n]"""
    X64 = np.asarray(X, np.float64)
    if metric == "euclidean":
        diff = X64[:, None, :] - X64[None, :, :]
        return np.sqrt((diff ** 2).sum(2))
    norm = np.sqrt((X64 ** 2).sum(1))
    inv = np.divide(1.0, norm, out=np.zeros_like(norm), where=norm > 0)
    return 1.0 - (X64 @ X64.T) * inv[:, None] * inv[None, :]


def brute(X, labels, k, metric):
    """the definition in float64 numpy -> (s, a, b, nearest, means [n, k] (NaN: not a candidate), D)"""
    D = distances64(X, metric)
    labels = np.asarray(labels)
    n = len(labels)
    member = (labels >= 0) & (labels < k)
    counts = np.bincount(labels[member], minlength=k)
    a, b, s = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    nearest = np.full(n, -1, np.int32)
    means = np.full((n, k), np.nan)
    for i in range(n):
        if not member[i]:
            continue
        L = labels[i]
        others = (labels == L) & (np.arange(n) != i)
        a[i] = D[i, others].sum() / (counts[L] - 1) if counts[L] > 1 else 0.0
        b[i] = np.inf
        for c in range(k):
            if c == L or counts[c] == 0:
                continue
            means[i, c] = D[i, labels == c].sum() / counts[c]
            if means[i, c] < b[i]:
                b[i], nearest[i] = means[i, c], c
        mx = max(a[i], b[i])
        s[i] = 0.0 if counts[L] == 1 or nearest[i] < 0 or mx == 0.0 else (b[i] - a[i]) / mx
    return s, a, b, nearest, means, D


def distance_bound(X, metric, D) -> np.ndarray:
    """[n, n]: what |d_fp32(i, j) - d(i, j)| cannot exceed, from the unit roundoff U = 2^-24 alone.

    Euclidean.  u' = fl(fl(xn_i - 2 dot) + xn_j): the dot is a chain of dim_pad fmaf (Higham 3.1), xn a sum of dim
    terms in some order, two more roundings: |u' - u| <= gamma_(dim_pad + 2) (2 sum |x_i x_j| + |x_i|^2 + |x_j|^2)
    = E2.  For u > 0, u' >= 0 (the fmaxf): |sqrt u' - sqrt u| <= |u' - u| / sqrt u; the rounding of the square root
    adds U times its value: E = E2 / d + U (d + E2 / d).  The bound needs d > 0: the cases keep the rows apart.
    Cosine.  1 - dot inv_i inv_j: inv carries gamma_(dim + 8) (sum of squares, square root, division), the dot
    gamma_dim_pad sum |x_i x_j| <= gamma_dim_pad |x_i| |x_j| (Cauchy-Schwarz), two products and one subtraction
    of a value below 2 four more roundings: E <= gamma_(dim_pad + 2 (dim + 8) + 4) (|cos| + A) with
    A = sum |x_i x_j| / (|x_i| |x_j|) <= 1; E = 2 gamma_(..) is used."""
    X64 = np.asarray(X, np.float64)
    dim = X64.shape[1]
    dp = (dim + 15) // 16 * 16
    if metric == "cosine":
        return np.full(D.shape, 2.0 * gamma(dp + 2 * (dim + 8) + 4))
    sq = (X64 ** 2).sum(1)
    E2 = gamma(dp + 2) * (2.0 * (np.abs(X64) @ np.abs(X64).T) + sq[:, None] + sq[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        E = E2 / D + U * (D + E2 / D)
    np.fill_diagonal(E, 0.0)  # j == i is skipped by index
    return E


def mean_bounds(E, labels, k) -> np.ndarray:
    """[n, k]: the bound on row i's mean distance to cluster c (its own: over the other rows): the mean of the
    distances' bounds; the fp64 chain of at most n additions and the division add (n + 1) 2^-53 relative, which a
    factor 1 + 2^-40 covers"""
    labels = np.asarray(labels)
    n = len(labels)
    out = np.zeros((n, k))
    for c in range(k):
        col = labels == c
        cnt = int(col.sum())
        if cnt == 0:
            continue
        tot = E[:, col].sum(1)
        own = col  # rows of c: the diagonal term is 0 and the divisor cnt - 1
        out[:, c] = tot / cnt
        if cnt > 1:
            out[own, c] = tot[own] / (cnt - 1)
    return out * (1.0 + 2.0 ** -40)


def lattice_case(n, dim, k, seed, noise=0.1):
    """n rows at least 0.5 apart: distinct integer lattice points, each moved by a vector of length < 0.25;
    labels: the nearest of k random lattice rows, a tenth of them redrawn -> (X fp32, labels int32).  (The fp32
    rounding of a coordinate moves a row by far less than the 0.5 claimed: asserted by the tests that use it.)"""
    rng = np.random.default_rng(seed)
    R = max(3, int(np.ceil((4.0 * n) ** (1.0 / dim) / 2.0)))
    seen, pts = set(), []
    while len(pts) < n:
        p = tuple(int(v) for v in rng.integers(-R, R + 1, dim))
        if p not in seen:
            seen.add(p)
            pts.append(p)
    X = np.array(pts, np.float64)
    step = rng.standard_normal((n, dim))
    step *= (rng.random(n) * 0.24 / np.sqrt((step ** 2).sum(1)))[:, None]
    X = (X + step).astype(np.float32)
    centres = X[rng.choice(n, k, replace=False)].astype(np.float64)
    d2 = ((X.astype(np.float64)[:, None, :] - centres[None, :, :]) ** 2).sum(2)
    labels = d2.argmin(1).astype(np.int32)
    redraw = rng.random(n) < noise
    labels[redraw] = rng.integers(0, k, int(redraw.sum()))
    return X, labels


def normal_case(n, dim, k, seed):
    """seeded normal rows, random labels in [0, k) -> (X, labels)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.integers(0, k, n).astype(np.int32)


def sized_labels(sizes, extra_none=0, seed=0):
    """labels with exactly sizes[c] rows of cluster c and extra_none rows of label -1, shuffled"""
    labels = np.concatenate([np.full(s, c, np.int32) for c, s in enumerate(sizes)] +
                            [np.full(extra_none, -1, np.int32)])
    np.random.default_rng(seed).shuffle(labels)
    return labels
