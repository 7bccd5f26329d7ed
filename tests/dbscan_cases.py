"""Shared by tests/test_dbscan_host.py and tests/test_dbscan_gpu.py: the CPU restatement of csrc/n2v_dbscan.hip
(tests/cpu_dbscan/n2v_dbscan_cpu.c) behind numpy, a brute-force float64 DBSCAN by the canonical rule, scikit-learn's
brute-force DBSCAN, and the case builders.  Every builder of a "gapped" case asserts, in float64, that no pairwise
distance lies within a relative 1e-4 of eps: scikit-learn, the float64 brute force and the fp32 kernel then agree on
the set of pairs within eps, and so -- the result being a function of that set -- on every label."""
import ctypes as C
from typing import NamedTuple

import numpy as np

import cpu_build

METRICS = {"euclidean": 0, "cosine": 1}
P = C.c_void_p
GAP = 1e-4


class Db(NamedTuple):
    labels: np.ndarray  # int32 [n], -1: noise
    core: np.ndarray    # bool [n]
    counts: np.ndarray  # int32 [n]
    n_clusters: int


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_dbscan/n2v_dbscan_cpu.c", out_dir)
    L.n2v_dbscan_cpu_dot.restype = C.c_float
    L.n2v_dbscan_cpu_dot.argtypes = [P, P, C.c_int32]
    L.n2v_dbscan_cpu_sumsq.restype = None
    L.n2v_dbscan_cpu_sumsq.argtypes = [P, C.c_int64, C.c_int32, P]
    L.n2v_dbscan_cpu_inv_norms.restype = None
    L.n2v_dbscan_cpu_inv_norms.argtypes = [P, C.c_int64, C.c_int32, P]
    L.n2v_dbscan_cpu_within.restype = C.c_int32
    L.n2v_dbscan_cpu_within.argtypes = [P, P, C.c_int32, C.c_int32, C.c_float, C.c_int64, C.c_int64]
    L.n2v_dbscan_cpu.restype = C.c_int32
    L.n2v_dbscan_cpu.argtypes = [P, P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, P, P, P]
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def inv_norms(L, X) -> np.ndarray:
    X = _f32(X)
    out = np.empty(X.shape[0], np.float32)
    L.n2v_dbscan_cpu_inv_norms(X.ctypes.data, X.shape[0], X.shape[1], out.ctypes.data)
    return out


def sumsq(L, X) -> np.ndarray:
    X = _f32(X)
    out = np.empty(X.shape[0], np.float32)
    L.n2v_dbscan_cpu_sumsq(X.ctypes.data, X.shape[0], X.shape[1], out.ctypes.data)
    return out


def restated(L, X, eps, min_samples, metric, inv=None) -> Db:
    X = _f32(X)
    n, dim = X.shape
    if metric == "cosine" and inv is None:
        inv = inv_norms(L, X)
    inv = None if inv is None else _f32(inv)
    counts, core, labels = np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.int32)
    k = L.n2v_dbscan_cpu(X.ctypes.data, None if inv is None else inv.ctypes.data, n, dim, METRICS[metric],
                         float(np.float32(eps)), int(min_samples), counts.ctypes.data, core.ctypes.data,
                         labels.ctypes.data)
    assert k >= 0
    return Db(labels, core.astype(bool), counts, int(k))


def distances64(X, metric) -> np.ndarray:
    """float64 [n, n]: Euclidean distances (from the differences, nothing cancels) or 1 - cosine"""
    X64 = np.asarray(X, np.float64)
    if metric == "euclidean":
        sq = (X64 ** 2).sum(1)
        D2 = sq[:, None] + sq[None, :] - 2.0 * (X64 @ X64.T)
        if X64.shape[0] * X64.shape[0] * X64.shape[1] <= 1 << 24:  # small: the differences themselves
            D2 = ((X64[:, None, :] - X64[None, :, :]) ** 2).sum(2)
        return np.sqrt(np.maximum(D2, 0.0))
    norm = np.sqrt((X64 ** 2).sum(1))
    inv = np.divide(1.0, norm, out=np.zeros_like(norm), where=norm > 0)
    return 1.0 - (X64 @ X64.T) * inv[:, None] * inv[None, :]


def canonical(within, min_samples) -> Db:
    """the canonical result from a boolean [n, n] "within eps" matrix (its diagonal is taken as True)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    A = np.array(within, bool)
    n = A.shape[0]
    np.fill_diagonal(A, True)
    counts = A.sum(1).astype(np.int32)
    core = counts >= min_samples
    labels = np.full(n, -1, np.int32)
    idx = np.nonzero(core)[0]
    k = 0
    if len(idx):
        k, comp = connected_components(csr_matrix(A[np.ix_(idx, idx)]), directed=False)
        first = np.full(k, n)
        np.minimum.at(first, comp, idx)                 # a component's lowest core row
        rank = np.empty(k, np.int64)
        rank[np.argsort(first)] = np.arange(k)          # clusters numbered by it
        labels[idx] = rank[comp]
        for b in np.nonzero(~core)[0]:
            near = idx[A[b, idx]]
            if len(near):
                labels[b] = labels[near].min()
    return Db(labels, core, counts, int(k))


def brute(X, eps, min_samples, metric) -> Db:
    """float64 numpy DBSCAN: eps as the fp32 value the kernels take"""
    return canonical(distances64(X, metric) <= float(np.float32(eps)), min_samples)


def sklearn_dbscan(X, eps, min_samples, metric):
    """(labels, core mask) of sklearn.cluster.DBSCAN(algorithm="brute") on the float64 rows"""
    from sklearn.cluster import DBSCAN

    m = DBSCAN(eps=float(np.float32(eps)), min_samples=int(min_samples), metric=metric, algorithm="brute")
    m.fit(np.asarray(X, np.float64))
    core = np.zeros(len(X), bool)
    core[m.core_sample_indices_] = True
    return m.labels_.astype(np.int32), core


def assert_gapped(X, eps, metric):
    """the inputs' own property, in float64: no pair within a relative GAP of eps"""
    D = distances64(X, metric)
    e = float(np.float32(eps))
    off = ~np.eye(len(X), dtype=bool)
    closest = np.abs(D[off] - e).min() if len(X) > 1 else np.inf
    assert closest > GAP * e, (closest, e)


def dyadic_blobs(n_blob, n_noise, dim, seed, eps2_steps, quantum=1.0 / 16, sigma=0.25, spread=4.0):
    """three Gaussian blobs of n_blob rows and n_noise rows of noise (half of them a wider halo around the blobs, half
    uniform), shuffled, every coordinate a multiple of
    `quantum` inside [-spread - 2, spread + 2]: every squared distance is then a multiple of quantum^2 (and exact in
    fp32), and eps^2 = (eps2_steps + 0.5) quantum^2 sits half a step from all of them -- gapped by construction,
    asserted all the same.  -> (X fp32, eps)"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, dim))
    centres[0, 0], centres[1, 0], centres[2, min(1, dim - 1)] = -spread, spread, spread * (1.0 if dim > 1 else 0.0)
    rows = [centres[c] + sigma * rng.standard_normal((n_blob, dim)) for c in range(3)]
    halo = n_noise // 2  # rows around the blobs, a little wider than they are: border rows and near misses
    rows.append(centres[rng.integers(0, 3, halo)] + 1.25 * sigma * rng.standard_normal((halo, dim)))
    rows.append(rng.uniform(-spread - 1.0, spread + 1.0, (n_noise - halo, dim)))
    X = np.concatenate(rows)
    X = (np.round(X / quantum) * quantum)[rng.permutation(len(X))].astype(np.float32)
    eps = float(np.float32(np.sqrt((eps2_steps + 0.5) * quantum * quantum)))
    assert_gapped(X, eps, "euclidean")
    return X, eps


def cosine_blobs(n_blob, n_noise, dim, seed, eps0, sigma=0.05):
    """three bundles of directions and n_noise random directions, of assorted lengths, shuffled; eps: the first of
    eps0 (1 + 3e-4 t), t = 0, 1, .., that is gapped -> (X fp32, eps)"""
    rng = np.random.default_rng(seed)
    axes = rng.standard_normal((3, dim))
    axes /= np.sqrt((axes ** 2).sum(1))[:, None]
    rows = [axes[c] + sigma * rng.standard_normal((n_blob, dim)) / np.sqrt(dim) * 4.0 for c in range(3)]
    rows.append(rng.standard_normal((n_noise, dim)))
    X = np.concatenate(rows)
    X *= rng.uniform(0.5, 2.0, len(X))[:, None]
    X = X[rng.permutation(len(X))].astype(np.float32)
    D = distances64(X, "cosine")
    np.fill_diagonal(D, np.inf)
    near = D[np.abs(D - eps0) < 0.1 * eps0]  # the distances any of the candidates can be close to
    for t in range(200):
        eps = float(np.float32(eps0 * (1.0 + 3e-4 * t)))
        if near.size == 0 or np.abs(near - eps).min() > GAP * eps:
            return X, eps
    raise AssertionError("no gapped eps near %g" % eps0)


def grid_case(n, dim, side, seed):
    """n rows of small integer coordinates in [0, side): every distance is exact in fp32, and with eps in {1, 2}
    many lie exactly on the boundary d2 == eps2"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, side, (n, dim)).astype(np.float32)


# Border rows between clusters whose numbering does not follow the rows' order; in the second case a border row's
# lowest-index core neighbour belongs to the HIGHER-numbered cluster: "the cluster of the lowest core neighbour" would
# be the wrong rule.  (X, eps, min_samples, labels)
CONTESTED = [
    (np.array([[0, 0], [10, 0], [10, 1], [11, 0], [3, 0], [3, 1], [3, -1], [2, 0], [1.5, 0], [8.5, 0], [9, 0]],
              np.float32), 1.0, 3, [-1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0]),
    # a line, x = .5 3.5 1.5 2.5 0 1 4 4.5 5: row 3 (x = 2.5) has three rows within 1 and is not core; its core
    # neighbours are row 1 (x = 3.5, cluster 1) and row 2 (x = 1.5, cluster 0), both at exactly eps
    (np.array([[.5, 0], [3.5, 0], [1.5, 0], [2.5, 0], [0, 0], [1, 0], [4, 0], [4.5, 0], [5, 0]], np.float32), 1.0, 4,
     [0, 1, 0, 0, 0, 0, 1, 1, 1]),
]


def lowest_neighbour_rule(X, eps, min_samples):
    """the WRONG border rule, for showing that a case tells the two apart: the cluster of the lowest core neighbour"""
    D = distances64(X, "euclidean") <= eps
    good = canonical(D, min_samples)
    labels = good.labels.copy()
    for b in np.nonzero(~good.core)[0]:
        near = np.nonzero(D[b] & good.core)[0]
        labels[b] = good.labels[near[0]] if len(near) else -1
    return labels


def chain(n=700, dim=4, interleaved=False):
    """n points at integer positions on a line in dim dimensions (along the second axis), every gap exactly 1.
    interleaved: two lines 1000 apart, even rows on one and odd rows on the other."""
    X = np.zeros((n, dim), np.float32)
    if interleaved:
        X[:, 1] = np.arange(n) // 2
        X[1::2, 0] = 1000.0
    else:
        X[:, 1] = np.arange(n)
    return X
