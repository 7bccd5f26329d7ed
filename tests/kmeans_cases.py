"""Shared by tests/test_cluster_host.py and tests/test_cluster_gpu.py: the CPU restatement of
csrc/n2v_kmeans.hip (tests/cpu_kmeans/n2v_kmeans_cpu.c) behind numpy, and the case builders."""
import ctypes as C

import numpy as np

import cpu_build
from pairs_cases import same_bits  # noqa: F401  (bit for bit, a NaN equals any NaN)

METRICS = {"euclidean": 0, "cosine": 1}
P = C.c_void_p


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_kmeans/n2v_kmeans_cpu.c", out_dir)
    L.n2v_kmeans_cpu_dot.restype = C.c_float
    L.n2v_kmeans_cpu_dot.argtypes = [P, P, C.c_int32]
    L.n2v_kmeans_cpu_sumsq.restype = C.c_float
    L.n2v_kmeans_cpu_sumsq.argtypes = [P, C.c_int32]
    L.n2v_kmeans_cpu_inv_norms.restype = None
    L.n2v_kmeans_cpu_inv_norms.argtypes = [P, C.c_int64, C.c_int32, P]
    L.n2v_kmeans_cpu_slab_rows.restype = C.c_int64
    L.n2v_kmeans_cpu_slab_rows.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.n2v_kmeans_cpu_assign.restype = None
    L.n2v_kmeans_cpu_assign.argtypes = [P, P, C.c_int64, C.c_int32, P, C.c_int32, C.c_int32, P, P]
    L.n2v_kmeans_cpu_update.restype = None
    L.n2v_kmeans_cpu_update.argtypes = [P, P, C.c_int64, C.c_int32, P, C.c_int32, C.c_int32, P, P, P, P, P]
    L.n2v_kmeans_cpu_step.restype = None
    L.n2v_kmeans_cpu_step.argtypes = [P, P, C.c_int64, C.c_int32, P, C.c_int32, C.c_int32, P, P, P, P, P, P, P, P]
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _inv(inv):
    return None if inv is None else _f32(inv)


def _p(a):
    return None if a is None else a.ctypes.data


def dot(L, c, x) -> np.float32:
    c, x = _f32(c), _f32(x)
    return np.float32(L.n2v_kmeans_cpu_dot(c.ctypes.data, x.ctypes.data, c.shape[0]))


def inv_norms(L, X) -> np.ndarray:
    X = _f32(X)
    out = np.empty(X.shape[0], np.float32)
    L.n2v_kmeans_cpu_inv_norms(X.ctypes.data, X.shape[0], X.shape[1], out.ctypes.data)
    return out


def unit(L, Cm) -> np.ndarray:
    Cm = _f32(Cm)
    return Cm * inv_norms(L, Cm)[:, None]


def slab_rows(L, n, dim, k) -> int:
    return int(L.n2v_kmeans_cpu_slab_rows(n, dim, k))


def assign(L, X, inv, Cm, metric):
    X, Cm, inv = _f32(X), _f32(Cm), _inv(inv)
    labels, dist = np.empty(X.shape[0], np.int32), np.empty(X.shape[0], np.float32)
    L.n2v_kmeans_cpu_assign(X.ctypes.data, _p(inv), X.shape[0], X.shape[1], Cm.ctypes.data, Cm.shape[0],
                            METRICS[metric], labels.ctypes.data, dist.ctypes.data)
    return labels, dist


def update(L, X, inv, labels, k, metric, prev):
    X, prev, inv = _f32(X), _f32(prev), _inv(inv)
    labels = np.ascontiguousarray(labels, np.int32)
    out, counts = np.empty_like(prev), np.empty(k, np.int64)
    part, total = np.empty(prev.size, np.float32), np.empty(prev.size, np.float64)
    L.n2v_kmeans_cpu_update(X.ctypes.data, _p(inv), X.shape[0], X.shape[1], labels.ctypes.data, k, METRICS[metric],
                            prev.ctypes.data, out.ctypes.data, counts.ctypes.data, part.ctypes.data,
                            total.ctypes.data)
    return out, counts


def step(L, X, inv, Cm, metric, labels):
    """-> (labels, dist, centroids, counts, [n_changed, n_unassigned]); `labels`: the previous ones"""
    X, Cm, inv = _f32(X), _f32(Cm), _inv(inv)
    labels = np.array(labels, np.int32)
    k = Cm.shape[0]
    dist, out, counts, stats = np.empty(X.shape[0], np.float32), np.empty_like(Cm), np.empty(k, np.int64), np.empty(2, np.int64)
    scratch, part, total = np.empty(X.shape[0], np.int32), np.empty(Cm.size, np.float32), np.empty(Cm.size, np.float64)
    L.n2v_kmeans_cpu_step(X.ctypes.data, _p(inv), X.shape[0], X.shape[1], Cm.ctypes.data, k, METRICS[metric],
                          labels.ctypes.data, dist.ctypes.data, out.ctypes.data, counts.ctypes.data,
                          stats.ctypes.data, scratch.ctypes.data, part.ctypes.data, total.ctypes.data)
    return labels, dist, out, counts, stats


def lloyd(L, X, inv, Cm, metric, max_iter=100):
    """cluster.kmeans' loop (tol = 0) on the restatement -> (centroids, labels, dist, n_iter, converged)"""
    labels = np.full(X.shape[0], -1, np.int32)
    Cm = _f32(Cm)
    for it in range(1, max_iter + 1):
        labels, dist, Cm, _, stats = step(L, X, inv, Cm, metric, labels)
        if stats[0] == 0:
            return Cm, labels, dist, it, True
    labels, dist = assign(L, X, inv, Cm, metric)
    return Cm, labels, dist, max_iter, False


def normal_case(n, dim, k, seed):
    """seeded normal rows and normal centroids: far from ties at dim >= 32"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((k, dim)).astype(np.float32)


def special_rows(dim, seed):
    """12 rows: -0.0, denormals and inf beside ordinary values, a zero row, a NaN row"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((12, dim)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e-39, 1.0, -1.0, 2.5, -0.5], np.float32)
    X[:5] = special[rng.integers(0, special.size, (5, dim))]
    X[5] = 0.0
    X[6] = -0.0
    X[7, rng.integers(dim)] = np.inf
    X[8, rng.integers(dim)] = -np.inf
    X[9] = np.nan
    X[10] *= np.float32(1e-20)  # products that are denormal
    return X


def blobs(n, dim, k, seed, spread=0.05):
    """k well separated planted blobs -> (X, planted labels, centres)"""
    rng = np.random.default_rng(seed)
    centres = (rng.standard_normal((k, dim)) * 4.0).astype(np.float32)
    planted = rng.integers(0, k, n).astype(np.int32)
    planted[:k] = np.arange(k)
    X = centres[planted] + (rng.standard_normal((n, dim)) * spread).astype(np.float32)
    return X.astype(np.float32), planted, centres
