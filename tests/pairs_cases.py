"""Shared by tests/test_linkpred_host.py and tests/test_linkpred_gpu.py: the CPU restatement of
csrc/n2v_pairs.hip (tests/cpu_pairs/n2v_pairs_cpu.c) behind numpy, and the comparisons the two files make."""
import ctypes as C

import numpy as np

import cpu_build

OPS = {"average": 0, "hadamard": 1, "l1": 2, "l2": 3}
METRICS = {"dot": 0, "cosine": 1}


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_pairs/n2v_pairs_cpu.c", out_dir)
    L.n2v_pairs_cpu_dot.restype = C.c_float
    L.n2v_pairs_cpu_dot.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.n2v_pairs_cpu_scores.restype = None
    L.n2v_pairs_cpu_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int32, C.c_void_p]
    L.n2v_pairs_cpu_features.restype = None
    L.n2v_pairs_cpu_features.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_void_p]
    return L


def dot(L, a, b) -> np.float32:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.float32(L.n2v_pairs_cpu_dot(a.ctypes.data, b.ctypes.data, a.shape[0]))


def scores(L, X, inv_norm, a, b, metric) -> np.ndarray:
    X = np.ascontiguousarray(X, np.float32)
    a, b = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)
    out = np.empty(a.shape[0], np.float32)
    inv = None if inv_norm is None else np.ascontiguousarray(inv_norm, np.float32)
    L.n2v_pairs_cpu_scores(X.ctypes.data, None if inv is None else inv.ctypes.data, X.shape[0], X.shape[1],
                           a.ctypes.data, b.ctypes.data, a.shape[0], METRICS[metric], out.ctypes.data)
    return out


def features(L, X, a, b, op) -> np.ndarray:
    X = np.ascontiguousarray(X, np.float32)
    a, b = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)
    out = np.empty((a.shape[0], X.shape[1]), np.float32)
    L.n2v_pairs_cpu_features(X.ctypes.data, X.shape[0], X.shape[1], a.ctypes.data, b.ctypes.data, a.shape[0],
                             OPS[op], out.ctypes.data)
    return out


def numpy_features(X, a, b, op) -> np.ndarray:
    """the four operators as numpy float32 expressions (every intermediate is float32)"""
    x, y = X[a].astype(np.float32), X[b].astype(np.float32)
    with np.errstate(all="ignore"):
        if op == "average":
            return (x + y) * np.float32(0.5)
        if op == "hadamard":
            return x * y
        if op == "l1":
            return np.abs(x - y)
        return (x - y) * (x - y)


def same_bits(got, want) -> bool:
    """equal bit for bit, signed zeros included; a NaN equals any NaN (its payload is not part of the contract)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        return False
    return np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w])


def auc_quadratic(pos, neg) -> float:
    """the O(P N) count, in float64"""
    p, n = np.asarray(pos, np.float64)[:, None], np.asarray(neg, np.float64)[None, :]
    return float(((p > n) + 0.5 * (p == n)).mean())
