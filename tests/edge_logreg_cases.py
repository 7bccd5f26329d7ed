"""Shared by tests/test_edge_logreg_host.py and tests/test_edge_logreg_gpu.py: the CPU restatement of
csrc/n2v_edge_logreg.hip (tests/cpu_edge_logreg/n2v_edge_logreg_cpu.c) behind numpy, a float64 numpy reference on the
materialised features and the case builders."""
import ctypes as C

import numpy as np

import cpu_build
import logreg_cases as lc
import pairs_cases as pc

P = C.c_void_p
OPS = pc.OPS
same_bits = lc.same_bits


def build(out_dir) -> C.CDLL:
    """the restatement (it holds the two older ones: their functions are set up as lc.build and pc.build do)"""
    L = cpu_build.build("cpu_edge_logreg/n2v_edge_logreg_cpu.c", out_dir)
    L.n2v_pairs_cpu_dot.restype = C.c_float
    L.n2v_pairs_cpu_dot.argtypes = [P, P, C.c_int32]
    L.n2v_pairs_cpu_features.restype = None
    L.n2v_pairs_cpu_features.argtypes = [P, C.c_int64, C.c_int32, P, P, C.c_int64, C.c_int32, P]
    L.n2v_logreg_cpu_slab_rows.restype = C.c_int64
    L.n2v_logreg_cpu_slab_rows.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.n2v_edge_logreg_cpu_slab_pairs.restype = C.c_int64
    L.n2v_edge_logreg_cpu_slab_pairs.argtypes = [C.c_int64, C.c_int32]
    L.n2v_edge_logreg_cpu_scores.restype = None
    L.n2v_edge_logreg_cpu_scores.argtypes = [P, C.c_int64, C.c_int32, P, P, C.c_int64, C.c_int32, P, C.c_float, P]
    L.n2v_edge_logreg_cpu_loss_grad.restype = None
    L.n2v_edge_logreg_cpu_loss_grad.argtypes = [P, C.c_int64, C.c_int32, P, P, P, C.c_int64, C.c_int32, P, C.c_float,
                                                P, P, P]
    return L


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _i64(x):
    return np.ascontiguousarray(x, np.int64)


def slab_pairs(L, n_pairs, dim) -> int:
    return int(L.n2v_edge_logreg_cpu_slab_pairs(n_pairs, dim))


def lane_groups(dim) -> int:
    """P of the restatement: pairs side by side in a wave"""
    return 64 // (16 if dim <= 128 else 32 if dim <= 256 else 64)


def features(L, X, a, b, op) -> np.ndarray:
    return pc.features(L, X, a, b, op)


def scores(L, X, a, b, w, b0, op) -> np.ndarray:
    X, w, a, b = _f32(X), _f32(w), _i64(a), _i64(b)
    z = np.empty(a.shape[0], np.float32)
    L.n2v_edge_logreg_cpu_scores(X.ctypes.data, X.shape[0], X.shape[1], a.ctypes.data, b.ctypes.data, a.shape[0],
                                 OPS[op], w.ctypes.data, float(np.float32(b0)), z.ctypes.data)
    return z


def loss_grad(L, X, a, b, y, w, b0, op):
    """-> (loss float64 [1], gw float64 [dim], gb float64 [1])"""
    X, w, a, b = _f32(X), _f32(w), _i64(a), _i64(b)
    y = np.ascontiguousarray(np.asarray(y) != 0, np.uint8)
    dim = X.shape[1]
    loss, gw, gb = np.empty(1, np.float64), np.empty(dim, np.float64), np.empty(1, np.float64)
    L.n2v_edge_logreg_cpu_loss_grad(X.ctypes.data, X.shape[0], dim, a.ctypes.data, b.ctypes.data, y.ctypes.data,
                                    a.shape[0], OPS[op], w.ctypes.data, float(np.float32(b0)), loss.ctypes.data,
                                    gw.ctypes.data, gb.ctypes.data)
    return loss, gw, gb


def torch_loss_grad_fn(L, X, a, b, y, op):
    """linkpred.fit_edges' loss_grad_fn on the restatement (CPU tensors; w arrives as [1, dim], b as [1])"""
    import torch

    def fn(w, b0):
        loss, gw, gb = loss_grad(L, X, a, b, y, w.numpy().reshape(-1), b0.numpy().reshape(-1)[0], op)
        return torch.from_numpy(loss), torch.from_numpy(gw), torch.from_numpy(gb)
    return fn


# ---- the float64 reference, on the materialised features

def ref_loss_grad(F, y, w, b0):
    """F: the feature rows.  -> what lc.ref_loss_grad returns, for one class"""
    return lc.ref_loss_grad(F, np.asarray(y).reshape(-1, 1), np.asarray(w).reshape(1, -1), np.array([b0]))


# ---- cases

def normal_case(rows, dim, n_pairs, seed, scale=0.5):
    """seeded normal rows, random pairs (with repeats and a == b), weights, a bias and labels"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    a, b = rng.integers(0, rows, n_pairs), rng.integers(0, rows, n_pairs)
    a[:3], b[:3] = (1, 2, 2), (1, 3, 3)
    w = (rng.standard_normal(dim) * scale).astype(np.float32)
    b0 = np.float32(rng.standard_normal())
    y = rng.random(n_pairs) < 0.4
    return X, a.astype(np.int64), b.astype(np.int64), y, w, b0


def planted(rows=60, dim=8, n_pairs=400, seed=5, margin=2.0, op="hadamard"):
    """pairs over seeded rows whose labels are planted from a random w*: y = (f . w* + b* + logistic noise > 0), as
    logreg_cases.planted plants its classes"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    a, b = rng.integers(0, rows, n_pairs).astype(np.int64), rng.integers(0, rows, n_pairs).astype(np.int64)
    F = pc.numpy_features(X, a, b, op).astype(np.float64)
    ws = rng.standard_normal(dim) * margin
    bs = rng.standard_normal()
    y = (F @ ws + bs + rng.logistic(size=n_pairs)) > 0
    return X, a, b, y
