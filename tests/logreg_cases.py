"""Shared by tests/test_classify_host.py and tests/test_classify_gpu.py: the CPU restatement of
csrc/n2v_logreg.hip (tests/cpu_logreg/n2v_logreg_cpu.c) behind numpy, a float64 numpy reference (loss, gradient, a
per-class Newton solver) and the case builders."""
import ctypes as C

import numpy as np

import cpu_build

P = C.c_void_p


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_logreg/n2v_logreg_cpu.c", out_dir)
    L.n2v_logreg_cpu_exp_neg.restype = C.c_float
    L.n2v_logreg_cpu_exp_neg.argtypes = [C.c_float]
    L.n2v_logreg_cpu_log1p01.restype = C.c_float
    L.n2v_logreg_cpu_log1p01.argtypes = [C.c_float]
    L.n2v_logreg_cpu_points.restype = None
    L.n2v_logreg_cpu_points.argtypes = [P, C.c_int64, C.c_int32, P]
    L.n2v_logreg_cpu_dot.restype = C.c_float
    L.n2v_logreg_cpu_dot.argtypes = [P, P, C.c_int32]
    L.n2v_logreg_cpu_slab_rows.restype = C.c_int64
    L.n2v_logreg_cpu_slab_rows.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.n2v_logreg_cpu_scores.restype = None
    L.n2v_logreg_cpu_scores.argtypes = [P, C.c_int64, C.c_int32, P, P, C.c_int32, P]
    L.n2v_logreg_cpu_loss_grad.restype = None
    L.n2v_logreg_cpu_loss_grad.argtypes = [P, P, C.c_int64, C.c_int32, P, P, C.c_int32, P, P, P, P, P]
    return L


def same_bits(got, want) -> bool:
    """equal bit for bit in their own precision (float32 or float64, the same for both), signed zeros included; a
    NaN equals any NaN (its payload is not part of the contract)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.dtype not in (np.float32, np.float64) or got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        return False
    word = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.array_equal(got.view(word)[~nan_g], want.view(word)[~nan_w])


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def points(L, z, y):
    """the spelled functions at every z, label y -> float32 [len(z), 4]: e = exp(-|z|), p, res, l"""
    z = _f32(z)
    out = np.empty((z.size, 4), np.float32)
    L.n2v_logreg_cpu_points(z.ctypes.data, z.size, int(y), out.ctypes.data)
    return out


def slab_rows(L, n, dim, c) -> int:
    return int(L.n2v_logreg_cpu_slab_rows(n, dim, c))


def pack(Y) -> np.ndarray:
    """bool [n, c] -> uint32 [n, ceil(c / 32)]: bit j of word w is class 32 w + j"""
    Y = np.asarray(Y) != 0
    n, c = Y.shape
    words = (c + 31) // 32
    bits = np.zeros((n, words * 32), np.uint64)
    bits[:, :c] = Y
    return (bits.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def scores(L, X, W, b) -> np.ndarray:
    X, W, b = _f32(X), _f32(W), _f32(b)
    Z = np.empty((X.shape[0], W.shape[0]), np.float32)
    L.n2v_logreg_cpu_scores(X.ctypes.data, X.shape[0], X.shape[1], W.ctypes.data, b.ctypes.data, W.shape[0],
                            Z.ctypes.data)
    return Z


def loss_grad(L, X, Y, W, b):
    """-> (loss float64 [1], gW float64 [c, dim], gb float64 [c])"""
    X, W, b = _f32(X), _f32(W), _f32(b)
    yb = np.ascontiguousarray(pack(Y))
    c, dim = W.shape
    loss, gW, gb = np.empty(1, np.float64), np.empty((c, dim), np.float64), np.empty(c, np.float64)
    part, res = np.empty(c * dim, np.float32), np.empty(c, np.float32)
    L.n2v_logreg_cpu_loss_grad(X.ctypes.data, yb.ctypes.data, X.shape[0], dim, W.ctypes.data, b.ctypes.data, c,
                               loss.ctypes.data, gW.ctypes.data, gb.ctypes.data, part.ctypes.data, res.ctypes.data)
    return loss, gW, gb


def torch_loss_grad_fn(L, X, Y):
    """classify.fit's loss_grad_fn on the restatement (CPU tensors)"""
    import torch

    def fn(W, b):
        loss, gW, gb = loss_grad(L, X, Y, W.numpy(), b.numpy())
        return torch.from_numpy(loss), torch.from_numpy(gW), torch.from_numpy(gb)
    return fn


# ---- the float64 reference

def ref_loss_grad(X, Y, W, b):
    """float64 numpy: (sum of the logistic losses, gW, gb, |terms| sums for the bounds)"""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    Yf = (np.asarray(Y) != 0).astype(np.float64)
    Z = X @ W.T + b
    loss = np.logaddexp(0.0, np.where(Yf > 0, -Z, Z))
    Pm = np.exp(-np.logaddexp(0.0, -Z))
    R = Pm - Yf
    return loss.sum(), R.T @ X, R.sum(0), Z, R


def newton(X, Y, C=1.0, tol=1e-12, max_iter=200):
    """per class, Newton's method on sum l + |w|^2 / (2 C) (bias free) in float64 to max |grad| <= tol"""
    X = np.asarray(X, np.float64)
    n, dim = X.shape
    Yf = (np.asarray(Y) != 0).astype(np.float64)
    A = np.hstack([X, np.ones((n, 1))])
    reg = np.diag(np.r_[np.full(dim, 1.0 / C), 0.0])
    out = np.zeros((Yf.shape[1], dim + 1))
    for k in range(Yf.shape[1]):
        th = np.zeros(dim + 1)
        for _ in range(max_iter):
            z = A @ th
            p = np.exp(-np.logaddexp(0.0, -z))
            g = A.T @ (p - Yf[:, k]) + reg @ th
            if np.abs(g).max() <= tol:
                break
            H = (A * (p * (1 - p))[:, None]).T @ A + reg
            step = np.linalg.solve(H, g)
            f0 = np.logaddexp(0.0, np.where(Yf[:, k] > 0, -z, z)).sum() + 0.5 * th @ reg @ th
            t = 1.0
            while True:  # damped: never raise the objective
                z1 = A @ (th - t * step)
                th1 = th - t * step
                f1 = np.logaddexp(0.0, np.where(Yf[:, k] > 0, -z1, z1)).sum() + 0.5 * th1 @ reg @ th1
                if f1 <= f0 or t < 1e-10:
                    break
                t *= 0.5
            th = th - t * step
        else:
            raise AssertionError(f"Newton did not reach {tol} for class {k}")
        out[k] = th
    return out[:, :dim], out[:, dim]


# ---- cases

def normal_case(n, dim, c, seed, scale=0.5):
    """seeded normal rows, weights, biases and labels"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    W = (rng.standard_normal((c, dim)) * scale).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    Y = rng.random((n, c)) < 0.3
    return X, W, b, Y


def planted(n=400, dim=8, c=3, seed=5, margin=2.0):
    """blobs whose labels are planted from a random W*: Y = (x . w* + b* + noise > 0)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((4, dim)) * 2.0
    X = (centres[rng.integers(0, 4, n)] + rng.standard_normal((n, dim))).astype(np.float32)
    Ws = rng.standard_normal((c, dim)) * margin
    bs = rng.standard_normal(c)
    Y = (X.astype(np.float64) @ Ws.T + bs + rng.logistic(size=(n, c))) > 0
    return X, Y
