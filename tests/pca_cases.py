"""Shared by tests/test_pca_host.py and tests/test_pca_gpu.py: the CPU restatement of csrc/n2v_pca.hip
(tests/cpu_pca/n2v_pca_cpu.c) behind numpy, a float64 numpy reference with the terms of the error bound, and the case
builders."""
import ctypes as C

import numpy as np

import cpu_build

P = C.c_void_p
U24 = 2.0 ** -24  # the unit roundoff of fp32


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_pca/n2v_pca_cpu.c", out_dir)
    L.n2v_pca_cpu_slab_rows.restype = C.c_int64
    L.n2v_pca_cpu_slab_rows.argtypes = [C.c_int64, C.c_int32]
    L.n2v_pca_cpu_mean.restype = None
    L.n2v_pca_cpu_mean.argtypes = [P, P, C.c_int64, C.c_int32, P, P]
    L.n2v_pca_cpu_scatter.restype = None
    L.n2v_pca_cpu_scatter.argtypes = [P, P, C.c_int64, C.c_int32, P, P, P]
    L.n2v_pca_cpu_scatter_slabs.restype = None
    L.n2v_pca_cpu_scatter_slabs.argtypes = [P, P, C.c_int32, P, P, C.c_int32, P, P]
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
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def slab_rows(L, n, dim) -> int:
    return int(L.n2v_pca_cpu_slab_rows(n, dim))


def mean(L, X, inv_norm=None):
    """-> (mean float64 [dim], n_used)"""
    X, inv_norm = _f32(X), _f32(inv_norm)
    out, used = np.empty(X.shape[1], np.float64), np.zeros(1, np.int64)
    L.n2v_pca_cpu_mean(X.ctypes.data, _ptr(inv_norm), X.shape[0], X.shape[1], out.ctypes.data, used.ctypes.data)
    return out, int(used[0])


def scatter(L, X, inv_norm=None, center=None, bounds=None):
    """-> (S float64 [dim, dim], n_used); bounds: the slabs' first rows and the end, instead of the plan's"""
    X, inv_norm, center = _f32(X), _f32(inv_norm), _f32(center)
    n, dim = X.shape
    S, used = np.empty((dim, dim), np.float64), np.zeros(1, np.int64)
    if bounds is None:
        L.n2v_pca_cpu_scatter(X.ctypes.data, _ptr(inv_norm), n, dim, _ptr(center), S.ctypes.data, used.ctypes.data)
    else:
        b = np.ascontiguousarray(bounds, np.int64)
        L.n2v_pca_cpu_scatter_slabs(X.ctypes.data, _ptr(inv_norm), dim, _ptr(center), b.ctypes.data, len(b) - 1,
                                    S.ctypes.data, used.ctypes.data)
    return S, int(used[0])


def moments(L, X, inv_norm=None, centered=True):
    """what node2vec_amd.pca.moments computes: the centre of the scatter pass is float32(mean)"""
    m, used = mean(L, X, inv_norm)
    S, used_s = scatter(L, X, inv_norm, m.astype(np.float32) if centered else None)
    assert used == used_s
    return m, S, used


# ---- the float64 reference

def scaled(X, inv_norm=None) -> np.ndarray:
    """xh in fp32: one multiply per element"""
    X = _f32(X)
    return X if inv_norm is None else X * _f32(inv_norm)[:, None]


def ref_scatter(X, inv_norm=None, center=None):
    """float64: (S64, A) around the SAME fp32 centre, over the rows whose xh are all finite: S64 = sum_r xc xc^T and
    A = sum_r |xc| |xc|^T with xc = (double)xh - (double)center unrounded"""
    xh = scaled(X, inv_norm)
    xh = xh[np.isfinite(xh).all(1)].astype(np.float64)
    xc = xh if center is None else xh - np.asarray(center, np.float32).astype(np.float64)
    return xc.T @ xc, np.abs(xc).T @ np.abs(xc)


def element_bound(A, slab_rows_) -> np.ndarray:
    """|S - S64| <= (slab_rows + 4) 2^-24 A, element by element: an fp32 fma chain of at most slab_rows terms
    (gamma_k ~ k u; the fp64 fold of the slabs adds 2048 2^-53, far below one more u), plus the rounding of the two
    centred factors of every product (2 u, and 2 u of slack for the second-order terms)"""
    return (slab_rows_ + 4) * U24 * A


# ---- cases

def normal_case(n, dim, seed, offset=0.5, with_norms=False):
    """seeded normal rows around `offset`; with_norms: also fp32 1 / |row| (computed in float64, rounded once: any
    fp32 vector serves as inv_norm)"""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dim)) + offset).astype(np.float32)
    inv = None
    if with_norms:
        inv = (1.0 / np.sqrt((X.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    return X, inv


def planted(n=4000, dim=24, seed=7):
    """three orthonormal directions with standard deviations 3, 2, 1, isotropic noise of 0.01, a mean of 0.5"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((dim, 3)))[0]
    Z = rng.standard_normal((n, 3)) * np.array([3.0, 2.0, 1.0])
    return (Z @ Q.T + 0.01 * rng.standard_normal((n, dim)) + 0.5).astype(np.float32)
