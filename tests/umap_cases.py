"""Shared by tests/test_umap_host.py and tests/test_umap_gpu.py: the CPU restatement of csrc/n2v_umap.hip
(tests/cpu_umap/n2v_umap_cpu.c) behind numpy, the counter-based draws and a float64 evaluation of the same law in
numpy, the sweeps of x^b, and the case builders."""
import ctypes as C

import numpy as np

import cpu_build
from tsne_cases import blobs, cosine_neighbours64, foreign_nearest, same_bits  # noqa: F401

P = C.c_void_p
F = C.c_float
AB = (1.5769, 0.8951)  # umap-learn's published fit for spread 1, min_dist 0.1
BS = (0.5, 0.7, 0.8951, 1.3)
LONG = 128  # csrc/n2v_umap.hip's kLong: a row of more entries is chained by a wave


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_umap/n2v_umap_cpu.c", out_dir)
    L.n2v_umap_cpu_powb.restype = None
    L.n2v_umap_cpu_powb.argtypes = [P, C.c_int64, F, P]
    L.n2v_umap_cpu_epoch.restype = None
    L.n2v_umap_cpu_epoch.argtypes = [P, P, P, C.c_int64, P, P, C.c_int64, C.c_int32, F, F, F, F, C.c_int32, C.c_uint64,
                                     P]
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def powb(L, x, b) -> np.ndarray:
    x = _f32(x)
    out = np.empty_like(x)
    L.n2v_umap_cpu_powb(x.ctypes.data, x.size, b, out.ctypes.data)
    return out


def epoch(L, csr, Y, e, a, b, gamma, alpha, negative, seed):
    """-> (Y_next fp32, the number of draws that hit their own row); the arguments are left as they are"""
    rowptr = np.ascontiguousarray(csr[0], np.int64)
    col = np.ascontiguousarray(csr[1], np.int32)
    eps, Y = _f32(csr[2]), _f32(Y)
    Y_next = np.empty_like(Y)
    hits = C.c_int64(0)
    L.n2v_umap_cpu_epoch(rowptr.ctypes.data, col.ctypes.data, eps.ctypes.data, col.shape[0], Y.ctypes.data,
                         Y_next.ctypes.data, Y.shape[0], e, a, b, gamma, alpha, negative, seed, C.addressof(hits))
    return Y_next, hits.value


def fit_loop(L, csr, Y0, n_epochs, a, b, learning_rate=1.0, negative=5, gamma=1.0, seed=0) -> np.ndarray:
    """node2vec_amd.umap.fit's loop on the restatement"""
    Y = _f32(Y0).copy()
    for e in range(n_epochs):
        Y, _ = epoch(L, csr, Y, e, a, b, gamma, learning_rate * (1.0 - e / n_epochs), negative, seed)
    return Y


# ---- the draws, and the law in float64

_M = np.uint64


def mix64(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
        return z ^ (z >> _M(31))


def draws(seed, e, t, negative, n) -> np.ndarray:
    """int64 [len(t), negative]: the vertices entry t draws in epoch e"""
    with np.errstate(over="ignore"):
        he = mix64(_M(seed) ^ mix64(_M(e) + _M(0x9E3779B97F4A7C15)))
        ht = mix64(he + (np.asarray(t, np.uint64) + _M(1)) * _M(0xD1B54A32D192ED03))
        s = (np.arange(negative, dtype=np.uint64) + _M(1)) * _M(0x8CB92BA72F3D8DD7)
        r = mix64(ht[:, None] ^ s[None, :])
        return (((r >> _M(32)) * _M(n)) >> _M(32)).astype(np.int64)


def fires(eps, e) -> np.ndarray:
    """the kernel's predicate, in fp32"""
    eps = _f32(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (eps >= 1.0) & np.isfinite(eps)
        safe = np.where(ok, eps, np.float32(1.0))
        return ok & (np.floor(np.float32(e + 1) / safe) > np.floor(np.float32(e) / safe))


def epoch64(csr, Y, e, a, b, gamma, alpha, negative, seed):
    """The same law with the same draws in float64 numpy and float64 pow, on the fp32 values of the arguments ->
    (Y_next float64, counts of what the rows met: self draws, coincident neighbours, coincident negatives)"""
    rowptr, col, eps = np.asarray(csr[0]), np.asarray(csr[1]), _f32(csr[2])
    Y = np.asarray(_f32(Y), np.float64)
    n = Y.shape[0]
    a, b, gamma, alpha = (float(np.float32(v)) for v in (a, b, gamma, alpha))
    act = fires(eps, e) & (col >= 0) & (col < n)
    ks = draws(seed, e, np.arange(col.shape[0]), negative, n)
    out = Y.copy()
    met = dict(self_draws=0, coincident_neighbours=0, coincident_negatives=0, fired=int(act.sum()))
    for i in range(n):
        y = Y[i].copy()
        for t in range(max(0, rowptr[i]), min(col.shape[0], rowptr[i + 1])):
            if not act[t]:
                continue
            for _ in range(2):
                d = y - Y[col[t]]
                d2 = d[1] * d[1] + d[0] * d[0]
                c = 0.0
                if d2 > 0:
                    pw = d2 ** b
                    c = (-2.0 * a * b * pw / d2) / (a * pw + 1.0)
                else:
                    met["coincident_neighbours"] += 1
                y = y + alpha * np.clip(c * d, -4.0, 4.0)
            for s in range(negative):
                k = ks[t, s]
                if k == i:
                    met["self_draws"] += 1
                    continue
                d = y - Y[k]
                d2 = d[1] * d[1] + d[0] * d[0]
                if d2 > 0:
                    c = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                    y = y + alpha * np.clip(c * d, -4.0, 4.0)
                else:
                    met["coincident_negatives"] += 1
                    y = y + alpha * 4.0
        out[i] = y
    return out, met


# ---- cases

def powb_sweep(lo=-40, hi=40, per_octave=64, seed=1) -> np.ndarray:
    """fp32 arguments 2^lo .. 2^hi: per_octave per octave, evenly spaced in the exponent, and random ones"""
    grid = 2.0 ** (lo + np.arange((hi - lo) * per_octave + 1) / per_octave)
    rnd = 2.0 ** np.random.default_rng(seed).uniform(lo, hi, 20000)
    return _f32(np.concatenate([grid, rnd]))


def powb_edges() -> np.ndarray:
    """subnormal arguments, both ends of the normal range, the neighbours of 1 and of the mantissa's split at
    sqrt(1/2), and what is not positive"""
    f = np.float32
    tiny = np.array([1, 2, 3, 0x7fffff, 0x400000, 0x12345], np.uint32).view(np.float32)  # subnormal
    ends = np.array([0x00800000, 0x00800001, 0x7f7fffff, 0x7f7ffffe, 0x7f800000], np.uint32).view(np.float32)
    split = np.array([0x3f3504f2, 0x3f3504f3, 0x3f3504f4, 0x3f800000, 0x3f7fffff, 0x3f800001], np.uint32)
    split = split.view(np.float32)
    rest = np.array([0.0, -0.0, -1.0, np.nan, -np.inf], np.float32)
    sub = (np.random.default_rng(2).integers(1, 0x800000, 2000).astype(np.uint32)).view(np.float32)
    return np.concatenate([tiny, ends, split, rest, sub, f(2.0) ** np.arange(-149, 128).astype(f)])


def graph_case(n, seed):
    """-> ((rowptr int64, col int32, eps fp32), Y fp32 [n, 2]).  Row 0 has no entries; rows 1 .. 4 have 70, 300, LONG
    and LONG + 1 entries (as many as n allows), the rest 0 .. 23.  eps: 1, values in [1, 6), and what never fires (0.5,
    inf, NaN, -2, 1e6); some firing entries name columns outside [0, n).  The first neighbour of row 1 coincides with
    row 1 (an edge of length zero, eps 1); row 5 and its six neighbours coincide with point 0."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 24, n)
    for row, m in enumerate((0, 70, 300, LONG, LONG + 1, 6)):
        if row < n:
            lengths[row] = m
    lengths = np.minimum(lengths, n)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, m, replace=False)) for m in lengths] + [np.zeros(0, np.int64)])
    col = col.astype(np.int32)
    nnz = col.shape[0]
    kind = rng.random(nnz)
    eps = (1.0 + 5.0 * rng.random(nnz)).astype(np.float32)
    eps[kind < 0.25] = 1.0
    never = np.array([0.5, np.inf, np.nan, -2.0, 1e6], np.float32)
    dead = kind > 0.8
    eps[dead] = never[rng.integers(0, never.shape[0], int(dead.sum()))]
    out = (kind > 0.3) & (kind < 0.36)
    outside = np.array([-1, n, n + 7, -2 ** 31, 2 ** 31 - 1], np.int64)
    col[out] = outside[rng.integers(0, 5, int(out.sum()))].astype(np.int32)
    Y = (rng.standard_normal((n, 2)) * 3.0).astype(np.float32)
    if n > 1 and lengths[1] > 0:
        t = rowptr[1]
        if not 0 <= col[t] < n:
            col[t] = 0
        eps[t] = 1.0
        Y[col[t]] = Y[1]
    if n > 5:  # row 5 and all its neighbours stand on point 0: no attraction moves it, so a negative drawn from
        lo, hi = rowptr[5], rowptr[6]  # among them meets it at distance zero
        inside = (col[lo:hi] >= 0) & (col[lo:hi] < n)
        Y[col[lo:hi][inside]] = Y[0]
        Y[5] = Y[0]
        eps[lo:hi] = 1.0
    return (rowptr, col, eps), Y


def self_draw_seed(L, csr, Y, e, negative, start=0):
    """the first seed from `start` on for which some draw of the epoch hits its own row"""
    for seed in range(start, start + 10000):
        if epoch(L, csr, Y, e, 1.0, 1.0, 1.0, 1.0, negative, seed)[1] > 0:
            return seed
    raise AssertionError("no seed draws a row's own vertex")


BLOB_SEPARATION = 8.0  # fixed on the CPU by test_umap_host's restated loop: no foreign nearest neighbour


def blob_neighbours(X, k=15):
    """(idx [n, k], dist [n, k]): the cosine neighbours in float64 numpy, dist = max(0, 1 - cos)"""
    idx, d2 = cosine_neighbours64(X, k)
    return idx, d2 / 2.0


def span10(Y) -> np.ndarray:
    Y = np.asarray(Y, np.float64)
    lo = Y.min(0)
    return 10.0 * (Y - lo) / (Y.max(0) - lo)


def pca_init64(X) -> np.ndarray:
    """the unit rows on their two leading principal components, every coordinate spanning [0, 10]"""
    X = np.asarray(X, np.float64)
    Xn = X / np.sqrt((X ** 2).sum(1))[:, None]
    Xc = Xn - Xn.mean(0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    return span10(Xc @ Vt[:2].T).astype(np.float32)
