"""Shared by tests/test_tsne_host.py and tests/test_tsne_gpu.py: the CPU restatement of csrc/n2v_tsne.hip
(tests/cpu_tsne/n2v_tsne_cpu.c) behind numpy, the float64 numpy definitions of P, of the gradient and of KL, a
float64 numpy optimiser with the kernel's update rule, the rounding bounds, and the case builders."""
import ctypes as C

import numpy as np

import cpu_build
from pca_cases import same_bits  # noqa: F401  (bit for bit in their own precision)
from silhouette_cases import U, gamma  # noqa: F401  (U = 2^-24, gamma(n) = n U / (1 - n U))

P = C.c_void_p
F = C.c_float
TILE = 1024  # n2v_tsne_plan's tile: a tile sum is a chain of at most this many fp32 additions
PAIR_ROUNDINGS = 6  # dx, dy, dx * dx, the fmaf, 1 + d2 and the division: (1 + U)^6 on w at most (see pair_bound)


def build(out_dir) -> C.CDLL:
    """the restatement, compiled by cpu_build (no contraction: one rounding per spelled operation)"""
    L = cpu_build.build("cpu_tsne/n2v_tsne_cpu.c", out_dir)
    L.n2v_tsne_cpu_repulse.restype = None
    L.n2v_tsne_cpu_repulse.argtypes = [P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, P, C.c_int64, P, P]
    L.n2v_tsne_cpu_z.restype = C.c_double
    L.n2v_tsne_cpu_z.argtypes = [P, C.c_int64]
    L.n2v_tsne_cpu_step.restype = None
    L.n2v_tsne_cpu_step.argtypes = [P, P, P, C.c_int64, P, P, C.c_double, C.c_int64, F, F, F, F, P, P, P, P]
    return L


def host_plan(n, tile=TILE, target=2048, rows=256):
    """a plan of the same shape as n2v_tsne_plan's, for the host tests (the GPU tests read the library's)"""
    n_tiles = -(-n // tile)
    want = max(1, min(n_tiles, target // max(1, -(-n // rows))))
    per = -(-n_tiles // want)
    return tile, per * tile, -(-n_tiles // per)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def repulse(L, Y, plan, rows=None):
    """-> (rep float64 [m, 2], zrow float64 [m]) of the rows (None: all), by the plan (tile, slab_cols, n_slabs)"""
    Y = _f32(Y)
    n = Y.shape[0]
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    m = n if rows is None else rows.shape[0]
    rep, zrow = np.empty((m, 2), np.float64), np.empty(m, np.float64)
    L.n2v_tsne_cpu_repulse(Y.ctypes.data, n, plan[0], plan[1], plan[2], None if rows is None else rows.ctypes.data, m,
                           rep.ctypes.data, zrow.ctypes.data)
    return rep, zrow


def z_of(L, zrow) -> float:
    zrow = np.ascontiguousarray(zrow, np.float64)
    return float(L.n2v_tsne_cpu_z(zrow.ctypes.data, zrow.shape[0]))


def step(L, csr, Y, rep, Z, exaggeration, learning_rate, momentum, min_gain, vel, gain):
    """-> (Y_next, grad, vel, gain): fp32 copies, the arguments are left as they are"""
    rowptr, col, val = csr
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    val, Y = _f32(val), _f32(Y)
    rep = np.ascontiguousarray(rep, np.float64)
    vel, gain = _f32(vel).copy(), _f32(gain).copy()
    n = Y.shape[0]
    Y_next, grad = np.empty_like(Y), np.empty_like(Y)
    L.n2v_tsne_cpu_step(rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, col.shape[0], Y.ctypes.data,
                        rep.ctypes.data, float(Z), n, exaggeration, learning_rate, momentum, min_gain,
                        vel.ctypes.data, gain.ctypes.data, Y_next.ctypes.data, grad.ctypes.data)
    return Y_next, grad, vel, gain


def fit_loop(L, csr, Y0, plan, n_iter, exaggeration_iter, early_exaggeration, learning_rate, momentum, min_gain):
    """node2vec_amd.tsne.fit's loop on the restatement -> (Y, vel, gain, grad)"""
    Y = _f32(Y0).copy()
    vel, gain = np.zeros_like(Y), np.ones_like(Y)
    grad = np.zeros_like(Y)
    for it in range(n_iter):
        early = it < exaggeration_iter
        rep, zrow = repulse(L, Y, plan)
        Y, grad, vel, gain = step(L, csr, Y, rep, z_of(L, zrow), early_exaggeration if early else 1.0, learning_rate,
                                  momentum[0] if early else momentum[1], min_gain, vel, gain)
    return Y, vel, gain, grad


# ---- the float64 definitions

def w64(Y):
    """(w [n, n] with a zero diagonal, diff [n, n, 2]) in float64"""
    Y = np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(2))
    np.fill_diagonal(w, 0.0)
    return w, diff


def repulse64(Y):
    """-> (rep [n, 2], zrow [n], Z)"""
    w, diff = w64(Y)
    return ((w ** 2)[:, :, None] * diff).sum(1), w.sum(1), float(w.sum())


def dense_of(csr, n) -> np.ndarray:
    rowptr, col, val = (np.asarray(a) for a in csr)
    Pd = np.zeros((n, n))
    Pd[np.repeat(np.arange(n), np.diff(rowptr)), col] = val
    return Pd


def gradient64(Pd, Y, exaggeration=1.0):
    """4 sum_j (exaggeration p_ij - q_ij) w_ij (y_i - y_j), q = w / Z, for a dense float64 P"""
    w, diff = w64(Y)
    coeff = (exaggeration * Pd - w / w.sum()) * w
    return 4.0 * (coeff[:, :, None] * diff).sum(1)


def kl64(Pd, Y) -> float:
    w, _ = w64(Y)
    q = w / w.sum()
    live = Pd > 0
    return float((Pd[live] * np.log(Pd[live] / q[live])).sum())


def entropy_perplexity(p) -> np.ndarray:
    """exp(H) of every row of conditional probabilities"""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(p > 0, p * np.log(p), 0.0).sum(1)
    return np.exp(h)


def calibrate64(d2, perplexity, tol=1e-5, halvings=100) -> np.ndarray:
    """the definition, row by row: bisection on beta as in the original t-SNE"""
    d2 = np.asarray(d2, np.float64)
    out = np.zeros_like(d2)
    target = np.log(perplexity)
    for i, row in enumerate(d2):
        d = row - row.min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(halvings):
            p = np.exp(-beta * d)
            s = p.sum()
            diff = np.log(s) + beta * (d * p).sum() / s - target
            if abs(diff) <= tol:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if np.isinf(hi) else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if np.isinf(lo) else (beta + lo) / 2.0
        p = np.exp(-beta * d)
        out[i] = p / p.sum()
    return out


def dense_affinities64(idx, p_cond, n) -> np.ndarray:
    """(C + C^T) / (2 n) dense, C[i, idx[i, j]] = p_cond[i, j]"""
    Cd = np.zeros((n, n))
    Cd[np.repeat(np.arange(n), idx.shape[1]), np.asarray(idx).reshape(-1)] = np.asarray(p_cond).reshape(-1)
    return (Cd + Cd.T) / (2.0 * n)


def cosine_neighbours64(X, k):
    """(idx [n, k], d2 [n, k]) of the unit rows in float64: the k nearest other rows, d2 = max(0, 2 (1 - cos))"""
    X = np.asarray(X, np.float64)
    Xn = X / np.sqrt((X ** 2).sum(1))[:, None]
    S = Xn @ Xn.T
    np.fill_diagonal(S, -np.inf)
    idx = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return idx, np.maximum(0.0, 2.0 * (1.0 - np.take_along_axis(S, idx, 1)))


def pca_init64(X) -> np.ndarray:
    """the unit rows on their two leading principal components, the first column scaled to a deviation of 1e-4"""
    X = np.asarray(X, np.float64)
    Xn = X / np.sqrt((X ** 2).sum(1))[:, None]
    Xc = Xn - Xn.mean(0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    Y = Xc @ Vt[:2].T
    return Y / Y[:, 0].std() * 1e-4


def optimise64(Pd, Y0, n_iter, exaggeration_iter, early_exaggeration=12.0, learning_rate=None,
               momentum=(0.5, 0.8), min_gain=0.01) -> np.ndarray:
    """the kernel's update rule in float64 numpy on a dense P"""
    n = Pd.shape[0]
    if learning_rate is None:
        learning_rate = max(n / early_exaggeration / 4.0, 50.0)
    Y = np.array(Y0, np.float64)
    vel, gain = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iter):
        early = it < exaggeration_iter
        g = gradient64(Pd, Y, early_exaggeration if early else 1.0)
        gain = np.where((g > 0) != (vel > 0), gain + 0.2, gain * 0.8)
        gain = np.maximum(gain, min_gain)
        vel = (momentum[0] if early else momentum[1]) * vel - learning_rate * (gain * g)
        Y = Y + vel
    return Y


def foreign_nearest(Y, labels) -> int:
    """points whose nearest other point carries another label"""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d, np.inf)
    labels = np.asarray(labels)
    return int((labels[d.argmin(1)] != labels).sum())


# ---- the bounds

def pair_bound():
    """The relative error of the fp32 w against the float64 w of the same fp32 points, from U = 2^-24 alone (Higham,
    Accuracy and Stability, lemma 3.1: a product of k factors (1 + e)^(+-1), |e| <= U, is 1 + t with |t| <=
    gamma_k; no underflow: the cases keep the points within a few hundred units of each other).

    dx and dy are one rounding each off the exact differences: dx' = dx (1 + e1).  dx' * dx' carries (1 + e1)^2
    (1 + e3); dy' * dy' (exact inside the fmaf) (1 + e2)^2; their sum rounds once; both terms are non-negative, so
    d2' = d2 (1 + t4).  1 + d2' is off 1 + d2 by at most gamma_4 relative (d2 / (1 + d2) <= 1) and rounds once: t5.
    The correctly rounded division: w' = w (1 + t6)."""
    return gamma(PAIR_ROUNDINGS)


def repulse_bounds(Y, tile=TILE):
    """(rep_bound [n, 2], zrow_bound [n], Z_bound) on |restatement - repulse64| for fp32 points Y.

    zrow: a term w' (t6) passes through at most `tile` fp32 additions of its tile's chain: gamma_(6 + tile) sum_j
    w_ij.  rep: w' * w' rounds once (t13), dx' carries one more (t14), the fmaf multiplies exactly and adds with one
    rounding per link of the chain: gamma_(14 + tile) sum_j w_ij^2 |y_i - y_j|, per coordinate.  The fp64 additions
    a term passes through (tiles, slabs, Z's chains of 256 rows and of the blocks: fewer than 2^12 in every case
    here) add less than 2^-41 relative: the factor 1 + 2^-40."""
    w, diff = w64(_f32(Y))
    slack = 1.0 + 2.0 ** -40
    t = min(tile, max(1, w.shape[0]))
    zb = w.sum(1) * gamma(PAIR_ROUNDINGS + t) * slack
    rb = ((w ** 2)[:, :, None] * np.abs(diff)).sum(1) * gamma(2 * PAIR_ROUNDINGS + 2 + t) * slack
    return rb, zb, float(zb.sum()) * slack


def gradient_bound(Pd, Y, exaggeration=1.0, tile=TILE):
    """[n, 2] on |grad_fp32 - gradient64| for fp32 points Y and a P whose values are fp32 numbers.

    Attraction: a = p w' (t7), a dx' (t8, exact inside the fmaf), a chain of at most m = ceil(row / 16) links and
    four butterfly additions: e_att = gamma_(8 + m + 4) A_abs, A_abs = sum_j p_ij w_ij |y_i - y_j|.
    Repulsion: r' = fl32((rep + dr) / (Z (1 + z))), |dr| <= rep_bound, |z| <= Z_bound / Z:
    e_rep = (rep_bound / Z + |r| Z_bound / Z) / (1 - Z_bound / Z) (1 + U) + U |r|.
    t' = fl(exaggeration a'): |a'| <= A_abs + e_att = a_mag / exaggeration, so t_err = exaggeration e_att + U a_mag.
    u' = fl(t' - r'): u_err = t_err + e_rep + U (a_mag (1 + U) + |r| + e_rep).  g = 4 u' is exact."""
    Y = _f32(Y)
    w, diff = w64(Y)
    rep, _, Z = repulse64(Y)
    rb, _, zb = repulse_bounds(Y, tile)
    longest = int((Pd > 0).sum(1).max()) if Pd.size else 0
    A_abs = ((Pd * w)[:, :, None] * np.abs(diff)).sum(1)
    e_att = gamma(8 + -(-longest // 16) + 4) * A_abs
    r_abs = np.abs(rep) / Z
    e_rep = (rb / Z + r_abs * zb / Z) / (1.0 - zb / Z) * (1.0 + U) + U * r_abs
    a_mag = exaggeration * (A_abs + e_att)
    t_err = exaggeration * e_att + U * a_mag
    u_err = t_err + e_rep + U * (a_mag * (1.0 + U) + r_abs + e_rep)
    return 4.0 * u_err * (1.0 + 2.0 ** -40)


# ---- cases

def lattice_points(n, seed, spacing=1.0):
    """n fp32 points in the plane at least 0.5 apart: distinct lattice points, each moved by less than 0.24"""
    rng = np.random.default_rng(seed)
    R = max(3, int(np.ceil(np.sqrt(4.0 * n) / 2.0)))
    seen, pts = set(), []
    while len(pts) < n:
        p = (int(rng.integers(-R, R + 1)), int(rng.integers(-R, R + 1)))
        if p not in seen:
            seen.add(p)
            pts.append(p)
    Y = np.array(pts, np.float64) * spacing
    move = rng.standard_normal((n, 2))
    move *= (rng.random(n) * 0.24 / np.sqrt((move ** 2).sum(1)))[:, None]
    return (Y + move).astype(np.float32)


def normal_points(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(np.float32)


def random_csr(n, lengths, seed):
    """a CSR matrix whose row i holds lengths[i % len(lengths)] distinct ascending columns (never i) and positive
    fp32 values that sum to 1 -> (rowptr int64, col int32, val fp32)"""
    rng = np.random.default_rng(seed)
    rowptr, cols = [0], []
    for i in range(n):
        m = min(int(lengths[i % len(lengths)]), n - 1)
        c = rng.choice(n - 1, m, replace=False)
        c = np.sort(np.where(c >= i, c + 1, c))
        cols.append(c)
        rowptr.append(rowptr[-1] + m)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    val = rng.random(col.shape[0]) + 0.1
    return np.array(rowptr, np.int64), col, (val / val.sum()).astype(np.float32)


def random_symmetric_p(n, seed) -> np.ndarray:
    """a dense symmetric float64 P with a zero diagonal that sums to 1"""
    A = np.random.default_rng(seed).random((n, n))
    A = A + A.T
    np.fill_diagonal(A, 0.0)
    return A / A.sum()


BLOB_SEPARATION = 6.0  # the centres are BLOB_SEPARATION e_c: fixed by test_tsne_host's reference optimiser


def blobs(per=100, dim=16, seed=5, separation=BLOB_SEPARATION):
    """three Gaussian blobs of `per` rows with unit deviation around separation * e_0, e_1, e_2 -> (X fp32, labels)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * per, dim))
    labels = np.repeat(np.arange(3), per)
    X[np.arange(3 * per), labels] += separation
    return X.astype(np.float32), labels


def blob_affinities64(X, perplexity=10.0):
    idx, d2 = cosine_neighbours64(X, int(3 * perplexity))
    return dense_affinities64(idx, calibrate64(d2, perplexity), X.shape[0])
