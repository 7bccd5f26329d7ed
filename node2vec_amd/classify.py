"""Multi-label node classification over trained vectors, on the GPU (csrc/n2v_logreg.hip): the protocol of the
node2vec paper (section 4.3) -- one-vs-rest L2 logistic regression on a fraction of the labelled vertices, Micro- and
Macro-F1 on the rest -- without copying the matrix to the host.

One evaluation of the objective is one pass over X (n2v_logreg_loss_grad scores, takes the residuals and multiplies
them back into the gradient in one launch).  Every score, loss and gradient is computed in one fixed order of fp32 /
fp64 operations (DESIGN.md "Node classification"): the same call gives the same bits.  The optimiser is a host-driven
L-BFGS in float64 over the [c, dim + 1] parameters; the iterate itself is fp32, as the kernel reads it.

Device tensors in and out.  There is no CPU path: a missing GPU or library raises.
"""
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from node2vec_amd import _dense, _lib

MAX_CLASSES = 1024
ARMIJO_C1 = 1e-4
MAX_HALVINGS = 30


class LogRegResult(NamedTuple):
    W: torch.Tensor      # fp32 [c, dim]
    b: torch.Tensor      # fp32 [c]
    loss: float          # the objective at (W, b): sum of the logistic losses + |W|^2 / (2 C)
    grad_max: float      # max |gradient of the objective| at (W, b)
    n_iter: int
    n_evals: int         # passes over X
    converged: bool
    reason: str          # "gradient" | "max_iter" | "line_search"


def _params(W, b, dim: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    if not isinstance(W, torch.Tensor) or W.ndim != 2 or W.shape[1] != dim:
        raise ValueError(f"W must be a [c, {dim}] tensor")
    c = int(W.shape[0])
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"c = {c} classes outside [1, {MAX_CLASSES}]")
    if not isinstance(b, torch.Tensor) or b.ndim != 1 or b.shape[0] != c:
        raise ValueError(f"b must be a [{c}] tensor")
    return (W.to(device=device, dtype=torch.float32).contiguous(),
            b.to(device=device, dtype=torch.float32).contiguous())


def alloc_workspace(n: int, dim: int, c: int, device) -> torch.Tensor:
    return _dense.workspace(_lib.load().n2v_logreg_workspace_bytes, n, dim, c, device=device)


def slab_rows(n: int, dim: int, c: int) -> int:
    """rows per slab of the gradient's fixed order of summation (n2v_logreg_slab_rows)"""
    return int(_lib.load().n2v_logreg_slab_rows(n, dim, c))


def pack_labels(Y: torch.Tensor) -> torch.Tensor:
    """bool or 0/1 [n, c] -> int32 [n, ceil(c / 32)] holding the uint32 words the kernel reads: bit j of word w of a
    row is its label of class 32 w + j"""
    if not isinstance(Y, torch.Tensor) or Y.ndim != 2:
        raise ValueError("Y must be a 2-D [n, c] tensor")
    n, c = int(Y.shape[0]), int(Y.shape[1])
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"c = {c} classes outside [1, {MAX_CLASSES}]")
    words = (c + 31) // 32
    weights = torch.ones(32, dtype=torch.int64, device=Y.device) << torch.arange(32, device=Y.device)
    packed = torch.empty((n, words), dtype=torch.int32, device=Y.device)
    for w in range(words):  # a word at a time: the temporaries are [n, 32], not [n, c]
        part = (Y[:, 32 * w:32 * w + 32] != 0).to(torch.int64)
        word = (part * weights[:part.shape[1]]).sum(1)  # in [0, 2^32)
        packed[:, w] = torch.where(word >= (1 << 31), word - (1 << 32), word).to(torch.int32)
    return packed


def labels_from_frame(df, ids) -> Tuple[torch.Tensor, np.ndarray]:
    """A DataFrame with one ["id", "label"] row per (vertex, label) -> (Y bool [len(ids), c] on the host, classes):
    classes are the distinct labels, sorted; row i of Y belongs to ids[i]; a vertex without a row is all-zero; an id
    that `ids` does not hold is a KeyError."""
    if "id" not in df.columns or "label" not in df.columns:
        raise ValueError('df must have the columns "id" and "label"')
    import pandas as pd

    ids = np.asarray(ids)
    rows = pd.Index(ids).get_indexer(df["id"].to_numpy())
    if (rows < 0).any():
        raise KeyError(df["id"].to_numpy()[rows < 0][0])
    classes, cols = np.unique(df["label"].to_numpy(), return_inverse=True)
    Y = torch.zeros((len(ids), max(len(classes), 1)), dtype=torch.bool)
    Y[torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64).reshape(-1))] = True
    return Y, classes


def decision_function(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp32 [n, c]: z[r][k] = dot(W_k, x_r) + b[k] (n2v_logreg_scores)"""
    n, dim = _dense.shape(X)
    X = _dense.matrix(X)
    W, b = _params(W, b, dim, X.device)
    c = W.shape[0]
    Z = torch.empty((n, c), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        ws = alloc_workspace(n, dim, c, X.device)
        _lib.check(_lib.load().n2v_logreg_scores(X.data_ptr(), n, dim, W.data_ptr(), b.data_ptr(), c, Z.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "n2v_logreg_scores")
    return Z


def _loss_grad_flat(X, y_bits, W, b, workspace=None) -> torch.Tensor:
    """float64 [1 + c dim + c] on the device: loss, gW, gb"""
    n, dim = _dense.shape(X)
    X = _dense.matrix(X)
    W, b = _params(W, b, dim, X.device)
    c = W.shape[0]
    if not isinstance(y_bits, torch.Tensor) or y_bits.dtype != torch.int32 or \
            tuple(y_bits.shape) != (n, (c + 31) // 32):
        raise ValueError(f"y_bits must be pack_labels' int32 [{n}, {(c + 31) // 32}] tensor")
    y_bits = y_bits.to(X.device).contiguous()
    out = torch.zeros(1 + c * dim + c, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        ws = workspace if workspace is not None else alloc_workspace(n, dim, c, X.device)
        _lib.check(_lib.load().n2v_logreg_loss_grad(X.data_ptr(), y_bits.data_ptr(), n, dim, W.data_ptr(),
                                                    b.data_ptr(), c, out.data_ptr(), out[1:].data_ptr(),
                                                    out[1 + c * dim:].data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _lib.current_stream_ptr()), "n2v_logreg_loss_grad")
    return out


def loss_grad(X: torch.Tensor, y_bits: torch.Tensor, W: torch.Tensor, b: torch.Tensor,
              workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss float64 [1], gW float64 [c, dim], gb float64 [c]), device tensors: the summed logistic loss of every
    (row, class) and its gradient -- unregularised sums, one pass over X (n2v_logreg_loss_grad)"""
    out = _loss_grad_flat(X, y_bits, W, b, workspace)
    c, dim = int(W.shape[0]), int(W.shape[1])
    return out[:1], out[1:1 + c * dim].view(c, dim), out[1 + c * dim:]


def two_loop(g: torch.Tensor, pairs) -> torch.Tensor:
    """L-BFGS's two-loop recursion: -H g for the (s, y) pairs, oldest first (float64, any shape); without pairs -g"""
    q = g.clone()
    alphas = []
    for s, y in reversed(pairs):
        rho = 1.0 / float((s * y).sum())
        a = rho * float((s * q).sum())
        alphas.append((a, rho))
        q -= a * y
    if pairs:
        s, y = pairs[-1]
        q *= float((s * y).sum()) / float((y * y).sum())
    for (s, y), (a, rho) in zip(pairs, reversed(alphas)):
        beta = rho * float((y * q).sum())
        q += (a - beta) * s
    return -q


def lbfgs(evaluate_at: Callable, shape: Tuple[int, int], n: int, max_iter: int, tol: float, history: int):
    """The host-driven L-BFGS of fit() and linkpred.fit_edges(): minimises from theta = 0 (fp32, `shape` = [c, dim + 1])
    the objective evaluate_at(theta) -> (f, g float64 of `shape`, max |g|).  `history` pairs, Armijo backtracking
    (c1 = 1e-4, halving, at most 30 halvings, first step 1 / max(1, |g|)), in float64; the iterate is fp32:
    theta+ = float32(theta + alpha d), s from the rounded values; a pair enters the history only if s.y > 0.  Stops
    when max |g| / n <= tol ("gradient"), after max_iter iterations ("max_iter") or when the line search fails
    ("line_search").  -> (theta, f, max |g|, n_iter, n_evals, reason)"""
    theta = torch.zeros(shape, dtype=torch.float32)
    f, g, gmax = evaluate_at(theta)
    n_evals = 1
    pairs = []
    n_iter, reason = 0, "max_iter"
    while True:
        if gmax / n <= tol:
            reason = "gradient"
            break
        if n_iter >= int(max_iter):
            break
        d = two_loop(g, pairs)
        slope = float((g * d).sum())
        if not slope < 0.0:  # not a descent direction: restart from steepest descent
            pairs, d = [], -g
            slope = float((g * d).sum())
        alpha = 1.0 if pairs else 1.0 / max(1.0, float(g.norm()))
        for _ in range(MAX_HALVINGS + 1):
            nxt = (theta.double() + alpha * d).to(torch.float32)
            f_new, g_new, gmax_new = evaluate_at(nxt)
            n_evals += 1
            if f_new <= f + ARMIJO_C1 * alpha * slope:  # false for NaN
                break
            alpha *= 0.5
        else:
            reason = "line_search"
            break
        s = nxt.double() - theta.double()
        y = g_new - g
        if float((s * y).sum()) > 0.0:
            pairs = (pairs + [(s, y)])[-int(history):]
        theta, f, g, gmax = nxt, f_new, g_new, gmax_new
        n_iter += 1
    return theta, f, gmax, n_iter, n_evals, reason


def regularised(loss_grad_fn: Callable, c: int, dim: int, lam: float) -> Callable:
    """lbfgs's evaluate_at for f = loss + lam |W|^2 / 2 over theta = [W | b] (the bias is not penalised), from
    loss_grad_fn(W, b) -> (loss, gW, gb), the unregularised sums"""
    def evaluate_at(th):
        loss, gW, gb = loss_grad_fn(th[:, :dim].contiguous(), th[:, dim].contiguous())
        w64 = th[:, :dim].double()
        g = torch.cat([gW.cpu().double().view(c, dim) + lam * w64, gb.cpu().double().view(c, 1)], 1)
        f = float(loss.cpu().double().reshape(())) + 0.5 * lam * float((w64 * w64).sum())
        return f, g, float(g.abs().max())
    return evaluate_at


def fit(X: torch.Tensor, Y: torch.Tensor, C: float = 1.0, max_iter: int = 100, tol: float = 1e-4, history: int = 10,
        loss_grad_fn: Optional[Callable] = None) -> LogRegResult:
    """One-vs-rest L2 logistic regression from W = 0, b = 0: minimises f = sum of the logistic losses +
    |W|^2 / (2 C) (the bias is not penalised; the minimiser of scikit-learn's
    OneVsRestClassifier(LogisticRegression(C=C))).  L-BFGS with `history` pairs and Armijo backtracking (c1 = 1e-4,
    halving, at most 30 halvings, first step 1 / max(1, |g|)), in float64 on the [c, dim + 1] parameters, on the
    host.  The iterate is fp32: theta+ = float32(theta + alpha d), s from the rounded values; a pair enters the
    history only if s.y > 0.  Stops when max |grad f| / n <= tol ("gradient", converged), after max_iter iterations
    ("max_iter") or when the line search fails ("line_search").  One evaluation is one pass over X and one
    synchronisation (the copy of the [c, dim + 1] sums to the host).  X holding a non-finite value is a ValueError.
    loss_grad_fn(W, b) -> (loss, gW, gb) replaces the kernel (host tensors in and out), for tests."""
    n, dim = _dense.shape(X)
    if not isinstance(Y, torch.Tensor) or Y.ndim != 2 or Y.shape[0] != n:
        raise ValueError(f"Y must be a [{n}, c] tensor")
    c = int(Y.shape[1])
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"c = {c} classes outside [1, {MAX_CLASSES}]")
    if not float(C) > 0.0 or int(max_iter) < 1 or not float(tol) >= 0.0 or int(history) < 1 or n < 1:
        raise ValueError("C must be > 0, max_iter, history and n >= 1, tol >= 0")
    if loss_grad_fn is None:
        X = _dense.matrix(X)
        y_bits = pack_labels(Y.to(X.device))
        ws = alloc_workspace(n, dim, c, X.device)

        def loss_grad_fn(W, b):  # host parameters in, host sums out: the copy back is the one synchronisation
            flat = _loss_grad_flat(X, y_bits, W.to(X.device), b.to(X.device), ws).cpu()
            return flat[:1], flat[1:1 + c * dim], flat[1 + c * dim:]
    if not bool(torch.isfinite(X).all()):
        raise ValueError("X holds a non-finite value")
    theta, f, gmax, n_iter, n_evals, reason = lbfgs(regularised(loss_grad_fn, c, dim, 1.0 / float(C)), (c, dim + 1),
                                                    n, max_iter, tol, history)
    dev = X.device
    return LogRegResult(theta[:, :dim].contiguous().to(dev), theta[:, dim].contiguous().to(dev), f, gmax, n_iter,
                        n_evals, reason == "gradient", reason)


def predict(scores: torch.Tensor, threshold: float = 0.0) -> torch.Tensor:
    """bool [n, c]: score > threshold"""
    return scores > threshold


def predict_top(scores: torch.Tensor, counts) -> torch.Tensor:
    """bool [n, c], the paper's protocol: row r gets its counts[r] highest-scoring classes (the number of labels it
    truly has); ties go to the lower class"""
    n, c = scores.shape
    counts = torch.as_tensor(counts, device=scores.device).to(torch.int64).reshape(n)
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    take = torch.arange(c, device=scores.device)[None, :] < counts[:, None]
    out = torch.zeros((n, c), dtype=torch.bool, device=scores.device)
    out.scatter_(1, order, take)
    return out


def f1_scores(Y_true: torch.Tensor, Y_pred: torch.Tensor) -> Dict[str, object]:
    """{"micro", "macro", "per_class"} in float64 from exact int64 TP / FP / FN counts; a class (or the whole) with
    TP + FP + FN = 0 scores 0"""
    t, p = Y_true != 0, Y_pred.to(Y_true.device) != 0
    if t.shape != p.shape or t.ndim != 2:
        raise ValueError("Y_true and Y_pred must be [n, c] tensors of one shape")
    tp = (t & p).sum(0, dtype=torch.int64)
    fp = (~t & p).sum(0, dtype=torch.int64)
    fn = (t & ~p).sum(0, dtype=torch.int64)
    den = 2 * tp + fp + fn
    per = torch.where(den > 0, 2.0 * tp.double() / den.clamp(min=1).double(),
                      torch.zeros_like(den, dtype=torch.float64))
    all_den = int(den.sum())
    micro = 2.0 * int(tp.sum()) / all_den if all_den else 0.0
    return {"micro": micro, "macro": float(per.mean()), "per_class": per}


def split_rows(n: int, train_fraction: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(train rows, test rows): numpy.random.default_rng(seed).permutation(n), the first round(train_fraction n)
    train"""
    if not 0.0 < float(train_fraction) <= 1.0:
        raise ValueError("train_fraction must be in (0, 1]")
    perm = np.random.default_rng(seed).permutation(n)
    n_train = int(round(float(train_fraction) * n))
    return perm[:n_train], perm[n_train:]


def evaluate(X: torch.Tensor, Y: torch.Tensor, train_fraction: float = 0.5, seed: int = 0, top: bool = True,
             **fit_kw):
    """The paper's protocol -> (LogRegResult, F1 dictionary of the held-out rows); the rows are split_rows(n,
    train_fraction, seed).  X[train] is gathered once into a contiguous copy.  top: predict_top with every test
    row's true number of labels; else     predict at 0."""
    n, _ = _dense.shape(X)
    X = _dense.matrix(X)
    Y = Y.to(X.device)
    train, test = split_rows(n, train_fraction, seed)
    tr, te = torch.from_numpy(train).to(X.device), torch.from_numpy(test).to(X.device)
    result = fit(X[tr].contiguous(), Y[tr], **fit_kw)
    if len(test) == 0:
        return result, {"micro": 0.0, "macro": 0.0, "per_class": torch.zeros(Y.shape[1], dtype=torch.float64)}
    scores = decision_function(X[te].contiguous(), result.W, result.b)
    truth = Y[te] != 0
    pred = predict_top(scores, truth.sum(1)) if top else predict(scores)
    return result, f1_scores(truth, pred)
