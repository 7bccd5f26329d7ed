"""Link prediction over trained vectors, on the GPU (csrc/n2v_pairs.hip, csrc/n2v_edge_logreg.hip): the node2vec
paper's headline task.

Scores of a list of vertex pairs (dot or cosine), the paper's four edge features (Table 1: average, hadamard,
l1, l2), membership of pairs in a DeviceGraph, seeded samples of edges and of non-edges, and the exact AUC
(Mann-Whitney, ties one half).  A score is summed in one fixed order that depends on the dimension alone and is
symmetric in the pair, so it does not depend on how pairs are batched (DESIGN.md "Link prediction").  Only the
output is ever allocated: no [pairs, dim] gather of either side is made.

The paper's own protocol (section 4.4) trains a binary classifier on the edge feature op(x_a, x_b): fit_edges() does
that with the L-BFGS of node2vec_amd.classify over a fused kernel that gathers the two rows of a pair, forms the
feature in registers and accumulates the loss and gradient in one fixed order -- no feature row ever reaches memory
(DESIGN.md "Link-prediction classifier").  edge_scores() scores pairs with the fitted weights, link_classifier_auc()
runs the whole protocol.

Ranks against EVERY candidate (csrc/n2v_linkrank.hip, DESIGN.md "Link ranking"): holdout_edges() takes a seeded share
of the edges out of a graph before training, target_ranks() counts for every held-out pair (u, v) the rows that score
above, and equal to, v against u once u's known neighbours are left out -- fused, so that no [queries, n] score
matrix exists -- ranking_metrics() turns the counts into filtered MRR, mean rank and Hits@K, and link_ranking() runs
the three on a KeyedVectors.

Device tensors in and out.  There is no CPU path for the kernels: a missing GPU or library raises.  auc(),
ranking_metrics() and holdout_edges() are plain torch and work on CPU tensors too.
"""
from typing import Callable, Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from node2vec_amd import _dense, _lib

METRICS = {"dot": _lib.PAIR_DOT, "cosine": _lib.PAIR_COSINE}
OPERATORS = {"average": _lib.PAIR_AVERAGE, "hadamard": _lib.PAIR_HADAMARD, "l1": _lib.PAIR_L1, "l2": _lib.PAIR_L2}
NON_EDGE_ROUNDS = 32  # sample_non_edges gives up after this many rounds of redrawing
TIE_RULES = ("mean", "optimistic", "pessimistic")


def _pairs(a, b, n: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a, b) as int64 [n_pairs] on `device`; an index outside [0, n) is an IndexError before any launch"""
    a = torch.as_tensor(a, device=device).to(torch.int64).reshape(-1).contiguous()
    b = torch.as_tensor(b, device=device).to(torch.int64).reshape(-1).contiguous()
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a and b must have the same length, not {a.shape[0]} and {b.shape[0]}")
    if a.numel():
        (lo_a, hi_a), (lo_b, hi_b) = torch.aminmax(a), torch.aminmax(b)
        lo, hi = torch.stack((torch.minimum(lo_a, lo_b), torch.maximum(hi_a, hi_b))).tolist()  # one synchronisation
        if lo < 0 or hi >= n:
            raise IndexError(f"pair index outside [0, {n})")
    return a, b


def pair_scores(X: torch.Tensor, a, b, metric: str = "cosine", inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """score of every pair (a[i], b[i]) of rows of X, fp32 [n_pairs]: "dot", or "cosine" = dot * (inv_norm[a] *
    inv_norm[b]) with inv_norm = similarity.inv_norms(X) (computed when not given).  A zero row scores 0 by
    cosine; a row holding NaN or inf scores NaN."""
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: " + " | ".join(METRICS))
    X = _dense.matrix(X)
    n = X.shape[0]
    a, b = _pairs(a, b, n, X.device)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=X.device)
    norms = _dense.norms(X, inv_norm) if metric == "cosine" else None
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().n2v_pair_scores(X.data_ptr(), None if norms is None else norms.data_ptr(), n,
                                               X.shape[1], a.data_ptr(), b.data_ptr(), a.shape[0], METRICS[metric],
                                               out.data_ptr(), _lib.current_stream_ptr()), "n2v_pair_scores")
    return out


def pair_features(X: torch.Tensor, a, b, op: str = "hadamard", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the edge feature of every pair, fp32 [n_pairs, dim]: "average" (x_a + x_b) / 2, "hadamard" x_a * x_b,
    "l1" |x_a - x_b|, "l2" (x_a - x_b)^2, element by element, bit for bit numpy float32.  out: a contiguous
    fp32 [n_pairs, dim] tensor on X's device to fill (and return)."""
    if op not in OPERATORS:
        raise ValueError(f"operator {op!r}: " + " | ".join(OPERATORS))
    X = _dense.matrix(X)
    n, dim = X.shape
    a, b = _pairs(a, b, n, X.device)
    if a.shape[0] * dim >= 1 << 31:
        raise MemoryError(f"pair_features: {a.shape[0]} x {dim} values in one output; call it on chunks of the "
                          f"pair list (at most {((1 << 31) - 1) // dim} pairs each) and consume each chunk")
    if out is None:
        out = torch.empty((a.shape[0], dim), dtype=torch.float32, device=X.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != X.device
          or tuple(out.shape) != (a.shape[0], dim) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 [{a.shape[0]}, {dim}] tensor on {X.device}")
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().n2v_pair_features(X.data_ptr(), n, dim, a.data_ptr(), b.data_ptr(), a.shape[0],
                                                 OPERATORS[op], out.data_ptr(), _lib.current_stream_ptr()),
                   "n2v_pair_features")
    return out


def _graph_arrays(graph):
    if not graph.rowptr.is_cuda:
        raise ValueError("the graph must be on a HIP device")
    return graph.rowptr, graph.col, graph.n_vertices


def has_edge(graph, a, b) -> torch.Tensor:
    """bool [n_pairs]: row a[i] of the graph holds b[i] (a binary search in the row; direction as stored)"""
    rowptr, col, nv = _graph_arrays(graph)
    a, b = _pairs(a, b, nv, rowptr.device)
    mask = torch.empty(a.shape[0], dtype=torch.uint8, device=rowptr.device)
    with torch.cuda.device(rowptr.device):
        _lib.check(_lib.load().n2v_pairs_in_graph(rowptr.data_ptr(), col.data_ptr() if col.numel() else None, nv,
                                                  a.data_ptr(), b.data_ptr(), a.shape[0], mask.data_ptr(),
                                                  _lib.current_stream_ptr()), "n2v_pairs_in_graph")
    return mask.bool()


def sample_edges(graph, n: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """n edges (src, dst int64), each a uniform draw (with replacement) over the stored edge slots; the same
    seed on the same device gives the same pairs"""
    rowptr, col, _ = _graph_arrays(graph)
    if col.numel() == 0:
        raise ValueError("the graph has no edges")
    gen = torch.Generator(device=rowptr.device).manual_seed(int(seed))
    slot = torch.randint(0, col.numel(), (int(n),), generator=gen, device=rowptr.device)
    src = torch.searchsorted(rowptr, slot, right=True) - 1  # the row whose range holds the slot
    return src, col[slot].to(torch.int64)


def sample_non_edges(graph, n: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """n pairs (a, b int64) of vertices of degree > 0 with a != b that are an edge in neither direction: uniform
    draws, the rejected share redrawn in rounds.  RuntimeError when NON_EDGE_ROUNDS rounds do not reach n (a
    graph that is complete or nearly so).  The same seed on the same device gives the same pairs."""
    rowptr, _, _ = _graph_arrays(graph)
    n = int(n)
    live = torch.nonzero(graph.degrees() > 0).reshape(-1)
    gen = torch.Generator(device=rowptr.device).manual_seed(int(seed))
    got_a, got_b, have = [], [], 0
    for _ in range(NON_EDGE_ROUNDS):
        if have >= n or live.numel() < 2:
            break
        need = n - have
        draw = torch.randint(0, live.numel(), (2, need + need // 4 + 16), generator=gen, device=rowptr.device)
        a, b = live[draw[0]], live[draw[1]]
        keep = (a != b) & ~has_edge(graph, a, b) & ~has_edge(graph, b, a)
        a, b = a[keep][:need], b[keep][:need]
        got_a.append(a)
        got_b.append(b)
        have += int(a.shape[0])
    if have < n:
        raise RuntimeError(f"graph too dense to sample non-edges: {have} of {n} found in {NON_EDGE_ROUNDS} rounds")
    if not got_a:
        empty = torch.empty(0, dtype=torch.int64, device=rowptr.device)
        return empty, empty.clone()
    return torch.cat(got_a), torch.cat(got_b)


def auc(pos, neg) -> float:
    """The exact area under the ROC curve of scores `pos` against `neg` (the Mann-Whitney statistic, a tie
    counting one half): (sum over p of #{neg < p} + #{neg == p} / 2) / (P N).  One sort and two binary
    searches, O((P + N) log N); counts in int64, the division in float64.  NaN or empty input: ValueError."""
    pos = torch.as_tensor(pos).reshape(-1)
    neg = torch.as_tensor(neg).reshape(-1)
    if pos.numel() == 0 or neg.numel() == 0:
        raise ValueError("auc of an empty set of scores")
    neg = neg.to(device=pos.device)
    pos, neg = pos.to(torch.float64), neg.to(torch.float64)  # exact for every float type: the order is kept
    if bool(torch.isnan(pos).any()) or bool(torch.isnan(neg).any()):
        raise ValueError("auc of NaN scores")
    neg = torch.sort(neg).values
    below = torch.searchsorted(neg, pos, right=False)  # neg < p
    upto = torch.searchsorted(neg, pos, right=True)    # neg <= p
    twice = int((below.to(torch.int64) + upto.to(torch.int64)).sum())  # 2 below + ties
    return twice / (2 * pos.numel() * neg.numel())  # integers: one correctly rounded division


def _rows_of(wv, ids: torch.Tensor) -> torch.Tensor:
    """row of every vertex id in wv's vocabulary (-1: not in it), on ids' device"""
    if wv.ids is not None:
        keys, order = torch.sort(torch.from_numpy(np.ascontiguousarray(wv.ids)).to(ids.device))
        k = torch.searchsorted(keys, ids).clamp(max=max(keys.numel() - 1, 0))
        return torch.where(keys[k] == ids, order[k], torch.full_like(ids, -1))
    uniq, inverse = torch.unique(ids, return_inverse=True)
    rows = [wv.vocab.get(str(int(v)), -1) for v in uniq.tolist()]
    return torch.tensor(rows, dtype=torch.int64, device=ids.device)[inverse]


def link_auc(graph, wv, n_pairs: int, seed: int, metric: str = "cosine", center: bool = True) -> Dict[str, float]:
    """The link AUC of the vectors `wv` (a KeyedVectors whose tokens are vertex ids) on `graph`: n_pairs edges
    (sample_edges, seed) against n_pairs non-edges (sample_non_edges, seed + 1), scored by `metric`.  center:
    the column mean is subtracted from the vectors first (SGNS gives small graphs a common direction).  Pairs
    with a vertex outside the vocabulary are dropped and counted.
    -> {"auc", "pairs_pos", "pairs_neg", "dropped"}"""
    X = wv._device_vectors()
    inv_norm = None
    if center:
        X = X - X.mean(dim=0, keepdim=True)
    elif metric == "cosine":
        wv.init_sims()
        inv_norm = wv._inv_norm
    scores, dropped = [], 0
    for a, b in (sample_edges(graph, n_pairs, seed), sample_non_edges(graph, n_pairs, seed + 1)):
        ra, rb = _rows_of(wv, a.to(X.device)), _rows_of(wv, b.to(X.device))
        keep = (ra >= 0) & (rb >= 0)
        dropped += int((~keep).sum())
        scores.append(pair_scores(X, ra[keep], rb[keep], metric, inv_norm=inv_norm))
    return {"auc": auc(scores[0], scores[1]), "pairs_pos": int(scores[0].numel()),
            "pairs_neg": int(scores[1].numel()), "dropped": dropped}


class EdgeClassifier(NamedTuple):
    w: torch.Tensor      # fp32 [dim]
    b: torch.Tensor      # fp32 [1]
    op: str              # the edge feature the weights belong to
    loss: float          # the objective at (w, b): sum of the logistic losses + |w|^2 / (2 C)
    grad_max: float      # max |gradient of the objective| at (w, b)
    n_iter: int
    n_evals: int         # passes over the pairs
    converged: bool
    reason: str          # "gradient" | "max_iter" | "line_search"


def _operator(op: str) -> int:
    if op not in OPERATORS:
        raise ValueError(f"operator {op!r}: " + " | ".join(OPERATORS))
    return OPERATORS[op]


def _weights(w, b0, dim: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    w = torch.as_tensor(w)
    if w.ndim != 1 or w.shape[0] != dim:
        raise ValueError(f"w must be a [{dim}] tensor")
    b0 = torch.as_tensor(b0)
    if b0.numel() != 1:
        raise ValueError("b0 must be one value")
    return (w.to(device=device, dtype=torch.float32).contiguous(),
            b0.to(device=device, dtype=torch.float32).reshape(1).contiguous())


def _labels(y, n_pairs: int, device) -> torch.Tensor:
    """uint8 [n_pairs] on `device`: 1 where y is nonzero"""
    y = torch.as_tensor(y, device=device).reshape(-1)
    if y.shape[0] != n_pairs:
        raise ValueError(f"y must hold one label per pair ({n_pairs}), not {y.shape[0]}")
    return (y != 0).to(torch.uint8).contiguous()


def edge_slab_pairs(n_pairs: int, dim: int) -> int:
    """pairs per slab of the gradient's fixed order of summation (n2v_edge_logreg_slab_pairs)"""
    return int(_lib.load().n2v_edge_logreg_slab_pairs(n_pairs, dim))


def alloc_edge_workspace(n_pairs: int, dim: int, device) -> torch.Tensor:
    return _dense.workspace(_lib.load().n2v_edge_logreg_workspace_bytes, n_pairs, dim, device=device)


def edge_scores(X: torch.Tensor, a, b, w, b0, op: str = "hadamard") -> torch.Tensor:
    """z of every pair, fp32 [n_pairs]: dot(w, op(x_a, x_b)) + b0, the feature formed in registers
    (n2v_edge_logreg_scores).  The dot is pair_scores' fixed order with (w, feature) in the place of the two rows."""
    code = _operator(op)
    X = _dense.matrix(X)
    n, dim = X.shape
    a, b = _pairs(a, b, n, X.device)
    w, b0 = _weights(w, b0, dim, X.device)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().n2v_edge_logreg_scores(X.data_ptr(), n, dim, a.data_ptr(), b.data_ptr(), a.shape[0],
                                                      code, w.data_ptr(), b0.data_ptr(), out.data_ptr(),
                                                      _lib.current_stream_ptr()), "n2v_edge_logreg_scores")
    return out


def _edge_loss_grad_flat(X, a, b, y, w, b0, code: int, workspace=None) -> torch.Tensor:
    """float64 [1 + dim + 1] on the device: loss, gw, gb.  X, a, b, y as the checked device tensors."""
    n, dim = X.shape
    w, b0 = _weights(w, b0, dim, X.device)
    out = torch.zeros(dim + 2, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        ws = workspace if workspace is not None else alloc_edge_workspace(a.shape[0], dim, X.device)
        _lib.check(_lib.load().n2v_edge_logreg_loss_grad(X.data_ptr(), n, dim, a.data_ptr(), b.data_ptr(),
                                                         y.data_ptr(), a.shape[0], code, w.data_ptr(), b0.data_ptr(),
                                                         out.data_ptr(), out[1:].data_ptr(), out[1 + dim:].data_ptr(),
                                                         ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                   "n2v_edge_logreg_loss_grad")
    return out


def edge_loss_grad(X: torch.Tensor, a, b, y, w, b0, op: str = "hadamard",
                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss float64 [1], gw float64 [dim], gb float64 [1]), device tensors: the summed logistic loss of every pair's
    score against its label y (nonzero: an edge) and its gradient by (w, b0) -- unregularised sums, one pass over the
    pairs, no feature matrix (n2v_edge_logreg_loss_grad)"""
    code = _operator(op)
    X = _dense.matrix(X)
    a, b = _pairs(a, b, X.shape[0], X.device)
    out = _edge_loss_grad_flat(X, a, b, _labels(y, a.shape[0], X.device), w, b0, code, workspace)
    dim = X.shape[1]
    return out[:1], out[1:1 + dim], out[1 + dim:]


def fit_edges(X: torch.Tensor, a, b, y, op: str = "hadamard", C: float = 1.0, max_iter: int = 100, tol: float = 1e-4,
              history: int = 10, loss_grad_fn: Optional[Callable] = None) -> EdgeClassifier:
    """The paper's link-prediction classifier: L2 logistic regression on the edge feature op(x_a, x_b) of the pairs
    (a[i], b[i]) with labels y (nonzero: an edge), from w = 0, b = 0.  Minimises sum of the logistic losses +
    |w|^2 / (2 C) (the bias is not penalised) with classify.lbfgs, as classify.fit does for one class: the same
    stopping rule (max |grad| / n_pairs <= tol), the same reasons.  One evaluation is one pass over the pairs and one
    synchronisation; no [n_pairs, dim] matrix is made.  An index outside [0, n) is an IndexError before any launch, a
    non-finite value in X a ValueError.  loss_grad_fn(w [1, dim], b [1]) -> (loss, gw, gb) replaces the kernel (host
    tensors in and out), for tests."""
    from node2vec_amd import classify

    code = _operator(op)
    n, dim = _dense.shape(X)
    if not float(C) > 0.0 or int(max_iter) < 1 or not float(tol) >= 0.0 or int(history) < 1:
        raise ValueError("C must be > 0, max_iter and history >= 1, tol >= 0")
    if loss_grad_fn is None:
        X = _dense.matrix(X)
    a, b = _pairs(a, b, n, X.device)
    n_pairs = int(a.shape[0])
    if n_pairs < 1:
        raise ValueError("fit_edges needs at least one pair")
    y = _labels(y, n_pairs, X.device)
    if not bool(torch.isfinite(torch.stack(torch.aminmax(X))).all()):  # NaN propagates; no [n, dim] temporary
        raise ValueError("X holds a non-finite value")
    if loss_grad_fn is None:
        ws = alloc_edge_workspace(n_pairs, dim, X.device)

        def loss_grad_fn(w, b0):  # host parameters in, host sums out: the copy back is the one synchronisation
            flat = _edge_loss_grad_flat(X, a, b, y, w.reshape(dim), b0, code, ws).cpu()
            return flat[:1], flat[1:1 + dim], flat[1 + dim:]
    theta, f, gmax, n_iter, n_evals, reason = classify.lbfgs(
        classify.regularised(loss_grad_fn, 1, dim, 1.0 / float(C)), (1, dim + 1), n_pairs, max_iter, tol, history)
    dev = X.device
    return EdgeClassifier(theta[0, :dim].contiguous().to(dev), theta[0, dim:].contiguous().to(dev), op, f, gmax,
                          n_iter, n_evals, reason == "gradient", reason)


def link_classifier_auc(graph, wv, n_pairs: int, seed: int, op: str = "hadamard", train_fraction: float = 0.5,
                        center: bool = True, **fit_kw) -> Dict[str, object]:
    """The paper's link-prediction protocol on the vectors `wv` (a KeyedVectors whose tokens are vertex ids): n_pairs
    edges (sample_edges, seed) against n_pairs non-edges (sample_non_edges, seed + 1), as link_auc draws them; pairs
    with a vertex outside the vocabulary are dropped and counted; the rest are split by classify.split_rows(.,
    train_fraction, seed); fit_edges (whose other arguments pass through) on the training pairs; the exact auc of
    edge_scores on the held-out pairs (NaN when they lack a class).  center: the column mean is subtracted from the
    vectors first, as in link_auc.  The edges are sampled from `graph` as it is -- the graph the vectors were trained
    on, unless the caller removed the test edges before training, which is the caller's job as it is for link_auc.
    -> {"auc", "train_pairs", "test_pairs", "dropped", "result"}"""
    from node2vec_amd import classify

    _operator(op)
    if not 0.0 < float(train_fraction) <= 1.0:
        raise ValueError("train_fraction must be in (0, 1]")
    X = wv._device_vectors()
    if center:
        X = X - X.mean(dim=0, keepdim=True)
    rows_a, rows_b, labels, dropped = [], [], [], 0
    for label, (a, b) in ((1, sample_edges(graph, n_pairs, seed)), (0, sample_non_edges(graph, n_pairs, seed + 1))):
        ra, rb = _rows_of(wv, a.to(X.device)), _rows_of(wv, b.to(X.device))
        keep = (ra >= 0) & (rb >= 0)
        dropped += int((~keep).sum())
        rows_a.append(ra[keep])
        rows_b.append(rb[keep])
        labels.append(torch.full((int(keep.sum()),), label, dtype=torch.uint8, device=X.device))
    ra, rb, y = torch.cat(rows_a), torch.cat(rows_b), torch.cat(labels)
    train, test = classify.split_rows(int(y.shape[0]), train_fraction, seed)
    tr, te = torch.from_numpy(train).to(X.device), torch.from_numpy(test).to(X.device)
    result = fit_edges(X, ra[tr], rb[tr], y[tr], op=op, **fit_kw)
    z = edge_scores(X, ra[te], rb[te], result.w, result.b, op)
    pos, neg = z[y[te] != 0], z[y[te] == 0]
    value = auc(pos, neg) if pos.numel() and neg.numel() else float("nan")
    return {"auc": value, "train_pairs": int(len(train)), "test_pairs": int(len(test)), "dropped": dropped,
            "result": result}


def link_rank_plan(n: int, dim: int, n_queries: int) -> Tuple[int, int]:
    """(chunk_rows, n_chunks) of target_ranks' scan for one launch of these sizes (n2v_link_rank_plan)"""
    import ctypes

    rows, chunks = ctypes.c_int64(), ctypes.c_int32()
    _lib.check(_lib.load().n2v_link_rank_plan(n, dim, n_queries, ctypes.byref(rows), ctypes.byref(chunks)),
               "n2v_link_rank_plan")
    return int(rows.value), int(chunks.value)


def target_ranks(X: torch.Tensor, a, b, graph=None, metric: str = "cosine",
                 inv_norm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Where row b[i] stands among ALL rows of X as a partner of row a[i]: (greater, equal int64 [n_pairs], thr fp32
    [n_pairs]).  With s(u, w) the score similarity.scores gives query row u against row w, bit for bit ("dot": the
    same with every inverse norm 1), thr = s(a[i], b[i]) and, over the rows w other than a[i], b[i] and the columns
    of row a[i] of `graph` (a CSR over the rows of X -- the known edges, multi-edges once; None: no filter),
    greater = #{s(a[i], w) > thr} and equal = #{s(a[i], w) == thr}.  A NaN counts on neither side: a NaN thr gives
    (0, 0).  One scan of X per batch of queries, the counts kept in registers: nothing of size n_pairs x n is stored
    (n2v_link_rank).  The queries go in equal batches whose workspace stays under similarity.WORKSPACE_LIMIT; the
    result does not depend on the batches.  An index outside [0, n) is an IndexError before any launch."""
    from node2vec_amd import similarity

    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: " + " | ".join(METRICS))
    X = _dense.matrix(X)
    n, dim = X.shape
    a, b = _pairs(a, b, n, X.device)
    nq = int(a.shape[0])
    rowptr = col = None
    if graph is not None:
        rowptr, col, nv = _graph_arrays(graph)
        if nv != n or rowptr.device != X.device:
            raise ValueError(f"the filter graph must have one vertex per row of X ({n}) on {X.device}, "
                             f"not {nv} on {rowptr.device}")
        if col.numel() == 0:
            rowptr = col = None
    counts = torch.zeros((nq, 2), dtype=torch.int64, device=X.device)
    thr = torch.full((nq,), float("nan"), dtype=torch.float32, device=X.device)
    if nq == 0:
        return counts[:, 0].contiguous(), counts[:, 1].contiguous(), thr
    if metric == "cosine":
        norms = _dense.norms(X, inv_norm)
    else:
        norms = torch.ones(n, dtype=torch.float32, device=X.device)
    L = _lib.load()
    step = nq
    while step > 1 and L.n2v_link_rank_workspace_bytes(n, dim, step) > similarity.WORKSPACE_LIMIT:
        step = (step + 1) // 2
    with torch.cuda.device(X.device):
        for i in range(0, nq, step):
            j = min(nq, i + step)
            ws = _dense.workspace(L.n2v_link_rank_workspace_bytes, n, dim, j - i, device=X.device)
            _lib.check(L.n2v_link_rank(X.data_ptr(), norms.data_ptr(), n, dim, a[i:j].data_ptr(), b[i:j].data_ptr(),
                                       j - i, _dense.ptr(rowptr), _dense.ptr(col), thr[i:j].data_ptr(),
                                       counts[i:j].data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                       "n2v_link_rank")
    return counts[:, 0].contiguous(), counts[:, 1].contiguous(), thr


def ranking_metrics(greater, equal, ks: Sequence[int] = (1, 10, 50, 100), tie: str = "mean") -> Dict[str, float]:
    """{"mrr", "mean_rank", "hits@k" for every k of ks, "n"} of target_ranks' counts.  The rank of a query is
    1 + greater + equal / 2 ("mean": the expected place among its ties), 1 + greater ("optimistic") or
    1 + greater + equal ("pessimistic"); mrr is the mean of 1 / rank, hits@k the share of ranks <= k.  Float64 on the
    host, from the integers.  No query: ValueError."""
    if tie not in TIE_RULES:
        raise ValueError(f"tie {tie!r}: " + " | ".join(TIE_RULES))
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError("every k must be >= 1")
    g = torch.as_tensor(greater).reshape(-1).cpu().to(torch.float64)
    e = torch.as_tensor(equal).reshape(-1).cpu().to(torch.float64)
    if g.shape[0] != e.shape[0]:
        raise ValueError(f"greater and equal must have the same length, not {g.shape[0]} and {e.shape[0]}")
    if g.numel() == 0:
        raise ValueError("ranking metrics of no query")
    if bool((g < 0).any()) or bool((e < 0).any()):
        raise ValueError("counts must be >= 0")
    rank = 1.0 + g + {"mean": 0.5, "optimistic": 0.0, "pessimistic": 1.0}[tie] * e
    out = {"mrr": float((1.0 / rank).mean()), "mean_rank": float(rank.mean())}
    for k in ks:
        out[f"hits@{k}"] = float((rank <= k).to(torch.float64).mean())
    out["n"] = int(g.numel())
    return out


def _member(sorted_keys: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """bool: keys[i] is among sorted_keys (ascending)"""
    if sorted_keys.numel() == 0:
        return torch.zeros_like(keys, dtype=torch.bool)
    k = torch.searchsorted(sorted_keys, keys).clamp(max=sorted_keys.numel() - 1)
    return sorted_keys[k] == keys


def holdout_edges(graph, fraction: float, seed: int, undirected: bool = True):
    """(train_graph, test_a, test_b): `graph` without a seeded sample of its edges, and the edges taken (int64).

    undirected: an edge is the unordered pair {a, b}; both arcs (every copy of them) leave together and the pair is
    reported once, with a < b.  Otherwise an edge is the arc a -> b (every copy of it).  Self-loops are never taken.
    The distinct edges are put in one seeded order (a permutation drawn on the host, so the split is a function of
    (graph, fraction, seed) alone); an edge may leave unless it is, in that order, the last edge with an arc out of
    one of its endpoints, and the first round(fraction * edges) that may leave do.  So every vertex that had an
    out-edge keeps one -- its degree stays >= 1, which every walk needs -- but the graph may still fall apart:
    connectivity is not kept.  Where few edges may leave (a star: none) fewer are returned than asked for.  Weights
    stay with the arcs that remain.  Plain torch, on the graph's device (host tensors work too)."""
    from node2vec_amd.graph import DeviceGraph

    fraction = float(fraction)
    if not 0.0 <= fraction < 1.0:
        raise ValueError("fraction must be in [0, 1)")
    rowptr, col, nv = graph.rowptr, graph.col, graph.n_vertices
    dev = rowptr.device
    src = torch.repeat_interleave(torch.arange(nv, dtype=torch.int64, device=dev), graph.degrees())
    dst = col.to(torch.int64)
    scale = max(nv, 1)
    if undirected:
        key = torch.minimum(src, dst) * scale + torch.maximum(src, dst)
    else:
        key = src * scale + dst
    edges = torch.unique(key[src != dst])  # ascending: the order the permutation is laid over
    ea, eb = edges // scale, edges % scale
    n_edges = int(edges.numel())
    perm = torch.randperm(n_edges, generator=torch.Generator().manual_seed(int(seed))).to(dev)
    place = torch.empty(n_edges, dtype=torch.int64, device=dev)
    place[perm] = torch.arange(n_edges, dtype=torch.int64, device=dev)
    if undirected:
        arcs = torch.unique(src * scale + dst)
        out_a, out_b = _member(arcs, ea * scale + eb), _member(arcs, eb * scale + ea)
    else:
        out_a, out_b = torch.ones_like(ea, dtype=torch.bool), torch.zeros_like(ea, dtype=torch.bool)
    last = torch.full((max(nv, 1),), -1, dtype=torch.int64, device=dev)  # place of each vertex's last out-edge
    last.scatter_reduce_(0, ea[out_a], place[out_a], "amax")
    last.scatter_reduce_(0, eb[out_b], place[out_b], "amax")
    may_leave = ~((out_a & (last[ea] == place)) | (out_b & (last[eb] == place))) if n_edges else out_a
    in_order = perm[may_leave[perm]]
    taken = in_order[:int(round(fraction * n_edges))]
    keep = ~_member(torch.sort(edges[taken]).values, key)
    train_rowptr = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(src[keep], minlength=nv), 0, out=train_rowptr[1:])
    train = DeviceGraph(train_rowptr, col[keep], None if graph.unit_weights else graph.w[keep])
    return train, ea[taken], eb[taken]


def rows_graph(graph, wv):
    """`graph` (over vertex ids) as a unit-weight CSR over the rows of wv's vocabulary, on the graph's device: the
    filter target_ranks wants.  Arcs with a vertex outside the vocabulary are left out."""
    from node2vec_amd.graph import DeviceGraph

    rowptr, col, nv = _graph_arrays(graph)
    rows = _rows_of(wv, torch.arange(nv, dtype=torch.int64, device=rowptr.device))
    src = torch.repeat_interleave(rows, graph.degrees())
    dst = rows[col.to(torch.int64)]
    keep = (src >= 0) & (dst >= 0)
    return DeviceGraph.from_edges(src[keep], dst[keep], None, n_vertices=len(wv), device=rowptr.device)


def link_ranking(train_graph, wv, test_a, test_b, ks: Sequence[int] = (1, 10, 50, 100), metric: str = "cosine",
                 both: bool = True, tie: str = "mean") -> Dict[str, float]:
    """Filtered ranking of held-out edges (test_a[i], test_b[i]) (vertex ids, as holdout_edges returns them) under
    the vectors `wv` (a KeyedVectors whose tokens are vertex ids): test_b[i] is ranked among every vocabulary vertex
    as a partner of test_a[i], the neighbours test_a[i] has in `train_graph` left out (target_ranks) -- and, with
    `both`, test_a[i] among the partners of test_b[i] as well, the two pooled.  Pairs with a vertex outside the
    vocabulary are dropped and counted.  -> ranking_metrics' dict (n: the ranked queries) and "dropped"."""
    X = wv._device_vectors()
    inv_norm = None
    if metric == "cosine":
        wv.init_sims()
        inv_norm = wv._inv_norm
    ra = _rows_of(wv, torch.as_tensor(test_a).to(device=X.device, dtype=torch.int64).reshape(-1))
    rb = _rows_of(wv, torch.as_tensor(test_b).to(device=X.device, dtype=torch.int64).reshape(-1))
    if ra.shape[0] != rb.shape[0]:
        raise ValueError(f"test_a and test_b must have the same length, not {ra.shape[0]} and {rb.shape[0]}")
    known = (ra >= 0) & (rb >= 0)
    dropped = int((~known).sum())
    ra, rb = ra[known], rb[known]
    if both:
        ra, rb = torch.cat((ra, rb)), torch.cat((rb, ra))
    filt = None if train_graph is None else rows_graph(train_graph.to(X.device), wv)
    greater, equal, _ = target_ranks(X, ra, rb, graph=filt, metric=metric, inv_norm=inv_norm)
    out = ranking_metrics(greater, equal, ks, tie)
    out["dropped"] = dropped
    return out
