"""Link prediction over trained vectors, on the GPU (csrc/n2v_pairs.hip): the node2vec paper's headline task.

Scores of a list of vertex pairs (dot or cosine), the paper's four edge features (Table 1: average, hadamard,
l1, l2), membership of pairs in a DeviceGraph, seeded samples of edges and of non-edges, and the exact AUC
(Mann-Whitney, ties one half).  A score is summed in one fixed order that depends on the dimension alone and is
symmetric in the pair, so it does not depend on how pairs are batched (DESIGN.md "Link prediction").  Only the
output is ever allocated: no [pairs, dim] gather of either side is made.

Device tensors in and out.  There is no CPU path for the kernels: a missing GPU or library raises.  auc() is
plain torch and works on CPU tensors too.
"""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from node2vec_amd import _dense, _lib

METRICS = {"dot": _lib.PAIR_DOT, "cosine": _lib.PAIR_COSINE}
OPERATORS = {"average": _lib.PAIR_AVERAGE, "hadamard": _lib.PAIR_HADAMARD, "l1": _lib.PAIR_L1, "l2": _lib.PAIR_L2}
NON_EDGE_ROUNDS = 32  # sample_non_edges gives up after this many rounds of redrawing


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
