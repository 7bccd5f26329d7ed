"""What the dense tasks over the trained vectors (similarity, ann, linkpred, cluster, classify, pca, tsne) share on the
host: the checks of the matrix X, of the inv_norm=, queries= and rows= arguments, the buffers handed to the library,
and the batched launch of a top-k scan with its exclude_self epilogue."""
from typing import Optional, Tuple

import torch

MAX_DIM = 1024


def shape(X) -> Tuple[int, int]:
    if not isinstance(X, torch.Tensor) or X.ndim != 2:
        raise ValueError("X must be a 2-D tensor on a HIP device")
    return int(X.shape[0]), int(X.shape[1])


def matrix(X: torch.Tensor) -> torch.Tensor:
    if not isinstance(X, torch.Tensor) or X.ndim != 2 or not X.is_cuda:
        raise ValueError("X must be a 2-D tensor on a HIP device")
    if X.dtype != torch.float32:
        raise ValueError(f"X must be float32, not {X.dtype}")
    if not 1 <= X.shape[1] <= MAX_DIM:
        raise ValueError(f"vector dimension {X.shape[1]} outside [1, {MAX_DIM}]")
    if X.shape[0] >= 1 << 31:
        raise ValueError("at most 2^31 - 1 rows")
    return X.contiguous()


def check_inv_norm(n: int, inv_norm) -> None:
    """the host half of norms(), for callers that check their arguments before any device work"""
    if inv_norm is not None and (not isinstance(inv_norm, torch.Tensor) or inv_norm.ndim != 1
                                 or inv_norm.shape[0] < n):
        raise ValueError("inv_norm must hold one value per row of X")


def norms(X: torch.Tensor, inv_norm: Optional[torch.Tensor]) -> torch.Tensor:
    """the inv_norm= argument: similarity.inv_norms(X) when not given, else its first n values, fp32 on X's device"""
    if inv_norm is None:
        from node2vec_amd import similarity

        return similarity.inv_norms(X)
    check_inv_norm(X.shape[0], inv_norm)
    return inv_norm[:X.shape[0]].to(device=X.device, dtype=torch.float32).contiguous()


def queries(q, dim: int, device) -> torch.Tensor:
    """the queries= argument: fp32 [n_queries, dim] on `device`; one vector [dim] is one query"""
    q = torch.as_tensor(q, device=device)
    if q.ndim == 1:
        q = q[None]
    if q.ndim != 2 or q.shape[1] != dim:
        raise ValueError(f"queries must be [n_queries, {dim}]")
    return q.to(torch.float32).contiguous()


def rows(r, n: int, device) -> torch.Tensor:
    """the rows= argument: int64 [n_queries] on `device`; a row outside [0, n) is an IndexError before any launch"""
    r = torch.as_tensor(r, device=device).to(torch.int64).reshape(-1).contiguous()
    if r.numel() and (int(r.min()) < 0 or int(r.max()) >= n):
        raise IndexError("query row outside [0, n)")
    return r


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def workspace(bytes_fn, *sizes, device) -> torch.Tensor:
    """the workspace of a launch: bytes_fn(*sizes) bytes (one of the library's n2v_*_workspace_bytes), at least 16"""
    return torch.empty(max(int(bytes_fn(*sizes)), 16), dtype=torch.uint8, device=device)


def topk_batches(need, launch, nq: int, k: int, device, max_step: Optional[int] = None, empty: bool = False):
    """(rows int64 [nq, k], scores fp32 [nq, k]) of a top-k scan over nq queries, (-1, -inf) where `launch` writes
    nothing.  The queries go in equal batches, the largest whose workspace need(count) bytes stays under
    similarity.WORKSPACE_LIMIT (halved until it does; one query is launched whatever it needs).
    launch(i, j, ws, out_r, out_s) scans queries [i, j) into those rows of the outputs.  max_step: a scan that takes
    at most so many queries a launch and answers sizes it refuses with need() < 0, which then halves as well.
    empty: nothing to scan."""
    from node2vec_amd import similarity

    out_r = torch.full((nq, k), -1, dtype=torch.int64, device=device)
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=device)
    if empty or nq == 0:
        return out_r, out_s
    step = nq if max_step is None else min(nq, max_step)
    refused = float("-inf") if max_step is None else 0  # need() below this: the sizes are refused
    while step > 1 and not refused <= need(step) <= similarity.WORKSPACE_LIMIT:
        step = (step + 1) // 2
    for i in range(0, nq, step):
        j = min(nq, i + step)
        launch(i, j, workspace(need, j - i, device=device), out_r, out_s)
    return out_r, out_s


def drop_self(out_r: torch.Tensor, out_s: torch.Tensor, self_rows: torch.Tensor, k: int):
    """exclude_self: out_r / out_s [nq, k + 1] without every query's own row -- or, where it is not among the
    k + 1, without the last one"""
    drop = out_r == self_rows[:, None]
    drop[:, -1] |= ~drop.any(dim=1)
    keep = ~drop
    return out_r[keep].view(-1, k), out_s[keep].view(-1, k)
