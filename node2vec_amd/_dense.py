"""What the dense tasks over the trained vectors (similarity, linkpred, cluster, classify) share on the host: the
checks of the matrix X and the buffers handed to the library."""
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


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def workspace(bytes_fn, *sizes, device) -> torch.Tensor:
    """the workspace of a launch: bytes_fn(*sizes) bytes (one of the library's n2v_*_workspace_bytes), at least 16"""
    return torch.empty(max(int(bytes_fn(*sizes)), 16), dtype=torch.uint8, device=device)
