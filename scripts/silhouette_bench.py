"""cluster.silhouette_samples (n2v_silhouette) against the torch a user would write without it: chunked torch.cdist
(Euclidean) or 1 - Xn Xn^T (cosine) times a one-hot label matrix, in score chunks of at most 1 GiB
-> profiles/silhouette.json.

X: n seeded rows around k planted centres (noise as large as the centres' spread, so the clusters overlap), the
planted labels; m scored rows (m < n: a seeded sample, scored against all rows by both sides).  Before timing, both
results are compared with a float64 silhouette of CHECK sampled rows.  Per shape: milliseconds of both, the ratio,
the bound max(4 n dim / 6.3 TB/s, 2 m n dim / 157.3 TFLOP/s) and the share of it the call reaches.  The call is
timed whole (list build, padding, norms and the scan kernel); kernel-only times are not measured here.

    python scripts/silhouette_bench.py     (SHAPES=n:m:dim:k,... METRICS=euclidean,cosine REPS=5 CHECK=64 OUT=...)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, cluster, similarity  # noqa: E402

HBM, FP32 = 6.3e12, 157.3e12
CHUNK_BYTES = 1 << 30  # the torch baseline's score chunk
SHAPES = "100000:100000:64:8,100000:100000:128:8,100000:100000:128:64,100000:100000:128:1024,1000000:10000:128:64"


def torch_silhouette(X, labels, k, metric, rows):
    """s of `rows` (every row: None) as plain torch: distance chunks of at most 1 GiB times a one-hot matrix"""
    n = X.shape[0]
    onehot = torch.zeros((n, k), dtype=torch.float32, device=X.device)
    onehot[torch.arange(n, device=X.device), labels.long()] = 1.0
    counts = onehot.sum(0)
    Xn = X * (1.0 / X.norm(dim=1).clamp(min=1e-30))[:, None] if metric == "cosine" else X
    idx = torch.arange(n, device=X.device) if rows is None else rows
    out = torch.empty(idx.shape[0], dtype=torch.float32, device=X.device)
    step = max(1, CHUNK_BYTES // (4 * n))
    for lo in range(0, idx.shape[0], step):
        sel = idx[lo:lo + step]
        D = 1.0 - Xn[sel] @ Xn.t() if metric == "cosine" else torch.cdist(Xn[sel], Xn)
        D[torch.arange(sel.shape[0], device=X.device), sel] = 0.0  # j == i
        S = D @ onehot
        own = labels[sel].long()
        own_cnt = counts[own]
        a = S.gather(1, own[:, None])[:, 0] / (own_cnt - 1).clamp(min=1)
        mean = S / counts.clamp(min=1)[None, :]
        mean[:, counts == 0] = float("inf")
        mean.scatter_(1, own[:, None], float("inf"))
        b = mean.amin(1)
        s = (b - a) / torch.maximum(a, b)
        out[lo:lo + step] = torch.where(own_cnt > 1, s, torch.zeros_like(s))
    return out


def float64_silhouette(X, labels, k, metric, rows):
    X64 = X.double()
    if metric == "cosine":
        X64 = X64 / X64.norm(dim=1)[:, None]
        D = 1.0 - X64[rows] @ X64.t()
    else:
        D = torch.cdist(X64[rows], X64)
    D[torch.arange(rows.shape[0], device=X.device), rows] = 0.0
    onehot = torch.zeros((X.shape[0], k), dtype=torch.float64, device=X.device)
    onehot[torch.arange(X.shape[0], device=X.device), labels.long()] = 1.0
    counts = onehot.sum(0)
    S = D @ onehot
    own = labels[rows].long()
    a = S.gather(1, own[:, None])[:, 0] / (counts[own] - 1).clamp(min=1)
    mean = S / counts.clamp(min=1)[None, :]
    mean[:, counts == 0] = float("inf")
    mean.scatter_(1, own[:, None], float("inf"))
    b = mean.amin(1)
    return torch.where(counts[own] > 1, (b - a) / torch.maximum(a, b), torch.zeros_like(a))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    best.sort()
    return best[len(best) // 2] * 1e3, best[0] * 1e3, best[-1] * 1e3


def main():
    shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", SHAPES).split(",")]
    metrics = os.environ.get("METRICS", "euclidean,cosine").split(",")
    reps = int(os.environ.get("REPS", "5"))
    check = int(os.environ.get("CHECK", "64"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "silhouette.json"))
    dev = _lib.require_gpu()
    rows_out = []
    for n, m, dim, k in shapes:
        gen = torch.Generator(dev).manual_seed(n + dim + k)
        centres = torch.randn((k, dim), device=dev, generator=gen)
        labels = torch.randint(0, k, (n,), device=dev, generator=gen, dtype=torch.int32)
        X = (centres[labels.long()] + torch.randn((n, dim), device=dev, generator=gen)).contiguous()
        rows = None if m == n else torch.randperm(n, device=dev, generator=gen)[:m].sort().values
        scored = torch.arange(n, device=dev) if rows is None else rows
        probe = torch.randperm(m, device=dev, generator=gen)[:check]
        for metric in metrics:
            inv = similarity.inv_norms(X) if metric == "cosine" else None

            def call():
                return cluster.silhouette_samples(X, labels, metric, k, rows, inv_norm=inv)

            mine = call().s
            theirs = torch_silhouette(X, labels, k, metric, rows)
            want = float64_silhouette(X, labels, k, metric, scored[probe])
            agree = {"sampled": int(probe.numel()),
                     "kernel_max_abs_diff": float((mine[probe] - want).abs().max()),
                     "torch_max_abs_diff": float((theirs[probe].double() - want).abs().max()),
                     "kernel_vs_torch_max_abs_diff": float((mine - theirs.double()).abs().max()),
                     "mean_s": float(mine.mean())}
            assert agree["kernel_max_abs_diff"] < 1e-4, agree
            ms_call = timed(call, reps)
            ms_torch = timed(lambda: torch_silhouette(X, labels, k, metric, rows), reps)
            t_mem, t_flop = 4.0 * n * dim / HBM, 2.0 * m * n * dim / FP32
            bound_ms = max(t_mem, t_flop) * 1e3
            row = {"n": n, "m": m, "dim": dim, "k": k, "metric": metric, "call_ms": ms_call, "torch_ms": ms_torch,
                   "torch_over_call": ms_torch[0] / ms_call[0], "bound_ms": bound_ms,
                   "bound": "HBM" if t_mem > t_flop else "fp32", "share_of_bound": bound_ms / ms_call[0],
                   "workspace_bytes": int(_lib.load().n2v_silhouette_workspace_bytes(n, dim, k, m)), "check": agree}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, each ended by a device "
                              "synchronise; call_ms = cluster.silhouette_samples whole (workspace allocation, list "
                              "build, padding, norms, scan); torch_ms = chunked cdist / matmul times a one-hot matrix; "
                              "check = largest |s - float64 s| on the sampled rows; kernel-only time: not measured",
                   "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
