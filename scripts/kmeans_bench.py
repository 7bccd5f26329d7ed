"""One Lloyd iteration of n2v_kmeans_step, and of the public cluster.kmeans loop, against the torch a user would
write without it (chunked mm for the distances, argmin, index_add_ for the sums) -> profiles/kmeans.json.

X: N seeded normal rows (N=10^7 by default), dim in DIMS, k in KS; Euclidean.  Before timing, the torch labels are
compared with the kernel's on the rows whose float64 gap between the best and second-best distance exceeds the
rounding bound of tests/test_cluster_host.py (a sample of rows).  Per shape: milliseconds of both, the ratio, the
bound max(4 n dim / 6.3 TB/s, 2 n k dim / 157.3 TFLOP/s) and the share of it the step reaches.

    python scripts/kmeans_bench.py            (N= DIMS=64,128,256 KS=8,64,1024 REPS=5 OUT=profiles/kmeans.json)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, cluster  # noqa: E402

HBM, FP32 = 6.3e12, 157.3e12
CHUNK_BYTES = 1 << 30  # the torch baseline's score chunk


def torch_step(X, C, sums, counts):
    """labels and new centroids as plain torch: scores in chunks of at most 1 GiB"""
    n, k = X.shape[0], C.shape[0]
    rows = max(1, CHUNK_BYTES // (4 * k))
    labels = torch.empty(n, dtype=torch.int64, device=X.device)
    cn = (C * C).sum(1)
    for lo in range(0, n, rows):
        t = torch.addmm(cn[None, :], X[lo:lo + rows], C.t(), alpha=-2.0)
        labels[lo:lo + rows] = t.argmin(1)
    sums.zero_().index_add_(0, labels, X)
    counts.zero_().index_add_(0, labels, torch.ones(n, dtype=torch.float32, device=X.device))
    return labels, sums / counts.clamp(min=1)[:, None]


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


def check_labels(X, C, mine, theirs, sample=20000):
    """both label sets against the float64 argmin on the sampled rows outside the rounding bound"""
    dim = X.shape[1]
    u = 2.0 ** -24
    dp = (dim + 15) // 16 * 16
    g = (dp + 2) * u / (1 - (dp + 2) * u)
    idx = torch.randperm(X.shape[0], device=X.device, generator=torch.Generator(X.device).manual_seed(1))[:sample]
    x, c = X[idx].double(), C.double()
    cn = (c * c).sum(1)
    t = cn[None, :] - 2.0 * x @ c.t()
    bound = (g * (2.0 * x.abs() @ c.abs().t() + cn[None, :])).amax(1)
    if C.shape[0] > 1:
        two = torch.topk(t, 2, dim=1, largest=False).values
        decided = (two[:, 1] - two[:, 0]) > 2.0 * bound
    else:
        decided = torch.ones_like(bound, dtype=torch.bool)
    want = t.argmin(1)
    return {"sampled": int(idx.numel()), "decided": int(decided.sum()),
            "kernel_wrong": int((mine[idx].long() != want)[decided].sum()),
            "torch_wrong": int((theirs[idx] != want)[decided].sum())}


def main():
    n = int(float(os.environ.get("N", "1e7")))
    dims = [int(v) for v in os.environ.get("DIMS", "64,128,256").split(",")]
    ks = [int(v) for v in os.environ.get("KS", "8,64,1024").split(",")]
    reps = int(os.environ.get("REPS", "5"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "kmeans.json"))
    dev = _lib.require_gpu()
    L = _lib.load()
    rows = []
    for dim in dims:
        X = torch.randn((n, dim), device=dev, generator=torch.Generator(dev).manual_seed(dim))
        for k in ks:
            C = X[torch.randperm(n, device=dev, generator=torch.Generator(dev).manual_seed(k))[:k]].contiguous()
            labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
            dist = torch.empty(n, dtype=torch.float32, device=dev)
            nxt, counts = torch.empty_like(C), torch.zeros(k, dtype=torch.int64, device=dev)
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            ws = cluster.alloc_workspace(n, dim, k, dev)

            def step():
                _lib.check(L.n2v_kmeans_step(X.data_ptr(), None, n, dim, C.data_ptr(), k, _lib.KMEANS_EUCLIDEAN,
                                             labels.data_ptr(), dist.data_ptr(), nxt.data_ptr(), counts.data_ptr(),
                                             stats.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                           "n2v_kmeans_step")

            sums, cnt = torch.empty_like(C), torch.empty(k, dtype=torch.float32, device=dev)
            step()
            theirs, their_c = torch_step(X, C, sums, cnt)
            agree = check_labels(X, C, labels, theirs)
            agree["centroid_max_abs_diff"] = float((their_c - nxt).abs().max())
            ms_step = timed(step, reps)
            ms_torch = timed(lambda: torch_step(X, C, sums, cnt), reps)
            ms_loop = timed(lambda: cluster.kmeans(X, k, init=C, max_iter=1), max(2, reps // 2))
            bound_ms = max(4.0 * n * dim / HBM, 2.0 * n * k * dim / FP32) * 1e3
            row = {"n": n, "dim": dim, "k": k, "step_ms": ms_step, "torch_ms": ms_torch,
                   "kmeans_max_iter_1_ms": ms_loop, "torch_over_step": ms_torch[0] / ms_step[0],
                   "bound_ms": bound_ms, "bound": "HBM" if 4.0 * n * dim / HBM > 2.0 * n * k * dim / FP32 else "fp32",
                   "share_of_bound": bound_ms / ms_step[0], "workspace_bytes": int(ws.numel()), "labels": agree}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ws, labels, dist, theirs
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, each ended by a device "
                              "synchronise; kmeans_max_iter_1_ms = cluster.kmeans(init=C, max_iter=1): one step and "
                              "the closing assignment", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
