"""time of cluster.dbscan's three scans (n2v_dbscan_count, n2v_dbscan_union, n2v_dbscan_border) at a few (n, dim) on
three Gaussian blobs plus uniform noise, beside cluster.assign against k = 1024 centroids on the same X -- the same
MFMA chain with an argmin behind it, and the only comparison there is: the rate per scored pair -> profiles/dbscan.json.

Per shape: milliseconds of every scan (device events around the library call, median / min / max of REPS runs after a
warm-up), the pairs it scores (n^2; core^2 / 2; border x core), pairs per second, the same for assign (n x 1024 pairs),
and what the clustering found.

    python scripts/time_dbscan.py     (SHAPES=n:dim,... REPS=5 OUT=...)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _dense, _lib, cluster  # noqa: E402

SHAPES = "20000:16,100000:16,100000:128,400000:16"
SIGMA = 0.25


def blobs(n, dim, dev):
    """three blobs of 0.3 n rows each, sigma 0.25, centres 8 apart; 0.1 n uniform rows in [-6, 6]"""
    gen = torch.Generator(dev).manual_seed(n + dim)
    m = (3 * n) // 10
    centres = torch.zeros((3, dim), device=dev)
    centres[0, 0], centres[1, 0], centres[2, min(1, dim - 1)] = -4.0, 4.0, 4.0
    rows = [centres[c] + SIGMA * torch.randn((m, dim), device=dev, generator=gen) for c in range(3)]
    rows.append(torch.rand((n - 3 * m, dim), device=dev, generator=gen) * 12.0 - 6.0)
    X = torch.cat(rows)
    return X[torch.randperm(n, device=dev, generator=gen)].contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(t))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", SHAPES).split(",")]
    reps = int(os.environ.get("REPS", "5"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "dbscan.json"))
    dev = _lib.require_gpu()
    L = _lib.load()
    rows_out = []
    for n, dim in shapes:
        X = blobs(n, dim, dev)
        eps = float((2.0 * dim) ** 0.5 * SIGMA)  # the typical distance inside a blob: about half its pairs
        min_samples = max(5, n // 100)
        res = cluster.dbscan(X, eps, min_samples)
        core = torch.nonzero(res.core_mask)[:, 0].to(torch.int32)
        border = torch.nonzero(~res.core_mask)[:, 0].to(torch.int32)
        ws = _dense.workspace(L.n2v_dbscan_workspace_bytes, n, dim, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        root = torch.empty(n, dtype=torch.int32, device=dev)
        labels = res.labels.clone()
        st = _lib.current_stream_ptr()
        args = (X.data_ptr(), None, n, dim, _lib.KMEANS_EUCLIDEAN, eps)
        tail = (ws.data_ptr(), ws.numel(), 0, st)
        scans = {
            "count": (lambda: _lib.check(L.n2v_dbscan_count(*args, min_samples, counts.data_ptr(), None, *tail), "count"),
                      float(n) * n),
            "union": (lambda: _lib.check(L.n2v_dbscan_union(*args, core.data_ptr(), core.numel(), root.data_ptr(),
                                                            *tail), "union"), core.numel() * (core.numel() + 1) / 2.0),
            "border": (lambda: _lib.check(L.n2v_dbscan_border(*args, core.data_ptr(), core.numel(), border.data_ptr(),
                                                              border.numel(), labels.data_ptr(), *tail), "border"),
                       float(core.numel()) * border.numel()),
        }
        row = {"n": n, "dim": dim, "eps": eps, "min_samples": min_samples, "n_clusters": res.n_clusters,
               "core_rows": int(core.numel()), "noise_rows": int((res.labels == -1).sum()),
               "workspace_bytes": int(ws.numel())}
        for name, (fn, pairs) in scans.items():
            ms = timed(fn, reps)
            row[name] = {"ms": ms, "pairs": pairs, "pairs_per_s": pairs / (ms[0] * 1e-3) if pairs else 0.0}
        assert torch.equal(counts, res.counts) and torch.equal(labels, res.labels)
        ms = timed(lambda: cluster.dbscan(X, eps, min_samples), reps)
        row["dbscan_whole_ms"] = ms
        C = X[torch.randperm(n, device=dev)[:1024]].contiguous()
        ms = timed(lambda: cluster.assign(X, C), reps)
        row["assign_k1024"] = {"ms": ms, "pairs": float(n) * 1024, "pairs_per_s": n * 1024 / (ms[0] * 1e-3)}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        del X, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, device events around the "
                              "library call (assign_k1024 and dbscan_whole_ms: around the Python call, allocations "
                              "and host synchronisations included); pairs_per_s = pairs / median; Euclidean metric; "
                              "the union scan's pairs are those on or above the diagonal of the core list",
                   "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
