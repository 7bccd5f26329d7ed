"""linkpred.target_ranks (n2v_link_rank) against what the library could do for the same answer without it: n2v_knn_scores
into a [queries per batch, n] buffer of at most 1 GiB, then the comparisons in torch -> profiles/linkrank.json.

X: n seeded normal rows; Q seeded query pairs; unfiltered, and filtered by a seeded random graph of mean out-degree
DEGREE.  Before timing, the two results are required to be EQUAL (integers, and the thresholds' bits).  Per shape:
milliseconds of both, the ratio, and the share of the fp32 MFMA rate (2 Q n dim flop / 157.3 TFLOP/s) the call reaches,
beside similarity.knn's (n2v_knn_topk, k = 10) on the same queries -- the same score chain with a selection behind it.
The calls are timed whole (workspace allocation, norms excluded: they are passed in).

    python scripts/linkrank_bench.py     (SHAPES=n:dim:Q,... DEGREE=10 REPS=5 OUT=...)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, linkpred, similarity  # noqa: E402
from node2vec_amd.graph import DeviceGraph  # noqa: E402

FP32 = 157.3e12
SHAPES = "1048576:128:4096"


def stored_ranks(X, inv, a, b, graph):
    """(greater, equal, thr) from stored score rows: similarity's own batches of n2v_knn_scores, the rows that are
    no candidates set to NaN, two comparisons and two sums"""
    n = X.shape[0]
    step = max(1, similarity.WORKSPACE_LIMIT // (4 * n))
    greater, equal, thr = [], [], []
    for i in range(0, a.shape[0], step):
        qa, qb = a[i:i + step], b[i:i + step]
        S = similarity._scores(X, inv, None, qa)
        q = torch.arange(qa.shape[0], device=X.device)
        t = S[q, qb].clone()
        S[q, qa] = float("nan")
        S[q, qb] = float("nan")
        if graph is not None:
            deg = graph.rowptr[qa + 1] - graph.rowptr[qa]
            owner = torch.repeat_interleave(q, deg)
            first = torch.repeat_interleave(graph.rowptr[qa] - (torch.cumsum(deg, 0) - deg), deg)
            S[owner, graph.col[first + torch.arange(owner.shape[0], device=X.device)].long()] = float("nan")
        greater.append((S > t[:, None]).sum(1))
        equal.append((S == t[:, None]).sum(1))
        thr.append(t)
    return torch.cat(greater), torch.cat(equal), torch.cat(thr)


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
    degree = int(os.environ.get("DEGREE", "10"))
    reps = int(os.environ.get("REPS", "5"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "linkrank.json"))
    dev = _lib.require_gpu()
    rows_out = []
    for n, dim, nq in shapes:
        gen = torch.Generator(dev).manual_seed(n + dim + nq)
        X = torch.randn((n, dim), device=dev, generator=gen)
        inv = similarity.inv_norms(X)
        a = torch.randint(0, n, (nq,), device=dev, generator=gen)
        b = torch.randint(0, n, (nq,), device=dev, generator=gen)
        src = torch.randint(0, n, (degree * n,), device=dev, generator=gen)
        dst = torch.randint(0, n, (degree * n,), device=dev, generator=gen)
        graphs = {"none": None, f"degree {degree}": DeviceGraph.from_edges(src, dst, n_vertices=n, device=dev)}
        del src, dst
        ms_topk = timed(lambda: similarity.knn(X, 10, rows=a, inv_norm=inv), reps)
        flop = 2.0 * nq * n * dim
        for name, graph in graphs.items():
            mine = linkpred.target_ranks(X, a, b, graph=graph, inv_norm=inv)
            theirs = stored_ranks(X, inv, a, b, graph)
            assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1]), name
            assert torch.equal(mine[2].view(torch.int32), theirs[2].view(torch.int32)), name
            ms_call = timed(lambda: linkpred.target_ranks(X, a, b, graph=graph, inv_norm=inv), reps)
            ms_stored = timed(lambda: stored_ranks(X, inv, a, b, graph), reps)
            row = {"n": n, "dim": dim, "queries": nq, "filter": name, "call_ms": ms_call, "stored_ms": ms_stored,
                   "stored_over_call": ms_stored[0] / ms_call[0], "share_of_fp32_rate": flop / (ms_call[0] * 1e-3) / FP32,
                   "knn_topk_ms": ms_topk, "knn_topk_share_of_fp32_rate": flop / (ms_topk[0] * 1e-3) / FP32,
                   "scan": dict(zip(("chunk_rows", "n_chunks"), linkpred.link_rank_plan(n, dim, nq))),
                   "mean_greater": float(mine[0].double().mean()), "queries_with_ties": int((mine[1] > 0).sum()),
                   "workspace_bytes": int(_lib.load().n2v_link_rank_workspace_bytes(n, dim, nq))}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, each ended by a device "
                              "synchronise; call_ms = linkpred.target_ranks whole; stored_ms = n2v_knn_scores into "
                              "batches of at most 1 GiB of scores plus the torch comparisons; both results equal; "
                              "share_of_fp32_rate = 2 Q n dim / median time / 157.3 TFLOP/s",
                   "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
