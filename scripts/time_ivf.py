"""The inverted-file index (node2vec_amd.ann, csrc/n2v_ivf.hip) beside the exact scan (similarity.knn) on the same
queries -> profiles/ivf.json.

Data: N seeded rows around CENTRES Gaussian directions (x = centre + SPREAD * noise), dim DIM; the index has NLIST
lists (spherical k-means, MAX_ITER Lloyd iterations at most); NQ row queries, k = K.  Reported: the index build time
(one run, host clock around a device synchronise), and per nprobe in NPROBES the time of one ann.search batch (probe,
scan, merge and the status read) beside similarity.knn's on the same queries (HIP events, one warm-up, the median,
minimum and maximum of REPS runs), recall@K against knn's rows, and the rows and bytes of candidates a query reads
(row, row id and inverse norm).  No threshold is asserted here.

    python scripts/time_ivf.py     (N=4e6 DIM=128 NLIST=1024 NQ=4096 K=10 NPROBES=1,8,32,1024 REPS=5 MAX_ITER=25
                                    CENTRES=4096 SPREAD=0.5 OUT=profiles/ivf.json)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, ann, similarity  # noqa: E402


def mixture(n, dim, centres, spread, dev, seed=1, chunk=1 << 20):
    g = torch.Generator(dev).manual_seed(seed)
    C = torch.randn((centres, dim), device=dev, generator=g)
    C /= C.norm(dim=1, keepdim=True)
    X = torch.empty((n, dim), device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        pick = torch.randint(0, centres, (m,), device=dev, generator=g)
        X[lo:lo + m] = C[pick] + (spread / dim ** 0.5) * torch.randn((m, dim), device=dev, generator=g)
    return X


def timed(fn, reps):
    """[median, min, max] milliseconds by HIP events, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return [ms[len(ms) // 2], ms[0], ms[-1]]


def main():
    env = os.environ.get
    n, dim, nlist = int(float(env("N", "4e6"))), int(env("DIM", "128")), int(env("NLIST", "1024"))
    nq, k, reps = int(env("NQ", "4096")), int(env("K", "10")), int(env("REPS", "5"))
    nprobes = [int(v) for v in env("NPROBES", "1,8,32,1024").split(",")]
    max_iter = int(env("MAX_ITER", "25"))
    out_path = env("OUT", os.path.join(ROOT, "profiles", "ivf.json"))
    dev = _lib.require_gpu()
    X = mixture(n, dim, int(env("CENTRES", "4096")), float(env("SPREAD", "0.5")), dev)
    inv = similarity.inv_norms(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = ann.build_index(X, nlist=nlist, seed=0, inv_norm=inv, max_iter=max_iter)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    lens = idx.list_off[1:] - idx.list_off[:-1]
    rows = torch.randint(0, n, (nq,), device=dev, generator=torch.Generator(dev).manual_seed(2))
    exact_ms = timed(lambda: similarity.knn(X, k, rows=rows, inv_norm=inv), reps)
    exact = similarity.knn(X, k, rows=rows, inv_norm=inv)[0]
    head = {"n": n, "dim": dim, "nlist": idx.nlist, "nq": nq, "k": k, "build_s": build_s, "kmeans_max_iter": max_iter,
            "max_list_rows": idx.max_list_rows, "mean_list_rows": float(lens.double().mean()),
            "empty_lists": int((lens == 0).sum()), "knn_ms": exact_ms}
    print(json.dumps(head), flush=True)
    out = []
    for nprobe in nprobes:
        nprobe = min(nprobe, idx.nlist)
        ms = timed(lambda: ann.search(X, idx, k, rows=rows, nprobe=nprobe, inv_norm=inv), reps)
        probe_ms = timed(lambda: ann.probe(idx, rows=rows, X=X, nprobe=nprobe), reps)
        got = ann.search(X, idx, k, rows=rows, nprobe=nprobe, inv_norm=inv)[0]
        hit = ((got[:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)).any(2).sum()
        scanned = lens[ann.probe(idx, rows=rows, X=X, nprobe=nprobe).long().clamp(min=0)].sum(1).double().mean()
        row = {"nprobe": nprobe, "search_ms": ms, "of_which_probe_ms": probe_ms, "knn_over_search": exact_ms[0] / ms[0],
               "recall_at_k": float(hit) / float((exact >= 0).sum()), "rows_per_query": float(scanned),
               "share_of_rows": float(scanned) / n, "candidate_bytes_per_query": float(scanned) * (4 * dim + 8),
               "plan": ann.plan(n, dim, idx.nlist, idx.max_list_rows, nq, nprobe, k)}
        out.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, by HIP events around the whole "
                              "call; search_ms includes the probe (of_which_probe_ms, timed alone)", **head,
                   "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
