"""Product-quantised codes (node2vec_amd.ann build_pq / search_pq, csrc/n2v_ivfpq.hip) beside the IVF-flat index
(ann.search) and the exact scan (similarity.knn) on the same data and queries, in one run -> profiles/ivfpq.json.

Data and protocol of scripts/time_ivf.py: N seeded rows around CENTRES Gaussian directions, dim DIM, NLIST lists, NQ
row queries, k = K; milliseconds by HIP events around the whole call, one warm-up, the median, minimum and maximum of
REPS runs; recall@K against similarity.knn's rows.  Per m in MS: the seconds of pq_train and pq_encode (one run, host
clock around a device synchronise) and the bytes of the index (codes, codebooks, row ids, offsets, centroids); per
nprobe in NPROBES and refine in REFINES one ann.search_pq batch, beside ann.search at the same nprobe.  No threshold
is asserted here.

    python scripts/time_ivfpq.py   (N=4e6 DIM=128 NLIST=1024 NQ=4096 K=10 MS=8,16,32 NPROBES=8,32 REFINES=0,4,12
                                    REPS=5 MAX_ITER=25 CENTRES=4096 SPREAD=0.5 OUT=profiles/ivfpq.json)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from node2vec_amd import _lib, ann, similarity  # noqa: E402
from time_ivf import mixture, timed  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def recall(got, exact):
    hit = ((got[:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)).any(2).sum()
    return float(hit) / float((exact >= 0).sum())


def main():
    env = os.environ.get
    n, dim, nlist = int(float(env("N", "4e6"))), int(env("DIM", "128")), int(env("NLIST", "1024"))
    nq, k, reps = int(env("NQ", "4096")), int(env("K", "10")), int(env("REPS", "5"))
    ms_ = [int(v) for v in env("MS", "8,16,32").split(",")]
    nprobes = [int(v) for v in env("NPROBES", "8,32").split(",")]
    refines = [int(v) for v in env("REFINES", "0,4,12").split(",")]
    max_iter = int(env("MAX_ITER", "25"))
    out_path = env("OUT", os.path.join(ROOT, "profiles", "ivfpq.json"))
    dev = _lib.require_gpu()
    X = mixture(n, dim, int(env("CENTRES", "4096")), float(env("SPREAD", "0.5")), dev)
    inv = similarity.inv_norms(X)
    idx, build_s = wall(lambda: ann.build_index(X, nlist=nlist, seed=0, inv_norm=inv, max_iter=max_iter))
    rows = torch.randint(0, n, (nq,), device=dev, generator=torch.Generator(dev).manual_seed(2))
    exact_ms = timed(lambda: similarity.knn(X, k, rows=rows, inv_norm=inv), reps)
    exact = similarity.knn(X, k, rows=rows, inv_norm=inv)[0]
    flat_bytes = 4 * idx.row_ids.numel() + 8 * idx.list_off.numel() + 4 * idx.centroids.numel()
    head = {"n": n, "dim": dim, "nlist": idx.nlist, "nq": nq, "k": k, "coarse_build_s": build_s,
            "kmeans_max_iter": max_iter, "max_list_rows": idx.max_list_rows, "knn_ms": exact_ms,
            "matrix_bytes": 4 * n * dim, "flat_index_bytes": flat_bytes}
    print(json.dumps(head), flush=True)
    flat = []
    for nprobe in nprobes:
        ms = timed(lambda: ann.search(X, idx, k, rows=rows, nprobe=nprobe, inv_norm=inv), reps)
        got = ann.search(X, idx, k, rows=rows, nprobe=nprobe, inv_norm=inv)[0]
        row = {"nprobe": nprobe, "search_ms": ms, "recall_at_k": recall(got, exact)}
        flat.append(row)
        print(json.dumps({"ivf_flat": row}), flush=True)
    out = []
    for m in ms_:
        codebooks, train_s = wall(lambda: ann.pq_train(X, idx, m, seed=0, inv_norm=inv, max_iter=max_iter))
        codes, encode_s = wall(lambda: ann.pq_encode(X, idx, codebooks, inv_norm=inv))
        pq = ann.IVFPQIndex(idx, codebooks, codes, m, codebooks.shape[2])
        built = {"m": m, "train_s": train_s, "encode_s": encode_s, "code_stride": codes.shape[1],
                 "index_bytes": flat_bytes + codes.numel() + 4 * codebooks.numel(),
                 "plan": ann.plan_pq(n, dim, m, idx.nlist, idx.max_list_rows, nq, nprobes[0], k)}
        print(json.dumps(built), flush=True)
        for nprobe in nprobes:
            for refine in refines:
                def run():
                    return ann.search_pq(pq, k, rows=rows, X=X, nprobe=nprobe, refine=refine, inv_norm=inv)
                ms = timed(run, reps)
                row = {"m": m, "nprobe": nprobe, "refine": refine, "search_ms": ms,
                       "recall_at_k": recall(run()[0], exact)}
                flat_ms = next(f["search_ms"][0] for f in flat if f["nprobe"] == nprobe)
                row["flat_over_pq"] = flat_ms / ms[0]
                out.append({**built, **row})
                print(json.dumps(row), flush=True)
        del pq, codes
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, by HIP events around the whole "
                              "call (probe, tables, scan, merge, re-rank and the status read)", **head,
                   "ivf_flat": flat, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
