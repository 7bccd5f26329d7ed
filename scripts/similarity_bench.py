"""Timing of the nearest-neighbour queries (node2vec_amd.similarity.knn, csrc/n2v_knn.hip) against the
torch path with the same semantics (chunked torch.mm of the normalised queries with X, times the inverse row
norms, torch.topk per chunk, then a topk over the chunks' winners).

    python scripts/similarity_bench.py [--n 10000000 100000000] [--dim 128] [--nq 1 16 256 4096]
                                       [--k 10 100] [--seconds 3] [--out FILE]

Inputs: seeded torch.randn matrices on the device.  Before timing a point the two results are compared
with a tie-aware rule (every rank's score within tol = dim * 2^-22 of the other's, and rows that differ
only where their score lies within 2 tol of the k-th).  Each measurement warms up, then repeats the call
until --seconds of work have run (device synchronise around the window).  One JSON line per point:
ms per call for both, achieved TB/s and TFLOP/s of the fused kernel and its share of the binding bound
(DESIGN.md "Nearest neighbours": bytes 4 n dim ceil(nq / Qt), FLOPs 2 nq n dim; 8 TB/s, 157.3 TFLOP/s).
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from node2vec_amd import similarity  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE, FP32_PEAK = 8.0e12, 6.29e12, 157.3e12


def query_tile(nq, k):
    """queries per block of n2v_knn_topk's plan (plan_topk in csrc/n2v_knn.hip)"""
    if k <= 128 and nq > 32:
        return 64
    if k <= 384 and nq > 16:
        return 32
    return 16 if k <= 896 else 8


def torch_topk(X, inv, Q, k, chunk_elems=1 << 29):
    """the same scores and order by torch: score = (q / |q|) . x_r * inv_norm[r]; ties by row ascending"""
    qh = Q * (1.0 / Q.norm(dim=1, keepdim=True)).nan_to_num(0.0, 0.0, 0.0)
    rows = max(k, chunk_elems // max(Q.shape[0], 1))
    best_s, best_r = [], []
    for lo in range(0, X.shape[0], rows):
        s = torch.mm(qh, X[lo:lo + rows].T) * inv[lo:lo + rows]
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        best_s.append(v)
        best_r.append(i + lo)
    s, r = torch.cat(best_s, 1), torch.cat(best_r, 1)
    v, i = torch.topk(s, k, dim=1)
    return torch.gather(r, 1, i), v


def agree(a, b, dim):
    (ra, sa), (rb, sb) = a, b
    tol = dim * 2.0 ** -22
    if (sa - sb).abs().max().item() > tol:
        return False
    kth = torch.minimum(sa[:, -1:], sb[:, -1:])
    for q in range(ra.shape[0]):
        diff = set(ra[q].tolist()) ^ set(rb[q].tolist())
        if diff:
            idx = torch.tensor(sorted(diff), device=ra.device)
            # a row only one side has must be a near-tie with the k-th score
            s = torch.cat([sa[q][torch.isin(ra[q], idx)], sb[q][torch.isin(rb[q], idx)]])
            if (s - kth[q]).abs().max().item() > 2 * tol:
                return False
    return True


def timed(fn, seconds):
    fn()  # warm-up: code objects, allocator, algorithm choice
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el >= seconds:
            return el / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10 ** 7, 10 ** 8])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similarity_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    out = open(a.out, "w") if a.out else None
    for n in a.n:
        g = torch.Generator(device=dev).manual_seed(n)
        X = torch.empty(n, a.dim, device=dev)
        for lo in range(0, n, 1 << 24):
            X[lo:lo + (1 << 24)].normal_(generator=g)
        inv = similarity.inv_norms(X)
        for nq in a.nq:
            Q = torch.randn(nq, a.dim, device=dev, generator=g)
            for k in a.k:
                mine = similarity.knn(X, k, queries=Q, inv_norm=inv)
                ref = torch_topk(X, inv, Q, k)
                ok = agree(mine, ref, a.dim)
                if not ok:
                    raise SystemExit(f"fused and torch results differ at n={n} nq={nq} k={k}")
                t, calls = timed(lambda: similarity.knn(X, k, queries=Q, inv_norm=inv), a.seconds)
                tt, tcalls = timed(lambda: torch_topk(X, inv, Q, k), a.seconds)
                bytes_ = 4.0 * n * a.dim * math.ceil(nq / query_tile(nq, k))
                flops = 2.0 * nq * n * a.dim
                t_hbm, t_fp32 = bytes_ / HBM_PEAK, flops / FP32_PEAK
                rec = {"n": n, "dim": a.dim, "nq": nq, "k": k, "agree": ok,
                       "fused_ms": round(t * 1e3, 3), "fused_calls": calls,
                       "torch_ms": round(tt * 1e3, 3), "torch_calls": tcalls,
                       "speedup_vs_torch": round(tt / t, 2),
                       "achieved_TBps": round(bytes_ / t / 1e12, 3), "achieved_TFLOPs": round(flops / t / 1e12, 2),
                       "bound": "hbm" if t_hbm >= t_fp32 else "fp32",
                       "share_of_bound": round(max(t_hbm, t_fp32) / t, 3),
                       "share_of_achievable_hbm": round(bytes_ / HBM_ACHIEVABLE / t, 3)}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
        del X, inv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
