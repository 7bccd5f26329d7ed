"""Timing and memory of the link-prediction classifier (node2vec_amd.linkpred.fit_edges, csrc/n2v_edge_logreg.hip)
against the composition that was the only way before it: linkpred.pair_features into an [n_pairs, dim] matrix, then
node2vec_amd.classify on that matrix with a [n_pairs, 1] label matrix.

    python scripts/edge_logreg_bench.py [--rows 1000000 10000000] [--dim 64 128 256] [--pairs 100000 4000000]
                                        [--iters 10] [--seconds 0.5] [--windows 5] [--out profiles/edge_logreg.json]

Inputs: a seeded normal matrix, seeded uniform pairs and labels planted from a seeded weight vector, on the device.
The small pair count touches at most 2 * pairs rows, which stay in cache from one evaluation to the next; the large
one touches the whole matrix: eight times over at 10^6 rows (a matrix of 256 MB to 1 GB), less than once at 10^7 rows
(2.6 GB to 10 GB: gathers that miss every cache).  Before a point is timed the two ways are compared at a random
(w, b0): loss and gradient must agree to 1e-4 of their size.  Every shape is warmed up; then `windows` windows per form, alternating
the forms, each window repeating the call until about `seconds` of device work have run between two events; the
median window is reported with the fastest and slowest.  Per point:
  fused_eval_ms     n2v_edge_logreg_loss_grad alone (workspace allocated once); fused_gbps = pairs * (8 dim + 17)
                    bytes / fused_eval_ms, the algorithmic bytes (two rows, two indices, a label)
  composed_eval_ms  n2v_logreg_loss_grad with c = 1 over the materialised feature matrix (4 dim + 4 bytes per pair)
  features_ms       n2v_pair_features writing that matrix once
  fused_fit_ms      fit_edges for `iters` iterations (tol = 0), with its evaluations
  composed_fit_ms   pair_features + classify.fit for `iters` iterations (tol = 0), with its evaluations
  *_peak_mib        the peak of device memory above the inputs (X, a, b, y) during one fit
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from node2vec_amd import _lib, classify, linkpred  # noqa: E402


def window_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def measure(forms, seconds, windows):
    """{name: (median, fastest, slowest) ms per call}; the forms alternate window by window"""
    reps = {}
    for name, fn in forms.items():
        fn()  # warm-up of this shape
        once = max(window_ms(fn, 1), 1e-3)
        reps[name] = max(1, min(10000, int(seconds * 1e3 / once)))
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, fn in forms.items():
            times[name].append(window_ms(fn, reps[name]))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def peak_mib(fn):
    """the peak of allocated device memory during fn() above what is allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--pairs", type=int, nargs="+", default=[10 ** 5, 4 * 10 ** 6])
    ap.add_argument("--op", default="hadamard")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "edge_logreg.json"))
    args = ap.parse_args()
    dev = _lib.require_gpu()
    gen = torch.Generator(device=dev).manual_seed(1)
    code = linkpred.OPERATORS[args.op]
    points = []
    for rows, dim in ((r, d) for r in args.rows for d in args.dim):
        X = torch.empty((rows, dim), device=dev).normal_(generator=gen)
        w_true = torch.empty(dim, device=dev).normal_(generator=gen) * (2.0 / dim ** 0.5)
        w = (torch.empty(dim, device=dev).normal_(generator=gen) * (0.5 / dim ** 0.5)).contiguous()
        b0 = torch.full((1,), 0.25, device=dev)
        for n_pairs in args.pairs:
            a = torch.randint(0, rows, (n_pairs,), generator=gen, device=dev)
            b = torch.randint(0, rows, (n_pairs,), generator=gen, device=dev)
            noise = torch.empty(n_pairs, device=dev).uniform_(1e-6, 1 - 1e-6, generator=gen)
            noise = torch.log(noise) - torch.log1p(-noise)  # logistic
            y = ((linkpred.edge_scores(X, a, b, w_true, 0.0, args.op) + noise) > 0).to(torch.uint8)
            del noise
            ws = linkpred.alloc_edge_workspace(n_pairs, dim, dev)

            def fused_eval():
                return linkpred._edge_loss_grad_flat(X, a, b, y, w, b0, code, ws)

            F = linkpred.pair_features(X, a, b, args.op)
            Y = y.view(-1, 1)
            y_bits = classify.pack_labels(Y)
            cws = classify.alloc_workspace(n_pairs, dim, 1, dev)

            def composed_eval():
                return classify._loss_grad_flat(F, y_bits, w.view(1, dim), b0, cws)

            def features():
                return linkpred.pair_features(X, a, b, args.op, out=F)

            got, want = fused_eval().cpu(), composed_eval().cpu()
            scale = float(want[1:].abs().max())
            worst = max(float((got[1:] - want[1:]).abs().max()) / scale, abs(float(got[0] - want[0])) / float(want[0]))
            if not worst <= 1e-4:
                raise SystemExit(f"{rows} rows, dim {dim}, {n_pairs} pairs: the two ways differ by {worst:.3g} of "
                                 "their size")
            t = measure({"fused_eval": fused_eval, "composed_eval": composed_eval, "features": features},
                        args.seconds, args.windows)
            del F, y_bits, cws
            kw = dict(max_iter=args.iters, tol=0.0)
            evals = {}

            def fused_fit():
                res = linkpred.fit_edges(X, a, b, y, op=args.op, **kw)
                evals["fused"] = res.n_evals
                return res

            def composed_fit():
                res = classify.fit(linkpred.pair_features(X, a, b, args.op), Y, **kw)
                evals["composed"] = res.n_evals
                return res

            tf = measure({"fused_fit": fused_fit, "composed_fit": composed_fit}, args.seconds, args.windows)
            peaks = {"fused": peak_mib(fused_fit), "composed": peak_mib(composed_fit)}
            rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
            point = {"rows": rows, "dim": dim, "pairs": n_pairs, "op": args.op,
                     "fused_eval_ms": round(t["fused_eval"][0], 4), "fused_eval_ms_range": rnd(t["fused_eval"][1:]),
                     "composed_eval_ms": round(t["composed_eval"][0], 4),
                     "composed_eval_ms_range": rnd(t["composed_eval"][1:]),
                     "features_ms": round(t["features"][0], 4), "features_ms_range": rnd(t["features"][1:]),
                     "eval_speedup": round(t["composed_eval"][0] / t["fused_eval"][0], 3),
                     "bytes_per_pair": 8 * dim + 17,
                     "fused_gbps": round(n_pairs * (8 * dim + 17) / (t["fused_eval"][0] * 1e-3) / 1e9, 1),
                     "composed_gbps": round(n_pairs * (4 * dim + 4) / (t["composed_eval"][0] * 1e-3) / 1e9, 1),
                     "iters": args.iters, "fused_fit_ms": round(tf["fused_fit"][0], 3),
                     "fused_fit_ms_range": rnd(tf["fused_fit"][1:]), "fused_fit_evals": evals["fused"],
                     "fused_fit_ms_per_eval": round(tf["fused_fit"][0] / evals["fused"], 4),
                     "composed_fit_ms": round(tf["composed_fit"][0], 3),
                     "composed_fit_ms_range": rnd(tf["composed_fit"][1:]), "composed_fit_evals": evals["composed"],
                     "composed_fit_ms_per_eval": round(tf["composed_fit"][0] / evals["composed"], 4),
                     "fit_speedup": round(tf["composed_fit"][0] / tf["fused_fit"][0], 3),
                     "fused_peak_mib": round(peaks["fused"], 1), "composed_peak_mib": round(peaks["composed"], 1),
                     "worst_difference": float(f"{worst:.3g}")}
            print(json.dumps(point), flush=True)
            points.append(point)
            del a, b, y, Y, ws
            torch.cuda.empty_cache()
        del X
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(dev), "seconds_per_window": args.seconds, "windows": args.windows,
              "points": points}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
