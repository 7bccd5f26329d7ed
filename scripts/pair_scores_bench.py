"""Timing of the pair scores (node2vec_amd.linkpred.pair_scores, csrc/n2v_pairs.hip) against the expression the
quality scripts use today, (X[a] * X[b]).sum(1), chunked so that its two [pairs, dim] gathers fit, and against
the random-row rate of this device (n2v_mem_probe mode 2 at row_bytes = 4 dim over the same matrix).

    python scripts/pair_scores_bench.py [--rows 10000000] [--dim 64 128 256] [--pairs 400000 40000000]
                                        [--seconds 0.5] [--windows 5] [--out profiles/pair_scores.json]

Inputs: a seeded normal matrix and seeded uniform pairs on the device.  Before a point is timed the two
results are compared on its first 100 000 pairs: |kernel - torch| <= 2 gamma_dim sum |a_i b_i| (each side
within gamma_dim of the exact sum, whatever its order).  Every shape is warmed up; then `windows` windows per
form, alternating the forms, each window repeating the call until about `seconds` of device work have run
between two events; the median window is reported with the fastest and slowest.  Per point:
  pair_scores_ms  the public call, metric "dot" (with its index check, one host synchronisation)
  kernel_ms       n2v_pair_scores alone; gbps = pairs * (8 dim + 16 + 4) bytes / kernel_ms
  torch_ms        the chunked torch expression (it moves 3x the row bytes and more: gathers written, read back)
  probe_gbps      the device's random-row rate at this row width; fraction_of_probe = gbps / probe_gbps
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from node2vec_amd import _lib, linkpred  # noqa: E402

TORCH_CHUNK_BYTES = 1 << 30  # per gathered side


def torch_scores(X, a, b):
    step = max(1, TORCH_CHUNK_BYTES // (4 * X.shape[1]))
    out = torch.empty(a.shape[0], dtype=torch.float32, device=X.device)
    for lo in range(0, a.shape[0], step):
        out[lo:lo + step] = (X[a[lo:lo + step]] * X[b[lo:lo + step]]).sum(1)
    return out


def kernel_only(X, a, b, out):
    _lib.check(_lib.load().n2v_pair_scores(X.data_ptr(), None, X.shape[0], X.shape[1], a.data_ptr(), b.data_ptr(),
                                           a.shape[0], _lib.PAIR_DOT, out.data_ptr(), _lib.current_stream_ptr()),
               "n2v_pair_scores")


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


def probe_gbps(X, seconds, windows):
    L = _lib.load()
    sink = torch.zeros(4, dtype=torch.int32, device=X.device)
    n = C.c_int64(0)
    row_bytes = 4 * X.shape[1]

    def run():
        _lib.check(L.n2v_mem_probe(X.data_ptr(), X.numel() * 4, 2, 256, row_bytes, C.byref(n), sink.data_ptr(),
                                   _lib.current_stream_ptr()), "n2v_mem_probe")

    ms = measure({"probe": run}, seconds, windows)["probe"][0]
    return n.value * row_bytes / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--pairs", type=int, nargs="+", default=[4 * 10 ** 5, 4 * 10 ** 7])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "pair_scores.json"))
    args = ap.parse_args()
    dev = _lib.require_gpu()
    gen = torch.Generator(device=dev).manual_seed(1)
    points = []
    for dim in args.dim:
        X = torch.empty((args.rows, dim), device=dev).normal_(generator=gen)
        ceiling = probe_gbps(X, args.seconds, args.windows)
        for n_pairs in args.pairs:
            a = torch.randint(0, args.rows, (n_pairs,), generator=gen, device=dev)
            b = torch.randint(0, args.rows, (n_pairs,), generator=gen, device=dev)
            out = torch.empty(n_pairs, dtype=torch.float32, device=dev)
            k = min(n_pairs, 100000)
            got, want = linkpred.pair_scores(X, a[:k], b[:k], "dot"), torch_scores(X, a[:k], b[:k])
            u = 2.0 ** -24
            bound = 2 * dim * u / (1 - dim * u) * (X[a[:k]].double() * X[b[:k]].double()).abs().sum(1)
            worst = float(((got.double() - want.double()).abs() / bound).max())
            if not worst <= 1.0:
                raise SystemExit(f"dim {dim}: kernel and torch differ by {worst:.3f} of the bound")
            t = measure({"pair_scores": lambda: linkpred.pair_scores(X, a, b, "dot"),
                         "kernel": lambda: kernel_only(X, a, b, out),
                         "torch": lambda: torch_scores(X, a, b)}, args.seconds, args.windows)
            gbps = n_pairs * (8 * dim + 20) / (t["kernel"][0] * 1e-3) / 1e9
            point = {"rows": args.rows, "dim": dim, "pairs": n_pairs,
                     "pair_scores_ms": round(t["pair_scores"][0], 4), "pair_scores_ms_range": [round(x, 4) for x in t["pair_scores"][1:]],
                     "kernel_ms": round(t["kernel"][0], 4), "kernel_ms_range": [round(x, 4) for x in t["kernel"][1:]],
                     "torch_ms": round(t["torch"][0], 4), "torch_ms_range": [round(x, 4) for x in t["torch"][1:]],
                     "speedup_vs_torch": round(t["torch"][0] / t["pair_scores"][0], 2),
                     "bytes_per_pair": 8 * dim + 20, "gbps": round(gbps, 1), "probe_gbps": round(ceiling, 1),
                     "fraction_of_probe": round(gbps / ceiling, 3), "worst_difference_over_bound": round(worst, 4)}
            print(json.dumps(point), flush=True)
            points.append(point)
            del a, b, out
        del X
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(dev), "seconds_per_window": args.seconds, "windows": args.windows,
              "torch_chunk_bytes": TORCH_CHUNK_BYTES, "points": points}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
