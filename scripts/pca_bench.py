"""The two passes of principal components, n2v_pca_mean and n2v_pca_scatter, and the public pca.fit, on seeded
normal rows -> profiles/pca.json.

Per shape (n, dim): milliseconds of both passes, the bytes of X per second each reaches beside the read rate that
n2v_mem_probe sustains in this process (mode 2, random 2 KiB rows read by a wave each over the same buffer: the
probe's nearest shape to a stream), the fp32 flop/s of the scatter pass (n dim_pad^2 useful flops: the upper
triangle's multiply-adds) beside the 157.3 TFLOP/s of the fp32 MFMA, and pca.fit with its host eigenproblem.

    python scripts/pca_bench.py            (SHAPES=1048576x128,10000000x128,4000000x256 REPS=5 OUT=profiles/pca.json)
"""
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, pca  # noqa: E402

FP32 = 157.3e12


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


def read_ceiling(L, X, reps):
    """bytes per second of n2v_mem_probe mode 2 (2 KiB rows) over X's own memory"""
    sink = torch.zeros(4, dtype=torch.int32, device=X.device)
    count = C.c_int64(0)
    nbytes = X.numel() * 4 // 2048 * 2048

    def probe():
        _lib.check(L.n2v_mem_probe(X.data_ptr(), nbytes, 2, 64, 2048, C.byref(count), sink.data_ptr(),
                                   _lib.current_stream_ptr()), "n2v_mem_probe")

    ms = timed(probe, reps)
    return count.value * 2048 / (ms[1] * 1e-3)


def main():
    shapes = [tuple(int(v) for v in s.split("x"))
              for s in os.environ.get("SHAPES", "1048576x128,10000000x128,4000000x256").split(",")]
    reps = int(os.environ.get("REPS", "5"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "pca.json"))
    dev = _lib.require_gpu()
    L = _lib.load()
    rows = []
    for n, dim in shapes:
        X = torch.randn((n, dim), device=dev, generator=torch.Generator(dev).manual_seed(dim)) + 0.5
        ceiling = read_ceiling(L, X, reps)
        mean = torch.zeros(dim, dtype=torch.float64, device=dev)
        S = torch.zeros((dim, dim), dtype=torch.float64, device=dev)
        used = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = pca.alloc_workspace(n, dim, dev)

        def mean_pass():
            _lib.check(L.n2v_pca_mean(X.data_ptr(), None, n, dim, mean.data_ptr(), used.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _lib.current_stream_ptr()), "n2v_pca_mean")

        mean_pass()
        centre = mean.float()

        def scatter_pass():
            _lib.check(L.n2v_pca_scatter(X.data_ptr(), None, n, dim, centre.data_ptr(), S.data_ptr(), used.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()), "n2v_pca_scatter")

        ms_mean, ms_scatter = timed(mean_pass, reps), timed(scatter_pass, reps)
        ms_fit = timed(lambda: pca.fit(X, 2), max(2, reps // 2))
        want = torch.cov(X[:200000].double().t())  # a sanity check of the values, not a test
        got = pca.moments(X[:200000])
        dp = (dim + 15) // 16 * 16
        nbytes, flops = 4.0 * n * dim, float(n) * dp * dp
        row = {"n": n, "dim": dim, "slab_rows": pca.slab_rows(n, dim), "workspace_bytes": int(ws.numel()),
               "mean_ms": ms_mean, "scatter_ms": ms_scatter, "fit_ms": ms_fit,
               "probe_read_bytes_per_s": ceiling,
               "mean_bytes_per_s": nbytes / (ms_mean[1] * 1e-3),
               "scatter_bytes_per_s": nbytes / (ms_scatter[1] * 1e-3),
               "mean_share_of_probe": nbytes / (ms_mean[1] * 1e-3) / ceiling,
               "scatter_share_of_probe": nbytes / (ms_scatter[1] * 1e-3) / ceiling,
               "scatter_flops_per_s": flops / (ms_scatter[1] * 1e-3),
               "scatter_share_of_fp32_mfma": flops / (ms_scatter[1] * 1e-3) / FP32,
               "cov_max_abs_diff_200k_rows": float((got[1] / (got[2] - 1) - want).abs().max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS runs after one warm-up, each ended by a device "
                              "synchronise; rates from the minimum", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
