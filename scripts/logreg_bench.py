"""One n2v_logreg_loss_grad call against the torch a user would write without it (Z = X W^T + b in chunks of at
most 1 GiB, sigmoid, (P - Y)^T X accumulated per chunk) -> profiles/logreg.json.

X: N seeded normal rows (N=10^7 by default), dim in DIMS, c in CS; W seeded normal / sqrt(dim), labels seeded at
density 0.3.  Before timing, the two gradients are compared (largest absolute difference over the largest absolute
value).  Per shape: milliseconds of both as [median, min, max] of REPS calls after one warm-up, each ended by a device
synchronise, the ratio of the medians, the bound max(4 n dim / 6.3 TB/s, 4 n c dim / 157.3 TFLOP/s) and the share of
it the call reaches.

    python scripts/logreg_bench.py            (N= DIMS=64,128,256 CS=8,64,1024 REPS=5 OUT=profiles/logreg.json)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, classify  # noqa: E402

HBM, FP32 = 6.3e12, 157.3e12
CHUNK_BYTES = 1 << 30  # the torch baseline's score chunk


def torch_loss_grad(X, Y, W, b):
    """plain torch: scores in chunks of at most 1 GiB, the gradient accumulated over the chunks in fp32"""
    n, c = X.shape[0], W.shape[0]
    rows = max(1, CHUNK_BYTES // (4 * c))
    gW, gb = torch.zeros_like(W), torch.zeros_like(b)
    for lo in range(0, n, rows):
        x = X[lo:lo + rows]
        R = torch.sigmoid(torch.addmm(b[None, :], x, W.t())) - Y[lo:lo + rows]
        gW.addmm_(R.t(), x)
        gb += R.sum(0)
    return gW, gb


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e3, t[0] * 1e3, t[-1] * 1e3


def main():
    n = int(float(os.environ.get("N", "1e7")))
    dims = [int(v) for v in os.environ.get("DIMS", "64,128,256").split(",")]
    cs = [int(v) for v in os.environ.get("CS", "8,64,1024").split(",")]
    reps = int(os.environ.get("REPS", "5"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "logreg.json"))
    dev = _lib.require_gpu()
    L = _lib.load()
    rows = []
    for dim in dims:
        X = torch.randn((n, dim), device=dev, generator=torch.Generator(dev).manual_seed(dim))
        for c in cs:
            gen = torch.Generator(dev).manual_seed(c)
            W = torch.randn((c, dim), device=dev, generator=gen) / dim ** 0.5
            b = torch.randn(c, device=dev, generator=gen)
            Yb = torch.rand((n, c), device=dev, generator=gen) < 0.3
            y_bits = classify.pack_labels(Yb)
            Y = Yb.float()  # the baseline's labels, made outside the timed region
            del Yb
            out = torch.zeros(1 + c * dim + c, dtype=torch.float64, device=dev)
            ws = classify.alloc_workspace(n, dim, c, dev)

            def call():
                _lib.check(L.n2v_logreg_loss_grad(X.data_ptr(), y_bits.data_ptr(), n, dim, W.data_ptr(), b.data_ptr(),
                                                  c, out.data_ptr(), out[1:].data_ptr(), out[1 + c * dim:].data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
                           "n2v_logreg_loss_grad")

            call()
            tW, tb = torch_loss_grad(X, Y, W, b)
            gW = out[1:1 + c * dim].view(c, dim)
            agree = {"gW_max_abs_diff_over_max_abs": float((tW.double() - gW).abs().max() / gW.abs().max()),
                     "gb_max_abs_diff_over_max_abs": float((tb.double() - out[1 + c * dim:]).abs().max()
                                                           / out[1 + c * dim:].abs().max())}
            ms_call = timed(call, reps)
            ms_torch = timed(lambda: torch_loss_grad(X, Y, W, b), reps)
            hbm_ms, flop_ms = 4.0 * n * dim / HBM * 1e3, 4.0 * n * c * dim / FP32 * 1e3
            row = {"n": n, "dim": dim, "c": c, "loss_grad_ms": ms_call, "torch_ms": ms_torch,
                   "torch_over_loss_grad": ms_torch[0] / ms_call[0], "bound_ms": max(hbm_ms, flop_ms),
                   "bound": "HBM" if hbm_ms > flop_ms else "fp32", "share_of_bound": max(hbm_ms, flop_ms) / ms_call[0],
                   "workspace_bytes": int(ws.numel()), "agreement": agree}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ws, Y, y_bits, out
            torch.cuda.empty_cache()
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"columns": "ms as [median, min, max] of REPS calls after one warm-up, each ended by a device "
                              "synchronise; the torch baseline reads float labels [n, c] prepared outside the timed "
                              "region and accumulates in fp32", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
