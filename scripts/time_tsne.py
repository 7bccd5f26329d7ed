"""Milliseconds per iteration of the two t-SNE kernels, n2v_tsne_repulse and n2v_tsne_step, on seeded points, beside
a torch baseline made in the same process: the same two sums in row chunks with torch.cdist (repulsion) and gathers
over the CSR entries (step).  One n per run, so that each size can have a time limit of its own:

    python scripts/time_tsne.py 10000 && python scripts/time_tsne.py 100000      (REPS=5 K=90 OUT=profiles/tsne.jsonl)

Prints one JSON line and appends it to OUT.  The VALU ceiling is the rate at which the CUs issue the counted
instructions of a pair (DESIGN.md "t-SNE"), at the clock named there.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from node2vec_amd import _lib, tsne  # noqa: E402

VALU_PER_PAIR = 18          # counted in the compiled loop (DESIGN.md "t-SNE")
LANE_OPS_PER_S = 256 * 64 * 2.4e9  # 256 CUs, 4 SIMDs of 16 lanes, 2.4 GHz


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    took = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
    took.sort()
    return [took[len(took) // 2] * 1e3, took[0] * 1e3, took[-1] * 1e3]


def torch_repulse(Y, chunk):
    """the same three sums in float32 torch, row chunks of `chunk`"""
    n = Y.shape[0]
    rep = torch.empty((n, 2), dtype=torch.float64, device=Y.device)
    zrow = torch.empty(n, dtype=torch.float64, device=Y.device)
    for i in range(0, n, chunk):
        yi = Y[i:i + chunk]
        w = 1.0 / (1.0 + torch.cdist(yi, Y) ** 2)
        w[torch.arange(yi.shape[0], device=Y.device), torch.arange(i, i + yi.shape[0], device=Y.device)] = 0.0
        zrow[i:i + chunk] = w.sum(1, dtype=torch.float64)
        w2 = w * w
        rep[i:i + chunk] = (yi * w2.sum(1, keepdim=True) - w2 @ Y).double()
    return rep, zrow, zrow.sum()


def torch_step(aff, rows, Y, rep, Z, vel, gain, ex, lr, mom, min_gain):
    cols = aff.col.long()
    diff = Y[rows] - Y[cols]
    a = aff.val / (1.0 + (diff * diff).sum(1))
    att = torch.zeros_like(Y).index_add_(0, rows, a[:, None] * diff)
    g = 4.0 * (ex * att - (rep / Z).float())
    gain = torch.where((g > 0) != (vel > 0), gain + 0.2, gain * 0.8).clamp_(min=min_gain)
    vel = mom * vel - lr * (gain * g)
    return Y + vel, vel, gain, g


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps, k = int(os.environ.get("REPS", "5")), int(os.environ.get("K", "90"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "tsne.jsonl"))
    dev = _lib.require_gpu()
    gen = torch.Generator(dev).manual_seed(n)
    Y = torch.randn((n, 2), device=dev, generator=gen) * 10.0
    # a symmetric P of about 2 k entries a row: k random neighbours a row, symmetrised as affinities() does
    idx = torch.randint(0, n - 1, (n, k), device=dev, generator=gen)
    idx = idx + (idx >= torch.arange(n, device=dev)[:, None]).long()
    idx, _ = torch.sort(idx, dim=1)  # a repeated neighbour becomes an absent entry
    idx = torch.where(torch.cat([torch.ones((n, 1), dtype=torch.bool, device=dev),
                                 idx[:, 1:] != idx[:, :-1]], 1), idx, torch.full_like(idx, -1))
    p = torch.rand((n, k), device=dev, generator=gen, dtype=torch.float64)
    rowptr, col, val = tsne.symmetrise(idx, p / p.sum(1, keepdim=True), n)
    aff = tsne.Affinities(rowptr, col, val, float(k) / 3.0, k)
    loop = tsne._Loop(aff, Y)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])

    def gpu_step():
        loop.step(12.0, 200.0, 0.5, 0.01)
        loop.at = 0  # the same layout every time

    chunk = max(1, min(n, (1 << 28) // (4 * n)))  # 256 MiB of fp32 per [chunk, n] temporary
    ms_rep = timed(loop.repulse, reps)
    ms_step = timed(gpu_step, reps)
    t_rep, t_zrow, t_Z = torch_repulse(Y, chunk)
    ms_t_rep = timed(lambda: torch_repulse(Y, chunk), max(2, reps // 2))
    vel, gain = torch.zeros_like(Y), torch.ones_like(Y)
    ms_t_step = timed(lambda: torch_step(aff, rows, Y, loop.rep, loop.Z, vel, gain, 12.0, 200.0, 0.5, 0.01), reps)
    pairs = float(n) * (n - 1)
    ceiling_ms = pairs * VALU_PER_PAIR / LANE_OPS_PER_S * 1e3
    row = {"n": n, "nnz": int(col.numel()), "plan": tsne.plan(n), "workspace_bytes": int(loop.ws.numel()),
           "repulse_ms": ms_rep, "step_ms": ms_step, "torch_repulse_ms": ms_t_rep, "torch_step_ms": ms_t_step,
           "torch_chunk_rows": chunk, "repulse_speedup": ms_t_rep[1] / ms_rep[1],
           "step_speedup": ms_t_step[1] / ms_step[1], "pairs_per_s": pairs / (ms_rep[1] * 1e-3),
           "valu_ceiling_ms": ceiling_ms, "share_of_valu_ceiling": ceiling_ms / ms_rep[1],
           "iteration_ms": ms_rep[1] + ms_step[1],
           # a sanity check of the values, not a test
           "Z_rel_diff_torch": float(((loop.Z[0] - t_Z) / t_Z).abs()),
           "rep_max_abs_diff_torch": float((loop.rep - t_rep).abs().max())}
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
