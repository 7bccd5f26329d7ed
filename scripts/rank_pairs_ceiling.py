"""What the p = q = 1 walk on the pair table (graph.build_rank_pairs, walk_uniform_kernel form 4) reaches of its
ceiling: the kernel's walk-steps/s over the rate of dependent random 8-byte gathers on the pair table itself
(n2v_mem_probe mode 1, width 8), in one process, on the graph of a bench configuration.  Also the one-off
build times of the pair table and of the 16-byte hop table.  Untimed setup around HIP-event timings; prints
one JSON line.

    python scripts/rank_pairs_ceiling.py [--config cfg4] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch

    import bench
    from node2vec_amd import randomwalk as rw

    args = bench.parse(["--config", a.config])
    cfg = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    setup = {}
    g = bench.build_graph(cfg, torch, dev, setup, args.trim)
    out = {"config": a.config, "n_vertices": g.n_vertices, "n_edges": g.n_edges}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    g.build_hops8()
    out["hops8_accepted"] = g.hops8 is not None
    out["hop_table_build_s"] = timed(g.build_hops)
    g.hops = None
    out["pair_table_first_build_s"] = timed(g.build_rank_pairs)  # with the rank tables (two sorts of the degrees)
    assert g.rank_pairs is not None, "the graph declines the pair table"
    out["pair_table_rebuild_s"] = timed(g.build_rank_pairs)  # the rank tables at hand: cumsum + the fill kernel
    out["pair_table_GB"] = g.rank_pairs.numel() * 8 / 1e9
    out["rank_classes"] = g.rank_class_first.numel()
    out["rank_head"] = 0 if g.rank_head is None else g.rank_head.numel()
    c = bench.measure_ceilings(torch, g.rank_pairs, gather_width=8)
    out["chain_8B_per_s"] = c["gather_chain"]
    out["independent_8B_per_s"] = c["gather_independent"]

    W, L, batch = args.num_walks, args.walk_length, cfg["batch"]
    start_all = rw.start_vertices(g)
    n_batches = max(1, start_all.numel() // batch)
    rep = {}
    walks, valid = rw.audition_buffers(g, start_all[:batch], W, L, 1.0, 1.0, 42, report=rep)
    assert g.hops is None and g.hops8 is None  # the pair table serves
    ev = []
    for k in range(a.warmup + a.steps):
        st = start_all[(k % n_batches) * batch:(k % n_batches + 1) * batch]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rw.walk(g, st, W, L, 1.0, 1.0, 42, out=(walks, valid), check=False)
        e1.record()
        ev.append((e0, e1, int(st.numel())))
    torch.cuda.synchronize()
    ms = [x.elapsed_time(y) for x, y, _ in ev[a.warmup:]]
    rate = [n * W * L / (1e-3 * t) for t, (_, _, n) in zip(ms, ev[a.warmup:])]  # launched walker-steps
    out["kernel_ms_mean"] = sum(ms) / len(ms)
    out["kernel_ms_min_max"] = [min(ms), max(ms)]
    out["launched_steps_per_s"] = sum(rate) / len(rate)
    out["of_chain_ceiling"] = out["launched_steps_per_s"] / out["chain_8B_per_s"]
    out["audition"] = rep
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
