"""Fold-in rate on one MI355X (csrc/n2v_foldin.hip, DESIGN.md "Fold-in"):
    python scripts/time_foldin.py [--vocab 10000000] [--new 1000 100000] [--out FILE]

Workload: dim 128, negative 5, window 5, a frozen model of --vocab rows, n_new new vertices with 10 walks of 80 tokens
each (the new vertex at the start and now and then again, the rest known words drawn by count^0.75-like Zipf counts).
Per n_new, after two warm-up passes, the median over 9 repeats of device-event times of
  * the chain kernel n2v_foldin_train alone (pairs/s, and bytes/s at 4 * dim * (1 + K) bytes per pair against the
    6.3 TB/s HBM rate MI355X_MICROARCH.md calls achievable),
  * the pair listing (two passes, the prefix over rows and the stable sort),
and beside them n2v_sgns_train's pairs/s (hogwild, the model's default launch) on walks of the same shape over the
same model.  Prints one JSON line; needs a GPU (there is no fallback)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from node2vec_amd import _lib, foldin, sgns  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s (MI355X_MICROARCH.md)
DIM, K, WINDOW, WALKS_PER_VERTEX, LENGTH = 128, 5, 5, 10, 80
WARMUP, REPEATS = 2, 9


def timed(fn):
    """median milliseconds of fn() between device events, after the warm-up"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=10_000_000)
    ap.add_argument("--new", type=int, nargs="+", default=[1000, 100_000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _lib.require_gpu()
    n = args.vocab
    gen = torch.Generator(device=dev).manual_seed(1)
    counts = (1e9 / torch.arange(1, n + 1, dtype=torch.float64, device=dev)).ceil().long() + 4
    vocab = sgns.Vocab(torch.arange(n, device=dev), counts, torch.arange(n, dtype=torch.int32, device=dev))
    m = sgns.SgnsModel(vocab, DIM, WINDOW, K, seed=1, sample=0.0)
    m.syn1neg.normal_(0.0, 0.1, generator=gen)  # a trained output matrix is not zero: f matters to the cut only
    token_p = counts.double() / counts.sum()
    result = {"dim": DIM, "negative": K, "window": WINDOW, "n_vocab": n, "walks_per_vertex": WALKS_PER_VERTEX,
              "walk_length": LENGTH, "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev),
              "bytes_per_pair": 4 * DIM * (1 + K), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "runs": []}
    for n_new in args.new:
        rows = n_new * WALKS_PER_VERTEX
        known = torch.multinomial(token_p, rows * LENGTH, replacement=True, generator=gen).reshape(rows, LENGTH)
        own = n + torch.arange(n_new, device=dev).repeat_interleave(WALKS_PER_VERTEX)
        again = torch.rand((rows, LENGTH), generator=gen, device=dev) < 0.03  # the walk comes back to its start
        again[:, 0] = True
        walks = torch.where(again, own[:, None], known).to(torch.int32)
        records, off = foldin.pair_records(m, walks, n_new, 0)
        new_rows = sgns.init_syn0(n_new, DIM, 2, dev)
        pairs = int(records.shape[0])
        t_train = timed(lambda: foldin.train_pass(m, records, off, new_rows, rows, LENGTH, 0.025, 0))
        t_list = timed(lambda: foldin.pair_records(m, walks, n_new, 0))
        assert torch.isfinite(new_rows).all()
        # the trainer on walks of the same shape over the same model (its own pair count)
        base = [0]
        known32 = known.to(torch.int32)

        def train():
            base[0] += rows
            m.train_block(known32, 0.025, base[0])

        m.pairs.zero_()
        t_sgns = timed(train)
        sgns_pairs = int(m.pairs.item()) // (WARMUP + REPEATS)
        run = {"n_new": n_new, "rows": rows, "pairs": pairs, "longest_chain": int((off[1:] - off[:-1]).max()),
               "train_ms_median_min_max": t_train, "listing_ms_median_min_max": t_list,
               "foldin_pairs_per_s": pairs / (t_train[0] * 1e-3),
               "foldin_bytes_per_s": pairs * 4 * DIM * (1 + K) / (t_train[0] * 1e-3),
               "share_of_achievable_hbm": pairs * 4 * DIM * (1 + K) / (t_train[0] * 1e-3) / HBM_ACHIEVABLE,
               "sgns_train_ms_median_min_max": t_sgns, "sgns_train_pairs": sgns_pairs,
               "sgns_train_pairs_per_s": sgns_pairs / (t_sgns[0] * 1e-3), "sgns_hub_rows": m.hub_rows}
        result["runs"].append(run)
        del walks, known, known32, records, off
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
