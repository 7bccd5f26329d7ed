"""Timing of CBOW negative sampling (SgnsModel(sg=0), csrc/n2v_cbow.hip) against the skip-gram trainer
on the same corpus, in one process.

    python scripts/cbow_bench.py [--scale 20] [--dims 64 128 256] [--rows 262144] [--seconds 3] [--out FILE]

Corpus: that of scripts/hs_bench.py -- an RMAT graph of 2^scale vertices (5 draws per vertex,
symmetrised), one p = q = 1 walk of 80 steps per vertex, vocabulary of every visited vertex.  Each point
trains launches of --rows sentences of 81 tokens in hogwild mode (window 5, negative 5, no subsampling,
plain stores: hub_rows 0 for both trainers), warmed up by one launch, then repeated until --seconds of
work have run, device synchronised around the window.  One JSON line per dimension: positions/s and
tokens/s of CBOW, pairs/s and tokens/s of skip-gram, the algorithmic bytes per position
    CBOW: 4 dim c (context rows read) + 8 dim (1 + k) (targets read and written) + 8 dim c (context rows
          read and written),   c = mean context words per position = skip-gram pairs / positions
    SGNS: 8 dim (2 + k) per pair, c pairs per position
and their rate as a share of the measured random-row ceiling, 5.7 TB/s."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from node2vec_amd import sgns, synthetic  # noqa: E402
from node2vec_amd import randomwalk as rw  # noqa: E402

ROW_CEILING = 5.7e12  # random 512-byte row reads on one MI355X
K, WINDOW = 5, 5


def timed(fn, seconds):
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el >= seconds:
            return el / calls, calls


def point(vocab, rows, dim, seconds, sg, cbow_mean=1):
    m = sgns.SgnsModel(vocab, dim, WINDOW, K, seed=1, sample=0.0, sg=sg, cbow_mean=cbow_mean)
    m.hub_rows = 0
    launch = {"n": 0}

    def run():
        m.train_block(rows, 0.025, launch["n"] * rows.shape[0])
        launch["n"] += 1

    t, calls = timed(run, seconds)
    assert torch.isfinite(m.syn0[:1000]).all()
    return t, calls, int(m.pairs.item()) / (calls + 1), m.hogwild_waves(*rows.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cbow_bench needs a HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    g = synthetic.rmat(a.scale, 5 << a.scale, device="cuda")
    walks, _ = rw.walk(g, rw.start_vertices(g), 1, 80, 1.0, 1.0, 7)
    vocab = sgns.build_vocab(walks, 1)
    rows = vocab.index_of[walks.long()][:a.rows].contiguous()
    tokens = int((rows >= 0).sum().item())
    emit({"corpus": f"rmat{a.scale}", "vocab": len(vocab), "rows": int(rows.shape[0]), "len": int(rows.shape[1]),
          "tokens_per_launch": tokens, "window": WINDOW, "negative": K})
    for dim in a.dims:
        tc, cc, positions, wc = point(vocab, rows, dim, a.seconds, 0)
        ts, cs, pairs, ws = point(vocab, rows, dim, a.seconds, 1)
        c = pairs / positions
        cbow_bytes = 4.0 * dim * (3.0 * c + 2.0 * (1 + K))
        sgns_bytes = 8.0 * dim * (2 + K) * c
        emit({"dim": dim, "mean_context_words": round(c, 3),
              "cbow": {"ms_per_launch": round(tc * 1e3, 3), "calls": cc, "waves": wc,
                       "Mpositions_per_s": round(positions / tc / 1e6, 1), "Mtokens_per_s": round(tokens / tc / 1e6, 1),
                       "algorithmic_bytes_per_position": round(cbow_bytes, 1),
                       "algorithmic_TBps": round(positions * cbow_bytes / tc / 1e12, 3),
                       "share_of_row_ceiling": round(positions * cbow_bytes / tc / ROW_CEILING, 3)},
              "sgns": {"ms_per_launch": round(ts * 1e3, 3), "calls": cs, "waves": ws,
                       "Mpairs_per_s": round(pairs / ts / 1e6, 1), "Mpositions_per_s": round(positions / ts / 1e6, 1),
                       "Mtokens_per_s": round(tokens / ts / 1e6, 1),
                       "algorithmic_bytes_per_position": round(sgns_bytes, 1),
                       "algorithmic_TBps": round(positions * sgns_bytes / ts / 1e12, 3),
                       "share_of_row_ceiling": round(positions * sgns_bytes / ts / ROW_CEILING, 3)},
              "cbow_over_sgns_tokens_per_s": round(ts / tc, 3)})


if __name__ == "__main__":
    main()
