"""Timing of skip-gram hierarchical softmax (node2vec_amd.hs, csrc/n2v_hs.hip) against the SGNS trainer on
the same corpus.

    python scripts/hs_bench.py [--scale 20] [--dims 64 128 256] [--rows 262144] [--seconds 3] [--out FILE]

Corpus: an RMAT graph of 2^scale vertices (5 draws per vertex, symmetrised), one p = q = 1 walk of 80
steps per vertex, vocabulary of every visited vertex (minCount 1).  Each point trains launches of
--rows sentences in hogwild mode, warmed up, then repeated until --seconds of work have run (device
synchronise around the window).  One JSON line per point: HS pairs/s, path-node updates/s (pairs x mean
code length), the frequency-weighted mean code length, algorithmic bytes/s and their share of the
measured random-row ceiling, and the SGNS trainer's pairs/s on the same rows.  Algorithmic bytes per
pair: the context row read and written (8 dim), the levels of the path the kernel caches in LDS (the top
16 / 8 / 4 / 2 / 1 at dim <= 64 / 128 / 256 / 512 / 1024 in hogwild mode, none with the cache off) read
and written once per centre position (spread over its pairs), and the levels below read and written per
pair (8 dim each).  --variants: at dim 128, the path cache off.  --quality adds the
planted-partition community AUC of deterministic and hogwild HS, and the link AUC on the corpus graph
after two hogwild epochs at dim 128 (with the time per epoch).  (profiles/hs_bench.json also holds the
hot_nodes 16 / 64 / 256 points of the atomic variant the library now refuses.)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from node2vec_amd import hs, sgns, synthetic  # noqa: E402
from node2vec_amd import randomwalk as rw  # noqa: E402

# random 512-byte row reads, measured on one MI355X (the SGNS rows of cfg 5)
ROW_CEILING = 5.7e12
CACHE_BYTES_PER_WAVE = 8192  # csrc/n2v_hs.hip kCacheBytesPerWave (hogwild: both copies of a cached row)


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


def corpus(scale):
    g = synthetic.rmat(scale, 5 << scale, device="cuda")
    walks, _ = rw.walk(g, rw.start_vertices(g), 1, 80, 1.0, 1.0, 7)
    vocab = sgns.build_vocab(walks, 1)
    idx = vocab.index_of[walks.long()]
    return vocab, idx, g


def link_auc(g, vocab, hot_list, idx, epochs=2, n=200000):
    """link AUC on the corpus graph after `epochs` hogwild epochs of HS at dim 128, by hot_nodes: cosine of
    the endpoints of n sampled edges against n random vertex pairs"""
    gen = torch.Generator(device="cuda").manual_seed(3)
    rowptr, col = g.rowptr, g.col
    e = torch.randint(0, col.numel(), (n,), generator=gen, device="cuda")
    src = torch.searchsorted(rowptr, e, right=True) - 1
    lut = torch.full((rowptr.numel() - 1,), -1, dtype=torch.int64, device="cuda")
    lut[vocab.ids.long()] = torch.arange(len(vocab), device="cuda")
    a, b = lut[src], lut[col[e].long()]
    ra = torch.randint(0, len(vocab), (n,), generator=gen, device="cuda")
    rb = torch.randint(0, len(vocab), (n,), generator=gen, device="cuda")
    ok = (a >= 0) & (b >= 0)
    out = {}
    for hot in hot_list:
        m = hs.HsModel(vocab, 128, 5, seed=1)
        m.hot_nodes = hot
        t0 = time.perf_counter()
        m.train(idx, epochs, 0.025)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        v = torch.nn.functional.normalize(m.syn0, dim=1)
        pos = (v[a[ok]] * v[b[ok]]).sum(1).cpu().numpy()
        neg = (v[ra] * v[rb]).sum(1).cpu().numpy()
        neg.sort()
        auc = float(np.searchsorted(neg, pos, side="left").mean() / neg.size)
        out[str(hot)] = {"link_auc": round(auc, 4), "s_per_epoch": round(el / epochs, 3)}
    return out


def hs_point(vocab, rows, dim, seconds, hot_nodes=None, path_cache=True):
    m = hs.HsModel(vocab, dim, 5, seed=1)
    m.hot_nodes, m.path_cache = hot_nodes, path_cache
    launch = {"n": 0}

    def run():
        m.train_block(rows, 0.025, launch["n"] * rows.shape[0])
        launch["n"] += 1

    m._counters.zero_()
    t, calls = timed(run, seconds)
    pairs = int(m.pairs.item()) / (calls + 1)
    positions = int((rows >= 0).sum().item())
    L = m.mean_code_length
    # the top `cached` levels of a path move once per centre position, the levels below once per pair
    vec = 1 << max(0, (dim - 1).bit_length() - 6)
    cached = min(64, CACHE_BYTES_PER_WAVE // (2 * 256 * vec)) if path_cache else 0
    c = m.vocab.counts.cpu().numpy().astype(np.float64)
    Lc = float((c * np.minimum(m.tree.lengths, cached)).sum() / c.sum())
    per_pair = 8.0 * dim * (1.0 + (L - Lc) + Lc * positions / pairs)
    assert np.isfinite(m.syn0[:1000].cpu().numpy()).all()
    return {"dim": dim, "hot_nodes": hs.HOT_NODES if hot_nodes is None else hot_nodes, "path_cache": path_cache,
            "rows": int(rows.shape[0]), "waves": m.hogwild_waves_used, "ms_per_launch": round(t * 1e3, 3),
            "calls": calls, "pairs_per_launch": int(pairs), "hs_Mpairs_per_s": round(pairs / t / 1e6, 1),
            "mean_code_length": round(L, 3), "cached_levels": cached, "mean_cached_levels": round(Lc, 3), "node_updates_G_per_s": round(pairs * L / t / 1e9, 2),
            "algorithmic_bytes_per_pair": round(per_pair, 1),
            "algorithmic_TBps": round(pairs * per_pair / t / 1e12, 3),
            "share_of_row_ceiling": round(pairs * per_pair / t / ROW_CEILING, 3)}


def sgns_point(vocab, rows, dim, seconds):
    m = sgns.SgnsModel(vocab, dim, 5, 5, seed=1, sample=0.0)
    launch = {"n": 0}

    def run():
        m.train_block(rows, 0.025, launch["n"] * rows.shape[0])
        launch["n"] += 1

    t, calls = timed(run, seconds)
    pairs = int(m.pairs.item()) / (calls + 1)
    return {"sgns_Mpairs_per_s": round(pairs / t / 1e6, 1), "sgns_hub_rows": m.hub_rows}


def _planted(nc=50, sz=40, seed=0):
    """the planted-partition graph of tests/test_sgns_batched_gpu.py"""
    from node2vec_amd.graph import DeviceGraph

    rng = np.random.default_rng(seed)
    nv = nc * sz
    comm = np.repeat(np.arange(nc), sz)
    src, dst = [], []
    for v in range(nv):
        inside = rng.choice(np.nonzero(comm == comm[v])[0], 8)
        for u in list(inside) + list(rng.integers(0, nv, 2)):
            if u != v:
                src += [v, int(u)]
                dst += [int(u), v]
    return DeviceGraph.from_edges(src, dst, None, n_vertices=nv, device="cuda"), comm


def _unit(v):
    v = v - v.mean(0)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def planted_quality(hot_list):
    g, comm = _planted()
    walks, _ = rw.walk(g, rw.start_vertices(g), 10, 40, 1.0, 1.0, 1)
    vocab = sgns.build_vocab(walks, 1)
    rows = hs.sentences(vocab.index_of[walks.long()], 10000)
    ids = vocab.ids.cpu().numpy()
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, len(ids), 200000), rng.integers(0, len(ids), 200000)
    same = comm[ids[a]] == comm[ids[b]]
    out = {}
    for hot in hot_list:
        m = hs.HsModel(vocab, 64, 5, seed=7)
        m.hot_nodes = None if hot == "det" else hot
        m.train(rows, 3, 0.025, deterministic=hot == "det")
        v = _unit(m.syn0.cpu().numpy())
        s = (v[a] * v[b]).sum(1)
        out[str(hot)] = round(float((s[same][:, None] > s[~same][None, :3000]).mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--variants", action="store_true", help="the path cache off at dim 128")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hs_bench needs a HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    t0 = time.perf_counter()
    vocab, idx, g = corpus(a.scale)
    t_tree = time.perf_counter()
    hs.build_tree(vocab.counts)
    emit({"corpus": f"rmat{a.scale}", "vocab": len(vocab), "rows": int(idx.shape[0]), "len": int(idx.shape[1]),
          "setup_s": round(t_tree - t0, 2), "tree_build_s": round(time.perf_counter() - t_tree, 3)})
    rows = idx[:a.rows].contiguous()
    for dim in a.dims:
        rec = hs_point(vocab, rows, dim, a.seconds)
        rec.update(sgns_point(vocab, rows, dim, a.seconds))
        emit(rec)
    if a.variants:
        emit(hs_point(vocab, rows, 128, a.seconds, path_cache=False))
    if a.quality:
        emit({"planted_auc": planted_quality(["det", 0])})
        emit({"rmat_link_auc": link_auc(g, vocab, [0], idx)})


if __name__ == "__main__":
    main()
