"""Is fold-in useful?  A measurement on the CPU (the GPU kernels equal the restatement bit for bit):
    python scripts/foldin_usefulness.py [--seeds 5]

A planted-partition graph: 4 communities of 100 vertices, every vertex with about 10 neighbours inside its community
and 2 outside.  40 vertices (10 per community) are held out; uniform walks (10 per vertex, 40 steps) over the rest
train a skip-gram model with the deterministic trainer restated in oracle/ (dim 32, window 5, 5 negatives, 3 epochs);
walks over the FULL graph from the held-out vertices are then folded in with tests/cpu_foldin/n2v_foldin_cpu.c.
The statistic: the share of held-out vertices whose nearest known vertex (cosine) lies in their own community.
Beside it the same statistic for the same vertices after a full retrain on walks over the full graph: the yardstick.
Prints one line per seed and the spread over the seeds."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

COMMUNITIES, SIZE, HELD_PER_COMMUNITY = 4, 100, 10
DIM, WINDOW, K, EPOCHS, ALPHA, MIN_ALPHA = 32, 5, 5, 3, 0.025, 1e-4
WALKS_PER_VERTEX, LENGTH = 10, 40


def graph(rng):
    n = COMMUNITIES * SIZE
    comm = np.arange(n) // SIZE
    same = comm[:, None] == comm[None, :]
    adj = rng.random((n, n)) < np.where(same, 10.0 / SIZE, 2.0 / (n - SIZE))
    adj = np.triu(adj, 1)
    adj = adj | adj.T
    return comm, [np.flatnonzero(adj[v]) for v in range(n)]


def walk(rng, nbrs, starts, allowed):
    """uniform walks that stay inside `allowed` (a walker with no allowed neighbour stands still), all at once"""
    inside = [nb[allowed[nb]] for nb in nbrs]
    deg = np.array([len(x) for x in inside])
    table = np.zeros((len(nbrs), max(int(deg.max()), 1)), np.int64)
    for v, x in enumerate(inside):
        table[v, :len(x)] = x
    v = np.repeat(np.asarray(starts), WALKS_PER_VERTEX)
    out = np.empty((len(v), LENGTH), np.int64)
    for t in range(LENGTH):
        out[:, t] = v
        pick = (rng.random(len(v)) * deg[v]).astype(np.int64)
        v = np.where(deg[v] > 0, table[v, np.minimum(pick, np.maximum(deg[v] - 1, 0))], v)
    return out


def train(oracle, walks, seed):
    """vocabulary, tables and EPOCHS passes of the oracle's deterministic SGNS; returns (ids, syn0, syn1neg, tables)"""
    from node2vec_amd import sgns

    vocab = sgns.build_vocab(torch.from_numpy(walks), 0)
    n = len(vocab)
    idx = vocab.index_of[torch.from_numpy(walks)].numpy().astype(np.int32)
    cum = sgns.make_cum_table(vocab.counts).numpy()
    syn0 = sgns.init_syn0(n, DIM, seed, "cpu").numpy().copy()
    syn1 = np.zeros((n, DIM), np.float32)
    exp = sgns.exp_table()
    for ep in range(EPOCHS):
        a = max(MIN_ALPHA, ALPHA - (ALPHA - MIN_ALPHA) * ep / EPOCHS)
        oracle.sgns_train(idx, syn0, syn1, cum, None, exp, n, ep * idx.shape[0], seed, DIM, WINDOW, K, a)
    return vocab, syn0, syn1, cum


def own_community_share(comm, held, held_rows, known_ids, known_rows):
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)  # noqa: E731
    nearest = known_ids[np.argmax(unit(held_rows) @ unit(known_rows).T, axis=1)]
    return float(np.mean(comm[nearest] == comm[held]))


def measure(seed, oracle, cpu):
    """(fold-in share, retrain share) for one seed"""
    import foldin_cases as fc
    from node2vec_amd import sgns

    rng = np.random.default_rng(seed)
    comm, nbrs = graph(rng)
    n = len(comm)
    held = np.concatenate([c * SIZE + rng.choice(SIZE, HELD_PER_COMMUNITY, replace=False) for c in range(COMMUNITIES)])
    is_known = np.ones(n, bool)
    is_known[held] = False
    known = np.flatnonzero(is_known)
    vocab, syn0, syn1, cum = train(oracle, walk(rng, nbrs, known, is_known), seed)
    n_vocab = len(vocab)
    # walks over the full graph from the held-out vertices: known words by index, held-out vertex k as n_vocab + k
    grown = walk(rng, nbrs, held, np.ones(n, bool))
    index = np.full(n, -1, np.int64)
    ids = vocab.ids.numpy()
    index[ids] = np.arange(n_vocab)
    index[np.sort(held)] = n_vocab + np.arange(len(held))
    case = {"walks": index[grown].astype(np.int32), "n_vocab": n_vocab, "n_new": len(held), "dim": DIM,
            "window": WINDOW, "negative": K, "syn1neg": syn1, "cum_table": cum.view(np.uint32), "sample_int": None,
            "row_alpha": None, "alpha": ALPHA, "seed": seed, "sentence_base": 0}
    rows = sgns.init_syn0(len(held), DIM, seed ^ 0x666f6c64, "cpu").numpy().copy()
    for ep in range(EPOCHS):
        a = max(MIN_ALPHA, ALPHA - (ALPHA - MIN_ALPHA) * (ep / EPOCHS))
        fc.cpu_pass(cpu, case, rows, alpha=a, sentence_base=ep * grown.shape[0])
    fold = own_community_share(comm, np.sort(held), rows, ids, syn0)
    # the yardstick: a full retrain on walks over the full graph
    vocab2, full0, _, _ = train(oracle, walk(rng, nbrs, np.arange(n), np.ones(n, bool)), seed)
    ids2 = vocab2.ids.numpy()
    row_of = np.full(n, -1, np.int64)
    row_of[ids2] = np.arange(len(ids2))
    keep = is_known[ids2]
    retrain = own_community_share(comm, np.sort(held), full0[row_of[np.sort(held)]], ids2[keep], full0[keep])
    return fold, retrain


def main():
    import foldin_cases as fc
    import n2v_oracle

    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    args = ap.parse_args()
    n2v_oracle.build()
    cpu = fc.build_cpu(tempfile.mkdtemp())
    out = []
    for seed in range(1, args.seeds + 1):
        fold, retrain = measure(seed, n2v_oracle, cpu)
        out.append((fold, retrain))
        print(f"seed {seed}: fold-in {fold:.3f}  full retrain {retrain:.3f}", flush=True)
    f, r = np.array(out).T
    print(f"fold-in {f.mean():.3f} (min {f.min():.3f}, max {f.max():.3f}); retrain {r.mean():.3f} "
          f"(min {r.min():.3f}, max {r.max():.3f}); fold-in - retrain: min {np.min(f - r):+.3f}, max {np.max(f - r):+.3f}")


if __name__ == "__main__":
    main()
