"""Vocabularies whose Huffman codes are 32 .. 64 bits long, and what the HS tests on them share.

n2v_hs_tree_build accepts trees up to 64 levels and the kernel keeps a word's code in one uint64 and
its path in the 64 lanes of a wave, so the bits and lanes past 31 must be trained on, not only built.
Fibonacci counts give a pure chain, the smallest vocabulary that reaches a given depth:

    V        33  34  64  65  66
    longest  32  33  63  64  65 (refused)      (two words share the longest code)

The counts only shape the tree; the corpora are uniform (every row a permutation of all words), so
the two deepest words are centres and contexts as often as any other.

Not a test module: helpers shared by tests/test_hs_host.py and tests/test_hs_deep_gpu.py.
"""
import numpy as np

WINDOW = 5
ROWS = 4
# hs_cache_rows (csrc/n2v_hs.hip): path rows kept in LDS per VEC
CACHE_ROWS_DETERMINISTIC = {1: 64, 2: 64, 4: 32, 8: 16, 16: 8}
CACHE_ROWS_HOGWILD = {1: 16, 2: 8, 4: 4, 8: 2, 16: 1}
GROUP_NODES = {1: 8, 2: 8, 4: 4, 8: 2, 16: 2}  # group_nodes<VEC>(): path nodes trained together
SATURATED = 8.0  # conflict_free.SATURATED: f = 8 * syn0[., 0] at a preset row


def fib_counts(V):
    """the first V Fibonacci numbers (1, 1, 2, 3, ...), descending"""
    f = [1, 1]
    while len(f) < V:
        f.append(f[-1] + f[-2])
    return np.array(f[:V][::-1], np.int64)


def mixed_counts():
    """50 Fibonacci numbers and 30 words of count 10^9: a bushy top over a deep chain (code lengths
    2 .. 48), so short and long paths alternate within one sentence"""
    return np.sort(np.concatenate([fib_counts(50), np.full(30, 10 ** 9, np.int64)]))[::-1].copy()


def vec_width(dim):
    v = 1
    while 64 * v < dim:
        v *= 2
    return v


def vocab(counts, device="cpu"):
    """word k is vertex k with count counts[k] (descending): the vocabulary order is the identity"""
    import torch

    from node2vec_amd import sgns

    V = len(counts)
    return sgns.Vocab(torch.arange(V, device=device), torch.from_numpy(np.asarray(counts, np.int64)).to(device),
                      torch.arange(V, dtype=torch.int32, device=device))


def corpus(V, seed, rows=ROWS):
    """`rows` rows, each a seeded permutation of all V words: int32 [rows, V]"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(V) for _ in range(rows)]).astype(np.int32)


def syn0_init(V, dim, seed):
    """word2vec's initialisation, (U[0, 1) - 0.5) / dim, from numpy (for runs of the restatement alone)"""
    rng = np.random.default_rng(seed)
    return ((rng.random((V, dim)) - 0.5) / dim).astype(np.float32)


def cpu_train(L, walks, s0, s1, path_off, points, codes, seed, window, base=0, alpha=0.025, row_alpha=None):
    """the restatement (tests/cpu_hs/n2v_hs_cpu.c) on numpy arrays, s0 / s1 trained in place; the pairs"""
    from node2vec_amd import sgns

    w = np.ascontiguousarray(walks, np.int32)
    off = np.ascontiguousarray(path_off, np.int64)
    pts = np.ascontiguousarray(points, np.int32) if len(points) else np.zeros(1, np.int32)
    cod = np.ascontiguousarray(codes, np.uint64)
    ra = None if row_alpha is None else np.ascontiguousarray(row_alpha, np.float32)
    exp = sgns.exp_table()  # held in a name: the address of a temporary would dangle during the call
    assert s0.dtype == np.float32 and s1.dtype == np.float32 and s0.flags.c_contiguous and s1.flags.c_contiguous
    n = L.n2v_hs_cpu_train(w.ctypes.data, w.shape[0], w.shape[1], s0.ctypes.data, s1.ctypes.data, off.ctypes.data,
                           pts.ctypes.data, cod.ctypes.data, exp.ctypes.data, len(off) - 1, base, seed,
                           s0.shape[1], window, float(alpha), None if ra is None else ra.ctypes.data)
    assert n >= 0
    return int(n)


def cut_paths(tree, keep):
    """the tree with every path cut to its first `keep` nodes: (path_off, points, codes) rebuilt"""
    lens = np.minimum(tree.lengths, keep)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)]).astype(np.int64)
    pts = np.concatenate([tree.path(w)[:lens[w]] for w in range(len(lens))]).astype(np.int32)
    mask = np.uint64((1 << keep) - 1) if keep < 64 else np.uint64(2 ** 64 - 1)
    return off, pts, tree.codes & mask


def same_bits(name, got, want):
    """equality of the bit patterns (so -0.0 is not 0.0), and on a failure where they differ"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (f"{name}: {len(bad)} elements differ, rows {np.unique(bad[:, 0])[:16].tolist()}, "
                           f"largest difference {float(np.abs(got - want).max())}")


def cache_branch(lengths, cache_rows):
    """which side of `d < nc` (nc = min(len, cache_rows)) the paths of a case take in the kernel:
    'inside'    every path is shorter than the cache: all levels from LDS;
    'fills'     the longest path is exactly as long as the cache: all levels from LDS, the last slot used;
    'straddles' some word's path ends inside the cache AND some word's goes past it, so that the levels
                d >= nc are loaded and stored per pair beside cached ones;
    'past'      every path goes past the cache;
    'uncached'  no cache"""
    lo, hi = int(np.min(lengths)), int(np.max(lengths))
    if cache_rows == 0:
        return "uncached"
    if hi < cache_rows:
        return "inside"
    if hi == cache_rows:
        return "fills"
    return "straddles" if lo <= cache_rows else "past"
