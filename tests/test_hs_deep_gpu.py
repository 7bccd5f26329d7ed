"""The HS trainer (csrc/n2v_hs.hip) on Huffman codes of 32 .. 64 bits, bit for bit.

A word's code is one uint64 and its path sits in the 64 lanes of a wave ("len <= 64"); the other GPU
tests stop at codes of 23 bits.  The vocabularies of tests/hs_deep_cases.py reach bit 32, bit 63 and
lane 63, and test_hs_host.py shows with the CPU restatement alone that their corpora notice a code
masked to 32 bits, a lost bit 63 and a path cut at level 32 or 63.  Everything here is exact equality
of bits with tests/cpu_hs/n2v_hs_cpu.c except the many-wave run, which races by design.
"""
import numpy as np
import pytest
import torch

import hs_deep_cases as deep
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)

pytestmark = pytest.mark.gpu

VOCABS = {"fib33": lambda: deep.fib_counts(33), "fib34": lambda: deep.fib_counts(34),
          "fib65": lambda: deep.fib_counts(65), "mixed": deep.mixed_counts}
LONGEST = {"fib33": 32, "fib34": 33, "fib65": 64, "mixed": 48}


def _model(name, dim, seed):
    from node2vec_amd import hs

    counts = VOCABS[name]()
    m = hs.HsModel(deep.vocab(counts, "cuda"), dim, deep.WINDOW, seed=seed)
    assert int(m.tree.lengths.max()) == LONGEST[name]
    assert np.array_equal(m.codes.cpu().numpy().view(np.uint64), m.tree.codes)
    return m


def _cpu(L, m, walks, s0, s1, base, alpha, row_alpha=None):
    t = m.tree
    return deep.cpu_train(L, walks, s0, s1, t.path_off, t.points, t.codes, m.seed, m.window, base, alpha, row_alpha)


def _check_bits(L, m, walks, launches=((0, 0.025, None),), deterministic=True):
    """the pattern of test_hs_gpu._check_bits, on bit patterns; returns the restatement's (syn0, syn1)"""
    idx = torch.from_numpy(walks).cuda()
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    n = 0
    for base, alpha, ra in launches:
        m.train_block(idx, alpha, base, deterministic=deterministic,
                      row_alpha=None if ra is None else torch.from_numpy(ra).cuda())
        n += _cpu(L, m, walks, s0, s1, base, alpha, ra)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n > 0
    g0, g1 = m.syn0.cpu().numpy(), m.syn1.cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(g1).all()
    deep.same_bits("syn0", g0, s0)
    deep.same_bits("syn1", g1, s1)
    return s0, s1


# dim -> VEC 1, 1, 2, 4, 8, 16: a ragged or a full row of each.  What `d < nc` does in each cached case,
# from hs_cache_rows (64 / 64 / 64 / 32 / 16 / 8 rows at these dims) and the longest code:
#   VEC 1 and 2 keep every path in LDS; V = 65 uses the last of the 64 slots and lane 63 of my_point;
#   dim 256 (32 rows): V = 33 fills the cache exactly, V = 34 leaves one level, d = 32, to the per-pair loads;
#   every other case has words on both sides: paths that end inside the cache and paths that go past it.
DIMS = [16, 64, 100, 256, 300, 1024]
BRANCH = {(name, dim): "straddles" for name in VOCABS for dim in DIMS}
for _name in VOCABS:
    for _dim in (16, 64, 100):
        BRANCH[_name, _dim] = "fills" if _name == "fib65" else "inside"
BRANCH["fib33", 256] = "fills"


@pytest.mark.parametrize("path_cache", [True, False])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(VOCABS))
def test_deterministic_bit_identical_on_deep_codes(hs_cpu, name, dim, path_cache):
    m = _model(name, dim, seed=dim + len(name))
    m.path_cache = path_cache
    lens = m.tree.lengths
    cache = deep.CACHE_ROWS_DETERMINISTIC[deep.vec_width(dim)] if path_cache else 0
    branch = deep.cache_branch(lens, cache)
    print(name, "dim", dim, "cache rows", cache, "code lengths", int(lens.min()), "..", int(lens.max()), "->", branch)
    assert branch == (BRANCH[name, dim] if path_cache else "uncached")
    if branch == "straddles":  # a word on each side of the boundary, and one that ends exactly on it
        assert (lens < cache).any() and (lens == cache).any() and (lens > cache).any()
    _, s1 = _check_bits(hs_cpu, m, deep.corpus(len(lens), seed=dim))
    deepest = m.tree.path(int(np.argmax(lens)))
    assert np.abs(s1[deepest]).max(1).min() > 0  # every level of the longest path trained


@pytest.mark.parametrize("dim", [16, 128, 256, 512, 1024])
@pytest.mark.parametrize("name", ["fib65", "mixed"])
def test_single_wave_hogwild_on_deep_codes(hs_cpu, name, dim):
    """hogwild mode on one wave: caches of 16 / 8 / 4 / 2 / 1 rows (both LDS copies), so every long path
    has 48 or more levels behind the cache; at dim 1024 the one cached row shares its group of 2 nodes
    with an uncached one"""
    m = _model(name, dim, seed=3 + dim)
    cache = deep.CACHE_ROWS_HOGWILD[deep.vec_width(dim)]
    # (the shortest code of `mixed` has 2 bits: past a cache of one row)
    assert deep.cache_branch(m.tree.lengths, cache) == ("past" if (name, cache) == ("mixed", 1) else "straddles")
    assert (cache % deep.GROUP_NODES[deep.vec_width(dim)] != 0) == (dim == 1024)
    m.max_waves, m.hot_nodes = 1, 0
    _check_bits(hs_cpu, m, deep.corpus(len(m.tree.lengths), seed=dim + 1), deterministic=False)
    assert m.hogwild_waves_used == 1


@pytest.mark.parametrize("dim", [100, 300])
def test_two_launches_with_per_row_rates_on_deep_codes(hs_cpu, dim):
    """the second launch starts from deep syn1 rows that are already non-zero; Spark's rate per row"""
    from node2vec_amd import hs

    m = _model("fib65", dim, seed=11)
    walks = deep.corpus(65, seed=dim + 2)
    words = (walks >= 0).sum(1)
    launches = [(ep * walks.shape[0], 0.025, hs.spark_row_alpha(words * 4000, ep, 2, 0.025)) for ep in range(2)]
    assert len({float(a) for _, _, ra in launches for a in ra}) > 2
    mid0, mid1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    _cpu(hs_cpu, m, walks, mid0, mid1, *launches[0])
    deepest = m.tree.path(64)
    assert len(deepest) == 64 and np.abs(mid1[deepest[32:]]).max(1).min() > 0  # what the second launch starts from
    _check_bits(hs_cpu, m, walks, launches)


@pytest.mark.parametrize("path_cache", [True, False])
@pytest.mark.parametrize("dim", [64, 256, 1024])
def test_saturated_nodes_deep_in_the_path(hs_cpu, dim, path_cache):
    """syn1 rows of depths 31, 32 and 63 are [8, 0, ...] and syn0[:, 0] = 1 (the construction of
    conflict_free.py): their f stays >= 6, so the `continue` inside a node group fires at d = 31, 32 and
    63 beside nodes that train, and those rows are never written"""
    m = _model("fib65", dim, seed=dim)
    m.path_cache = path_cache
    chain = m.tree.path(64)  # the chain's inner nodes, root first: chain[d] is THE node of depth d
    assert len(chain) == 64 and len(set(chain.tolist())) == 64
    preset = chain[[31, 32, 63]]
    m.syn0[:, 0] = 1.0
    m.syn1[torch.from_numpy(preset).long().cuda(), 0] = deep.SATURATED
    before = m.syn1.cpu().numpy().copy()
    s0, s1 = _check_bits(hs_cpu, m, deep.corpus(65, seed=dim + 3))
    deep.same_bits("the saturated rows", s1[preset], before[preset])
    others = np.setdiff1d(chain, preset)
    assert (s1[others] != before[others]).any(1).all()  # every other level trained, those past 32 too
    assert (s0[:, 0] * deep.SATURATED >= 6.0).all()


def test_hogwild_pair_count_and_finite_on_mixed_codes(hs_cpu):
    """several waves on short and long codes: races by design, so the pair count and finiteness only"""
    m = _model("mixed", 128, seed=1)
    walks = deep.corpus(80, seed=9, rows=64)
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    m.train_block(torch.from_numpy(walks).cuda(), 0.025, 0)
    torch.cuda.synchronize()
    assert m.hogwild_waves_used > 1
    assert int(m.pairs.item()) == _cpu(hs_cpu, m, walks, s0, s1, 0, 0.025) > 0
    g0, g1 = m.syn0.cpu().numpy(), m.syn1.cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and np.abs(g1).max() > 0
