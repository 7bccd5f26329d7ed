"""Hierarchical softmax (Node2VecSpark), the parts that need no GPU: n2v_hs_tree_build against a
pure-Python restatement of word2vec.c CreateBinaryTree, the CPU restatement of the HS update
(tests/cpu_hs/n2v_hs_cpu.c) against a float64 numpy HS update, Spark's learning-rate rule against
a sequential loop, the C ABI's argument checks, and the host logic of Node2VecSpark."""
import ctypes as C
import os
import time
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import cpu_build
from conftest import ROOT



@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def hs_cpu(tmp_path_factory):
    """the CPU restatement, built once per session by cpu_build"""
    L = cpu_build.build("cpu_hs/n2v_hs_cpu.c", tmp_path_factory.mktemp("hs_cpu"))
    L.n2v_hs_cpu_train.restype = C.c_int64
    L.n2v_hs_cpu_train.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                   C.c_float, C.c_void_p]
    L.n2v_hs_cpu_windows.restype = C.c_int
    L.n2v_hs_cpu_windows.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_uint64, C.c_int32,
                                     C.c_void_p]
    return L


def create_binary_tree(counts):
    """word2vec.c CreateBinaryTree, line by line (count[] of 2V + 1 with the 1e15 sentinel as an
    unbounded integer here, the reversal of code / point into root-first order)"""
    V = len(counts)
    count = [int(c) for c in counts] + [10 ** 30] * (V + 1)
    binary = [0] * (2 * V + 1)
    parent = [0] * (2 * V + 1)
    pos1, pos2 = V - 1, V
    for a in range(V - 1):
        if pos1 >= 0 and count[pos1] < count[pos2]:
            min1i, pos1 = pos1, pos1 - 1
        else:
            min1i, pos2 = pos2, pos2 + 1
        if pos1 >= 0 and count[pos1] < count[pos2]:
            min2i, pos1 = pos1, pos1 - 1
        else:
            min2i, pos2 = pos2, pos2 + 1
        count[V + a] = count[min1i] + count[min2i]
        parent[min1i] = V + a
        parent[min2i] = V + a
        binary[min2i] = 1
    codes, points = [], []
    for a in range(V):
        if V == 1:
            codes.append([])
            points.append([])
            continue
        b, code, point = a, [], []
        while True:
            code.append(binary[b])
            point.append(b)
            b = parent[b]
            if b == 2 * V - 2:
                break
        n = len(code)
        codes.append([code[n - k - 1] for k in range(n)])
        pt = [V - 2] + [point[n - k] - V for k in range(1, n)]
        points.append(pt)
    return codes, points


def _check_tree(counts):
    from node2vec_amd import hs

    t = hs.build_tree(np.asarray(counts, np.int64))
    want_codes, want_points = create_binary_tree(counts)
    V = len(counts)
    for w in range(V):
        assert t.code(w) == want_codes[w], w
        assert t.path(w).tolist() == want_points[w], w
    if V > 1:
        lens = t.lengths
        assert Fraction(0) + sum(Fraction(1, 2 ** int(n)) for n in lens) == 1  # Kraft sum, exactly
        words = {tuple(t.code(w)) for w in range(V)}
        assert len(words) == V
        for w in range(V):  # prefix-free
            c = tuple(t.code(w))
            assert not any(c[:k] in words for k in range(1, len(c)))
        assert t.points.min() >= 0 and t.points.max() < V - 1
        assert all(t.path(w)[0] == V - 2 for w in range(V))
    else:
        assert t.lengths.tolist() == [0]
    return t


@pytest.mark.parametrize("kind", ["random", "powerlaw", "equal", "ties"])
@pytest.mark.parametrize("V", [3, 10, 257, 5000])
def test_tree_build_equals_create_binary_tree(lib, kind, V):
    rng = np.random.default_rng(V + len(kind))
    if kind == "random":
        c = rng.integers(1, 10 ** 6, V)
    elif kind == "powerlaw":
        c = (1e7 / np.arange(1, V + 1) ** 1.1).astype(np.int64) + 1
    elif kind == "equal":
        c = np.full(V, 7)
    else:
        c = rng.integers(1, 4, V) * 5
    _check_tree(np.sort(c)[::-1].copy())


def test_tree_build_large_and_tiny_vocabularies(lib):
    rng = np.random.default_rng(3)
    c = np.sort((rng.pareto(1.2, 100000) * 10).astype(np.int64) + 1)[::-1].copy()
    from node2vec_amd import hs

    t = hs.build_tree(c)
    want_codes, want_points = create_binary_tree(c)
    for w in range(0, len(c), 97):
        assert t.code(w) == want_codes[w] and t.path(w).tolist() == want_points[w]
    assert Fraction(0) + sum(Fraction(1, 2 ** int(n)) for n in t.lengths) == 1
    for V in (1, 2, 3):
        _check_tree(list(range(V + 5, 5, -1)))
    assert _check_tree([4, 4]).lengths.tolist() == [1, 1]


def test_tree_build_refuses_unsorted_counts_and_codes_past_64_bits(lib):
    from node2vec_amd import hs

    with pytest.raises(ValueError):
        hs.build_tree(np.array([1, 5, 3]))
    fib = [1, 1]
    while len(fib) < 70:
        fib.append(fib[-1] + fib[-2])
    with pytest.raises(ValueError):  # Fibonacci counts: a chain, code length 69
        hs.build_tree(np.array(fib[::-1], np.int64))
    assert int(hs.build_tree(np.array(fib[:64][::-1], np.int64)).lengths.max()) == 63


def _mix64(z):
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _reference_f64(walks, syn0, syn1, tree, n_vocab, seed, sentence_base, window, alphas, exp_tab):
    """skip-gram HS in float64, sequential, from the published rules (windows from the same stream)"""
    m = (1 << 64) - 1
    pairs = 0
    for r in range(walks.shape[0]):
        hs_ = _mix64(seed ^ _mix64((sentence_base + r + 0xA0761D6478BD642F) & m))
        sent, red = [], []
        for t, tok in enumerate(walks[r]):
            if 0 <= tok < n_vocab:
                sent.append(int(tok))
                red.append((_mix64((hs_ + (2 * t + 2) * 0xE7037ED1A0B428DB) & m) >> 32) % window)
        for i, c in enumerate(sent):
            lo, hi = max(0, i - window + red[i]), min(len(sent), i + window + 1 - red[i])
            code, path = tree.code(c), tree.path(c)
            for j in range(lo, hi):
                if j == i:
                    continue
                pairs += 1
                x = syn0[sent[j]]
                neu = np.zeros_like(x)
                for d, p in enumerate(path):
                    f = float(x @ syn1[p])
                    if f <= -6 or f >= 6:
                        continue
                    g = (1 - code[d] - float(exp_tab[int((f + 6) * 83)])) * alphas[r]
                    neu += g * syn1[p]
                    syn1[p] += g * x
                syn0[sent[j]] = x + neu
    return pairs


@pytest.mark.parametrize("dim,window", [(16, 2), (63, 5), (100, 3)])
def test_restatement_computes_hierarchical_softmax(lib, hs_cpu, dim, window):
    """the CPU restatement against a float64 HS update: within dim * 2^-22"""
    from node2vec_amd import hs, sgns

    rng = np.random.default_rng(dim)
    V = 40
    counts = np.sort(rng.integers(1, 200, V))[::-1].copy()
    tree = hs.build_tree(counts)
    walks = rng.integers(-2, V + 2, (12, 20)).astype(np.int32)
    syn0 = ((rng.random((V, dim)) - 0.5) / dim).astype(np.float32)
    syn1 = ((rng.random((V - 1, dim)) - 0.5) * 0.4).astype(np.float32)
    alphas = np.linspace(0.025, 0.02, walks.shape[0]).astype(np.float32)
    exp_tab = sgns.exp_table()
    s0, s1 = syn0.copy(), syn1.copy()
    pts = np.ascontiguousarray(tree.points)
    n = hs_cpu.n2v_hs_cpu_train(walks.ctypes.data, walks.shape[0], walks.shape[1], s0.ctypes.data, s1.ctypes.data,
                                tree.path_off.ctypes.data, pts.ctypes.data, tree.codes.ctypes.data,
                                exp_tab.ctypes.data, V, 5, 77, dim, window, 0.0, alphas.ctypes.data)
    d0, d1 = syn0.astype(np.float64), syn1.astype(np.float64)
    want = _reference_f64(walks, d0, d1, tree, V, 77, 5, window, alphas.astype(np.float64), exp_tab)
    assert n == want > 0
    tol = dim * 2.0 ** -22
    assert np.abs(s0 - d0).max() <= tol and np.abs(s1 - d1).max() <= tol
    assert np.abs(s1 - syn1).max() > 100 * tol  # it trained


def test_spark_rate_per_row_equals_the_sequential_loop():
    from node2vec_amd import hs

    rng = np.random.default_rng(5)
    words = rng.integers(0, 81, 3000)
    train_words = int(words.sum())
    step, epochs = 0.025, 3
    for ep in range(epochs):
        got = hs.spark_row_alpha(words, ep, epochs, step)
        # the issue's floored rule as a loop: the rate is recomputed at every multiple of 10 000 words
        # (Spark's own loop refreshes when MORE than 10 000 words passed and keeps the unfloored count)
        alpha, refreshed, wc, want = step, 0, 0, []
        alpha = step * max(1e-4, 1 - (ep * train_words) / (epochs * train_words + 1))
        for w in words:
            if wc - refreshed >= 10000:
                refreshed = wc - wc % 10000
                alpha = step * max(1e-4, 1 - (ep * train_words + refreshed) / (epochs * train_words + 1))
            want.append(np.float32(alpha))
            wc += int(w)
        assert np.array_equal(got, np.array(want, np.float32))
    assert hs.spark_row_alpha([10 ** 6], 0, 1, 0.1, 10 ** 6)[0] == np.float32(0.1)
    assert hs.spark_row_alpha([5, 5], 3, 1, 0.1)[0] == np.float32(0.1 * 1e-4)


def test_sentences_drop_oov_tokens_then_cut_rows():
    from node2vec_amd import hs

    idx = torch.tensor([[3, -1, 4, 5, -1, 6], [-1, -1, -1, -1, -1, -1], [1, 2, -1, -1, -1, 7]], dtype=torch.int32)
    assert hs.sentences(idx, 10000).tolist() == [[3, 4, 5, 6], [1, 2, 7, -1]]
    assert hs.sentences(idx, 3).tolist() == [[3, 4, 5], [6, -1, -1], [1, 2, 7]]
    assert hs.sentences(idx, 1).tolist() == [[3], [4], [5], [6], [1], [2], [7]]
    long = torch.arange(600, dtype=torch.int32).reshape(1, 600)
    out = hs.sentences(long, 10000)
    assert out.shape == (3, 256) and out[2, 88:].eq(-1).all() and out[out >= 0].tolist() == list(range(600))


def test_hs_abi_refuses_bad_arguments_without_a_gpu(lib):
    from node2vec_amd import _lib

    L = lib
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def P(**kw):
        d = dict(n_vocab=10, sentence_base=0, seed=1, dim=16, window=5, alpha=0.025, deterministic=0,
                 row_alpha=None, max_waves=0, hot_nodes=0, path_cache=1, reserved=0)
        d.update(kw)
        return _lib.HsParams(**d)

    def train(n_walks=1, walk_len=8, ptrs=True, **kw):
        q = p if ptrs else None
        return L.n2v_hs_train(q, n_walks, walk_len, q, q, q, q, q, q, P(**kw), None, None)

    assert train(n_walks=0) == _lib.OK  # nothing to do: nothing launched
    for kw in (dict(dim=0), dict(dim=1025), dict(window=0), dict(window=33), dict(n_vocab=0),
               dict(n_vocab=1 << 31), dict(deterministic=2), dict(path_cache=2), dict(hot_nodes=-1),
               dict(max_waves=-1), dict(hot_nodes=1), dict(walk_len=0), dict(walk_len=257), dict(n_walks=-1), dict(ptrs=False)):
        assert train(**kw) == _lib.EINVAL, kw
    assert L.n2v_hs_train(p, 1, 8, p, p, p, p, p, p, None, None, None) == _lib.EINVAL
    assert L.n2v_hs_hogwild_waves(P(dim=0), 10, 8) == _lib.EINVAL
    assert L.n2v_hs_hogwild_waves(P(), 0, 8) == 0
    off = (C.c_int64 * 4)()
    codes = (C.c_uint64 * 3)()
    cnt = (C.c_int64 * 3)(5, 3, 1)
    assert L.n2v_hs_tree_build(None, 3, off, codes, None, 0) == _lib.EINVAL
    assert L.n2v_hs_tree_build(cnt, 0, off, codes, None, 0) == _lib.EINVAL
    assert L.n2v_hs_tree_build(cnt, 3, off, codes, None, 0) == _lib.OK and off[3] == 5
    pts = (C.c_int32 * 5)()
    assert L.n2v_hs_tree_build(cnt, 3, off, codes, pts, 4) == _lib.EINVAL  # too small for the points
    assert L.n2v_hs_tree_build(cnt, 3, off, codes, pts, 5) == _lib.OK and pts[0] == 1
    neg = (C.c_int64 * 3)(5, 3, -1)
    assert L.n2v_hs_tree_build(neg, 3, off, codes, None, 0) == _lib.EINVAL


def test_hs_params_layout_matches_the_header():
    import re

    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    body = text[text.index("typedef struct n2v_hs_params {"):text.index("} n2v_hs_params;")]
    fields = re.findall(r"\*?\s*\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.HsParams._fields_]
    assert C.sizeof(_lib.HsParams) == 3 * 8 + 4 * 4 + 8 + 4 * 4


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_node2vecspark_host_logic():
    """tests/test_embedding.py:87-135 of the reference, the parts before fit()"""
    from node2vec_amd.constants import WORD2VEC_PARAMS
    from node2vec_amd.embedding import Node2VecSpark

    params = {}
    t0 = int(time.time())
    n2v = Node2VecSpark(WALKS, w2v_params=params)
    assert isinstance(n2v, Node2VecSpark)
    assert set(WORD2VEC_PARAMS) <= set(params)
    assert {k: params[k] for k in WORD2VEC_PARAMS if k != "seed"} == {
        k: v for k, v in WORD2VEC_PARAMS.items() if k != "seed"}
    assert t0 <= params["seed"] <= int(time.time())  # int(time.time()), not // 60
    params = {"maxIter": 3, "seed": 5}
    n2v = Node2VecSpark(WALKS, w2v_params=params, window_size=6, vector_size=64, random_seed=1000)
    assert params["seed"] == 1000 and params["windowSize"] == 6 and params["vectorSize"] == 64
    assert params["maxIter"] == 3 and params["minCount"] == WORD2VEC_PARAMS["minCount"]
    for kw in (dict(window_size=3), dict(window_size=31), dict(vector_size=16), dict(vector_size=2048)):
        with pytest.raises(ValueError):
            Node2VecSpark(WALKS, {}, **kw)
    with pytest.raises(TypeError):
        Node2VecSpark(WALKS, {"min_count": 1})
    for bad in ({"vectorSize": 0}, {"windowSize": -1}, {"stepSize": 0.0}, {"numPartitions": 0},
                {"maxSentenceLength": 0}, {"maxIter": -1}, {"minCount": -1}):
        with pytest.raises(ValueError):
            Node2VecSpark(WALKS, dict(bad))
    n2v = Node2VecSpark(WALKS, {"minCount": 0, "maxIter": 1, "maxSentenceLength": 1, "windowSize": 4})
    with pytest.raises(ValueError):
        n2v.embedding()
    with pytest.raises(ValueError):
        n2v.get_vector(1)


# ---- codes of 33 .. 64 bits (tests/hs_deep_cases.py) ---------------------------------------------------------

@pytest.mark.parametrize("V,longest", [(33, 32), (34, 33), (64, 63), (65, 64)])
def test_tree_build_at_the_depth_boundary(lib, V, longest):
    """Fibonacci counts: a chain whose two deepest words have codes of `longest` bits; 65 bits are refused"""
    import hs_deep_cases as deep

    t = _check_tree(deep.fib_counts(V))  # word for word against create_binary_tree, codes and points
    assert int(t.lengths.max()) == longest and int((t.lengths == longest).sum()) == 2
    assert t.codes.dtype == np.uint64 and t.path_off.dtype == np.int64
    if V == 65:
        assert any((int(c) >> 63) & 1 for c in t.codes)  # as a Python int: no sign, no wrap


def test_tree_build_refuses_a_code_of_65_bits(lib):
    import hs_deep_cases as deep
    from node2vec_amd import hs

    assert int(deep.fib_counts(66).sum()) < 2 ** 61  # refused for its depth, not for its sums
    with pytest.raises(ValueError):
        hs.build_tree(deep.fib_counts(66))


def test_mixed_counts_give_short_and_long_codes(lib):
    import hs_deep_cases as deep

    c = deep.mixed_counts()
    assert len(c) == 80 and (np.diff(c) <= 0).all()
    t = _check_tree(c)
    assert int(t.lengths.min()) == 2 and int(t.lengths.max()) == 48
    assert int((t.lengths <= 8).sum()) >= 30 and int((t.lengths > 32).sum()) >= 10


def test_model_keeps_bit_63_of_the_codes(lib):
    """uint64 -> int64 -> torch in HsModel: the tensor, viewed back as uint64, is tree.codes"""
    import hs_deep_cases as deep
    from node2vec_amd import hs

    m = hs.HsModel(deep.vocab(deep.fib_counts(65)), 16, 5, seed=1)
    assert m.codes.dtype == torch.int64 and int(m.codes.min()) < 0  # bit 63 is the sign there
    back = m.codes.cpu().numpy().view(np.uint64)
    assert np.array_equal(back, m.tree.codes) and any((int(c) >> 63) & 1 for c in back)
    assert np.array_equal(m.path_off.cpu().numpy(), m.tree.path_off)
    assert np.array_equal(m.points.cpu().numpy(), m.tree.points)


def _deep_mutants(tree, V):
    """trees that are wrong only past bit / level 31 (V = 65: also only at bit / level 63)"""
    import hs_deep_cases as deep

    out = {"codes masked to 32 bits": (tree.path_off, tree.points, tree.codes & np.uint64(0xFFFFFFFF)),
           "paths cut to 32 nodes": deep.cut_paths(tree, 32)}
    if V == 65:
        out["bit 63 cleared"] = (tree.path_off, tree.points, tree.codes & np.uint64(2 ** 63 - 1))
        out["paths cut to 63 nodes"] = deep.cut_paths(tree, 63)
    return out


@pytest.mark.parametrize("V", [34, 65])
def test_deep_cases_tell_a_wrong_deep_level_from_the_true_tree(lib, hs_cpu, V):
    """A condition on the INPUTS of tests/test_hs_deep_gpu.py, shown with the restatement alone: the
    corpus trains bit 32 (V = 65: and bit 63) of a code and level 32 (63) of a path, so a trainer that
    gets them wrong cannot produce the restatement's bits."""
    import hs_deep_cases as deep
    from node2vec_amd import hs

    dim = 16
    tree = hs.build_tree(deep.fib_counts(V))
    walks = deep.corpus(V, seed=V)

    def train(path_off, points, codes):
        s0, s1 = deep.syn0_init(V, dim, seed=V), np.zeros((V - 1, dim), np.float32)
        n = deep.cpu_train(hs_cpu, walks, s0, s1, path_off, points, codes, seed=7, window=deep.WINDOW)
        return s0, s1, n

    t0, t1, n = train(tree.path_off, tree.points, tree.codes)
    assert n > 0 and np.abs(t1).max() > 1e-3
    for name, (off, pts, codes) in _deep_mutants(tree, V).items():
        assert len(off) == V + 1 and off[-1] == len(pts) <= len(tree.points)
        m0, m1, mn = train(off, pts, codes)
        assert mn == n, name  # the pairs do not depend on the tree
        changed = not (np.array_equal(m0, t0) and np.array_equal(m1, t1))
        assert changed, f"{name}: the case does not notice"
