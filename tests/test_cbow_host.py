"""CBOW with negative sampling (sg=0), the parts that need no GPU: the CPU restatement
tests/cpu_cbow/n2v_cbow_cpu.c against a second restatement in numpy float64 with ordinary dot
products, hand-made sentences whose result can be written down, the constructor contract of
Node2VecHIP / SgnsModel, the argument checks of n2v_cbow_train, and the integer replay
tests/cbow_groups.py (which rows a position touches) against the restatement's own counters."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

import cpu_build

M64 = (1 << 64) - 1


@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


def cbow_argtypes():
    """the parameters of n2v_cbow_cpu_train"""
    return [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
            C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p,
            C.c_int32, C.c_int32]


@pytest.fixture(scope="session")
def cbow_cpu(tmp_path_factory):
    """the CPU restatement, built once per session by cpu_build"""
    L = cpu_build.build("cpu_cbow/n2v_cbow_cpu.c", tmp_path_factory.mktemp("cbow_cpu"))
    L.n2v_cbow_cpu_train.restype = C.c_int64
    L.n2v_cbow_cpu_train.argtypes = cbow_argtypes()
    return L


def cpu_train(L, walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, k, alpha, cbow_mean,
              row_alpha=None, stats=None, hub_rows=0, mutation=0):
    """n2v_cbow_cpu_train on numpy arrays (s0 / s1 float32, updated in place); returns the count.  hub_rows > 0:
    the kernel's hub form (atomic adds below hub_rows); mutation: test-only, see the C file"""
    from node2vec_amd import sgns

    w = np.ascontiguousarray(walks, np.int32)
    cum = np.ascontiguousarray(cum).view(np.uint32)
    si = None if sample_int is None else np.ascontiguousarray(sample_int).view(np.uint32)
    ra = None if row_alpha is None else np.ascontiguousarray(row_alpha, np.float32)
    exp = sgns.exp_table()  # held in a name: the address of a temporary would dangle during the call
    assert s0.dtype == np.float32 and s1.dtype == np.float32 and s0.flags.c_contiguous and s1.flags.c_contiguous
    return L.n2v_cbow_cpu_train(w.ctypes.data, w.shape[0], w.shape[1], s0.ctypes.data, s1.ctypes.data,
                                cum.ctypes.data, None if si is None else si.ctypes.data, exp.ctypes.data,
                                n_vocab, base, seed, dim, window, k, float(alpha),
                                None if ra is None else ra.ctypes.data, cbow_mean,
                                None if stats is None else stats.ctypes.data, hub_rows, mutation)


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def reference_cbow(walks, syn0, syn1, cum, sample_int, table, seed, base, window, k, alpha, cbow_mean):
    """float64 restatement of gensim's CBOW negative-sampling update, written from its description:
    filter -> reduced windows -> per position the context sum (or mean), the label-1 target and k
    negatives drawn once per position via bisect_left on the cumulative table, then the error added
    to every context row.  Shares only mix64 with the C file."""
    syn0, syn1 = syn0.astype(np.float64), syn1.astype(np.float64)
    n_vocab, ln = len(cum), walks.shape[1]
    positions = 0
    for r in range(walks.shape[0]):
        hs = mix64(seed ^ mix64(base + r + 0xA0761D6478BD642F))
        draw = lambda idx: mix64(hs + (idx + 1) * 0xE7037ED1A0B428DB)  # noqa: E731
        sent, red = [], []
        for t in range(ln):
            tok = int(walks[r, t])
            if tok < 0 or tok >= n_vocab:
                continue
            if sample_int is not None and int(sample_int[tok]) < (draw(2 * t) >> 32):
                continue
            sent.append(tok)
            red.append((draw(2 * t + 1) >> 32) % window)
        for i, centre in enumerate(sent):
            ctx = [sent[m] for m in range(max(0, i - window + red[i]), min(len(sent), i + window + 1 - red[i]))
                   if m != i]
            if not ctx:
                continue
            neu1 = np.zeros(syn0.shape[1])
            for w in ctx:
                neu1 += syn0[w]
            if cbow_mean:
                neu1 /= len(ctx)
            work = np.zeros(syn0.shape[1])
            for d in range(k + 1):
                if d == 0:
                    target, label = centre, 1.0
                else:
                    idx = 2 * ln + i * k + (d - 1)
                    target = int(np.searchsorted(cum, (draw(idx) >> 16) % int(cum[-1]), side="left"))
                    if target == centre:
                        continue
                    label = 0.0
                f = float(neu1 @ syn1[target])
                if f <= -6.0 or f >= 6.0:
                    continue
                g = (label - float(table[int((f + 6.0) * 83.0)])) * alpha
                work += g * syn1[target]
                syn1[target] += g * neu1
            if not cbow_mean:
                work /= len(ctx)
            for w in ctx:
                syn0[w] += work
            positions += 1
    return syn0, syn1, positions


@pytest.mark.parametrize("cbow_mean", [0, 1])
def test_c_restatement_matches_independent_float64_restatement(cbow_cpu, cbow_mean):
    """the cases and the bound of tests/test_sgns_oracle_independent.py"""
    from node2vec_amd import sgns

    rng = np.random.default_rng(4)
    for dim, window, k, sample in ((16, 5, 5, 0.0), (48, 3, 7, 1e-2), (128, 5, 5, 1e-3)):
        walks = torch.from_numpy(rng.integers(0, 30, size=(12, 15)).astype(np.int32))
        walks[rng.random((12, 15)) < 0.1] = -1
        vocab = sgns.build_vocab(walks, 1)
        idx = torch.where(walks >= 0, vocab.index_of[walks.clamp(min=0).long()],
                          torch.full_like(walks, -1)).numpy()
        cum = sgns.make_cum_table(vocab.counts).numpy().view(np.uint32)
        si = sgns.make_sample_int(vocab.counts, sample)
        si_np = None if si is None else si.numpy().view(np.uint32)
        s0 = sgns.init_syn0(len(vocab), dim, 7, "cpu").numpy()
        s1 = (rng.normal(size=s0.shape) * 0.05).astype(np.float32)  # non-zero outputs: f matters
        table = sgns.exp_table()
        r0, r1, rp = reference_cbow(idx, s0, s1, cum, si_np, table, 99, 1000, window, k, 0.05, cbow_mean)
        c0, c1 = s0.copy(), s1.copy()
        cp = cpu_train(cbow_cpu, idx, c0, c1, cum, si_np, len(vocab), 1000, 99, dim, window, k, 0.05, cbow_mean)
        assert cp == rp and cp > 20
        # fp32 vs fp64 arithmetic and a different summation order: rounding-level agreement
        np.testing.assert_allclose(c0, r0, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(c1, r1, rtol=2e-4, atol=2e-6)
        assert np.abs(c0 - s0).max() > 1e-4  # and the pass did change the vectors


def bit_corpus(n_tok, rows, ln, seed, sample, min_count=1):
    """the Zipf corpus of test_sgns_gpu._setup without a GPU: (idx, cum_table, sample_int or None) as
    int32 / uint32 / uint32 numpy arrays, what SgnsModel derives from the same walks"""
    from node2vec_amd import sgns

    gen = torch.Generator().manual_seed(seed)
    p = 1.0 / torch.arange(1, n_tok + 1, dtype=torch.float64)
    walks = torch.multinomial(p, rows * ln, replacement=True, generator=gen).reshape(rows, ln).to(torch.int32)
    vocab = sgns.build_vocab(walks, min_count)
    idx = vocab.index_of[walks.long()].numpy()
    cum = sgns.make_cum_table(vocab.counts).numpy().view(np.uint32)
    si = sgns.make_sample_int(vocab.counts, sample)
    return idx, cum, None if si is None else si.numpy().view(np.uint32)


@pytest.mark.parametrize("sample", [0.0, 1e-2])
@pytest.mark.parametrize("window,negative", [(5, 5), (1, 1), (32, 21), (5, 32)])
def test_replay_of_touched_rows_matches_the_restatements_counters(cbow_cpu, window, negative, sample):
    """tests/cbow_groups.py on the corpus of the bit tests (12 rows of 21 tokens, two launches): its
    trained positions, its draws equal to their centre and its windows that hold a word twice are the
    restatement's return value, stats[1] and stats[0]"""
    import cbow_groups

    dim, seed = 48, 53
    idx, cum, si = bit_corpus(60, 12, 21, seed, sample)
    n_vocab = len(cum)
    rng = np.random.default_rng(3)
    s0 = ((rng.random((n_vocab, dim)) - 0.5) / dim).astype(np.float32)
    s1 = np.zeros((n_vocab, dim), np.float32)
    stats = np.zeros(2, np.int64)
    bases = (0, 12)
    n = sum(cpu_train(cbow_cpu, idx, s0, s1, cum, si, n_vocab, base, seed, dim, window, negative, 0.025, 1,
                      None, stats) for base in bases)
    got = cbow_groups.replay(idx, cum, si, n_vocab, seed, bases, window, negative, 6, 8)
    assert got["positions"] == n > 100
    assert got["centre_draws"] == stats[1] > 0
    assert got["windows_twice"] == stats[0] > 0
    assert (got["max_kept"] < 21) == (sample > 0) and got["max_count"] <= min(2 * window, 20)
    # the grouping changes what is counted per group, never the positions or the draws
    other = cbow_groups.replay(idx, cum, si, n_vocab, seed, bases, window, negative, 2, 1)
    for key in ("positions", "centre_draws", "windows_twice", "max_count", "max_kept", "max_position"):
        assert other[key] == got[key], key
    assert other["ctx_dup_in_group"] == 0  # groups of one context row
    assert other["ctx_dup_across_groups"] >= got["windows_twice"]  # every such window repeats a row


# a vocabulary of 5 words whose negative draws land on words 2 and 3 only (a draw of exactly 0, one
# in 2^31, aside): bisect_left([0, 0, 2^30, 2^31 - 1, 2^31 - 1], x) is 2 or 3 for every x > 0
CUM5 = np.array([0, 0, 1 << 30, (1 << 31) - 1, (1 << 31) - 1], np.uint32)


def test_one_token_sentence_trains_nothing(cbow_cpu):
    rng = np.random.default_rng(0)
    s0 = rng.normal(size=(5, 8)).astype(np.float32)
    s1 = rng.normal(size=(5, 8)).astype(np.float32)
    k0, k1 = s0.copy(), s1.copy()
    walks = np.array([[-1, 4, -1, 7], [-1, -1, -1, -1]], np.int32)  # 7 is outside the vocabulary
    for mean in (0, 1):
        assert cpu_train(cbow_cpu, walks, s0, s1, CUM5, None, 5, 0, 1, 8, 5, 3, 0.05, mean) == 0
    assert np.array_equal(s0, k0) and np.array_equal(s1, k1)


def test_two_token_sentence_neu1_is_the_other_row(cbow_cpu):
    """[a, b], cbow_mean=1, zero outputs: f = 0 for every target, so syn1neg[a] becomes exactly
    g * syn0[b] with g = (1 - EXP_TABLE[498]) * alpha in fp32 -- neu1 for centre a is syn0[b]"""
    from node2vec_amd import sgns

    rng = np.random.default_rng(1)
    dim = 24
    s0 = rng.normal(size=(5, dim)).astype(np.float32)
    s1 = np.zeros((5, dim), np.float32)
    k0 = s0.copy()
    alpha = np.float32(0.05)
    n = cpu_train(cbow_cpu, np.array([[0, 1]], np.int32), s0, s1, CUM5, None, 5, 3, 9, dim, 1, 2, alpha, 1)
    assert n == 2
    g = (np.float32(1.0) - sgns.exp_table()[498]) * alpha
    assert g.dtype == np.float32
    # centre a is the first target of the first position, and no later target is word a again
    assert np.array_equal(s1[0], g * k0[1]) and np.abs(s1[0]).max() > 1e-3
    assert np.array_equal(s0[2:], k0[2:]) and s1[1].any()  # centre b was trained; words 2 .. 4 are no context
    assert np.abs(s1[2:4]).max() > 0 and not s1[4].any()  # the negatives were trained, on words 2 and 3


def test_word_twice_in_the_window_receives_work_twice(cbow_cpu):
    """[1, 0, 1] against [1, 0, 4] with syn0[1] = syn0[4] = 0: at centre 0 both windows sum to the
    same neu1 and compute the same `work`; word 4 and word 1 of the second sentence end at 0 + work,
    word 1 of the first at (0 + work) + work = 2 work exactly (cbow_mean=0, window 1: count 2)"""
    rng = np.random.default_rng(2)
    dim = 40
    base0 = rng.normal(size=(5, dim)).astype(np.float32) * 0.1
    base0[1] = base0[4] = 0.0
    base1 = rng.normal(size=(5, dim)).astype(np.float32) * 0.1
    out = {}
    for name, sent in (("twice", [1, 0, 1]), ("once", [1, 0, 4])):
        s0, s1 = base0.copy(), base1.copy()
        assert cpu_train(cbow_cpu, np.array([sent], np.int32), s0, s1, CUM5, None, 5, 0, 5, dim, 1, 2, 0.05, 0) == 3
        out[name] = s0
    work = out["once"][1]
    assert np.abs(work).max() > 1e-5 and np.array_equal(out["once"][4], work)
    assert np.array_equal(out["twice"][1], work + work)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_constructor_contract():
    from node2vec_amd import sgns
    from node2vec_amd.constants import HIP_SGNS_PARAMS
    from node2vec_amd.embedding import Node2VecHIP

    assert HIP_SGNS_PARAMS["sg"] == 1 and HIP_SGNS_PARAMS["cbow_mean"] == 1
    params = {"sg": 0}
    n2v = Node2VecHIP(WALKS, params)
    assert isinstance(n2v, Node2VecHIP) and params["sg"] == 0
    Node2VecHIP(WALKS, {"sg": 0, "cbow_mean": 0})
    Node2VecHIP(WALKS, {})  # a missing sg still means skip-gram
    for bad in ({"sg": 0, "batched": True}, {"cbow_mean": 2}, {"sg": 0, "cbow_mean": -1}, {"hs": 1},
                {"sg": 0, "hs": 1}, {"sg": 2}):
        with pytest.raises(ValueError):
            Node2VecHIP(WALKS, dict(bad))
    walks = torch.tensor([[0, 1, 2, 1]], dtype=torch.int32)
    vocab = sgns.build_vocab(walks, 1)
    m = sgns.SgnsModel(vocab, 8, 2, 2, seed=1, sg=0)
    assert (m.sg, m.cbow_mean) == (0, 1) and sgns.SgnsModel(vocab, 8, 2, 2, seed=1).sg == 1
    assert m._hub_rows(10, 4) == 0 and not m.hub_rows_auto  # hub_rows=None means 0 for CBOW
    m.hub_rows = 3
    assert m._hub_rows(10, 4) == 3  # an explicit value is honoured
    for kw in ({"sg": 2}, {"sg": 0, "cbow_mean": 2}):
        with pytest.raises(ValueError):
            sgns.SgnsModel(vocab, 8, 2, 2, seed=1, **kw)


def test_fit_streaming_checks_the_objective_before_touching_the_graph():
    from node2vec_amd.pipeline import fit_streaming

    for bad in ({"sg": 0, "batched": True}, {"cbow_mean": 2}, {"hs": 1}):
        with pytest.raises(ValueError):
            fit_streaming(None, {}, dict(bad), 1)


def test_cbow_abi_refuses_bad_arguments_without_a_gpu(lib):
    from node2vec_amd import _lib

    L = lib
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def P(**kw):
        d = dict(n_vocab=10, sentence_base=0, seed=1, dim=16, window=5, negative=5, alpha=0.025, deterministic=0,
                 cum_index_bits=0, cum_index=None, max_waves=0, batched=0, window_cache=0, hub_rows=0,
                 row_alpha=None)
        d.update(kw)
        return _lib.SgnsParams(**d)

    def train(n_walks=1, walk_len=8, ptrs=True, cbow_mean=1, **kw):
        q = p if ptrs else None
        return L.n2v_cbow_train(q, n_walks, walk_len, q, q, q, None, q, P(**kw), cbow_mean, None, None)

    assert train(n_walks=0) == _lib.OK  # nothing to do: nothing launched
    for kw in (dict(dim=0), dict(dim=1025), dict(window=0), dict(window=33), dict(negative=0), dict(negative=33),
               dict(n_vocab=0), dict(batched=1), dict(window_cache=1), dict(cbow_mean=2), dict(cbow_mean=-1),
               dict(hub_rows=-1), dict(cum_index=p, cum_index_bits=0), dict(cum_index=p, cum_index_bits=31),
               dict(walk_len=0), dict(walk_len=257), dict(n_walks=-1), dict(ptrs=False)):
        assert train(**kw) == _lib.EINVAL, kw
    assert L.n2v_cbow_train(p, 1, 8, p, p, p, None, p, None, 1, None, None) == _lib.EINVAL
    assert L.n2v_cbow_hogwild_waves(P(dim=0), 10, 8) == _lib.EINVAL
    assert L.n2v_cbow_hogwild_waves(P(batched=1), 10, 8) == _lib.EINVAL
    assert L.n2v_cbow_hogwild_waves(None, 10, 8) == _lib.EINVAL
    assert L.n2v_cbow_hogwild_waves(P(), 0, 8) == 0
