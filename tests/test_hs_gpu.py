"""Skip-gram hierarchical softmax on the GPU (csrc/n2v_hs.hip, node2vec_amd/hs.py, Node2VecSpark).

Deterministic mode (one wave, rows in order) must equal the CPU restatement tests/cpu_hs/n2v_hs_cpu.c
BIT FOR BIT -- syn0, syn1 and the pair count -- through the LDS path cache (on and off), the node
groups and every VEC variant.  The statistical tests bound the hogwild mode's quality.
"""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from test_hs_host import hs_cpu  # noqa: F401  (the session fixture that builds the restatement)

pytestmark = pytest.mark.gpu

# TOLERANCES of the hogwild (racy) tests:
#   karate (cfg 1 walks, minCount 10, dim 16, 10 epochs): link AUC > 0.8, as the SGNS test asks
#   planted partition (50 x 40, 3 epochs, dim 64): community AUC of hogwild HS within 0.02 of the
#     deterministic run, both above 0.95
KARATE_AUC_MIN = 0.8
PLANTED_AUC_MIN, PLANTED_AUC_DIFF_MAX = 0.95, 0.02


def _corpus(n_tok, rows, ln, seed):
    gen = torch.Generator().manual_seed(seed)
    p = 1.0 / torch.arange(1, n_tok + 1, dtype=torch.float64)
    return torch.multinomial(p, rows * ln, replacement=True, generator=gen).reshape(rows, ln).to(torch.int32).cuda()


def _model(walks, dim, window, seed, min_count=1):
    from node2vec_amd import hs, sgns

    vocab = sgns.build_vocab(walks, min_count)
    m = hs.HsModel(vocab, dim, window, seed=seed)
    idx = torch.where(walks >= 0, vocab.index_of[walks.clamp(min=0).long()], torch.full_like(walks, -1))
    return m, idx


def _cpu_train(L, m, idx, s0, s1, base, alpha, row_alpha=None):
    from node2vec_amd import sgns

    w = np.ascontiguousarray(idx.cpu().numpy(), np.int32)
    t = m.tree
    pts = np.ascontiguousarray(t.points) if t.points.size else np.zeros(1, np.int32)
    ra = None if row_alpha is None else np.ascontiguousarray(row_alpha, np.float32)
    exp = sgns.exp_table()  # held in a name: the address of a temporary would dangle during the call
    return L.n2v_hs_cpu_train(w.ctypes.data, w.shape[0], w.shape[1], s0.ctypes.data, s1.ctypes.data,
                              t.path_off.ctypes.data, pts.ctypes.data, t.codes.ctypes.data,
                              exp.ctypes.data, len(m.vocab), base, m.seed, m.dim, m.window,
                              float(alpha), None if ra is None else ra.ctypes.data)


def _check_bits(L, m, idx, launches=((0, 0.025, None),), path_cache=True):
    m.path_cache = path_cache
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    n = 0
    for base, alpha, ra in launches:
        m.train_block(idx, alpha, base, deterministic=True,
                      row_alpha=None if ra is None else torch.from_numpy(ra).cuda())
        n += _cpu_train(L, m, idx, s0, s1, base, alpha, ra)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == n
    g0, g1 = m.syn0.cpu().numpy(), m.syn1.cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(g1).all()
    assert np.array_equal(g0, s0), float(np.abs(g0 - s0).max())
    assert np.array_equal(g1, s1), float(np.abs(g1 - s1).max())
    return n


@pytest.mark.parametrize("dim", [1, 16, 63, 64, 100, 128, 256, 1024])
@pytest.mark.parametrize("window", [1, 5, 32])
def test_deterministic_bit_identical_to_restatement(hs_cpu, dim, window):
    walks = _corpus(300, 12, 40, dim * 100 + window)
    m, idx = _model(walks, dim, window, seed=dim + window)
    assert _check_bits(hs_cpu, m, idx) > 0
    assert np.abs(m.syn1.cpu().numpy()).max() > 0


@pytest.mark.parametrize("dim", [64, 128, 1024])
def test_deterministic_without_path_cache(hs_cpu, dim):
    walks = _corpus(200, 10, 30, dim)
    m, idx = _model(walks, dim, 5, seed=3)
    _check_bits(hs_cpu, m, idx, path_cache=False)


def test_oov_tokens_long_rows_and_per_row_rates(hs_cpu):
    """-1 and out-of-range tokens, rows of 700 tokens cut by split_rows, three launches with
    per-row rate arrays (Spark's schedule)"""
    from node2vec_amd import hs, sgns

    walks = _corpus(500, 6, 700, 11)
    walks[0, ::3] = -1
    walks[1, 5:40] = -7
    m, idx = _model(walks, 128, 5, seed=4, min_count=3)
    idx[2, 10:20] = len(m.vocab) + 5  # >= n_vocab: dropped like a -1
    assert int((idx < 0).sum()) > 0
    rows = sgns.split_rows(idx)
    assert rows.shape[1] == sgns.MAX_SENTENCE and rows.shape[0] == 18
    words = (rows >= 0).sum(1).cpu().numpy()
    launches = [(ep * rows.shape[0], 0.025, hs.spark_row_alpha(words * 400, ep, 3, 0.025)) for ep in range(3)]
    _check_bits(hs_cpu, m, rows, launches)


@pytest.mark.parametrize("n_vocab", [1, 2])
def test_vocabulary_of_one_and_two_words(hs_cpu, n_vocab):
    walks = (torch.arange(60, dtype=torch.int32).reshape(3, 20) % n_vocab).cuda()
    m, idx = _model(walks, 32, 5, seed=9)
    assert len(m.vocab) == n_vocab
    s0 = m.syn0.cpu().numpy().copy()
    n = _check_bits(hs_cpu, m, idx)
    assert n > 0
    if n_vocab == 1:  # code length 0: pairs are formed, nothing trains
        assert np.array_equal(m.syn0.cpu().numpy(), s0) and not m.syn1.cpu().numpy().any()


@pytest.mark.parametrize("dim", [16, 128, 256, 1024])
def test_single_wave_hogwild_equals_restatement(hs_cpu, dim):
    """hogwild mode on ONE wave (max_waves = 1): its smaller LDS path cache (16 / 8 / 4 / 1 rows, so
    every pair mixes cached and HBM rows) is bit-identical to the restatement"""
    from node2vec_amd import hs, sgns

    V = 300  # geometric counts: a deep tree (codes of 2 .. 23 bits)
    counts = torch.from_numpy(np.maximum(1, 1.5 ** (40 - np.arange(V))).astype(np.int64)).cuda()
    vocab = sgns.Vocab(torch.arange(V).cuda(), counts, torch.arange(V, dtype=torch.int32).cuda())
    m = hs.HsModel(vocab, dim, 5, seed=5)
    gen = torch.Generator().manual_seed(dim)
    idx = torch.randint(0, V, (8, 60), generator=gen, dtype=torch.int32).cuda()
    assert m.tree.lengths.max() > 16
    m.max_waves = 1
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    m.hot_nodes = 0
    m.train_block(idx, 0.025, 0)
    n = _cpu_train(hs_cpu, m, idx, s0, s1, 0, 0.025)
    torch.cuda.synchronize()
    assert m.hogwild_waves_used == 1 and int(m.pairs.item()) == n > 0
    assert np.array_equal(m.syn0.cpu().numpy(), s0) and np.array_equal(m.syn1.cpu().numpy(), s1)
    assert np.abs(s1).max() > 1e-3
    m.hot_nodes = 1  # atomic adds on the top nodes: refused (measured slower and worse)
    with pytest.raises(ValueError):
        m.train_block(idx, 0.02, idx.shape[0])


def test_hogwild_pair_count_and_finite(hs_cpu):
    walks = _corpus(3000, 2000, 41, 5)
    m, idx = _model(walks, 128, 5, seed=1)
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1.cpu().numpy().copy()
    m.train_block(idx, 0.025, 0)
    torch.cuda.synchronize()
    assert m.hogwild_waves_used > 1
    assert int(m.pairs.item()) == _cpu_train(hs_cpu, m, idx, s0, s1, 0, 0.025)
    assert np.isfinite(m.syn0.cpu().numpy()).all() and np.isfinite(m.syn1.cpu().numpy()).all()


def test_offsets_past_2_31_elements(hs_cpu):
    """a model of more than 2^31 syn0 (and syn1) elements: a few rows of the rarest words, at the
    end of syn0, trained deterministically; compared with the restatement on the rows they touch"""
    from node2vec_amd import hs, sgns

    dim = 1024
    V = (1 << 21) + 64
    counts = torch.arange(V, 0, -1, dtype=torch.int64) + 10
    vocab = sgns.Vocab(torch.arange(V).cuda(), counts.cuda(), torch.arange(V, dtype=torch.int32).cuda())
    m = hs.HsModel(vocab, dim, 5, seed=2)
    assert m.syn0.numel() > 2 ** 31 and m.syn1.numel() > 2 ** 31
    gen = torch.Generator().manual_seed(0)
    idx = (V - 1 - torch.randint(0, 40, (4, 30), generator=gen)).to(torch.int32).cuda()
    words = sorted(set(idx.cpu().numpy().reshape(-1).tolist()))
    t = m.tree
    nodes = sorted({int(p) for w in words for p in t.path(w)})
    assert max(nodes) * dim >= 2 ** 31 and words[0] * dim >= 2 ** 31
    s0 = m.syn0[words].cpu().numpy().copy()
    s1 = m.syn1[nodes].cpu().numpy().copy()
    m.train_block(idx, 0.025, 0, deterministic=True)
    torch.cuda.synchronize()
    # the same training on the compacted model: word k is row k, node nodes[k] is syn1 row k
    wmap = {w: k for k, w in enumerate(words)}
    nmap = {p: k for k, p in enumerate(nodes)}
    off = np.zeros(len(words) + 1, np.int64)
    pts, codes = [], np.zeros(len(words), np.uint64)
    for k, w in enumerate(words):
        path = [nmap[int(p)] for p in t.path(w)]
        pts += path
        off[k + 1] = off[k] + len(path)
        codes[k] = t.codes[w]
    pts = np.asarray(pts, np.int32)
    cidx = np.vectorize(wmap.get)(idx.cpu().numpy()).astype(np.int32)
    exp = sgns.exp_table()
    n = hs_cpu.n2v_hs_cpu_train(cidx.ctypes.data, cidx.shape[0], cidx.shape[1], s0.ctypes.data, s1.ctypes.data,
                                off.ctypes.data, pts.ctypes.data, codes.ctypes.data, exp.ctypes.data,
                                len(words), 0, m.seed, dim, 5, 0.025, None)
    assert n == int(m.pairs.item()) > 0
    assert np.array_equal(m.syn0[words].cpu().numpy(), s0)
    assert np.array_equal(m.syn1[nodes].cpu().numpy(), s1)


def _karate_graph():
    from node2vec_amd.graph import DeviceGraph

    edges = np.array(load_golden("karate_edges.json"), dtype=np.float64).reshape(-1, 3)
    g = DeviceGraph.from_edges(edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), None,
                               n_vertices=34, device="cuda")
    adj = np.zeros((34, 34), bool)
    adj[edges[:, 0].astype(int), edges[:, 1].astype(int)] = True
    return g, adj


def _unit(v):
    v = v - v.mean(0)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.statistical
def test_karate_hogwild_link_auc():
    from node2vec_amd import hs
    from node2vec_amd import randomwalk as rw
    from node2vec_amd import sgns

    g, adj = _karate_graph()
    aucs = []
    for seed in range(3):
        walks, _ = rw.walk(g, rw.start_vertices(g), 10, 10, 1.0, 1.0, 100 + seed)  # cfg 1
        vocab = sgns.build_vocab(walks, 10)
        idx = vocab.index_of[walks.long()]
        m = hs.HsModel(vocab, 16, 5, seed=seed)
        m.train(hs.sentences(idx, 10000), 10, 0.025)
        torch.cuda.synchronize()
        v = _unit(m.syn0.cpu().numpy()[np.argsort(vocab.ids.cpu().numpy())])
        s = v @ v.T
        iu = np.triu_indices(34, 1)
        pos, neg = s[iu][adj[iu]], s[iu][~adj[iu]]
        aucs.append(float((pos[:, None] > neg[None, :]).mean()))
    print("karate HS link AUC:", aucs)
    assert min(aucs) > KARATE_AUC_MIN, aucs


def _planted(nc=50, sz=40, seed=0):
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


@pytest.mark.statistical
def test_planted_partition_hogwild_matches_deterministic():
    from node2vec_amd import hs
    from node2vec_amd import randomwalk as rw
    from node2vec_amd import sgns

    g, comm = _planted()
    walks, _ = rw.walk(g, rw.start_vertices(g), 10, 40, 1.0, 1.0, 1)
    vocab = sgns.build_vocab(walks, 1)
    rows = hs.sentences(vocab.index_of[walks.long()], 10000)
    ids = vocab.ids.cpu().numpy()
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, len(ids), 200000), rng.integers(0, len(ids), 200000)
    same = comm[ids[a]] == comm[ids[b]]

    def auc(det):
        m = hs.HsModel(vocab, 64, 5, seed=7)
        m.train(rows, 3, 0.025, deterministic=det)
        torch.cuda.synchronize()
        v = _unit(m.syn0.cpu().numpy())
        s = (v[a] * v[b]).sum(1)
        return float((s[same][:, None] > s[~same][None, :3000]).mean()), m.hogwild_waves_used

    (det, _), (hog, waves) = auc(True), auc(False)
    print("planted partition HS community AUC: deterministic", det, "hogwild", hog, "waves", waves)
    assert waves > 1
    assert min(det, hog) > PLANTED_AUC_MIN and abs(det - hog) < PLANTED_AUC_DIFF_MAX, (det, hog)


def test_node2vecspark_end_to_end_on_karate(tmp_path):
    from node2vec_amd.embedding import HsW2VModel, KeyedVectors, Node2VecSpark
    from node2vec_amd.fugue import random_walk

    e = load_golden("karate_edges.json")
    df_walks = random_walk("hip", pd.DataFrame(e, columns=["src", "dst", "weight"]),
                           {"num_walks": 10, "walk_length": 10}, random_seed=42)
    params = {"minCount": 0, "maxIter": 5, "seed": 1000}
    n2v = Node2VecSpark(df_walks, params, window_size=5, vector_size=32, random_seed=1000)
    model = n2v.fit()
    assert isinstance(model, HsW2VModel) and isinstance(model.wv, KeyedVectors) and model.pairs_trained > 0
    assert model.stats["mean_code_length"] > 3 and model.stats["hogwild_waves"] >= 1
    emb = n2v.embedding()
    assert list(emb.columns) == ["id", "vector"] and len(emb) == 34 and all(len(v) == 32 for v in emb["vector"])
    assert emb["id"].dtype == np.int64
    v1, v1s = n2v.get_vector(1), n2v.get_vector("1")
    assert list(v1.columns) == ["word", "vector"] and len(v1) == 1 and v1["vector"][0] == v1s["vector"][0]
    assert len(n2v.get_vector(99)) == 0 and len(n2v.get_vector("x")) == 0
    hits = model.wv.most_similar("0", topn=5)
    assert len(hits) == 5 and all(t != "0" for t, _ in hits)
    n2v.save_model(str(tmp_path), "tmp")
    assert os.path.isdir(tmp_path / "tmp.sparkml")
    loaded = n2v.load_model(str(tmp_path), "tmp.sparkml")
    assert isinstance(loaded, HsW2VModel) and np.array_equal(loaded.wv.vectors, model.wv.vectors)
    # an inner join with name_id: ids it does not list are dropped, not a KeyError
    name_id = pd.DataFrame({"name": [f"v{i}" for i in range(30)], "id": list(range(30))})
    n2v = Node2VecSpark(df_walks, dict(params), name_id=name_id, random_seed=3)
    with pytest.raises(ValueError):
        n2v.embedding()
    n2v.fit()
    res = n2v.embedding()
    assert list(res.columns) == ["name", "vector"] and len(res) == 30
    # the reference's own case: maxSentenceLength 1 trains nothing and still fits
    walks = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})
    n2v = Node2VecSpark(walks, {"minCount": 0, "maxIter": 1, "seed": 1000, "maxSentenceLength": 1,
                                "windowSize": 4})
    m = n2v.fit()
    assert m.pairs_trained == 0 and len(n2v.embedding()) == 5
