"""Nearest-neighbour queries, the parts that need no GPU: the C ABI's symbols and argument checks
(nothing is launched), and the host half of KeyedVectors.most_similar (parsing, the query vector,
the errors raised before any device call)."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

KNN_SYMBOLS = ("n2v_knn_inv_norms", "n2v_knn_workspace_bytes", "n2v_knn_topk", "n2v_knn_scores")


def test_knn_symbols_are_declared_and_exported():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    text = open(f"{ROOT}/include/n2v_hip.h").read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in KNN_SYMBOLS:
        assert name + "(" in text and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 15 and _lib.load().n2v_abi_version() == 15


def _fake():
    buf = (ctypes.c_int64 * 64)()
    return ctypes.addressof(buf) & ~15, buf


def test_knn_entry_points_refuse_bad_arguments_without_a_gpu():
    from node2vec_amd import _lib

    L = _lib.load()
    p_, keep = _fake()
    ws_need = L.n2v_knn_workspace_bytes(1000, 16, 4, 10)
    assert ws_need > 0 and L.n2v_knn_workspace_bytes(1000, 16, 4, 0) > 0

    def topk(**kw):
        a = dict(X=p_, inv=p_, n=1000, dim=16, queries=p_, rows=None, nq=4, k=10, out_r=p_, out_s=p_, ws=p_,
                 ws_bytes=ws_need)
        a.update(kw)
        return L.n2v_knn_topk(a["X"], a["inv"], a["n"], a["dim"], a["queries"], a["rows"], a["nq"], a["k"],
                              a["out_r"], a["out_s"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(dim=0), dict(dim=1025), dict(k=0), dict(k=1025), dict(rows=p_), dict(queries=None),
                dict(X=None), dict(inv=None), dict(out_r=None), dict(out_s=None), dict(ws=None),
                dict(ws_bytes=ws_need - 1), dict(n=-1), dict(n=1 << 31), dict(nq=-1), dict(ws=p_ + 4)):
        assert topk(**bad) == _lib.EINVAL, bad
    assert topk(n=0) == _lib.OK and topk(nq=0) == _lib.OK  # nothing to do: nothing launched
    assert topk(n=0, out_r=None, ws=None) == _lib.OK

    def scores(**kw):
        a = dict(X=p_, inv=p_, n=1000, dim=16, queries=None, rows=p_, nq=4, out=p_, ws=p_,
                 ws_bytes=L.n2v_knn_workspace_bytes(1000, 16, 4, 0))
        a.update(kw)
        return L.n2v_knn_scores(a["X"], a["inv"], a["n"], a["dim"], a["queries"], a["rows"], a["nq"], a["out"],
                                a["ws"], a["ws_bytes"], None)

    for bad in (dict(dim=0), dict(dim=1025), dict(queries=p_), dict(rows=None), dict(X=None), dict(inv=None),
                dict(out=None), dict(ws=None), dict(ws_bytes=1), dict(nq=1 << 20, ws_bytes=1 << 40)):
        assert scores(**bad) == _lib.EINVAL, bad
    assert scores(n=0) == _lib.OK and scores(nq=0) == _lib.OK

    inv = L.n2v_knn_inv_norms
    assert inv(p_, 10, 0, p_, None) == _lib.EINVAL and inv(p_, 10, 1025, p_, None) == _lib.EINVAL
    assert inv(None, 10, 4, p_, None) == _lib.EINVAL and inv(p_, 10, 4, None, None) == _lib.EINVAL
    assert inv(p_, 0, 4, p_, None) == _lib.OK
    ws = L.n2v_knn_workspace_bytes
    assert ws(10, 0, 1, 1) == -1 and ws(10, 1025, 1, 1) == -1 and ws(10, 4, 1, 1025) == -1
    assert ws(10, 4, -1, 1) == -1 and ws(0, 4, 1, 1) == 0 and ws(10, 4, 0, 1) == 0


def _kv(n=40, dim=8, seed=0):
    from node2vec_amd.embedding import KeyedVectors

    rng = np.random.default_rng(seed)
    return KeyedVectors([f"w{i}" for i in range(n)], rng.standard_normal((n, dim)).astype(np.float32))


def _gensim_mean(kv, positive, negative):
    """gensim 3.8 most_similar's query, restated in float64"""
    V = kv.vectors.astype(np.float64)
    vn = V / np.linalg.norm(V, axis=1, keepdims=True)
    items = [(w, 1.0) if isinstance(w, (str, np.ndarray)) else w for w in positive]
    items += [(w, -1.0) if isinstance(w, (str, np.ndarray)) else w for w in negative]
    mean = [wt * (w.astype(np.float64) if isinstance(w, np.ndarray) else vn[kv.vocab[w]]) for w, wt in items]
    mean = np.mean(mean, axis=0)
    return mean / np.linalg.norm(mean)


@pytest.fixture
def no_device(monkeypatch):
    """any call that would reach the GPU fails loudly"""
    from node2vec_amd import _lib, similarity

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    for name in ("knn", "scores", "inv_norms"):
        monkeypatch.setattr(similarity, name, boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)


def test_query_vector_is_gensims_mean(no_device):
    kv = _kv()
    extra = np.linspace(-1, 1, 8).astype(np.float32)
    for pos, neg in ((["w3"], []), (["w1", "w2"], ["w5"]), ([("w1", 0.5), "w7"], [("w9", -2.0)]),
                     ([extra, "w4"], ["w0"])):
        q, own = kv._query(pos, neg)
        assert q.dtype == np.float32 and q.shape == (8,)
        np.testing.assert_allclose(q.astype(np.float64), _gensim_mean(kv, pos, neg), atol=1e-6)
        assert own == sorted({kv.vocab[w if isinstance(w, str) else w[0]] for w in pos + neg
                              if not isinstance(w, np.ndarray)})
    # a bare token is [token]; (token, weight) pairs keep their weight
    assert np.array_equal(kv._query("w3", None)[0], kv._query(["w3"], None)[0])
    np.testing.assert_allclose(kv._query([("w3", 2.0)], None)[0], kv._query(["w3"], None)[0], atol=1e-7)


def test_int_tokens_are_looked_up_as_strings(no_device):
    from node2vec_amd.embedding import KeyedVectors

    kv = KeyedVectors(np.array([10, 11, 12, 13], dtype=np.int64), np.eye(4, dtype=np.float32))
    q, own = kv._query(12, None)
    assert own == [2] and np.array_equal(q, np.eye(4, dtype=np.float32)[2])
    assert kv.similarity(10, "10") == pytest.approx(1.0) and kv.similarity(10, 11) == pytest.approx(0.0)


def test_most_similar_errors_come_before_the_gpu(no_device):
    kv = _kv()
    with pytest.raises(KeyError):
        kv.most_similar("nope")
    with pytest.raises(KeyError):
        kv.most_similar(["w1"], negative=["nope"])
    with pytest.raises(KeyError):
        kv.similar_by_word("nope")
    with pytest.raises(ValueError):
        kv.most_similar()
    with pytest.raises(ValueError):
        kv.most_similar(positive=[], negative=[])
    assert kv.most_similar("w1", topn=0) == [] and kv.most_similar("nope", topn=-3) == []


def test_node2vec_most_similar_needs_a_model():
    import pandas as pd

    from node2vec_amd.embedding import Node2VecHIP

    n2v = Node2VecHIP(pd.DataFrame({"src": [0], "walk": [[0, 1]]}), {"min_count": 1}, random_seed=1)
    with pytest.raises(ValueError, match="Model is not available"):
        n2v.most_similar(0)


def test_saved_model_carries_no_query_cache(tmp_path):
    import torch

    from node2vec_amd.embedding import HipW2V

    kv = _kv()
    kv._inv_norm = torch.ones(40)  # as init_sims leaves it
    HipW2V(kv, np.zeros((40, 8), np.float32), {}, 0).save(str(tmp_path / "m"))
    d = torch.load(str(tmp_path / "m"), weights_only=False)
    assert sorted(d) == ["pairs", "params", "syn1neg", "tokens", "vectors"]
    assert HipW2V.load(str(tmp_path / "m")).wv._inv_norm is None
