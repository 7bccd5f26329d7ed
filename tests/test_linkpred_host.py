"""Link prediction (node2vec_amd/linkpred.py, csrc/n2v_pairs.hip), the parts that need no GPU: the CPU
restatement of the score's fixed order (tests/cpu_pairs/n2v_pairs_cpu.c) against exact arithmetic, its
symmetry, the four operators against numpy float32, auc() against the O(P N) count, the C ABI's argument
checks, the header and the binding, and the argument paths of KeyedVectors / Node2Vec* that touch no GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import pairs_cases as pc
from conftest import ROOT

DIMS = (1, 3, 64, 100, 129, 1024)


@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def pairs_cpu(tmp_path_factory):
    return pc.build(tmp_path_factory.mktemp("pairs_cpu"))


def _rows(dim, kind, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(dim).astype(np.float32)
    if kind == "random":
        return a, rng.standard_normal(dim).astype(np.float32)
    k = int(rng.integers(dim))
    if kind == "halves":  # the products of the two halves cancel: the exact sum is tiny against sum |a_i b_i|
        h = dim // 2
        a[h:2 * h] = a[:h]
        b = rng.standard_normal(dim).astype(np.float32)
        b[h:2 * h] = -b[:h]
        if dim % 2:
            b[-1] = np.float32(2.0 ** -12)
        b[k] = np.float32(b[k] * np.float32(1.0 + 2.0 ** -10))
        return a, b
    b = -a
    b[k] = np.float32(b[k] * np.float32(1.0 + 2.0 ** -10) + np.float32(2.0 ** -12))
    return a, b


@pytest.mark.parametrize("kind", ["random", "cancel", "halves"])
@pytest.mark.parametrize("dim", DIMS)
def test_restatement_is_a_dot_product(pairs_cpu, dim, kind):
    """|got - exact| <= gamma_dim * sum |a_i b_i|, gamma_n = n u / (1 - n u), u = 2^-24: the bound of ANY order of
    summation of n products (Higham, Accuracy and Stability, section 3.1; an fmaf chain rounds no more often)"""
    u = 2.0 ** -24
    gamma = dim * u / (1.0 - dim * u)
    for seed in range(20):
        a, b = _rows(dim, kind, 1000 * dim + seed)
        prod = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 x 24 bits
        exact = sum(Fraction(float(p)) for p in prod)
        bound = Fraction(gamma) * sum(Fraction(float(abs(p))) for p in prod)
        got = float(pc.dot(pairs_cpu, a, b))
        assert abs(Fraction(got) - exact) <= bound, (dim, kind, seed, got, float(exact))
        if kind == "halves" and dim >= 64:  # the case is one: the sum is far below the terms
            assert abs(exact) <= Fraction(1, 256) * sum(Fraction(float(abs(p))) for p in prod)


@pytest.mark.parametrize("dim", DIMS)
def test_restatement_is_symmetric(pairs_cpu, dim):
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((40, dim)).astype(np.float32)
    inv = (1.0 / np.sqrt((X.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    a, b = rng.integers(0, 40, 500), rng.integers(0, 40, 500)
    for metric in ("dot", "cosine"):
        ab, ba = pc.scores(pairs_cpu, X, inv, a, b, metric), pc.scores(pairs_cpu, X, inv, b, a, metric)
        assert np.array_equal(ab.view(np.uint32), ba.view(np.uint32))
    assert np.isnan(pc.scores(pairs_cpu, X, inv, [0, 40, -1], [40, 0, 0], "dot")).all()  # outside [0, n): NaN


def _special_rows(dim):
    """rows holding -0.0, denormals, inf and NaN beside ordinary values"""
    rng = np.random.default_rng(dim + 7)
    X = rng.standard_normal((12, dim)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 1.0, -1.0],
                       np.float32)
    X[:6] = special[rng.integers(0, special.size, (6, dim))]
    X[6] = -X[7]  # a sum of exactly (+-)0 in every element
    return X


@pytest.mark.parametrize("op", list(pc.OPS))
@pytest.mark.parametrize("dim", DIMS)
def test_restated_operators_equal_numpy_float32(pairs_cpu, dim, op):
    X = _special_rows(dim)
    a, b = np.repeat(np.arange(12), 12), np.tile(np.arange(12), 12)
    assert pc.same_bits(pc.features(pairs_cpu, X, a, b, op), pc.numpy_features(X, a, b, op))
    assert np.isnan(pc.features(pairs_cpu, X, [12, 0], [0, -1], op)).all()


def _check_auc(pos, neg):
    from node2vec_amd import linkpred

    want = pc.auc_quadratic(pos, neg)
    assert linkpred.auc(torch.from_numpy(pos), torch.from_numpy(neg)) == want
    assert linkpred.auc(pos, neg.astype(np.float64)) == want  # numpy in, mixed float types
    return want


@pytest.mark.parametrize("P", [1, 2, 63, 1000])
@pytest.mark.parametrize("N", [1, 2, 63, 1000])
def test_auc_equals_the_quadratic_count(P, N):
    rng = np.random.default_rng(P * 1009 + N)
    values = np.array([-1.5, 0.0, 0.25, 0.25 + 2.0 ** -20, 7.0], np.float32)
    _check_auc(values[rng.integers(0, 5, P)], values[rng.integers(0, 5, N)])  # heavy ties
    _check_auc(rng.standard_normal(P).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    assert _check_auc(np.full(P, 0.5, np.float32), np.full(N, 0.5, np.float32)) == 0.5
    lo, hi = rng.random(N).astype(np.float32), (rng.random(P) + 2).astype(np.float32)
    assert _check_auc(hi, lo) == 1.0
    assert _check_auc(lo[:P] if P <= N else np.resize(lo, P), (rng.random(N) + 2).astype(np.float32)) == 0.0
    assert _check_auc(np.array([0.0] * P, np.float32), np.array([-0.0] * N, np.float32)) == 0.5  # -0 ties with +0
    assert _check_auc(np.full(P, np.inf, np.float32), np.full(N, -np.inf, np.float32)) == 1.0


def test_auc_refuses_nan_and_empty_input():
    from node2vec_amd import linkpred

    one, none = np.array([1.0], np.float32), np.array([], np.float32)
    for pos, neg in ((none, one), (one, none), (none, none), (np.array([np.nan, 1.0], np.float32), one),
                     (one, np.array([0.0, np.nan], np.float32))):
        with pytest.raises(ValueError):
            linkpred.auc(pos, neg)


def test_pairs_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; an empty list is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def scores(X=p, inv=p, n=10, dim=16, a=p, b=p, n_pairs=1, metric=_lib.PAIR_COSINE, out=p):
        return lib.n2v_pair_scores(X, inv, n, dim, a, b, n_pairs, metric, out, None)

    def feats(X=p, n=10, dim=16, a=p, b=p, n_pairs=1, op=_lib.PAIR_HADAMARD, out=p):
        return lib.n2v_pair_features(X, n, dim, a, b, n_pairs, op, out, None)

    def edges(rowptr=p, col=p, nv=10, a=p, b=p, n_pairs=1, out=p):
        return lib.n2v_pairs_in_graph(rowptr, col, nv, a, b, n_pairs, out, None)

    for call in (scores, feats):
        assert call(n_pairs=0) == _lib.OK
        assert call(n_pairs=0, dim=1) == _lib.OK and call(n_pairs=0, dim=1024) == _lib.OK
        for kw in (dict(dim=0), dict(dim=1025), dict(n_pairs=-1), dict(n=-1), dict(n=1 << 31), dict(X=None),
                   dict(a=None), dict(b=None), dict(out=None), dict(n_pairs=1 << 40)):
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
        assert call(n_pairs=0, dim=0) == _lib.EINVAL  # (refused before the empty list returns)
    for metric in (-1, 2):
        assert scores(metric=metric) == _lib.EINVAL and scores(metric=metric, n_pairs=0) == _lib.EINVAL
    for op in (-1, 4):
        assert feats(op=op) == _lib.EINVAL and feats(op=op, n_pairs=0) == _lib.EINVAL
    assert scores(inv=None) == _lib.EINVAL  # cosine needs the norms
    assert scores(inv=None, metric=_lib.PAIR_DOT, n_pairs=0) == _lib.OK  # dot ignores them
    assert edges(n_pairs=0) == _lib.OK
    for kw in (dict(n_pairs=-1), dict(nv=-1), dict(nv=1 << 31), dict(rowptr=None), dict(a=None), dict(b=None),
               dict(out=None), dict(n_pairs=1 << 40)):
        assert edges(**kw) == _lib.EINVAL, kw


def test_header_and_binding_name_the_new_entry_points(lib):
    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("n2v_pair_scores", "n2v_pair_features", "n2v_pairs_in_graph"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code) and hasattr(lib, name)
    for name, value in (("DOT", 0), ("COSINE", 1), ("AVERAGE", 0), ("HADAMARD", 1), ("L1", 2), ("L2", 3)):
        assert re.search(r"#define\s+N2V_PAIR_%s\s+%d\b" % (name, value), code)
        assert getattr(_lib, "PAIR_" + name) == value
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15
    assert re.search(r"#define\s+N2V_ABI_VERSION\s+15\b", code)


def test_keyedvectors_pair_queries_check_their_arguments_before_the_gpu():
    from node2vec_amd.embedding import KeyedVectors

    wv = KeyedVectors(np.array([5, 7, 9]), np.ones((3, 4), np.float32))
    for call in (wv.pair_scores, wv.edge_features):
        with pytest.raises(KeyError):
            call([5, 6], [7, 9])
        with pytest.raises(KeyError):
            call(["5"], ["07"])
        with pytest.raises(ValueError):
            call([5], [7, 9])
    with pytest.raises(ValueError):
        wv.pair_scores([5], [7], metric="euclid")
    with pytest.raises(ValueError):
        wv.edge_features([5], [7], op="concat")
    named = KeyedVectors(["a", "b"], np.ones((2, 4), np.float32))
    with pytest.raises(KeyError):
        named.pair_scores(["a"], ["c"])


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_plugin_classes_refuse_pair_queries_before_fit_and_unknown_ids():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    edges = pd.DataFrame({"src": [0, 1], "dst": [1, 2]})
    wv = KeyedVectors(np.array([0, 1, 2, 3, 4]), np.ones((5, 4), np.float32))
    for n2v, model in ((Node2VecHIP(WALKS, {}), HipW2V(wv, np.zeros((5, 4), np.float32), {}, 0)),
                       (Node2VecSpark(WALKS, {}), HsW2VModel(wv, np.zeros((4, 4), np.float32), {}, 0, {}))):
        for call in (n2v.link_scores, n2v.edge_embedding):
            with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
                call(edges)
        n2v.model = model
        for call in (n2v.link_scores, n2v.edge_embedding):
            with pytest.raises(KeyError):
                call(pd.DataFrame({"src": [0, 9], "dst": [1, 2]}))
            with pytest.raises(ValueError):
                call(pd.DataFrame({"a": [0], "b": [1]}))


def test_linkpred_refuses_host_tensors_and_bad_names():
    """no CPU path for the kernels: a host matrix is refused, as in similarity"""
    from node2vec_amd import linkpred

    X = torch.zeros((4, 8))
    with pytest.raises(ValueError):
        linkpred.pair_scores(X, [0], [1])
    with pytest.raises(ValueError):
        linkpred.pair_features(X, [0], [1])
    with pytest.raises(ValueError):
        linkpred.pair_scores(X, [0], [1], metric="l2")
    with pytest.raises(ValueError):
        linkpred.pair_features(X, [0], [1], op="dot")
