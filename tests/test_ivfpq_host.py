"""Product-quantised codes for the inverted-file index (node2vec_amd/ann.py build_pq / search_pq,
csrc/n2v_ivfpq.hip), the parts that need no GPU: the numpy restatement the GPU tests compare against
(tests/ivfpq_cases.py) checked against float64, the argument checks, size queries and LDS budget of the entry points
(nothing is launched: the library loads without a device), and the routing of KeyedVectors.build_index(pq=)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ivf_cases as ic
import ivfpq_cases as pc
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)


# ---- the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,m", [(3, 2), (17, 4), (64, 8), (129, 16), (64, 64)])
def test_restatement_is_within_the_rounding_bound_of_float64(oracle, dim, m):
    """A table entry is a sum of at most dsub products, each rounded once, added one at a time: its error is at
    most gamma_dsub * sum |q_t w_t| <= dsub * 2^-23 * sum |q_t w_t| (gamma_n = n u / (1 - n u), u = 2^-24).  A
    score adds m entries to the coarse score: m more roundings, each at most 2^-24 of a partial sum that is at
    most A = |coarse| + sum |entry|, on top of the entries' own errors."""
    rng = np.random.default_rng(dim * 100 + m)
    cb, Q, coarse = pc.gaussian_problem(rng, dim, m, 20, 1)
    qh = pc.qhat(oracle, Q)
    lut = pc.lut_expect(qh, cb, dim)
    want, mass = pc.lut_float64(qh, cb, dim)
    dsub = pc.dsub_of(dim, m)
    entry_bound = dsub * 2.0 ** -23 * mass
    assert (np.abs(lut - want) <= entry_bound).all()
    assert lut.dtype == np.float32 and lut.shape == (20, m, 256)
    codes = pc.hand_codes(rng, 500, m)
    pos = np.arange(500)
    s = pc.scores_expect(lut, codes, pos, coarse[:, 0])
    j = np.arange(m)
    s64 = coarse[:, :1].astype(np.float64) + want[:, j, codes[:, :m]].sum(axis=2)
    A = np.abs(coarse[:, :1]).astype(np.float64) + np.abs(want[:, j, codes[:, :m]]).sum(axis=2)
    bound = entry_bound[:, j, codes[:, :m]].sum(axis=2) + m * 2.0 ** -23 * A
    assert (np.abs(s - s64) <= bound).all()


def test_restatement_on_exact_values_and_its_selection(oracle):
    """multiples of 1/8 against +-1 / sqrt(s): every sum is exact, so fp32 equals float64; the selection keeps
    (score descending, original row ascending), drops NaN and pads with (-1, -inf)"""
    rng = np.random.default_rng(3)
    dim, m, nq = 64, 8, 12
    cb, Q, coarse = pc.exact_problem(rng, dim, m, nq, 2)
    qh = pc.qhat(oracle, Q)
    assert np.array_equal(qh, Q)  # the sum of squares is exactly 1
    lut = pc.lut_expect(qh, cb, dim)
    assert np.array_equal(lut.astype(np.float64), pc.lut_float64(qh, cb, dim)[0])
    list_off, row_ids = pc.hand_lists(rng, 40)
    codes = pc.hand_codes(rng, len(row_ids), m)
    probes = np.tile(np.array([ic.LONG_LIST, 7]), (nq, 1))
    probes[1] = -1
    coarse[2, 0] = np.nan
    r, s = pc.scan_expect(lut, codes, list_off, row_ids, probes, coarse, 120)
    assert (r[1] == -1).all() and (s[1] == -np.inf).all()
    assert (r[0] >= 0).sum() == 40 + 65 and (r[2] >= 0).sum() == 65  # the NaN probe contributes nothing
    for q in (0, 2, 5):
        live = r[q] >= 0
        keys = list(zip(-s[q][live], r[q][live]))
        assert keys == sorted(keys) and len(set(r[q][live])) == live.sum()
    assert (np.diff(s[0][r[0] >= 0]) == 0).any()  # heavily tied, as meant


# ---- the C ABI --------------------------------------------------------------------------------------------------

def _calls():
    from node2vec_amd import _lib

    L = _lib.load()
    buf = (ctypes.c_int64 * 1024)()
    p_ = (ctypes.addressof(buf) + 255) & ~255  # aligned, inside the buffer: never dereferenced

    def topk(**kw):
        a = dict(codes=p_, cb=p_, m=4, X=p_, inv=p_, n=100, dim=8, off=p_, ids=p_, nlist=4, mlr=50, q=p_, qr=0, nq=3,
                 probes=p_, coarse=p_, nprobe=2, k=5, out_r=p_, out_s=p_, status=p_, ws=p_, ws_bytes=1 << 40)
        a.update(kw)
        return L.n2v_ivfpq_topk(a["codes"], a["cb"], a["m"], a["X"], a["inv"], a["n"], a["dim"], a["off"], a["ids"],
                                a["nlist"], a["mlr"], a["q"], a["qr"], a["nq"], a["probes"], a["coarse"], a["nprobe"],
                                a["k"], a["out_r"], a["out_s"], a["status"], a["ws"], a["ws_bytes"], None)

    def lut(**kw):
        a = dict(X=p_, inv=p_, n=100, dim=8, q=p_, qr=0, nq=3, cb=p_, m=4, out=p_, ws=p_, ws_bytes=1 << 40)
        a.update(kw)
        return L.n2v_ivfpq_lut(a["X"], a["inv"], a["n"], a["dim"], a["q"], a["qr"], a["nq"], a["cb"], a["m"],
                               a["out"], a["ws"], a["ws_bytes"], None)

    def sizes(**kw):
        a = dict(n=100, dim=8, m=4, nlist=4, mlr=50, nq=3, nprobe=2, k=5)
        a.update(kw)
        return a["n"], a["dim"], a["m"], a["nlist"], a["mlr"], a["nq"], a["nprobe"], a["k"]

    return L, p_, topk, lut, sizes


BAD_SIZES = [dict(m=0), dict(m=9), dict(m=65, dim=128), dict(m=-1), dict(nlist=0), dict(nlist=1025, nprobe=1),
             dict(nprobe=0), dict(nprobe=5), dict(k=129), dict(k=-1), dict(dim=0), dict(dim=1025), dict(mlr=0),
             dict(mlr=101), dict(nq=-1), dict(nq=1 << 20), dict(n=-1), dict(n=1 << 31)]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    L, p_, topk, lut, sizes = _calls()
    plan5 = (ctypes.c_int64 * 5)()
    for bad in BAD_SIZES:
        assert topk(**bad) == -1, bad
        assert L.n2v_ivfpq_workspace_bytes(*sizes(**bad)) == -1, bad
        assert L.n2v_ivfpq_plan(*sizes(**bad), plan5) == -1, bad
    assert topk(k=0) == -1 and L.n2v_ivfpq_plan(*sizes(k=0), plan5) == -1  # k = 0 is n2v_ivfpq_lut's size query only
    assert L.n2v_ivfpq_plan(*sizes(), None) == -1
    for name in ("codes", "cb", "off", "ids", "probes", "coarse", "out_r", "out_s", "status", "ws"):
        assert topk(**{name: 0}) == -1, name
    assert topk(codes=p_ + 4) == -1  # the code rows are read 16 bytes at a time
    assert topk(q=p_, qr=p_) == -1 and topk(q=0, qr=0) == -1  # exactly one of queries / query_rows
    assert topk(q=0, qr=p_, X=0) == -1 and topk(q=0, qr=p_, inv=0) == -1  # a query row is a row of X
    need = L.n2v_ivfpq_workspace_bytes(*sizes())
    assert need > 0
    assert topk(ws_bytes=need - 1) == -1 and topk(ws=p_ + 4) == -1 and topk(ws=p_ + 8) == -1
    # nothing to do: N2V_OK and no launch (there is no device here to launch on); queries need no X
    assert topk(nq=0) == 0 and topk(nq=0, q=0, qr=p_) == 0 and topk(nq=0, X=0, inv=0) == 0
    assert topk(n=0, mlr=1) == 0
    assert L.n2v_ivfpq_workspace_bytes(*sizes(nq=0)) == 0 and L.n2v_ivfpq_workspace_bytes(*sizes(n=0, mlr=1)) == 0
    # n2v_ivfpq_lut
    for bad in (dict(m=0), dict(m=9), dict(m=65, dim=128), dict(dim=0), dict(dim=1025), dict(nq=-1), dict(nq=1 << 20),
                dict(n=-1)):
        assert lut(**bad) == -1, bad
    for name in ("cb", "out", "ws"):
        assert lut(**{name: 0}) == -1, name
    assert lut(q=p_, qr=p_) == -1 and lut(q=0, qr=0) == -1 and lut(q=0, qr=p_, X=0) == -1
    need = L.n2v_ivfpq_workspace_bytes(*sizes(k=0))
    assert need > 0 and lut(ws_bytes=need - 1) == -1 and lut(ws=p_ + 8) == -1
    assert lut(nq=0) == 0 and lut(nq=0, X=0, inv=0) == 0
    assert L.n2v_ivfpq_workspace_bytes(*sizes(k=0, nlist=0, mlr=0, nprobe=0)) == need  # not looked at for k = 0
    assert L.n2v_ivfpq_workspace_bytes(*sizes(k=0, m=9)) == -1


def test_plan_and_its_lds_budget():
    from node2vec_amd import ann

    L, _, _, _, sizes = _calls()
    for m in range(1, 65):
        want_t = 16 if m <= 7 else 8 if m <= 16 else 4 if m <= 32 else 2
        for k in (1, 10, 127, 128):
            t, chunk, chunks, lds, stride = ann.plan_pq(100000, 128, m, 32, 9000, 200, 8, k)
            assert t == want_t and stride == pc.code_stride(m) == ann.code_stride(m) and stride >= m
            # the tile's tables (m KiB each) and the candidate buffers (256 scores and rows a pair) fit beside
            # each other in the 160 KiB of a CU
            assert t * m * 1024 + t * 256 * 8 <= lds <= 160 * 1024, (m, k, lds)
            assert chunk % 128 == 0 and chunks == -(-9000 // chunk) and (chunk, chunks) == (3072, 3)
    # the cut of a list depends on max_list_rows alone
    assert ann.plan_pq(pc.HAND_N, 64, 8, ic.NLIST, pc.HAND_MAX_LIST_ROWS, 200, 1, 10)[:3] == (8, pc.HAND_CHUNK, 3)
    assert ann.plan_pq(pc.HAND_N, 64, 64, ic.NLIST, pc.HAND_MAX_LIST_ROWS, 100, 4, 128)[:3] == (2, pc.HAND_CHUNK, 3)
    assert ann.plan_pq(6000, 64, 8, 9, 1, 100, 1, 10)[1:3] == (128, 1)
    assert ann.plan_pq(6000, 64, 8, 9, 4096, 5, 1, 1)[1:3] == (4096, 1)
    assert ann.plan_pq(6000, 64, 8, 9, 4097, 5, 1, 1)[1:3] == (2176, 2)
    with pytest.raises(ValueError):
        ann.plan_pq(6000, 64, 8, 9, 4096, 100, 1, 129)
    with pytest.raises(ValueError):
        ann.plan_pq(6000, 64, 65, 9, 4096, 100, 1, 10)
    grid = dict(nq=(1, 2, 15, 16, 17, 63, 64, 65, 200, 1000, 4096), nprobe=(1, 2, 3, 7, 8, 16, 32),
                k=(1, 2, 10, 64, 127, 128), m=(1, 2, 7, 8, 16, 17, 64))
    base = dict(n=100000, dim=64, nlist=32, mlr=9000)
    for name, values in grid.items():
        for other in ({}, dict(nq=200, nprobe=8, k=10), dict(nq=4096, nprobe=32, k=128)):
            got = [L.n2v_ivfpq_workspace_bytes(*sizes(**{**base, **other, name: v})) for v in values]
            assert all(b > 0 for b in got) and got == sorted(got), (name, other, got)
    # more scan blocks than one launch takes: refused, so that callers split the queries
    assert L.n2v_ivfpq_workspace_bytes(1 << 24, 64, 64, 1024, 1 << 24, (1 << 20) - 1, 1024, 1) == -1


def test_symbols_are_bound_and_declared():
    from node2vec_amd import _lib

    header = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("n2v_ivfpq_workspace_bytes", "n2v_ivfpq_plan", "n2v_ivfpq_lut", "n2v_ivfpq_topk"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15
    assert "#define N2V_ABI_VERSION 15" in header


# ---- ann.build_pq / ann.search_pq: the checks that come before the GPU -------------------------------------------

def _host_index(n=50, dim=8, nlist=4, m=4):
    from node2vec_amd import ann

    labels = torch.arange(n) % nlist
    off, rows = ann.layout(labels, nlist)
    base = ann.IVFIndex(torch.eye(nlist, dim), torch.ones(nlist), off, rows, int((off[1:] - off[:-1]).max()), n, dim, 2)
    dsub = -(-dim // m)
    return ann.IVFPQIndex(base, torch.zeros(m, 256, dsub), torch.zeros(len(rows), ann.code_stride(m),
                                                                      dtype=torch.uint8), m, dsub)


def test_build_pq_checks_its_arguments_before_the_gpu(monkeypatch):
    from node2vec_amd import _dense, ann

    monkeypatch.setattr(_dense, "matrix", lambda X: X)  # a host tensor stands for the device matrix
    X = torch.zeros(50, 8)
    idx = _host_index()
    for m in (0, 9, -1):
        with pytest.raises(ValueError, match="m = "):
            ann.build_pq(X, idx, m)
    with pytest.raises(ValueError, match="m = "):
        ann.build_pq(torch.zeros(50, 100), _host_index(dim=100), 65)
    with pytest.raises(ValueError, match="built on"):
        ann.build_pq(torch.zeros(51, 8), idx, 4)
    with pytest.raises(ValueError, match="IVFIndex"):
        ann.build_pq(X, None, 4)
    with pytest.raises(ValueError, match="train_rows"):
        ann.build_pq(X, idx, 4, train_rows=0)
    with pytest.raises(ValueError, match="inv_norm"):
        ann.build_pq(X, idx, 4, inv_norm=torch.ones(49))
    assert [ann.code_stride(m) for m in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]


def test_search_pq_checks_its_arguments_before_the_gpu():
    from node2vec_amd import ann

    idx = _host_index()
    assert isinstance(idx, ann.IVFIndex) and (idx.m, idx.dsub, idx.refine, idx.nlist) == (4, 2, 0, 4)
    Q, X = torch.zeros(3, 8), torch.zeros(50, 8)
    with pytest.raises(ValueError, match="similarity.knn"):
        ann.search_pq(idx, 129, queries=Q)
    with pytest.raises(ValueError, match="similarity.knn"):
        ann.search_pq(idx, 128, rows=[1], X=X, exclude_self=True)
    with pytest.raises(ValueError):
        ann.search_pq(idx, 0, queries=Q)
    with pytest.raises(ValueError, match="refine"):
        ann.search_pq(idx, 5, queries=Q, refine=-1)
    with pytest.raises(ValueError, match="exclude_self"):
        ann.search_pq(idx, 5, queries=Q, exclude_self=True)
    with pytest.raises(ValueError, match="IVFPQIndex"):
        ann.search_pq(ann.IVFIndex(idx.centroids, None, idx.list_off, idx.row_ids, 13, 50, 8, 2), 5, queries=Q)
    with pytest.raises(ValueError, match="exactly one"):
        ann.search_pq(idx, 5)
    with pytest.raises(ValueError, match="exactly one"):
        ann.search_pq(idx, 5, queries=Q, rows=[1], X=X)
    with pytest.raises(ValueError, match="rows= needs X"):
        ann.search_pq(idx, 5, rows=[1])
    with pytest.raises(ValueError, match="refine > 0 needs X"):
        ann.search_pq(idx, 5, queries=Q, refine=2)
    with pytest.raises(ValueError, match="built on"):
        ann.search_pq(idx, 5, queries=Q, X=torch.zeros(51, 8), refine=1)


# ---- KeyedVectors: which search an index is handed to ------------------------------------------------------------

def test_keyed_vectors_routes_an_index_by_its_kind(monkeypatch):
    """the library mocked: build_index(pq=m) builds the coarse index, then the codes, and indexer= goes to
    ann.search_pq for an IVFPQIndex (with X, for the query rows and the re-rank) and to ann.search otherwise"""
    from node2vec_amd import ann
    from node2vec_amd.embedding import KeyedVectors

    n, dim = 30, 8
    kv = KeyedVectors(np.arange(n, dtype=np.int64), np.eye(n, dim, dtype=np.float32) + 1)
    X = torch.from_numpy(np.asarray(kv.vectors, np.float32))
    monkeypatch.setattr(kv, "_device_vectors", lambda: X)
    monkeypatch.setattr(kv, "init_sims", lambda replace=False: None)
    kv._inv_norm = torch.ones(n)
    pq_index = _host_index(n, dim, 4, 4)
    flat = ann.IVFIndex(pq_index.centroids, pq_index.centroid_inv_norm, pq_index.list_off, pq_index.row_ids,
                        pq_index.max_list_rows, n, dim, 2)
    calls = []

    def build_index(Xa, **kw):
        calls.append(("build_index", kw))
        return flat

    def build_pq(Xa, index, m, **kw):
        calls.append(("build_pq", index, m, kw))
        return pq_index

    def search(Xa, index, k, **kw):
        calls.append(("search", index, k, kw))
        return torch.arange(k)[None], torch.zeros(1, k)

    def search_pq(index, k, **kw):
        calls.append(("search_pq", index, k, kw))
        return torch.arange(k)[None], torch.zeros(1, k)

    for name, fn in (("build_index", build_index), ("build_pq", build_pq), ("search", search),
                     ("search_pq", search_pq)):
        monkeypatch.setattr(ann, name, fn)
    assert kv.build_index(nlist=4, seed=3) is flat and [c[0] for c in calls] == ["build_index"]
    calls.clear()
    got = kv.build_index(nlist=4, seed=3, pq=4, refine=7, max_iter=5)
    assert got is pq_index and got.refine == 7
    assert [c[0] for c in calls] == ["build_index", "build_pq"]
    assert calls[0][1]["nlist"] == 4 and calls[0][1]["seed"] == 3 and calls[0][1]["max_iter"] == 5
    assert calls[1][1] is flat and calls[1][2] == 4 and calls[1][3]["seed"] == 3
    with pytest.raises(ValueError, match="refine"):
        kv.build_index(nlist=4, pq=4, refine=-1)
    calls.clear()
    hits = kv.most_similar("3", topn=5, indexer=pq_index)
    assert calls[0][0] == "search_pq" and calls[0][1] is pq_index and calls[0][2] == 6  # topn + the token itself
    assert calls[0][3]["X"] is X and calls[0][3]["refine"] == 7 and "queries" in calls[0][3]
    assert [t for t, _ in hits] == ["0", "1", "2", "4", "5"]
    kv.similar_by_vector(np.ones(dim, np.float32), topn=4, indexer=pq_index)
    assert calls[-1][0] == "search_pq" and calls[-1][2] == 4
    kv.nearest([1, 2], 3, indexer=pq_index)
    assert calls[-1][0] == "search_pq" and calls[-1][3]["exclude_self"] is True and calls[-1][3]["rows"] == [1, 2]
    calls.clear()
    kv.most_similar("3", topn=5, indexer=flat)
    kv.nearest([1, 2], 3, exclude_self=False, indexer=flat)
    assert [c[0] for c in calls] == ["search", "search"] and calls[0][1] is flat and calls[0][2] == 6
    assert calls[1][3]["exclude_self"] is False and calls[1][3]["inv_norm"] is kv._inv_norm
    for call in (lambda: kv.most_similar("3", restrict_vocab=10, indexer=pq_index),
                 lambda: kv.most_similar("3", topn=None, indexer=pq_index)):
        with pytest.raises(ValueError):
            call()
