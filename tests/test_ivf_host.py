"""The inverted-file index (node2vec_amd/ann.py, csrc/n2v_ivf.hip), the parts that need no GPU: the numpy restatement
the GPU tests compare against (tests/ivf_cases.py) checked against the exact oracle, ann.layout, and the argument
checks and size queries of the three entry points (nothing is launched: the library loads without a device)."""
import ctypes

import numpy as np
import pytest
import torch

import ivf_cases as ic
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)


@pytest.mark.parametrize("n,dim,nq,k,nlist", [(300, 17, 9, 10, 7), (1000, 64, 20, 128, 32), (50, 3, 5, 60, 4)])
def test_restatement_with_every_list_probed_is_the_exact_oracle(oracle, n, dim, nq, k, nlist):
    rng = np.random.default_rng(n + dim)
    X = ic.mixed_rows(rng, n, dim)
    X[5, 0] = np.nan
    labels = rng.integers(0, nlist, n)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    R = rng.integers(0, n, nq)
    probes = np.tile(rng.permutation(nlist), (nq, 1))
    ic.same(ic.expect(oracle, X, labels, probes, k, queries=Q), oracle.knn_topk(X, k, queries=Q), "queries")
    ic.same(ic.expect(oracle, X, labels, probes, k, rows=R), oracle.knn_topk(X, k, rows=R), "rows")
    ic.same(ic.expect(oracle, X, labels, probes, k, rows=R, exclude=R), oracle.knn_topk(X, k, rows=R, exclude=R),
            "exclude")
    lists = ic.lists_of(labels, nlist)
    ic.same(ic.expect(oracle, X, lists, probes, k, queries=Q), oracle.knn_topk(X, k, queries=Q), "lists")


def test_layout():
    from node2vec_amd import ann

    labels = torch.tensor([2, 0, -1, 2, 5, 0, 1, 2, 4, 0, -7], dtype=torch.int32)
    off, rows = ann.layout(labels, 4)
    assert off.dtype == torch.int64 and rows.dtype == torch.int32
    assert off.tolist() == [0, 3, 4, 7, 7]  # list 3 is empty: equal offsets; labels -1, -7, 4 and 5 are dropped
    assert rows.tolist() == [1, 5, 9, 6, 0, 3, 7]  # ascending inside every list
    assert int(off[-1]) == len(rows)
    rng = np.random.default_rng(1)
    lab = rng.integers(-1, 40, 5000)
    off, rows = ann.layout(torch.from_numpy(lab), 37)
    off, rows = off.numpy(), rows.numpy()
    assert off[-1] == len(rows) == int(((lab >= 0) & (lab < 37)).sum())
    for l in range(37):
        mine = rows[off[l]:off[l + 1]]
        assert np.array_equal(mine, np.nonzero(lab == l)[0])  # stable: original order, nothing lost
    off, rows = ann.layout(torch.full((10,), -1), 3)
    assert off.tolist() == [0, 0, 0, 0] and rows.numel() == 0
    with pytest.raises(ValueError):
        ann.layout(torch.zeros(4), 3)
    with pytest.raises(ValueError):
        ann.layout(torch.zeros(4, dtype=torch.int64), 0)


def _calls():
    from node2vec_amd import _lib

    L = _lib.load()
    buf = (ctypes.c_int64 * 1024)()
    p_ = (ctypes.addressof(buf) + 255) & ~255  # aligned, inside the buffer: never dereferenced

    def topk(**kw):
        a = dict(X=p_, inv=p_, n=100, dim=8, off=p_, ids=p_, nlist=4, mlr=50, q=p_, qr=0, nq=3, probes=p_, nprobe=2,
                 k=5, out_r=p_, out_s=p_, status=p_, ws=p_, ws_bytes=1 << 40)
        a.update(kw)
        return L.n2v_ivf_topk(a["X"], a["inv"], a["n"], a["dim"], a["off"], a["ids"], a["nlist"], a["mlr"], a["q"],
                              a["qr"], a["nq"], a["probes"], a["nprobe"], a["k"], a["out_r"], a["out_s"], a["status"],
                              a["ws"], a["ws_bytes"], None)

    def sizes(**kw):
        a = dict(n=100, dim=8, nlist=4, mlr=50, nq=3, nprobe=2, k=5)
        a.update(kw)
        return a["n"], a["dim"], a["nlist"], a["mlr"], a["nq"], a["nprobe"], a["k"]

    return L, p_, topk, sizes


BAD_SIZES = [dict(nlist=0), dict(nlist=1025, nprobe=1), dict(nprobe=0), dict(nprobe=5), dict(k=0), dict(k=129),
             dict(dim=0), dict(dim=1025), dict(mlr=0), dict(mlr=101), dict(nq=-1), dict(nq=1 << 20), dict(n=-1),
             dict(n=1 << 31)]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    L, p_, topk, sizes = _calls()
    plan3 = (ctypes.c_int64 * 3)()
    for bad in BAD_SIZES:
        assert topk(**bad) == -1, bad
        assert L.n2v_ivf_workspace_bytes(*sizes(**bad)) == -1, bad
        assert L.n2v_ivf_plan(*sizes(**bad), plan3) == -1, bad
    assert L.n2v_ivf_plan(*sizes(), None) == -1
    for name in ("X", "inv", "off", "ids", "probes", "out_r", "out_s", "status", "ws"):
        assert topk(**{name: 0}) == -1, name
    assert topk(q=p_, qr=p_) == -1 and topk(q=0, qr=0) == -1  # exactly one of queries / query_rows
    need = L.n2v_ivf_workspace_bytes(*sizes())
    assert need > 0
    assert topk(ws_bytes=need - 1) == -1 and topk(ws=p_ + 4) == -1 and topk(ws=p_ + 8) == -1
    # nothing to do: N2V_OK and no launch (there is no device here to launch on)
    assert topk(nq=0) == 0 and topk(nq=0, q=0, qr=p_) == 0
    assert topk(n=0, mlr=1) == 0
    assert topk(nq=0, k=0) == -1 and topk(nq=0, q=0) == -1  # (refused before the empty batch returns)
    assert L.n2v_ivf_workspace_bytes(*sizes(nq=0)) == 0 and L.n2v_ivf_workspace_bytes(*sizes(n=0, mlr=1)) == 0


def test_workspace_bytes_and_plan():
    from node2vec_amd import ann

    L, _, _, sizes = _calls()
    grid = dict(nq=(1, 2, 15, 16, 17, 63, 64, 65, 200, 1000, 4096), nprobe=(1, 2, 3, 7, 8, 16, 32),
                k=(1, 2, 10, 64, 127, 128))
    base = dict(n=100000, dim=64, nlist=32, mlr=9000)
    for name, values in grid.items():
        for other in ({}, dict(nq=200, nprobe=8, k=10), dict(nq=4096, nprobe=32, k=128)):
            got = [L.n2v_ivf_workspace_bytes(*sizes(**{**base, **other, name: v})) for v in values]
            assert all(b > 0 for b in got) and got == sorted(got), (name, other, got)
    # the plan: pairs per tile by the average group, the chunks by max_list_rows alone
    assert ann.plan(100000, 64, 32, 9000, 200, 8, 10) == (64, 1920, 5)
    assert ann.plan(100000, 64, 32, 9000, 64, 8, 10)[0] == 16 and ann.plan(100000, 64, 32, 9000, 65, 8, 10)[0] == 64
    assert ann.plan(6000, 64, 9, 5376, 200, 1, 10) == (64, 1792, 3)
    assert ann.plan(6000, 64, 9, 5376, 100, 1, 10) == (16, 1792, 3)
    assert ann.plan(6000, 64, 9, 1, 100, 1, 10) == (16, 128, 1) and ann.plan(6000, 64, 9, 2048, 5, 1, 1)[1:] == (2048, 1)
    assert ann.plan(6000, 64, 9, 2049, 5, 1, 1)[1:] == (1152, 2)
    with pytest.raises(ValueError):
        ann.plan(6000, 64, 9, 5376, 100, 1, 129)
    # more scan blocks than one launch takes: refused by all three, so that callers split the queries
    assert L.n2v_ivf_workspace_bytes(1 << 24, 64, 1024, 1 << 24, (1 << 20) - 1, 1024, 1) == -1


def test_symbols_are_bound_and_declared():
    import os

    from node2vec_amd import _lib

    header = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("n2v_ivf_workspace_bytes", "n2v_ivf_plan", "n2v_ivf_topk"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert _lib.ABI_VERSION == 15


def test_search_checks_its_arguments_before_the_gpu():
    from node2vec_amd import ann

    X = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="similarity.knn"):
        ann.search(X, None, 129, queries=X)
    with pytest.raises(ValueError, match="similarity.knn"):
        ann.search(X, None, 128, rows=[1], exclude_self=True)
    with pytest.raises(ValueError):
        ann.search(X, None, 0, queries=X)
    with pytest.raises(ValueError):
        ann.search(X, None, 5, queries=X, exclude_self=True)
