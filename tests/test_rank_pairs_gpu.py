"""The pair table of a unit-weight graph (n2v_rank_pairs_build: 8-byte {vertex id, rank} entries in the
degree-ranked layout) and the p = q = 1 walk that writes vertex ids from it (n2v_graph.rank_emit == 2):
table contents against numpy, walks bit-identical to the 16-byte hop table, the CSR arrays, the 4-byte
ranked form and the CPU oracle -- with and without the head table, sinks, hubs, multi-edges, walk lengths 0, 1
and across output sectors; what walk() builds and what it leaves alone; the argument checks (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
gpu = pytest.mark.gpu


def _graph(seed=8, nv=4000):
    """sinks (ids >= nv - 60), ten hubs, multi-edges (the graph of tests/test_ranked_gpu.py)"""
    from node2vec_amd.graph import DeviceGraph

    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, nv - 60, 30000), rng.integers(0, 10, 12000), rng.integers(0, nv - 60, 9000)])
    dst = np.concatenate([rng.integers(0, nv, 30000), rng.integers(0, nv, 12000), rng.integers(0, 10, 9000)])
    return DeviceGraph.from_edges(src, dst, None, n_vertices=nv, device="cuda")


def _rows_from_tables(g):
    """(row start, degree) of every rank as the walk kernel derives them: head table, else class search"""
    n = g.n_vertices
    head = np.zeros(0, np.uint64) if g.rank_head is None else g.rank_head.cpu().numpy().astype(np.uint64)
    first = g.rank_class_first.cpu().numpy().astype(np.uint32).astype(np.int64)
    off = g.rank_class_off.cpu().numpy().astype(np.uint32).astype(np.int64)
    P = first.size
    assert P & (P - 1) == 0 and 2 <= P <= 8192 and first[0] == head.size
    assert first[-1] == n and off[-1] == g.n_edges  # the entry that closes the last class
    r = np.arange(n, dtype=np.int64)
    c = np.zeros(n, np.int64)
    half = P >> 1
    while half:  # the kernel's fixed-depth search
        c = np.where(first[np.minimum(c + half, P - 1)] <= r, c + half, c)
        half >>= 1
    deg = (off[c + 1] - off[c]) // (first[c + 1] - first[c])
    row = off[c] + (r - first[c]) * deg
    H = head.size
    row[:H] = (head & np.uint64((1 << 40) - 1)).astype(np.int64)
    deg[:H] = (head >> np.uint64(40)).astype(np.int64)
    return row, deg


def _without_hops8(g):
    """the small test graph's field widths would accept the 8-byte hop table, which comes first: decline it"""
    g.hops8_tried = True
    return g


@gpu
@pytest.mark.parametrize("max_classes", [8191, 16, 1])
def test_pair_table_holds_the_graph(max_classes):
    g = _graph()
    g.RANK_MAX_CLASSES = max_classes  # few classes: most ranks go through the head table
    g.build_rank_pairs()
    assert g.rank_pairs is not None and g.rank_pairs.dtype == torch.int64 and g.rank_pairs.numel() == g.n_edges
    assert g.rank_hops is None and g.hops is None  # neither the 4-byte nor the 16-byte table as a side effect
    deg = g.degrees().cpu().numpy()
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    rv, ro = g.rank_vertex.cpu().numpy(), g.rank_of.cpu().numpy()
    assert np.array_equal(rv, np.argsort(-deg, kind="stable"))
    assert np.array_equal(ro[rv], np.arange(g.n_vertices))
    row, d = _rows_from_tables(g)  # the rows as the walk kernel derives them
    assert np.array_equal(d, deg[rv])
    assert np.array_equal(row, np.concatenate([[0], np.cumsum(deg[rv])[:-1]]))
    if max_classes < 4096:
        assert g.rank_head is not None and g.rank_class_first.numel() == 2 * max_classes
    pairs = g.rank_pairs.cpu().numpy().view(np.uint64)
    low = (pairs & np.uint64(0xffffffff)).astype(np.int64)
    high = (pairs >> np.uint64(32)).astype(np.int64)
    # every entry: rows in rank order, the CSR's neighbour order inside a row
    src_rank = np.repeat(np.arange(g.n_vertices), d)
    at_csr = rowptr[rv[src_rank]] + (np.arange(col.size) - row[src_rank])
    assert np.array_equal(low, col[at_csr].astype(np.int64))
    assert np.array_equal(high, ro[col[at_csr]].astype(np.int64))


@gpu
@pytest.mark.parametrize("max_classes", [8191, 16, 1])
def test_pair_walks_change_no_bit(oracle, max_classes):
    from node2vec_amd import randomwalk as rw

    g = _without_hops8(_graph())
    g.RANK_MAX_CLASSES = max_classes
    start = rw.start_vertices(g)
    for L in (0, 1, 14, 15, 16, 30, 80):
        a, av = rw.walk(g, start, 3, L, 1.0, 1.0, 4)
        assert g.rank_pairs is not None and g.hops is None and g.hops8 is None  # the pair table served
        b, bv = rw.walk(g, start, 3, L, 1.0, 1.0, 4, use_hops8=False)  # the 16-byte table
        assert g.hops is not None
        c, cv = rw.walk(g, start, 3, L, 1.0, 1.0, 4, use_hops=False)  # the CSR arrays
        d, dv = rw.walk(g, start, 3, L, 1.0, 1.0, 4, use_ranked=True)  # 4-byte ranks + rank_vertex
        assert torch.equal(a, b) and torch.equal(av, bv) and torch.equal(a, c) and torch.equal(av, cv)
        assert torch.equal(a, d) and torch.equal(av, dv)
        g.hops = None
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    want, wv = oracle.random_walk(rowptr, col, None, start.cpu().numpy(), 3, 30, 1.0, 1.0, 4, n_threads=8)
    a, av = rw.walk(g, start, 3, 30, 1.0, 1.0, 4)
    assert g.hops is None
    assert np.array_equal(av.cpu().numpy(), wv) and np.array_equal(a.cpu().numpy()[wv], want[wv])
    assert not wv.all()  # walkers vanished at sinks
    # start vertices that are sinks (3999) or repeated, an odd number of walkers
    odd = torch.tensor([5, 0, 3999, 17, 5], dtype=torch.int32)
    a, av = rw.walk(g, odd, 7, 33, 1.0, 1.0, 9)
    assert g.hops is None
    b, bv = rw.walk(g, odd, 7, 33, 1.0, 1.0, 9, use_hops8=False)
    c, cv = rw.walk(g, odd, 7, 33, 1.0, 1.0, 9, use_hops=False)
    assert torch.equal(a, b) and torch.equal(av, bv) and torch.equal(a, c) and torch.equal(av, cv)
    assert not bool(av[14:21].any()) and bool((a[14:21] == -1).all())  # the sink's walkers
    want, wv = oracle.random_walk(rowptr, col, None, odd.numpy(), 7, 33, 1.0, 1.0, 9, n_threads=8)
    assert np.array_equal(av.cpu().numpy(), wv) and np.array_equal(a.cpu().numpy()[wv], want[wv])
    g.hops = None
    with pytest.raises(ValueError):  # out of range: raises as on every other path
        rw.walk(g, torch.tensor([4000], dtype=torch.int32), 1, 3, 1.0, 1.0, 1)
    assert g.hops is None


@gpu
def test_default_walk_builds_the_pair_table_and_nothing_else():
    from node2vec_amd import randomwalk as rw

    g = _without_hops8(_graph())
    start = rw.start_vertices(g)
    a, av = rw.walk(g, start, 3, 25, 1.0, 1.0, 9)
    assert g.rank_pairs is not None and g.rank_pairs_tried
    assert g.rank_hops is None and g.hops is None and g.hops8 is None
    b, bv = rw.walk(g, start, 3, 25, 1.0, 1.0, 9, use_rank_pairs=False)  # the 16-byte table
    assert g.hops is not None and g.rank_hops is None
    assert torch.equal(a, b) and torch.equal(av, bv)
    # the 8-byte hop table comes first where the graph accepts it
    g2 = _graph()
    c, cv = rw.walk(g2, start, 3, 25, 1.0, 1.0, 9)
    assert g2.hops8 is not None and g2.rank_pairs is None and not g2.rank_pairs_tried
    assert torch.equal(a, c) and torch.equal(av, cv)
    # biased walks and rank_ids never ask for it
    g3 = _without_hops8(_graph())
    rw.walk(g3, start, 1, 5, 0.5, 2.0, 9)
    rw.walk(g3, start, 1, 5, 1.0, 1.0, 9, rank_ids=True)
    assert g3.rank_pairs is None and g3.rank_hops is not None
    # the copy of a graph carries the table and the bookkeeping
    g4 = g.to(g.device)
    assert g4.rank_pairs is not None and g4.rank_pairs_tried and g4.rank_hops is None


@gpu
def test_pair_table_is_declined_where_it_does_not_apply():
    from node2vec_amd import randomwalk as rw
    from node2vec_amd.graph import DeviceGraph

    w = DeviceGraph.from_edges(np.array([0, 1, 2]), np.array([1, 2, 0]), np.array([1.0, 2.0, 3.0]), n_vertices=3,
                               device="cuda")
    assert w.build_rank_pairs().rank_pairs is None and w.rank_pairs_tried
    g = _without_hops8(_graph())
    assert g.build_rank_pairs(max_bytes=8 * g.n_edges - 1).rank_pairs is None  # no room
    assert g.rank_of is None
    start = rw.start_vertices(g)
    a, av = rw.walk(g, start, 3, 25, 1.0, 1.0, 9)  # declined once: the 16-byte table serves
    assert g.rank_pairs is None and g.hops is not None
    g.RANK_MAX_HEAD = 4  # more top vertices than the head table may list: as build_ranked
    g.RANK_MAX_CLASSES = 1
    assert g.build_rank_pairs().rank_pairs is None and g.build_ranked().rank_hops is None
    g.RANK_MAX_HEAD, g.RANK_MAX_CLASSES = DeviceGraph.RANK_MAX_HEAD, DeviceGraph.RANK_MAX_CLASSES
    b, bv = rw.walk(g.build_rank_pairs(), start, 3, 25, 1.0, 1.0, 9)
    assert g.rank_pairs is not None and torch.equal(a, b) and torch.equal(av, bv)
    # after the ranked form: its tables are shared, its 4-byte entries stay
    g5 = _without_hops8(_graph()).build_ranked()
    ro = g5.rank_of
    c, cv = rw.walk(g5, start, 3, 25, 1.0, 1.0, 9)
    assert g5.rank_pairs is not None and g5.rank_of is ro and g5.rank_hops is not None
    assert torch.equal(a, c) and torch.equal(av, cv)


# ---- host only: nothing below launches anything ------------------------------------------------------------

def test_pair_table_entry_point_is_declared_and_exported():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bn2v_rank_pairs_build\s*\(", text)
    assert "n2v_rank_pairs_build" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "n2v_rank_pairs_build")


def _fake():
    buf = (ctypes.c_int64 * 64)()
    return buf, ctypes.addressof(buf) & ~31  # (inside the buffer's page: never dereferenced)


def test_pair_table_build_validates_its_arguments():
    """argument errors come back as N2V_EINVAL (-1) before any launch, as from n2v_rank_hops_build"""
    from node2vec_amd import _lib

    L = _lib.load()
    buf, p_ = _fake()

    def build(fn, rank_of=p_, rank_vertex=p_, rank_rowptr=p_, out=p_, **kw):
        g = _lib.Graph()
        g.n_vertices, g.n_edges, g.rowptr, g.col = 4, 8, p_, p_
        for k, v in kw.items():
            setattr(g, k, v)
        return fn(g, rank_of, rank_vertex, rank_rowptr, out, None)

    for fn in (L.n2v_rank_pairs_build, L.n2v_rank_hops_build):
        assert build(fn, n_edges=0) == 0  # nothing to do
        assert build(fn, n_edges=-1) == -1 and build(fn, n_vertices=-1) == -1 and build(fn, rowptr=0) == -1
        assert build(fn, w=p_) == -1 and build(fn, w64=p_) == -1  # unit weights only
        assert build(fn, n_edges=1 << 40) == -1 and build(fn, n_vertices=1 << 31) == -1
        assert build(fn, col=0) == -1 and build(fn, rank_of=0) == -1 and build(fn, rank_vertex=0) == -1
        assert build(fn, rank_rowptr=0) == -1 and build(fn, out=0) == -1
    assert L.n2v_rank_pairs_build(None, p_, p_, p_, p_, None) == -1


def test_walk_refuses_a_rank_emit_it_does_not_know():
    """n2v_walk with the rank tables set: rank_emit 3, and rank_emit 2 (the pair table) without rank_of or the
    class tables, are N2V_EINVAL before anything is put on the stream"""
    from node2vec_amd import _lib

    L = _lib.load()
    buf, p_ = _fake()

    def walk(**kw):
        g = _lib.Graph()
        g.n_vertices, g.n_edges, g.rowptr, g.col = 4, 8, p_, p_
        g.rank_hops = g.rank_of = g.rank_vertex = g.rank_class_first = g.rank_class_off = p_
        g.rank_classes, g.rank_emit = 2, 2
        for k, v in kw.items():
            setattr(g, k, v)
        return L.n2v_walk(g, p_, 1, 1, 3, 1.0, 1.0, 7, _lib.WALK_EXACT, p_, p_, p_, None)

    assert walk(rank_emit=3) == -1 and walk(rank_emit=-1) == -1 and walk(rank_emit=4) == -1
    assert walk(rank_of=0) == -1
    assert walk(rank_class_first=0) == -1 and walk(rank_class_off=0) == -1
    assert walk(rank_classes=3) == -1 and walk(rank_classes=16384) == -1
    assert walk(rank_head_n=2) == -1  # head ranks without a head table
    assert walk(n_edges=1 << 32) == -1  # row offsets are 32 bits in this form
    assert walk(rank_emit=0, rank_vertex=0) == -1  # the 4-byte form translating back needs rank_vertex
