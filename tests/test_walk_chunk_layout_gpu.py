"""The p = q = 1 walk stores its paths step-major per wave (walk_uniform_kernel<.., true>) and a second kernel
turns every wave's region row-major in place (walk_chunk_transpose_kernel): what comes back is the row-major
array of before, bit for bit the CPU oracle's -- for every form of the kernel (CSR arrays, 16-byte table,
hops8, degree ranks mapped back through rank_vertex, the pair table), walker counts around the 64 of a region
and past one grid pass, walk lengths around the 16 words of a sector and on either side of the LDS bound
(walk_length + 1 <= 256: longer walks keep the register-sector path), sinks, a start vertex without edges, an
output that is a view at a 4-byte aligned offset into a larger buffer whose other words must not change, and
twice the same bytes from two calls."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

FORMS = ("csr", "hops16", "hops8", "ranked", "pairs")
NV = 4000
_graphs = {}
_refs = {}


def _graph(form):
    """sinks (ids >= NV - 60), ten hubs, multi-edges (the graph of tests/test_rank_pairs_gpu.py); one graph
    takes the 8-byte hop table, the other declines it so that the pair table serves"""
    from node2vec_amd.graph import DeviceGraph

    key = "hops8" if form == "hops8" else "other"
    if key not in _graphs:
        rng = np.random.default_rng(8)
        src = np.concatenate([rng.integers(0, NV - 60, 30000), rng.integers(0, 10, 12000),
                              rng.integers(0, NV - 60, 9000)])
        dst = np.concatenate([rng.integers(0, NV, 30000), rng.integers(0, NV, 12000), rng.integers(0, 10, 9000)])
        g = DeviceGraph.from_edges(src, dst, None, n_vertices=NV, device="cuda")
        if key == "other":
            g.hops8_tried = True
        _graphs[key] = g
    return _graphs[key]


def _starts(n):
    """n start vertices: sinks and vertices with edges, repeated once n exceeds the graph"""
    return torch.from_numpy(((np.arange(n, dtype=np.int64) * 7 + 3) % NV).astype(np.int32))


def _want(oracle, start, W, L, seed):
    """the oracle's walks and valid flags, computed once per case and shared by the five forms"""
    key = (start.numel(), W, L, seed)
    if key not in _refs:
        g = _graph("csr")
        want, wv = oracle.random_walk(g.rowptr.cpu().numpy(), g.col.cpu().numpy(), None, start.numpy(), W, L,
                                      1.0, 1.0, seed, n_threads=8)
        want.setflags(write=False)
        wv.setflags(write=False)
        _refs[key] = (want, wv)
    return _refs[key]


def _walk(form, start, W, L, seed, out=None):
    """walks as vertex ids (numpy int32) and valid (numpy bool) from the given form of the kernel"""
    from node2vec_amd import randomwalk as rw

    g = _graph(form)
    kw = {"csr": dict(use_hops=False), "hops16": dict(use_hops8=False), "hops8": {}, "ranked": dict(rank_ids=True),
          "pairs": {}}[form]
    walks, valid = rw.walk(g, start, W, L, 1.0, 1.0, seed, out=out, **kw)
    if form == "hops8":
        assert g.hops8 is not None
    if form == "pairs":
        assert g.rank_pairs is not None and g.hops8 is None
    if form == "ranked":
        assert g.rank_hops is not None
        walks = torch.where(walks >= 0, g.rank_vertex[walks.clamp(min=0).long()].to(walks.dtype), walks)
    if form == "hops16":
        assert g.hops is not None
    return walks.cpu().numpy(), valid.cpu().numpy().astype(bool)


def _check(oracle, form, start, W, L, seed):
    want, wv = _want(oracle, start, W, L, seed)
    got, gv = _walk(form, start, W, L, seed)
    assert got.shape == want.shape and got.dtype == np.int32
    assert np.array_equal(gv, wv)
    assert np.array_equal(got, want)  # every row: a walker that vanished keeps its prefix, the tail is -1
    return got, gv


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_start,W", [(5, 1), (64, 1), (65, 1), (37, 3), (65537, 1)])
def test_walker_counts_around_a_region(oracle, form, n_start, W):
    _check(oracle, form, _starts(n_start), W, 6 if n_start > 1000 else 17, 4)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_more_walkers_than_resident_lanes(oracle, form):
    """524 288 lanes are resident on 256 CUs: the waves of the second pass take their regions from the same
    counter, the last region holds 197 - 192 = 5 rows"""
    _, gv = _check(oracle, form, _starts(524288 + 197), 1, 4, 11)
    assert gv.any() and not gv.all()


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L", [0, 1, 15, 16, 63, 64, 80, 255, 256])
def test_walk_lengths(oracle, form, L):
    """255 is the longest walk whose tile fits (64 * 256 words = 64 KB of LDS); 256 takes the register-sector
    path in one kernel"""
    _check(oracle, form, _starts(100), 3, L, 5)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_sinks_and_a_start_vertex_without_edges(oracle, form):
    g = _graph(form)
    deg = g.degrees().cpu().numpy()
    assert deg[NV - 1] == 0 and deg[5] > 0
    start = torch.tensor([5, NV - 1, 17, 0, NV - 2], dtype=torch.int32)
    got, gv = _check(oracle, form, start, 7, 33, 9)
    assert not gv[7:14].any() and (got[7:14] == -1).all()  # the walkers of the vertex without edges
    dead = ~gv
    dead[7:14] = False
    dead[28:35] = False
    assert dead.any()  # walkers that vanished at a sink on their way
    for row in got[dead]:
        end = int(np.argmax(row == -1))
        assert end >= 1 and (row[:end] >= 0).all() and (row[end:] == -1).all() and deg[row[end - 1]] == 0


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_start,W", [(37, 3), (64, 2)])
def test_view_at_a_four_byte_offset_keeps_its_surroundings(oracle, form, n_start, W):
    """111 walkers end in a partial region, 128 fill two; the output starts an odd number of words into a larger
    buffer (aligned to 4 bytes only) and no word before or after rows [0, total) may change"""
    L, total = 21, n_start * W
    L1 = L + 1
    sentinel = -77
    off = 2 * L1 + 1
    flat = torch.full((off + total * L1 + 2 * L1,), sentinel, dtype=torch.int32, device="cuda")
    vflat = torch.full((3 + total + 5,), 99, dtype=torch.uint8, device="cuda")
    walks = flat[off:off + total * L1].view(total, L1)
    assert walks.data_ptr() % 8 == 4
    start = _starts(n_start)
    want, wv = _want(oracle, start, W, L, 6)
    got, gv = _walk(form, start, W, L, 6, out=(walks, vflat[3:3 + total]))
    assert np.array_equal(gv, wv) and np.array_equal(got, want)
    assert bool((flat[:off] == sentinel).all()) and bool((flat[off + total * L1:] == sentinel).all())
    assert bool((vflat[:3] == 99).all()) and bool((vflat[3 + total:] == 99).all())


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_two_calls_return_the_same_bytes(form):
    start = _starts(333)
    a, av = _walk(form, start, 3, 80, 12)
    b, bv = _walk(form, start, 3, 80, 12)
    assert a.tobytes() == b.tobytes() and av.tobytes() == bv.tobytes()
