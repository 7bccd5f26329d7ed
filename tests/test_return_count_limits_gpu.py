"""Exact walks where an edge's return count leaves its field of the class word.

edge_classes[e] keeps the return count of an edge in 8 bits.  From 128 on the inline hop-table form (7 bits) is
declined for the whole graph; 255 stands for "255 or more", the wedge lists are declined for the whole graph and
every exact kernel classifies such a row itself.  The graphs of return_count_cases.py put bundles of 126 .. 129,
254, 255, 256 and 300 parallel edges on both sides of both limits; test_return_count_cases_host.py proves them, and
that the oracle draws from every bundle's table hundreds of times per (p, q).

Here: the class words, edge by edge, against plain Python counts; what the host decides from them; and the walks of
every dispatch that the flags of randomwalk.walk reach against the oracle, bit for bit (walks and valid flags, so the
runs also equal each other), with the status word read back and the tables that the launch saw asserted after every
run.  Which kernel a set of tables means (n2v_walk_exact_unit_try, n2v_walk_wedge_try) is said beside each flag set.
No comparison here has a tolerance.
"""
import numpy as np
import pytest
import torch

import return_count_cases as R

pytestmark = pytest.mark.gpu

# the flags of randomwalk.walk and the kernel they reach on a graph WITH wedge lists / on `saturated` (no lists: the
# lanes kernel walk_exact_unit_lanes_kernel for dyadic p, q with 1/q <= 1 and 1/p >= 1/q, else the wave-per-walker
# kernel walk_exact_unit_kernel -- "lanes | wave" below)
FLAGS = {
    "default": {},                                   # wedge slots kernel | lanes / wave, hop table
    "no hops": {"use_hops": False},                  # lanes / wave on the CSR arrays, lists at hand | the same, none
    "by search": {"use_hops": False, "use_edge_classes": False},  # wave kernel, classes by search | the same
    "no wedges": {"use_wedges": False},              # lanes / wave, hop table, membership by search | the same
    "no hops, no wedges": {"use_hops": False, "use_wedges": False},  # lanes / wave on the CSR arrays | the same
    "no wedge kernel": {"use_wedge_kernel": False},  # lanes / wave with lists and hop table | lanes / wave
    "no wedge slots": {"use_wedge_slots": False},    # wedge kernel through wedge_off | lanes / wave
    "no inline rpos": {"use_inline_rpos": False},    # wedge slots kernel, plain class words | lanes / wave
}
WEIGHTED_FLAGS = {  # all of them end in the wave-per-walker kernel of n2v_walk: the lists are declined
    "default": {},
    "lanes asked for": {"use_weighted_lanes": True},
    "wave": {"use_weighted_lanes": False},
    "wave, by search": {"use_weighted_lanes": False, "use_edge_classes": False},
}
_CACHE = {}


def _graph(name, key=None):
    """a DeviceGraph of the case; with a key: built once per (case, key), its tables with it"""
    from node2vec_amd.graph import DeviceGraph

    if key is None or (name, key) not in _CACHE:
        c = R.graphs()[name]
        w = None if c["weight"] is None else torch.from_numpy(c["weight"])
        g = DeviceGraph.from_edges(c["src"], c["dst"], w, device="cuda")
        assert g.unit_weights == (w is None)
        if key is None:
            return g
        _CACHE[(name, key)] = g
    return _CACHE[(name, key)]


def _start(g):
    from node2vec_amd import randomwalk as rw

    start = rw.start_vertices(g)
    assert start.numel() == g.n_vertices  # every vertex walks
    return start


def _walk(g, start, pq, **flags):
    """one exact walk with the status word checked by walk() and read back: no bit of it may be set"""
    from node2vec_amd import randomwalk as rw

    stats = {}
    walks, valid = rw.walk(g, start, R.NUM_WALKS, R.WALK_LENGTH, pq[0], pq[1], R.SEED, check=True, stats=stats,
                           **flags)
    assert int(stats["status"][0].item()) == 0, (pq, flags)
    return walks, valid, stats


def _assert_equal(got, want, what):
    walks, valid = got[0].cpu().numpy(), got[1].cpu().numpy().astype(bool)
    assert np.array_equal(valid, want[1]), what
    assert np.array_equal(walks, want[0]), what


def _assert_tables(g, name, flags):
    """the tables the launch saw (built on first use, so read after the walk) are the ones the flags stand for"""
    classes = flags.get("use_edge_classes", True)
    hops = flags.get("use_hops", True)
    wedges = classes and flags.get("use_wedges", True) and name != "saturated"
    assert (g.edge_classes is not None) == classes
    assert (g.hops is not None) == hops
    assert g.hops_have_classes == (hops and classes)
    assert (g.wedge_off is not None) == wedges and (g.wedge_slots is not None) == wedges
    assert g.hops8 is None and g.rank_hops is None and g.rank_pairs is None
    if name == "saturated" and classes and flags.get("use_wedges", True):
        assert g.wedge_tried and g.wedge_pos is None  # asked for, and declined
    assert g.hops_inline_rpos == (name == "below" and not flags)  # any flag off, or a count >= 128: plain words


# ---------------------------------------------------------------------------------- 1. the class words
@pytest.mark.parametrize("name", ["below", "inline_limit", "saturated", "saturated_w32", "saturated_w64", "hubs"])
def test_class_words_equal_the_plain_counts(name):
    g = _graph(name)
    g.build_edge_classes()
    got = g.edge_classes.cpu().numpy().view(np.uint32)
    want = R.class_words(name)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
    n_ret = R.edge_counts(name)[0]
    for m in {x["m"] for x in R.graphs()[name]["gadgets"]}:  # 254 stays 254; 255, 256 and 300 all read 255
        assert set((got[n_ret == m] >> 24).tolist()) == {min(m, R.RETURN_SAT)}, m


# ------------------------------------------------------------------------------ 2. what the host decides
def test_below_keeps_the_inline_form():
    g = _graph("below")
    g.build_wedges()
    assert g.wedge_off is not None and g.wedge_slots is not None and g.can_inline_rpos()
    _walk(g, _start(g), (0.5, 2.0))
    assert g.hops is not None and g.hops_inline_rpos


def test_inline_limit_declines_the_inline_form():
    from node2vec_amd import _lib

    g = _graph("inline_limit")
    g.build_wedges()
    assert g.wedge_off is not None and g.wedge_pos is not None and g.wedge_slots is not None and g.wedge_mode == 0
    assert not g.can_inline_rpos()
    g.build_hops(inline_rpos=True)  # asked for all the same: the plain form
    assert g.hops is not None and not g.hops_inline_rpos
    _walk(g, _start(g), (0.5, 2.0))
    assert g.hops is not None and g.hops_have_classes and not g.hops_inline_rpos
    # the kernel itself, handed N2V_HOPS_INLINE_RPOS on this graph: N2V_ST_RANGE and nothing else
    cs = g.c_struct()
    assert cs.reserved2 == 0
    cs.reserved2 = 1  # N2V_HOPS_INLINE_RPOS
    hops = torch.empty((g.n_edges, 4), dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = _lib.load().n2v_hops_build(cs, hops.data_ptr(), status.data_ptr(), _lib.current_stream_ptr())
    assert rc == _lib.OK
    torch.cuda.synchronize()
    assert int(status[0].item()) == _lib.ST_RANGE
    # ... and handed the same flag on `below` it raises nothing
    b = _graph("below")
    b.build_wedges()
    cs = b.c_struct()
    cs.reserved2 = 1
    hops = torch.empty((b.n_edges, 4), dtype=torch.int32, device="cuda")
    status.zero_()
    assert _lib.load().n2v_hops_build(cs, hops.data_ptr(), status.data_ptr(), _lib.current_stream_ptr()) == _lib.OK
    torch.cuda.synchronize()
    assert int(status[0].item()) == 0


def test_saturated_declines_the_lists():
    from node2vec_amd import randomwalk as rw

    g = _graph("saturated")
    g.build_wedges()
    assert g.edge_classes is not None
    assert g.wedge_off is None and g.wedge_pos is None and g.wedge_slots is None
    assert not g.can_inline_rpos()
    for name in R.WEIGHTED:
        t = _graph(name)
        assert not t.unit_weights
        assert rw.weighted_lanes_tables(t, insist=True) is False
        assert t.edge_classes is not None and t.wedge_off is None and t.wedge_pos is None and t.wedge_slots is None


# ------------------------------------------------------------------------ 3. the walks of every dispatch
@pytest.mark.parametrize("fname", list(FLAGS))
@pytest.mark.parametrize("name", R.UNIT)
def test_exact_walks_equal_the_oracle_on_every_dispatch(oracle, name, fname):
    flags = FLAGS[fname]
    g = _graph(name, fname)
    start = _start(g)
    for pq in R.PQ:
        want = R.oracle_walks(oracle, name, pq)
        walks, valid, _ = _walk(g, start, pq, **flags)
        _assert_tables(g, name, flags)
        _assert_equal((walks, valid), want, (name, fname, pq))


@pytest.mark.parametrize("fname", list(WEIGHTED_FLAGS))
@pytest.mark.parametrize("name", R.WEIGHTED)
def test_weighted_exact_walks_fall_back_to_the_wave_kernel(oracle, name, fname):
    flags = WEIGHTED_FLAGS[fname]
    g = _graph(name, fname)
    start = _start(g)
    assert g.w.dtype == (torch.float32 if name == "saturated_w32" else torch.float64)
    for pq in R.PQ:
        want = R.oracle_walks(oracle, name, pq)
        walks, valid, stats = _walk(g, start, pq, **flags)  # (must not raise)
        assert "undecided" not in stats  # not the step-synchronous form: it would not step a walker here
        classes = flags.get("use_edge_classes", True)
        assert (g.edge_classes is not None) == classes and g.wedge_tried == classes
        assert g.wedge_off is None and g.wedge_pos is None and g.hops is None
        _assert_equal((walks, valid), want, (name, fname, pq))


@pytest.mark.parametrize("name", R.UNIT + R.WEIGHTED)
def test_shards_of_the_start_list_give_the_same_rows(oracle, name):
    g = _graph(name, "default")
    start = _start(g)
    cuts = [0, 1, 100, start.numel()]
    for pq in R.PQ:
        want = R.oracle_walks(oracle, name, pq)
        parts = [_walk(g, start[a:b].contiguous(), pq)[:2] for a, b in zip(cuts[:-1], cuts[1:])]
        walks, valid = torch.cat([w for w, _ in parts]), torch.cat([v for _, v in parts])
        _assert_equal((walks, valid), want, (name, pq))


# ------------------------------------------------------------------------------ 4. the partitioned walker
@pytest.mark.parametrize("n_parts", sorted(R.PART_ORDERS))
def test_partitioned_walks_with_a_cut_inside_the_saturated_gadget(oracle, n_parts):
    from node2vec_amd import partitioned as P
    from test_partitioned_gpu import _walk_all_routings

    name = "saturated_parts%d" % n_parts
    g = _graph(name)
    parts = P.partition_graph(g, n_parts)
    assert len(parts) == n_parts and [pt.lo for pt in parts[1:]] == R.part_cuts(name, n_parts)
    x = next(x for x in R.graphs()[name]["gadgets"] if x["m"] == 300)
    assert sum(x["s"] < pt.lo <= x["v"] for pt in parts) == 1  # s in one part, v in the next
    # one saturated count: no part has lists, whole rows travel with the walkers
    assert all(pt.wedge_off is None and pt.wedge_pos is None and pt.edge_classes is None for pt in parts)
    start = _start(g)
    for pq in ((0.5, 2.0), (3.0, 0.7)):
        want, wv, _ = _walk(g, start, pq)
        _assert_equal((want, wv), R.oracle_walks(oracle, name, pq), (name, pq))
        _walk_all_routings(P, parts, start, R.NUM_WALKS, R.WALK_LENGTH, pq[0], pq[1], R.SEED, want, wv)


@pytest.mark.parametrize("n_parts", [2, 3])
def test_partitioned_walks_keep_their_lists_below_saturation(oracle, n_parts):
    from node2vec_amd import partitioned as P
    from test_partitioned_gpu import _walk_all_routings

    g = _graph("inline_limit")
    parts = P.partition_graph(g, n_parts)
    assert all(pt.wedge_off is not None and pt.wedge_pos is not None and pt.edge_classes is not None
               and pt.wedge_off.numel() == pt.col.numel() > 0 for pt in parts)
    top = max(int((pt.edge_classes >> 24 & 0xff).max()) for pt in parts)
    assert top == 129
    start = _start(g)
    for pq in ((0.5, 2.0), (3.0, 0.7)):
        want, wv, _ = _walk(g, start, pq)
        _assert_equal((want, wv), R.oracle_walks(oracle, "inline_limit", pq), pq)
        assert P._forward_mode(parts, pq[0], pq[1], P.hip_step) == 2  # the lists travel
        _walk_all_routings(P, parts, start, R.NUM_WALKS, R.WALK_LENGTH, pq[0], pq[1], R.SEED, want, wv)


# --------------------------------------------------------------------------------------- 5. fast mode
def test_fast_walks_on_inline_limit_do_not_depend_on_the_hop_table():
    from node2vec_amd import randomwalk as rw

    g = _graph("inline_limit")
    start = _start(g)
    a, av = rw.walk(g, start, R.NUM_WALKS, R.WALK_LENGTH, 0.5, 2.0, R.SEED, mode="fast")
    assert g.hops is not None and not g.hops_inline_rpos
    b, bv = rw.walk(_graph("inline_limit"), start, R.NUM_WALKS, R.WALK_LENGTH, 0.5, 2.0, R.SEED, mode="fast",
                    use_hops=False)
    assert torch.equal(a, b) and torch.equal(av, bv) and bool(av.all())
