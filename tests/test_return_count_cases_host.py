"""The graphs of return_count_cases.py are what they claim, and the oracle's walks with the parameters of
test_return_count_limits_gpu.py draw from every gadget's table often enough -- all on the CPU.

Structure: plain Python counts on the CSR that the GPU test builds (DeviceGraph.from_edges, here on the CPU, equals
the numpy restatement).  Conditions on the inputs, checked on the reference alone: at every gadget and every (p, q)
at least 100 steps are taken from v with previous vertex s, at least 20 of them back to s and at least 20 to a leaf of
v alone.  Measured with this seed, the smallest figures over all gadgets, graphs and (p, q): 764 such steps (813 on
the weighted twins), 107 back to s, 57 to a leaf of v alone.  Should another seed miss a floor, choose another seed."""
import numpy as np
import pytest

import return_count_cases as R

GRAPHS = R.graphs()
MIN_STEPS, MIN_RETURNS, MIN_OTHERS = 100, 20, 20


@pytest.mark.parametrize("name", list(GRAPHS))
def test_numpy_csr_is_the_csr_of_from_edges(name):
    import torch

    from node2vec_amd.graph import DeviceGraph

    g = GRAPHS[name]
    rowptr, col, w = R.csr(name)
    d = DeviceGraph.from_edges(g["src"], g["dst"], None if g["weight"] is None else torch.from_numpy(g["weight"]),
                               device="cpu")
    assert np.array_equal(d.rowptr.numpy(), rowptr) and np.array_equal(d.col.numpy(), col)
    assert d.unit_weights == (w is None)
    if w is not None:
        assert d.w.numpy().dtype == w.dtype and np.array_equal(d.w.numpy(), w)
    assert (np.diff(rowptr) > 0).all()  # every vertex has an out-edge: no walker vanishes
    edges = set(zip(g["src"].tolist(), g["dst"].tolist()))
    assert all((b, a) in edges for a, b in edges)  # every edge runs both ways


def test_sizes():
    for name, mults in R.MULTS.items():
        g = GRAPHS[name]
        assert [x["m"] for x in g["gadgets"]] == list(mults)
        assert g["n_vertices"] == 47 * len(mults) and all(x["end"] - x["base"] == 47 for x in g["gadgets"])
        assert g["src"].size == sum(2 * m + 100 for m in mults)
    g = GRAPHS["saturated"]
    assert g["n_vertices"] == 376 and g["src"].size == 3950
    for n, order in R.PART_ORDERS.items():
        assert sorted(order) == sorted(R.MULTS["saturated"])
        assert GRAPHS["saturated_parts%d" % n]["src"].size == 3950


@pytest.mark.parametrize("name", list(GRAPHS))
def test_gadget_structure(name):
    rowptr, col, w = R.csr(name)
    n_ret, n_shared = R.edge_counts(name)
    hub = name == "hubs"
    for k, x in enumerate(GRAPHS[name]["gadgets"]):
        s, v, m = x["s"], x["v"], x["m"]
        row_s = col[rowptr[s]:rowptr[s + 1]].tolist()
        row_v = col[rowptr[v]:rowptr[v + 1]].tolist()
        extra_m, extra_a = R.HUBS[k][1:] if hub else (0, 0)
        assert row_s.count(v) == m and row_v.count(s) == m
        assert len(x["shared"]) == 3 + extra_m and len(x["s_only"]) == 2 + extra_a and len(x["v_only"]) == 40
        assert sorted(set(row_s) - {v}) == sorted(x["shared"].tolist() + x["s_only"].tolist())
        assert sorted(set(row_v) - {s}) == sorted(x["shared"].tolist() + x["v_only"].tolist())
        assert len(row_s) == m + 5 + extra_m + extra_a and len(row_v) == m + 3 + extra_m + 39 + 5
        assert row_v.count(x["five_fold"]) == 5 and x["five_fold"] in x["v_only"]  # a multi-edge among the other slots
        assert col[rowptr[x["five_fold"]]:rowptr[x["five_fold"] + 1]].tolist() == [v]
        # the runs lie inside their rows: slots of other classes in front of them and behind them
        assert 0 < row_v.index(s) and row_v.index(s) + m < len(row_v)
        assert 0 < row_s.index(v) and row_s.index(v) + m < len(row_s)
        # the plain count per edge: m for every edge of both bundles, 3 shared slots
        for a, b in ((s, v), (v, s)):
            e0 = R.edge_index(name, a, b)
            assert (n_ret[e0:e0 + m] == m).all() and (n_shared[e0:e0 + m] == 3 + extra_m).all()
            assert (col[e0:e0 + m] == b).all()
        if w is not None:
            for a, b in ((s, v), (v, s), (v, x["five_fold"])):
                e0 = R.edge_index(name, a, b)
                ww = w[e0:e0 + (5 if b == x["five_fold"] else m)].astype(np.float64)
                assert np.unique(ww).size == 5  # parallel edges of different weights
                assert any(np.frexp(t)[0] != 0.5 for t in ww)  # one of them no power of two
    # no count beyond a bundle's reaches a limit
    big = n_ret >= 100
    assert sorted(set(n_ret[big].tolist())) == sorted({x["m"] for x in GRAPHS[name]["gadgets"]})


def test_the_graphs_straddle_the_limits():
    top = {name: int(R.edge_counts(name)[0].max()) for name in GRAPHS}
    assert top["below"] == R.INLINE_LIMIT - 1
    assert R.INLINE_LIMIT <= top["inline_limit"] < R.RETURN_SAT
    for name in ("saturated", "saturated_w32", "saturated_w64", "saturated_parts2", "saturated_parts3", "hubs"):
        assert top[name] == 300
    for name in ("saturated", "hubs"):
        ms = {x["m"] for x in GRAPHS[name]["gadgets"]}
        assert {254, 255, 300} <= ms  # the last exact count, the first that saturates, one far beyond
    words = R.class_words("saturated")
    n_ret = R.edge_counts("saturated")[0]
    assert set((words[n_ret >= 255] >> 24).tolist()) == {255} and set((words[n_ret == 254] >> 24).tolist()) == {254}
    w32, w64 = GRAPHS["saturated_w32"]["weight"], GRAPHS["saturated_w64"]["weight"]
    assert w32.dtype == np.float32 and w64.dtype == np.float64
    assert (w64.astype(np.float32).astype(np.float64) != w64).all()
    for name in R.WEIGHTED:  # the twins: the ids of saturated
        assert np.array_equal(R.csr(name)[1], R.csr("saturated")[1])


def test_the_hub_instance_reaches_the_wave_path_in_both_directions():
    """classes_wave runs when the shorter of N(a), N(b) has more than kLaneMax entries, and searches N(b) in N(a)
    (len N(b) <= len N(a)) or the other way round: a bundle whose count saturates, and one that stays at 254, is
    seen by both branches"""
    rowptr, col, _ = R.csr("hubs")
    deg = np.diff(rowptr)
    n_ret = R.edge_counts("hubs")[0]
    src = np.repeat(np.arange(deg.size), deg)
    wave = np.minimum(deg[src], deg[col]) > R.LANE_MAX
    first = deg[col] <= deg[src]
    for want in (254, 255, 300):
        at = n_ret == want
        assert wave[at].all() and first[at].any() and (~first[at]).any(), want
    for x, (m, extra_m, extra_a) in zip(GRAPHS["hubs"]["gadgets"], R.HUBS):
        assert (deg[x["s"]] > deg[x["v"]]) == (extra_a > 0) and min(deg[x["s"]], deg[x["v"]]) > 64


@pytest.mark.parametrize("n_parts", sorted(R.PART_ORDERS))
def test_a_cut_falls_inside_the_300_fold_gadget(n_parts):
    name = "saturated_parts%d" % n_parts
    x = next(x for x in GRAPHS[name]["gadgets"] if x["m"] == 300)
    cuts = R.part_cuts(name, n_parts)
    assert len(cuts) == n_parts - 1 and cuts == sorted(set(cuts)) and 0 < cuts[0] and cuts[-1] < 376
    assert sum(x["s"] < c <= x["v"] for c in cuts) == 1  # s in one part, v in the next


@pytest.mark.parametrize("name", R.UNIT + R.WEIGHTED)
def test_the_oracle_draws_from_every_gadgets_table(oracle, name):
    low = []
    for pq in R.PQ:
        walks, valid = R.oracle_walks(oracle, name, pq)
        assert valid.all() and walks.shape == (GRAPHS[name]["n_vertices"] * R.NUM_WALKS, R.WALK_LENGTH + 1)
        for x in GRAPHS[name]["gadgets"]:
            steps, returns, others = R.context_steps(walks, x)
            low.append((steps, returns, others))
            assert steps >= MIN_STEPS and returns >= MIN_RETURNS and others >= MIN_OTHERS, (pq, x["m"], steps,
                                                                                           returns, others)
    print(name, "smallest: steps %d returns %d others %d" % tuple(np.array(low).min(axis=0)))
