"""The cases of fast_law_cases.py are what they claim, their law is the oracle's, and the statistic of
test_fast_law_gpu.py has the power to see the seven ways this sampler could be wrong -- all on the CPU.

Structure: plain Python set arithmetic on the CSR that the GPU test builds (DeviceGraph.from_edges, here on
the CPU, equals the numpy restatement).  Law: the closed-form law of every context equals
oracle.transition_probs to 1e-12.  Conditions of the statistic, checked on the reference law alone for the
walker count of the GPU test: >= 20 000 expected arrivals, every pooled cell expected >= 5 times (so no cell is
ever left out).  Power: under each analytic mutant law the statistic's expected z is >= 10 (twice the
threshold) on at least one context and (p, q)."""
import numpy as np
import pytest

import fast_law_cases as F

GRAPHS = F.graphs()
CONTEXTS = F.contexts()


def _csr(ctx):
    return F.csr(GRAPHS[ctx["graph"]])


@pytest.mark.parametrize("name", list(GRAPHS))
def test_numpy_csr_is_the_csr_of_from_edges(name):
    import torch

    from node2vec_amd.graph import DeviceGraph

    g = GRAPHS[name]
    rowptr, col, w = F.csr(g)
    d = DeviceGraph.from_edges(g["src"], g["dst"], None if g["weight"] is None else torch.from_numpy(g["weight"]),
                               device="cpu")
    assert np.array_equal(d.rowptr.numpy(), rowptr) and np.array_equal(d.col.numpy(), col)
    assert d.unit_weights == (w is None)
    if w is not None:
        assert d.w.numpy().dtype == w.dtype and np.array_equal(d.w.numpy(), w)
    # a few hundred vertices, around a thousand directed edges; every vertex has an out-edge (no walker vanishes)
    assert 50 <= g["n_vertices"] <= 600 and 700 <= col.size <= 5000
    assert (np.diff(rowptr) > 0).all()


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_context_structure(name):
    ctx = CONTEXTS[name]
    rowptr, col, w = _csr(ctx)
    s, v = ctx["s"], ctx["v"]
    row_v = [int(x) for x in col[rowptr[v]:rowptr[v + 1]]]
    row_s = [int(x) for x in col[rowptr[s]:rowptr[s + 1]]]
    set_s = set(row_s)
    ret = [i for i, x in enumerate(row_v) if x == s]
    shared = [i for i, x in enumerate(row_v) if x != s and x in set_s]
    assert len(row_v) == ctx["deg_v"] and len(row_s) == ctx["deg_s"]
    assert len(ret) == ctx["nR"] and ret == list(range(ctx["rpos"], ctx["rpos"] + ctx["nR"]))
    assert shared == ctx["shared_pos"] and len(shared) == ctx["shared"]
    assert row_v == [int(x) for x in ctx["slot_ids"]]
    assert [0 if i in ret else 1 if i in shared else 2 for i in range(len(row_v))] == list(ctx["slot_cls"])
    if w is not None:
        assert np.array_equal(w[rowptr[v]:rowptr[v + 1]].astype(np.float64),
                              ctx["slot_w"].astype(w.dtype).astype(np.float64))
    assert abs(row_s.count(v) / len(row_s) - ctx["arrive"]) < 1e-15  # (every weight out of s is 1)
    assert w is None or (w[rowptr[s]:rowptr[s + 1]] == 1.0).all()
    assert [row_s.index(x) for x in sorted({row_v[i] for i in shared})] == ctx["s_pos_shared"]


def test_required_shapes():
    c = CONTEXTS
    x = c["short_list"]
    assert 1 <= x["shared"] <= 14 and x["nR"] == 3 and 0 < x["rpos"] and x["rpos"] + 3 < x["deg_v"]
    assert x["deg_v"] < F.WIDE_FROM  # the narrow twin on the mixed table
    x = c["long_list"]
    assert x["shared"] >= 40 and x["deg_v"] >= 120 and x["deg_s"] >= 64 and x["nR"] > 1
    assert x["deg_v"] >= F.WIDE_FROM and x["rpos"] >= F.WIDE_FROM  # wide_row
    assert sum(p >= F.WIDE_FROM for p in x["shared_pos"]) >= 1 and sum(p < F.WIDE_FROM for p in x["shared_pos"]) >= 1
    x = c["no_shared"]
    assert x["shared"] == 0 and x["nR"] == 2 and x["deg_v"] >= 64 and x["rpos"] > 0
    assert x["nR"] < 128  # the inline form holds 7 bits of return count
    x = c["saturated_return"]
    assert x["nR"] == 300 > 255 and round(x["arrive"] * x["deg_s"]) == 300  # both bundles
    assert x["deg_v"] - 300 >= 40 and x["shared"] > 0
    assert sorted((c[n]["deg_v"], c[n]["nR"]) for n in c if n.startswith("low_degree")) \
        == [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2)]
    for n in ["pivoted"] + [n for n in c if "_heavy_" in n]:
        x = c[n]
        rowptr, _, _ = _csr(x)
        first, last = int(rowptr[x["s"]]), int(rowptr[x["s"] + 1])
        assert x["deg_s"] >= 100 and first % 32 == x["align"] != 0 and last % 32 != 0
        blocks = sorted({(first + i) // 32 for i in x["s_pos_shared"]})
        assert blocks[0] == first // 32 and blocks[-1] == (last - 1) // 32
        assert any(first // 32 < b < (last - 1) // 32 for b in blocks)
    for gname, dtype in (("weighted32", np.float32), ("weighted64", np.float64)):
        w = GRAPHS[gname]["weight"]
        assert w.dtype == dtype
        if dtype == np.float64:
            assert (w.astype(np.float32).astype(np.float64) != w).any()
        for heavy, cls in (("return", F.RET), ("shared", F.SHARED), ("other", F.OTHER)):
            x = c["%s_heavy_%s" % (gname, heavy)]
            assert x["deg_v"] >= 100 and x["slot_cls"][int(np.argmax(x["slot_w"]))] == cls
            assert (x["slot_w"] == 0.0).sum() == 1
            ids, cnt = np.unique(x["slot_ids"], return_counts=True)
            par = [x["slot_w"][x["slot_ids"] == i] for i in ids[cnt > 1] if i != x["s"]]
            assert len(par) >= 3 and all(np.unique(p).size > 1 for p in par)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_law_equals_the_oracle(oracle, name):
    ctx = CONTEXTS[name]
    rowptr, col, w = _csr(ctx)
    ow = np.ones(col.size, np.float32) if w is None else w
    for p, q in F.PQ:
        nb, cls, pr = F.csr_law(rowptr, col, w, ctx["s"], ctx["v"], p, q)
        ref = oracle.transition_probs(rowptr, col, ow, ctx["s"], ctx["v"], p, q)
        assert np.abs(pr - ref).max() <= 1e-12
        ids, cid, pv, mass = F.context_law(ctx, p, q)
        i2, c2, p2 = F.pool(nb, cls, pr)
        assert np.array_equal(ids, i2) and np.array_equal(cid, c2) and np.abs(pv - p2).max() <= 1e-12
        assert abs(mass.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_conditions_of_the_statistic(name):
    ctx = CONTEXTS[name]
    n = F.NUM_WALKS * ctx["arrive"]
    assert n >= 20000
    for p, q in F.PQ:
        _, _, pv, _ = F.context_law(ctx, p, q)
        assert (n * pv).min() >= 5.0  # every cell: nothing is ever left out of a row


def test_every_graph_sums_enough_degrees_of_freedom():
    for g in GRAPHS.values():
        assert sum(np.unique(c["slot_ids"]).size - 1 for c in g["contexts"].values()) >= F.MIN_DOF


def _power(kind):
    best = (0.0, None)
    for name, ctx in CONTEXTS.items():
        for p, q in F.PQ:
            pm = F.mutant_law(kind, ctx, p, q, wide_from=F.WIDE_FROM)
            if pm is None:
                continue
            z = F.expected_z(ctx, p, q, pm, F.NUM_WALKS * ctx["arrive"])
            for stat, val in z.items():
                if val > best[0]:
                    best = (val, (name, (p, q), stat))
    return best


@pytest.mark.parametrize("kind", list(F.MUTANTS))
def test_power_against_mutant(kind):
    z, where = _power(kind)
    print(kind, F.MUTANTS[kind], "expected z %.1f at %s" % (z, where))
    assert z >= 10.0, (kind, z, where)


def test_low_degree_keeps_its_power_against_the_round_2_error():
    """degree 2 at p = 0.5, q = 2: 0.8 -> 0.889 (the figure of test_fast_unit_gpu.py)"""
    ctx = CONTEXTS["low_degree_2_1"]
    pm = F.mutant_law("a", ctx, 0.5, 2.0)
    assert abs(pm[ctx["slot_cls"] == F.RET].sum() - 8.0 / 9.0) < 1e-12
    assert F.expected_z(ctx, 0.5, 2.0, pm, F.NUM_WALKS * ctx["arrive"])["share"] >= 10.0


def test_a_sample_of_the_reference_law_passes():
    rng = np.random.default_rng(20240607)
    for g in GRAPHS.values():
        for p, q in F.PQ:
            stats = {}
            for name, ctx in g["contexts"].items():
                _, cid, pv, _ = F.context_law(ctx, p, q)
                n = rng.binomial(F.NUM_WALKS, ctx["arrive"])
                stats[name] = F.statistic(rng.multinomial(n, pv), cid, pv)
            assert F.failures(stats) == [], F.report(stats)


def test_the_statistic_sees_a_mutant_sample():
    """the same draw from mutant (b) on the long list: the statistic must fail"""
    rng = np.random.default_rng(7)
    ctx = CONTEXTS["long_list"]
    _, cid, pv, _ = F.context_law(ctx, 0.5, 2.0)
    _, _, pm = F.pool(ctx["slot_ids"], ctx["slot_cls"], F.mutant_law("b", ctx, 0.5, 2.0))
    st = F.statistic(rng.multinomial(int(F.NUM_WALKS * ctx["arrive"]), pm), cid, pv)
    assert F.failures({"long_list": st}) != []
