"""Fast-mode walks against the exact transition law on every sampler path of walk_fast_kernel.

For each context (s, v) of fast_law_cases.py: 2^20 walkers start at s with walk_length = 2 and mode="fast"; the
ones whose first step went to v are kept, and their second step is compared with the law of
generate_edge_alias_tables (w * (1/p | 1 | 1/q), normalised; fast_law_cases.context_law, equal to the oracle by
test_fast_law_host.py).  Statistic and thresholds: fast_law_cases.statistic / failures -- the three class
masses within 5 binomial sigma, the chi-square over the pooled cells of the row and the chi-square of
proportionality to w inside each class as z < 4.5.  The random numbers are counter-based: an outcome is a fixed
function of the seed, so a failure repeats and is a finding.

Which path a context takes is a matter of the tables; every test asserts from the graph's state that the tables
it was written for are the ones the launch saw.
"""
import numpy as np
import pytest
import torch

import fast_law_cases as F
from test_fast_unit_gpu import TABLES

pytestmark = pytest.mark.gpu

# name: (TABLES entry, how the wedge table is built, further flags of walk())
SETS = {name: (name, None, {}) for name in TABLES}
SETS.update({
    "wedges, no slots": ("hops+classes+wedges", None, {"use_wedge_slots": False}),
    "wedges, no inline rpos": ("hops+classes+wedges", None, {"use_inline_rpos": False}),
    "mixed: hops+classes+wedges": ("hops+classes+wedges", "mixed", {}),
    "mixed: classes+wedges": ("classes+wedges", "mixed", {}),
    "mixed: wedges, no slots": ("hops+classes+wedges", "mixed", {"use_wedge_slots": False}),
    "wide: hops+classes+wedges": ("hops+classes+wedges", "wide", {}),
    "wide: classes+wedges": ("classes+wedges", "wide", {}),
})
GRAPH_SETS = ([("main", s) for s in SETS] + [("saturated", s) for s in TABLES]
              + [("weighted32", "alias"), ("weighted64", "alias")])
SEED = 20240611
_CACHE = {}


def _graph(gname, sname, fresh=False):
    """the DeviceGraph of (graph, table set): built once, its tables with it"""
    from node2vec_amd.graph import DeviceGraph

    if fresh or (gname, sname) not in _CACHE:
        c = F.graphs()[gname]
        w = None if c["weight"] is None else torch.from_numpy(c["weight"])
        g = DeviceGraph.from_edges(c["src"], c["dst"], w, device="cuda")
        assert g.unit_weights == (w is None)
        if sname != "alias" and TABLES[SETS[sname][0]][2]:
            how = SETS[sname][1]
            g.build_edge_classes()
            if how == "mixed":
                g.build_wedges(wide_from=F.WIDE_FROM)
            elif how == "wide":
                g.build_wedges(wide=True)
            else:
                g.build_wedges()
        if fresh:
            return g
        _CACHE[(gname, sname)] = g
    return _CACHE[(gname, sname)]


def _flags(sname):
    if sname == "alias":
        return {}
    classes, hops, wedges = TABLES[SETS[sname][0]]
    return dict(use_edge_classes=classes, use_hops=hops, use_wedges=wedges, **SETS[sname][2])


def _assert_path(g, gname, sname):
    """the tables the launch saw are the ones this set stands for (after the first walk: they are built on use)"""
    if sname == "alias":
        want = torch.float32 if gname == "weighted32" else torch.float64
        assert not g.unit_weights and g.slots is not None and g.pivots is not None and g.w.dtype == want
        return
    classes, hops, wedges = TABLES[SETS[sname][0]]
    how, extra = SETS[sname][1], SETS[sname][2]
    assert g.unit_weights and g.pivots is not None
    assert (g.hops is not None) == hops
    if gname == "saturated":
        ctx = F.contexts()["saturated_return"]
        if g.edge_classes is None:
            g.build_edge_classes()  # (bare: the launch did not see them; the count is read for the record)
        row = g.col[int(g.rowptr[ctx["s"]]):int(g.rowptr[ctx["s"] + 1])]
        e = int(g.rowptr[ctx["s"]]) + int((row == ctx["v"]).nonzero()[0])
        assert (int(g.edge_classes[e]) >> 24) & 0xff == 255  # saturated: the rho fold must stay off
        assert g.wedge_off is None and g.wedge_slots is None  # build_wedges declines the lists: no layers
        return
    if not wedges:
        assert g.wedge_off is None
        return
    assert g.wedge_off is not None and g.edge_classes is not None
    if how == "wide":
        assert g.wedge_mode == 1 and g.wedge_pos.dtype == torch.int32 and g.wedge_slots is None
        assert not g.hops_inline_rpos
    else:
        assert g.wedge_mode == (F.WIDE_FROM if how == "mixed" else 0) and g.wedge_pos.dtype == torch.int16
        assert g.wedge_slots is not None and (how != "mixed" or g.slots_folded)
        if hops:
            assert g.hops_inline_rpos == (not extra)  # either flag off: the plain class words


def _second_steps(g, ctx, p, q, flags):
    from node2vec_amd import randomwalk as rw

    start = torch.tensor([ctx["s"]], dtype=torch.int32, device="cuda")
    walks, valid = rw.walk(g, start, F.NUM_WALKS, 2, p, q, SEED, mode="fast", **flags)
    assert bool(valid.all())
    nxt = walks[walks[:, 1] == ctx["v"], 2].long()
    return torch.bincount(nxt, minlength=g.n_vertices).cpu().numpy()


@pytest.mark.statistical
@pytest.mark.parametrize("pq", F.PQ, ids=lambda pq: "p%g-q%g" % pq)
@pytest.mark.parametrize("gname,sname", GRAPH_SETS)
def test_second_step_follows_the_law(gname, sname, pq):
    p, q = pq
    g = _graph(gname, sname)
    stats = {}
    for name, ctx in F.graphs()[gname]["contexts"].items():
        counts = _second_steps(g, ctx, p, q, _flags(sname))
        ids, cid, pv, _ = F.context_law(ctx, p, q)
        obs = counts[ids]
        assert obs.sum() == counts.sum(), name  # every second step is a neighbour of v
        assert abs(obs.sum() - F.NUM_WALKS * ctx["arrive"]) < 6 * np.sqrt(F.NUM_WALKS * ctx["arrive"]), name
        stats[name] = F.statistic(obs, cid, pv)
    _assert_path(g, gname, sname)
    print(F.report(stats))
    assert F.failures(stats) == [], (gname, sname, pq, F.failures(stats))


THIRD = [("main", "long_list", s) for s in ("hops+classes", "hops+classes+wedges", "classes+wedges",
                                            "wedges, no slots", "mixed: hops+classes+wedges",
                                            "mixed: wedges, no slots", "wide: hops+classes+wedges")]
THIRD += [("weighted32", "weighted32_heavy_return", "alias"), ("weighted64", "weighted64_heavy_return", "alias")]


@pytest.mark.statistical
@pytest.mark.parametrize("pq", [(0.5, 2.0), (2.0, 0.5), (3.0, 0.7)], ids=lambda pq: "p%g-q%g" % pq)
@pytest.mark.parametrize("gname,cname,sname", THIRD)
def test_third_step_follows_the_law(gname, cname, sname, pq):
    """walk_length = 3 from s: the law of the third step given (path[1], path[2]), over all contexts with at
    least 400 samples -- the state a step hands to the next (e_prev, hop row and degree, class word).  One of
    the contexts is (v, s), entered by a RETURN step: the edge (v -> s) found by lower_bound_lane after a
    folded return, and its hop entry, feed the step that is measured.  Pooling as in
    test_unit_fast_transition_distribution."""
    from node2vec_amd import randomwalk as rw

    p, q = pq
    g = _graph(gname, sname)
    ctx = F.contexts()[cname]
    rowptr, col, w = F.csr(F.graphs()[gname])
    nv = g.n_vertices
    start = torch.tensor([ctx["s"]], dtype=torch.int32, device="cuda")
    walks, valid = rw.walk(g, start, F.NUM_WALKS, 3, p, q, SEED + 1, mode="fast", **_flags(sname))
    assert bool(valid.all())
    _assert_path(g, gname, sname)
    wl = walks.long()
    key, cnt = torch.unique((wl[:, 1] * nv + wl[:, 2]) * nv + wl[:, 3], return_counts=True)
    key, cnt = key.cpu().numpy(), cnt.cpu().numpy()
    pair = key // nv
    cuts = np.flatnonzero(np.diff(pair)) + 1
    chi2, dof, seen = 0.0, 0, set()
    ret_obs, ret_exp, ret_var = {}, {}, {}
    for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, key.size]):
        n = int(cnt[lo:hi].sum())
        if n < 400:
            continue
        s2, v2 = divmod(int(pair[lo]), nv)
        seen.add((s2, v2))
        ids, cid, pv = F.pool(*F.csr_law(rowptr, col, w, s2, v2, p, q))
        obs = np.zeros(ids.size)
        at = np.searchsorted(ids, key[lo:hi] % nv)
        assert (ids[np.minimum(at, ids.size - 1)] == key[lo:hi] % nv).all()  # every hop is an edge
        obs[at] = cnt[lo:hi]
        exp = pv * n
        ok = exp >= 5
        if ok.sum() >= 2:
            chi2 += (((obs - exp) ** 2) / np.maximum(exp, 1e-12))[ok].sum()
            dof += int(ok.sum()) - 1
        d = int(rowptr[v2 + 1] - rowptr[v2])
        pret = float(pv[cid == F.RET].sum())
        ret_obs[d] = ret_obs.get(d, 0) + float(obs[cid == F.RET].sum())
        ret_exp[d] = ret_exp.get(d, 0.0) + pret * n
        ret_var[d] = ret_var.get(d, 0.0) + pret * (1 - pret) * n
    assert (ctx["v"], ctx["s"]) in seen  # the context entered by a return step
    assert dof > 60, dof
    z = F.chi_z(chi2, dof)
    print("contexts %d chi2 %.1f dof %d z %.2f" % (len(seen), chi2, dof, z))
    assert z < F.Z_CHI2, (gname, sname, pq, chi2, dof, z)
    for d in ret_obs:
        if ret_var[d] > 0:
            zr = (ret_obs[d] - ret_exp[d]) / np.sqrt(ret_var[d])
            assert abs(zr) < F.Z_SHARE, (gname, sname, pq, "degree", d, ret_obs[d], ret_exp[d], zr)


@pytest.mark.parametrize("gname,sname", GRAPH_SETS)
def test_fast_walks_are_walks_whatever_the_launch(gname, sname):
    """not statistical: fast walks do not depend on how the start list is cut into launches, every hop is an
    edge, and with p = q = 1 they are the exact mode's walks bit for bit"""
    from node2vec_amd import randomwalk as rw

    g = _graph(gname, sname)
    flags = _flags(sname)
    nv = g.n_vertices
    start = rw.start_vertices(g)
    c = F.graphs()[gname]
    edges = np.unique(c["src"] * nv + c["dst"])
    for p, q in ((0.5, 2.0), (2.0, 0.5), (3.0, 0.7)):
        walks, valid = rw.walk(g, start, 5, 12, p, q, 77, mode="fast", **flags)
        assert bool(valid.all())
        parts = [rw.walk(g, part, 5, 12, p, q, 77, mode="fast", **flags)[0] for part in torch.chunk(start, 3)]
        assert torch.equal(torch.cat(parts), walks)
        wk = walks.cpu().numpy().astype(np.int64)
        assert np.isin(wk[:, :-1] * nv + wk[:, 1:], edges).all()
    _assert_path(g, gname, sname)
    fast, fv = rw.walk(g, start, 5, 12, 1.0, 1.0, 77, mode="fast", **flags)
    # (a graph of its own: the exact walk builds the tables IT wants, and the cached graph keeps this set's)
    exact, ev = rw.walk(_graph(gname, sname, fresh=True), start, 5, 12, 1.0, 1.0, 77, mode="exact")
    assert torch.equal(fast, exact) and torch.equal(fv, ev)
