"""The dyadic closed forms of the exact step on composed rows, through the HIP kernels.

closed_form_cases.py composes rows cell by cell -- code instance x class arrangement x the cut at 64 slots x the cut
at 14 list entries x ties -- and test_closed_form_cases_host.py proves on the CPU that they lie where they claim and
that the walkers started here draw what decides.  Here every row is embedded in a graph (step_rows.py), walked two
steps, and every walker's second vertex compared with the oracle's table of that row (oracle.edge_alias_tables, built
once per row and (p, q)): equalities, no tolerance.  The same walkers go through every dispatch that reads the forms:

  slots        the default: walk_exact_wedge_slots_kernel, return positions inline in the class words where they fit
  wedge_off    use_wedge_slots=False: walk_exact_wedge_kernel, the lists through wedge_off
  lanes        use_wedge_kernel=False: the lanes kernel of n2v_walk_unit.hip (instance 0), else a wave per walker
  plain rpos   use_inline_rpos=False: the slots kernel with every return position read from the slot
  table-free   use_hops=False, use_edge_classes=False: the classes by search, a wave per walker -- the independent
               third implementation

and after each the tables the launch saw are asserted.  A mixed table WITHOUT folded slots is a sixth case: the
launcher sends it to walk_exact_wedge_kernel although nothing is switched off ("unfolded" below)."""
import numpy as np
import pytest
import torch

import closed_form_cases as C
from step_rows import _check_rows

pytestmark = pytest.mark.gpu

DISPATCHES = [("slots", {}), ("wedge_off", {"use_wedge_slots": False}), ("lanes", {"use_wedge_kernel": False}),
              ("plain rpos", {"use_inline_rpos": False}),
              ("table-free", {"use_hops": False, "use_edge_classes": False})]  # (last: it leaves the hop table alone)
# default flags on a mixed table without folded slots: n2v_walk_wedge_try declines the slots kernel, wedge_off serves
UNFOLDED = [("unfolded, through wedge_off", {})]
WIDE_FROM = 48


def _ids(keys):
    return ["-".join(str(x) for x in k) for k in keys]


def _by_walkers(rows):
    groups = {}
    for r in rows:
        groups.setdefault(r["W"], []).append(r)
    return sorted(groups.items())


def _inline_expected(L):
    """DeviceGraph.can_inline_rpos: every return count of the graph below 128 -- the runs, and the bundles s -> v
    that an edge v -> s looks back on (a row without a run has no such edge)"""
    return max(max(r["cls"].count("R"), r["parallel"]) if "R" in r["cls"] else 0 for r in L.rows) < 128


def _assert_tables(g, name, inline, mode):
    assert g.edge_classes is not None and g.wedge_off is not None and g.wedge_slots is not None
    assert g.wedge_mode == mode
    if name != "table-free":
        assert g.hops is not None and g.hops_have_classes
        assert g.hops_inline_rpos == (inline and name == "slots")


def _walk_rows(oracle, L, g, p, q, dispatches=DISPATCHES, tables=None, mode=0, inline=None):
    """every row, the walkers the host test proved, through every dispatch; -> walkers checked"""
    tables = {} if tables is None else tables
    inline = _inline_expected(L) if inline is None else inline
    checked = 0
    for name, kw in dispatches:
        for W, rows in _by_walkers(L.rows):
            checked += _check_rows(oracle, g, rows, W, p, q, C.SEED, kw, tables)[0]
        _assert_tables(g, name, inline, mode)
    return checked


def _graph(L):
    g = L.graph(weighted=False)
    assert g.unit_weights
    return g


A_KEYS = [("A", pq) for inst in (0, 3, 1) for pq in C.A_PAIRS[inst]]


@pytest.mark.parametrize("key", A_KEYS, ids=_ids([k[1] for k in A_KEYS]))
def test_every_composition_of_two_to_five_slots(oracle, key):
    L = C.layout(*key)
    p, q = key[1]
    assert len(L.rows) == 260 and _inline_expected(L)
    n = _walk_rows(oracle, L, _graph(L), p, q)
    assert n > 5 * 260 * 128


B_KEYS = [("B", pq + (half,)) for pq in C.B_PAIRS for half in ("low", "high")]


@pytest.mark.parametrize("key", B_KEYS, ids=_ids([k[1] for k in B_KEYS]))
def test_rows_at_the_cuts(oracle, key):
    """63 | 64 | 65 slots, 14 | 15 | 16 and 300 list entries, return runs of 0 .. 200 (127 | 128: `low` keeps the inline
    return positions, `high` loses them); then the same graph with the rows of 48 slots and more WIDE: folded slots
    on the rows of 63 .. 400 slots, plain ones below -- and without the fold, where the same default flags reach the
    kernel that reads wedge_off"""
    L = C.layout(*key)
    p, q = key[1][:2]
    assert _inline_expected(L) == (key[1][2] == "low")
    tables = {}
    _walk_rows(oracle, L, _graph(L), p, q, tables=tables)
    g = _graph(L)
    g.build_wedges(wide_from=WIDE_FROM)
    g.wedge_tried = True
    assert g.wedge_mode == WIDE_FROM and g.slots_folded and g.wedge_slots is not None
    _walk_rows(oracle, L, g, p, q, dispatches=DISPATCHES[:2], tables=tables, mode=WIDE_FROM)
    assert g.slots_folded
    g = _graph(L)
    g.build_wedges(wide_from=WIDE_FROM, fold=False)
    g.wedge_tried = True
    assert g.wedge_mode == WIDE_FROM and not g.slots_folded and g.wedge_slots is not None
    _walk_rows(oracle, L, g, p, q, dispatches=UNFOLDED, tables=tables, mode=WIDE_FROM, inline=False)


C_KEYS = [("C", pq) for pq in C.C_PAIRS]


@pytest.mark.parametrize("key", C_KEYS, ids=_ids([k[1] for k in C_KEYS]))
def test_rows_on_which_the_exact_loop_ties(oracle, key):
    """a tie and a tie-free row of <= 64 and of 65 .. 400 slots per cell: the forms must decline the first"""
    L = C.layout(*key)
    p, q = key[1]
    assert {r["tie"] for r in L.rows} == {True, False}
    tables = {}
    _walk_rows(oracle, L, _graph(L), p, q, tables=tables)
    g = _graph(L)
    g.build_wedges(wide_from=WIDE_FROM)
    g.wedge_tried = True
    assert g.wedge_mode == WIDE_FROM and g.slots_folded
    _walk_rows(oracle, L, g, p, q, dispatches=DISPATCHES[:2], tables=tables, mode=WIDE_FROM)
    g = _graph(L)
    g.build_wedges(wide_from=WIDE_FROM, fold=False)
    g.wedge_tried = True
    assert not g.slots_folded
    _walk_rows(oracle, L, g, p, q, dispatches=UNFOLDED, tables=tables, mode=WIDE_FROM, inline=False)


D_KEYS = [("D", pq) for pq in C.D_PAIRS]


@pytest.mark.parametrize("key", D_KEYS, ids=_ids([k[1] for k in D_KEYS]))
def test_long_runs_absorbed_by_one_or_two_slots(oracle, key):
    """4096 and 20 000 slots, class values of 2^-10 and 1024: the run absorption across binades"""
    L = C.layout(*key)
    _walk_rows(oracle, L, _graph(L), *key[1])


E_KEYS = [("E", pq) for pq in C.E_SHORT_PAIRS]


@pytest.mark.parametrize("key", E_KEYS, ids=_ids([k[1] for k in E_KEYS]))
def test_awkward_dyadic_values_on_short_rows(oracle, key):
    """1/p, 1/q of 1 +- 2^-20, 1.5, 0.75: reduced integers near 2^20 in every product of the forms"""
    L = C.layout(*key)
    _walk_rows(oracle, L, _graph(L), *key[1])


G_KEYS = [("Eg", pq) for pq in sorted({g[0] for g in C.E_GUARD})]


@pytest.mark.parametrize("key", G_KEYS, ids=_ids([k[1] for k in G_KEYS]))
def test_awkward_dyadic_values_on_both_sides_of_the_exactness_guard(oracle, key):
    """rows at 0.9 and 1.1 times the length at which dn * isum reaches 2.0e14: the form decides the first (reduced
    integers near 2^20 in every product) and declines the second to the replays"""
    L = C.layout(*key)
    assert len(L.rows) % 2 == 0 and min(r["n"] for r in L.rows) > 9000
    _walk_rows(oracle, L, _graph(L), *key[1])


P_KEYS = [("B", pq + (half,)) for pq in ((0.5, 2.0), (4.0, 2.0)) for half in ("low", "high")]


@pytest.mark.parametrize("key", P_KEYS, ids=_ids([k[1] for k in P_KEYS]))
def test_partitioned_walks_over_the_rows_at_the_cuts(oracle, key):
    """partition_step_wedge_kernel instantiates the same pair_listed: two parts, every routing, row for row the
    single-device walk -- which is checked against the oracle's tables first"""
    from node2vec_amd import partitioned as P
    from node2vec_amd import randomwalk as rw
    from test_partitioned_gpu import _walk_all_routings

    L = C.layout(*key)
    p, q = key[1][:2]
    W = 2048
    g = _graph(L)
    _check_rows(oracle, g, L.rows, W, p, q, C.SEED, {})
    start = torch.tensor(sorted(r["s"] for r in L.rows), dtype=torch.int32, device="cuda")
    want, wv = rw.walk(g, start, W, 2, p, q, C.SEED)
    parts = P.partition_graph(g, 2)
    assert len(parts) == 2 and all(pt.wedge_off is not None and pt.wedge_pos is not None for pt in parts)
    _walk_all_routings(P, parts, start, W, 2, p, q, C.SEED, want, wv)


S_KEYS = B_KEYS  # both halves: `high` has the runs of 128 and 200 and no inline return positions


@pytest.mark.parametrize("key", S_KEYS, ids=_ids([k[1] for k in S_KEYS]))
def test_shards_of_the_start_list_give_the_same_rows(key):
    from node2vec_amd import randomwalk as rw

    L = C.layout(*key)
    p, q = key[1][:2]
    g = _graph(L)
    start = torch.tensor(sorted(r["s"] for r in L.rows), dtype=torch.int32, device="cuda")
    whole, wv = rw.walk(g, start, 1024, 2, p, q, C.SEED)
    assert g.wedge_slots is not None
    odd = min(37, start.numel() - 2) | 1
    assert 1 < odd < start.numel()
    cuts = [0, 1, odd, start.numel()]
    parts = [rw.walk(g, start[a:b].contiguous(), 1024, 2, p, q, C.SEED) for a, b in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(torch.cat([w for w, _ in parts]), whole)
    assert torch.equal(torch.cat([v for _, v in parts]), wv)
    assert int(np.count_nonzero(whole[:, 2].cpu().numpy() >= 0)) > 0
