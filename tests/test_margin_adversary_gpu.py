"""Adversarial rows through the HIP kernels: rows whose INTERNAL comparisons -- X_i - k D of the closed forms with
margins (n2v_unit_near.h), E_k - D_j / probs[pick] - 1 of the weighted decision (n2v_walk_wlanes.hip) -- were placed
at 0.01 ... 10 x the margin by exact rational arithmetic (scripts/models/margin_adversary.py), embedded in a graph
and walked.  The Python models of the two procedures pass the same rows on CPU (tests/test_closed_form_models.py);
this is the check that the KERNELS decide as their models do where random graphs never go.

Each row becomes three kinds of vertices: v, whose out-edges are the row (slot i -> vertex base + i; the return run
-> the vertex s, parallel edges); s, with edges to v (parallel ones: half of its walkers go there first)
and to the shared slots' vertices; sinks.  A walk of two steps from s stands on v with prev = s: its second step is a
draw from the table generate_edge_alias_tables builds for (s, N(s), N(v)) (randomwalk.py:193-232).  That table comes
from the oracle once per row; every walker's uniforms from the RNG restated below (pinned by rng_kat.json through
oracle.uniform_bits): the expected vertex of every walker in O(1)."""
import os
import sys

import numpy as np
import pytest
import torch

from step_rows import _Rows, _check_rows, _mix64, _uniform_bits  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "models"))

M64 = (1 << 64) - 1


def test_rng_restatement_equals_the_oracle(oracle):
    keys = np.array([0, 1, 7, 12345, 2 ** 40 + 3, 2 ** 63 + 11], dtype=np.uint64)
    for seed in (0, 42, 2 ** 64 - 5):
        for step in (0, 1, 79):
            u1, u2 = _uniform_bits(seed, keys, step)
            for k, a, b in zip(keys.tolist(), u1.tolist(), u2.tolist()):
                assert oracle.uniform_bits(seed, k, step) == (a, b)


def _near_rows(n_max, per, seed):
    import margin_adversary as A

    got = []
    tot = A.attack_near(n_max, per, seed, out=lambda *_: None, collect=got)
    assert tot[3] == 0  # (the MODEL passes them: tests/test_closed_form_models.py)
    return got


def _weighted_rows(n_max, per, seed):
    import margin_adversary as A

    got = []
    tot = A.attack_weighted(n_max, per, seed, out=lambda *_: None, collect=got)
    assert tot[3] == 0
    return got


def _walkers_for(rows):
    # ~6 walkers on v per slot of the longest row (the placed comparison decides the draws of two or three slots)
    return int(min(max(max(6 * r["n"] / r["to_v"] for r in rows), 4096), 1 << 20))


@pytest.mark.parametrize("slots_kernel", [True, False])
def test_closed_forms_with_margins_on_rows_placed_at_the_margin(oracle, slots_kernel):
    """unit weights, 1/p or 1/q not dyadic: walk_exact_wedge_slots_kernel<2> (and, without the slots, the same forms
    through wedge_off) on rows of 8 ... 10^4 slots in all five class arrangements, the comparison nearest to a tie at
    +-{0.01 ... 10} x the margin of the counts stage or of the exact-sum stage"""
    placed = _near_rows(10_000, 1, 5 if slots_kernel else 6)
    assert len(placed) > 250 and len({r["arr"] for r in placed}) == 5
    L = _Rows()
    for r in placed:
        cls = r["cls"]
        rp = cls.index('R')
        ids = [rp if c == 'R' else i for i, c in enumerate(cls)]
        L.add(ids, None, [i for i, c in enumerate(cls) if c == 'M'], rp,
              dict(info=(r["n"], r["arr"], r["p"], r["q"], r["margin"], round(r["multiple"], 3)), slots=r["slots"],
                   p=r["p"], q=r["q"]))
    g = L.graph(weighted=False)
    assert g.unit_weights
    checked = hits = 0
    for r in L.rows:  # q is the knob of the placement: every row has its own
        c, h = _check_rows(oracle, g, [r], _walkers_for([r]), r["p"], r["q"], 77,
                           {} if slots_kernel else {"use_wedge_slots": False})
        checked, hits = checked + c, hits + h
    assert g.wedge_off is not None and g.wedge_slots is not None  # the kernels with the closed forms did run
    print(f"near rows {len(L.rows)}: {checked} walkers checked on the adversarial rows, {hits} draws of placed slots")
    assert hits > 4 * len(L.rows)


def test_weighted_decision_with_margins_on_rows_placed_at_the_margin(oracle):
    """weighted graphs: n2v_walk_weighted_step (lane kernel below 768 slots, wave kernel and block summaries above,
    second chance, exact kernel) on fp32 / fp64 / 24-decade / integer rows of 8 ... 10^4 slots whose crossing
    E_k - D_j or probs[pick] - 1 sits at +-{0.01 ... 10} x the margin"""
    placed = _weighted_rows(10_000, 1, 9)
    assert len(placed) > 150
    by_size = {}
    for r in placed:
        by_size.setdefault((r["n"], r["kind"] in ("fp32", "integers")), []).append(r)
    checked = hits = undecided = 0
    for (n, grid32), rows in sorted(by_size.items()):
        # one graph per row size and weight grid: the power of two that divides every stored weight is a property of
        # the GRAPH (row_sums[n_vertices]) -- rows of one size share the binade of their small weights
        L = _Rows()
        for r in rows:
            cls = np.asarray(r["cls"])
            rp = int(np.nonzero(cls == 2)[0][0])
            L.add(list(range(n)), r["w"], np.nonzero(cls == 1)[0].tolist(), rp,
                  dict(info=(n, r["kind"], r["where"], r["p"], r["q"], r["exact"], round(r["multiple"], 3)),
                       slots=r["slots"], p=r["p"], q=r["q"]))
        g = L.graph(weighted=True)
        assert not g.unit_weights
        groups = {}
        for r in L.rows:
            groups.setdefault((r["p"], r["q"]), []).append(r)
        for (p, q), rs in sorted(groups.items()):
            st = {}
            c, h = _check_rows(oracle, g, rs, _walkers_for(rs), p, q, 78, {"use_weighted_lanes": True, "stats": st})
            checked, hits = checked + c, hits + h
            assert "undecided" in st  # the step kernels with margins ran
            undecided += int(st["undecided"].item()) if torch.is_tensor(st["undecided"]) else int(st["undecided"])
    print(f"weighted rows {len(placed)}: {checked} walkers checked, {hits} draws of placed slots, "
          f"{undecided} walker-steps left to the exact kernel")
    assert hits > 4 * len(placed)
