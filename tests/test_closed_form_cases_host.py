"""The rows of closed_form_cases.py are what they claim (CPU: fractions, numpy, the oracle's CPU library; no kernel).

test_closed_form_rows_gpu.py walks these rows on every dispatch of the exact step and compares every draw with the
oracle's table.  That proves something only if the rows reach the code they are meant for and the walkers draw what
decides: here the cells (instance, arrangement, row size, list class, tie) are counted, the cells that cannot exist
are shown not to, and the draws of the very walkers the GPU test starts (seed and count per row from the case module)
are shown to pick every slot of a short row at least 4 times and to fall on both sides of every probability, and to
reach the return run and the edges of the list on a long row."""
import itertools

import numpy as np
import pytest

import closed_form_cases as C


def _all_rows():
    for key in C.all_keys():
        for r in C.layout(*key).rows:
            yield key, r


def test_pairs_select_the_three_instances():
    for inst, pairs in C.A_PAIRS.items():
        assert [C.instance(p, q) for p, q in pairs] == [inst] * len(pairs)
    assert sorted(C.instance(p, q) for p, q in C.B_PAIRS) == [0, 0, 1, 1, 3, 3]
    assert sorted(C.instance(p, q) for p, q in C.E_PAIRS) == [0, 0, 0, 1, 1, 1, 3, 3, 3]
    assert C.E_SHORT_PAIRS == C.E_PAIRS  # every awkward pair walks short rows
    assert {C.instance(*g[0]) for g in C.E_GUARD} == {0, 1, 3}
    assert sorted(C.instance(p, q) for p, q in C.D_PAIRS) == [0, 1, 1, 3]
    # every pair of every family passes the library's own predicate for dyadic values, the bound 2^31 included:
    # the walk runs the instances 0, 1, 3 of the kernels, not the code for values that are not dyadic
    every = ([pq for v in C.A_PAIRS.values() for pq in v] + C.B_PAIRS + C.C_PAIRS + C.D_PAIRS + C.E_PAIRS
             + [g[0] for g in C.E_GUARD] + [k[1][:2] for k in C.all_keys()])
    for p, q in every:
        assert C.library_dyadic(p) and C.library_dyadic(q), (p, q)
        from node2vec_amd.randomwalk import _dyadic
        assert _dyadic(p) and _dyadic(q), (p, q)
    assert not C.library_dyadic(1.0 / 2048.0) and C.library_dyadic(1.0 / 1536.0)  # (2^31 itself is out)
    for p, q in C.E_PAIRS:  # multiples of 2^-20 that the kernels take for dyadic, and not powers of two
        for v in (1.0 / p, 1.0 / q):
            assert (v * 2.0 ** 20).is_integer() and not np.log2(v).is_integer()


def test_cells_that_cannot_exist_do_not():
    """every count (nR, nM, nO) of up to 40 slots under every pair of the suite: no arrangement in a cell that the
    module declares empty -- and every other (instance, arrangement, list) occurs"""
    pairs = [pq for v in C.A_PAIRS.values() for pq in v] + C.B_PAIRS + C.E_PAIRS + C.D_PAIRS
    seen = set()
    for p, q in pairs:
        inst = C.instance(p, q)
        for n in range(2, 41):
            for nR in range(0, n + 1):
                for nM in range(0, n - nR + 1):
                    cR, cM, cO = C._merged_counts(n, nR, nM, p, q)
                    arr = C.arrangement(cR, cM, cO, p, q)
                    if arr != "none":
                        assert C.no_cell(inst, arr, C.list_class(cM)) is None, (p, q, nR, nM, n, arr)
                        seen.add((inst, arr, C.list_class(cM)))
    want = {c for c in itertools.product((0, 1, 3), range(6), range(3)) if C.no_cell(*c) is None}
    assert seen == want


def test_every_cell_holds_a_tie_and_a_tie_free_row():
    cells = {}
    for _, r in _all_rows():
        if r["cell"][1] != "none":
            cells.setdefault(r["cell"], set()).add(r["tie"])
    for inst, arr, big, lst in itertools.product((0, 1, 3), range(6), (False, True), range(3)):
        if C.no_cell(inst, arr, lst):
            assert (inst, arr, big, lst) not in cells
        else:
            assert cells.get((inst, arr, big, lst)) == {True, False}, (inst, arr, big, lst)


def test_rows_without_a_return_run_in_every_cell_that_can_have_one():
    """arrangements 0, 3, 4, 5 name the return class; 1 and 2 without a list and without a run are "other" slots alone"""
    got = {r["cell"] for _, r in _all_rows() if "R" not in C.effective(r["cls"], r["p"], r["q"])}
    for inst, arr, big, lst in itertools.product((0, 1, 3), (1, 2), (False, True), (1, 2)):
        if not C.no_cell(inst, arr, lst):
            assert (inst, arr, big, lst) in got, (inst, arr, big, lst)
    # and the gadget places the s of such rows on both sides of the row's ids
    sides = {(r["s"] > r["v"]) for _, r in _all_rows() if "R" not in r["cls"]}
    assert sides == {True, False}


def test_family_a_is_every_composition():
    rows = C.family_a()
    assert len(rows) == len(set(rows)) == 9 + 25 + 65 + 161
    for cls in rows:
        r = [i for i, c in enumerate(cls) if c == "R"]
        assert not r or r == list(range(r[0], r[-1] + 1))
    for n in range(2, 6):  # counted another way: a run of length ln at n - ln + 1 places, any subset of the rest
        assert sum(len(c) == n for c in rows) == 2 ** n + sum((n - ln + 1) * 2 ** (n - ln) for ln in range(1, n + 1))


def test_family_b_stands_on_both_sides_of_every_cut():
    for p, q in C.B_PAIRS:
        rows = C.family_b(p, q)
        by_arr = {}
        for cls in rows:
            by_arr.setdefault(C.cell(cls, p, q, tie=False)[0][1], []).append(cls)
        for arr, group in by_arr.items():
            if arr == "none":
                continue
            assert {63, 64, 65} <= {len(c) for c in group}, (p, q, arr)
            lists = {c.count("M") for c in group}
            runs = {c.count("R") for c in group}
            if arr in (0, 3, 4, 5):  # (they need both a list and a run)
                assert {14, 15, 16} <= lists and min(runs) >= 1, (p, q, arr, lists, runs)
            for nM in (14, 15, 16):  # both sides of the list cut wherever the arrangement can have such a list
                if any(C.arrangement(r, nM, 64 - r - nM, p, q) == arr for r in range(0, 64 - nM + 1)):
                    assert nM in lists, (p, q, arr, nM)
            where = set()
            for c in group:
                if "R" in c and len(c) - c.count("R") >= 2:
                    a, b = c.index("R"), c.rindex("R")
                    where.add("first" if a == 0 else ("last" if b == len(c) - 1 else "middle"))
                    if c.count("M") >= 2 and 0 < a and b < len(c) - 1:
                        assert c[a - 1] == "M" and c[b + 1] == "M"  # shared slots directly below and above the run
            if max(runs) > 0:  # (arrangements 1 and 2 of instance 1 leave one of the two classes out)
                assert where == {"first", "middle", "last"}, (p, q, arr, where)
        every = set(rows)
        assert {c.count("M") for c in every} >= set(C.B_LISTS)
        assert {c.count("R") for c in every} >= set(C.B_RUNS)
        assert "R" * 64 in every  # (1ull << nR) - 1 with nR = 64
    arrs = {(C.instance(p, q), C.cell(c, p, q, tie=False)[0][1]) for p, q in C.B_PAIRS for c in C.family_b(p, q)}
    assert arrs >= {(i, a) for i in (0, 1, 3) for a in range(6) if not C.no_cell(i, a, 1)}


def test_family_c_ties_on_long_rows():
    for (inst, arr, big, lst), by_tie in C.family_c().items():
        for tie, (cls, p, q) in by_tie.items():
            assert C.cell(cls, p, q) == ((inst, arr, big, lst), tie)
            assert (len(cls) > 64) == big and len(cls) <= 400


def test_family_d_absorbs_thousands():
    for p, q in C.D_PAIRS:
        rows = C.family_d(p, q)
        assert {len(c) for c in rows} == {4096, 20000}
        assert {C.cell(c, p, q, tie=False)[0][1] for c in rows} <= {1, 2}
    few = 0
    for p, q in C.D_PAIRS:
        for cls in C.family_d(p, q):
            eff = C.effective(cls, p, q)
            _, probs = C.float_tables(eff, p, q)
            start = np.array([{"R": 1.0 / p, "M": 1.0, "O": 1.0 / q}[c] for c in eff])
            over = start >= start.mean()
            if over.sum() <= 2:
                assert (~over).sum() >= 4000  # one or two overfull slots, thousands of underfull ones
                few += 1
    assert few >= 6
    assert {1.0 / q for _, q in C.D_PAIRS} == {2.0 ** -10, 1024.0}


def test_family_e_rows_stand_on_both_sides_of_the_guard():
    pairs = C.family_e_long()
    assert {(C.instance(p, q), arr) for _, _, p, q, arr in pairs} == {(0, 1), (3, 2), (1, 1), (1, 2), (1, 3), (1, 5)}
    for lo, hi, p, q, arr in pairs:
        n0 = C.guard_length(p, q, C.effective(lo, p, q).count("R"), C.effective(lo, p, q).count("M"))
        assert len(lo) == int(0.9 * n0) and len(hi) == int(1.1 * n0) and 9000 < len(lo) < len(hi) < 17000
        assert C.guard_product(lo, p, q) <= C.GUARD_BOUND < C.guard_product(hi, p, q)
        assert hi[:len(lo)] == lo and set(hi[len(lo):]) == {"O"}
        assert max(int(1.0 / p * 2 ** 20), int(1.0 / q * 2 ** 20)) > 2 ** 20 - 3  # reduced integers near 2^20
    assert all(len(c) <= 65 for c in C.E_SHORT)
    for pq in C.E_SHORT_PAIRS:
        assert [r["cls"] for r in C.layout("E", pq).rows] == C.E_SHORT  # no row left out


@pytest.mark.parametrize("key", C.all_keys(), ids=lambda k: "%s-%s" % (k[0], "-".join(map(str, k[1]))))
def test_the_walkers_draw_what_decides(key):
    rows = C.layout(*key).rows
    assert rows
    for r in rows:
        assert r["W"] < C.W_MAX
        assert C.conditions(r, r["W"]) == [], (r["info"], r["W"])
        pick, _ = C.draws(r, r["W"])
        assert pick.size > 0.5 * r["W"] * r["to_v"]


def test_slots_exempt_from_the_two_sides_condition_are_named():
    """a probability within 2^-14 of 0 or 1: in families A - D only the fp64 residue of an exact 0 or 1 (no draw can
    fall on its other side: r2 is a multiple of 2^-32); family E names real ones, and still walks those rows"""
    named = 0
    for key, r in _all_rows():
        probs = r["table"][1]
        if r["n"] > 65:
            assert r["unbracketable"] == set()
            continue
        assert r["unbracketable"] == C.unbracketable(probs)
        for i in r["unbracketable"]:
            if key[0] != "E":
                assert min(probs[i], 1.0 - probs[i]) < 1e-9, (key, r["cls"], i, probs[i])
            else:
                named += 1
        inner = [i for i in range(r["n"]) if 0.0 < probs[i] < 1.0 and i not in r["unbracketable"]]
        assert all(C.EDGE <= probs[i] <= 1.0 - C.EDGE for i in inner)
    assert named > 0


def test_restated_first_step_and_tables_equal_the_oracle(oracle):
    """the walkers that standing() puts on v are those of the oracle's walk, and float_tables() is the oracle's table:
    the draw conditions above are conditions on the reference's draws"""
    for key in (("A", (0.5, 2.0)), ("A", (4.0, 2.0)), ("E", C.E_SHORT_PAIRS[0])):
        L = C.layout(*key)
        p, q = key[1]
        src, dst = np.concatenate(L.src), np.concatenate(L.dst)
        order = np.argsort(src * L.base + dst, kind="stable")
        rowptr = np.zeros(L.base + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=L.base), out=rowptr[1:])
        col = dst[order].astype(np.int32)
        for r in L.rows[::7]:
            nbs = col[rowptr[r["s"]]:rowptr[r["s"] + 1]]
            row = col[rowptr[r["v"]]:rowptr[r["v"] + 1]]
            assert np.array_equal(row, r["ids"])
            alias, probs = oracle.edge_alias_tables(r["s"], nbs.tolist(), row, np.ones(row.size), p, q)
            assert np.array_equal(np.asarray(alias), r["table"][0]) and np.array_equal(np.asarray(probs), r["table"][1])
            W = r["W"]
            walks, _ = oracle.random_walk(rowptr, col, None, np.array([r["s"]], np.int32), W, 2, p, q, C.SEED)
            first_v = int(np.searchsorted(nbs, r["v"]))
            ords = C.standing(r["s"], W, nbs.size, first_v, r["parallel"])
            assert np.array_equal(np.nonzero(walks[:, 1] == r["v"])[0], ords)
            pick, r2 = C.draws(r, W)
            want = r["ids"][np.where(r2 < r["table"][1][pick], pick, r["table"][0][pick])]
            assert np.array_equal(walks[ords, 2], want)
