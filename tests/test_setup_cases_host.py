"""The cases of tests/setup_cases.py are what they claim to be -- proven on the CPU, so that the GPU file
(test_setup_kernels_gpu.py) pins the kernels on inputs known to reach the branches they were built for."""
import bisect

import numpy as np
import pytest

import setup_cases as sc


@pytest.fixture(scope="module")
def traced(oracle):
    """every deliberate K1 row with the oracle's table and the events of the pairing loop"""
    out = []
    for name, w in sc.alias_rows():
        if len(w) == 0:
            continue
        alias, probs, facts = sc.alias_trace(w)
        a, p = oracle.alias_tables(w)
        assert a == alias and np.array_equal(np.array(p).view(np.uint64), np.array(probs).view(np.uint64)), name
        out.append((name, w, alias, probs, facts))
    return out


def test_past_one_pass_sizes_exceed_any_resident_grid():
    """a CU holds at most 32 waves: 2 x that many rows / items cannot be covered by one trip of a resident
    grid, whatever the occupancy query answered"""
    for cus in (1, 64, 256, 304):
        waves = cus * sc.WAVES_PER_CU
        assert sc.rows_past_one_pass(cus) > 2 * waves
        for m in (2, 4):
            # the launcher's cap is resident_blocks x m blocks of 256 threads <= waves x 64 x m threads
            assert sc.items_past_one_pass(cus, m) > 2 * waves * 64 * m
            assert sc.items_past_one_pass(cus, m) % 256 != 0  # and ends inside a block


def test_alias_rows_have_every_length_and_pattern(traced):
    by_len = {}
    for name, w, *_ in traced:
        by_len.setdefault(len(w), set()).add(name.split("/")[0])
    assert set(by_len) == set(sc.ALIAS_LENGTHS) | {10}
    for n in sc.ALIAS_LENGTHS:
        assert "equal_exact" in by_len[n]
        if n >= 3:
            assert {"light_once", "zeros", "not_fp32", "decades_f32", "under_low_over_high",
                    "over_low_under_high", "heavy_at_0", f"heavy_at_{n - 1}", "light_chain_0"} <= by_len[n], n
        if n > 64:
            assert {"heavy_at_63", "heavy_at_64", "light_chain_63", "light_chain_64"} <= by_len[n], n
    assert by_len[10] == {"decimal_10", "decimal_under_10"}
    assert {"equal_decimal", "equal_decimal_under"} <= by_len[64] and {"equal_decimal", "equal_decimal_under"} <= by_len[65]
    names = [n for n, _ in sc.alias_rows()]
    lens = [len(w) for _, w in sc.alias_rows()]
    assert lens[0] == 0 and lens[-1] == 0 and lens[-2] == 0  # empty first, last and in a run
    assert len(set(names)) == len(names)


def test_alias_rows_storage_forms(traced):
    """some rows are not fp32 values (they need the fp64 graph), the decades rows are fp32 values spanning
    24 decades, and enough rows are fp32 values to make an fp32 graph of them"""
    f32 = {name for name, w, *_ in traced if sc.is_f32(w)}
    assert not any(n.startswith("not_fp32") or n.startswith("equal_decimal") for n in f32)
    dec = [w for name, w, *_ in traced if name.startswith("decades_f32/")]
    assert all(sc.is_f32(w) for w in dec) and all(w.max() / w.min() > 0.99e24 for w in dec)
    assert len(f32) > 100


def test_alias_rows_reach_every_exit_of_the_pairing_loop(traced):
    facts = {name: f for name, _, _, _, f in traced}
    probs = {name: p for name, _, _, p, _ in traced}
    # no pairing at all, because no slot is underfull: every prob is 1.0
    for n in sc.ALIAS_LENGTHS:
        f = facts[f"equal_exact/{n}"]
        assert f["pairings"] == 0 and f["initial_under"] == 0 and set(probs[f"equal_exact/{n}"]) == {1.0}
    # no pairing at all although no prob is 1.0: the ulp quirk of [0.1] * 10 (G1) leaves every slot
    # overfull at 1.0000000000000002, at chunk-sized rows too ...
    for n in ("decimal_10", "equal_decimal/64", "equal_decimal/65"):
        f = facts[n]
        assert f["pairings"] == 0 and f["initial_under"] == 0 and f["left"] == "over" and f["left_prob"] > 1.0
    # ... and [0.7] * n leaves every slot UNDERFULL: the loop ends on its first look for an overfull
    for n in ("decimal_under_10", "equal_decimal_under/64", "equal_decimal_under/65"):
        f = facts[n]
        assert f["pairings"] == 0 and f["initial_over"] == 0 and f["left"] == "under" and f["left_prob"] < 1.0
    # the leftover is an underfull, after pairings
    assert any(f["left"] == "under" and f["pairings"] > 0 for f in facts.values())
    # ... because the last overfull was demoted on the last iteration
    assert sum(f["last_demoted"] for f in facts.values()) >= 10
    # the leftover is an overfull whose prob is not 1.0 (rounding: exact arithmetic always ends on 1.0)
    odd = [n for n, f in facts.items() if f["left"] == "over" and f["pairings"] > 0 and f["left_prob"] != 1.0]
    assert len(odd) >= 5 and any(len(probs[n]) > 128 for n in odd)
    # the leftover is an overfull of exactly 1.0
    assert facts["light_once/193"]["left"] == "over" and facts["light_once/193"]["left_prob"] == 1.0
    assert facts["light_once/193"]["pairings"] == 1 and not facts["light_once/193"]["demotions"]
    # an index is an alias target, falls below 1.0 and is then paired as an underfull itself
    assert sum(f["demoted_then_paired"] > 0 for f in facts.values()) >= 20


def test_alias_rows_carry_state_across_chunks(traced):
    facts = {name: f for name, _, _, _, f in traced}
    # a chain of demotions that crosses chunk boundaries: consecutive demoted indices in different chunks,
    # through every chunk of the row
    for n in (65, 129, 193, 4099):
        d = facts[f"light_chain_0/{n}"]["demotions"]
        assert len(d) >= n - 3 and d == sorted(d, reverse=True)  # (rounding may end the chain a slot early)
        assert {i // 64 for i in d} == set(range((n + 63) // 64))
    # one overfull that takes every underfull of the row, chunk after chunk, placed in chunk 0 and chunk 1
    for k in (0, 63, 64):
        f = facts[f"heavy_at_{k}/193"]
        assert f["initial_over"] == 1 and f["pairings"] >= 191
    # the only underfull in chunk 0 while the top overfull is in the last chunk, and the mirror image
    for n in (129, 193, 4099):
        f = facts[f"under_low_over_high/{n}"]
        assert f["initial_under"] == 1 and f["pairings"] >= 1
        f = facts[f"over_low_under_high/{n}"]
        assert f["initial_under"] == 1 and f["pairings"] >= 1
    # zeros among positive weights: underfulls of prob 0.0
    _, w, _, p, f = next(t for t in traced if t[0] == "zeros/129")
    assert (w == 0).sum() == 43 and f["demoted_then_paired"] > 0


def test_short_rows_graph_has_empty_rows_where_promised():
    n = sc.rows_past_one_pass(4)
    rowptr, col, w, z = sc.short_rows_graph(n)
    lens = np.diff(rowptr)
    assert len(lens) == n and lens.max() == 9 and w.dtype == np.float32
    assert (lens[:3] == 0).all() and (lens[-2:] == 0).all()
    assert (lens[n // 5: n // 5 + 40] == 0).all() and (lens[n - n // 7: n - n // 7 + 25] == 0).all()
    assert n - n // 7 > n // 2  # a run in the second trip as well
    assert z > n // 2 + 1 and rowptr[z + 1] - rowptr[z] == 3 and (w[rowptr[z]:rowptr[z + 1]] > 0).all()
    rowptr0, col0, w0, z0 = sc.short_rows_graph(n, zero=True)
    assert z0 == z and np.array_equal(rowptr0, rowptr) and np.array_equal(col0, col)
    assert (w0[rowptr[z]:rowptr[z + 1]] == 0).all() and (w0 != w).sum() == 3  # nothing else changes


def test_bias_cases_membership_in_closed_form_is_membership_by_search():
    small = sc.bias_edges_case()
    assert np.array_equal(small.classes(), small.classes_by_search())
    stride = sc.bias_stride_case(sc.items_past_one_pass(1, 2))
    assert len(stride.ids) == sc.items_past_one_pass(1, 2)
    assert np.array_equal(stride.classes(), stride.classes_by_search())
    for c in (small, stride):
        assert set(np.unique(c.classes())) == {0, 1, 2, 3}
        for r in range(c.n_rows):  # what the kernels' searches need: ascending, distinct
            for a, ptr in ((c.ids, c.rowptr), (c.src_nbs, c.src_rowptr)):
                assert (np.diff(a[ptr[r]:ptr[r + 1]].astype(np.int64)) > 0).all()
        assert not sc.is_f32(c.w64) and c.ids.min() >= 0


def test_bias_edges_case_probes_every_edge_of_every_source_list():
    c = sc.bias_edges_case()
    lens, ms = np.diff(c.rowptr), np.diff(c.src_rowptr)
    assert lens[0] == 0 and lens[1] == 0 and lens[-1] == 0 and lens[-2] == 0  # empty rows first, last, in runs
    assert any(lens[i] == 0 and lens[i + 1] == 0 and lens[i + 2] == 0 for i in range(2, len(lens) - 4))
    assert set(ms[lens > 0]) == set(sc.SRC_LENGTHS)
    assert ((c.src_id < 0) & (lens > 0)).sum() >= 8 and ((c.src_id >= 0) & (lens > 0)).sum() >= 24
    cls = c.classes()
    seen = set()
    for r in range(c.n_rows):
        if lens[r] == 0 or c.src_id[r] < 0 or ms[r] == 0:
            continue
        nb = c.src_nbs[c.src_rowptr[r]:c.src_rowptr[r + 1]]
        ids = c.ids[c.rowptr[r]:c.rowptr[r + 1]]
        assert nb[0] in ids and nb[-1] in ids and ids.min() < nb[0] and ids.max() > nb[-1]
        s = c.src_id[r]
        if s in nb and s in ids:  # x == s with s in the source list too: the return branch must win
            assert cls[c.rowptr[r] + list(ids).index(s)] == 0
            seen.add(int(ms[r]))
    assert seen == set(sc.SRC_LENGTHS) - {0}


def test_bias_stride_case_shape():
    c = sc.bias_stride_case(sc.items_past_one_pass(2, 2))
    lens, ms = np.diff(c.rowptr), np.diff(c.src_rowptr)
    assert lens[0] == 0 and (lens[-3:] == 0).all() and lens.max() == 1000
    for length in (5, 17, 64, 1000):  # every row length meets every source-list length
        assert set(ms[lens == length]) == set(sc.SRC_LENGTHS)
    assert (c.src_id[lens > 0] < 0).any() and (c.src_id[lens > 0] >= 0).any()


def test_draw_expected_is_the_oracle(oracle):
    """the numpy statement used for the large draw cases equals sampling_from_alias / _wiki of the oracle"""
    rowptr, col, alias_idx, prob = sc.draw_table([1, 3, 64, 300, 7, 2])
    rng = np.random.default_rng(1)
    n_rows = len(rowptr) - 1
    for trial in range(40):
        r1, r2 = rng.random(n_rows), rng.random(n_rows)
        if trial == 0:
            r1[:] = 0.0
        if trial == 1:
            r1[:] = np.nextafter(1.0, 0.0)
        if trial == 2:  # r2 == prob[pick] exactly: `<` is false, the alias is chosen
            pick = (r1 * np.diff(rowptr)).astype(np.int64)
            r2 = prob[rowptr[:-1] + pick].copy()
        two, bad2 = sc.draw_expected(rowptr, col, alias_idx, prob, r1, r2)
        one, bad1 = sc.draw_expected(rowptr, col, alias_idx, prob, r1, None)
        assert not bad1.any() and not bad2.any()
        for r in range(n_rows):
            b, e = rowptr[r], rowptr[r + 1]
            assert two[r] == col[b + oracle.sampling_from_alias(alias_idx[b:e], prob[b:e], r1[r], r2[r])]
            assert one[r] == col[b + oracle.sampling_from_alias_wiki(alias_idx[b:e], prob[b:e], r1[r])]
        if trial == 1:
            assert np.array_equal(two, np.where(r2 < prob[rowptr[1:] - 1], col[rowptr[1:] - 1],
                                                col[rowptr[:-1] + alias_idx[rowptr[1:] - 1]]))
        if trial == 2:
            assert np.array_equal(two, col[rowptr[:-1] + alias_idx[rowptr[:-1] + pick]])
    # Python's int() truncates toward zero: r1 = -0.25 on three slots is pick 0, r1 = -1.0 is outside
    v, bad = sc.draw_expected(rowptr[:3], col, alias_idx, prob, np.array([-0.25, -0.25]), np.array([0.0, 2.0]))
    assert not bad.any() and int(-0.25 * 3) == 0
    v, bad = sc.draw_expected(rowptr[:3], col, alias_idx, prob, np.array([1.0, -1.0]), np.array([0.5, 0.5]))
    assert bad.all() and (v == -1).all()
    for n in (1, 3, 64, 3000):  # int(r1 * n) == n - 1 at the last fp64 below 1.0
        assert int(np.nextafter(1.0, 0.0) * n) == n - 1


def test_uniform_bits_restatement_is_the_oracle(oracle):
    keys, steps = sc.uniform_keys(400)
    for seed in (0, 42, 2 ** 64 - 1):
        u1, u2 = sc.uniform_bits(seed, keys, steps)
        for i in range(len(keys)):
            assert (int(u1[i]), int(u2[i])) == oracle.uniform_bits(seed, int(keys[i]) & (2 ** 64 - 1), int(steps[i]))
    assert keys.min() == -2 ** 63 and keys.max() == 2 ** 63 - 1 and steps.max() == 2 ** 31 - 1


def test_trim_cases_have_rows_on_both_sides_of_the_cap(oracle):
    for cap in sc.TRIM_CAPS:
        for n_rows in sc.TRIM_ROWS:
            rowptr = sc.trim_rowptr(n_rows, cap)
            deg = np.diff(rowptr)
            assert len(deg) == n_rows and deg[0] > cap and deg[-1] > cap
            assert {cap - 1, cap, cap + 1, 2 * cap} <= set(deg.tolist())
            keep = oracle.trim_mark(rowptr, cap, 20)
            kept = np.add.reduceat(keep.astype(np.int64), rowptr[:-1][deg > 0])
            assert np.array_equal(kept, np.minimum(deg[deg > 0], cap))


def test_cum_tables_with_runs_really_have_runs():
    import torch

    from node2vec_amd import sgns

    for n_side, bits in ((2500, 10), (20000, 12)):
        counts = sc.runs_counts(n_side)
        n = len(counts)
        assert int(min(24, max(10, int(np.ceil(np.log2(max(n, 2)))) - 4))) == bits  # SgnsModel's rule
        tab = sgns.make_cum_table(torch.from_numpy(counts)).numpy().astype(np.int64)
        d = np.diff(tab)
        assert (d >= 0).all() and tab[-1] == sc.CUM_DOMAIN
        assert (tab[:200] == 0).all() and tab[n_side - 1] < 100  # starts on a run of zeros: the bucket edge 0 hits it exactly
        assert (d[:n_side - 1] == 0).sum() > n_side - 100
        assert (d[n_side + 1:] == 0).sum() > n_side // 2  # runs after the giant as well
        want = sc.cum_index_expected(tab, bits)
        assert want[0] == 0 and want[1] == n_side and want[-1] == n
        for b in (0, 1, (1 << bits) - 1, 1 << bits):
            assert want[b] == bisect.bisect_left(tab.tolist(), b << (31 - bits))
    for bits in (10, 12):
        tab = sc.edge_hitting_table(bits)
        left = sc.cum_index_expected(tab, bits)
        edges = np.arange((1 << bits) + 1, dtype=np.int64) << (31 - bits)
        right = np.searchsorted(tab, edges, side="right")
        assert ((right - left) >= 5).sum() >= (1 << bits) // 37  # runs sitting exactly on bucket edges
        assert (np.diff(tab) >= 0).all() and tab[-1] == sc.CUM_DOMAIN and left[-1] == len(tab)
    for n in (1, 2, 17):  # the smallest vocabularies: bits = 10
        tab = sgns.make_cum_table(torch.arange(n, 0, -1)).numpy().astype(np.int64)
        assert len(tab) == n and tab[-1] == sc.CUM_DOMAIN
        assert sc.cum_index_expected(tab, 10)[-1] == n
