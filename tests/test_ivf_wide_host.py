"""The cases of tests/ivf_wide_cases.py are what they claim (no GPU: the plans are the library's own, n2v_ivf_plan and
n2v_ivfpq_plan, which load without a device): every plan value tests/test_ivf_wide_gpu.py relies on, the empty runs of
the wide indexes, the pair counts on both sides of the flat scan's tile switch, that every table but the duplicate
ones is distinct per query, and that the ragged-m cases leave bytes of their code rows unused."""
import numpy as np
import pytest

import ivf_cases as ic
import ivf_wide_cases as wc
import ivfpq_cases as pc
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)

WIDE_K, WIDE_DIMS, WIDE_PQ = 10, (17, 64), ((24, 4), (24, 12))  # as the GPU file searches the wide indexes


@pytest.mark.parametrize("nlist", wc.WIDE_NLISTS)
def test_wide_indexes_and_their_empty_runs(nlist):
    idx = wc.wide_index(nlist)
    lens = idx.lens()
    assert idx.nlist == nlist == len(lens) and idx.n == wc.WIDE_N <= 11000
    assert lens[idx.long_list] == idx.max_list_rows == wc.WIDE_LONG == lens.max()
    assert len(np.unique(idx.row_ids)) == len(idx.row_ids) == idx.list_off[-1] and idx.row_ids.max() < idx.n
    mine = idx.lists[idx.long_list]
    assert (np.diff(mine) < 0).any() and (np.diff(mine) > 0).any()  # not ascending inside a list
    others = np.delete(lens, idx.long_list)
    assert ((others == 0) | ((others >= 1) & (others <= 17))).all()
    if nlist <= 2:
        assert idx.runs == [] and idx.long_list == nlist - 1
        return
    assert len(idx.runs) == 3 and idx.runs[0][0] == 0 and idx.runs[2][1] == nlist  # the start, the middle, the end
    for lo, hi in idx.runs:
        assert hi - lo >= 100 and (lens[lo:hi] == 0).all()
        assert (lo == 0 or lens[lo - 1] > 0) and (hi == nlist or lens[hi] > 0)  # the run ends where it says
    assert idx.long_list == idx.runs[1][1]  # the middle run leads straight up to the long list
    assert (others == 0).sum() > nlist // 2 and (others > 0).sum() > 100


@pytest.mark.parametrize("nlist", wc.WIDE_NLISTS)
def test_wide_probe_tables_and_plans(nlist):
    from node2vec_amd import ann

    idx = wc.wide_index(nlist)
    tables = wc.wide_probes(idx)
    want = {f"nprobe {min(p, nlist)}" for p in (1, 5, 64)} | {"every list", "just below the wide tile",
                                                              "just above the narrow tile"}
    assert set(tables) == want | ({"one empty run and the long list"} if nlist > 2 else set())
    for name, p in tables.items():
        nq, nprobe = p.shape
        assert wc.is_distinct(p) and p.min() >= -1 and p.max() < nlist and 1 <= nq <= wc.MAX_NQ, name
        assert (p == idx.long_list).any(), name
        qt = 64 if nq * nprobe > 16 * nlist else 16
        for dim in WIDE_DIMS:
            assert ann.plan(idx.n, dim, nlist, idx.max_list_rows, nq, nprobe, WIDE_K) == (qt, *wc.WIDE_PLAN[wc.FLAT]), name
        for dim, m in WIDE_PQ:
            got = ann.plan_pq(idx.n, dim, m, nlist, idx.max_list_rows, nq, nprobe, WIDE_K)
            assert got[:3] == (wc.tile_pairs(m), *wc.WIDE_PLAN[wc.PQ]) and got[4] == pc.code_stride(m), name
    assert tables["every list"].shape == (5, nlist) and (np.sort(tables["every list"], axis=1) == np.arange(nlist)).all()
    if nlist > 2:
        assert (tables["nprobe 1"] == -1).any() and (tables["nprobe 64"] == -1).any()
        run = tables["one empty run and the long list"]
        lo, hi = idx.runs[1]
        assert (((run >= lo) & (run < hi)) | (run == idx.long_list) | (run == -1)).all()
        assert (run == idx.long_list).sum(axis=1).tolist() == [1] * len(run)
        assert (idx.lens()[run[run != idx.long_list]] == 0).all()  # (-1 reads the last list: empty as well)
        # the slots of one query for the merge: far above 256 / k
        assert nlist * wc.WIDE_PLAN[wc.FLAT][1] >= 3000 and nlist * wc.WIDE_PLAN[wc.PQ][1] >= 2000
    # the two sides of the flat scan's tile switch
    nprobe, nq_below, nq_above = wc.tile_switch_queries(nlist)
    below, above = tables["just below the wide tile"], tables["just above the narrow tile"]
    assert below.shape == (nq_below, nprobe) and above.shape == (nq_above, nprobe) and nq_above == nq_below + 1
    assert below.size <= 16 * nlist < above.size
    if nlist == 1024:
        assert above.shape == (257, 64) and below.shape == (256, 64)
    for dim in WIDE_DIMS:
        assert ann.plan(idx.n, dim, nlist, idx.max_list_rows, nq_below, nprobe, WIDE_K)[0] == 16
        assert ann.plan(idx.n, dim, nlist, idx.max_list_rows, nq_above, nprobe, WIDE_K)[0] == 64
        assert ann.plan(idx.n, dim, nlist, idx.max_list_rows, 1, nprobe, WIDE_K)[0] == 16  # one query of them alone


def test_slot_count_cases():
    from node2vec_amd import ann

    seen = {1: set(), 3: set()}
    for nprobe, chunks in wc.SLOT_CASES:
        for scan in (wc.FLAT, wc.PQ):
            mlr, chunk_rows, long_len = wc.SLOT_PLAN[scan][chunks]
            idx = wc.slot_index(scan, chunks)
            assert (idx.nlist, idx.n, idx.max_list_rows) == (wc.SLOT_NLIST, wc.SLOT_N, mlr) and idx.n <= 11000
            lens = idx.lens()
            assert lens[wc.SLOT_LONG] == long_len == lens.max() and (lens == 0).sum() == 4
            assert (chunks - 1) * chunk_rows < long_len <= mlr  # the long list reaches the last chunk
            for k in wc.SLOT_KS:
                if scan == wc.FLAT:
                    got = ann.plan(idx.n, 16, idx.nlist, mlr, wc.SLOT_NQ, nprobe, k)[1:]
                else:
                    got = ann.plan_pq(idx.n, 16, 4, idx.nlist, mlr, wc.SLOT_NQ, nprobe, k)[1:3]
                assert got == (chunk_rows, chunks), (scan, nprobe, chunks, k)
            p = wc.slot_probes(np.random.default_rng(1), nprobe)
            assert p.shape == (wc.SLOT_NQ, nprobe) and wc.is_distinct(p) and p.max() < idx.nlist
            assert (p[::2] >= 0).all() and (p[::2] == wc.SLOT_LONG).any(axis=1).all()
        seen[chunks].add(nprobe * chunks)
    assert seen[1] == set(wc.SLOT_COUNTS) and seen[3] == {3, 12, 33} and wc.SLOT_KS == (1, 128)


def test_small_chunk_cases():
    from node2vec_amd import ann

    assert sorted(wc.SMALL_CHUNKS) == [1, 127, 128, 129]
    for mlr, (chunk_rows, chunks) in wc.SMALL_CHUNKS.items():
        idx = wc.small_index(mlr)
        assert idx.lens().tolist() == [0, 1, mlr, 1, 0, mlr] and idx.max_list_rows == mlr and idx.n == wc.SMALL_N
        assert chunks == 1 and chunk_rows in (128, 256)
        for k in (1, 10, 128):
            assert ann.plan(idx.n, 16, 6, mlr, 30, 3, k)[1:] == (chunk_rows, chunks)
            assert ann.plan_pq(idx.n, 16, 4, 6, mlr, 30, 3, k)[1:3] == (chunk_rows, chunks)
    for scan in (wc.FLAT, wc.PQ):
        mlr, chunk_rows, chunks = wc.SPARSE_PLAN[scan]
        idx = wc.sparse_index(scan)
        assert chunks == 5 and idx.max_list_rows == mlr == idx.n and idx.lens().max() == chunk_rows
        assert idx.list_off[-1] <= 5000 and (idx.lens() == 0).sum() == 2
        got = ann.plan(idx.n, 16, 6, mlr, 30, 3, 10)[1:] if scan == wc.FLAT else \
            ann.plan_pq(idx.n, 16, 4, 6, mlr, 30, 3, 10)[1:3]
        assert got == (chunk_rows, chunks)
    for p in wc.small_probes().values():
        assert wc.is_distinct(p) and p.max() == 5 and len(p) == 30


def test_ragged_m_cases():
    from node2vec_amd import ann

    assert tuple(m for _, m, *_ in wc.RAGGED_CASES) == wc.RAGGED_MS
    dsub_one, ragged, past = [], [], []
    for dim, m, k, long_kind, nq in wc.RAGGED_CASES:
        t, chunk, chunks, _, stride = ann.plan_pq(pc.HAND_N, dim, m, ic.NLIST, pc.HAND_MAX_LIST_ROWS, nq, 1, k)
        assert (t, chunk, chunks) == (wc.tile_pairs(m), pc.HAND_CHUNK, 3) and stride == pc.code_stride(m)
        assert m < stride and m <= dim <= 129 and nq > t + 1  # bytes of every code row that must not be looked at
        if m in wc.WIDE_ROW_MS:
            assert stride >= 16  # W >= 4: the unrolled look-up loop runs past m
        dsub = pc.dsub_of(dim, m)
        if dsub == 1:
            dsub_one.append(m)
        if dim % dsub:
            ragged.append(m)
        if (m - 1) * dsub >= dim:
            past.append(m)
        codes = pc.hand_codes(np.random.default_rng(m), 400, m)
        assert codes.shape == (400, stride) and codes[:, m:].any()  # the bytes past m are random, not zero
    assert sorted(m for m in wc.RAGGED_MS if pc.code_stride(m) >= 16) == sorted(wc.WIDE_ROW_MS)
    assert dsub_one == [3, 6, 12, 33] and ragged == [2, 5, 17, 63] and past == [24, 48, 63]
    assert {pc.code_stride(m) for m in wc.RAGGED_MS} == {4, 8, 16, 32, 64}


def test_duplicate_tables_repeat_one_list_in_one_query():
    tables = wc.duplicate_tables()
    assert [name for name, *_ in tables] == ["[5, 5]", "[LONG, 3, LONG]", "64 probes, the last repeats the first"]
    for name, where, p, bad, fixed in tables:
        nlist = wc.SLOT_NLIST if where == "slots" else 1024
        assert p.min() >= -1 and p.max() < nlist and not wc.is_distinct(p)
        assert wc.is_distinct(np.delete(p, bad, axis=0))  # every other query is valid
        row = p[bad]
        assert row[-1] == row[0] and len(np.unique(row)) == len(row) - 1 and (row >= 0).all()
        q = p.copy()
        q[bad] = fixed
        assert wc.is_distinct(q) and fixed[:-1] == row[:-1].tolist() and fixed[-1] == -1
    assert tables[0][2][4].tolist() == [5, 5] and tables[1][2][7].tolist() == [wc.SLOT_LONG, 3, wc.SLOT_LONG]
    assert tables[2][2].shape == (12, 64)
