"""Shared by tests/test_ivf_wide_host.py and tests/test_ivf_wide_gpu.py: the launch geometry of the two inverted-file
scans (csrc/n2v_ivf.hip, csrc/n2v_ivfpq.hip, their n2v_ivf_group.h and n2v_topk_select.h) away from the one index shape
of ivf_cases / ivfpq_cases (9 lists, nprobe <= 4, three chunks).  numpy only.

What a search must return is not restated here: ivf_cases.expect and ivfpq_cases.scan_expect / lut_expect / qhat know
nothing of tiles, chunks or groups, so they are the reference for every case below as they stand.  This module builds
  * wide indexes: 1, 2, 1023 and 1024 lists, nearly all empty or of 1 .. 17 rows, with runs of empty lists at the
    start, in the middle and at the end, one list exactly max_list_rows long, the row numbers a seeded permutation;
  * probe tables for them: distinct per query, -1 in the unused slots, 1 / 5 / 64 probes and every list, a table that
    stays inside one empty run but for the long list, and two tables just below and just above the 16 nlist pairs at
    which the flat plan changes its tile;
  * slot-count cases (nprobe x chunks = 1, 2, 3, 5, 7, 12, 33), small-chunk cases (max_list_rows 1, 127, 128, 129 and
    five chunks over short lists), ragged-m cases for the product-quantised codes;
  * probe tables with a repeated list, which the library must refuse.
Every plan value a case claims is asserted from n2v_ivf_plan / n2v_ivfpq_plan in test_ivf_wide_host.py."""
import numpy as np

import ivf_cases as ic
import ivfpq_cases as pc

FLAT, PQ = "flat", "pq"

# ---- wide indexes -------------------------------------------------------------------------------------------------

WIDE_NLISTS = (1, 2, 1023, 1024)
WIDE_N = 8000        # rows of the matrix the row numbers belong to
WIDE_LONG = 4200     # the long list and max_list_rows: three chunks of 1408 rows (flat), two of 2176 positions (PQ)
WIDE_PLAN = {FLAT: (1408, 3), PQ: (2176, 2)}
RUN = 110            # lists of an empty run
MAX_NQ = 260


class WideIndex:
    """list_off int64 [nlist + 1], row_ids int32, lists (row arrays, for ivf_cases.expect), the long list's number,
    the empty runs [(first, past)], n and max_list_rows"""

    def __init__(self, lens, long_list, runs, n, max_list_rows, rng):
        self.nlist = len(lens)
        self.list_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert self.list_off[-1] <= n and max(lens) <= max_list_rows <= n
        self.row_ids = rng.permutation(n)[:self.list_off[-1]].astype(np.int32)
        self.lists = [self.row_ids[self.list_off[l]:self.list_off[l + 1]].astype(np.int64) for l in range(self.nlist)]
        self.long_list, self.runs, self.n, self.max_list_rows = long_list, runs, n, max_list_rows

    def lens(self):
        return np.diff(self.list_off)


def wide_index(nlist):
    """1 list: the long one.  2 lists: 7 rows and the long one.  1023 / 1024: empty runs of RUN lists at the start,
    in the middle and at the end; the long list is the one right after the middle run, so the tile offsets are flat
    all the way up to it; elsewhere 60 % of the lists are empty and the others hold 1 .. 17 rows"""
    rng = np.random.default_rng(7000 + nlist)
    if nlist <= 2:
        lens, long_list, runs = ([WIDE_LONG], 0, []) if nlist == 1 else ([7, WIDE_LONG], 1, [])
        return WideIndex(np.array(lens), long_list, runs, WIDE_N, WIDE_LONG, rng)
    lens = np.where(rng.random(nlist) < 0.6, 0, rng.integers(1, 18, nlist))
    mid = nlist // 2 - RUN
    runs = [(0, RUN), (mid, mid + RUN), (nlist - RUN, nlist)]
    for lo, hi in runs:
        lens[lo:hi] = 0
    long_list = mid + RUN
    lens[long_list] = WIDE_LONG
    lens[RUN], lens[mid - 1], lens[nlist - RUN - 1] = 1, 17, 3  # the runs' neighbours are not empty
    return WideIndex(lens, long_list, runs, WIDE_N, WIDE_LONG, rng)


def distinct_probes(rng, nq, nprobe, nlist, full=False, favour=None, among=None):
    """int64 [nq, nprobe]: per query a random number (full: nprobe) of distinct lists (of `among`, default all) in
    random slots, -1 in the others; every third query that has a probe names the list `favour`"""
    among = np.arange(nlist) if among is None else np.asarray(among)
    out = np.full((nq, nprobe), -1, np.int64)
    for q in range(nq):
        m = nprobe if full else int(rng.integers(0, nprobe + 1))
        slots = np.sort(rng.choice(nprobe, m, replace=False))
        out[q, slots] = rng.choice(among, m, replace=False)
        if favour is not None and m > 0 and q % 3 == 0 and favour not in out[q]:
            out[q, slots[int(rng.integers(0, m))]] = favour
    return out


def tile_switch_queries(nlist):
    """(nprobe, nq below, nq above): nq x nprobe pairs are at most 16 nlist for the first, more for the second"""
    nprobe = min(64, nlist)
    below = 16 * nlist // nprobe
    return nprobe, below, below + 1


def wide_probes(index):
    """name -> probes int64 [nq <= MAX_NQ, nprobe]"""
    rng = np.random.default_rng(7100 + index.nlist)
    nlist, long_list = index.nlist, index.long_list
    out = {}
    for nprobe, nq in ((1, 100), (5, 100), (64, 40)):
        nprobe = min(nprobe, nlist)
        out.setdefault(f"nprobe {nprobe}", distinct_probes(rng, nq, nprobe, nlist, favour=long_list))
    out["every list"] = distinct_probes(rng, 5, nlist, nlist, full=True)
    if index.runs:
        lo, hi = index.runs[1]
        p = distinct_probes(rng, 60, 5, nlist, full=True, among=np.arange(lo, hi))
        p[np.arange(60), rng.integers(0, 5, 60)] = long_list
        p[7] = [lo, -1, hi - 1, -1, long_list]
        out["one empty run and the long list"] = p
    nprobe, below, above = tile_switch_queries(nlist)
    out["just below the wide tile"] = distinct_probes(rng, below, nprobe, nlist, favour=long_list)
    out["just above the narrow tile"] = distinct_probes(rng, above, nprobe, nlist, favour=long_list)
    assert all(len(p) <= MAX_NQ for p in out.values())
    return out


def is_distinct(probes):
    return all(len(np.unique(row[row >= 0])) == (row >= 0).sum() for row in np.asarray(probes))


# ---- slot counts: nprobe x chunks lists for the merge -------------------------------------------------------------------

SLOT_NLIST, SLOT_LONG, SLOT_N, SLOT_NQ = 40, 17, pc.HAND_N, 24
SLOT_KS = (1, 128)
# (nprobe, chunks): 1, 2, 3, 5, 7, 12, 33 slots of one chunk; 3, 12, 33 slots of three
SLOT_CASES = [(1, 1), (2, 1), (3, 1), (5, 1), (7, 1), (12, 1), (33, 1), (1, 3), (4, 3), (11, 3)]
SLOT_COUNTS = (1, 2, 3, 5, 7, 12, 33)
# chunks -> (max_list_rows, rows per chunk, the long list): one chunk that the long list fills; three chunks (the
# hand-made indexes' bound) with the long list one row into the third
SLOT_PLAN = {FLAT: {1: (300, 384, 300), 3: (ic.HAND_MAX_LIST_ROWS, 1792, 2 * 1792 + 1)},
             PQ: {1: (300, 384, 300), 3: (pc.HAND_MAX_LIST_ROWS, pc.HAND_CHUNK, 2 * pc.HAND_CHUNK + 1)}}


def slot_index(scan, chunks):
    """40 lists: the long one at SLOT_LONG, four empty, the others of 1 .. 60 rows"""
    rng = np.random.default_rng(7200 + chunks + (10 if scan == PQ else 0))
    mlr, _, long_len = SLOT_PLAN[scan][chunks]
    lens = rng.integers(1, 61, SLOT_NLIST)
    lens[[0, 9, 18, 39]] = 0
    lens[SLOT_LONG] = long_len
    return WideIndex(lens, SLOT_LONG, [], SLOT_N, mlr, rng)


def slot_probes(rng, nprobe):
    """SLOT_NQ queries: the even ones name nprobe lists, the long one among them; the odd ones a random number"""
    p = distinct_probes(rng, SLOT_NQ, nprobe, SLOT_NLIST, favour=SLOT_LONG)
    p[::2] = distinct_probes(rng, SLOT_NQ // 2, nprobe, SLOT_NLIST, full=True)
    for q in range(0, SLOT_NQ, 2):
        if SLOT_LONG not in p[q]:
            p[q, int(rng.integers(0, nprobe))] = SLOT_LONG
    return p


# ---- small chunks ---------------------------------------------------------------------------------------------------

# max_list_rows -> (rows per chunk, chunks) of both plans
SMALL_CHUNKS = {1: (128, 1), 127: (128, 1), 128: (128, 1), 129: (256, 1)}
SMALL_N = 600
# max_list_rows of five chunks over lists no longer than one: (max_list_rows = n, rows per chunk, chunks).  The PQ
# plan cuts at 4096 positions, so its five chunks need row numbers up to 20480; no matrix of that size exists (the PQ
# scan reads codes, and only 4926 positions are listed)
SPARSE_PLAN = {FLAT: (10240, 2048, 5), PQ: (20480, 4096, 5)}


def small_index(mlr):
    """lists of 0, 1, mlr, 1, 0 and mlr rows"""
    return WideIndex(np.array([0, 1, mlr, 1, 0, mlr]), 2, [], SMALL_N, mlr, np.random.default_rng(7300 + mlr))


def sparse_index(scan):
    """lists of 0, 1, one whole chunk, 700, 129 and 0 rows under a max_list_rows of five chunks: the blocks of four
    of the five grid rows find their list ended"""
    mlr, chunk, _ = SPARSE_PLAN[scan]
    return WideIndex(np.array([0, 1, chunk, 700, 129, 0]), 2, [], mlr, mlr, np.random.default_rng(7400 + chunk))


def small_probes(nlist=6, nq=30):
    """name -> probes: three random distinct lists a query; one list a query, every list in turn"""
    rng = np.random.default_rng(7500)
    return {"three lists": distinct_probes(rng, nq, 3, nlist), "one list": (np.arange(nq) % nlist)[:, None].copy()}


# ---- product-quantised codes whose m does not fill the code row ---------------------------------------------------------

# dim, m, k, the long list in terms of the plan's chunk, queries.  dsub = 1 (m == dim): (3, 3), (6, 6), (12, 12),
# (33, 33); a ragged last sub-space: (3, 2), (17, 5), (129, 17), (127, 63); sub-spaces wholly past dim: (100, 24) from
# the 21st, (129, 48) from the 44th, (127, 63) from the 44th.  m < code_stride(m) in every case: m = 2, 3 in 4-byte
# rows; 5, 6 in 8; 12 in 16 (W = 4); 17, 24 in 32 (W = 8); 33, 48, 63 in 64 (W = 16)
RAGGED_CASES = [
    (3, 2, 10, "c+1", 60), (3, 3, 1, "c", 60), (17, 5, 128, "c-1", 60), (6, 6, 10, "2c+1", 60),
    (12, 12, 127, "c+1", 60), (129, 17, 10, "c", 60), (100, 24, 128, "c+1", 60), (33, 33, 10, "2c+1", 60),
    (129, 48, 1, "c-1", 60), (127, 63, 128, "c+1", 60),
]
RAGGED_MS = (2, 3, 5, 6, 12, 17, 24, 33, 48, 63)
WIDE_ROW_MS = (12, 17, 24, 33, 48, 63)  # code rows of 16 bytes and more (W >= 4) that m does not fill


def tile_pairs(m):
    return 16 if m <= 7 else 8 if m <= 16 else 4 if m <= 32 else 2


# ---- a list a query names twice -----------------------------------------------------------------------------------------

def duplicate_tables():
    """[(name, which index, probes int64 [12, nprobe], the query with the repeat, its row with the repeat taken
    out)]: every other query is valid.  The first two are for slot_index(scan, 1), the third for wide_index(1024)"""
    rng = np.random.default_rng(7600)
    out = []
    for name, row in (("[5, 5]", [5, 5]), ("[LONG, 3, LONG]", [SLOT_LONG, 3, SLOT_LONG])):
        p = distinct_probes(rng, 12, len(row), SLOT_NLIST, favour=SLOT_LONG)
        bad = 4 if len(row) == 2 else 7
        p[bad] = row
        out.append((name, "slots", p, bad, row[:-1] + [-1]))
    wide = wide_index(1024)
    p = distinct_probes(rng, 12, 64, wide.nlist, favour=wide.long_list)
    row = distinct_probes(rng, 1, 64, wide.nlist, full=True)[0]
    row[0] = wide.long_list if wide.long_list not in row else row[0]
    row[63] = row[0]
    p[9] = row
    fixed = row.copy()
    fixed[63] = -1
    out.append(("64 probes, the last repeats the first", "wide 1024", p, 9, fixed.tolist()))
    return out
