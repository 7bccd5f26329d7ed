"""Inputs of the forwarding tests, built on the CPU: a gadget graph with its wedge tables computed in numpy straight
from the definition in include/n2v_hip.h, walker batches, and the case table (tests/test_forward_host.py proves
the table with the restatement alone; tests/test_forward_gpu.py runs it through the kernels).

Not a test module: helpers shared by the two.
"""
import functools
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

import forward_restatement as R

I64 = np.int64
GADGET_LENGTHS = (0, 1, 14, 15, 31, 32, 33, 63, 64, 65, 200)
WALK_LENGTH = 9
# n2v::resident_blocks(forward kernel, 1024 threads) * 1024 as it comes out on the MI355X: 256 CUs x 1 resident block
# (the occupancy query answers 1 for this kernel's 1024 threads and 36 KB of LDS) = 256 blocks = 262 144 walkers per
# pass of the grid-stride loop
RESIDENT_WALKERS = 256 * 1024
K_BEYOND_GRID = 4 * RESIDENT_WALKERS + 4099  # 1 052 675: five passes, the last one ragged (4099 = 4 blocks + 3)


@dataclass
class Graph:
    n: int
    rowptr: np.ndarray  # int64 [n + 1]
    col: np.ndarray  # int32 [E], rows sorted, multi-edges kept
    edge_classes: np.ndarray  # uint32 [E]
    wedge_off: np.ndarray  # uint64 [E]: offset | return position << 40
    pos16: np.ndarray  # uint16 [W]
    pos32: np.ndarray  # uint32 [W], the same lists
    pos32_high: np.ndarray  # uint32 [W]: the lists of odd edges moved up by 70 000 (a table of a graph with wide rows)
    gadget_edge: dict  # m -> index of the edge s_m -> v_m
    sinks: np.ndarray


@functools.lru_cache(maxsize=None)
def gadget_graph() -> Graph:
    """For every m of GADGET_LENGTHS a pair (s_m, v_m) joined both ways with exactly m common out-neighbours, so that
    the edge s_m -> v_m (and v_m -> s_m) has a wedge list of exactly m entries.  Ids are laid out c.. s_m c.. v_m, so
    that s_m stands in the middle of N(v_m) (a non-zero return position); every other pair has its return edge
    v_m -> s_m twice and its edge s_m -> v_m twice (return counts of 2).  A few sinks at the top of the id range, and
    4000 random edges from vertices that are no s_m or v_m (their out-rows are fixed by the construction)."""
    rng = np.random.default_rng(20)
    src, dst, pairs, nxt_id = [], [], {}, 0
    for j, m in enumerate(GADGET_LENGTHS):
        ids = np.arange(nxt_id, nxt_id + m + 2)
        nxt_id += m + 2
        s, v = int(ids[m // 2]), int(ids[-1])
        common = np.delete(ids, [m // 2, m + 1])
        assert common.size == m
        pairs[m] = (s, v)
        reps = 2 if j % 2 else 1
        src += [s] * reps + [v] * reps + [s] * m + [v] * m
        dst += [v] * reps + [s] * reps + common.tolist() + common.tolist()
    fixed = np.array([x for p in pairs.values() for x in p])
    n_free = 300
    n_sinks = 6
    n = nxt_id + n_free + n_sinks
    sinks = np.arange(n - n_sinks, n)
    sources = np.setdiff1d(np.arange(n - n_sinks), fixed)
    a = rng.choice(sources, 4000)
    b = rng.integers(0, n, 4000)
    # a dense corner, so that lists of assorted lengths (up to a few dozen entries) surround the gadgets
    corner = np.arange(nxt_id, nxt_id + 60)
    ca, cb = rng.choice(corner, 1500), rng.choice(corner, 1500)
    src = np.concatenate([np.array(src), a, ca])
    dst = np.concatenate([np.array(dst), b, cb])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rowptr = np.zeros(n + 1, dtype=I64)
    np.add.at(rowptr, src + 1, 1)
    rowptr = np.cumsum(rowptr)
    col = dst.astype(np.int32)
    E = col.size
    # the tables, edge by edge, from the definition: for e = (s -> v) the positions j with N(v)[j] in N_out(s) and
    # N(v)[j] != s, ascending; the return count = entries of N(v) equal to s, the return position = the first of them
    ec = np.zeros(E, dtype=np.uint32)
    off = np.zeros(E, dtype=np.uint64)
    lists = []
    total = 0
    rows = [col[rowptr[x]:rowptr[x + 1]] for x in range(n)]
    for s in range(n):
        for e in range(rowptr[s], rowptr[s + 1]):
            nv = rows[col[e]]
            back = nv == s
            shared = np.nonzero(np.isin(nv, rows[s]) & ~back)[0]
            ret = int(back.sum())
            rpos = int(np.argmax(back)) if ret else 0
            assert ret < 255 and shared.size < EC_LIMIT
            ec[e] = shared.size | ret << 24
            off[e] = total | rpos << 40
            total += shared.size
            lists.append(shared)
    pos = np.concatenate(lists).astype(I64)
    assert pos.size == total and (pos.max() < 65536)
    odd = np.repeat(np.arange(E) % 2 == 1, (ec & 0xFFFFFF).astype(I64))
    gadget_edge = {}
    for m, (s, v) in pairs.items():
        e = int(rowptr[s] + np.nonzero(rows[s] == v)[0][0])
        assert int(ec[e] & 0xFFFFFF) == m
        gadget_edge[m] = e
    return Graph(n, rowptr, col, ec, off, pos.astype(np.uint16), pos.astype(np.uint32),
                 (pos + 70_000 * odd).astype(np.uint32), gadget_edge, sinks)


EC_LIMIT = 0xFFFFFF


@dataclass(frozen=True)
class Case:
    name: str
    k: int
    n_parts: int
    bounds: str = "even"  # even | gap (an empty part in the middle and an empty last part) | last (all to the last
    #                       part: every first vertex is 0) | first (all to part 0: every other part is empty)
    carry: int = 2
    head_cols: int = 5
    wide: int = 0
    table: str = "plain"  # plain | high (pos32_high) | null (NULL tables)
    api: str = "forward"  # forward | boxes | paths (n2v_partition_forward with log_out == NULL)
    fit: str = "tight"  # tight | head | pool | both | cap0 | middle (the overflow kinds) | ragged (boxes: slack, gaps,
    #                     boxes of capacity 0 and pools of 0 words where nothing is needed)
    vanish: float = 0.1
    finish: float = 0.1
    empty: float = 0.0
    empty_runs: Tuple[Tuple[int, int], ...] = ()  # [from, to) made empty slots
    gadgets: float = 0.25  # share of the walkers that leave along a gadget edge
    batches: int = 1
    seed: int = 1
    expect_overflow: bool = field(default=False)


def _cases():
    c = []
    for i, k in enumerate((1, 63, 64, 65, 1023, 1024, 1025, 4097)):
        c.append(Case(f"k{k}", k, (2, 5)[i % 2], wide=i % 2, bounds=("even", "gap")[i % 2], seed=10 + i))
    c.append(Case("beyond_grid", K_BEYOND_GRID, 2, gadgets=0.002, seed=30))
    c.append(Case("empty_wave", 1500, 5, empty_runs=((128, 192),), empty=0.05, seed=31))
    c.append(Case("empty_block_and_tail", 3300, 5, wide=1, empty_runs=((1024, 2048), (3290, 3300)), seed=32))
    c.append(Case("empty_everything", 1100, 2, empty_runs=((0, 1100),), seed=33))
    for i, p in enumerate((1, 2, 5, 64, 65, 256)):
        c.append(Case(f"parts{p}", 2500, p, wide=i % 2, bounds=("even", "gap")[p >= 5 and i % 2], seed=40 + i))
    c.append(Case("parts256_gap", 3000, 256, bounds="gap", seed=46))
    c.append(Case("all_to_last", 2100, 5, bounds="last", seed=47))
    c.append(Case("all_to_first", 2100, 64, bounds="first", wide=1, seed=48))
    for carry, cols in ((0, 4), (0, 5), (2, 5), (2, 7), (3, 5), (3, 7)):
        c.append(Case(f"carry{carry}_cols{cols}", 1300, 5, carry=carry, head_cols=cols, seed=50 + cols))
    c.append(Case("carry2_cols7_wide", 1300, 5, carry=2, head_cols=7, wide=1, seed=58))
    c.append(Case("wide_high_positions", 1300, 3, wide=1, table="high", seed=59))
    c.append(Case("null_tables", 700, 3, carry=2, table="null", seed=60))
    c.append(Case("null_tables_carry3", 700, 3, carry=3, table="null", seed=61))
    c.append(Case("boxes_ragged", 2600, 5, api="boxes", fit="ragged", bounds="gap", seed=62))
    c.append(Case("boxes_ragged_wide", 2600, 64, api="boxes", fit="ragged", bounds="gap", wide=1, seed=63))
    c.append(Case("boxes_ragged_carry0", 1200, 5, api="boxes", fit="ragged", carry=0, head_cols=4, seed=64))
    c.append(Case("two_batches", 1700, 5, batches=2, seed=65))
    c.append(Case("two_batches_boxes", 1700, 5, batches=2, api="boxes", fit="ragged", wide=1, seed=66))
    c.append(Case("paths", 1900, 5, api="paths", seed=67))
    c.append(Case("paths_carry0", 1100, 2, api="paths", carry=0, head_cols=4, seed=68))
    for i, fit in enumerate(("head", "pool", "both", "cap0")):
        c.append(Case(f"overflow_{fit}", 2300, 5, fit=fit, wide=i % 2, expect_overflow=True, seed=70 + i))
        c.append(Case(f"overflow_{fit}_boxes", 2300, 5, fit=fit, api="boxes", wide=1 - i % 2, expect_overflow=True,
                      seed=80 + i))
    c.append(Case("overflow_middle", 2300, 5, fit="middle", api="boxes", expect_overflow=True, seed=75))
    c.append(Case("overflow_two_batches", 1700, 3, fit="both", batches=2, expect_overflow=True, seed=76))
    c.append(Case("overflow_head_carry0", 1500, 5, fit="head", carry=0, head_cols=4, expect_overflow=True, seed=77))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def bounds_of(case: Case, n: int) -> np.ndarray:
    """the first vertex of every part, ascending"""
    P = case.n_parts
    if case.bounds == "last":
        return np.zeros(P, dtype=I64)
    if case.bounds == "first":
        return np.array([0] + [n] * (P - 1), dtype=I64)
    b = (np.arange(P, dtype=I64) * n) // P
    if case.bounds == "gap" and P >= 3:
        b[P - 1] = n  # the last part is empty: no vertex is >= n
        b[P // 2] = b[P // 2 + 1]  # and so is part P // 2: of parts with equal first vertices the last one owns
    return b


def empty_parts(bounds: np.ndarray, n: int) -> np.ndarray:
    return np.nonzero(np.append(bounds[1:], n) == bounds)[0]


def make_batch(case: Case, g: Graph, batch: int, n_rows: int, rows: np.ndarray):
    """-> head int64 [k, head_cols], next int32 [k], edge int64 [k]: unique rows, 64-bit keys with high bits set,
    steps up to WALK_LENGTH - 1, the previous vertex -1 (the high word all ones) on step 0"""
    rng = np.random.default_rng(1000 * case.seed + batch)
    k = case.k
    E = g.col.size
    edge = rng.integers(0, E, k)
    gad = rng.random(k) < case.gadgets
    if k >= len(GADGET_LENGTHS) and case.gadgets > 0:  # every gadget at least once, in every batch that has room
        gad[:len(GADGET_LENGTHS)] = True
        rng.shuffle(gad)
    which = np.array([g.gadget_edge[m] for m in GADGET_LENGTHS])
    pick = rng.integers(0, which.size, k)
    pick[np.nonzero(gad)[0][:which.size]] = np.arange(min(which.size, int(gad.sum())))
    edge = np.where(gad, which[pick], edge).astype(I64)
    v = (np.searchsorted(g.rowptr, edge, side="right") - 1).astype(I64)
    nxt = g.col[edge].astype(np.int32)
    u = rng.random(k)
    vanish = ~gad & (u < case.vanish)
    finish = ~gad & ~vanish & (u < case.vanish + case.finish)
    nxt[vanish] = -1
    step = rng.integers(0, WALK_LENGTH - 1, k)
    step[finish] = WALK_LENGTH - 1
    prev = rng.integers(0, g.n, k)
    prev[step == 0] = 0xFFFFFFFF
    head = rng.integers(-2 ** 62, 2 ** 62, (k, case.head_cols)).astype(I64)  # (the words a launch must overwrite)
    head[:, 0] = rows
    head[:, 1] = rng.integers(0, 2 ** 63 - 1, k) | (1 << 62) | np.where(rng.random(k) < 0.5, -2 ** 63, 0)
    head[:, 2] = (prev << 32) | v
    head[:, 3] = step
    empty = ~gad & (rng.random(k) < case.empty)
    for a, b in case.empty_runs:
        empty[a:b] = True
    head[empty, 0] = -1 - rng.integers(0, 1000, int(empty.sum()))
    return head, nxt, edge


@dataclass
class Built:
    case: Case
    g: Graph
    bounds: np.ndarray
    batches: list  # (head, next, edge) per batch
    routes: list
    expected: R.Expected
    table: Optional[np.ndarray]  # the list words handed to the kernel (uint16 / uint32), or None
    starts: Optional[np.ndarray]  # box_starts (boxes) or None
    cap: int
    wcap: int
    lay: tuple
    n_rows: int


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    case = CASES[CASE_IDS.index(name)]
    g = gadget_graph()
    bounds = bounds_of(case, g.n)
    null = case.table == "null"
    table = None if null or case.carry == 0 else (g.pos16 if not case.wide else
                                                  g.pos32_high if case.table == "high" else g.pos32)
    rng = np.random.default_rng(case.seed)
    n_rows = case.k * case.batches + 37
    all_rows = rng.permutation(n_rows)
    batches, routes = [], []
    for b in range(case.batches):
        head, nxt, edge = make_batch(case, g, b, n_rows, all_rows[b * case.k:(b + 1) * case.k])
        batches.append((head, nxt, edge))
        routes.append(R.route(head, nxt, edge, WALK_LENGTH, bounds, case.carry, None if null else g.edge_classes,
                              None if null else g.wedge_off))
    exp = R.expected_boxes(routes, case.n_parts, table if case.carry == 2 else None)
    P = case.n_parts
    nh, nw = exp.need[:P], exp.need[P:]
    starts, cap, wcap = None, 0, 0
    rng = np.random.default_rng(case.seed + 7)
    fit = case.fit
    busiest = int(np.argmax(nh))
    if case.api == "boxes":
        hc, wc = nh.copy(), nw.copy()
        if fit == "ragged":
            # some boxes exactly full, some with slack, a box of 0 slots / a pool of 0 words where none is needed
            hc += np.where(nh > 0, np.arange(P) % 4, 0)
            wc += np.where(nw > 0, np.arange(P) % 3 * 13, 0)
        elif fit == "head":
            hc = nh // 2
        elif fit == "pool":
            wc = nw // 2
        elif fit == "both":
            hc, wc = nh // 2, nw // 3
        elif fit == "cap0":
            hc = np.zeros(P, dtype=I64)
        elif fit == "middle":
            d = int(np.clip(busiest, 1, P - 2))
            hc[d], wc[d] = nh[d] // 2, nw[d] // 2
        # mailbox d is [starts[d], starts[d + 1]): back to back; the first may begin anywhere in the arrays
        h0, w0 = (3, 17) if fit == "ragged" else (0, 0)
        starts = np.concatenate([h0 + np.concatenate([[0], np.cumsum(hc)]),
                                 w0 + np.concatenate([[0], np.cumsum(wc)])]).astype(I64)
        lay = R.layout(P, starts=starts)
    else:
        cap, wcap = int(nh.max()), int(nw.max())
        if fit == "head":
            cap = cap // 2
        elif fit == "pool":
            wcap = wcap // 2
        elif fit == "both":
            cap, wcap = cap // 2, wcap // 3
        elif fit == "cap0":
            cap = 0
        lay = R.layout(P, cap=cap, wcap=wcap)
    return Built(case, g, bounds, batches, routes, exp, table, starts, cap, wcap, lay, n_rows)


def allocation(b: Built):
    """(slots, words, origin): sizes of the box arrays with their guards, and where the kernel's arrays begin.  A guard
    is at least as long as the longest list of the case (and 64 slots); behind the last box there is room for the
    FULL need of every destination from where its box starts, so that a kernel that ignored a capacity would
    write into guards, not out of the allocation."""
    P = b.case.n_parts
    hstart, hcap, wstart, wcap = b.lay
    guard = max(64, b.expected.longest)
    nh, nw = b.expected.need[:P], b.expected.need[P:]
    slots = int(max((hstart + np.maximum(hcap, nh + 1)).max(), 0)) + 2 * guard
    words = int(max((wstart + np.maximum(wcap, nw)).max(), 0)) + 3 * guard
    return slots, words, (guard, guard)
