"""The case table of the forwarding tests (tests/forward_cases.py) proved with the restatement alone
(tests/forward_restatement.py): no GPU.  What tests/test_forward_gpu.py runs through the kernels must contain what
it claims to contain -- every gadget length in both widths, overflow of every kind, first / last / empty
destinations hit or provably not -- and the judgment (check_boxes) must accept a correct mailbox filling and reject
corrupted ones, or the GPU tests could pass vacuously."""
import numpy as np
import pytest

import forward_cases as C
import forward_restatement as R

I64 = np.int64


def fill(b, seed=0):
    """a correct filling of the boxes of case `b`, in numpy: the walkers appended in a shuffled order, every one at
    the place and words its destination's counters give it, written only if both fit
    -> (box_head, box_off, box_words, box_count, status, logs)"""
    case, exp = b.case, b.expected
    P = case.n_parts
    slots, words, (gh, gw) = C.allocation(b)
    box_head = np.full((slots, case.head_cols), R.HEAD_SENTINEL, dtype=I64)
    box_off = np.full(slots, R.HEAD_SENTINEL, dtype=I64)
    box_words = np.full(words, R.WORD_SENTINEL, dtype=np.int32)
    count = np.zeros(2 * P, dtype=I64)
    hstart, hcap, wstart, wcap = b.lay
    status = 0
    rng = np.random.default_rng(seed)
    for r in b.routes:
        status |= R.ST_RANGE if r["range"] else 0
        for i in rng.permutation(np.nonzero(r["fwd"])[0]):
            d, n, s = int(r["dest"][i]), int(r["len"][i]), int(r["start"][i])
            pos, woff = int(count[d]), int(count[P + d])
            count[d] += 1
            count[P + d] += n
            if pos < hcap[d] and woff + n <= wcap[d]:
                h = gh + int(hstart[d]) + pos
                box_head[h, :] = 0
                c = min(case.head_cols, 5)
                box_head[h, :c] = r["head"][i, :c]
                box_off[h] = woff
                w = gw + int(wstart[d]) + woff
                box_words[w:w + n] = exp.table[s:s + n].astype(np.int32)
            else:
                status |= R.ST_OVERFLOW
    return box_head, box_off, box_words, count, status


SMALL = [n for n in C.CASE_IDS if C.CASES[C.CASE_IDS.index(n)].k <= 5000]


@pytest.mark.parametrize("name", SMALL)
def test_a_correct_filling_is_accepted_and_the_case_is_what_its_name_says(name):
    b = C.build(name)
    case = b.case
    P = case.n_parts
    bh, bo, bw, cnt, status = fill(b)
    R.check_boxes(b.expected, bh, bo, bw, cnt, b.lay, status, origin=C.allocation(b)[2],
                  want_range=any(r["range"] for r in b.routes))
    over_h, over_w = R.overflows(b.expected, b.lay)
    assert bool((over_h | over_w).any()) == case.expect_overflow == bool(status & R.ST_OVERFLOW)
    nh, nw = b.expected.need[:P], b.expected.need[P:]
    if case.fit in ("head", "cap0"):
        assert over_h.any() and not over_w.any()  # headers too small, the pools ample
        assert case.fit != "cap0" or int(b.lay[1].max()) == 0
    elif case.fit == "pool":
        assert over_w.any() and not over_h.any()
    elif case.fit == "both":
        assert bool((over_h & over_w).any())
    elif case.fit == "middle":
        d = int(np.nonzero(over_h)[0][0])
        assert over_h.sum() == 1 and over_w.sum() == 1 and over_w[d] and 0 < d < P - 1
        assert nh[d - 1] > 0 and nh[d + 1] > 0  # two that fit, and hold walkers, on either side
    elif case.fit == "ragged":
        hcap, wcap = b.lay[1], b.lay[3]
        assert bool((hcap == nh).any()) and bool((hcap > nh).any())  # exactly full boxes and boxes with slack
        assert case.bounds != "gap" or (bool((hcap == 0).any()) and (case.carry != 2 or bool((wcap == 0).any())))
    for head, nxt, edge in b.batches:
        assert not bool((head == R.HEAD_SENTINEL).any())  # no input word equals the sentinel
        live = head[:, 0] >= 0
        assert np.unique(head[live, 0]).size == int(live.sum())
        assert bool((head[:, 1] >> 62 != 0).any())  # keys with high bits set


def test_every_gadget_length_is_forwarded_in_both_widths():
    """lists of exactly 0, 1, 14, 15, 31, 32, 33, 63, 64, 65 and 200 entries (either side of the cut between the
    lane's copy and the wave's, and of the wave's stride of 64) leave in a carry 2 case of each width"""
    g = C.gadget_graph()
    for m in C.GADGET_LENGTHS:
        e = g.gadget_edge[m]
        assert int(g.edge_classes[e] & 0xFFFFFF) == m
    seen = {0: set(), 1: set()}
    for name in SMALL:
        b = C.build(name)
        if b.case.carry != 2 or b.case.table == "null":
            continue
        for d in range(b.case.n_parts):
            seen[b.case.wide] |= set(b.expected.len[d].tolist())
    for wide in (0, 1):
        assert set(C.GADGET_LENGTHS) <= seen[wide], (wide, sorted(set(C.GADGET_LENGTHS) - seen[wide]))
    # return counts above 1 and non-zero return positions occur among the gadget edges
    ge = np.array(list(g.gadget_edge.values()))
    assert int((g.edge_classes[ge] >> 24).max()) >= 2 and int((g.wedge_off[ge] >> np.uint64(40)).max()) > 0


def test_the_geometry_the_issue_names_is_in_the_table():
    ks = {c.k for c in C.CASES}
    assert {1, 63, 64, 65, 1023, 1024, 1025, 4097} <= ks
    assert C.K_BEYOND_GRID in ks and C.K_BEYOND_GRID >= 2 * C.RESIDENT_WALKERS + 1 and C.K_BEYOND_GRID % 1024 % 2 == 1
    assert {1, 2, 5, 64, 65, 256} <= {c.n_parts for c in C.CASES}
    combos = {(c.carry, c.head_cols) for c in C.CASES}
    assert {(0, 4), (0, 5), (2, 5), (2, 7), (3, 5), (3, 7)} <= combos
    assert {(c.carry, c.wide) for c in C.CASES} >= {(2, 0), (2, 1)}
    assert any(c.api == "boxes" for c in C.CASES) and any(c.api == "paths" for c in C.CASES)
    assert any(c.batches == 2 and not c.expect_overflow for c in C.CASES)
    # empty slots over a whole wave, a whole block of 1024 and the ragged tail
    b = C.build("empty_wave")
    assert bool((b.batches[0][0][128:192, 0] < 0).all())
    b = C.build("empty_block_and_tail")
    h = b.batches[0][0]
    assert bool((h[1024:2048, 0] < 0).all()) and bool((h[3290:, 0] < 0).all()) and h.shape[0] % 1024 != 0
    assert C.build("empty_everything").expected.need.sum() == 0


def test_first_last_and_empty_destinations_are_hit_or_provably_not():
    g = C.gadget_graph()
    for name in SMALL:
        b = C.build(name)
        case, P = b.case, b.case.n_parts
        nh = b.expected.need[:P]
        assert np.array_equal(b.bounds, np.sort(b.bounds)) and b.bounds[0] == 0
        empty = C.empty_parts(b.bounds, g.n)
        assert int(nh[empty].sum()) == 0  # an empty part owns nothing
        if case.table == "null" or name == "empty_everything":
            assert nh.sum() == 0
            continue
        if case.bounds == "gap" and P >= 3:
            assert P // 2 in empty and P - 1 in empty
        if case.bounds == "last":
            assert nh[P - 1] == nh.sum() > 0 and empty.size == P - 1
        elif case.bounds == "first":
            assert nh[0] == nh.sum() > 0 and empty.size == P - 1
        elif case.k >= 1000 and P <= 64:
            assert nh[0] > 0  # the first part is hit; the last one unless it is empty
            assert (nh[P - 1] > 0) != (P - 1 in empty)
    # the destinations against a search written out: the owner of x is the part whose range holds x
    b = C.build("parts256_gap")
    hi = np.append(b.bounds[1:], g.n)
    for x in (0, 1, 17, g.n // 2, g.n - 1):
        (own,) = np.nonzero((b.bounds <= x) & (x < hi))
        assert own.size == 1 and int(R.destination(b.bounds, np.array([x]))[0]) == int(own[0])


def test_a_32_bit_case_forwards_a_position_that_differs_from_its_low_16_bits():
    """In the gadget cases both widths hold the SAME positions (all below 65 536: the graph has 846 vertices), so a
    kernel that read the wrong width is caught by the element size -- it reads other words --, not by the value of a
    position.  The case with the table of a graph with wide rows (positions moved up by 70 000) forwards words that
    16 bits cannot hold; tests/test_partitioned_gpu.py walks a graph whose tables really hold such positions."""
    g = C.gadget_graph()
    assert int(g.pos32.max()) < 65536 and np.array_equal(g.pos16.astype(np.uint32), g.pos32)
    b = C.build("wide_high_positions")
    assert b.case.wide == 1 and b.table is g.pos32_high
    n_high = 0
    for d in range(b.case.n_parts):
        idx = R._ragged_index(b.expected.start[d], b.expected.len[d])
        w = b.expected.table[idx]
        n_high += int(((w & 0xFFFF) != w).sum())
    assert n_high > 1000


def test_check_boxes_rejects_corrupted_outputs():
    b = C.build("carry2_cols5")
    origin = C.allocation(b)[2]
    P = b.case.n_parts
    hstart, hcap, wstart, wcap = b.lay

    def judge(bh, bo, bw, cnt, status):
        R.check_boxes(b.expected, bh, bo, bw, cnt, b.lay, status, origin=origin)

    good = fill(b)
    judge(*good)
    d = int(np.argmax(b.expected.need[:P]))
    h0, w0 = origin[0] + int(hstart[d]), origin[1] + int(wstart[d])

    def corrupt(f):
        bh, bo, bw, cnt, status = (x.copy() if isinstance(x, np.ndarray) else x for x in good)
        out = f(bh, bo, bw, cnt)
        with pytest.raises(AssertionError):
            judge(bh, bo, bw, cnt, status if out is None else out)

    slot = h0 + int(np.argmax(b.expected.len[d][np.searchsorted(b.expected.rows[d], good[0][h0:h0 + hcap[d], 0])] > 3))

    def shifted(bh, bo, bw, cnt):  # a list shifted by one word
        bo[slot] += 1

    def shifted_words(bh, bo, bw, cnt):  # ... or its words moved while the start stays
        bw[w0:w0 + wcap[d]] = np.roll(bw[w0:w0 + wcap[d]], 1)

    def duplicate(bh, bo, bw, cnt):  # a walker twice: over its neighbour in the same box, and in another box
        bh[h0 + 1], bo[h0 + 1] = bh[h0], bo[h0]

    def duplicate_elsewhere(bh, bo, bw, cnt):
        d2 = (d + 1) % P
        bh[origin[0] + int(hstart[d2])] = bh[h0]

    def in_guard(bh, bo, bw, cnt):
        bh[origin[0] - 1] = bh[h0]

    def in_last_guard(bh, bo, bw, cnt):
        bh[-1, 2] = 7

    def word_in_guard(bh, bo, bw, cnt):
        bw[origin[1] + int(wstart[-1] + wcap[-1])] = 3

    def short_count(bh, bo, bw, cnt):
        cnt[d] -= 1

    def short_words(bh, bo, bw, cnt):
        cnt[P + d] -= 1

    def lost_walker(bh, bo, bw, cnt):
        bh[h0 + 2], bo[h0 + 2] = R.HEAD_SENTINEL, R.HEAD_SENTINEL

    def header_word(bh, bo, bw, cnt):
        bh[h0 + 3, 4] ^= 1 << 40

    def spurious_overflow(bh, bo, bw, cnt):
        return R.ST_OVERFLOW

    for f in (shifted, shifted_words, duplicate, duplicate_elsewhere, in_guard, in_last_guard, word_in_guard,
              short_count, short_words, lost_walker, header_word, spurious_overflow):
        corrupt(f)
    # an overflowing case: the OVERFLOW bit missing, a count that reports only what fitted
    for name in ("overflow_head", "overflow_pool_boxes"):
        o = C.build(name)
        bh, bo, bw, cnt, status = fill(o)
        org = C.allocation(o)[2]
        R.check_boxes(o.expected, bh, bo, bw, cnt, o.lay, status, origin=org)
        with pytest.raises(AssertionError):
            R.check_boxes(o.expected, bh, bo, bw, cnt, o.lay, status & ~R.ST_OVERFLOW, origin=org)
        fitted = np.minimum(cnt, np.concatenate([o.lay[1], o.lay[3]]))
        with pytest.raises(AssertionError):
            R.check_boxes(o.expected, bh, bo, bw, fitted, o.lay, status, origin=org)
    # header overflow alone: a slot left free although walkers were turned away
    o = C.build("overflow_head")
    bh, bo, bw, cnt, status = fill(o)
    org = C.allocation(o)[2]
    dd = int(np.nonzero(R.overflows(o.expected, o.lay)[0])[0][0])
    bh[org[0] + int(o.lay[0][dd])], bo[org[0] + int(o.lay[0][dd])] = R.HEAD_SENTINEL, R.HEAD_SENTINEL
    with pytest.raises(AssertionError):
        R.check_boxes(o.expected, bh, bo, bw, cnt, o.lay, status, origin=org)


def test_the_paths_form_and_the_logs_are_restated():
    b = C.build("paths")
    walks, valid = R.expected_paths(b.routes, b.n_rows, C.WALK_LENGTH)
    head, nxt, _ = b.batches[0]
    live = head[:, 0] >= 0
    went = live & (nxt >= 0)
    assert int((walks != R.WORD_SENTINEL).sum()) == int(went.sum()) > 0
    assert int((valid == 0).sum()) == int((live & (nxt < 0)).sum()) > 0
    i = int(np.nonzero(went)[0][0])
    assert walks[head[i, 0], head[i, 3] + 1] == nxt[i]
    r = b.routes[0]
    log = np.full((head.shape[0], 3), R.HEAD_SENTINEL, dtype=I64)
    log[r["live"]] = r["log"][r["live"]]
    R.check_log(r, log)
    log[i, 2] += 1
    with pytest.raises(AssertionError):
        R.check_log(r, log)
