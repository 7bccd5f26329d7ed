"""The mailbox contract of n2v_partition_forward / n2v_partition_forward_boxes, restated: numpy only.

What csrc/n2v_partition.hip (the forward kernel, and route + group + gather as a second witness) is held to
(tests/test_forward_host.py, tests/test_forward_gpu.py).  Written from include/n2v_hip.h, not from the kernel,
and importing nothing of the package:

  a walker is a header (row, key, s << 32 | v, step[, classes, ...]), the vertex `next` it drew and the edge it
  drew it along.  A header whose row is negative is an EMPTY SLOT: nothing is logged or forwarded for it.

  log          (row, step + 1, next), or (row, -1, -1) when next < 0 (it vanished on arrival)
  forwarded    next >= 0 and step + 1 < walk_length
  destination  the last part whose first vertex is <= next (an empty part owns nothing)
  header out   (row, key, v << 32 | next, step + 1, edge_classes[e] | return position << 32, 0 ...);
               with carry 0 nothing of an edge travels: the fifth word is 0 as well
  list         carry 2: the shared count of edge_classes[e] words from wedge_off[e] & (2^40 - 1); carry 0 and 3: none
  NULL tables with carry >= 2: nobody is forwarded, the logs are written, N2V_ST_RANGE is reported

  a mailbox    appended to in any order; box_count = walkers per destination, then words per destination: the FULL
               need, whether it fits or not; N2V_ST_OVERFLOW if and only if some need exceeds its capacity; nothing
               is written outside the boxes; what is written is whole walkers (header, list start, list)

Not a test module: helpers shared by the two.
"""
import numpy as np

ST_RANGE, ST_OVERFLOW = 2, 4
EC_SHARED_MASK = 0xFFFFFF
WEDGE_OFF_MASK = (1 << 40) - 1
WEDGE_RPOS_SHIFT = 40

# what boxes, guards, logs and output rows are filled with before a launch: no row, list start, position, step or
# vertex is negative, so no header (its first word is the row), list start or word can equal its sentinel
HEAD_SENTINEL = -0x5A5A5A5A5A5A5A5B
WORD_SENTINEL = -0x5A5A5A5B
BYTE_SENTINEL = 0x5A

I64 = np.int64


def _i64(a):
    a = np.asarray(a)
    assert a.dtype == I64, a.dtype
    return a


def destination(bounds, nxt):
    """the last part whose first vertex is <= next: of parts with equal first vertices (all but the last of them
    are empty) the last one"""
    return np.searchsorted(_i64(bounds), np.asarray(nxt, dtype=I64), side="right") - 1


def route(head, nxt, edge, walk_length, bounds, carry, edge_classes, wedge_off):
    """per walker: dict of
      live [k] bool      not an empty slot
      log [k, 3]         the path record (rows of empty slots: undefined, see `live`)
      fwd [k] bool       forwarded
      dest [k]           its destination (-1 when not forwarded)
      head [k, 5]        the first five words of the outgoing header (further words are 0)
      len, start [k]     the list that travels: words, and where it starts in the wedge table
      range bool         N2V_ST_RANGE is expected (somebody would have been forwarded, but the tables are NULL)"""
    head = _i64(head)
    k = head.shape[0]
    nxt = np.asarray(nxt).astype(I64)
    assert carry in (0, 2, 3)
    row, key = head[:, 0], head[:, 1]
    v = head[:, 2] & 0xFFFFFFFF
    step = head[:, 3]
    live = row >= 0
    gone = nxt < 0
    log = np.stack([row, np.where(gone, -1, step + 1), np.where(gone, -1, nxt)], 1)
    fwd = live & ~gone & (step + 1 < walk_length)
    no_tables = carry >= 2 and (edge_classes is None or wedge_off is None)
    want_range = bool(no_tables and fwd.any())
    if no_tables:
        fwd = np.zeros(k, dtype=bool)
    dest = np.where(fwd, destination(bounds, np.where(gone, 0, nxt)), -1)
    extra = np.zeros(k, dtype=I64)
    length = np.zeros(k, dtype=I64)
    start = np.zeros(k, dtype=I64)
    if carry >= 2 and not no_tables:
        e = np.where(fwd, _i64(edge), 0)
        if len(edge_classes):
            ec = np.asarray(edge_classes).astype(I64)[e]
            raw = np.asarray(wedge_off).astype(np.uint64)[e]
            extra = np.where(fwd, ec | ((raw >> np.uint64(WEDGE_RPOS_SHIFT)).astype(I64) << 32), 0)
            if carry == 2:
                start = np.where(fwd, (raw & np.uint64(WEDGE_OFF_MASK)).astype(I64), 0)
                length = np.where(fwd, ec & EC_SHARED_MASK, 0)
    out = np.stack([row, key, (v << 32) | (nxt & 0xFFFFFFFF), step + 1, extra], 1)
    return dict(live=live, log=log, fwd=fwd, dest=dest, head=out, len=length, start=start, range=want_range)


class Expected:
    """per destination d: rows[d] ascending (the key of the set), head[d] [n, 5], start[d] / len[d] of every list in
    `table`; need [2 * n_parts]: walkers per destination, then words per destination"""

    def __init__(self, n_parts, rows, head, start, length, table):
        self.n_parts, self.rows, self.head, self.start, self.len, self.table = n_parts, rows, head, start, length, table
        self.need = np.array([r.size for r in rows] + [int(x.sum()) for x in length], dtype=I64)
        self.longest = max([int(x.max()) for x in length if x.size] + [0])

    def entries(self, d):
        """the set itself, for small cases: {row: (header, list)}"""
        return {int(r): (tuple(int(x) for x in h), tuple(int(x) for x in self.table[s:s + n]))
                for r, h, s, n in zip(self.rows[d], self.head[d], self.start[d], self.len[d])}


def expected_boxes(routes, n_parts, table):
    """what the boxes must hold after all of `routes` (one route(), or several appended to the same boxes) --
    `table`: the wedge table the lists are cut from (any integer type; None when nothing travels)"""
    if isinstance(routes, dict):
        routes = [routes]
    fwd = np.concatenate([r["fwd"] for r in routes])
    dest = np.concatenate([r["dest"] for r in routes])[fwd]
    head = np.concatenate([r["head"] for r in routes])[fwd]
    start = np.concatenate([r["start"] for r in routes])[fwd]
    length = np.concatenate([r["len"] for r in routes])[fwd]
    assert np.unique(head[:, 0]).size == head.shape[0], "rows must be unique"
    table = np.zeros(0, dtype=I64) if table is None else np.asarray(table).astype(I64)
    assert not length.size or int((start + length).max()) <= table.size
    order = np.lexsort((head[:, 0], dest))
    dest, head, start, length = dest[order], head[order], start[order], length[order]
    cuts = np.searchsorted(dest, np.arange(n_parts + 1))
    sl = [slice(cuts[d], cuts[d + 1]) for d in range(n_parts)]
    return Expected(n_parts, [head[s, 0] for s in sl], [head[s] for s in sl], [start[s] for s in sl],
                    [length[s] for s in sl], table)


def layout(n_parts, starts=None, cap=None, wcap=None):
    """(hstart, hcap, wstart, wcap) per destination, from box_starts [2 n_parts + 2] or the equal shares"""
    if starts is not None:
        s = _i64(starts)
        assert s.size == 2 * n_parts + 2
        h, w = s[:n_parts + 1], s[n_parts + 1:]
        return h[:-1], np.diff(h), w[:-1], np.diff(w)
    d = np.arange(n_parts, dtype=I64)
    return d * cap, np.full(n_parts, cap, I64), d * wcap, np.full(n_parts, wcap, I64)


def overflows(expected, lay):
    """(header overflow, pool overflow) per destination, from the restatement's numbers alone"""
    _, hcap, _, wcap = lay
    P = expected.n_parts
    return expected.need[:P] > hcap, expected.need[P:] > wcap


def _ragged_index(start, length):
    """indices start[i] .. start[i] + length[i] of every i, back to back"""
    total = int(length.sum())
    if total == 0:
        return np.zeros(0, dtype=I64)
    first = np.cumsum(length) - length
    return np.repeat(start - first, length) + np.arange(total, dtype=I64)


def check_boxes(expected, box_head, box_off, box_words, box_count, lay, status, origin=(0, 0), want_range=False):
    """The judgment, fitting or overflowing.  box_head [slots, head_cols], box_off [slots], box_words [words]: the
    WHOLE allocations, guards included, as numpy; `origin` = (slot, word) at which the arrays handed to the kernel
    begin inside them; lay = layout(...).  Raises AssertionError with what is wrong."""
    P = expected.n_parts
    box_head, box_off = _i64(box_head), _i64(box_off)
    box_words = np.asarray(box_words).astype(I64)
    head_cols = box_head.shape[1]
    hstart, hcap, wstart, wcap = lay
    need = expected.need
    got = np.asarray(box_count).astype(I64)
    assert np.array_equal(got[:P], need[:P]), ("walkers per destination", got[:P].tolist(), need[:P].tolist())
    assert np.array_equal(got[P:2 * P], need[P:]), ("words per destination", got[P:].tolist(), need[P:].tolist())
    over_h, over_w = overflows(expected, lay)
    want_status = (ST_OVERFLOW if bool((over_h | over_w).any()) else 0) | (ST_RANGE if want_range else 0)
    assert int(status) == want_status, ("status word", int(status), want_status)
    in_box_h = np.zeros(box_off.size, dtype=bool)
    in_box_w = np.zeros(box_words.size, dtype=bool)
    seen = []
    for d in range(P):
        h0, w0 = origin[0] + int(hstart[d]), origin[1] + int(wstart[d])
        hc, wc = int(hcap[d]), int(wcap[d])
        assert 0 <= h0 and h0 + hc <= box_off.size and 0 <= w0 and w0 + wc <= box_words.size
        in_box_h[h0:h0 + hc] = True
        in_box_w[w0:w0 + wc] = True
        hd, off, words = box_head[h0:h0 + hc], box_off[h0:h0 + hc], box_words[w0:w0 + wc]
        occ = hd[:, 0] != HEAD_SENTINEL
        assert bool((hd[~occ] == HEAD_SENTINEL).all()) and bool((off[~occ] == HEAD_SENTINEL).all()), \
            ("destination", d, "a slot without a row holds something")
        rows = hd[occ, 0]
        at = np.searchsorted(expected.rows[d], rows)
        ok = (at < expected.rows[d].size)
        ok[ok] = expected.rows[d][at[ok]] == rows[ok]
        assert bool(ok.all()), ("destination", d, "holds walkers that do not belong there", rows[~ok][:8].tolist())
        assert np.unique(rows).size == rows.size, ("destination", d, "a walker appears twice")
        seen.append(rows)
        want_head = np.zeros((rows.size, head_cols), dtype=I64)
        c = min(head_cols, 5)
        want_head[:, :c] = expected.head[d][at, :c]
        bad = (hd[occ] != want_head).any(1)
        assert not bool(bad.any()), ("destination", d, "header differs", hd[occ][bad][:4].tolist(),
                                     want_head[bad][:4].tolist())
        o, n, s = off[occ], expected.len[d][at], expected.start[d][at]
        assert bool(((o >= 0) & (o + n <= wc)).all()), ("destination", d, "a list leaves the pool")
        by = np.argsort(o, kind="stable")
        nz = by[n[by] > 0]
        assert bool((o[nz][:-1] + n[nz][:-1] <= o[nz][1:]).all()), ("destination", d, "lists overlap")
        idx = _ragged_index(o, n)
        bad = words[idx] != expected.table[_ragged_index(s, n)]
        assert not bool(bad.any()), ("destination", d, "list words differ", int(bad.sum()))
        covered = np.zeros(wc, dtype=bool)
        covered[idx] = True
        assert bool((words[~covered] == WORD_SENTINEL).all()), ("destination", d, "words that belong to no walker")
        n_h, n_w = int(need[d]), int(need[P + d])
        if not over_h[d] and not over_w[d]:
            assert rows.size == n_h and bool(occ[:n_h].all()), ("destination", d, "fits but is not whole")
            assert bool(covered[:n_w].all()) and int(n.sum()) == n_w, ("destination", d, "lists do not tile the pool")
        elif over_h[d] and not over_w[d]:
            assert bool(occ.all()), ("destination", d, "header overflow alone: every slot must be used")
    rows = np.concatenate(seen) if seen else np.zeros(0, dtype=I64)
    assert np.unique(rows).size == rows.size, "a walker appears in two mailboxes"
    assert bool((box_head[~in_box_h] == HEAD_SENTINEL).all()), "a header outside every mailbox"
    assert bool((box_off[~in_box_h] == HEAD_SENTINEL).all()), "a list start outside every mailbox"
    assert bool((box_words[~in_box_w] == WORD_SENTINEL).all()), "a word outside every pool"


def check_log(r, log):
    """the path records: row i of every live walker, the sentinel in the rows of empty slots"""
    log = _i64(log)
    live = r["live"]
    assert np.array_equal(log[live], r["log"][live]), "path records differ"
    assert bool((log[~live] == HEAD_SENTINEL).all()), "a path record for an empty slot"


def expected_paths(routes, n_rows, walk_length):
    """the log_out == NULL form: walks_out [n_rows][walk_length + 1] int32 and valid_out [n_rows] uint8, every cell at
    its sentinel except walks_out[row][step + 1] = next, and valid_out[row] = 0 of a walker that vanished"""
    if isinstance(routes, dict):
        routes = [routes]
    walks = np.full((n_rows, walk_length + 1), WORD_SENTINEL, dtype=np.int32)
    valid = np.full(n_rows, BYTE_SENTINEL, dtype=np.uint8)
    for r in routes:
        lg = r["log"][r["live"]]
        went = lg[:, 1] >= 0
        walks[lg[went, 0], lg[went, 1]] = lg[went, 2].astype(np.int32)
        valid[lg[~went, 0]] = 0
    return walks, valid
