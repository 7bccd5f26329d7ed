"""The forwarding kernels of graph-partitioned walking (csrc/n2v_partition.hip) held to their mailbox contract:
the case table of tests/forward_cases.py through n2v_partition_forward / n2v_partition_forward_boxes, judged by
tests/forward_restatement.py (written from include/n2v_hip.h; tests/test_forward_host.py proves the table and the
judgment without a GPU) -- overflowing boxes, both list widths, 1 .. 256 destinations, batches of 1 .. 1 052 675
walkers, empty slots, lists on either side of the 32-word cut.  Every box array lies between guards filled with a
sentinel and has room for the full need behind every box: a wrong kernel writes into guards, never out of an
allocation.  Route + group + gather is the second witness; n2v_partition_group and n2v_gather_wedges are checked on
their own at their limits.  Everything is an equality on integers."""
import numpy as np
import pytest
import torch

import forward_cases as C
import forward_restatement as R

pytestmark = pytest.mark.gpu

I64 = np.int64


def _dev(a):
    """numpy -> cuda, unsigned types through the signed view of the same width"""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def tables():
    g = C.gadget_graph()
    return dict(ec=_dev(g.edge_classes), off=_dev(g.wedge_off), pos16=_dev(g.pos16), pos32=_dev(g.pos32),
                high=_dev(g.pos32_high))


def _table_of(b, tables):
    if b.table is None:
        return None
    return tables["pos16"] if not b.case.wide else tables["high"] if b.case.table == "high" else tables["pos32"]


def _forward(b, tables):
    """the case through the kernel -> numpy (box_head, box_off, box_words, box_count, status, logs, walks, valid)"""
    from node2vec_amd import _lib

    L = _lib.load()
    case = b.case
    P, cols = case.n_parts, case.head_cols
    slots, words, (gh, gw) = C.allocation(b)
    box_head = torch.full((slots, cols), R.HEAD_SENTINEL, dtype=torch.int64, device="cuda")
    box_off = torch.full((slots,), R.HEAD_SENTINEL, dtype=torch.int64, device="cuda")
    box_words = torch.full((words,), R.WORD_SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.zeros(2 * P, dtype=torch.int64, device="cuda")  # zeroed ONCE: batches append
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    bounds = _dev(b.bounds)
    null = case.table == "null"
    ec = None if null or case.carry == 0 else tables["ec"]
    off = None if null or case.carry == 0 else tables["off"]
    pos = None if null else _table_of(b, tables)
    starts = None if b.starts is None else _dev(b.starts)
    walks = valid = None
    if case.api == "paths":
        walks = torch.full((b.n_rows, C.WALK_LENGTH + 1), R.WORD_SENTINEL, dtype=torch.int32, device="cuda")
        valid = torch.full((b.n_rows,), R.BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    logs = []
    stream = _lib.current_stream_ptr()
    for head, nxt, edge in b.batches:
        head_d, nxt_d = _dev(head), _dev(nxt)
        edge_d = None if case.carry == 0 else _dev(edge)
        log = None
        if case.api != "paths":
            log = torch.full((case.k, 3), R.HEAD_SENTINEL, dtype=torch.int64, device="cuda")
        common = (head_d.data_ptr(), cols, nxt_d.data_ptr(), _ptr(edge_d), case.k, C.WALK_LENGTH, bounds.data_ptr(), P,
                  case.carry, _ptr(ec), _ptr(off), _ptr(pos), case.wide, box_head[gh:].data_ptr(),
                  box_off[gh:].data_ptr(), box_words[gw:].data_ptr(), count.data_ptr())
        if case.api == "boxes":
            rc = L.n2v_partition_forward_boxes(*common, starts.data_ptr(), log.data_ptr(), status.data_ptr(), stream)
        else:
            rc = L.n2v_partition_forward(*common, b.cap, b.wcap, _ptr(log), _ptr(walks), _ptr(valid),
                                         status.data_ptr(), stream)
        assert rc == 0, rc
        logs.append(log)
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return (n(box_head), n(box_off), n(box_words), n(count), int(status[0].item()), [n(x) for x in logs], n(walks),
            n(valid))


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_forwarding_fills_the_mailboxes_as_the_contract_says(name, tables):
    """Every case of the table: counts = the full need, N2V_ST_OVERFLOW exactly when a need exceeds a capacity, whole
    walkers only, lists word for word, nothing outside the boxes, the path records equal.  `beyond_grid` runs the
    grid-stride loop five times, the last pass ragged: on the MI355X the launch rule gives 256 resident blocks of
    1024 walkers (256 CUs x 1 block: the occupancy query's answer) = 262 144 walkers per pass, and the case has
    1 052 675 = 4 x 262 144 + 4099."""
    b = C.build(name)
    bh, bo, bw, cnt, status, logs, walks, valid = _forward(b, tables)
    P = b.case.n_parts
    print(name, "need", b.expected.need[:P].sum(), b.expected.need[P:].sum(), "counted", cnt[:P].sum(), cnt[P:].sum(),
          "status", status)
    R.check_boxes(b.expected, bh, bo, bw, cnt, b.lay, status, origin=C.allocation(b)[2],
                  want_range=any(r["range"] for r in b.routes))
    if b.case.api == "paths":
        want_walks, want_valid = R.expected_paths(b.routes, b.n_rows, C.WALK_LENGTH)
        assert np.array_equal(walks, want_walks) and np.array_equal(valid, want_valid)
    else:
        for r, log in zip(b.routes, logs):
            R.check_log(r, log)


def _canonical(rows, head, lens, words_at, words):
    """a destination's walkers by ascending row: headers, list lengths, the list words back to back"""
    order = np.argsort(rows, kind="stable")
    return head[order], lens[order], words[R._ragged_index(words_at[order], lens[order])]


WITNESS = [c.name for c in C.CASES if not c.expect_overflow and c.n_parts <= 64 and c.table != "null"
           and c.api != "paths" and c.k <= 5000]


@pytest.mark.parametrize("name", WITNESS)
def test_route_group_and_gather_deliver_the_same_sets(name, tables):
    """the launch-per-stage routing on the same batches (the walkers that are no empty slots): the same walkers,
    headers and lists per destination as the restatement, and cuts = the running sum of its counts"""
    from node2vec_amd import _lib

    L = _lib.load()
    b = C.build(name)
    case = b.case
    P, cols, carry = case.n_parts, case.head_cols, case.carry
    stream = _lib.current_stream_ptr()
    bounds = _dev(b.bounds)
    got = [[] for _ in range(P)]
    total = np.zeros(P + 1, dtype=I64)
    for head, nxt, edge in b.batches:
        live = head[:, 0] >= 0
        k = int(live.sum())
        if k == 0:
            continue
        head_d, nxt_d, edge_d = _dev(head[live]), _dev(nxt[live]), _dev(edge[live])
        log = torch.empty((k, 3), dtype=torch.int64, device="cuda")
        ho = torch.full((k, cols), 7, dtype=torch.int64, device="cuda")
        dest = torch.empty(k, dtype=torch.int32, device="cuda")
        ln = torch.empty(k, dtype=torch.int64, device="cuda")
        src = torch.empty(k, dtype=torch.int64, device="cuda")
        _lib.check(L.n2v_partition_route(head_d.data_ptr(), cols, nxt_d.data_ptr(), edge_d.data_ptr(), k, C.WALK_LENGTH,
                                         bounds.data_ptr(), P, carry, 0, 0, tables["ec"].data_ptr(), log.data_ptr(),
                                         ho.data_ptr(), dest.data_ptr(), ln.data_ptr(), src.data_ptr(), stream), "route")
        work = torch.empty(((k + 255) // 256 + 1) * (P + 1), dtype=torch.int64, device="cuda")
        hg, lg, sg = torch.empty_like(ho), torch.empty_like(ln), torch.empty_like(src)
        cuts = torch.empty(P + 1, dtype=torch.int64, device="cuda")
        _lib.check(L.n2v_partition_group(dest.data_ptr(), ho.data_ptr(), cols, ln.data_ptr(), src.data_ptr(), k, P,
                                         work.data_ptr(), hg.data_ptr(), lg.data_ptr(), sg.data_ptr(), cuts.data_ptr(),
                                         stream), "group")
        cuts_h = cuts.cpu().numpy()
        k2 = int(cuts_h[P])
        ptr = torch.zeros(k2 + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lg[:k2], 0, out=ptr[1:])
        out = torch.full((max(int(ptr[-1]), 1),), R.WORD_SENTINEL, dtype=torch.int32, device="cuda")
        if carry >= 2 and k2:
            _lib.check(L.n2v_gather_wedges(tables["ec"].data_ptr(), tables["off"].data_ptr(),
                                           _table_of(b, tables).data_ptr(), case.wide, sg.data_ptr(), ptr.data_ptr(), k2,
                                           out.data_ptr(), hg.data_ptr(), cols, stream), "gather")
        torch.cuda.synchronize()
        r = R.route(head[live], nxt[live], edge[live], C.WALK_LENGTH, b.bounds, carry, C.gadget_graph().edge_classes,
                    C.gadget_graph().wedge_off)
        assert np.array_equal(log.cpu().numpy(), r["log"])
        assert np.array_equal(dest.cpu().numpy(), np.where(r["fwd"], r["dest"], P))
        hg_h, lg_h, ptr_h, out_h = hg.cpu().numpy(), lg.cpu().numpy(), ptr.cpu().numpy(), out.cpu().numpy()
        for d in range(P):
            s = slice(int(cuts_h[d]), int(cuts_h[d + 1]))
            got[d].append((hg_h[s], lg_h[s], out_h[R._ragged_index(ptr_h[:-1][s], lg_h[s])].astype(I64)))
        total += cuts_h
    exp = b.expected
    assert np.array_equal(total[1:] - total[:-1], exp.need[:P]) and total[0] == 0  # the cuts
    for d in range(P):
        head = np.concatenate([x[0] for x in got[d]]) if got[d] else np.zeros((0, cols), dtype=I64)
        lens = np.concatenate([x[1] for x in got[d]]) if got[d] else np.zeros(0, dtype=I64)
        words = np.concatenate([x[2] for x in got[d]]) if got[d] else np.zeros(0, dtype=I64)
        h, n, w = _canonical(head[:, 0], head, lens, np.cumsum(lens) - lens, words)
        want = np.zeros((exp.rows[d].size, cols), dtype=I64)
        want[:, :min(cols, 5)] = exp.head[d][:, :min(cols, 5)]
        assert np.array_equal(h, want), d
        assert np.array_equal(n, exp.len[d]), d
        assert np.array_equal(w, exp.table[R._ragged_index(exp.start[d], exp.len[d])]), d


def test_the_numpy_tables_equal_what_the_device_builds():
    """edge_classes, wedge_off and the lists of the gadget graph as computed in numpy from the definition, against
    n2v_edge_classes_build + n2v_wedge_build in both uniform widths (the return position is compared where the
    return count is not 0: only there does the header give it a meaning)"""
    from node2vec_amd.graph import DeviceGraph

    g = C.gadget_graph()
    for wide in (False, True):
        dg = DeviceGraph(_dev(g.rowptr), _dev(g.col), None)
        dg.build_wedges(wide=wide, slots=False)
        assert dg.wedge_off is not None and dg.wedge_mode == int(wide)
        assert np.array_equal(dg.edge_classes.cpu().numpy().view(np.uint32), g.edge_classes)
        off = dg.wedge_off.cpu().numpy().view(np.uint64)
        mask = np.uint64(R.WEDGE_OFF_MASK)
        assert np.array_equal(off & mask, g.wedge_off & mask)
        back = (g.edge_classes >> 24) > 0
        assert back.any() and np.array_equal(off[back], g.wedge_off[back])
        pos = dg.wedge_pos.cpu().numpy()
        assert pos.dtype == (np.int32 if wide else np.int16)
        assert np.array_equal(pos.view(np.uint32 if wide else np.uint16)[:g.pos32.size], g.pos32 if wide else g.pos16)


@pytest.mark.parametrize("n_parts", [1, 2, 64])
def test_group_equals_a_stable_sort(n_parts):
    """n2v_partition_group at its limit of 64 parts and at sizes around its blocks of 256 (4 waves rank inside a
    block), against torch's stable sort; every walker to one destination; nobody forwarded; 65 parts are refused"""
    from node2vec_amd import _lib

    L = _lib.load()
    cols = 5
    gen = torch.Generator().manual_seed(n_parts)
    stream = _lib.current_stream_ptr()

    def group(dest, parts=n_parts):
        k = dest.numel()
        head = torch.randint(-2 ** 62, 2 ** 62, (k, cols), generator=gen).cuda()
        ln = torch.randint(0, 1 << 40, (k,), generator=gen).cuda()
        src = torch.randint(0, 1 << 40, (k,), generator=gen).cuda()
        dest = dest.to(torch.int32).cuda()
        work = torch.empty(((k + 255) // 256 + 1) * (parts + 1), dtype=torch.int64, device="cuda")
        hg, lg, sg = torch.full_like(head, -3), torch.full_like(ln, -3), torch.full_like(src, -3)
        cuts = torch.full((parts + 1,), -3, dtype=torch.int64, device="cuda")
        rc = L.n2v_partition_group(dest.data_ptr(), head.data_ptr(), cols, ln.data_ptr(), src.data_ptr(), k, parts,
                                   work.data_ptr(), hg.data_ptr(), lg.data_ptr(), sg.data_ptr(), cuts.data_ptr(), stream)
        if rc != 0:
            return rc
        ds, order = torch.sort(dest, stable=True)
        assert torch.equal(hg, head[order]) and torch.equal(lg, ln[order]) and torch.equal(sg, src[order])
        assert torch.equal(cuts, torch.searchsorted(ds, torch.arange(parts + 1, dtype=torch.int32, device="cuda")))
        return 0

    for k in (1, 255, 256, 257, 1025, 70_001):
        assert group(torch.randint(0, n_parts + 1, (k,), generator=gen)) == 0
        assert group(torch.full((k,), n_parts - 1)) == 0  # every walker to one destination (the last part)
        assert group(torch.zeros(k, dtype=torch.int64)) == 0  # ... to the first
        assert group(torch.full((k,), n_parts)) == 0  # nobody forwarded
    assert group(torch.zeros(300, dtype=torch.int64), parts=65) == -1  # N2V_EINVAL


def test_gather_wedges_copies_32_bit_lists(tables):
    """n2v_gather_wedges with wide = 1 on the table whose positions need more than 16 bits, against the numpy lists:
    every gadget edge (lists of 0 .. 200 entries around the wave's stride) and 3000 others, in a shuffled order"""
    from node2vec_amd import _lib

    L = _lib.load()
    g = C.gadget_graph()
    rng = np.random.default_rng(4)
    edges = np.concatenate([np.array(list(g.gadget_edge.values())), rng.integers(0, g.col.size, 3000)]).astype(I64)
    rng.shuffle(edges)
    lens = (g.edge_classes[edges] & 0xFFFFFF).astype(I64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(I64)
    start = (g.wedge_off[edges] & np.uint64(R.WEDGE_OFF_MASK)).astype(I64)
    want = g.pos32_high[R._ragged_index(start, lens)].astype(I64)
    assert int(want.max()) >= 65536
    k = edges.size
    for wide, table, ref in ((1, tables["high"], want), (0, tables["pos16"],
                                                          g.pos16[R._ragged_index(start, lens)].astype(I64))):
        out = torch.full((int(ptr[-1]) + 64,), R.WORD_SENTINEL, dtype=torch.int32, device="cuda")
        head = torch.full((k, 6), 11, dtype=torch.int64, device="cuda")
        edges_d, ptr_d = _dev(edges), _dev(ptr)
        _lib.check(L.n2v_gather_wedges(tables["ec"].data_ptr(), tables["off"].data_ptr(), table.data_ptr(), wide,
                                       edges_d.data_ptr(), ptr_d.data_ptr(), k, out.data_ptr(), head.data_ptr(), 6,
                                       _lib.current_stream_ptr()), "gather")
        out_h, head_h = out.cpu().numpy().astype(I64), head.cpu().numpy()
        assert np.array_equal(out_h[:ref.size], ref) and bool((out_h[ref.size:] == R.WORD_SENTINEL).all())
        rpos = (g.wedge_off[edges] >> np.uint64(40)).astype(I64)
        assert np.array_equal(head_h[:, 4], g.edge_classes[edges].astype(I64) | rpos << 32)
        assert bool((head_h[:, [0, 1, 2, 3, 5]] == 11).all())  # the fifth word alone is written
