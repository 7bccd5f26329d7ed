"""The setup and corpus kernels -- K1 (n2v_alias_build), n2v_corpus_count / n2v_corpus_index, n2v_edge_bias,
n2v_alias_draw, n2v_walk_uniforms, n2v_trim_mark, n2v_pivots_build, n2v_cum_index_build -- through the C ABI,
at chunk edges and past one grid pass, against the oracle / numpy / torch statement of the same operation.

Every comparison is exact (integers equal, floats by bit pattern) and covers every row, token and bucket.
Every output buffer is preset to a sentinel the kernel can never write, so an item a grid-stride loop never
reached is a mismatch, not a stale correct value.  The cases come from tests/setup_cases.py;
test_setup_cases_host.py proves on the CPU that they reach the branches they were built for."""
import numpy as np
import pytest
import torch

import setup_cases as sc

pytestmark = pytest.mark.gpu

SENT = -7                     # never a vertex id, a vocabulary index or a table position
SENT_SLOT = 0x7FC0DEAD        # both int32 halves of a slot's prob: 1.5e306 as fp64, never a prob
SENT_F64 = 0x7FF8DEADBEEF0001  # a NaN payload no arithmetic produces


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lib():
    from node2vec_amd import _lib as lib

    return lib, lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f64_sentinel(n):
    return torch.full((max(n, 1),), SENT_F64, dtype=torch.int64, device="cuda").view(torch.float64)


def _bits(t):
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


def _first_bad_row(rowptr, bad):
    i = int(np.nonzero(bad)[0][0])
    return int(np.searchsorted(rowptr, i, side="right") - 1), i


# ---- 1. K1 ---------------------------------------------------------------------------------------------
def _k1(rowptr, col, w):
    """n2v_alias_build on a CSR held in numpy arrays (w float32 or float64: the storage form of the graph):
    (col, alias vertex, prob bits) of every slot, and the status word"""
    lib, L = _lib()
    rp, c, wt = _t(rowptr), _t(col), _t(w)
    nnz = len(col)
    slots = torch.full((nnz + 1, 4), SENT_SLOT, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    g = lib.Graph(n_vertices=len(rowptr) - 1, n_edges=nnz, rowptr=rp.data_ptr(), col=c.data_ptr(),
                  w=wt.data_ptr() if w.dtype == np.float32 else 0,
                  w64=wt.data_ptr() if w.dtype == np.float64 else 0)
    lib.check(L.n2v_alias_build(g, slots.data_ptr(), status.data_ptr(), lib.current_stream_ptr()), "n2v_alias_build")
    torch.cuda.synchronize()
    s = slots.cpu().numpy()
    assert (s[nnz] == SENT_SLOT).all()  # nothing written past the last slot
    s = s[:nnz]
    return s[:, 0], s[:, 1], np.ascontiguousarray(s[:, 2:]).view(np.uint64).reshape(-1), int(status[0].item())


def _assert_slots(oracle, rowptr, col, w, got, skip=()):
    g_col, g_alias, g_prob, _ = got
    alias_v, prob_bits, done = sc.expected_slots(oracle, rowptr, col, w, skip)
    bad = done & ((g_col != col) | (g_alias != alias_v) | (g_prob != prob_bits))
    assert not bad.any(), ("first differing (row, slot)", _first_bad_row(rowptr, bad), int(bad.sum()))
    # slots of skipped rows keep the sentinel in alias and prob or whatever the kernel left: not compared;
    # every other slot was written
    assert not (done & (g_alias == SENT_SLOT)).any()
    return done


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
def test_k1_deliberate_rows_equal_the_oracle(oracle, storage):
    """every length 1 .. 193 around the 64-lane chunk and one row past 4 096, under every weight pattern of
    setup_cases.alias_rows (each exit of the pairing loop, demotion chains across chunk boundaries, zeros,
    the ulp quirks, 24 decades): alias vertex through col and fp64 prob bits equal generate_alias_tables.
    fp64: all rows, stored as n2v_graph.w64; fp32: the rows whose weights are fp32 values, stored as w."""
    rows = [w for _, w in sc.alias_rows()]
    if storage == "fp32":
        rows = [w for w in rows if sc.is_f32(w)]
        assert len(rows) > 100
    rowptr, col, w = sc.pack_rows(rows)
    if storage == "fp32":
        w = w.astype(np.float32)
    got = _k1(rowptr, col, w)
    assert got[3] == 0
    done = _assert_slots(oracle, rowptr, col, w, got)
    assert done.all()


@pytest.fixture(scope="module")
def short_rows():
    return sc.short_rows_graph(sc.rows_past_one_pass(_cus()))


def test_k1_past_one_grid_pass_equals_the_oracle(oracle, short_rows):
    """2 x CUs x 32 + 3 short rows (fp32 weights, empty rows first, last and in runs): more rows than waves
    can be resident, so the row loop takes its stride trip; every row against the oracle"""
    rowptr, col, w, _ = short_rows
    assert len(rowptr) - 1 == 2 * _cus() * 32 + 3
    got = _k1(rowptr, col, w)
    assert got[3] == 0
    assert _assert_slots(oracle, rowptr, col, w, got).all()


def test_k1_zero_row_in_a_late_trip_sets_zerodiv(oracle, short_rows):
    """a zero-sum row in the last trip of the launch: N2V_ST_ZERODIV is set, every other row is still the
    oracle's, and the Python layer raises ZeroDivisionError"""
    from node2vec_amd import _lib as lib
    from node2vec_amd.graph import DeviceGraph

    rowptr, col, w, z = sc.short_rows_graph(sc.rows_past_one_pass(_cus()), zero=True)
    assert z > _cus() * 32
    got = _k1(rowptr, col, w)
    assert got[3] == lib.ST_ZERODIV
    done = _assert_slots(oracle, rowptr, col, w, got, skip={z})
    assert (~done).sum() == 3
    with pytest.raises(ZeroDivisionError):
        DeviceGraph(_t(rowptr), _t(col), _t(w)).build_alias()


# ---- 2. corpus passes ----------------------------------------------------------------------------------
INT32_MAX = 2 ** 31 - 1


def _corpus_index_raw(walks, valid, index_of):
    lib, L = _lib()
    out = torch.full_like(walks, SENT)
    v = None if valid is None else valid.to(torch.uint8).contiguous()
    lib.check(L.n2v_corpus_index(walks.data_ptr(), 0 if v is None else v.data_ptr(), index_of.data_ptr(),
                                 walks.shape[0], walks.shape[1], index_of.numel(), out.data_ptr(),
                                 lib.current_stream_ptr()), "n2v_corpus_index")
    return out


def _corpus_shapes():
    items = sc.items_past_one_pass(_cus(), 4)
    return {"len1": (5003, 1), "len81_past_one_pass": ((items + 80) // 81, 81), "len41_one_row": (1, 41)}


@pytest.mark.parametrize("shape", ["len1", "len81_past_one_pass", "len41_one_row"])
def test_corpus_passes_equal_torch(shape):
    """n2v_corpus_count (the kernel: sort_above beyond the batch) and the sort path, n2v_corpus_index, against
    torch ops: valid None / all true / all false / first and last row unlike their neighbours; tokens -1,
    n_vertices - 1, n_vertices and INT32_MAX; counts preset to non-zero values (the kernel accumulates)"""
    from node2vec_amd import sgns

    rows, length = _corpus_shapes()[shape]
    if shape == "len81_past_one_pass":
        assert rows * length > 2 * (_cus() * 32 * 64 * 4)
    nv = 5000
    gen = torch.Generator().manual_seed(rows + length)
    walks = torch.randint(-1, nv + 2, (rows, length), generator=gen, dtype=torch.int32)
    flat = walks.reshape(-1)
    flat[0], flat[-1] = INT32_MAX, nv
    flat[1 % flat.numel()], flat[flat.numel() // 2], flat[-2] = -1, nv - 1, INT32_MAX
    walks = walks.cuda()
    index_of = torch.randperm(nv, generator=gen).to(torch.int32)
    index_of[::7] = -1
    index_of = index_of.cuda()
    patterns = {"none": None, "all": torch.ones(rows, dtype=torch.bool), "nothing": torch.zeros(rows, dtype=torch.bool)}
    if rows >= 3:
        v = torch.rand(rows, generator=gen) < 0.7
        v[0], v[-1] = ~v[1], ~v[-2]
        patterns["edges"] = v
    preset = (torch.arange(nv, dtype=torch.int64) % 5 + 1).cuda()
    in_range = (walks >= 0) & (walks < nv)
    for name, valid in patterns.items():
        valid = None if valid is None else valid.cuda()
        ok = in_range if valid is None else in_range & valid.unsqueeze(1)
        want = torch.bincount(walks[ok].long(), minlength=nv) + preset
        counts = preset.clone()
        sgns.corpus_count(walks, valid, counts, sort_above=walks.numel() + 1)  # the kernel
        assert torch.equal(counts, want), name
        counts = preset.clone()
        sgns.corpus_count(walks, valid, counts, sort_above=1)  # the sort path
        assert torch.equal(counts, want), name
        ref = torch.where(ok, index_of[walks.clamp(0, nv - 1).long()], torch.full_like(walks, -1))
        idx = _corpus_index_raw(walks, valid, index_of)
        assert not bool((idx == SENT).any()), name
        assert torch.equal(idx, ref), name
        assert torch.equal(sgns.corpus_index(walks, valid, index_of), ref), name


def test_corpus_passes_past_2_31_tokens():
    """rows x 81 just above 2^31 tokens: the branch of both kernels that finds the row of a token by 64-bit
    division.  valid depends on the row (row % 3 != 0, last row valid), so a wrong row changes the result;
    compared with torch ops in slices.  About 17 GB of device memory.

    What this does NOT tell apart: a threshold of 2^31 from one of 2^32.  Token offsets here stay below
    2^32, where the 32-bit unsigned division gives the same rows; the case is not grown to find out."""
    lib, L = _lib()
    length = 81
    rows = (2 ** 31) // length + 1
    assert (rows - 1) * length < 2 ** 31 <= rows * length
    nv = 1 << 20
    step = 1 << 20
    gen = torch.Generator(device="cuda").manual_seed(17)
    walks = torch.empty((rows, length), dtype=torch.int32, device="cuda")
    for a in range(0, rows, step):
        b = min(a + step, rows)
        walks[a:b] = torch.randint(-1, nv + 2, (b - a, length), generator=gen, dtype=torch.int32, device="cuda")
    walks[0, 0], walks[-1, -1], walks[-1, 0] = INT32_MAX, nv - 1, 5
    valid = (torch.arange(rows, device="cuda") % 3 != 0)
    valid[-1] = True
    v8 = valid.to(torch.uint8)
    index_of = (torch.arange(nv, dtype=torch.int32, device="cuda") * 7 + 1) % nv
    index_of[::11] = -1
    counts = torch.full((nv,), 3, dtype=torch.int64, device="cuda")
    lib.check(L.n2v_corpus_count(walks.data_ptr(), v8.data_ptr(), rows, length, nv, counts.data_ptr(),
                                 lib.current_stream_ptr()), "n2v_corpus_count")
    idx = _corpus_index_raw(walks, valid, index_of)
    want = torch.full((nv,), 3, dtype=torch.int64, device="cuda")
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for a in range(0, rows, step):
        b = min(a + step, rows)
        w = walks[a:b]
        ok = (w >= 0) & (w < nv) & valid[a:b].unsqueeze(1)
        want += torch.bincount(w[ok].long(), minlength=nv)
        ref = torch.where(ok, index_of[w.clamp(0, nv - 1).long()], torch.full_like(w, -1))
        bad += (idx[a:b] != ref).sum()
        del w, ok, ref
    assert int(bad.item()) == 0
    assert torch.equal(counts, want)
    del walks, idx
    torch.cuda.empty_cache()


# ---- 3. transformer-level kernels ------------------------------------------------------------------------
def _edge_bias(case, w, p, q):
    """n2v_edge_bias on a BiasCase with weights w (None, float32 or float64): fp64 bit patterns"""
    lib, L = _lib()
    nnz = len(case.ids)
    out = _f64_sentinel(nnz + 1)
    keep = [_t(case.rowptr), _t(case.ids), None if w is None else _t(w), _t(case.src_id), _t(case.src_rowptr),
            _t(case.src_nbs if len(case.src_nbs) else np.zeros(1, np.int32))]
    wt = keep[2]
    lib.check(L.n2v_edge_bias(keep[0].data_ptr(), keep[1].data_ptr(),
                              wt.data_ptr() if wt is not None and wt.dtype == torch.float32 else 0,
                              wt.data_ptr() if wt is not None and wt.dtype == torch.float64 else 0,
                              keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), case.n_rows, nnz,
                              p, q, out.data_ptr(), lib.current_stream_ptr()), "n2v_edge_bias")
    torch.cuda.synchronize()
    bits = _bits(out)
    assert bits[nnz] == SENT_F64
    return bits[:nnz]


def _assert_bias(case, p, q):
    for w in (case.w64, case.w32, None):
        got = _edge_bias(case, w, p, q)
        want = case.expected(p, q, np.ones(len(case.ids)) if w is None else w).view(np.uint64)
        bad = got != want
        assert not bad.any(), ("first differing (row, entry)", _first_bad_row(case.rowptr, bad), int(bad.sum()),
                               None if w is None else w.dtype)


@pytest.mark.parametrize("pq", [(3.0, 0.7), (0.5, 2.0)])
def test_edge_bias_at_the_edges_of_the_source_lists(pq):
    """source lists of 0, 1, 31, 32, 33, 64, 65 and 1 000 ids probed at their first and last entry, just
    below and above them, and with x == s while s is in the list too (w / p wins); first-step rows
    interleaved; empty rows first, last and in runs, which the row search must step over; w, w64 and unit
    weights.  Expected: w / p, w, w / q in float64 numpy, one division each."""
    _assert_bias(sc.bias_edges_case(), *pq)


def test_edge_bias_past_one_grid_pass():
    case = sc.bias_stride_case(sc.items_past_one_pass(_cus(), 2))
    assert len(case.ids) > 2 * (_cus() * 32 * 64 * 2)
    _assert_bias(case, 3.0, 0.7)


def test_bias_table_draw_chain_equals_the_oracle_row_by_row(oracle):
    """n2v_edge_bias -> K1 -> n2v_alias_draw on the rows of the edge case == the oracle's
    generate_edge_alias_tables (generate_alias_tables on a first step) and sampling_from_alias per row"""
    from node2vec_amd import transformers as T

    c = sc.bias_edges_case()
    p, q = 3.0, 0.7
    rowptr, ids = _t(c.rowptr), _t(c.ids)
    biased = T._bias_rows(rowptr, ids, _t(c.w64), _t(c.src_id), _t(c.src_rowptr), _t(c.src_nbs), p, q)
    slots = T._build_tables(rowptr, ids, biased)
    rng = np.random.default_rng(2)
    r1, r2 = rng.random(c.n_rows), rng.random(c.n_rows)
    drawn = T._draw_device(rowptr, slots, _t(r1), _t(r2)).cpu().numpy()
    s = slots.cpu().numpy()
    prob = np.ascontiguousarray(s[:, 2:]).view(np.float64).reshape(-1)
    for r in range(c.n_rows):
        b, e = int(c.rowptr[r]), int(c.rowptr[r + 1])
        if e == b:
            assert drawn[r] == -1
            continue
        if c.src_id[r] < 0:
            alias, probs = oracle.alias_tables(c.w64[b:e])
        else:
            nb = c.src_nbs[c.src_rowptr[r]:c.src_rowptr[r + 1]]
            alias, probs = oracle.edge_alias_tables(int(c.src_id[r]), nb.tolist(), c.ids[b:e], c.w64[b:e], p, q)
        assert s[b:e, 1].tolist() == c.ids[b:e][np.array(alias)].tolist(), r
        assert prob[b:e].tolist() == probs, r
        assert drawn[r] == c.ids[b + oracle.sampling_from_alias(alias, probs, r1[r], r2[r])], r


def _slots_of(rowptr, col, alias_idx, prob):
    s = np.zeros((max(len(col), 1), 4), np.int32)
    n = len(col)
    lens = np.diff(rowptr)
    s[:n, 0] = col
    s[:n, 1] = col[np.repeat(rowptr[:-1], lens) + alias_idx]
    s[:n, 2:] = prob.view(np.int32).reshape(-1, 2)
    return s


def _draw(rowptr_t, slots_t, r1, r2):
    """n2v_alias_draw: (vertex per row, status word)"""
    lib, L = _lib()
    n_rows = rowptr_t.numel() - 1
    out = torch.full((n_rows + 1,), SENT, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    t1, t2 = _t(r1), None if r2 is None else _t(r2)
    lib.check(L.n2v_alias_draw(rowptr_t.data_ptr(), slots_t.data_ptr(), n_rows, t1.data_ptr(),
                               0 if t2 is None else t2.data_ptr(), out.data_ptr(), status.data_ptr(),
                               lib.current_stream_ptr()), "n2v_alias_draw")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[n_rows] == SENT
    return o[:n_rows], int(status[0].item())


def test_alias_draw_at_the_ends_of_the_unit_interval(oracle):
    """rows of 0, 1, 3, 64 and 3 000 slots: r1 = 0.0; r1 = nextafter(1, 0), where the pick is n - 1 like
    Python's int(r1 * n); r2 == prob[pick] exactly (`<`: the alias); the one-uniform (wiki) form; empty rows
    give -1; r1 = 1.0 and r1 = -1.0 give -1 and N2V_ST_RANGE without disturbing the other rows, while
    r1 = -0.25 on three slots truncates to pick 0 as int() does"""
    from node2vec_amd import _lib as lib

    rowptr, col, alias_idx, prob = sc.draw_table(sc.DRAW_EDGE_LENGTHS)
    n = np.diff(rowptr)
    n_rows = len(n)
    rp, sl = _t(rowptr), _t(_slots_of(rowptr, col, alias_idx, prob))
    rng = np.random.default_rng(4)
    below_one = np.nextafter(1.0, 0.0)

    def check(r1, r2, status_want=0):
        got, status = _draw(rp, sl, r1, r2)
        want, bad = sc.draw_expected(rowptr, col, alias_idx, prob, r1, r2)
        assert np.array_equal(got, want) and status == status_want
        for r in range(n_rows):  # and the oracle itself, row by row
            b, e = rowptr[r], rowptr[r + 1]
            if e == b or bad[r]:
                assert got[r] == -1
            elif r2 is None:
                assert got[r] == col[b + oracle.sampling_from_alias_wiki(alias_idx[b:e], prob[b:e], r1[r])]
            else:
                assert got[r] == col[b + oracle.sampling_from_alias(alias_idx[b:e], prob[b:e], r1[r], r2[r])]
        return got

    check(np.zeros(n_rows), rng.random(n_rows))
    check(np.zeros(n_rows), None)
    got = check(np.full(n_rows, below_one), np.zeros(n_rows))  # r2 = 0 < prob unless prob == 0
    last = rowptr[1:] - 1
    keeps = (n > 0) & (prob[np.maximum(last, 0)] > 0)
    assert np.array_equal(got[keeps], col[last[keeps]])  # the pick is the LAST slot
    check(np.full(n_rows, below_one), None)
    r1 = rng.random(n_rows)
    pick = (r1 * n).astype(np.int64)
    r2 = np.where(n > 0, prob[np.minimum(rowptr[:-1] + pick, len(prob) - 1)], 0.5)
    got = check(r1, r2)
    at = np.minimum(rowptr[:-1] + pick, len(prob) - 1)
    assert np.array_equal(got[n > 0], col[np.minimum(rowptr[:-1] + alias_idx[at], len(col) - 1)][n > 0])  # always the alias
    for _ in range(3):
        check(rng.random(n_rows), rng.random(n_rows))
        check(rng.random(n_rows), None)
    r1, r2 = rng.random(n_rows), rng.random(n_rows)
    assert n[3] == 64 and n[8] == 3 and n[2] == 3
    r1[3], r1[8], r1[2] = 1.0, -1.0, -0.25
    got = check(r1, r2, lib.ST_RANGE)
    assert got[3] == -1 and got[8] == -1 and got[2] in (col[rowptr[2]], col[rowptr[2] + alias_idx[rowptr[2]]])


def test_alias_draw_past_one_grid_pass():
    n_rows = sc.items_past_one_pass(_cus(), 2)
    lens = np.tile(np.array([0, 1, 3, 2, 7, 0, 0, 4]), n_rows // 8 + 1)[:n_rows]
    rowptr, col, alias_idx, prob = sc.draw_table(lens)
    rp, sl = _t(rowptr), _t(_slots_of(rowptr, col, alias_idx, prob))
    rng = np.random.default_rng(6)
    r1, r2 = rng.random(n_rows), rng.random(n_rows)
    pick = (r1 * lens).astype(np.int64)
    exact = (np.arange(n_rows) % 5 == 0) & (lens > 0)  # every fifth row: r2 == prob[pick]
    r2[exact] = prob[(rowptr[:-1] + pick)[exact]]
    for second in (r2, None):
        got, status = _draw(rp, sl, r1, second)
        want, bad = sc.draw_expected(rowptr, col, alias_idx, prob, r1, second)
        assert status == 0 and not bad.any()
        assert np.array_equal(got, want)


def test_walk_uniforms_past_one_grid_pass():
    """r = u / 2^32 of the stream of DESIGN.md "RNG" for keys over the whole int64 range: every key against
    the numpy restatement that test_setup_cases_host.py pins to the oracle's n2v_oracle_uniform_bits; and
    every key past the first pass equals the same key in a launch of its own"""
    lib, L = _lib()
    n = sc.items_past_one_pass(_cus(), 2)
    keys, steps = sc.uniform_keys(n)
    kt, st = _t(keys), _t(steps)

    def run(k, s, seed):
        m = k.numel()
        r1, r2 = _f64_sentinel(m + 1), _f64_sentinel(m + 1)
        lib.check(L.n2v_walk_uniforms(seed, k.data_ptr(), s.data_ptr(), m, r1.data_ptr(), r2.data_ptr(),
                                      lib.current_stream_ptr()), "n2v_walk_uniforms")
        torch.cuda.synchronize()
        b1, b2 = _bits(r1), _bits(r2)
        assert b1[m] == SENT_F64 and b2[m] == SENT_F64
        return b1[:m], b2[:m]

    for seed in (42, 2 ** 64 - 1):
        b1, b2 = run(kt, st, seed)
        u1, u2 = sc.uniform_bits(seed, keys, steps)
        assert np.array_equal(b1, (u1.astype(np.float64) * (1.0 / 4294967296.0)).view(np.uint64))
        assert np.array_equal(b2, (u2.astype(np.float64) * (1.0 / 4294967296.0)).view(np.uint64))
    half = n // 2
    t1, t2 = run(kt[half:].contiguous(), st[half:].contiguous(), 2 ** 64 - 1)
    assert np.array_equal(t1, b1[half:]) and np.array_equal(t2, b2[half:])


# ---- 4. trimming, pivots, cum index ----------------------------------------------------------------------
def _trim(rowptr, cap, seed):
    lib, L = _lib()
    rp = _t(rowptr)
    keep = torch.ones(int(rowptr[-1]) + 1, dtype=torch.uint8, device="cuda")  # the caller's preset
    keep[-1] = 9
    lib.check(L.n2v_trim_mark(rp.data_ptr(), len(rowptr) - 1, cap, seed, keep.data_ptr(),
                              lib.current_stream_ptr()), "n2v_trim_mark")
    k = keep.cpu().numpy()
    assert k[-1] == 9
    return k[:-1].astype(bool)


def _assert_trim(oracle, rowptr, cap, seed):
    got = _trim(rowptr, cap, seed)
    assert np.array_equal(got, oracle.trim_mark(rowptr, cap, seed))
    eff = cap if cap > 0 else 100000
    deg = np.diff(rowptr)
    kept = np.array([got[rowptr[r]:rowptr[r + 1]].sum() for r in range(len(deg))])
    assert np.array_equal(kept[deg > eff], np.full((deg > eff).sum(), eff))  # a hot row keeps exactly cap
    assert np.array_equal(kept[deg <= eff], deg[deg <= eff])                 # a cold row keeps everything
    return got


@pytest.mark.parametrize("cap", sc.TRIM_CAPS)
@pytest.mark.parametrize("n_rows", sc.TRIM_ROWS)
def test_trim_mark_around_the_cap_and_the_block(oracle, n_rows, cap):
    """degrees cap - 1, cap, cap + 1 and 2 cap, hot rows first and last, n_rows next to multiples of the
    64-thread block: marks equal the oracle's"""
    rowptr = sc.trim_rowptr(n_rows, cap)
    a = _assert_trim(oracle, rowptr, cap, 20)
    b = _assert_trim(oracle, rowptr, cap, 21)
    assert (a != b).any()


def test_trim_mark_cap_not_positive_means_100000(oracle):
    rowptr = np.array([0, 5, 5 + 100001, 5 + 100001 + 100000, 5 + 100001 + 100000 + 3], np.int64)
    for cap in (0, -5):
        got = _assert_trim(oracle, rowptr, cap, 3)
        assert got[5:5 + 100001].sum() == 100000


def test_pivots_build_at_block_edges_and_past_one_pass():
    """pivots[i] == col[min(32 i + 31, E - 1)] for E around the 32-entry block and for enough blocks to take
    the kernel past one grid pass"""
    lib, L = _lib()
    big = 32 * sc.items_past_one_pass(_cus(), 2) - 5
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n_edges in (1, 31, 32, 33, 63, 64, 65, big):
        col = torch.randint(0, INT32_MAX, (n_edges,), generator=gen, dtype=torch.int32, device="cuda")
        n_piv = (n_edges + 31) // 32
        piv = torch.full((n_piv + 2,), SENT, dtype=torch.int32, device="cuda")
        lib.check(L.n2v_pivots_build(col.data_ptr(), n_edges, piv.data_ptr(), lib.current_stream_ptr()),
                  "n2v_pivots_build")
        at = torch.clamp(torch.arange(n_piv, device="cuda") * 32 + 31, max=n_edges - 1)
        assert torch.equal(piv[:n_piv], col[at]), n_edges
        assert piv[n_piv:].tolist() == [SENT, SENT], n_edges


def _cum_index(tab, bits):
    lib, L = _lib()
    t = _t(np.asarray(tab, np.int64).astype(np.int32))
    n = (1 << bits) + 1
    index = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    lib.check(L.n2v_cum_index_build(t.data_ptr(), len(tab), bits, index.data_ptr(), lib.current_stream_ptr()),
              "n2v_cum_index_build")
    out = index.cpu().numpy()
    assert out[n:].tolist() == [SENT, SENT]
    return out[:n]


def _model_bits(n):
    import math

    return int(min(24, max(10, math.ceil(math.log2(max(n, 2))) - 4)))  # SgnsModel's rule


def test_cum_index_is_bisect_left_on_small_large_and_run_tables():
    """index[b] == bisect_left(cum_table, b << (31 - bits)) for every bucket and the last entry: vocabularies
    of 1, 2 and 17 words (bits 10), one large enough for bits > 10, tables with runs of equal neighbours
    (from counts, and made by hand so that the runs sit exactly on bucket edges, where bisect_left and
    bisect_right differ), and enough buckets to take the kernel past one grid pass"""
    from node2vec_amd import sgns

    tables = []
    for n in (1, 2, 17):
        tables.append((sgns.make_cum_table(torch.arange(n, 0, -1)).numpy().astype(np.int64), 10))
    gen = torch.Generator().manual_seed(2)
    counts = torch.sort(torch.randint(1, 1000, (40000,), generator=gen), descending=True).values
    tables.append((sgns.make_cum_table(counts).numpy().astype(np.int64), _model_bits(40000)))
    assert tables[-1][1] == 12
    for n_side in (2500, 20000):
        counts = torch.from_numpy(sc.runs_counts(n_side))
        tables.append((sgns.make_cum_table(counts).numpy().astype(np.int64), _model_bits(2 * n_side + 1)))
    tables += [(sc.edge_hitting_table(10), 10), (sc.edge_hitting_table(12), 12)]
    big = next(b for b in range(10, 31) if (1 << b) + 1 >= sc.items_past_one_pass(_cus(), 2))
    tables += [(sc.edge_hitting_table(12), big), (tables[4][0], big)]
    for tab, bits in tables:
        assert np.array_equal(_cum_index(tab, bits), sc.cum_index_expected(tab, bits)), (len(tab), bits)


def test_cum_index_over_runs_changes_no_draw(oracle):
    """on a vocabulary whose cum_table has runs of equal entries (a run of zeros at its start), a model built
    with the index and one built without it train the same bits in one deterministic launch, and both equal
    the oracle, which bisects the whole table"""
    from node2vec_amd import sgns

    counts = torch.from_numpy(sc.runs_counts(2500)).cuda()
    n = counts.numel()
    vocab = sgns.Vocab(torch.arange(n, device="cuda"), counts, torch.arange(n, dtype=torch.int32, device="cuda"))
    a = sgns.SgnsModel(vocab, 16, 5, 5, seed=3)
    b = sgns.SgnsModel(vocab, 16, 5, 5, seed=3, use_cum_index=False)
    assert a.cum_index is not None and b.cum_index is None and a.cum_index_bits == 10
    cum = a.cum_table.cpu().numpy().astype(np.int64)
    assert (cum[:200] == 0).all() and (np.diff(cum) == 0).sum() > 2500  # the device's table has the runs too
    assert np.array_equal(a.cum_index.cpu().numpy(), sc.cum_index_expected(cum, 10))
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, n, (64, 21), generator=gen, dtype=torch.int32).cuda()
    s0, s1 = a.syn0.cpu().numpy().copy(), a.syn1neg.cpu().numpy().copy()
    a.train_block(idx, 0.025, 5, deterministic=True)
    b.train_block(idx, 0.025, 5, deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(a.syn0, b.syn0) and torch.equal(a.syn1neg, b.syn1neg)
    pairs = oracle.sgns_train(idx.cpu().numpy(), s0, s1, cum.astype(np.uint32), None, sgns.exp_table(), n, 5, 3,
                              16, 5, 5, 0.025)
    assert pairs == int(a.pairs.item()) == int(b.pairs.item())
    assert np.array_equal(a.syn0.cpu().numpy(), s0) and np.array_equal(a.syn1neg.cpu().numpy(), s1)
