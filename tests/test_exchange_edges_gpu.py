"""The HIP passes of the replica exchange (csrc/n2v_sync.hip: n2v_delta_ref_init / pack / reduce / apply) and of
the streamed corpus (csrc/n2v_corpus.hip: n2v_corpus_count / index) where such kernels go wrong: world sizes whose
reciprocal is no fp32 number, bases off 16 bytes, ragged tails, special values, more than one trip round the
grid, a batch of more than 2^32 tokens.  The exchange is compared bit for bit with tests/exchange_restatement.py
(numpy, written apart from the kernels and from their host forms; tests/test_exchange_host.py holds the host
forms to the same), the corpus passes with bincount / gather.

No test here provokes a fault: every misaligned pointer lies inside a live allocation, and the entry points
fall back to scalar accesses for it."""
import gc

import numpy as np
import pytest
import torch

import exchange_cases as X
import exchange_restatement as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8                   # words before and after every buffer a kernel writes (8 fp32 = 32 B, 8 bf16 = 16 B)
F32_GUARD = 0x5EADBEEF      # (a finite fp32 and an int32)
BF16_GUARD = 0x5EAD
TAILS = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 4099)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _lib():
    from node2vec_amd import _lib as lib

    return lib, lib.load()


class _Buf:
    """n words of fp32 (width 4) or bf16 (width 2) at element offset `off` into a larger device allocation,
    with GUARD + off guard words in front and GUARD behind"""

    def __init__(self, n, width, off=0, init=None):
        self.n, self.width, self.lead = n, width, GUARD + off
        self.np_dtype = np.uint32 if width == 4 else np.uint16
        self.guard = F32_GUARD if width == 4 else BF16_GUARD
        host = np.full(self.lead + n + GUARD, self.guard, dtype=self.np_dtype)
        if init is not None:
            host[self.lead:self.lead + n] = np.ascontiguousarray(init).view(self.np_dtype)
        t_dtype = torch.int32 if width == 4 else torch.int16
        self.t = torch.from_numpy(host.view(np.int32 if width == 4 else np.int16)).to(DEV)
        assert self.t.dtype == t_dtype and self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lead * width

    def read(self, what):
        """the n words (fp32 as float32, bf16 as bits), after asserting the guards are as planted"""
        torch.cuda.synchronize()
        host = self.t.cpu().numpy().view(self.np_dtype)
        assert (host[:self.lead] == self.guard).all(), f"{what}: words BEFORE the buffer were written"
        assert (host[self.lead + self.n:] == self.guard).all(), f"{what}: words BEHIND the buffer were written"
        body = host[self.lead:self.lead + self.n].copy()
        return body.view(np.float32) if self.width == 4 else body


def _wire_buf(n, wire, off=0, init=None):
    return _Buf(n, 4 if wire == "fp32" else 2, off, init)


def dev_ref_init(cur, off_cur=0, off_ref=0):
    lib, L = _lib()
    n = cur.size
    c, r = _Buf(n, 4, off_cur, cur), _Buf(n, 2, off_ref)
    lib.check(L.n2v_delta_ref_init(c.ptr, n, r.ptr, lib.current_stream_ptr()), "n2v_delta_ref_init")
    R.assert_same_bits(c.read("ref_init cur"), cur, "ref_init changed its input")
    return r.read("ref_init ref")


def dev_pack(cur, ref, snapshot, wire, offs=(0, 0, 0, 0)):
    """offs: element offsets of (cur, before, wire, ref).  -> (wire, before or None); asserts that cur and ref are
    left alone and that nothing around the outputs is touched"""
    lib, L = _lib()
    n = cur.size
    c = _Buf(n, 4, offs[0], cur)
    b = _Buf(n, 4, offs[1]) if snapshot else None
    w = _wire_buf(n, wire, offs[2])
    r = _Buf(n, 2, offs[3], ref) if wire == "bf16" else None
    lib.check(L.n2v_delta_pack(c.ptr, 0 if r is None else r.ptr, n, 0 if b is None else b.ptr, w.ptr,
                               lib.WIRE_F32 if wire == "fp32" else lib.WIRE_BF16, lib.current_stream_ptr()),
              "n2v_delta_pack")
    R.assert_same_bits(c.read("pack cur"), cur, "pack changed cur")
    if r is not None:
        assert np.array_equal(r.read("pack ref"), ref), "pack changed the reference"
    return w.read("pack wire"), None if b is None else b.read("pack before")


def dev_reduce(parts, wire):
    lib, L = _lib()
    world, m = len(parts), parts[0].size
    p = _wire_buf(world * m, wire, 0, np.concatenate(parts))
    out = _wire_buf(m, wire)
    lib.check(L.n2v_delta_reduce(p.ptr, lib.WIRE_F32 if wire == "fp32" else lib.WIRE_BF16, world, m, out.ptr,
                                 lib.current_stream_ptr()), "n2v_delta_reduce")
    return out.read("reduce out")


def dev_apply(cur, ref, before, total, world, wire, offs=(0, 0, 0, 0)):
    """offs: element offsets of (cur, before, wire, ref).  -> (cur', ref' or None)"""
    lib, L = _lib()
    n = cur.size
    c = _Buf(n, 4, offs[0], cur)
    b = None if before is None else _Buf(n, 4, offs[1], before)
    w = _wire_buf(n, wire, offs[2], total)
    r = _Buf(n, 2, offs[3], ref) if wire == "bf16" else None
    lib.check(L.n2v_delta_apply(c.ptr, 0 if r is None else r.ptr, 0 if b is None else b.ptr, w.ptr,
                                lib.WIRE_F32 if wire == "fp32" else lib.WIRE_BF16, world, n,
                                lib.current_stream_ptr()), "n2v_delta_apply")
    if b is not None:
        R.assert_same_bits(b.read("apply before"), before, "apply changed the snapshot")
    got_w = w.read("apply wire")
    R.assert_same_bits(got_w, total, "apply changed the summed wire")
    return c.read("apply cur"), None if r is None else r.read("apply ref")


# -- world sizes: the whole exchange through DeltaSync._exchange ------------------------------------------------

@pytest.mark.parametrize("exact", [True, False], ids=["set", "add"])
@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", X.WORLDS + (4,))
def test_device_exchange_equals_the_restatement(world, wire, exact):
    """every rank of `world`, after one blocked exchange; in the add form the rows are changed between pack and
    apply (a kernel that set instead of added would lose the change).  World 3, 5, 6, 7 are the sizes where
    sum / world and sum * (1 / world) are different fp32 operations."""
    for case, block_rows in ((X.random_case(world, [(300, 16)], 21), 64),
                             (X.random_case(world, [(33, 5)], 11), 2),
                             (X.random_case(world, [(37, 7), (5, 3)], 12), 256),
                             (X.special_case(world), 97)):
        bad, _, _ = X.check_exchange(DEV, world, wire, case, block_rows, exact)
        assert bad == 0, (world, wire, exact, block_rows, bad)


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", X.WORLDS + (4,))
def test_mean_is_a_division(world, wire):
    """n2v_delta_apply alone on well-scaled sums: mean = sum / world, one fp32 division.  Printed: how many of the
    elements a product with the fp32 reciprocal would get differently (0 for a power of two), so that a failure
    here can be read against it."""
    rng = np.random.default_rng(31 + world)
    n = 100003
    if wire == "fp32":
        total, ref = rng.standard_normal(n, dtype=np.float32), None
    else:
        total = R.f32_to_bf16(0.05 * rng.standard_normal(n, dtype=np.float32))
        ref = R.f32_to_bf16(rng.standard_normal(n, dtype=np.float32))
    cur = rng.standard_normal(n, dtype=np.float32)
    want_c, want_r = R.apply(cur, ref, None, total, world)
    s = total if wire == "fp32" else R.bf16_to_f32(total)
    inv = np.float32(1) / np.float32(world)
    p = s * inv
    other = p if wire == "fp32" else R.bf16_to_f32(ref) + p
    got_c, got_r = dev_apply(cur, ref, None, total, world, wire)
    print(f"world {world} {wire}: kernel differs from sum / world in {R.count_differing(got_c, want_c)} of {n}; "
          f"sum * (1 / world) would in {R.count_differing(other, want_c)}")
    R.assert_same_bits(got_c, want_c, f"mean, world {world}, {wire}")
    if ref is not None:
        R.assert_same_bits(got_r, want_r, f"reference, world {world}")


@pytest.mark.parametrize("exact", [True, False], ids=["set", "add"])
@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", [2, 3])
def test_device_exchange_in_blocks_off_16_bytes(world, wire, exact):
    """(1000, 7) in blocks of 3 rows: block bases at multiples of 84 bytes (their bf16 reference at 42), so
    n2v_delta_pack takes its all-scalar form on three blocks of four"""
    case = X.random_case(world, [(1000, 7)], 13)
    bad, _, _ = X.check_exchange(DEV, world, wire, case, 3, exact, ranks=(0, world - 1))
    assert bad == 0, (world, wire, exact, bad)


# -- alignment and tails: the entry points called directly -------------------------------------------------------

def _mixed(n, seed):
    """n values drawn from the special vector and from normals, and a bf16 reference near them"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([R.special_values(), rng.standard_normal(2000, dtype=np.float32)])
    cur = pool[rng.integers(0, pool.size, n)]
    ref = R.f32_to_bf16(pool[rng.integers(0, pool.size, n)])
    near = rng.random(n) < 0.7
    ref = np.where(near, R.f32_to_bf16(cur), ref).astype(np.uint16)
    return cur, ref


def _offsets():
    """(cur, before, wire, ref): all aligned; each buffer alone off by 1..3 elements; all of them off"""
    out = [(0, 0, 0, 0)]
    for off in (1, 2, 3):
        for which in range(4):
            out.append(tuple(off if k == which else 0 for k in range(4)))
        out.append((off, off, off, off))
    return out


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_pack_at_every_offset_and_tail(wire):
    for n in TAILS:
        cur, ref = _mixed(n, n)
        for snapshot in (False, True):
            want_w, want_b = R.pack(cur, ref if wire == "bf16" else None, snapshot)
            for offs in _offsets():
                if (not snapshot and offs[1] and not offs[0]) or (wire == "fp32" and offs[3] and not offs[0]):
                    continue  # that buffer is not part of this call
                got_w, got_b = dev_pack(cur, ref, snapshot, wire, offs)
                R.assert_same_bits(got_w, want_w, f"pack {wire} n={n} offsets={offs} snapshot={snapshot}")
                if snapshot:
                    R.assert_same_bits(got_b, want_b, f"snapshot {wire} n={n} offsets={offs}")


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_apply_and_ref_init_at_every_offset_and_tail(wire):
    world = 3
    for n in TAILS:
        cur, ref = _mixed(n, 100 + n)
        mid, _ = _mixed(n, 200 + n)
        total, _ = R.pack(_mixed(n, 300 + n)[0], ref if wire == "bf16" else None)
        for add in (False, True):
            want_c, want_r = R.apply(mid if add else cur, ref if wire == "bf16" else None, cur if add else None,
                                     total, world)
            for offs in _offsets():
                if (not add and offs[1] and not offs[0]) or (wire == "fp32" and offs[3] and not offs[0]):
                    continue
                got_c, got_r = dev_apply(mid if add else cur, ref, cur if add else None, total, world, wire, offs)
                R.assert_same_bits(got_c, want_c, f"apply {wire} n={n} offsets={offs} add={add}")
                if wire == "bf16":
                    R.assert_same_bits(got_r, want_r, f"apply reference n={n} offsets={offs} add={add}")
        if wire == "bf16":
            for oc in range(4):
                for orf in range(4):
                    R.assert_same_bits(dev_ref_init(cur, oc, orf), R.ref_init(cur), f"ref_init n={n} {oc} {orf}")


# -- values ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", X.WORLDS)
def test_device_passes_equal_the_restatement_on_special_values(world):
    """signed zeros, infinities, NaNs, subnormals, FLT_MIN, FLT_MAX, bf16 ties to both sides and their
    neighbours, differences that cancel / are subnormal / overflow, a sweep over all binades: through
    ref_init, pack, reduce and apply"""
    curs, ref, mids = R.edge_case(world)
    for c in curs[:2]:
        R.assert_same_bits(dev_ref_init(c), R.ref_init(c), "ref_init")
    for wire in ("fp32", "bf16"):
        rf = ref if wire == "bf16" else None
        wires = []
        for r in range(world):
            for snap in (False, True):
                want_w, want_b = R.pack(curs[r], rf, snap)
                got_w, got_b = dev_pack(curs[r], ref, snap, wire)
                R.assert_same_bits(got_w, want_w, f"pack {wire} rank {r}")
                if snap:
                    R.assert_same_bits(got_b, want_b, "snapshot")
            wires.append(want_w)
        total = R.rank_sum(wires)
        R.assert_same_bits(dev_reduce(wires, wire), total, f"sum {wire}")
        for add in (False, True):
            want_c, want_r = R.apply(mids[0] if add else curs[0], rf, curs[0] if add else None, total, world)
            got_c, got_r = dev_apply(mids[0] if add else curs[0], ref, curs[0] if add else None, total, world, wire)
            R.assert_same_bits(got_c, want_c, f"apply {wire} add={add}")
            if wire == "bf16":
                R.assert_same_bits(got_r, want_r, f"apply {wire} add={add}: reference")


@pytest.mark.parametrize("world", X.WORLDS)
def test_device_apply_equals_the_restatement_on_every_bf16_sum(world):
    total = np.arange(1 << 16, dtype=np.uint16)
    ref = (total * np.uint16(40503) + np.uint16(world)).astype(np.uint16)
    cur = np.zeros(total.size, np.float32)
    want_c, want_r = R.apply(cur, ref, None, total, world)
    got_c, got_r = dev_apply(cur, ref, None, total, world, "bf16")
    R.assert_same_bits(got_c, want_c, "apply")
    R.assert_same_bits(got_r, want_r, "reference")


def test_device_ref_init_and_reduce_on_every_bf16_value():
    """ref_init of every bf16 value widened and of its two fp32 neighbours half a bf16 step away (the ties);
    the sum of every bf16 value with itself shifted"""
    every = np.arange(1 << 16, dtype=np.uint16)
    exact = R.bf16_to_f32(every)
    ties = ((every.astype(np.uint32) << 16) | 0x8000).view(np.float32)
    below = ((every.astype(np.uint32) << 16) | 0x7FFF).view(np.float32)
    for v in (exact, ties, below):
        R.assert_same_bits(dev_ref_init(v), R.ref_init(v), "ref_init")
    parts = [every, np.roll(every, 1), (every ^ np.uint16(0x8001)).astype(np.uint16)]
    R.assert_same_bits(dev_reduce(parts, "bf16"), R.rank_sum(parts), "sum of bf16")
    fparts = [ties, np.roll(below, 3), exact]
    R.assert_same_bits(dev_reduce(fparts, "fp32"), R.rank_sum(fparts), "sum of fp32")


# -- more than one trip round the grid ------------------------------------------------------------------------------

def _grid_bound():
    """an upper bound on the elements one trip of a capped grid covers: every kernel here launches at most
    resident_blocks x 4 blocks of 256 threads, and no more than max_threads_per_multi_processor threads are resident
    on a compute unit"""
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    return p.multi_processor_count * p.max_threads_per_multi_processor * 4


CHUNK = 1 << 22


def _chunks(n):
    return [(lo, min(n, lo + CHUNK)) for lo in range(0, n, CHUNK)]


def _normals(seed, lo, hi, scale=1.0):
    return (scale * np.random.default_rng([seed, lo]).standard_normal(hi - lo, dtype=np.float32)).astype(np.float32)


def _fill_f32(seed, n, scale=1.0):
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    for lo, hi in _chunks(n):
        t[lo:hi].copy_(torch.from_numpy(_normals(seed, lo, hi, scale)))
    return t


def _fill_bf16(seed, n, scale=1.0):
    t = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    for lo, hi in _chunks(n):
        t[lo:hi].copy_(X.bf16_tensor(R.f32_to_bf16(_normals(seed, lo, hi, scale))))
    return t


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_every_sync_kernel_beyond_its_grid_cap(wire):
    lib, L = _lib()
    bound = _grid_bound()
    n = 2 * 4 * bound + 3  # pack moves float4s: four times the elements per trip; + a ragged tail
    assert n >= 2 * (4 * bound) + 3 and n >= 2 * bound + 3
    print(f"grid bound {bound} elements per trip; n = {n} ({n * 4 / 2 ** 20:.0f} MiB per fp32 buffer)")
    world, code = 3, (lib.WIRE_F32 if wire == "fp32" else lib.WIRE_BF16)
    wdt = torch.float32 if wire == "fp32" else torch.bfloat16
    to_np = X.f32_array if wire == "fp32" else X.bf16_bits
    stream = lib.current_stream_ptr()
    cur = _fill_f32(1, n)
    ref = _fill_bf16(1, n) if wire == "bf16" else None  # bf16 of the same normals: small differences
    if wire == "bf16":  # ref_init, against the buffer just filled with the restated rounding
        made = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        lib.check(L.n2v_delta_ref_init(cur.data_ptr(), n, made.data_ptr(), stream), "n2v_delta_ref_init")
        torch.cuda.synchronize()
        for lo, hi in _chunks(n):
            R.assert_same_bits(X.bf16_bits(made[lo:hi]), R.ref_init(_normals(1, lo, hi)), f"ref_init at {lo}")
        del made
        cur.add_(_fill_f32(2, n, 0.01))  # trained on since
    # pack, with a snapshot
    before = torch.zeros(n, dtype=torch.float32, device=DEV)
    w = torch.zeros(n, dtype=wdt, device=DEV)
    assert cur.data_ptr() % 16 == 0 and before.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    lib.check(L.n2v_delta_pack(cur.data_ptr(), 0 if ref is None else ref.data_ptr(), n, before.data_ptr(),
                               w.data_ptr(), code, stream), "n2v_delta_pack")
    torch.cuda.synchronize()
    for lo, hi in _chunks(n):
        c = X.f32_array(cur[lo:hi])
        want_w, want_b = R.pack(c, None if ref is None else X.bf16_bits(ref[lo:hi]), True)
        R.assert_same_bits(to_np(w[lo:hi]), want_w, f"pack at {lo}")
        R.assert_same_bits(X.f32_array(before[lo:hi]), want_b, f"snapshot at {lo}")
    # reduce: three ranks' contributions of n elements each
    parts = torch.empty(world * n, dtype=wdt, device=DEV)
    parts[:n].copy_(w)
    for r in (1, 2):
        parts[r * n:(r + 1) * n].copy_((_fill_f32 if wire == "fp32" else _fill_bf16)(10 + r, n, 10.0 ** (r - 2)))
    total = torch.zeros(n, dtype=wdt, device=DEV)
    lib.check(L.n2v_delta_reduce(parts.data_ptr(), code, world, n, total.data_ptr(), stream), "n2v_delta_reduce")
    torch.cuda.synchronize()
    for lo, hi in _chunks(n):
        want = R.rank_sum([to_np(parts[r * n + lo:r * n + hi]) for r in range(world)])
        R.assert_same_bits(to_np(total[lo:hi]), want, f"sum at {lo}")
    del parts
    # apply, add form: the rows moved on since the snapshot
    held = cur.clone()
    cur.add_(_fill_f32(3, n, 0.01))
    mid = cur.clone()
    ref0 = None if ref is None else ref.clone()
    lib.check(L.n2v_delta_apply(cur.data_ptr(), 0 if ref is None else ref.data_ptr(), before.data_ptr(),
                                total.data_ptr(), code, world, n, stream), "n2v_delta_apply")
    torch.cuda.synchronize()
    for lo, hi in _chunks(n):
        want_c, want_r = R.apply(X.f32_array(mid[lo:hi]), None if ref is None else X.bf16_bits(ref0[lo:hi]),
                                 X.f32_array(held[lo:hi]), to_np(total[lo:hi]), world)
        R.assert_same_bits(X.f32_array(cur[lo:hi]), want_c, f"apply (add) at {lo}")
        if ref is not None:
            R.assert_same_bits(X.bf16_bits(ref[lo:hi]), want_r, f"apply (add) reference at {lo}")
    # apply, set form
    if ref is not None:
        ref.copy_(ref0)
    lib.check(L.n2v_delta_apply(cur.data_ptr(), 0 if ref is None else ref.data_ptr(), 0, total.data_ptr(), code,
                                world, n, stream), "n2v_delta_apply")
    torch.cuda.synchronize()
    for lo, hi in _chunks(n):
        want_c, want_r = R.apply(X.f32_array(mid[lo:hi]), None if ref is None else X.bf16_bits(ref0[lo:hi]), None,
                                 to_np(total[lo:hi]), world)
        R.assert_same_bits(X.f32_array(cur[lo:hi]), want_c, f"apply (set) at {lo}")
        if ref is not None:
            R.assert_same_bits(X.bf16_bits(ref[lo:hi]), want_r, f"apply (set) reference at {lo}")


# -- the corpus passes ------------------------------------------------------------------------------------------------

def _corpus_want(walks, valid, nv, index_of):
    """numpy: counts of the in-range tokens of the valid rows, and their vocabulary indices (-1 elsewhere)"""
    ok = (walks >= 0) & (walks < nv)
    if valid is not None:
        ok &= valid.astype(bool)[:, None]
    counts = np.bincount(walks[ok].astype(np.int64), minlength=nv).astype(np.int64)
    idx = np.where(ok, index_of[np.clip(walks, 0, nv - 1)], np.int32(-1)).astype(np.int32)
    return counts, idx


@pytest.mark.parametrize("masked", [True, False], ids=["valid", "no-valid"])
@pytest.mark.parametrize("length", [1, 7, 41, 81])
def test_corpus_passes_beyond_their_grid_cap(length, masked):
    from node2vec_amd import sgns

    lib, L = _lib()
    bound = _grid_bound()
    rows = -(-(2 * bound + 3) // length)
    total = rows * length
    assert total >= 2 * bound + 3
    print(f"grid bound {bound} tokens per trip; {rows} rows of {length} = {total} tokens")
    nv = 5000
    rng = np.random.default_rng(length)
    walks = rng.integers(-1, nv + 3, (rows, length), dtype=np.int32)
    flat = walks.reshape(-1)
    planted = np.array([-1, INT32_MIN, nv - 1, nv, INT32_MAX], dtype=np.int32)
    for at in (0, bound - 3, bound + 1, 2 * bound - 2, total - planted.size):  # the start, around the bound, the end
        flat[at:at + planted.size] = planted
    valid = (rng.random(rows) < 0.8) if masked else None
    index_of = rng.permutation(nv).astype(np.int32)
    index_of[::7] = -1
    want_counts, want_idx = _corpus_want(walks, valid, nv, index_of)
    want_counts[7] += 5
    d_walks = torch.from_numpy(walks).to(DEV)
    d_valid = None if valid is None else torch.from_numpy(valid).to(DEV)
    for sort_above in (1 << 62, 1):  # the atomic kernel, then the sort path of large batches on the same data
        counts = torch.zeros(nv, dtype=torch.int64, device=DEV)
        counts[7] = 5  # accumulates
        sgns.corpus_count(d_walks, d_valid, counts, sort_above=sort_above)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want_counts), f"counts, sort_above={sort_above}"
    idx = sgns.corpus_index(d_walks, d_valid, torch.from_numpy(index_of).to(DEV))
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx)


def test_corpus_passes_on_a_batch_beyond_2_to_the_32_tokens():
    """one batch whose token index passes 2^31 and 2^32 (rows of 81: > 16 GiB of walks), through the C entry
    points so that the atomic kernel runs; verified in row chunks with bincount / gather on the device.  The row
    of a token is t / len in 64 bits there: a 32-bit division would read the valid flag of a row near 0 for every
    token behind 2^32."""
    lib, L = _lib()
    length, nv = 81, 1 << 20
    marks = (1 << 31, 1 << 32)
    rows = marks[1] // length + 4096
    total = rows * length
    assert total >= (1 << 32) + 4000 * length
    batch = 4 * total
    need = 3 * batch
    gc.collect()
    torch.cuda.empty_cache()  # what earlier tests left in the allocator's cache is free for this one
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need} bytes of free device memory (3 x a batch of {batch} bytes), {free} are free")
    gen = torch.Generator(device=DEV).manual_seed(81)
    step = 1 << 20  # rows per chunk
    walks = torch.empty((rows, length), dtype=torch.int32, device=DEV)
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        walks[lo:hi] = torch.randint(-2, nv + 2, (hi - lo, length), generator=gen, device=DEV, dtype=torch.int32)
    valid = (torch.rand(rows, generator=gen, device=DEV) < 0.8).to(torch.uint8)
    valid[:64] = 0  # where a token index taken modulo 2^32 would look
    flat = walks.view(-1)
    planted = torch.tensor([nv - 1, INT32_MAX, -1, nv, 0, INT32_MIN], dtype=torch.int32, device=DEV)
    for mark in marks:  # out-of-range tokens and a dropped row on both sides of the mark
        flat[mark - 2:mark + 4] = planted
        r = mark // length
        valid[r - 1], valid[r], valid[r + 1] = 0, 1, 0
        valid[r + 2:r + 40] = 1
    valid[rows - 1] = 1
    index_of = torch.randperm(nv, generator=gen, device=DEV).to(torch.int32)
    index_of[::7] = -1
    counts = torch.zeros(nv, dtype=torch.int64, device=DEV)
    counts[7] = 5
    idx = torch.full((rows, length), -7, dtype=torch.int32, device=DEV)
    stream = lib.current_stream_ptr()
    lib.check(L.n2v_corpus_count(walks.data_ptr(), valid.data_ptr(), rows, length, nv, counts.data_ptr(), stream),
              "n2v_corpus_count")
    lib.check(L.n2v_corpus_index(walks.data_ptr(), valid.data_ptr(), index_of.data_ptr(), rows, length, nv,
                                 idx.data_ptr(), stream), "n2v_corpus_index")
    torch.cuda.synchronize()
    want = torch.zeros(nv, dtype=torch.int64, device=DEV)
    want[7] = 5
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        w = walks[lo:hi]
        ok = valid[lo:hi].bool().unsqueeze(1) & (w >= 0) & (w < nv)
        want += torch.bincount(w[ok].long(), minlength=nv)
        ref = torch.where(ok, index_of[w.clamp(0, nv - 1).long()], torch.full_like(w, -1))
        assert torch.equal(idx[lo:hi], ref), f"indices of rows {lo}..{hi}"
    assert torch.equal(counts, want), f"{int((counts != want).sum())} counts differ"
    print(f"ran: {rows} rows of {length} = {total} tokens, {batch} bytes of walks, {free} bytes were free")
