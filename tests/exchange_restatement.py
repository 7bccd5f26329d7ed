"""The replica exchange of the multi-GPU SGNS path, restated: numpy only, one fp32 operation per line.

What csrc/n2v_sync.hip (ref_init / pack / reduce / apply) and their host forms in sgns.DeltaSync and
shard._rank_ordered_reduce are held to (tests/test_exchange_host.py, tests/test_exchange_edges_gpu.py).
Written from the protocol, not from either implementation, and importing neither:

  ref_init   ref  = bf16(cur)
  pack       wire = cur                      (fp32 wire)      before = cur when a snapshot is asked for
             wire = bf16(cur - f32(ref))     (bf16 wire)
  sum        acc  = p[0]; acc = acc + p[r] for r = 1 .. world - 1, in fp32; one rounding to the wire type
  apply      mean = sum / world                              (fp32 wire)
             mean = f32(ref) + f32(sum) / world; ref = bf16(mean)   (bf16 wire)
             cur  = mean                     (set form, no snapshot)
             cur  = cur + (mean - before)    (add form)

bf16 lives in uint16 arrays.  fp32 -> bf16 is round to nearest, ties to even, in integer arithmetic on
the bit pattern; a NaN goes to a NaN.  bf16 -> fp32 is `bits << 16`.  numpy's float32 +, -, / are the
correctly rounded IEEE operations and keep subnormals.

Not a test module: helpers shared by the two.
"""
import numpy as np

F32, U16, U32 = np.float32, np.uint16, np.uint32


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == F32, a.dtype
    return a


def _bits16(a):
    a = np.asarray(a)
    assert a.dtype == U16, a.dtype
    return a


def f32_to_bf16(x):
    """round to nearest even on the uint32 view; NaN in, (quiet) NaN out"""
    u = _f32(x).view(U32).astype(np.uint64)
    is_nan = (u & 0x7FFFFFFF) > 0x7F800000
    lsb = (u >> 16) & 1  # the bit that becomes the last place: ties go to where it is 0
    rounded = (u + 0x7FFF + lsb) >> 16  # (an overflow of the mantissa carries into the exponent: up to inf)
    quiet = (u >> 16) | 0x0040
    return np.where(is_nan, quiet, rounded).astype(U16)


def bf16_to_f32(b):
    return (_bits16(b).astype(U32) << 16).view(F32)


def is_nan16(b):
    return (_bits16(b) & 0x7FFF) > 0x7F80


def ref_init(cur):
    return f32_to_bf16(cur)


def pack(cur, ref=None, snapshot=False):
    """-> (wire, before): wire float32 (ref None) or bf16 bits; before a copy of cur, or None"""
    cur = _f32(cur)
    before = cur.copy() if snapshot else None
    if ref is None:
        return cur.copy(), before
    with np.errstate(all="ignore"):
        r = bf16_to_f32(ref)
        d = cur - r
    return f32_to_bf16(d), before


def rank_sum(parts):
    """parts: one wire array per rank, in rank order -> their sum in the wire type"""
    bf16 = parts[0].dtype == U16
    with np.errstate(all="ignore"):
        acc = bf16_to_f32(parts[0]) if bf16 else _f32(parts[0]).copy()
        for p in parts[1:]:
            acc = acc + (bf16_to_f32(p) if bf16 else _f32(p))
    return f32_to_bf16(acc) if bf16 else acc


def apply(cur, ref, before, wire_sum, world):
    """-> (cur', ref'): ref' None on the fp32 wire.  before None = set form, else add form."""
    cur = _f32(cur)
    w = F32(world)
    with np.errstate(all="ignore"):
        if ref is None:
            mean = _f32(wire_sum) / w
            new_ref = None
        else:
            s = bf16_to_f32(wire_sum)
            q = s / w
            r = bf16_to_f32(ref)
            mean = r + q
            new_ref = f32_to_bf16(mean)
        if before is None:
            return mean.copy(), new_ref
        d = mean - _f32(before)
        out = cur + d
    return out, new_ref


def exchange(replicas, refs, block_rows, exact, meanwhile=None):
    """One blocked exchange over world = len(replicas) replicas.
    replicas[r][k]: float32 matrix k of rank r; refs[r][k]: its bf16 reference (bits), or refs None
    for the fp32 wire; meanwhile[r][k]: what matrix k of rank r holds when apply reaches it (training
    went on after the snapshot; add form only).  -> (new replicas, new refs), nothing is changed in place."""
    world = len(replicas)
    out = [[m.copy() for m in rep] for rep in replicas]
    out_refs = None if refs is None else [[m.copy() for m in rr] for rr in refs]
    for k in range(len(replicas[0])):
        rows = replicas[0][k].shape[0]
        for lo in range(0, rows, block_rows):
            hi = min(rows, lo + block_rows)
            packed = [pack(replicas[r][k][lo:hi].reshape(-1),
                           None if refs is None else refs[r][k][lo:hi].reshape(-1), not exact)
                      for r in range(world)]
            total = rank_sum([w for w, _ in packed])
            for r in range(world):
                now = replicas[r][k] if meanwhile is None else meanwhile[r][k]
                cur, ref = apply(now[lo:hi].reshape(-1),
                                 None if refs is None else refs[r][k][lo:hi].reshape(-1),
                                 packed[r][1], total, world)
                out[r][k][lo:hi] = cur.reshape(out[r][k][lo:hi].shape)
                if ref is not None:
                    out_refs[r][k][lo:hi] = ref.reshape(out_refs[r][k][lo:hi].shape)
    return out, out_refs


# -- comparison: raw bits (so -0 != +0), except that a NaN is only required to be a NaN -------------------

def count_differing(got, want):
    """count of elements where `got` departs from `want` (both float32, or both bf16 bits)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype == U16:
        g_nan, w_nan, g, w = is_nan16(got), is_nan16(want), got, want
    else:
        g_nan, w_nan = np.isnan(_f32(got)), np.isnan(_f32(want))
        g, w = np.ascontiguousarray(got).view(U32), np.ascontiguousarray(want).view(U32)
    bad = np.where(w_nan, ~g_nan, g != w)
    return int(bad.sum())


def assert_same_bits(got, want, what=""):
    bad = count_differing(got, want)
    if bad:
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        view = (lambda a: a) if want.dtype == U16 else (lambda a: np.ascontiguousarray(a).view(U32))
        g, w = view(got), view(want)
        nan = is_nan16(want) if want.dtype == U16 else np.isnan(want)
        g_nan = is_nan16(got) if want.dtype == U16 else np.isnan(got)
        at = np.flatnonzero(np.where(nan, ~g_nan, g != w))[:5]
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %s want %s" % (
            what, bad, want.size, at.tolist(), [hex(int(x)) for x in g[at]], [hex(int(x)) for x in w[at]]))


# -- the values where a pass goes wrong --------------------------------------------------------------------

def _bits(*words):
    return np.array(words, dtype=U32)


def special_values(seed=1):
    """float32 vector: signed zeros and infinities, NaNs, the ends of the subnormal range, FLT_MIN, FLT_MAX
    (rounds to bf16 inf), bf16 ties to the even and to the odd side in both signs with the values one fp32
    ulp either side, ties that carry into the exponent, and a sweep 2^-140 .. 2^127 with random mantissas"""
    fixed = _bits(
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,               # +-0, +-inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF,   # NaNs, quiet and signalling payloads
        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,               # smallest / largest subnormal
        0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,               # FLT_MIN, FLT_MAX
        0x3F808000, 0xBF808000, 0x3F818000, 0xBF818000,               # ties: kept bit even (down), odd (up)
        0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,               # one ulp either side
        0xBF807FFF, 0xBF808001, 0xBF817FFF, 0xBF818001,
        0x3FFF8000, 0x3FFF7FFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000,   # ties that carry: next binade, inf
        0x00008000, 0x00018000, 0x00007FFF, 0x00008001, 0x80008000,   # ties below the smallest bf16 subnormal
        0x007F8000, 0x007FFFFF, 0x00808000,                           # subnormal -> normal by rounding
        0x3F800000, 0xBF800000, 0x40400000, 0x3EAAAAAB, 0x3DCCCCCD)   # 1, -1, 3, 1/3, 0.1
    rng = np.random.default_rng(seed)
    sweep = []
    for e in range(-140, 128):
        for _ in range(4):
            sign = int(rng.integers(0, 2)) << 31
            if e >= -126:
                word = ((e + 127) << 23) | int(rng.integers(0, 1 << 23))
            else:
                top = 1 << (e + 149)  # subnormal with leading bit 2^e
                word = top | int(rng.integers(0, top))
            sweep.append(sign | word)
    return np.concatenate([fixed, np.array(sweep, dtype=U32)]).view(F32)


def cancelling_pairs():
    """(cur float32, ref bf16 bits): cur - f32(ref) is exactly 0 (both signs of the operands), a subnormal,
    the smallest subnormal, overflows bf16 but not fp32, overflows fp32, inf - inf"""
    cur = _bits(0x3F800000, 0xBF800000, 0x00000000, 0x80000000,   # x - x = +0
                0x00800001, 0x00FFFFFF, 0x80800001, 0x00810000,   # near FLT_MIN: subnormal differences
                0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,               # FLT_MAX - 0: bf16 overflow
                0x7F000000, 0xFF000000,                           # 2^127 - (-2^127): fp32 overflow
                0x7F800000, 0xFF800000, 0x7F800000,               # inf - inf = NaN, inf - (-inf) = inf
                0x3F808000, 0x3F818000).view(F32)                 # a tie in the difference (ref = 0)
    ref = np.array([0x3F80, 0xBF80, 0x0000, 0x8000,
                    0x0080, 0x0100, 0x8080, 0x0080,
                    0x0000, 0x8000, 0x0000,
                    0xFF00, 0x7F00,
                    0x7F80, 0xFF80, 0xFF80,
                    0x0000, 0x8000], dtype=U16)
    return cur, ref


def edge_case(world, seed=2):
    """One fixed problem per world size built from the vectors above.
    -> (curs, ref, mids): curs[r] the float32 rows of rank r at pack, ref the shared bf16 reference (bits),
    mids[r] what rank r holds at apply (the add form).  Rank r sees the special vector rotated by 3 r + 1
    places, so the rank sums mix every kind of value with every other."""
    v = special_values(seed)
    pc, pr = cancelling_pairs()
    rng = np.random.default_rng(seed + 100)
    base = np.concatenate([pc, v])
    # reference: the pairs' own, then bf16 of a neighbour of each special value (a small difference), and of a
    # far one on every fourth place (a large one)
    near = f32_to_bf16(v)
    far = f32_to_bf16(np.roll(v, 17))
    ref = np.concatenate([pr, np.where(np.arange(v.size) % 4 == 3, far, near)]).astype(U16)
    curs, mids = [], []
    for r in range(world):
        c = base.copy()
        if r:
            c[pc.size:] = np.roll(v, 3 * r + 1)
        curs.append(c)
        with np.errstate(all="ignore"):
            step = (rng.standard_normal(c.size) * 0.01).astype(F32)
            mids.append(c + step)
    return curs, ref, mids
