"""Case builders for the setup and corpus kernels (K1 n2v_alias_build, n2v_edge_bias, n2v_alias_draw,
n2v_walk_uniforms, n2v_trim_mark, n2v_cum_index_build), shared by test_setup_cases_host.py -- which proves on
the CPU that the cases are what they claim to be -- and test_setup_kernels_gpu.py, which runs the kernels on
them.  numpy only: nothing here needs a device.

"Past one grid pass": a CU holds at most 32 waves (8 per SIMD x 4 SIMDs), so no launch has more than
CUs x 32 waves resident.  A wave-per-row kernel given 2 x CUs x 32 + 3 rows, or a 256-thread streaming
kernel whose grid is capped at resident_blocks x m given 2 x (CUs x 32 x 64 x m) + 131 items, must take
the stride trip of its loop at least once whatever occupancy the launcher found."""
import numpy as np

WAVES_PER_CU = 32  # 8 per SIMD x 4 SIMDs


def rows_past_one_pass(cus):
    """rows for a wave-per-row kernel (K1)"""
    return 2 * cus * WAVES_PER_CU + 3


def items_past_one_pass(cus, m):
    """items for a one-item-per-thread kernel whose launcher caps the grid at resident_blocks x m"""
    return 2 * (cus * WAVES_PER_CU * 64 * m) + 131


# ---- K1: rows built deliberately ---------------------------------------------------------------------
ALIAS_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4099)
PHI = 0.6180339887498949


def _frac(n, mult=PHI):
    """n fp64 values in (0, 1) that are not fp32 values, no generator involved"""
    x = (np.arange(1, n + 1, dtype=np.float64) * mult) % 1.0
    return x


def _pattern_rows(n):
    """(name, fp64 weights) of every weight pattern that means something at length n"""
    out = [("equal_exact", np.full(n, 2.0))]
    if n in (64, 65):
        # equal and not exactly representable: the sum rounds, so every prob is one ulp-or-so off 1.0 --
        # all of them above it (0.1: the [0.1] * 10 quirk of G1) or all of them below it (0.7)
        out.append(("equal_decimal", np.full(n, 0.1)))
        out.append(("equal_decimal_under", np.full(n, 0.7)))
    if n >= 2:
        for k in sorted({0, n - 1, 63, 64}):
            if k < n:
                w = np.ones(n)
                w[k] = float(n)  # one overfull, every other slot underfull
                out.append((f"heavy_at_{k}", w))
                w = np.ones(n)
                w[k] = 0.25  # one underfull: every overfull it touches is demoted in turn
                out.append((f"light_chain_{k}", w))
        # avg is exactly 1.0: the one underfull pairs once with the top overfull, which stays (prob 1.0)
        w = np.ones(n)
        w[0], w[n - 1] = 0.5, 1.5
        out.append(("light_once", w))
        # zeros among positive weights
        w = np.ones(n)
        w[::3] = 0.0
        if n == 2:
            w[:] = (0.0, 1.0)
        out.append(("zeros", w))
    if n >= 3:
        # last underfull in chunk 0, the only overfull above 1.0 in the last chunk; and the mirror image
        w = np.ones(n)
        w[1], w[n - 2] = 0.25, 1.75
        out.append(("under_low_over_high", w))
        w = np.ones(n)
        w[1], w[n - 2] = 1.75, 0.25
        out.append(("over_low_under_high", w))
        out.append(("not_fp32", 0.1 + 1.9 * _frac(n)))
        out.append(("not_fp32_b", 0.05 + _frac(n, 0.7548776662466927) ** 3))
        dec = np.float32(10.0) ** np.linspace(-12.0, 12.0, n).astype(np.float32)
        out.append(("decades_f32", dec.astype(np.float32).astype(np.float64)))
        out.append(("decades_f32_desc", dec[::-1].astype(np.float32).astype(np.float64)))
    return out


def alias_rows():
    """[(name, fp64 weights)]: every length x every pattern, the G1 ulp quirk ([0.1] * 10) and empty rows at
    the start, the end and in between"""
    rows = [("empty_first", np.zeros(0)), ("decimal_10", np.full(10, 0.1)), ("decimal_under_10", np.full(10, 0.7))]
    for n in ALIAS_LENGTHS:
        for name, w in _pattern_rows(n):
            rows.append((f"{name}/{n}", w))
        rows.append((f"empty_after/{n}", np.zeros(0)))
    rows.append(("empty_last", np.zeros(0)))
    return rows


def is_f32(w):
    return bool(np.array_equal(w.astype(np.float32).astype(np.float64), w))


def pack_rows(weights):
    """CSR over a list of weight rows: rowptr int64, col int32 (ascending inside a row, NOT the position:
    the alias vertex has to come out of col), weights concatenated fp64"""
    lens = np.array([len(w) for w in weights], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.arange(int(rowptr[-1]), dtype=np.int64) - np.repeat(rowptr[:-1], lens)
    col = (7 * pos + 3 + np.repeat(np.arange(len(lens)) % 5, lens)).astype(np.int32)
    w = np.concatenate(weights).astype(np.float64) if len(weights) else np.zeros(0)
    return rowptr, col, w


def alias_trace(weights):
    """generate_alias_tables restated with its events kept: (alias, probs, facts).  facts: pairings,
    demotions (the overfull indices demoted, in order), initial_under / initial_over (stack sizes before the
    loop), left ("under" / "over": the stack that is not empty at the end), left_prob (prob of its top),
    last_demoted (the last iteration demoted the last overfull), demoted_then_paired."""
    w = [float(x) for x in weights]
    n = len(w)
    avg = sum(w) / n
    probs = [x / avg for x in w]
    alias = [0] * n
    under = [i for i in range(n) if probs[i] < 1.0]
    over = [i for i in range(n) if not probs[i] < 1.0]
    facts = {"pairings": 0, "demotions": [], "initial_under": len(under), "initial_over": len(over),
             "last_demoted": False}
    while under and over:
        u, o = under.pop(), over.pop()
        alias[u] = o
        probs[o] = probs[o] + probs[u] - 1.0
        facts["pairings"] += 1
        if probs[o] < 1.0:
            under.append(o)
            facts["demotions"].append(o)
            facts["last_demoted"] = not over
        else:
            over.append(o)
            facts["last_demoted"] = False
    facts["left"] = "under" if under else "over"
    facts["left_prob"] = probs[under[-1]] if under else probs[over[-1]]
    # an index that was an alias target, fell below 1.0 and was then paired as an underfull itself
    facts["demoted_then_paired"] = len(facts["demotions"]) - (1 if facts["last_demoted"] else 0)
    return alias, probs, facts


def short_rows_graph(n_rows, seed=5, zero=False):
    """n_rows rows of 0 .. 9 slots with fp32 weights; empty rows at the very start, at the very end and in
    runs (one run in each half).  Row n_rows - 6 (in the last trip of any launch) has three slots; with
    `zero` their weights are 0 and nothing else changes.  Returns rowptr, col, w, that row."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, n_rows)
    lens[:3] = 0
    lens[-2:] = 0
    lens[n_rows // 5: n_rows // 5 + 40] = 0
    lens[n_rows - n_rows // 7: n_rows - n_rows // 7 + 25] = 0
    z = n_rows - 6
    lens[z] = 3
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(rowptr[:-1], lens)
    col = (3 * pos + np.repeat(np.arange(n_rows) % 11, lens)).astype(np.int32)
    w = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 1.7, 0.3, 0.1, 5.5], np.float32), nnz)
    if zero:
        w[rowptr[z]:rowptr[z + 1]] = 0.0
    return rowptr, col, w.astype(np.float32), z


def expected_slots(oracle, rowptr, col, w, skip=()):
    """(col, alias VERTEX, prob bits) of K1 over the whole CSR from the oracle, row by row; rows in `skip`
    and empty rows produce nothing"""
    alias_v = np.zeros(len(col), np.int32)
    prob = np.zeros(len(col), np.float64)
    done = np.zeros(len(col), bool)
    for r in range(len(rowptr) - 1):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if e == b or r in skip:
            continue
        a, p = oracle.alias_tables(np.asarray(w[b:e], np.float64))
        alias_v[b:e] = col[b:e][np.asarray(a)]
        prob[b:e] = p
        done[b:e] = True
    return alias_v, prob.view(np.uint64), done


# ---- n2v_edge_bias ------------------------------------------------------------------------------------
SRC_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 1000)
SRC_BASE, SRC_STEP = 10, 3  # a source list is SRC_BASE + SRC_STEP * arange(m) (+ a per-row shift)


class BiasCase:
    """packed rows for n2v_edge_bias: rowptr / ids / w64 of the destination lists, src_id per row,
    src_rowptr / src_nbs of the source lists"""

    def __init__(self, rowptr, ids, w64, src_id, src_rowptr, src_nbs, src_shift):
        self.rowptr, self.ids, self.w64 = rowptr, ids, w64
        self.src_id, self.src_rowptr, self.src_nbs, self.src_shift = src_id, src_rowptr, src_nbs, src_shift
        self.w32 = w64.astype(np.float32)

    @property
    def n_rows(self):
        return len(self.rowptr) - 1

    def row_of_entry(self):
        return np.repeat(np.arange(self.n_rows), np.diff(self.rowptr))

    def classes(self):
        """per entry: 0 return (x == s), 1 shared (x in N(s)), 2 other, 3 first step (s < 0) -- membership
        in closed form from the arithmetic shape of the source lists"""
        row = self.row_of_entry()
        s = self.src_id[row].astype(np.int64)
        x = self.ids.astype(np.int64)
        m = np.diff(self.src_rowptr)[row]
        off = x - (SRC_BASE + self.src_shift[row])
        member = (off >= 0) & (off % SRC_STEP == 0) & (off // SRC_STEP < m)
        cls = np.where(member, 1, 2)
        cls[x == s] = 0
        cls[s < 0] = 3
        return cls

    def classes_by_search(self):
        """the same by looking every id up in its row's source list"""
        cls = np.empty(len(self.ids), np.int64)
        for r in range(self.n_rows):
            b, e = self.rowptr[r], self.rowptr[r + 1]
            nb = set(self.src_nbs[self.src_rowptr[r]:self.src_rowptr[r + 1]].tolist())
            s = int(self.src_id[r])
            for i in range(b, e):
                x = int(self.ids[i])
                cls[i] = 3 if s < 0 else 0 if x == s else 1 if x in nb else 2
        return cls

    def expected(self, p, q, w):
        """w / p, w, w / q in float64: one division each"""
        w = w.astype(np.float64)
        cls = self.classes()
        return np.where(cls == 0, w / p, np.where(cls == 2, w / q, w))


def _assemble_bias(rows):
    """rows: [(dst ids ascending, src_id, m, shift)]"""
    lens = np.array([len(r[0]) for r in rows], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = (np.concatenate([np.asarray(r[0], np.int64) for r in rows]) if rows else np.zeros(0)).astype(np.int32)
    src_id = np.array([r[1] for r in rows], np.int32)
    ms = np.array([r[2] for r in rows], np.int64)
    shift = np.array([r[3] for r in rows], np.int64)
    src_rowptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    inner = np.arange(int(src_rowptr[-1]), dtype=np.int64) - np.repeat(src_rowptr[:-1], ms)
    src_nbs = (SRC_BASE + np.repeat(shift, ms) + SRC_STEP * inner).astype(np.int32)
    w64 = 0.1 + 1.9 * _frac(len(ids), 0.7548776662466927)
    return BiasCase(rowptr, ids, w64, src_id, src_rowptr, src_nbs, shift)


def bias_edges_case():
    """every source-list length x every probe position, with first-step rows (src < 0) interleaved and
    empty destination rows first, last and in runs"""
    rows = [([], 5, 0, 0), ([], -1, 0, 0)]
    for j, m in enumerate(SRC_LENGTHS):
        shift = j  # lists that start at different residues
        first = SRC_BASE + shift
        last = first + SRC_STEP * (m - 1) if m else first
        mid = first + SRC_STEP * (m // 2)
        probes = {first, last, first - 1, last + 1, first - 7, last + 50, mid, mid + 1, first + SRC_STEP,
                  last - SRC_STEP, last - 1}
        probes = sorted(x for x in probes if x >= 0)
        # s outside the source list and outside the row; s a member of its own source list AND in the row
        # (w / p must win over "shared"); s in the row but not a member; a first step
        rows.append((probes, 4_000_000 + j, m, shift))
        rows.append((sorted(set(probes) | {mid}), mid, m, shift))
        rows.append(([], mid, m, shift))
        rows.append((sorted(set(probes) | {first - 2}), first - 2, m, shift))
        rows.append((probes, -(j % 3) - 1, m, shift))
        if j % 3 == 0:
            rows += [([], -2, 0, 0), ([], 7, m, shift), ([], 7, 0, 0)]
    rows += [([], 3, 0, 0), ([], -1, 0, 0)]
    return _assemble_bias(rows)


def bias_stride_case(nnz):
    """exactly nnz destination entries over rows whose lengths cycle through 0, 5, 0, 0, 1000, 17, 64, 0,
    source lists cycling through SRC_LENGTHS, every seventh row a first step; ends on empty rows"""
    cyc = (0, 5, 0, 0, 1000, 17, 64, 0)
    per = sum(cyc)
    n_cyc = nnz // per + 1
    lens = np.tile(np.array(cyc, np.int64), n_cyc)
    cum = np.cumsum(lens)
    cut = int(np.searchsorted(cum, nnz, side="left"))
    lens = lens[:cut + 1].copy()
    lens[cut] -= int(cum[cut]) - nnz
    lens = np.concatenate([lens, np.zeros(3, np.int64)])
    n_rows = len(lens)
    r = np.arange(n_rows)
    ms = np.array(SRC_LENGTHS, np.int64)[(r + r // len(cyc)) % len(SRC_LENGTHS)]  # every length meets every row
    ms = np.where(lens == 0, 0, ms)
    shift = (r % 4).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    row = np.repeat(r, lens)
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(rowptr[:-1], lens)
    ids = (SRC_BASE - 4 + 2 * pos + row % 3).astype(np.int32)  # ascending, distinct inside a row
    src_id = np.where(r % 7 == 0, -1 - r % 3, SRC_BASE + shift + SRC_STEP * (r % 5) + (r % 2)).astype(np.int32)
    src_rowptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    inner = np.arange(int(src_rowptr[-1]), dtype=np.int64) - np.repeat(src_rowptr[:-1], ms)
    src_nbs = (SRC_BASE + np.repeat(shift, ms) + SRC_STEP * inner).astype(np.int32)
    w64 = 0.1 + 1.9 * _frac(nnz, 0.7548776662466927)
    return BiasCase(rowptr, ids, w64, src_id, src_rowptr, src_nbs, shift)


# ---- n2v_alias_draw -----------------------------------------------------------------------------------
def draw_table(lens, seed=3):
    """an arbitrary table over rows of the given lengths: col ascending ids, alias an INDEX into the row,
    prob a multiple of 1/8 in [0, 1] (so that r2 == prob[pick] can be hit exactly)"""
    lens = np.asarray(lens, np.int64)
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(rowptr[:-1], lens)
    col = (5 * pos + 2).astype(np.int32)
    alias_idx = (rng.integers(0, 1 << 30, nnz) % np.repeat(np.maximum(lens, 1), lens)).astype(np.int32)
    prob = rng.integers(0, 9, nnz).astype(np.float64) / 8.0
    return rowptr, col, alias_idx, prob


def draw_expected(rowptr, col, alias_idx, prob, r1, r2):
    """sampling_from_alias / _wiki (r2 None) + the neighbour lookup in numpy: the vertex per row, -1 for an
    empty row and for a pick outside the row"""
    n = np.diff(rowptr)
    scaled = r1 * n.astype(np.float64)
    pick = np.trunc(scaled).astype(np.int64)  # int() truncates toward zero
    bad = (n <= 0) | (pick < 0) | (pick >= n)
    at = np.where(bad, 0, rowptr[:-1] + pick)
    at = np.minimum(at, max(len(col) - 1, 0))
    y = r2 if r2 is not None else scaled - pick.astype(np.float64)
    if len(col) == 0:
        return np.full(len(n), -1, np.int32), bad & (n > 0)
    keep = y < prob[at]
    alias_at = rowptr[:-1] + alias_idx[at]
    alias_at = np.minimum(alias_at, len(col) - 1)
    v = np.where(keep, col[at], col[alias_at])
    return np.where(bad, -1, v).astype(np.int32), bad & (n > 0)


DRAW_EDGE_LENGTHS = (0, 1, 3, 64, 3000, 0, 0, 1, 3, 64, 3000, 7, 0)


# ---- n2v_walk_uniforms --------------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform_bits(seed, keys, steps):
    """(u1, u2) uint32 arrays of DESIGN.md "RNG": walker_stream then step_bits, in wrapping uint64"""
    with np.errstate(over="ignore"):
        k = np.asarray(keys).astype(np.int64).view(np.uint64)
        h0 = _mix64(np.uint64(seed) ^ _mix64(k + np.uint64(0x9E3779B97F4A7C15)))
        st = np.asarray(steps).astype(np.int32).view(np.uint32).astype(np.uint64)
        bits = _mix64(h0 + (st + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03))
    return (bits >> np.uint64(32)).astype(np.uint32), (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def uniform_keys(n, seed=9):
    """keys over the whole int64 range (ends included) and steps 0 .. 200"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
    keys[:4] = (0, 1, -1, 2 ** 63 - 1)
    keys[-2:] = (-2 ** 63, 12345)
    steps = rng.integers(0, 201, n).astype(np.int32)
    steps[:2] = (0, 2 ** 31 - 1)
    return keys, steps


# ---- n2v_trim_mark ------------------------------------------------------------------------------------
def trim_rowptr(n_rows, cap):
    """degrees cycling through cap - 1, cap, cap + 1, 2 cap, 0, 1, with a hot row first and last"""
    cyc = np.array([cap + 1, cap - 1, cap, 2 * cap, 0, 1, cap + 1], np.int64)
    deg = np.maximum(cyc[np.arange(n_rows) % len(cyc)], 0)
    deg[0], deg[-1] = 2 * cap + 1, cap + 1
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


TRIM_ROWS = (63, 64, 65, 129)
TRIM_CAPS = (7, 1)


# ---- n2v_cum_index_build ------------------------------------------------------------------------------
CUM_DOMAIN = 2 ** 31 - 1


def runs_counts(n_side):
    """counts whose make_cum_table has runs of equal neighbours: n_side words of count 1, one word of
    count 10^16, n_side words of count 1.  The first run is a run of ZEROS, which the bucket edge 0 hits
    exactly; the words after the giant round to a handful of values just below 2^31 - 1."""
    return np.concatenate([np.ones(n_side, np.int64), [10 ** 16], np.ones(n_side, np.int64)])


def edge_hitting_table(bits, run=5):
    """a table made by hand whose runs sit EXACTLY on bucket edges b << (31 - bits): the case where
    bisect_left and bisect_right differ by the length of the run"""
    edges = (np.arange(1, 1 << bits, 37, dtype=np.int64) << (31 - bits))
    tab = np.sort(np.concatenate([np.repeat(edges, run), [0, 0, 1], [CUM_DOMAIN]]))
    return tab.astype(np.int64)


def cum_index_expected(tab, bits):
    """index[b] = bisect_left(tab, b << (31 - bits)) for b in 0 .. 2^bits; the last entry (2^31, above
    every table value) is the vocabulary size"""
    edges = np.arange((1 << bits) + 1, dtype=np.int64) << (31 - bits)
    return np.searchsorted(np.asarray(tab, np.int64), edges, side="left").astype(np.int32)
