"""Rows for the dyadic closed forms of the exact step (csrc/n2v_unit_core.h, n2v_wedge_step.h): numpy and fractions
only, no device.

A case is (cls, p, q): cls a string over {R, M, O} -- the class of every slot of the row N(v) seen from the previous
vertex s: R leads back to s (one run: rows are sorted by id), M to a neighbour of s, O to neither -- and the reference
draws the step from generate_alias_tables([1/p if R, 1 if M, 1/q if O]) (randomwalk.py:157-232).

The CELL of a case says which code the step runs.  It is computed here from the reference's definition alone, in exact
rational arithmetic (nothing of scripts/models is imported):

  instance     0 if 1/q <= 1 and 1/p >= 1/q; 3 if 1/q >= 1 and 1/p <= 1/q; 1 otherwise
  arrangement  a class is underfull when its value b < avg (a return or shared class without a slot takes no side):
               1 "other" alone underfull, 2 "other" alone overfull, 3 return + "other" underfull and shared overfull,
               4 return + "other" overfull and shared underfull, 5 return alone overfull, 0 any other row with both
               stacks non-empty, "none" one stack empty.  (2 and 4 need an "other" slot; for 1, 3 and 5 the VALUE 1/q
               decides.)  With p == q a return slot counts as "other", with q == 1 a shared slot does.
  size         n <= 64 or n > 64;  list  0, 1 - 14 or >= 15 shared slots (after the merges above)
  tie          the pairing loop run on fractions: some updated probs[over] equals exactly 1 while a stack still holds
               a slot (the last update of EVERY row gives exactly 1: the row sums to n)

Cells that cannot exist (no_cell() below gives the reason per cell):
  * instance 0 makes 1/q the smallest of the three values: "other" is underfull on every row with two stacks, so no
    row has arrangement 0, 2 or 4 (each has "other" overfull, or no underfull "other" value);
  * instance 3 makes 1/q the largest: "other" is never underfull, so no row has arrangement 1, 3 or 5;
  * arrangements 0, 3, 4 and 5 put the return and the shared class on different stacks: they need a shared slot,
    so their cells with an empty list do not exist.

Families: A every composition of 2 .. 5 slots x 14 pairs; B the cuts (row length 63 | 64 | 65, list length 14 | 15 | 16
and 300, return run 0, 1, 2, 64, 127 | 128, 200; the run first, in the middle and last; shared slots directly beside it);
C ties on rows of <= 64 and of 65 .. 400 slots in every cell (with a tie-free row beside each); D rows of 4096 and
20 000 slots where one or two overfull slots absorb thousands of equal underfull ones; E values such as
1/p = 1 + 2^-20, whose reduced integers are near 2^20: the same short rows under all nine pairs, and rows at 0.9 and
1.1 times the length at which dn * isum reaches 2.0e14, the first product of the forms' exactness guards.
Every pair of every family passes the library's own predicate for dyadic values (library_dyadic()).

(E, arrangement 4 at the guard: it needs 1 < 1/q < 1/p with (1/p - 1) nR < (1/q - 1) n; the family's values above 1
are 1 + 2^-20 and 1.5 alone, which would take nM > 2^19 nR.  Arrangement 4 meets the awkward values on short rows
only; arrangements 1, 2, 3 and 5 stand on both sides of the guard.)

Every row also carries the number of walkers W the GPU test starts on its s (layout(): one graph per family and
(p, q)); test_closed_form_cases_host.py proves that with SEED and W the draws reach what they must.
"""
import math
from fractions import Fraction

import numpy as np

from step_rows import _Rows, _uniform_bits

SEED = 20251020
E20 = 2.0 ** -20

A_PAIRS = {0: [(0.5, 2.0), (0.25, 4.0), (2.0, 4.0), (0.5, 1.0), (2.0, 2.0)],
           3: [(4.0, 0.25), (2.0, 0.5), (1.0, 0.5), (2.0, 1.0), (0.5, 0.5)],
           1: [(4.0, 2.0), (8.0, 2.0), (0.25, 0.5), (0.125, 0.25)]}
# the cuts: two pairs per instance, so that every arrangement of the instance occurs ((0.5, 0.25) is the only kind of
# pair under instance 3 with the return value above the average: arrangement 4)
B_PAIRS = [(0.5, 2.0), (2.0, 4.0), (4.0, 0.25), (0.5, 0.25), (4.0, 2.0), (0.25, 0.5)]


def library_dyadic(x):
    """the library's own predicate (scales_exactly, n2v_walk_unit.hip; randomwalk._dyadic), restated: 1/x * 2^20 is an
    exact integer in (0, 2^31) -- any other value sends the walk to the code for values that are not dyadic"""
    t = (1.0 / x) * 1048576.0
    return 0.0 < t < 2147483648.0 and t == float(int(t))


# (1/p = 1024 is the largest power of two that leaves room above it for 1/p * 2^20 < 2^31 ... 1536 = 1.5 * 1024 fits)
D_PAIRS = [(0.5, 1024.0), (2.0, 1.0 / 1024.0), (2048.0, 1024.0), (1.0 / 1536.0, 1.0 / 1024.0)]


def _pq(x, y):
    """(p, q) with 1/p = x and 1/q = y, both multiples of 2^-20 -- asserted on the doubles the kernels will see"""
    p, q = 1.0 / x, 1.0 / y
    for v, want in ((1.0 / p, x), (1.0 / q, y)):
        t = v * 1048576.0
        assert t == float(int(t)) and v == want, (x, y, v)
    assert library_dyadic(p) and library_dyadic(q)
    return p, q


# awkward dyadic values: (1/p, 1/q)
E_VALUES = [(1.5, 1.0 - E20), (1.0 + E20, 0.75), (1.0 + E20, 1.0 - E20),          # instance 0
            (0.75, 1.0 + E20), (1.0 - E20, 1.5), (1.0 - 2 * E20, 1.0 + E20),      # instance 3
            (0.75, 1.0 - E20), (1.0 - 2 * E20, 1.0 - E20), (1.5, 1.0 + E20)]      # instance 1
E_PAIRS = [_pq(x, y) for x, y in E_VALUES]
# short rows: every pair (three values within 2^-19 of each other give probabilities within 2^-14 of 1 on every short
# row: such slots are NAMED per row -- layout(), "unbracketable" -- and exempt from the two-sides condition alone)
E_SHORT_PAIRS = E_PAIRS
# at the guard: one pair per instance (two under instance 1: arrangements 1 - 3, and 5), (pair, arrangement, nR, nM)
E_GUARD = [(_pq(1.0 + E20, 1.0 - E20), 1, 2, 15), (_pq(1.0 + E20, 1.0 - E20), 1, 0, 40),
           (_pq(1.0 - E20, 1.5), 2, 2, 15), (_pq(1.0 - E20, 1.5), 2, 0, 40),
           (_pq(1.0 - 2 * E20, 1.0 - E20), 1, 0, 40), (_pq(1.0 - 2 * E20, 1.0 - E20), 2, 7, 0),
           (_pq(1.0 - 2 * E20, 1.0 - E20), 3, 7, 40), (_pq(1.5, 1.0 + E20), 5, 7, 40)]
GUARD_BOUND = 2.0e14


# ------------------------------------------------------------------------------------------- the cell
def instance(p, q):
    bR, bO = Fraction(1.0 / p), Fraction(1.0 / q)
    if bO <= 1 and bR >= bO:
        return 0
    if bO >= 1 and bR <= bO:
        return 3
    return 1


def effective(cls, p, q):
    """the classes as the table sees them: p == q makes a return slot an "other" slot, q == 1 a shared one"""
    if p == q:
        cls = cls.replace("R", "O")
    if q == 1.0:
        cls = cls.replace("M", "O")
    return cls


def _values(p, q):
    return {"R": Fraction(1.0 / p), "M": Fraction(1), "O": Fraction(1.0 / q)}


def arrangement(nR, nM, nO, p, q):
    """from the counts after the merges"""
    b = _values(p, q)
    n = nR + nM + nO
    avg = (nR * b["R"] + nM * b["M"] + nO * b["O"]) / n
    uR, uM, uO = b["R"] < avg, b["M"] < avg, b["O"] < avg
    under = (nR and uR) or (nM and uM) or (nO and uO)
    over = (nR and not uR) or (nM and not uM) or (nO and not uO)
    if not under or not over:
        return "none"
    r = None if nR == 0 else uR  # None: takes no side
    m = None if nM == 0 else uM
    if uO and r is not True and m is not True:
        return 1
    if not uO and nO > 0 and r is not False and m is not False:
        return 2
    if uO and r is True and m is False:
        return 3
    if not uO and nO > 0 and r is False and m is True:
        return 4
    if uO and r is False and m is True:
        return 5
    return 0


def exact_loop(cls, p, q):
    """the pairing loop of generate_alias_tables in exact arithmetic: every value is a fraction over the common
    denominator S = the row sum times a power of two, so integers t_i n against S.  -> (tie, alias, probs as fractions)"""
    b = _values(p, q)
    den = math.lcm(b["R"].denominator, b["O"].denominator)
    t = {c: int(b[c] * den) for c in "RMO"}
    n = len(cls)
    one = sum(t[c] for c in cls)
    probs = [t[c] * n for c in cls]
    alias = [0] * n
    under = [i for i in range(n) if probs[i] < one]
    over = [i for i in range(n) if probs[i] >= one]
    tie = False
    while under and over:
        u, o = under.pop(), over.pop()
        alias[u] = o
        probs[o] = probs[o] + probs[u] - one
        # (the LAST update gives exactly 1 on every row -- the row sums to n -- and decides nothing when both stacks
        # are empty then: an update counts when a stack still holds a slot, so that the side it takes is acted on)
        tie = tie or (probs[o] == one and bool(under or over))
        (under if probs[o] < one else over).append(o)
    return tie, alias, [Fraction(x, one) for x in probs]


def float_tables(cls, p, q):
    """the same loop in fp64, the additions of the row sum from left to right: the table the draws are compared with"""
    b = {"R": 1.0 / p, "M": 1.0, "O": 1.0 / q}
    w = [b[c] for c in cls]
    n = len(w)
    total = 0.0
    for x in w:
        total = total + x
    avg = total / n
    probs = [x / avg for x in w]
    alias = [0] * n
    under = [i for i in range(n) if probs[i] < 1.0]
    over = [i for i in range(n) if not probs[i] < 1.0]
    while under and over:
        u, o = under.pop(), over.pop()
        alias[u] = o
        probs[o] = probs[o] + probs[u] - 1.0
        (under if probs[o] < 1.0 else over).append(o)
    return np.array(alias), np.array(probs)


def list_class(nM):
    return 0 if nM == 0 else (1 if nM <= 14 else 2)


def cell(cls, p, q, tie=None):
    """(instance, arrangement, n > 64, list class) and whether the exact loop ties"""
    eff = effective(cls, p, q)
    nR, nM = eff.count("R"), eff.count("M")
    arr = arrangement(nR, nM, len(eff) - nR - nM, p, q)
    if tie is None:
        tie = exact_loop(eff, p, q)[0]
    return (instance(p, q), arr, len(cls) > 64, list_class(nM)), tie


def no_cell(inst, arr, lst):
    """the reason why no row lies in (inst, arr, any size, lst), or None"""
    if inst == 0 and arr in (0, 2, 4):
        return '1/q is the smallest value: "other" is underfull wherever two stacks exist'
    if inst == 3 and arr in (1, 3, 5):
        return '1/q is the largest value: "other" is never underfull'
    if lst == 0 and arr in (0, 3, 4, 5):
        return "return and shared class on different stacks: needs a shared slot"
    return None


def guard_product(cls, p, q):
    """dn * isum of the closed forms (lane_case_a_jump and its siblings), restated: isum = the row sum in units of
    2^-20 divided by the greatest common divisor of the three class values in those units"""
    t = [int(Fraction(1.0 / p) * 1048576), 1048576, int(Fraction(1.0 / q) * 1048576)]
    g = math.gcd(*t)
    eff = effective(cls, p, q)
    isum = sum(eff.count(c) * (x // g) for c, x in zip("RMO", t))
    return len(cls) * isum


# ------------------------------------------------------------------------------------------- the rows
def compose(n, nR, nM, where="middle", touch=True):
    """a row of n slots: the return run first, in the middle or last; with `touch` the first shared slots directly
    below and directly above the run, the others spread evenly over what is left"""
    assert nR + nM <= n and where in ("first", "middle", "last")
    rpos = {"first": 0, "middle": (n - nR) // 2, "last": n - nR}[where]
    cls = ["O"] * n
    for i in range(rpos, rpos + nR):
        cls[i] = "R"
    want = nM
    if touch and nR:
        for i in (rpos - 1, rpos + nR):
            if want and 0 <= i < n:
                cls[i] = "M"
                want -= 1
    free = [i for i in range(n) if cls[i] == "O"]
    for j in range(want):
        cls[free[(j * len(free)) // want]] = "M"
    return "".join(cls)


def family_a():
    """every return run (none, or any start and length) x every shared subset of the other slots, n = 2 .. 5"""
    out = []
    for n in range(2, 6):
        runs = [(0, 0)] + [(a, ln) for ln in range(1, n + 1) for a in range(n - ln + 1)]
        for a, ln in runs:
            rest = [i for i in range(n) if not a <= i < a + ln]
            for bits in range(1 << len(rest)):
                cls = ["R" if a <= i < a + ln else "O" for i in range(n)]
                for k, i in enumerate(rest):
                    if bits >> k & 1:
                        cls[i] = "M"
                out.append("".join(cls))
    return out


B_SHORT_N, B_LISTS, B_RUNS = (63, 64, 65), (0, 1, 14, 15, 16, 300), (0, 1, 2, 64, 127, 128, 200)
_WHERE = ("first", "middle", "last")


def family_b(p, q):
    """the grid of row lengths, list lengths and return runs; the place of the run rotates through the grid.  A row
    of a pair with p == q or q == 1 would lose its run or its list: B_PAIRS has no such pair"""
    out, k = [], 0
    for nM in B_LISTS:
        for nR in B_RUNS:
            for n in ((400,) if nM == 300 or nR >= 127 else B_SHORT_N):
                if nR + nM > n or (nR + nM == n and n == 400):
                    continue  # does not fit the row
                out.append(compose(n, nR, nM, _WHERE[k % 3]))
                k += 1
    # every arrangement of the pair at the three row lengths and on both sides of the list cut: the shortest run of
    # the grid's, else the shortest of all, that gives it
    for arr in range(6):
        for n in B_SHORT_N:
            for nM in (0, 1, 14, 15, 16):
                runs = [r for r in (0, 1, 2) + tuple(range(3, n - nM + 1))
                        if arrangement(r, nM, n - r - nM, p, q) == arr]
                if runs:
                    cls = compose(n, runs[0], nM, _WHERE[k % 3])
                    k += 1
                    if cls not in out:
                        out.append(cls)
    # the bit-mask replay with a run of 64 slots: the whole row, and the row of 65 with one slot beside it
    out += ["R" * 64, "R" * 64 + "M", "O" + "R" * 64]
    return out


def _search(p, q, want_cell, want_tie, sizes):
    """the first row of `sizes` in the wanted cell with / without a tie (counts in a fixed order, the three places)"""
    inst, arr, big, lst = want_cell
    lists = {0: (0,), 1: (1, 2, 3, 5, 8, 14), 2: (15, 16, 20, 24, 32, 40)}[lst]
    for n in sizes:
        for nM in lists:
            for nR in (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 100):
                if nR + nM > n:
                    continue
                if arrangement(*_merged_counts(n, nR, nM, p, q), p, q) != arr:
                    continue
                for where in _WHERE:
                    cls = compose(n, nR, nM, where, touch=where != "last")
                    got, tie = cell(cls, p, q)
                    if got == want_cell and tie == want_tie:
                        return cls
    return None


def _merged_counts(n, nR, nM, p, q):
    if p == q:
        nR = 0
    if q == 1.0:
        nM = 0
    return nR, nM, n - nR - nM


C_SHORT = (16, 20, 24, 30, 32, 36, 40, 45, 48, 50, 54, 56, 60, 63, 64)
C_LONG = (65, 66, 70, 72, 75, 80, 84, 90, 96, 100, 120, 128, 150, 160, 200, 240, 256, 300, 320, 400)
C_PAIRS = B_PAIRS


def family_c():
    """{cell: {tie: (cls, p, q)}} for every cell that exists: the first pair of C_PAIRS that has such a row"""
    if _C:
        return _C
    for inst in (0, 3, 1):
        for arr in range(6):
            for big in (False, True):
                for lst in range(3):
                    if no_cell(inst, arr, lst):
                        continue
                    for tie in (True, False):
                        for p, q in C_PAIRS:
                            if instance(p, q) != inst:
                                continue
                            cls = _search(p, q, (inst, arr, big, lst), tie, C_LONG if big else C_SHORT)
                            if cls is not None:
                                _C.setdefault((inst, arr, big, lst), {})[tie] = (cls, p, q)
                                break
    return _C


_C = {}


def family_d(p, q):
    """one or two overfull slots among thousands of equal underfull ones, and the mirror"""
    out = []
    bR, bO = 1.0 / p, 1.0 / q
    for n in (4096, 20000):
        if bO < 1.0 and bR >= bO:     # arrangement 1: "other" = 2^-10 underfull; two shared slots / a run of two absorb
            out += [compose(n, 0, 2, "middle"), compose(n, 2, 1, "first"), compose(n, 1, 0, "last")]
        elif bO > 1.0 and bR <= bO:   # arrangement 2: one or two "other" slots of 1024 absorb the run and a long list
            nM = n - 202 if n == 4096 else 300
            out += [_with_others(n, 200, nM, (n // 3, n - 1)), _with_others(n, 2, min(nM, 2000), (0,))]
        elif bO < 1.0:                # instance 1, 1/p < 1/q < 1: no run -> 1 (shared overfull); no list -> 2
            out += [compose(n, 0, 2, "middle"), _with_others(n, 200, 0, (5, n - 2))]
        else:                         # instance 1, 1 < 1/q < 1/p: no list -> 1 (run overfull); no run -> 2
            out += [compose(n, 2, 0, "middle"), _with_others(n, 0, min(n - 2, 2000), (n // 2, n - 1))]
    return out


def _with_others(n, nR, nM, others):
    """a row whose "other" slots are the given few -- the rest return run (after the first "other" slot), shared slots
    and, when those do not fill the row, "other" slots at its end"""
    cls = ["M"] * n
    for i in others:
        cls[i] = "O"
    a = others[0] + 1
    for i in range(a, a + nR):
        assert cls[i] == "M"
        cls[i] = "R"
    extra = cls.count("M") - nM
    i = n - 1
    while extra > 0:
        if cls[i] == "M":
            cls[i] = "O"
            extra -= 1
        i -= 1
    return "".join(cls)


E_SHORT = ["RMO", "ORM", "MOR", "OORRM", "MMOOR", "ROOOOM", "OMRROMOO", "O" * 6 + "M" * 3 + "RR" + "O" * 5,
           compose(63, 2, 14, "middle"), compose(64, 1, 15, "last"), compose(65, 2, 16, "first"),
           compose(64, 0, 3, "middle"), compose(65, 3, 0, "middle"), compose(40, 8, 20, "middle")]


def guard_length(p, q, nR, nM):
    """the smallest n at which dn * isum exceeds the bound, for these counts"""
    lo, hi = nR + nM + 1, 1 << 20
    while lo < hi:
        mid = (lo + hi) // 2
        if guard_product(compose(mid, nR, nM), p, q) > GUARD_BOUND:
            hi = mid
        else:
            lo = mid + 1
    return lo


def family_e_long():
    """(cls below the guard, cls above it, p, q, arrangement): equal but for the number of "other" slots at the end"""
    out = []
    for (p, q), arr, nR, nM in E_GUARD:
        n0 = guard_length(p, q, nR, nM)
        pair = []
        for n in (int(0.9 * n0), int(1.1 * n0)):
            head = compose(400, nR, nM, "middle")  # the same 400 slots, then "other" slots alone
            pair.append(head + "O" * (n - 400))
        assert guard_product(pair[0], p, q) <= GUARD_BOUND < guard_product(pair[1], p, q)
        assert pair[1].startswith(pair[0]) and set(pair[1][len(pair[0]):]) == {"O"}
        for cls in pair:
            assert cell(cls, p, q, tie=False)[0][:2] == (instance(p, q), arr), (p, q, arr, len(cls))
        out.append((pair[0], pair[1], p, q, arr))
    return out


# ------------------------------------------------------------------------------------- graphs and walkers
W_MAX = 1 << 22
EDGE = 2.0 ** -14


def standing(s, W, deg_s, first_v, parallel, seed=SEED):
    """ordinals of the W walkers started on s that stand on v after the first step: N(s) has unit weights, its table is
    all ones, the step is slot (u1 * deg) >> 32, and v fills the slots [first_v, first_v + parallel) of N(s)"""
    keys = np.uint64(s) * np.uint64(W) + np.arange(W, dtype=np.uint64)
    u1, _ = _uniform_bits(seed, keys, 0)
    slot = (u1 * deg_s) >> 32
    return np.nonzero((slot >= first_v) & (slot < first_v + parallel))[0]


def draws(row, W, seed=SEED):
    """(pick, r2) of the second step of every walker of `row` that stands on v"""
    nb = np.sort(np.concatenate([np.full(row["parallel"], row["v"]), row["shared"]]))
    first_v = int(np.searchsorted(nb, row["v"]))
    ords = standing(row["s"], W, nb.size, first_v, row["parallel"], seed)
    u1, u2 = _uniform_bits(seed, np.uint64(row["s"]) * np.uint64(W) + ords.astype(np.uint64), 1)
    return (u1 * row["n"]) >> 32, u2 / 4294967296.0


def must_draw(cls):
    """long rows: every slot of the return run, the first and last shared slot and the "other" slots next to them"""
    n = len(cls)
    need = {i for i, c in enumerate(cls) if c == "R"}
    ms = [i for i, c in enumerate(cls) if c == "M"]
    for i in (ms[:1] + ms[-1:]):
        need.add(i)
        need.update(j for j in (i - 1, i + 1) if 0 <= j < n and cls[j] == "O")
    return sorted(need)


def conditions(row, W, seed=SEED):
    """what the draws of W walkers miss on this row: [] when they reach all they must"""
    pick, r2 = draws(row, W, seed)
    n, cls = row["n"], row["cls"]
    counts = np.bincount(pick, minlength=n)
    miss = []
    if n <= 65:
        if counts.min() < 4:
            miss.append(("picked < 4 times", int(counts.argmin())))
        _, probs = row["table"]
        below = np.bincount(pick[r2 < probs[pick]], minlength=n)
        # every slot with 0 < probs < 1 but those named in row["unbracketable"] (within EDGE of 0 or 1)
        for i in np.nonzero((probs > 0.0) & (probs < 1.0))[0]:
            if int(i) not in row["unbracketable"] and (below[i] == 0 or below[i] == counts[i]):
                miss.append(("one side of probs only", int(i)))
    else:
        miss += [("never drawn", i) for i in must_draw(cls) if counts[i] == 0]
    return miss


def _walkers(row, per_slot):
    W = 256
    while W * row["to_v"] < per_slot * row["n"]:
        W *= 2
    while W < W_MAX and conditions(row, W):
        W *= 2
    return W


_LAYOUTS = {}


def unbracketable(probs):
    """the slots whose probability in the reference's table lies within EDGE = 2^-14 of 0 or 1 without being 0 or 1: no
    feasible number of draws puts one on each side of it.  In families A - D such a value is the fp64 residue of an
    exact 0 or 1 (the host test bounds it by 1e-9); family E has real ones: two class values 2^-20 apart side by side"""
    return {int(i) for i in np.nonzero(((probs > 0.0) & (probs < EDGE)) | ((probs > 1.0 - EDGE) & (probs < 1.0)))[0]}


def layout(family, key=None):
    """the rows of one graph: `_Rows` with, per row, cls / p / q / cell / tie / table (the fp64 restatement) / exact (the
    exact probabilities) / unbracketable / W.
    family "A" and "B": key = (p, q); "B" is two graphs, ("B", pq, "low") holds the rows whose return counts all stay
    below 128 (the inline return position survives), ("B", pq, "high") the others; "C", "D", "E", "Eg": key = (p, q)"""
    k = (family, key)
    if k in _LAYOUTS:
        return _LAYOUTS[k]
    p, q = key[0], key[1]
    cap = 200
    if family == "A":
        cases = family_a()
    elif family == "B":
        cases = [c for c in family_b(p, q) if (c.count("R") < 128) == (key[2] == "low")]
        cap = 127 if key[2] == "low" else 200
    elif family == "C":
        cases = [c for by_tie in family_c().values() for c, cp, cq in by_tie.values() if (cp, cq) == (p, q)]
    elif family == "D":
        cases = family_d(p, q)
    elif family == "E":
        cases = list(E_SHORT)
    elif family == "Eg":
        cases = [c for lo, hi, gp, gq, _ in family_e_long() if (gp, gq) == (p, q) for c in (lo, hi)]
    else:
        raise KeyError(family)
    L = _Rows()
    for i, cls in enumerate(cases):
        n = len(cls)
        rp = cls.index("R") if "R" in cls else None
        ids = [rp if c == "R" else j for j, c in enumerate(cls)]
        L.add(ids, None, [j for j, c in enumerate(cls) if c == "M"], rp,
              dict(info=(family, cls if n <= 70 else (n, cls.count("R"), cls.count("M"), rp), p, q), slots=[],
                   cls=cls, p=p, q=q), s_above=i % 2 == 1, max_parallel=cap)
    for r in L.rows:
        eff = effective(r["cls"], p, q)
        r["table"] = float_tables(eff, p, q)
        tie, _, r["exact"] = exact_loop(eff, p, q)
        r["cell"], r["tie"] = cell(r["cls"], p, q, tie=tie)
        r["unbracketable"] = unbracketable(r["table"][1]) if r["n"] <= 65 else set()
        r["W"] = _walkers(r, 12 if r["n"] <= 65 else (16 if family == "Eg" else 4))
    _LAYOUTS[k] = L
    return L


def all_keys():
    """every (family, key) of the suite"""
    keys = [("A", pq) for inst in (0, 3, 1) for pq in A_PAIRS[inst]]
    keys += [("B", pq + (half,)) for pq in B_PAIRS for half in ("low", "high")]
    keys += [("C", pq) for pq in C_PAIRS]
    keys += [("D", pq) for pq in D_PAIRS]
    keys += [("E", pq) for pq in E_SHORT_PAIRS]
    keys += [("Eg", pq) for pq in sorted({g[0] for g in E_GUARD})]
    return keys
