"""Graphs whose return counts sit on both sides of the two limits of the class word's 8-bit return field (numpy only).

edge_classes[e] of the edge (s -> v) holds the number of slots of N(v) that lead back to s in 8 bits
(n2v_edge_classes_build).  Two values of that count switch code paths:

  127 | 128   the inline hop-table form (N2V_EC_INLINE) has 7 bits for it: DeviceGraph.can_inline_rpos() declines
              the form for the whole graph from 128 on;
  254 | 255   255 stands for "255 or more" (N2V_EC_RETURN_SAT): DeviceGraph.build_wedges() declines the lists for
              the whole graph, and every exact kernel takes its "a count that did not fit" branch.

A graph is a row of disjoint GADGETS of 47 vertices, one per multiplicity m, ids ascending:

    15 low leaves   s   10 middle leaves   v   20 high leaves

s and v are joined by m parallel edges EACH WAY.  A leaf has a role: M (neighbour of s and of v: a shared slot of
the context (s, v)), A (neighbour of s only), B (neighbour of v only: an "other" slot); 3 M, 2 A and 40 B in all, one
B leaf hanging on v by 5 parallel edges.  Every leaf edge runs both ways (leaf -> v once), so no walker vanishes.
Rows are sorted by id: the return run of N(v) -- and the run of v in N(s) -- lies between the slots of the low and
of the later leaves.

test_return_count_cases_host.py proves on the CPU that the graphs are what they claim and that the oracle's walks
draw from every gadget's table often enough; test_return_count_limits_gpu.py walks them in exact mode on every
dispatch of randomwalk.walk and compares bit for bit.
"""
import numpy as np

PQ = [(0.5, 2.0), (4.0, 0.25), (4.0, 2.0), (3.0, 0.7), (0.7, 3.0), (2.0, 1.0), (1.0, 2.0)]
NUM_WALKS, WALK_LENGTH, SEED = 8, 12, 20241019
RETURN_SAT, INLINE_LIMIT = 255, 128

MULTS = {
    "below": (126, 127),
    "inline_limit": (126, 127, 128, 129),
    "saturated": (126, 127, 128, 129, 254, 255, 256, 300),
}
LOW, MID, HIGH = "BBBMBBBBABBBBBB", "BMBBBBBBBB", "BBBBBABBBMBBBBBBBBBB"
FIVE_FOLD = 5   # the low leaf (a B leaf) that hangs on v by 5 parallel edges
PAL = (0.5, 1.0, 1.5, 2.0, 3.0)  # weights of the parallel edges of a bundle, in turn: 1.5 and 3.0 are no powers of two

# the gadget orders of the partitioned walks: partition_graph(g, n) cuts where the running number of edges passes
# k * E / n, and with these orders one cut falls between s and v of the 300-fold gadget (part_cuts, host test)
PART_ORDERS = {2: (126, 127, 128, 254, 300, 129, 255, 256), 3: (126, 127, 128, 300, 129, 254, 255, 256)}

# the hub instance (class words on the wave path of edge_classes_kernel): m, extra M leaves, extra A leaves.  30 more
# shared leaves make both rows long; 80 more leaves on s alone make N(s) the longer row (it is the shorter otherwise)
HUBS = ((300, 30, 0), (300, 30, 80), (254, 30, 0), (255, 30, 80))
LANE_MAX = 24  # kLaneMax of n2v_edge_classes.hip: a shorter list above it goes to the whole wave


class _Builder:
    def __init__(self, name, dtype=None):
        self.name, self.dtype = name, dtype
        self.scale = 1.1 if dtype == np.float64 else 1.0  # x 1.1: no fp32 values
        self.src, self.dst, self.w = [], [], []
        self.next_id = 0
        self.gadgets = []

    def _edge(self, a, b, w=1.0):
        self.src.append(a)
        self.dst.append(b)
        self.w.append(w * self.scale if self.dtype is not None else 1.0)

    def gadget(self, m, extra_m=0, extra_a=0):
        base = self.next_id
        s = base + len(LOW)
        v = s + 1 + len(MID)
        high = HIGH + "M" * extra_m + "A" * extra_a
        self.next_id = v + 1 + len(high)
        roles = ([(base + i, r) for i, r in enumerate(LOW)] + [(s + 1 + i, r) for i, r in enumerate(MID)]
                 + [(v + 1 + i, r) for i, r in enumerate(high)])
        for leaf, role in roles:
            if role in "MA":
                self._edge(s, leaf)
                self._edge(leaf, s)
            if role in "MB":
                if leaf == base + FIVE_FOLD:
                    for w in PAL:
                        self._edge(v, leaf, w)
                else:
                    self._edge(v, leaf, PAL[leaf % 5])
                self._edge(leaf, v)
        for i in range(m):
            self._edge(s, v, PAL[i % 5])
            self._edge(v, s, PAL[(i + 2) % 5])
        assert LOW[FIVE_FOLD] == "B"
        self.gadgets.append(dict(
            m=m, s=s, v=v, base=base, end=self.next_id,
            shared=np.array([x for x, r in roles if r == "M"], np.int64),
            s_only=np.array([x for x, r in roles if r == "A"], np.int64),
            v_only=np.array([x for x, r in roles if r == "B"], np.int64),
            five_fold=base + FIVE_FOLD))

    def finish(self):
        w = None if self.dtype is None else np.array(self.w, np.float64).astype(self.dtype)
        return dict(name=self.name, src=np.array(self.src, np.int64), dst=np.array(self.dst, np.int64), weight=w,
                    n_vertices=self.next_id, gadgets=self.gadgets)


def _build(name, mults, dtype=None):
    b = _Builder(name, dtype)
    for m in mults:
        b.gadget(m)
    return b.finish()


def _hubs():
    b = _Builder("hubs")
    for m, extra_m, extra_a in HUBS:
        b.gadget(m, extra_m, extra_a)
    return b.finish()


_GRAPHS = {}


def graphs():
    """{name: graph}: below, inline_limit, saturated (unit weights), the weighted twins of saturated, the hub instance
    and saturated in the two gadget orders of the partitioned walks"""
    if not _GRAPHS:
        for name, mults in MULTS.items():
            _GRAPHS[name] = _build(name, mults)
        _GRAPHS["saturated_w32"] = _build("saturated_w32", MULTS["saturated"], np.float32)
        _GRAPHS["saturated_w64"] = _build("saturated_w64", MULTS["saturated"], np.float64)
        _GRAPHS["hubs"] = _hubs()
        for n, order in PART_ORDERS.items():
            _GRAPHS["saturated_parts%d" % n] = _build("saturated_parts%d" % n, order)
    return _GRAPHS


UNIT = ("below", "inline_limit", "saturated")
WEIGHTED = ("saturated_w32", "saturated_w64")
_CSR = {}


def csr(name):
    """DeviceGraph.from_edges restated: stable sort by (src, dst); -> rowptr, col, w (None = unit)"""
    if name not in _CSR:
        g = graphs()[name]
        nv = g["n_vertices"]
        order = np.argsort(g["src"] * nv + g["dst"], kind="stable")
        rowptr = np.zeros(nv + 1, np.int64)
        np.cumsum(np.bincount(g["src"], minlength=nv), out=rowptr[1:])
        w = g["weight"]
        _CSR[name] = (rowptr, g["dst"][order].astype(np.int32), None if w is None else w[order])
    return _CSR[name]


# ------------------------------------------------------------------------------------ expected tables
_COUNTS = {}


def edge_counts(name):
    """plain Python, per edge (a -> b) in CSR order: (number of slots of N(b) equal to a, number of slots of N(b)
    that are not a and lie in N(a)) -- the set arithmetic of generate_edge_alias_tables (randomwalk.py:223-230)"""
    if name not in _COUNTS:
        rowptr, col, _ = csr(name)
        rows = [col[rowptr[x]:rowptr[x + 1]].tolist() for x in range(len(rowptr) - 1)]
        sets = [set(r) for r in rows]
        n_ret, n_shared = [], []
        for a, row in enumerate(rows):
            memo = {}
            for b in row:
                if b not in memo:
                    memo[b] = (sum(1 for x in rows[b] if x == a),
                               sum(1 for x in rows[b] if x != a and x in sets[a]))
                n_ret.append(memo[b][0])
                n_shared.append(memo[b][1])
        _COUNTS[name] = (np.array(n_ret, np.int64), np.array(n_shared, np.int64))
    return _COUNTS[name]


def class_words(name):
    """edge_classes as n2v_edge_classes_build must write them: min(return count, 255) << 24 | shared count"""
    n_ret, n_shared = edge_counts(name)
    assert int(n_shared.max()) < 0xffffff
    return (np.minimum(n_ret, RETURN_SAT).astype(np.uint32) << np.uint32(24)) | n_shared.astype(np.uint32)


def edge_index(name, a, b):
    """the first edge a -> b in CSR order"""
    rowptr, col, _ = csr(name)
    row = col[rowptr[a]:rowptr[a + 1]]
    return int(rowptr[a]) + int(np.flatnonzero(row == b)[0])


def part_cuts(name, n_parts):
    """partition_graph(balance="edges") restated: the first vertices of parts 1 .. n_parts - 1"""
    rowptr, col, _ = csr(name)
    targets = np.arange(1, n_parts, dtype=np.int64) * col.size // n_parts
    return np.searchsorted(rowptr, targets, side="left").tolist()


# -------------------------------------------------------------------------------------- the reference
_WALKS = {}


def oracle_walks(oracle, name, pq):
    """the oracle's walks of the GPU test's parameters: every vertex x NUM_WALKS x WALK_LENGTH; computed once"""
    if (name, pq) not in _WALKS:
        rowptr, col, w = csr(name)
        start = np.arange(len(rowptr) - 1, dtype=np.int32)
        walks, valid = oracle.random_walk(rowptr, col, w, start, NUM_WALKS, WALK_LENGTH, pq[0], pq[1], SEED)
        walks.setflags(write=False)
        valid.setflags(write=False)
        _WALKS[(name, pq)] = (walks, valid)
    return _WALKS[(name, pq)]


def context_steps(walks, gadget):
    """steps taken from v with previous vertex s: (all of them, those back to s, those to a leaf of v alone)"""
    w = walks
    at = (w[:, :-2] == gadget["s"]) & (w[:, 1:-1] == gadget["v"])
    nxt = w[:, 2:][at]
    return int(nxt.size), int((nxt == gadget["s"]).sum()), int(np.isin(nxt, gadget["v_only"]).sum())
