"""Graphs, contexts, reference law and test statistic of the fast-mode law tests (numpy only).

Fast mode (csrc/n2v_walk_fast.hip) promises the transition law of generate_edge_alias_tables
(reference randomwalk.py:219-231): standing on v after the step (s -> v), slot x of N(v) is drawn with
probability ~ w(v, x) * (1/p if x == s, 1 if x in N(s), 1/q otherwise).  Which instructions turn a uniform
into a slot depends on the tables at hand and on the shape of the row: this module builds, BY CONSTRUCTION,
the smallest multigraphs whose contexts (s, v) reach each of those paths, and says in closed form what every
context looks like (return run, shared list, positions), so that test_fast_law_host.py can prove the claim on
the CSR and test_fast_law_gpu.py can compare the kernel's draws with the law.

A graph is a set of disjoint GADGETS, ids ascending:

    [pad0 pad1]  low leaves  s  high leaves  v

Every leaf has a role: M (neighbour of s and of v: a SHARED slot of the context), A (neighbour of s only),
B (neighbour of v only: an OTHER slot).  s -> v and v -> s are bundles of parallel edges (nR = the v -> s
bundle), a leaf may hang on v by several parallel edges.  Rows are sorted by id, so the return run of N(v)
lies between the slots of the low and of the high leaves, and the position of every slot is known.  The pad
pair in front (pad0 -> pad1 k times) shifts rowptr[s] to a chosen residue modulo 32: the place of N(s) among
the 32-entry blocks of `col` that member_pivoted_lane searches.

The statistic (one function for the host and the GPU test), thresholds as in test_fast_unit_gpu.py:
  * the mass of each class (return, shared, other): within Z_SHARE = 5 binomial sigma;
  * chi-square over all pooled cells (one per neighbour id) of the row, and the chi-square of
    proportionality to w inside each class (uniformity on unit weights), summed over the classes: as the
    normal score z = (chi2 - dof) / sqrt(2 dof) < Z_CHI2 = 4.5.
That score is a normal score only where dof is large: at one degree of freedom z < 4.5 means chi2 < 7.4, which
a CORRECT sampler exceeds in 0.7 % of its runs.  So a context's chi-square is asserted on its own from
MIN_DOF = 30 degrees of freedom on, and always as part of the sum over all contexts run together (the pooling
of test_unit_fast_transition_distribution); the contexts below MIN_DOF have at most three ids, one per class,
where the class masses ARE the law.
"""
import numpy as np

PQ = [(0.5, 2.0), (2.0, 0.5), (0.25, 0.5), (0.5, 0.25), (4.0, 2.0), (2.0, 4.0),  # the six orderings
      (1.0, 2.0), (2.0, 1.0), (3.0, 3.0),  # the ties p = 1, q = 1, p = q
      (3.0, 0.7)]  # not dyadic
NUM_WALKS = 1 << 20  # walkers started at s, per context
Z_SHARE, Z_CHI2, MIN_DOF = 5.0, 4.5, 30
WIDE_FROM = 40  # build_wedges(wide_from=...): rows of this many entries or more read 32-bit lists
RET, SHARED, OTHER = 0, 1, 2


# ------------------------------------------------------------------------------------------ builder
def _leaves(roles, weights=None):
    """[(role, weights of the parallel edges v -> leaf)]; `weights`: {index: [w, ...]}"""
    weights = weights or {}
    return [(r, list(weights.get(i, [1.0]))) for i, r in enumerate(roles)]


class _Builder:
    def __init__(self, name, dtype=None):
        self.name, self.dtype = name, dtype
        self.src, self.dst, self.w = [], [], []
        self.next_id = 0
        self.contexts = {}

    def _edge(self, a, b, w=1.0):
        self.src.append(a)
        self.dst.append(b)
        self.w.append(w)

    def gadget(self, name, purpose, low, high, sv, vs, align=None):
        """sv / vs: weights of the parallel edges s -> v / v -> s"""
        base = self.next_id
        first_leaf = base + (2 if align is not None else 0)
        s = first_leaf + len(low)
        v = s + 1 + len(high)
        self.next_id = v + 1
        edges_before = len(self.src)  # all of them leave smaller ids: rowptr[base]
        out_low = sum((r in "MA") + (r in "MB") for r, _ in low)  # out-edges of the low leaves
        if align is not None:
            k = (align - (edges_before + 1 + out_low)) % 32
            k = k if k > 0 else 32
            for _ in range(k):
                self._edge(base, base + 1)
            self._edge(base + 1, base)
        pos_v, rpos, shared_pos, s_pos_shared, n_s_leaf = 0, None, [], [], 0
        slots = []  # (id, class, weight) of N(v) in row order
        for side, group in ((0, low), (1, high)):
            if side == 1:
                rpos = pos_v
                for w in vs:
                    slots.append((s, RET, w))
                pos_v += len(vs)
            for i, (role, vw) in enumerate(group):
                leaf = (first_leaf if side == 0 else s + 1) + i
                if role in "MA":
                    self._edge(s, leaf)
                    self._edge(leaf, s)
                    if role == "M":
                        s_pos_shared.append(n_s_leaf)
                    n_s_leaf += 1
                if role in "MB":
                    for w in vw:
                        self._edge(v, leaf, w)
                        slots.append((leaf, SHARED if role == "M" else OTHER, w))
                        if role == "M":
                            shared_pos.append(pos_v)
                        pos_v += 1
                    self._edge(leaf, v)
        for w in sv:
            self._edge(s, v, w)
        for w in vs:
            self._edge(v, s, w)
        self.contexts[name] = dict(
            name=name, graph=self.name, purpose=purpose, s=s, v=v, nR=len(vs), shared=len(shared_pos),
            rpos=rpos, deg_v=pos_v, deg_s=n_s_leaf + len(sv), shared_pos=shared_pos,
            s_pos_shared=s_pos_shared, align=align, arrive=float(sum(sv)) / (n_s_leaf + float(sum(sv))),
            slot_ids=np.array([x for x, _, _ in slots], np.int64),
            slot_cls=np.array([c for _, c, _ in slots], np.int64),
            slot_w=np.array([w for _, _, w in slots], np.float64))

    def finish(self):
        src, dst = np.array(self.src, np.int64), np.array(self.dst, np.int64)
        w = np.array(self.w, np.float64)
        unit = bool((w == 1.0).all())
        if not unit and self.dtype == np.float32:
            assert (w.astype(np.float32).astype(np.float64) == w).all()
        return dict(name=self.name, src=src, dst=dst, weight=None if unit else w.astype(self.dtype),
                    n_vertices=self.next_id, contexts=self.contexts)


def csr(graph):
    """DeviceGraph.from_edges restated: stable sort by (src, dst); -> rowptr, col, w (None = unit)"""
    nv = graph["n_vertices"]
    order = np.argsort(graph["src"] * nv + graph["dst"], kind="stable")
    rowptr = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(graph["src"], minlength=nv), out=rowptr[1:])
    w = graph["weight"]
    return rowptr, graph["dst"][order].astype(np.int32), None if w is None else w[order]


# ------------------------------------------------------------------------------------------- graphs
def _main_graph():
    b = _Builder("main")
    b.gadget("short_list", "wedge list of 6 entries inside the slot; return run of 3 by index (slot word 0 / "
             "wedge_off); narrow row on the mixed table (twin of wide_row)",
             _leaves("MBMBAMB"), _leaves("BMABMMBABBBB"), [1.0] * 3, [1.0] * 3)
    # 24 M + 35 B below s, 24 M + 35 B above: return position 59, list of 48, half of it from position 40 on
    b.gadget("long_list", "list of 48 > 14 (pivots) and > 32 entries, hub to hub; on the mixed table the wide_row "
             "context (return position 59 and most shared positions >= 40), on the 32-bit table wide_table",
             _leaves(("MBB" * 12)[:35] + "A" * 6 + "M" * 12 + "B" * 12),
             _leaves("BMMBA" * 12 + "B" * 11), [1.0] * 8, [1.0] * 8)
    b.gadget("no_shared", "no shared slot, return run of 2 at position 30 of 72: the inline return position",
             _leaves("B" * 30 + "A" * 5), _leaves("B" * 40 + "A" * 5), [1.0] * 2, [1.0] * 2)
    for deg, n_ret, hi in ((1, 1, ""), (2, 1, "B"), (2, 2, ""), (3, 1, "MB"), (3, 2, "B")):
        b.gadget("low_degree_%d_%d" % (deg, n_ret), "deg(v) = %d with nR = %d: where the round-2 over-weight "
                 "n / (n - nR) of the return edge is large" % (deg, n_ret),
                 _leaves("A"), _leaves(hi), [1.0], [1.0] * n_ret)
    # N(s): 92 leaves + 8 edges to v = 100 entries from residue 7: blocks [7, 32) [32, 64) [64, 96) [96, 107)
    b.gadget("pivoted", "N(s) of 100 entries that starts and ends inside 32-entry blocks of col; shared "
             "neighbours in its first, a middle and its last block (member_pivoted_lane)",
             _leaves("AMA" + "B" * 20 + "A" * 37), _leaves("A" * 9 + "MM" + "B" * 20 + "A" * 38 + "MAM"),
             [1.0] * 8, [1.0] * 2, align=7)
    return b.finish()


def _saturated_graph():
    b = _Builder("saturated")
    b.gadget("saturated_return", "300 parallel edges each way: the return count saturates at 255, the rho fold "
             "must switch off and the wedge lists are declined",
             _leaves("MBBBA" * 5), _leaves("BMBB" * 5 + "B" * 5), [1.0] * 300, [1.0] * 300)
    return b.finish()


def _weighted_graph(name, dtype):
    scale = 1.0 if dtype == np.float32 else 1.1  # x 1.1: no fp32 values
    pal = [0.5, 1.0, 1.5, 2.0, 3.0]
    b = _Builder(name, dtype)
    lo_roles = "AMA" + "B" * 40 + "A" * 37       # first shared leaf: entry 1 of N(s)
    hi_roles = "A" * 9 + "MM" + "B" * 30 + "M" * 12 + "B" * 12 + "A" * 26 + "MAM"
    for heavy in ("return", "shared", "other"):
        wl = {i: [pal[(3 * i) % 5] * scale] for i in range(len(lo_roles))}
        wh = {i: [pal[(3 * i + 1) % 5] * scale] for i in range(len(hi_roles))}
        wl[5] = [0.5 * scale, 0.0, 2.0 * scale]   # parallel edges of different weights, one of them 0
        wh[9] = [1.5 * scale, 3.0 * scale]        # ... to a shared leaf
        wh[20] = [1.0 * scale, 0.5 * scale, 0.5 * scale]
        vs = [1.5 * scale, 0.5 * scale]
        if heavy == "return":
            vs[0] = 40.0 * scale
        elif heavy == "shared":
            wh[10] = [40.0 * scale]
        else:
            wl[10] = [40.0 * scale]
        b.gadget(name + "_heavy_" + heavy, "weighted rejection sampler (%s weights), row of more than 100 slots, "
                 "parallel edges of different weights, a zero-weight slot, heaviest slot a %s slot; N(s) as in "
                 "pivoted" % (np.dtype(dtype).name, heavy),
                 _leaves(lo_roles, wl), _leaves(hi_roles, wh), [1.0] * 8, vs, align=7)
    return b.finish()


_GRAPHS = {}


def graphs():
    if not _GRAPHS:
        for g in (_main_graph(), _saturated_graph(), _weighted_graph("weighted32", np.float32),
                  _weighted_graph("weighted64", np.float64)):
            _GRAPHS[g["name"]] = g
    return _GRAPHS


def contexts():
    """{name: context}; a context: graph, s, v, purpose and its closed-form structure"""
    return {c["name"]: c for g in graphs().values() for c in g["contexts"].values()}


# ---------------------------------------------------------------------------------------------- law
def slot_law(cls, w, p, q):
    """probability of every slot: w * (1/p | 1 | 1/q), normalised"""
    pr = np.asarray(w, np.float64) * np.array([1.0 / p, 1.0, 1.0 / q])[cls]
    return pr / pr.sum()


def csr_law(rowptr, col, w, s, v, p, q):
    """the law read off a CSR: (neighbour ids, class, probability) per slot of N(v)"""
    nb = col[rowptr[v]:rowptr[v + 1]].astype(np.int64)
    ww = np.ones(nb.size) if w is None else w[rowptr[v]:rowptr[v + 1]].astype(np.float64)
    ns = col[rowptr[s]:rowptr[s + 1]]
    cls = np.where(nb == s, RET, np.where(np.isin(nb, ns), SHARED, OTHER))
    return nb, cls, slot_law(cls, ww, p, q)


def pool(ids, cls, pr):
    """one cell per neighbour id: (ids, class of the id, probability)"""
    u, first, inv = np.unique(ids, return_index=True, return_inverse=True)
    return u, cls[first], np.bincount(inv, weights=pr)


def context_law(ctx, p, q):
    """pooled law and class masses of a context from its construction"""
    ids, cid, pv = pool(ctx["slot_ids"], ctx["slot_cls"], slot_law(ctx["slot_cls"], ctx["slot_w"], p, q))
    return ids, cid, pv, np.bincount(cid, weights=pv, minlength=3)


# ---------------------------------------------------------------------------------------- statistic
def statistic(obs, cid, pv):
    """obs: observed count per pooled cell; cid: class of the cell; pv: its probability"""
    obs, pv = np.asarray(obs, np.float64), np.asarray(pv, np.float64)
    n = obs.sum()
    share = {}
    for c in (RET, SHARED, OTHER):
        pc, oc = pv[cid == c].sum(), obs[cid == c].sum()
        if not (cid == c).any():
            continue
        var = n * pc * (1.0 - pc)
        share[c] = (oc - n * pc) / np.sqrt(var) if var > 1e-9 else (0.0 if oc == round(n * pc) else np.inf)
    exp = n * pv
    row = (float(((obs - exp) ** 2 / exp).sum()), obs.size - 1)
    chi2, dof = 0.0, 0
    for c in (RET, SHARED, OTHER):
        m = cid == c
        if m.sum() < 2 or obs[m].sum() == 0:
            continue
        e = obs[m].sum() * pv[m] / pv[m].sum()
        chi2 += float(((obs[m] - e) ** 2 / e).sum())
        dof += int(m.sum()) - 1
    return dict(n=n, share=share, row=row, within=(chi2, dof), min_exp=float(exp.min()))


def chi_z(chi2, dof):
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def failures(stats):
    """stats: {context name: statistic()} of the contexts run together -> list of violated assertions"""
    bad = []
    for key in ("row", "within"):
        tot, tdof = 0.0, 0
        for name, st in stats.items():
            chi2, dof = st[key]
            tot, tdof = tot + chi2, tdof + dof
            if dof >= MIN_DOF and not chi_z(chi2, dof) < Z_CHI2:
                bad.append((name, key, chi2, dof, chi_z(chi2, dof)))
        if tdof >= MIN_DOF and not chi_z(tot, tdof) < Z_CHI2:
            bad.append(("sum", key, tot, tdof, chi_z(tot, tdof)))
    for name, st in stats.items():
        for c, z in st["share"].items():
            if not abs(z) < Z_SHARE:
                bad.append((name, "share", ("return", "shared", "other")[c], z))
    return bad


def report(stats):
    lines = []
    for name, st in stats.items():
        lines.append("%-22s n=%7d share z %s row %.1f/%d z=%.2f within %.1f/%d z=%.2f" % (
            name, st["n"], " ".join("%+.2f" % z for z in st["share"].values()), st["row"][0], st["row"][1],
            chi_z(st["row"][0], max(st["row"][1], 1)), st["within"][0], st["within"][1],
            chi_z(st["within"][0], max(st["within"][1], 1))))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------ mutants
MUTANTS = {
    "a": "return edge over-weighted by n / (n - nR) (round 2)",
    "b": "shared slots treated as other",
    "c": "layer-2 mass computed with the count of the wrong class",
    "d": "by-index draw clamped one short",
    "e": "long list read through the wrong pivot segment",
    "f": "positions >= T folded but not unfolded",
    "g": "rho folded with a saturated count taken as 255",
}


def _layers(cls, p, q):
    """the layers of kClassFirst on unit weights: [(mass, mask of its set, drawn by index?)] and the total"""
    cls = np.where((cls == SHARED) & (q == 1.0), OTHER, cls)  # q == 1: shared slots ARE other slots
    wc, bc = [1.0 / p, 1.0, 1.0 / q], [RET, SHARED, OTHER]
    for a in range(2):  # the kernel's bubble sort
        for k in range(2 - a):
            if wc[k] > wc[k + 1]:
                wc[k], wc[k + 1] = wc[k + 1], wc[k]
                bc[k], bc[k + 1] = bc[k + 1], bc[k]
    n = cls.size
    sets = [np.ones(n, bool), cls != bc[0], cls == bc[2]]
    mass = [n * wc[0], sets[1].sum() * (wc[1] - wc[0]), sets[2].sum() * (wc[2] - wc[1])]
    return cls, bc, wc, sets, mass


def mutant_law(kind, ctx, p, q, wide_from=None):
    """slot probabilities of a context under mutant `kind`, None where the mutant does not touch it"""
    cls, w = ctx["slot_cls"], ctx["slot_w"]
    n, n_ret = cls.size, int((cls == RET).sum())
    unit = bool((w == 1.0).all())
    bias = np.array([1.0 / p, 1.0, 1.0 / q])
    if kind == "a":
        if n == n_ret or n_ret == 0:
            return None
        pr = w * bias[cls] * np.where(cls == RET, n / (n - n_ret), 1.0)
        return pr / pr.sum()
    if kind == "b":
        if q == 1.0 or not (cls == SHARED).any():
            return None
        pr = w * bias[np.where(cls == SHARED, OTHER, cls)]
        return pr / pr.sum()
    if kind == "g":
        if n_ret <= 255 or not 1.0 / p > max(1.0, 1.0 / q):  # (the fold: inv_p > b_hi)
            return None
        pr = w * bias[cls] * np.where(cls == RET, 255.0 / n_ret, 1.0)
        return pr / pr.sum()
    # the layered sampler: unit weights with wedge lists (a saturated return count declines them)
    if not unit or (p == 1.0 and q == 1.0) or n_ret >= 255:
        return None
    lc, bc, wc, sets, mass = _layers(cls, p, q)
    if kind == "c":
        if sets[1].sum() == 0 or (lc == bc[2]).sum() == (lc == bc[0]).sum():
            return None
        mass = [mass[0], (n - (lc == bc[2]).sum()) * (wc[1] - wc[0]), mass[2]]
    pr = np.zeros(n)
    for layer in range(3):
        m, k = sets[layer], int(sets[layer].sum())
        if k == 0 or mass[layer] == 0.0:
            continue
        per = np.where(m, mass[layer] / k, 0.0)
        if kind in "def" and not (m & (lc == OTHER)).any():  # drawn by index: the return run, then the list
            order = np.r_[np.flatnonzero(m & (lc == RET)), np.flatnonzero(m & (lc == SHARED))]
            lst = np.flatnonzero(m & (lc == SHARED))
            if kind == "d" and k >= 2:
                per[order[-2]] += per[order[-1]]
                per[order[-1]] = 0.0
            if kind == "e" and lst.size > 14:
                idx = [-1] + [((j + 1) * lst.size) // 9 for j in range(8)] + [lst.size - 1]
                seg4, seg3 = lst[idx[4] + 1:idx[5] + 1], lst[idx[3] + 1:idx[4] + 1]
                per[seg3] += per[seg4].sum() / seg3.size
                per[seg4] = 0.0
            if kind == "f" and wide_from and n >= wide_from:
                for pos in order[order >= wide_from]:
                    per[pos - wide_from] += per[pos]
                    per[pos] = 0.0
        pr += per
    pr /= pr.sum()
    return None if np.allclose(pr, slot_law(cls, w, p, q), rtol=0, atol=1e-15) else pr


def expected_z(ctx, p, q, pr_mut, n):
    """what the statistic is expected to show on n arrivals drawn from pr_mut: the largest of the class-mass
    shifts over sigma and of the chi-squares' noncentrality lambda as z = lambda / sqrt(2 dof) (a chi-square
    below MIN_DOF is not asserted per context and counts for nothing here)"""
    ids, cid, pv, _ = context_law(ctx, p, q)
    _, _, pm = pool(ctx["slot_ids"], ctx["slot_cls"], pr_mut)
    best = {}
    for c in (RET, SHARED, OTHER):
        pc, qc = pv[cid == c].sum(), pm[cid == c].sum()
        if 0.0 < pc < 1.0:
            best["share"] = max(best.get("share", 0.0), abs(qc - pc) * n / np.sqrt(n * pc * (1 - pc)))
    if ids.size - 1 >= MIN_DOF:
        best["row"] = n * float(((pm - pv) ** 2 / pv).sum()) / np.sqrt(2.0 * (ids.size - 1))
    lam, dof = 0.0, 0
    for c in (RET, SHARED, OTHER):
        m = cid == c
        if m.sum() >= 2 and pm[m].sum() > 0:
            a, b_ = pm[m] / pm[m].sum(), pv[m] / pv[m].sum()
            lam += n * pm[m].sum() * float(((a - b_) ** 2 / b_).sum())
            dof += int(m.sum()) - 1
    if dof >= MIN_DOF:
        best["within"] = lam / np.sqrt(2.0 * dof)
    return best
