"""One deliberately built row per gadget, embedded in a graph and walked two steps: shared by the tests that pin the
exact biased step row by row (test_margin_adversary_gpu.py, test_closed_form_rows_gpu.py).

Each row becomes three kinds of vertices: v, whose out-edges are the row (slot i -> vertex base + i; the return run
-> the vertex s, parallel edges); s, with edges to v (parallel ones: half of its walkers go there first)
and to the shared slots' vertices; sinks.  A walk of two steps from s stands on v with prev = s: its second step is a
draw from the table generate_edge_alias_tables builds for (s, N(s), N(v)) (randomwalk.py:193-232).  That table comes
from the oracle once per row; every walker's uniforms from the RNG restated below (pinned by rng_kat.json through
oracle.uniform_bits): the expected vertex of every walker in O(1).

A row WITHOUT a return run (rpos=None) has an s that is no neighbour of v: a vertex of its own, its id below the row's
id block or above it (s_above)."""
import numpy as np

M64 = (1 << 64) - 1


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _uniform_bits(seed, keys, step):
    """(u1, u2) of every walker key at `step`, numpy uint64 wrap-around arithmetic"""
    with np.errstate(over="ignore"):
        keys = keys.astype(np.uint64)
        h0 = _mix64(np.uint64(seed) ^ _mix64(keys + np.uint64(0x9E3779B97F4A7C15)))
        bits = _mix64(h0 + np.uint64(step + 1) * np.uint64(0xD1B54A32D192ED03))
    return (bits >> np.uint64(32)).astype(np.int64), (bits & np.uint64(0xFFFFFFFF)).astype(np.int64)


class _Rows:
    """adversarial rows laid out in one graph"""

    def __init__(self):
        self.src, self.dst, self.w, self.rows, self.base = [], [], [], [], 0

    def add(self, ids_in_row, weights, shared, rpos, info, s_above=False, max_parallel=200):
        """ids_in_row: slot -> offset inside the row's id block (return slots all = rpos); weights: per slot or None.
        rpos=None: no return run -- s is a vertex of its own, below the row's id block or (s_above) above v"""
        n = len(ids_in_row)
        base = self.base
        if rpos is None:
            if s_above:
                v, s = base + n, base + n + 1
            else:
                s, base = base, base + 1
                v = base + n
        else:
            v, s = base + n, base + rpos
        ids = base + np.asarray(ids_in_row, dtype=np.int64)
        self.src.append(np.full(n, v))
        self.dst.append(ids)
        self.w.append(np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64))
        sh = base + np.asarray(shared, dtype=np.int64)
        # as many parallel edges s -> v as s has other edges: half of the walkers go to v first.  (Parallel edges, not a
        # heavy one: the largest weight of the GRAPH enters the kernel's test for an exact row sum.)
        # (at most 200: the class word of the edge v -> s counts them in 8 bits, and 255 means "no lists")
        m = min(max(1, len(shared)), max_parallel)
        self.src.append(np.full(m + len(sh), s))
        self.dst.append(np.concatenate([np.full(m, v), sh]))
        self.w.append(np.ones(m + len(sh)))
        self.rows.append(dict(info, v=v, s=s, ids=ids.astype(np.int32), n=n, shared=sh, to_v=m / (m + len(sh)),
                              parallel=m))
        self.base = max(v, s) + 1

    def graph(self, weighted):
        from node2vec_amd.graph import DeviceGraph

        src, dst = np.concatenate(self.src), np.concatenate(self.dst)
        w = np.concatenate(self.w) if weighted else None
        return DeviceGraph.from_edges(src, dst, w, n_vertices=self.base, device="cuda")


def _check_rows(oracle, g, rows, W, p, q, seed, walk_kwargs, tables=None):
    """two steps from every s of `rows` (all with this p, q); every walker that stands on v after the first: its
    second vertex against the oracle's table.  Returns (walkers checked, hits on the placed slots).
    `tables`: {s of a row: (alias, probs)}, the oracle's table of that row for this (p, q) -- built here and stored
    there when the row's is missing, so that a second dispatch over the same rows builds none"""
    import torch
    from node2vec_amd import randomwalk as rw

    start = torch.tensor(sorted(r["s"] for r in rows), dtype=torch.int32, device="cuda")
    walks, valid = rw.walk(g, start, W, 2, p, q, seed, mode="exact", **walk_kwargs)
    walks = walks.cpu().numpy().reshape(len(rows), W, 3)
    valid = valid.cpu().numpy().reshape(len(rows), W)
    checked = hits = 0
    rowptr, col, wts = g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.w.cpu().numpy()
    for k, r in enumerate(sorted(rows, key=lambda r: r["s"])):
        s, v, n = r["s"], r["v"], r["n"]
        lo, hi = rowptr[v], rowptr[v + 1]
        assert hi - lo == n and np.array_equal(col[lo:hi], r["ids"])
        if tables is not None and s in tables:
            alias, probs = tables[s]
        else:
            nbs = col[rowptr[s]:rowptr[s + 1]]
            alias, probs = oracle.edge_alias_tables(s, nbs.tolist(), col[lo:hi], wts[lo:hi].astype(np.float64), p, q)
            alias, probs = np.asarray(alias), np.asarray(probs)
            if tables is not None:
                tables[s] = (alias, probs)
        at_v = walks[k, :, 1] == v
        assert at_v.sum() > 0.5 * W * r["to_v"]  # (the share of the edges of s that lead to v)
        ords = np.nonzero(at_v)[0]
        u1, u2 = _uniform_bits(seed, np.uint64(s) * np.uint64(W) + ords.astype(np.uint64), 1)
        pick = (u1 * n) >> 32
        r2 = u2 / 4294967296.0
        want = r["ids"][np.where(r2 < probs[pick], pick, alias[pick])]
        got = walks[k, ords, 2]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (r["info"], "walker", int(ords[bad[0]]), "pick", int(pick[bad[0]]), "r2", float(r2[bad[0]]),
                               "got", int(got[bad[0]]), "want", int(want[bad[0]]))
        assert valid[k, ords].all() or True  # (the second vertex may be a sink: the walk then ends, fugue.py:147)
        checked += ords.size
        hits += int(np.isin(pick, np.asarray(r["slots"])).sum())
    return checked, hits
