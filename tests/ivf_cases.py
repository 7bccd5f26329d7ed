"""Shared by tests/test_ivf_host.py and tests/test_ivf_gpu.py: what node2vec_amd.ann.search must return, restated in
numpy around the nearest-neighbour oracle (oracle/n2v_oracle_knn.c gives every score in the kernels' summation
order), and the case tables.

The restatement is the contract of csrc/n2v_ivf.hip word for word: a query's candidates are the rows of the lists it
probes; a NaN score is dropped; the rest is sorted by (score descending, original row ascending); the tail is
(-1, -inf).  Nothing in it knows about tiles, chunks or groups."""
import numpy as np

# the lengths of the hand-made lists 0 .. 7; list 8 is the long one, sized on the launch plan
SMALL_LISTS = (0, 1, 15, 16, 17, 63, 64, 65)
LONG_LIST = len(SMALL_LISTS)
NLIST = LONG_LIST + 1
# max_list_rows the hand-made indexes are searched with: three chunks by the plan's rule (asserted where used)
HAND_MAX_LIST_ROWS = 5376

# dim, k, long list's length in terms of the plan's chunk_rows c, n_queries, aligned base.  200 queries of one
# probe are more than 16 per list on average (the 64-wide tile), 100 are not (the 16-wide one)
HAND_CASES = [
    (64, 10, "c-1", 200, True), (128, 1, "c", 200, True), (129, 128, "c+1", 200, True), (3, 127, "2c+1", 200, True),
    (16, 10, "2c+1", 100, True), (17, 128, "c+1", 100, True), (64, 10, "c", 200, False),
    (128, 127, "c-1", 100, False),
]


def long_rows(kind, chunk_rows):
    return {"c-1": chunk_rows - 1, "c": chunk_rows, "c+1": chunk_rows + 1, "2c+1": 2 * chunk_rows + 1}[kind]


def lists_of(labels_or_lists, nlist):
    """nlist int64 row arrays, ascending: from labels [n] (a label outside [0, nlist) is in no list) or as given"""
    if isinstance(labels_or_lists, np.ndarray) and labels_or_lists.ndim == 1:
        return [np.nonzero(labels_or_lists == l)[0].astype(np.int64) for l in range(nlist)]
    assert len(labels_or_lists) >= nlist
    return [np.sort(np.asarray(rows, np.int64)) for rows in labels_or_lists]


def expect(oracle, X, labels_or_lists, probes, k, queries=None, rows=None, exclude=None):
    """(rows int64 [nq, k], scores fp32 [nq, k]) of ann.search.  labels_or_lists: one integer label per row, or a
    list of row arrays; probes: [nq, nprobe] list numbers, -1 unused; exclude: [nq] a row left out of each query's
    candidates."""
    probes = np.asarray(probes, np.int64)
    lists = lists_of(labels_or_lists, int(probes.max()) + 1)
    scores = oracle.knn_scores(X, queries=queries, rows=rows)
    nq = scores.shape[0]
    assert probes.shape[0] == nq
    out_r = np.full((nq, k), -1, np.int64)
    out_s = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        probed = [lists[l] for l in probes[q] if l >= 0]
        cand = np.concatenate(probed) if probed else np.zeros(0, np.int64)
        assert len(np.unique(cand)) == len(cand), "a row in two probed lists"
        if exclude is not None:
            cand = cand[cand != exclude[q]]
        s = scores[q, cand]
        cand, s = cand[~np.isnan(s)], s[~np.isnan(s)]
        order = np.lexsort((cand, -s))[:k]  # score descending, then row ascending (-0.0 == 0.0, as in the kernel)
        out_r[q, :len(order)] = cand[order]
        out_s[q, :len(order)] = s[order]
    return out_r, out_s


def bits(s):
    return np.ascontiguousarray(s, np.float32).view(np.int32)


def same(got, want, what=""):
    (gr, gs), (wr, ws) = got, want
    gr, gs = np.asarray(gr), np.asarray(gs)
    assert gr.shape == wr.shape, what
    bad = np.nonzero((gr != wr).any(axis=1) | (bits(gs) != bits(ws)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} queries differ, first {bad[0]}: rows {gr[bad[0]][:8]} want " \
                          f"{wr[bad[0]][:8]}, scores {gs[bad[0]][:8].tolist()} want {ws[bad[0]][:8].tolist()}"


def mixed_rows(rng, n, dim):
    """Gaussian rows; ~5 % copies of three hub rows spread over the whole matrix (ties), ~1 % zero rows"""
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n >= 20:
        hubs = X[:3].copy()
        for i, r in enumerate(rng.choice(n, n // 20, replace=False)):
            X[r] = hubs[i % 3]
        X[rng.choice(n, max(1, n // 100), replace=False)] = 0.0
    return X


def hand_labels(rng, long_len, n=5700):
    """seeded random labels of n rows (n >= HAND_MAX_LIST_ROWS, as n2v_ivf_topk wants of max_list_rows): list l < 8
    has SMALL_LISTS[l] rows, list 8 long_len rows, the others are in no list (label -1)"""
    lens = list(SMALL_LISTS) + [long_len]
    spare = n - sum(lens)
    assert spare >= 0
    labels = np.concatenate([np.full(m, l, np.int64) for l, m in enumerate(lens)] + [np.full(spare, -1, np.int64)])
    return labels[rng.permutation(len(labels))]


def probe_sets(rng, nq, qt):
    """name -> probes [nq, nprobe] over the hand-made lists: random distinct lists padded with -1; every query on the
    long list; groups of 1, qt - 1, qt and qt + 1 queries on the long list (the others share list 5)"""
    out = {}
    nprobe = 4
    rand = np.full((nq, nprobe), -1, np.int64)
    for q in range(nq):
        m = int(rng.integers(0, nprobe + 1))
        rand[q, :m] = rng.choice(NLIST, m, replace=False)
    out["random"] = rand
    out["all on the long list"] = np.full((nq, 1), LONG_LIST, np.int64)
    for g in (1, qt - 1, qt, qt + 1):
        p = np.full((nq, 1), 5, np.int64)
        p[rng.choice(nq, g, replace=False)] = LONG_LIST
        out[f"group of {g}"] = p
    return out
