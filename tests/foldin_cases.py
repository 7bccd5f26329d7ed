"""The case list of the fold-in tests (test_foldin_host.py, test_foldin_gpu.py): small frozen models and walks over
known words and new vertices, made with seeded numpy -- the smallest shapes that still reach every path of
csrc/n2v_foldin.hip (DESIGN.md "Fold-in").  A case is a dict of numpy arrays and scalars; nothing here needs a GPU."""
import ctypes as C

import numpy as np

import cpu_build

M64 = (1 << 64) - 1
SIGMOID_LAST = 995  # (int)((f + 6) * 83) for the largest f below 6: 12 * 83 = 996, so entries 996 .. 999 are never read

# name, n_vocab, n_new, rows, len, dim, K, window, cum_index, sample, row_alpha, extras
SHAPES = [
    ("one_vertex_dim1", 50, 1, 12, 5, 1, 1, 1, False, 0.0, False, ()),
    ("many_vertices_dim64", 3000, 300, 160, 81, 64, 5, 5, True, 1e-3, False, ()),
    ("ragged_dim100_two_passes", 200, 21, 30, 130, 100, 6, 5, False, 1e-2, False, ("never", "ends")),
    ("dim128_window32_row_alpha", 300, 24, 24, 81, 128, 5, 32, True, 0.0, True, ("ends",)),
    ("ragged_wide_dim200_k32", 120, 10, 12, 81, 200, 32, 5, True, 1e-2, False, ()),
    ("dim256_window1_two_passes", 150, 12, 16, 130, 256, 5, 1, False, 0.0, True, ()),
    ("dim1024_k6", 80, 6, 6, 81, 1024, 6, 5, True, 1e-2, False, ()),
    ("hot_vertex_many_batches", 60, 3, 4, 130, 64, 5, 5, False, 0.0, False, ("hot",)),
    ("two_word_vocabulary", 2, 4, 10, 21, 16, 5, 5, False, 0.0, False, ()),
]
NAMES = [s[0] for s in SHAPES] + ["sigmoid_cut"]


def _tables(counts, sample):
    import torch

    from node2vec_amd import sgns

    c = torch.from_numpy(counts)
    cum = sgns.make_cum_table(c).numpy().view(np.uint32).copy()
    si = sgns.make_sample_int(c, sample)
    return cum, None if si is None else si.numpy().view(np.uint32).copy()


def make(name):
    """the case `name`: walks int32 [rows, len], syn0 / syn1neg fp32 [n_vocab, dim], init fp32 [n_new, dim],
    cum_table / sample_int uint32, row_alpha fp32 [rows] or None, and the scalars"""
    if name == "sigmoid_cut":
        return _sigmoid_cut()
    _, n_vocab, n_new, rows, ln, dim, K, window, cum_index, sample, row_alpha, extras = SHAPES[NAMES.index(name)]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    counts = np.sort(rng.zipf(1.3, n_vocab).clip(max=10 ** 6).astype(np.int64) + 3)[::-1].copy()
    cum, si = _tables(counts, sample)
    occurring = n_new - 1 if "never" in extras else n_new  # "never": the last new vertex is in no walk
    pk = counts / counts.sum()
    kind = rng.random((rows, ln))
    walks = rng.choice(n_vocab, size=(rows, ln), p=pk).astype(np.int64)
    new = n_vocab + rng.integers(0, max(occurring, 1), size=(rows, ln))
    walks = np.where(kind < 0.18, new, walks)
    walks = np.where((kind >= 0.18) & (kind < 0.21), -1, walks)                 # dropped: negative
    walks = np.where((kind >= 0.21) & (kind < 0.23), n_vocab + n_new + 3, walks)  # dropped: past the new vertices
    if "ends" in extras:  # a new vertex at both ends of a sentence
        walks[::2, 0] = n_vocab
        walks[::2, -1] = n_vocab + occurring - 1
    if "hot" in extras:  # one new vertex at every other position of a walk: far more than 64 / K pairs in a row
        walks[1, ::2] = n_vocab + 1
    sigma = np.sqrt(2.5) / dim ** 0.25  # f = row . syn1neg has a deviation of ~2.5: the cut at |f| >= 6 is reached
    return {
        "name": name, "n_vocab": n_vocab, "n_new": n_new, "dim": dim, "negative": K, "window": window,
        "walks": walks.astype(np.int32), "cum_table": cum, "sample_int": si, "cum_index": cum_index,
        "syn0": (rng.standard_normal((n_vocab, dim)) * sigma).astype(np.float32),
        "syn1neg": (rng.standard_normal((n_vocab, dim)) * sigma).astype(np.float32),
        "init": (rng.standard_normal((n_new, dim)) * sigma).astype(np.float32),
        "row_alpha": (0.01 + 0.04 * rng.random(rows)).astype(np.float32) if row_alpha else None,
        "alpha": 0.025, "seed": 77 + NAMES.index(name), "sentence_base": 5 * NAMES.index(name),
        "never": n_new - 1 if "never" in extras else None,
    }


def _sigmoid_cut():
    """dim 1, every new row 1.0: the label-1 target of a vertex's first pair has f = syn1neg[centre] exactly --
    just inside the cut on either side (table entries 0 and SIGMOID_LAST), on it and beyond it"""
    s1 = np.array([[-5.995], [5.995], [6.0], [-6.0], [7.5], [-5.9], [5.9], [0.25]], np.float32)
    n_vocab, n_new = s1.shape[0], 8
    walks = np.full((n_new, 5), -1, np.int32)
    walks[:, 0] = np.arange(n_new) % n_vocab  # the centre ...
    walks[:, 1] = n_vocab + np.arange(n_new)  # ... and the new vertex after it
    cum, _ = _tables(np.arange(n_vocab, 0, -1, dtype=np.int64) * 5, 0.0)
    return {"name": "sigmoid_cut", "n_vocab": n_vocab, "n_new": n_new, "dim": 1, "negative": 5, "window": 1,
            "walks": walks, "cum_table": cum, "sample_int": None, "cum_index": False,
            "syn0": np.zeros((n_vocab, 1), np.float32), "syn1neg": s1, "init": np.ones((n_new, 1), np.float32),
            "row_alpha": None, "alpha": 0.05, "seed": 3, "sentence_base": 0, "never": None}


# ---- the CPU restatement tests/cpu_foldin/n2v_foldin_cpu.c ----
def build_cpu(out_dir):
    L = cpu_build.build("cpu_foldin/n2v_foldin_cpu.c", out_dir)
    L.n2v_foldin_cpu_pass.restype = C.c_int64
    L.n2v_foldin_cpu_pass.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def cpu_pass(L, case, new_rows=None, records=False, stats=None, alpha=None, sentence_base=None, walks=None,
             n_new=None, row_alpha="case"):
    """one pass of the restatement over a case: new_rows (fp32, updated in place) or None for the listing alone;
    returns (pairs, records int32 [pairs, 4] in (row, i, j) order or None)"""
    from node2vec_amd import sgns

    w = np.ascontiguousarray(case["walks"] if walks is None else walks, np.int32)
    exp = sgns.exp_table()  # held in a name: the address of a temporary would dangle during the call
    ra = case["row_alpha"] if isinstance(row_alpha, str) else row_alpha
    si = case["sample_int"]
    n_new = case["n_new"] if n_new is None else n_new
    if new_rows is not None:
        assert new_rows.dtype == np.float32 and new_rows.flags.c_contiguous and new_rows.shape == (n_new, case["dim"])

    def run(rows_ptr, rec_ptr, st):
        return L.n2v_foldin_cpu_pass(w.ctypes.data, w.shape[0], w.shape[1], case["n_vocab"], n_new, rows_ptr,
                                     case["syn1neg"].ctypes.data, case["cum_table"].ctypes.data,
                                     None if si is None else si.ctypes.data, exp.ctypes.data,
                                     case["sentence_base"] if sentence_base is None else sentence_base, case["seed"],
                                     case["dim"], case["window"], case["negative"],
                                     float(case["alpha"] if alpha is None else alpha),
                                     None if ra is None else ra.ctypes.data, rec_ptr, st)

    rec = None
    if records:
        n = run(None, None, None)
        assert n >= 0
        rec = np.zeros((n, 4), np.int32)
        assert run(None, rec.ctypes.data, None) == n
    n = run(None if new_rows is None else new_rows.ctypes.data, None, None if stats is None else stats.ctypes.data)
    return n, rec


def group_by_vertex(records, n_new):
    """records in (row, i, j) order -> grouped by new vertex with a stable sort, and the CSR offsets"""
    order = np.argsort(records[:, 0], kind="stable")
    off = np.zeros(n_new + 1, np.int64)
    np.cumsum(np.bincount(records[:, 0], minlength=n_new), out=off[1:])
    return records[order], off
