"""The cases of the hub-form tests, and the hub restatements' bindings.

A case is everything a launch needs, built on the CPU: the corpus (those of the existing bit tests:
test_sgns_gpu._setup, test_sgns_batched_gpu._corpus), the vocabulary, the cumulative table, the
subsampling thresholds and the initial matrices.  tests/test_hub_form_host.py proves on the CPU that the
cases are what they claim; tests/test_hub_form_gpu.py copies the same arrays into a model on the GPU and
asks the kernels for the restatement's bits.  (A model seeded on the GPU draws other initial values than
one seeded on the CPU, so the case's own syn0 is copied in.)

Not a test module: helpers shared by the two.
"""
import ctypes as C

import numpy as np
import torch

import cpu_build

MUT_CENTRE_TWICE, MUT_NEG_FMA, MUT_BOUNDARY, MUT_LAST_LANE = 1, 2, 3, 4
ALL = -1  # hub_rows: every row (n_vocab, known once the vocabulary is built)


def load_hub(out_dir, checked=False):
    """tests/cpu_sgns_hub/n2v_sgns_hub_cpu.c; checked: with the subnormal-operand counter"""
    L = cpu_build.build("cpu_sgns_hub/n2v_sgns_hub_cpu.c", out_dir, ("N2V_HUB_CHECK",) if checked else ())
    head = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
            C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_float]
    L.n2v_sgns_hub_cpu_train.restype = C.c_int64
    L.n2v_sgns_hub_cpu_train.argtypes = head + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.n2v_sgns_hub_cpu_train_batched.restype = C.c_int64
    L.n2v_sgns_hub_cpu_train_batched.argtypes = head + [C.c_int32, C.c_int32, C.c_int32]
    L.n2v_sgns_hub_cpu_subnormals.restype = C.c_int64
    return L


def load_cbow_checked(out_dir):
    """tests/cpu_cbow/n2v_cbow_cpu.c with the subnormal-operand counter"""
    from test_cbow_host import cbow_argtypes

    L = cpu_build.build("cpu_cbow/n2v_cbow_cpu.c", out_dir, ("N2V_HUB_CHECK",))
    L.n2v_cbow_cpu_train.restype = C.c_int64
    L.n2v_cbow_cpu_train.argtypes = cbow_argtypes()
    L.n2v_cbow_cpu_subnormals.restype = C.c_int64
    return L


def _head(walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, negative, alpha):
    from node2vec_amd import sgns

    w = np.ascontiguousarray(walks, np.int32)
    cum = np.ascontiguousarray(cum).view(np.uint32)
    si = None if sample_int is None else np.ascontiguousarray(sample_int).view(np.uint32)
    exp = sgns.exp_table()
    assert s0.dtype == np.float32 and s1.dtype == np.float32 and s0.flags.c_contiguous and s1.flags.c_contiguous
    keep = (w, cum, si, exp)  # alive until the call returns
    return keep, [w.ctypes.data, w.shape[0], w.shape[1], s0.ctypes.data, s1.ctypes.data, cum.ctypes.data,
                  None if si is None else si.ctypes.data, exp.ctypes.data, n_vocab, base, seed, dim, window,
                  negative, float(alpha)]


def hub_sgns_train(L, walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, negative, alpha, hub_rows,
                   window_cache=0, mutation=0, roles=None):
    """the default trainer's hub form, in place on (s0, s1); returns the pairs"""
    keep, head = _head(walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, negative, alpha)
    n = L.n2v_sgns_hub_cpu_train(*head, hub_rows, window_cache, mutation, None if roles is None else roles.ctypes.data)
    assert n >= 0, "the hub restatement refused its arguments"
    return int(n)


def hub_batched_train(L, walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, negative, alpha, hub_rows,
                      ctx_store=0, mutation=0):
    """the batched trainer's hogwild form (ctx_store = 1: context rows go back as stores)"""
    keep, head = _head(walks, s0, s1, cum, sample_int, n_vocab, base, seed, dim, window, negative, alpha)
    n = L.n2v_sgns_hub_cpu_train_batched(*head, hub_rows, ctx_store, mutation)
    assert n >= 0, "the hub restatement refused its arguments"
    return int(n)


class Case:
    """kind: "sgns" (the default trainer), "batched" or "cbow".  Arrays are numpy, on the host."""

    def __init__(self, kind, walks, dim, window, negative, sample, seed, hub_rows, window_cache=0, cbow_mean=1):
        from node2vec_amd import sgns

        self.kind, self.dim, self.window, self.negative, self.sample, self.seed = kind, dim, window, negative, sample, seed
        self.window_cache, self.cbow_mean = window_cache, cbow_mean
        self.vocab = sgns.build_vocab(walks, 1)
        self.n_vocab = len(self.vocab)
        self.hub_rows = self.n_vocab if hub_rows == ALL else hub_rows
        m = sgns.SgnsModel(self.vocab, dim, window, negative, seed=seed, sample=sample)  # on the CPU: tables only
        self.walks = self.vocab.index_of[walks.long()].numpy().astype(np.int32)
        self.cum = m.cum_table.numpy().copy()
        self.sample_int = None if m.sample_int is None else m.sample_int.numpy().copy()
        self.m0 = m.syn0.numpy().copy()
        self.m1 = np.zeros_like(self.m0)
        rows = self.walks.shape[0]
        self.launches = ((0, 0.025), (rows, 0.02))  # two launches: differences carry over
        self.name = (f"{kind}-d{dim}-w{window}-k{negative}-s{sample:g}-h{self.hub_rows}of{self.n_vocab}"
                     f"-c{window_cache}-m{cbow_mean}")

    def run(self, libs, hub_rows=None, store_form=False, mutation=0, roles=None, hub=None, cbow=None):
        """all launches from the initial state under the hub restatement (hub_rows: the case's own unless
        given), or under the pinned store-form restatement: (syn0, syn1neg, pairs).  hub / cbow: another
        build of the restatement (the instrumented one)."""
        from node2vec_amd import sgns
        from test_cbow_host import cpu_train

        h = self.hub_rows if hub_rows is None else hub_rows
        s0, s1, n = self.m0.copy(), self.m1.copy(), 0
        for base, alpha in self.launches:
            a = (self.walks, s0, s1, self.cum, self.sample_int, self.n_vocab, base, self.seed, self.dim, self.window,
                 self.negative, alpha)
            if self.kind == "cbow":
                n += int(cpu_train(cbow or libs.cbow, *a, self.cbow_mean, hub_rows=0 if store_form else h,
                                   mutation=mutation))
            elif store_form:
                n += libs.oracle.sgns_train(*a[:5], sgns.exp_table(), *a[5:], batched=self.kind == "batched")
            elif self.kind == "batched":
                n += hub_batched_train(hub or libs.hub, *a, h, 0, mutation)
            else:
                n += hub_sgns_train(hub or libs.hub, *a, h, self.window_cache, mutation, roles)
        return s0, s1, n


def zipf_walks(n_tok, rows, ln, seed):
    """the corpus of test_sgns_gpu._setup"""
    gen = torch.Generator().manual_seed(seed)
    p = 1.0 / torch.arange(1, n_tok + 1, dtype=torch.float64)
    return torch.multinomial(p, rows * ln, replacement=True, generator=gen).reshape(rows, ln).to(torch.int32)


def walk_like(n_tok, rows, ln, seed):
    """the walk-like corpus of test_sgns_batched_gpu._corpus: immediate returns and short cycles, so the
    window holds a word at several positions (shared ring rows, multiplicities > 1)"""
    gen = torch.Generator().manual_seed(seed)
    steps = torch.randint(-2, 3, (rows, ln), generator=gen)
    walks = (torch.cumsum(steps, 1) + torch.randint(0, n_tok, (rows, 1), generator=gen)) % n_tok
    back = torch.rand((rows, ln), generator=gen) < 0.3
    walks[:, 2:] = torch.where(back[:, 2:], walks[:, :-2], walks[:, 2:])
    return walks.to(torch.int32)


# ---- one wave: the parameters ------------------------------------------------------------------------------

# the default trainer: dim 200 has guarded tail lanes, 512 is VEC 8 with three negatives in flight; negative 12
# runs the further target groups; hub_rows 7 puts hub and plain rows into one position
SGNS_PARAMS = [(dim, negative, sample, hub, 0) for dim in (64, 128, 200, 512) for negative in (5, 12)
               for sample in (0.0, 1e-2) for hub in (1, 7, ALL)]
# the window cache: its ring write-back is an atomic add whatever hub_rows is
SGNS_PARAMS += [(dim, 5, 1e-2, hub, 1) for dim in (64, 128) for hub in (0, 7)]


def sgns_case(dim, negative, sample, hub, window_cache):
    return Case("sgns", zipf_walks(60, 40, 21, 5 + dim), dim, 5, negative, sample, 5 + dim, hub, window_cache)


# the batched trainer: both TROWS (1 + negative <= 8 or not) and both KC (2 * window + 2 <= 12 or not)
BATCHED_PARAMS = [(dim, window, negative, hub) for dim in (64, 128, 256) for window, negative in ((5, 5), (7, 15), (1, 1))
                  for hub in (0, 7, ALL)]


def batched_case(dim, window, negative, hub):
    sample = 1e-2 if window == 5 else 0.0
    return Case("batched", walk_like(60, 40, 21, 5 + dim), dim, window, negative, sample, 5 + dim, hub)


def cbow_params():
    from test_cbow_gpu import BIT_CASES

    return [(dim, window, mean, sample, hub) for dim, window, mean, sample in BIT_CASES for hub in (7, ALL)]


def cbow_case(dim, window, cbow_mean, sample, hub):
    return Case("cbow", zipf_walks(60, 40, 21, 5 + dim), dim, window, 5, sample, 5 + dim, hub, cbow_mean=cbow_mean)


# ---- many waves: the conflict-free corpora of conflict_free.py under the hub form ----------------------------

MANY_DIMS = (64, 128, 200, 512)
# every row a hub, and a cut in the middle of the vocabulary: the words of every sentence are dealt out at
# random over 1 .. 1024, so each sentence has words on both sides of it (asserted by the host test)
MANY_HUBS = (ALL, 513)
