"""Corpora on which the racy (hogwild) trainers are schedule-independent, and the proof that they are.

Both word2vec updates skip a node or target whose f <= -6 or f >= 6 BEFORE any store.  So a launch of
many unsynchronised waves computes exactly what one thread computes when
  * no two sentences train the same row, and
  * the rows every sentence reads (HS: the top of the tree; SGNS and CBOW: the negative samples) are
    saturated: nobody ever changes them (the batched kernel rewrites them, with the bits they hold).
CBOW: every target of a position other than its centre word is the sink, whose f against the summed
(or averaged) context is >= 6; what trains is syn1neg[centre] and syn0[context], all of them words of
one sentence.
The batched skip-gram kernel (n2v_sgns_batched.hip) has no skip before the store: it writes EVERY target
row of a position back, the saturated sinks included.  Schedule independence only needs that a shared row
is never given other bits than it holds, and that is what happens: the sink's coefficients G are the
literal 0.0f (|f| >= 6), so its store writes old + sum(0 * x) and its hub-form add puts +0 + sum(0 * x)
onto memory.  With finite x and no -0 in the sink row both are the row's own bits: every wave stores the
same 4-byte words over and over, and a reader sees those words under any schedule.  `prove` checks the
first half (the shared rows keep their bits under the restatement, which performs the same stores and
adds); tests/test_batched_geometry_host.py checks the two premises, finite values and no -0.
`prove` checks those conditions under the CPU restatement alone; only then is a GPU comparison with
the restatement's joint run meaningful (tests/test_train_geometry_cpu.py, test_train_geometry_gpu.py).

Not a test module: helpers shared by the two.
"""
import numpy as np

V_WORDS = 1024            # words that occur in sentences: 32 waves by the library's rule n_vocab / 32
TOKENS = 40               # tokens per sentence
WINDOW = 5
NEGATIVE = 5
SEED = 5
SATURATED = 8.0           # f = 8 * syn0[., 0] at a shared row; syn0[., 0] stays far above 6 / 8
# launches of one case: sentence_base moves on by the number of rows, the rate falls
ALPHAS = (0.025, 0.02, 0.015)


class Case:
    """one corpus and model: numpy matrices, and `run(walks, m0, m1, base, alpha) -> pairs`, the CPU
    restatement training `walks` in place on (m0, m1) with sentence ids base, base + 1, ..."""

    def __init__(self, name, dim, walks, m0, m1, shared, run, extra=None):
        self.name, self.dim, self.walks, self.m0, self.m1 = name, dim, walks, m0, m1
        self.shared = np.asarray(shared, np.int64)  # rows of m1 every sentence reads and nobody writes
        self.run = run
        self.extra = extra or {}

    def launches(self):
        rows = self.walks.shape[0]
        return [(k * rows, a) for k, a in enumerate(ALPHAS)]


def prove(case):
    """The conditions of the module docstring, under the restatement alone.  Returns the joint run:
    (m0, m1, pairs).  A case that fails here is a wrongly built case."""
    walks = case.walks
    j0, j1 = case.m0.copy(), case.m1.copy()
    pairs = 0
    for base, alpha in case.launches():
        pairs += case.run(walks, j0, j1, base, alpha)
    assert pairs > 0
    # the shared rows keep their bits
    assert np.array_equal(j1[case.shared].view(np.uint32), case.m1[case.shared].view(np.uint32)), \
        "a shared row was written: it is not saturated"
    # every sentence alone, from the initial state, under the sentence ids of the joint run
    merged0, merged1 = case.m0.copy(), case.m1.copy()
    touch0 = np.zeros(case.m0.shape[0], np.int64)
    touch1 = np.zeros(case.m1.shape[0], np.int64)
    alone = 0
    for r in range(walks.shape[0]):
        s0, s1 = case.m0.copy(), case.m1.copy()
        for base, alpha in case.launches():
            alone += case.run(walks[r:r + 1], s0, s1, base + r, alpha)  # n_walks = 1
        c0 = (s0.view(np.uint32) != case.m0.view(np.uint32)).any(1)
        c1 = (s1.view(np.uint32) != case.m1.view(np.uint32)).any(1)
        touch0 += c0
        touch1 += c1
        merged0[c0] = s0[c0]
        merged1[c1] = s1[c1]
    assert touch0.max() <= 1 and touch1.max() <= 1, "a row is changed by two sentences"
    assert not touch1[case.shared].any()
    assert alone == pairs
    assert np.array_equal(merged0.view(np.uint32), j0.view(np.uint32)), "merged per-sentence runs != joint run (syn0)"
    assert np.array_equal(merged1.view(np.uint32), j1.view(np.uint32)), "merged per-sentence runs != joint run (syn1)"
    # it trained, and widely: a vacuous case proves nothing
    assert touch0.sum() > walks.shape[0] * 4 and touch1.sum() > walks.shape[0] * 4
    return j0, j1, pairs


def _sentences(rng, groups, oov, tokens=TOKENS, back=0.0):
    walks = np.stack([rng.choice(g, tokens) for g in groups]).astype(np.int32)
    if back:  # walk-like: a token repeats the one two places back (a b a)
        for t in np.arange(2, tokens):
            again = rng.random(len(groups)) < back
            walks[again, t] = walks[again, t - 2]
    if oov:  # out-of-vocabulary tokens: dropped before windowing
        walks[rng.random(walks.shape) < 0.15] = -1
        walks[0, :3] = -1
        walks[-1, -2:] = -1
    return walks


def _syn0(rng, rows, dim, away_from_zero=False):
    if away_from_zero:
        # magnitudes in [0.5, 1) / dim with random signs (see sgns_case)
        x = (0.5 + 0.5 * rng.random((rows, dim))) * rng.choice([-1.0, 1.0], (rows, dim)) / dim
    else:
        x = (rng.random((rows, dim)) - 0.5) / dim  # word2vec's initialisation
    x = x.astype(np.float32)
    x[:, 0] = 1.0
    return x


# ---- hierarchical softmax ------------------------------------------------------------------------------------

def hs_tree():
    """1024 words of equal count: CreateBinaryTree gives a complete tree of depth 10"""
    from node2vec_amd import hs

    tree = hs.build_tree(np.full(V_WORDS, 7, np.int64))
    assert tree.lengths.min() == tree.lengths.max() == 10
    return tree


def hs_case(hs_cpu, dim, depth=5, oov=False, saturated=SATURATED):
    """2^depth sentences; sentence s draws only from the words under the s-th node of depth `depth`.
    The syn1 rows of depth < `depth` are [saturated, 0, ...]: with syn0[:, 0] = 1 their f is >= 6 and
    they are never written.  Every other syn1 row is zero (Spark's initialisation) and lies on the paths
    of one sentence's words only."""
    from node2vec_amd import sgns

    tree = hs_tree()
    paths = np.ascontiguousarray(tree.points.reshape(V_WORDS, 10))
    groups = {}
    for w in range(V_WORDS):
        groups.setdefault(int(paths[w, depth]), []).append(w)
    assert len(groups) == 2 ** depth and {len(g) for g in groups.values()} == {V_WORDS >> depth}
    shared = np.unique(paths[:, :depth])
    assert shared.size == 2 ** depth - 1
    rng = np.random.default_rng(1000 * dim + 10 * depth + int(oov))
    m0 = _syn0(rng, V_WORDS, dim)
    m1 = np.zeros((V_WORDS - 1, dim), np.float32)
    m1[shared, 0] = saturated
    walks = _sentences(rng, [groups[k] for k in sorted(groups)], oov)
    pts, exp = np.ascontiguousarray(tree.points), sgns.exp_table()

    def run(w, s0, s1, base, alpha):
        w = np.ascontiguousarray(w, np.int32)
        return int(hs_cpu.n2v_hs_cpu_train(w.ctypes.data, w.shape[0], w.shape[1], s0.ctypes.data, s1.ctypes.data,
                                           tree.path_off.ctypes.data, pts.ctypes.data, tree.codes.ctypes.data,
                                           exp.ctypes.data, V_WORDS, base, SEED, dim, WINDOW, float(alpha), None))

    return Case(f"hs-{dim}-{depth}-{int(oov)}", dim, walks, m0, m1, shared, run, {"tree": tree})


# ---- negative sampling ---------------------------------------------------------------------------------------

SINK = 0  # the word that takes every negative draw and occurs in no sentence


def sgns_cum_table():
    """all the mass of the noise distribution on word 0: bisect_left(cum_table, x) is 0 for every draw"""
    from node2vec_amd import sgns

    return np.full(V_WORDS + 1, sgns.CUM_DOMAIN, np.int32)


def sgns_case(oracle, dim, sentences=32, oov=False, saturated=SATURATED, hub_rows=0, hub_cpu=None):
    """`sentences` sentences over disjoint word sets (words 1 .. 1024 dealt out at random); every
    negative is the sink word 0, whose syn1neg row [saturated, 0, ...] has f >= 6 against every syn0 row
    (syn0[:, 0] = 1, and label-1 updates only raise it).  What trains is the label-1 pair: syn0[context]
    and syn1neg[centre], both words of the same sentence.

    The other syn0 elements have magnitudes in [0.5, 1) / dim.  With the window cache a context row
    goes back to memory as an atomic add of (value now - value as loaded); on a row nobody else writes
    that equals a store whenever the subtraction is exact, which Sterbenz's lemma gives while an element
    moves by less than half of itself between load and write-back.  Here a syn0 element moves by at most
    12 % of itself over a whole launch (measured under the oracle; test_train_geometry_cpu.py holds the
    three launches together under 50 %), and a row stays cached for a few positions of one sentence.

    hub_rows > 0: the case trains under the hub form instead (rows below hub_rows take atomic adds), stated
    by the restatement `hub_cpu` (hub_form_cases.load_hub) in place of the oracle.  Those adds need not be
    exact: what makes the launch schedule-independent is that one sentence alone adds to a row, in its own
    order, which `prove` checks under that restatement."""
    from node2vec_amd import sgns

    n_vocab = V_WORDS + 1
    rng = np.random.default_rng(2000 * dim + 10 * sentences + int(oov))
    words = 1 + rng.permutation(V_WORDS)
    groups = np.split(words, sentences)
    m0 = _syn0(rng, n_vocab, dim, away_from_zero=True)
    m1 = np.zeros((n_vocab, dim), np.float32)
    m1[SINK, 0] = saturated
    walks = _sentences(rng, groups, oov)
    assert not (walks == SINK).any()
    cum, exp = sgns_cum_table(), sgns.exp_table()

    def run(w, s0, s1, base, alpha):
        if hub_rows:
            from hub_form_cases import hub_sgns_train

            return hub_sgns_train(hub_cpu, w, s0, s1, cum, None, n_vocab, base, SEED, dim, WINDOW, NEGATIVE, alpha,
                                  hub_rows)
        return oracle.sgns_train(w, s0, s1, cum, None, exp, n_vocab, base, SEED, dim, WINDOW, NEGATIVE, alpha)

    return Case(f"sgns-{dim}-{sentences}-{int(oov)}" + (f"-h{hub_rows}" if hub_rows else ""), dim, walks, m0, m1,
                [SINK], run)


# ---- CBOW with negative sampling -----------------------------------------------------------------------------

def cbow_case(cbow_cpu, dim, sentences=32, oov=False, cbow_mean=1, saturated=SATURATED, negative=NEGATIVE,
              hub_rows=0):
    """the corpus of sgns_case under the CBOW update: every draw of a position is the sink word 0, whose
    syn1neg row [saturated, 0, ...] has f = saturated * neu1[0] >= 6 -- neu1[0] is the sum (cbow_mean 0)
    or the mean (1) of syn0[context, 0], all 1 at the start, and only raised: the label-1 update adds
    g * neu1 with g > 0 to syn1neg[centre], so work[0] = g * syn1neg[centre, 0] >= 0.  What trains is
    syn1neg[centre] and syn0[context], words of the same sentence.  CBOW has no window cache: rows go
    back by plain stores, so syn0 takes word2vec's own initialisation.  Any `negative` does: every
    draw is the sink.  hub_rows > 0: the restatement's hub form (rows below it take atomic adds)."""
    from test_cbow_host import cpu_train

    n_vocab = V_WORDS + 1
    rng = np.random.default_rng(3000 * dim + 10 * sentences + int(oov))
    words = 1 + rng.permutation(V_WORDS)
    groups = np.split(words, sentences)
    m0 = _syn0(rng, n_vocab, dim)
    m1 = np.zeros((n_vocab, dim), np.float32)
    m1[SINK, 0] = saturated
    walks = _sentences(rng, groups, oov)
    assert not (walks == SINK).any()
    cum = sgns_cum_table()

    def run(w, s0, s1, base, alpha):
        return int(cpu_train(cbow_cpu, w, s0, s1, cum, None, n_vocab, base, SEED, dim, WINDOW, negative, alpha,
                             cbow_mean, hub_rows=hub_rows))

    return Case(f"cbow-{dim}-{sentences}-{int(oov)}-{cbow_mean}-k{negative}" + (f"-h{hub_rows}" if hub_rows else ""),
                dim, walks, m0, m1, [SINK], run)


# ---- the batched skip-gram trainer (negatives shared by the pairs of a position) ------------------------------

def batched_case(hub_cpu, dim, window, negative, sinks, sentences=32, tokens=TOKENS, oov=False, hub_rows=0,
                 ctx_store=0):
    """`sinks` sink words at rows 0 .. sinks - 1, then the 1024 sentence words, dealt out at random over
    `sentences` disjoint groups.  The noise table spreads its mass evenly over the sinks, each with the
    syn1neg row [SATURATED, 0, ...]: every negative is a sink, f >= 6 against syn0[:, 0] = 1 (which the
    label-1 updates only raise), G = 0, and the row is rewritten with its own bits (module docstring).  One
    sink would give every position two targets and one multiplicity; several make the number of distinct
    targets and their multiplicities vary from position to position, which the target tile, the packed
    multiplicity words and the `late` masks need.

    syn0 takes word2vec's ordinary initialisation (column 0 apart): the ring's write-back add
    loaded + (t - loaded) then differs in bits from a store of t on some elements, so a kernel that stores
    where it should add fails (with magnitudes kept away from zero the two agree everywhere).  Sentences are
    walk-like -- about 30 % of the tokens from index 2 on repeat the token two places back -- so the window
    holds a word at several positions: shared ring rows, multiplicities > 1.

    The run is the hub restatement's (hub_form_cases.hub_batched_train) under hub_rows and ctx_store
    (1: context rows go back as stores, the deterministic form -- the twin a hogwild launch must differ from)."""
    from hub_form_cases import hub_batched_train
    from node2vec_amd import sgns

    n_vocab = V_WORDS + sinks
    rng = np.random.default_rng([4000, dim, window, negative, sinks, sentences, tokens, int(oov)])
    words = sinks + rng.permutation(V_WORDS)
    groups = np.split(words, sentences)
    m0 = _syn0(rng, n_vocab, dim, away_from_zero=False)
    m1 = np.zeros((n_vocab, dim), np.float32)
    m1[:sinks, 0] = SATURATED
    walks = _sentences(rng, groups, oov, tokens, back=0.3)
    assert walks.min() >= (-1 if oov else sinks)
    cum = np.full(n_vocab, sgns.CUM_DOMAIN, np.int64)
    cum[:sinks] = (np.arange(sinks) + 1) * sgns.CUM_DOMAIN // sinks
    cum = cum.astype(np.int32)

    def run(w, s0, s1, base, alpha):
        return hub_batched_train(hub_cpu, w, s0, s1, cum, None, n_vocab, base, SEED, dim, window, negative, alpha,
                                 hub_rows, ctx_store)

    name = f"batched-{dim}-w{window}-k{negative}-s{sinks}-{sentences}x{tokens}-{int(oov)}-h{hub_rows}-c{ctx_store}"
    return Case(name, dim, walks, m0, m1, np.arange(sinks), run,
                {"cum": cum, "n_vocab": n_vocab, "window": window, "negative": negative, "sinks": sinks})


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    """splitmix64's finaliser over a uint64 array (numpy's uint64 products wrap)"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def batched_plans(case):
    """What the batched trainer's plan holds for every (launch, sentence, kept position) of the case,
    restated in plain numpy from the trainers' draw streams: sentence stream mix64(seed ^ mix64(id + c0)),
    draw idx -> mix64(stream + (idx + 1) * c1), negative d of kept position i at idx 2 * walk_len +
    i * 2 * window * negative + d, word = bisect_left(cum, (draw >> 16) % domain); targets = the centre,
    then the distinct draws other than it.  Returns (distinct targets per position, largest multiplicity
    per position, nf per sentence) as three flat lists."""
    cum = case.extra["cum"].view(np.uint32)
    window, negative = case.extra["window"], case.extra["negative"]
    walk_len = case.walks.shape[1]
    domain = np.uint64(cum[-1])
    n_targets, max_mult, nfs = [], [], []
    with np.errstate(over="ignore"):
        for base, _ in case.launches():
            for r, row in enumerate(case.walks):
                sent = row[(row >= 0) & (row < case.extra["n_vocab"])]
                nfs.append(len(sent))
                if len(sent) < 2:
                    continue
                sid = np.array([base + r], np.uint64)
                hs = _mix64(np.uint64(SEED) ^ _mix64(sid + np.uint64(0xA0761D6478BD642F)))
                i = np.arange(len(sent), dtype=np.uint64)[:, None]
                d = np.arange(negative, dtype=np.uint64)[None, :]
                idx = np.uint64(2 * walk_len) + i * np.uint64(2 * window * negative) + d
                x = (_mix64(hs + (idx + np.uint64(1)) * np.uint64(0xE7037ED1A0B428DB)) >> np.uint64(16)) % domain
                word = np.searchsorted(cum, x.astype(np.uint32), side="left")
                for c, ws in zip(sent, word):
                    ws = ws[ws != c]
                    _, counts = np.unique(ws, return_counts=True)
                    n_targets.append(1 + len(counts))
                    max_mult.append(int(counts.max()) if len(counts) else 1)
    return n_targets, max_mult, nfs
