"""CBOW with negative sampling on the GPU (csrc/n2v_cbow.hip, SgnsModel(sg=0), Node2VecHIP {"sg": 0}).

Deterministic mode (one wave, rows in order) must equal the CPU restatement
tests/cpu_cbow/n2v_cbow_cpu.c BIT FOR BIT -- syn0, syn1neg and the count of trained positions -- for
every VEC instance of the kernel, at a dimension that fills the wave and at one that does not, with
cbow_mean 0 and 1.  Every bit case asserts from the restatement alone that it trains, that a window
holds a word twice and that a negative draw equals its centre word.  The statistical tests bound the
hogwild mode's quality.

Elsewhere: test_cbow_groups_gpu.py puts `negative` on the edges of the kernel's target groups for every
VEC, the batches of draws at their extremes and long windows over the context groups (every bit case
here has negative = 5); test_train_geometry_gpu.py compares the hogwild launch on many waves bit for
bit on the conflict-free corpora of conflict_free.py.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from test_cbow_host import cbow_cpu, cpu_train  # noqa: F401  (the session fixture that builds the restatement)

pytestmark = pytest.mark.gpu

# TOLERANCES, measured on one MI355X:
#   planted partition (test_sgns_gpu.planted_case trained with sg=0, cbow_mean=1; 64 waves in flight;
#   scripts/cbow_stat_runs.py -> profiles/cbow_stat_runs.log, 30 hogwild runs against the deterministic run):
#     community AUC deterministic 0.999974 (it separates the communities: the statistic discriminates);
#     hogwild 0.999986 +- 0.000003 (min 0.999980, max 0.999991), mean - 5 sd = 0.999972;
#     |hogwild - deterministic| 0.000012 +- 0.000003 (max 0.000017), mean + 5 sd = 0.000025.
#     Bounds, looser than mean -+ 5 sd and those of the skip-gram test: AUC > 0.99, |difference| < 0.01.
#   hub_rows on one wave (test_hub_rows_on_one_wave, over the 24 bit cases, two launches each): the largest
#     |difference| from the restatement is 4.858e-05, at dim 1 / window 5 / cbow_mean 0, where values reach 1.36
#     (every other case: 7e-10 .. 1.6e-06).  It is not 0: a hub row's target update is an atomic add of the
#     ROUNDED product g * neu1, two roundings where the store form's fmaf has one, and the difference is then
#     carried through two launches.  Bound: twice the measured value.
PLANTED_AUC_MIN, PLANTED_AUC_DIFF_MAX = 0.99, 0.01
HUB_ONE_WAVE_MAX_DIFF = 2 * 4.858e-05


def _case(n_tok, rows, ln, dim, window, negative, seed, sample, cbow_mean, min_count=1, oov=False):
    """the Zipf corpus and model of test_sgns_gpu._setup, turned into a CBOW model"""
    from test_sgns_gpu import _setup

    sgns, m, idx = _setup(n_tok, rows, ln, dim, seed, sample, min_count, oov)
    m.sg, m.cbow_mean, m.window, m.negative = 0, cbow_mean, window, negative
    return sgns, m, idx


def _cpu(L, m, idx, s0, s1, base, alpha, row_alpha=None, stats=None):
    return cpu_train(L, idx.cpu().numpy(), s0, s1, m.cum_table.cpu().numpy(),
                     None if m.sample_int is None else m.sample_int.cpu().numpy(), len(m.vocab), base, m.seed,
                     m.dim, m.window, m.negative, alpha, m.cbow_mean, row_alpha, stats)


def _assert_case_is_meaningful(s0_before, s0, n, stats):
    """from the restatement alone: the case trains, a window holds a word twice, a draw equals its centre"""
    assert n > 0 and float(np.abs(s0 - s0_before).max()) > 1e-4
    assert stats[0] > 0, "no window of this case holds a word twice"
    assert stats[1] > 0, "no negative draw of this case equals its centre word"


def _check_bits(L, m, idx, launches, deterministic=True, sched=None):
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1neg.cpu().numpy().copy()
    before = s0.copy()
    stats = np.zeros(2, np.int64)
    n = 0
    for base, alpha in launches:
        extra = {} if sched is None else {"sched": sched, "row0": 0}
        m.train_block(idx, alpha, base, deterministic=deterministic, **extra)
        ra = None if sched is None else sched.alpha_of_rows(0, idx.shape[0])
        n += _cpu(L, m, idx, s0, s1, base, alpha, ra, stats)
    torch.cuda.synchronize()
    _assert_case_is_meaningful(before, s0, n, stats)
    g0, g1 = m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy()
    assert int(m.pairs.item()) == n
    assert np.isfinite(g0).all() and np.isfinite(g1).all()
    assert np.array_equal(g0, s0), float(np.abs(g0 - s0).max())
    assert np.array_equal(g1, s1), float(np.abs(g1 - s1).max())
    return n


# every VEC instance (1 / 2 / 4 / 8 / 16) at a dimension that fills the wave (64 * VEC) and at one that
# does not; 1000 is the ragged dimension of VEC 16.  Window and subsampling rotate over the cases.
DIMS = [1, 16, 63, 64, 100, 128, 200, 256, 300, 512, 1000, 1024]
BIT_CASES = [(dim, (5, 1, 32)[j % 3], mean, (0.0, 1e-2)[(j + mean) % 2])
             for j, dim in enumerate(DIMS) for mean in (0, 1)]


def _vec(dim):
    v = 1
    while 64 * v < dim:
        v *= 2
    return v


def test_bit_cases_cover_what_they_claim():
    assert {c[1] for c in BIT_CASES} == {1, 5, 32} and {c[3] for c in BIT_CASES} == {0.0, 1e-2}
    for vec in (1, 2, 4, 8, 16):
        for mean in (0, 1):
            mine = [c[0] for c in BIT_CASES if c[2] == mean and _vec(c[0]) == vec]
            assert 64 * vec in mine and any(d != 64 * vec for d in mine), (vec, mean, mine)


@pytest.mark.parametrize("dim,window,cbow_mean,sample", BIT_CASES)
def test_deterministic_mode_bit_identical_to_restatement(cbow_cpu, dim, window, cbow_mean, sample):
    sgns, m, idx = _case(60, 40, 21, dim, window, 5, seed=5 + dim, sample=sample, cbow_mean=cbow_mean)
    rows = idx.shape[0]
    _check_bits(cbow_cpu, m, idx, ((0, 0.025), (rows, 0.02)))  # two launches: sentence_base moves on
    assert np.abs(m.syn1neg.cpu().numpy()).max() > 0


@pytest.mark.parametrize("cbow_mean", [0, 1])
def test_oov_tokens_min_count_and_long_window(cbow_cpu, cbow_mean):
    """min_count drops rare tokens, -1 and out-of-range tokens are dropped BEFORE windowing; window 30,
    negative 20 (several groups of targets, several groups of context rows)"""
    sgns, m, idx = _case(200, 30, 40, 32, 30, 20, seed=9, sample=1e-3, cbow_mean=cbow_mean, min_count=4, oov=True)
    idx = idx.clone()
    idx[2, 10:20] = len(m.vocab) + 5  # >= n_vocab: dropped like a -1
    idx[3, ::3] = -7
    _check_bits(cbow_cpu, m, idx, ((7, 0.025),))


def test_long_rows_through_split_rows_and_per_row_rates(cbow_cpu):
    """rows of 700 tokens cut by split_rows into sentences of 256; the rate of every row from JobSchedule"""
    sgns, m, idx = _case(500, 6, 700, 128, 5, 5, seed=11, sample=1e-3, cbow_mean=1)
    rows = sgns.split_rows(idx)
    assert rows.shape == (18, sgns.MAX_SENTENCE) and int((rows < 0).sum()) > 0
    sched = sgns.JobSchedule(4, rows.shape[0], 1, 3, 0.025, 1e-4)
    ra = sched.alpha_of_rows(0, rows.shape[0])
    assert len(set(ra.tolist())) == 5  # jobs of 4 rows: 5 different rates in the launch
    _check_bits(cbow_cpu, m, rows, ((36, 0.5),), sched=sched)  # (the launch's own alpha is not used)


@pytest.mark.parametrize("dim", [16, 128, 256, 1024])
@pytest.mark.parametrize("cbow_mean", [0, 1])
def test_single_wave_hogwild_equals_restatement(cbow_cpu, dim, cbow_mean):
    """hogwild mode on ONE wave (max_waves = 1, hub_rows = 0): rows come from the counter in order"""
    sgns, m, idx = _case(60, 40, 21, dim, 5, 5, seed=3 + dim, sample=1e-2, cbow_mean=cbow_mean)
    m.max_waves, m.hub_rows = 1, 0
    assert m.hogwild_waves(*idx.shape) == 1
    _check_bits(cbow_cpu, m, idx, ((0, 0.025), (idx.shape[0], 0.02)), deterministic=False)


def test_hogwild_count_equals_restatement_and_values_are_finite(cbow_cpu):
    """the set of trained positions does not depend on launch geometry"""
    sgns, m, idx = _case(3000, 4000, 41, 128, 5, 5, seed=1, sample=1e-3, cbow_mean=1)
    assert m.hogwild_waves(*idx.shape) > 1
    s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1neg.cpu().numpy().copy()
    m.train_block(idx, 0.025, 0)
    torch.cuda.synchronize()
    assert m.hub_rows == 0 and not m.hub_rows_auto  # hub_rows=None means 0 for CBOW
    assert int(m.pairs.item()) == _cpu(cbow_cpu, m, idx, s0, s1, 0, 0.025) > 0
    assert np.isfinite(m.syn0.cpu().numpy()).all() and np.isfinite(m.syn1neg.cpu().numpy()).all()


def test_batched_is_refused_with_cbow():
    sgns, m, idx = _case(60, 8, 12, 64, 5, 5, seed=1, sample=0.0, cbow_mean=1)
    m.batched = True
    with pytest.raises(ValueError):
        m.train_block(idx, 0.025, 0)
    m.batched, m.window_cache = False, 1
    with pytest.raises(ValueError):  # n2v_cbow_train: N2V_EINVAL
        m.train_block(idx, 0.025, 0)


def test_offsets_past_2_31_elements(cbow_cpu):
    """a model of more than 2^31 syn0 (and syn1neg) elements, trained deterministically on its last 40
    rows: the cumulative table sends every negative draw to those rows too, so the same training runs
    on the restatement with the 40 rows compacted"""
    from node2vec_amd import sgns

    dim, tail = 1024, 40
    V = (1 << 21) + 64
    counts = torch.arange(V, 0, -1, dtype=torch.int64) + 10
    vocab = sgns.Vocab(torch.arange(V).cuda(), counts.cuda(), torch.arange(V, dtype=torch.int32).cuda())
    m = sgns.SgnsModel(vocab, dim, 5, 5, seed=2, sg=0, use_cum_index=False)
    assert m.syn0.numel() > 2 ** 31 and m.syn1neg.numel() > 2 ** 31 and (V - tail) * dim >= 2 ** 31
    cum = torch.zeros(V, dtype=torch.int64)
    cum[V - tail:] = torch.linspace(1 << 20, sgns.CUM_DOMAIN, tail, dtype=torch.float64).to(torch.int64)
    cum[-1] = sgns.CUM_DOMAIN
    m.cum_table = cum.to(torch.int32).cuda()
    gen = torch.Generator().manual_seed(0)
    idx = (V - 1 - torch.randint(0, tail, (4, 30), generator=gen)).to(torch.int32).cuda()
    # non-zero outputs: f matters, and the error is large enough for the pass to move syn0 by > 1e-4
    m.syn1neg[V - tail:] = 0.05 * torch.randn((tail, dim), generator=torch.Generator(device="cuda").manual_seed(4),
                                              device="cuda")
    s0, s1 = m.syn0[V - tail:].cpu().numpy().copy(), m.syn1neg[V - tail:].cpu().numpy().copy()
    before = s0.copy()
    head_sum = m.syn0[:V - tail].sum(dtype=torch.float64).item()
    m.train_block(idx, 0.025, 0, deterministic=True)
    torch.cuda.synchronize()
    stats = np.zeros(2, np.int64)
    cidx = (idx.cpu().numpy() - (V - tail)).astype(np.int32)
    n = cpu_train(cbow_cpu, cidx, s0, s1, cum[V - tail:].numpy().astype(np.uint32), None, tail, 0, m.seed, dim, 5, 5,
                  0.025, 1, None, stats)
    _assert_case_is_meaningful(before, s0, n, stats)
    assert n == int(m.pairs.item())
    assert np.array_equal(m.syn0[V - tail:].cpu().numpy(), s0)
    assert np.array_equal(m.syn1neg[V - tail:].cpu().numpy(), s1)
    assert not m.syn1neg[:V - tail].any().item()  # nothing below the tail was touched
    assert m.syn0[:V - tail].sum(dtype=torch.float64).item() == head_sum


def test_hub_rows_on_one_wave(cbow_cpu):
    """every row a hub (hub_rows = n_vocab), one wave, over the bit-test corpus: the largest
    |difference| from the restatement, printed per case and bounded by HUB_ONE_WAVE_MAX_DIFF (TOLERANCES)"""
    worst = 0.0
    for dim, window, cbow_mean, sample in BIT_CASES:
        sgns, m, idx = _case(60, 40, 21, dim, window, 5, seed=5 + dim, sample=sample, cbow_mean=cbow_mean)
        m.max_waves, m.hub_rows = 1, len(m.vocab)
        s0, s1 = m.syn0.cpu().numpy().copy(), m.syn1neg.cpu().numpy().copy()
        n = 0
        for base, alpha in ((0, 0.025), (idx.shape[0], 0.02)):
            m.train_block(idx, alpha, base)
            n += _cpu(cbow_cpu, m, idx, s0, s1, base, alpha)
        torch.cuda.synchronize()
        assert int(m.pairs.item()) == n > 0
        d = max(float(np.abs(m.syn0.cpu().numpy() - s0).max()), float(np.abs(m.syn1neg.cpu().numpy() - s1).max()))
        print("hub_rows one wave: dim %d window %d cbow_mean %d sample %g: max |diff| %.3e (max |value| %.3e)"
              % (dim, window, cbow_mean, sample, d, float(np.abs(s0).max())))
        worst = max(worst, d)
    print("hub_rows one wave: largest |difference| over the bit-test corpus: %.3e" % worst)
    assert worst <= HUB_ONE_WAVE_MAX_DIFF, worst


def _karate_frame():
    from node2vec_amd.fugue import random_walk

    e = load_golden("karate_edges.json")
    return random_walk("hip", pd.DataFrame(e, columns=["src", "dst", "weight"]),
                       {"num_walks": 10, "walk_length": 10}, random_seed=42)


def test_node2vechip_cbow_end_to_end_on_karate(tmp_path):
    from node2vec_amd.embedding import HipW2V, Node2VecHIP
    from node2vec_amd.graph import DeviceGraph
    from node2vec_amd.pipeline import fit_streaming

    df_walks = _karate_frame()
    params = {"sg": 0, "negative": 5, "min_count": 0}
    n2v = Node2VecHIP(df_walks, params, random_seed=1000)
    model = n2v.fit()
    assert isinstance(model, HipW2V) and model.pairs_trained > 0
    assert model.params["sg"] == 0 and model.params["cbow_mean"] == 1 and model.params["hub_rows"] == 0
    emb = n2v.embedding()
    assert list(emb.columns) == ["id", "vector"] and len(emb) == 34 and all(len(v) == 128 for v in emb["vector"])
    assert np.isfinite(model.wv.vectors).all()
    hits = model.wv.most_similar("0", topn=5)
    assert len(hits) == 5 and all(t != "0" for t, _ in hits)
    assert len(n2v.most_similar(0, topn=3)) == 3
    n2v.save_model(str(tmp_path), "tmp")
    loaded = n2v.load_model(str(tmp_path), "tmp")
    assert np.array_equal(loaded.wv.vectors, model.wv.vectors) and np.array_equal(loaded.syn1neg, model.syn1neg)
    assert loaded.params["sg"] == 0 and loaded.pairs_trained == model.pairs_trained
    # deterministic mode: the same seed gives the same bits; cbow_mean=0 trains something else
    fits = []
    for extra in ({}, {}, {"cbow_mean": 0}):
        p = {"sg": 0, "negative": 5, "min_count": 0, "iter": 2, "deterministic": True, **extra}
        fits.append(Node2VecHIP(df_walks, p, vector_size=32, random_seed=7).fit())
    assert np.array_equal(fits[0].wv.vectors, fits[1].wv.vectors) and np.array_equal(fits[0].syn1neg, fits[1].syn1neg)
    assert fits[0].pairs_trained == fits[1].pairs_trained == fits[2].pairs_trained > 0
    assert not np.array_equal(fits[0].wv.vectors, fits[2].wv.vectors)
    # skip-gram on the same walks counts pairs, CBOW positions: fewer
    sg = Node2VecHIP(df_walks, {"negative": 5, "min_count": 0, "iter": 2, "deterministic": True}, vector_size=32,
                     random_seed=7).fit()
    assert sg.params["sg"] == 1 and sg.pairs_trained > fits[0].pairs_trained
    # the streaming pipeline
    edges = np.array(load_golden("karate_edges.json"), dtype=np.float64).reshape(-1, 3)
    g = DeviceGraph.from_edges(edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), None, n_vertices=34,
                               device="cuda")
    out = fit_streaming(g, {"num_walks": 10, "walk_length": 10}, {"sg": 0, "negative": 5, "min_count": 0, "iter": 2,
                                                                   "size": 32}, 42)
    assert out.pairs_trained > 0 and out.params["sg"] == 0 and len(out.wv) == 34
    assert np.isfinite(out.wv.vectors).all()


@pytest.mark.statistical
def test_planted_partition_hogwild_matches_deterministic(monkeypatch):
    """the planted-partition case of test_sgns_gpu.planted_case (50 communities x 40 vertices, dim 64,
    3 epochs) trained with sg=0: the community-separation AUC of the hogwild embedding against the
    deterministic one (= the CPU restatement, by the bit tests above).  Tolerances: above."""
    from node2vec_amd import sgns
    from test_sgns_gpu import planted_case

    case = planted_case()
    model = sgns.SgnsModel
    waves = []

    def cbow_model(*a, **kw):
        m = model(*a, sg=0, **kw)
        waves.append(m.hogwild_waves(20000, 41))
        return m

    monkeypatch.setattr(sgns, "SgnsModel", cbow_model)  # planted_case builds its models through the module
    det, hog = case["auc"](case["train"](True)), case["auc"](case["train"](False))
    print("planted partition CBOW community AUC: deterministic", det, "hogwild", hog, "waves", waves)
    assert len(waves) == 2 and waves[1] > 1
    assert min(det, hog) > PLANTED_AUC_MIN and abs(det - hog) < PLANTED_AUC_DIFF_MAX, (det, hog)
