"""The precondition of tests/test_batched_geometry_gpu.py, with no GPU: every corpus that file trains with the
batched skip-gram kernel in hogwild mode on many waves is conflict-free under the hub restatement
(tests/cpu_sgns_hub/n2v_sgns_hub_cpu.c, n2v_sgns_hub_cpu_train_batched), in the sense of
tests/conflict_free.py: no two sentences change a row, and the rows every sentence reads -- the saturated
sinks, which this kernel REWRITES at every position -- only ever receive the bits they hold.

For every case that goes to the GPU (CASES, imported by the GPU test):
  * conflict_free.prove passes unchanged, and syn0[:, 0] stays >= 1 (f >= 8 at every sink throughout);
  * no sink row holds a -0 and both matrices stay finite: the two premises under which old + sum(0 * x) and
    +0 + sum(0 * x) are the bits of `old`;
  * at hub_rows = 0 it differs in syn0 bits from its twin whose context rows go back as stores; with every
    row a hub, and with hub_rows = 513, it differs in syn1neg bits from hub_rows = 0: a kernel that stores
    where it should add, or the reverse, fails on the GPU;
  * every sentence has words on both sides of row 513;
  * under the instrumented build no atomic add has a subnormal operand.
The corpora reach what they were built for (a plain numpy restatement of the plan over the trainers' draw
streams, conflict_free.batched_plans): more than 8 distinct targets (the second multiplicity word, the
16-row tile), multiplicities > 1, a varying number of targets, sentences that keep every token; the
256-token case alone takes the launcher's own area for the raw draws and more than 64 KB of LDS, both
restated here from n2v_sgns_batched_launch so that a change to either formula shows.  And `prove` notices a
word shared by two sentences.
"""
import numpy as np
import pytest

import conflict_free as cf
import hub_form_cases as hc
from test_cbow_host import cbow_cpu  # noqa: F401  (session fixture behind hub_libs)
from test_hub_form_host import hub_libs  # noqa: F401  (session fixture: the restatements)

CUT = 513
# (window, negative, sinks): both target tiles (1 + negative <= 8 or not), both ring sizes (2 * window + 2 <= 12 or not)
SHAPES = ((5, 5, 4), (7, 15, 12), (1, 1, 2))
# (dim, window, negative, sinks, sentences, tokens, oov, hub_rows, max_waves, waves the launch must report)
# the library's own rule: 32 waves in 16 blocks of 2
RULE = [(dim, w, k, s, 32, cf.TOKENS, False, hub, 0, 32) for dim in (64, 128, 256) for w, k, s in SHAPES
        for hub in (0, hc.ALL, CUT)]
# 64 sentences with -1 tokens on 16 waves: about four sentences per wave through the row counter
COUNTER = [(dim, 5, 5, 4, 64, cf.TOKENS, True, hub, 16, 16) for dim in (64, 256) for hub in (0, hc.ALL)]
# max_waves = 3 is rounded up to two blocks of two waves
ROUNDED = [(128, 5, 5, 4, 32, cf.TOKENS, False, CUT, 3, 4)]
# 256 tokens x 15 negatives: the raw draws get their own LDS area, two waves take more than 64 KB
LONG = [(64, 7, 15, 12, 8, 256, False, hub, 0, 8) for hub in (0, hc.ALL)]
CASES = RULE + COUNTER + ROUNDED + LONG
IDS = ["-".join(str(x) for x in p) for p in CASES]


def _hub(p):
    return cf.V_WORDS + p[3] if p[7] == hc.ALL else p[7]


def build(libs, p, ctx_store=0, hub=None):
    dim, window, negative, sinks, sentences, tokens, oov = p[:7]
    return cf.batched_case(libs.hub, dim, window, negative, sinks, sentences, tokens, oov,
                           _hub(p) if hub is None else hub, ctx_store)


_proved = {}


def proved(libs, p):
    """(case, syn0, syn1neg, pairs) of conflict_free.prove, computed once per corpus and hub_rows and shared
    by the host and the GPU test; nobody changes the arrays"""
    key = p[:7] + (_hub(p),)
    if key not in _proved:
        case = build(libs, p)
        _proved[key] = (case,) + cf.prove(case)
    return _proved[key]


def _bits(a):
    return a.view(np.uint32)


def _joint(case):
    """the case's launches in order, from its initial state: (syn0, syn1neg, pairs)"""
    s0, s1, n = case.m0.copy(), case.m1.copy(), 0
    for base, alpha in case.launches():
        n += case.run(case.walks, s0, s1, base, alpha)
    return s0, s1, n


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_batched_corpus_is_conflict_free(hub_libs, p):
    dim, window, negative, sinks, sentences, tokens, oov = p[:7]
    case, j0, j1, pairs = proved(hub_libs, p)
    assert case.walks.shape == (sentences, tokens) and bool((case.walks < 0).any()) == oov
    assert j0[:, 0].min() >= 1.0  # label-1 updates only raise it: f >= 8 at every sink
    # the premises of "rewritten with the bits it holds"
    assert np.isfinite(j0).all() and np.isfinite(j1).all()
    for m in (case.m1, j1):
        assert not (_bits(m[:sinks]) == 0x80000000).any(), "a -0 in a sink row"
    # every sentence has words on both sides of the cut
    assert all((w[w >= 0] < CUT).any() and (w[w >= 0] >= CUT).any() for w in case.walks)
    assert case.walks[case.walks >= 0].min() >= sinks
    if _hub(p) == 0:
        s0, s1, n = _joint(build(hub_libs, p, ctx_store=1))
        d = int((_bits(s0) != _bits(j0)).sum())
        print(case.name, "pairs", pairs, "syn0 elements that differ from the stored ring:", d)
        assert n == pairs and d > 0
    else:
        _, z0, z1, n = proved(hub_libs, p[:7] + (0,) + p[8:])
        d = int((_bits(z1) != _bits(j1)).sum())
        print(case.name, "pairs", pairs, "syn1neg elements that differ from hub_rows = 0:", d)
        assert n == pairs and d > 0
    # the instrumented build: the same bits, and no subnormal operand of an atomic add
    hub_libs.hub_checked.n2v_sgns_hub_cpu_subnormals()
    checked = cf.batched_case(hub_libs.hub_checked, dim, window, negative, sinks, sentences, tokens, oov, _hub(p))
    c0, c1, n = _joint(checked)
    assert hub_libs.hub_checked.n2v_sgns_hub_cpu_subnormals() == 0
    assert n == pairs and np.array_equal(_bits(c0), _bits(j0)) and np.array_equal(_bits(c1), _bits(j1))


def _tiles(dim, window, negative):
    """PR, PT (floats between the planes of the ring and of the target tile) and the plan ints per position,
    as n2v_sgns_batched_launch derives them"""
    def bank_half_stride(n):
        return (n + 31) // 64 * 64 + 32

    rs = 16 * (dim // 64) + 4
    rrows = 12 if 2 * window + 2 <= 12 else 16
    trows = 8 if 1 + negative <= 8 else 16
    return bank_half_stride((rrows + 1) * rs), bank_half_stride(trows * rs), negative + 1 + (1 if trows == 8 else 2) + 1


def _own_negw(dim, window, negative, tokens):
    pr, pt, _ = _tiles(dim, window, negative)
    return tokens * negative > 4 * (pr + pt)


def _lds_bytes(dim, window, negative, tokens, waves_per_block=2):
    pr, pt, pl = _tiles(dim, window, negative)
    ints = (2 * tokens + tokens * pl + 32 + (tokens * negative if _own_negw(dim, window, negative, tokens) else 0)
            + 3) & ~3
    return 1000 * 4 + waves_per_block * (4 * pr + 4 * pt + 16 * 17 + ints) * 4


def test_the_corpora_reach_what_they_are_built_for(hub_libs):
    seen = set()
    for p in CASES:
        dim, window, negative, sinks, sentences, tokens, oov = p[:7]
        if p[1:7] in seen:  # (the draws do not depend on dim or hub_rows)
            continue
        seen.add(p[1:7])
        nt, mult, nfs = cf.batched_plans(build(hub_libs, p))
        print(p[1:7], "targets", sorted(set(nt)), "largest multiplicity", max(mult), "nf", min(nfs), "..", max(nfs))
        assert max(nfs) == tokens  # the whole sent / red / plan areas of a wave's share are in use
        assert min(nt) >= 2 and max(nt) <= 1 + min(negative, sinks)
        if negative > 1:
            assert max(mult) > 1 and len(set(nt)) >= 3
        else:
            assert set(nt) == {2}
        if negative == 15:
            assert max(nt) > 8  # the second multiplicity word of the 16-row tile
        if oov:
            assert min(nfs) < tokens - 3
        # the raw draws: their own area for the 256-token case alone
        assert _own_negw(dim, window, negative, tokens) == (tokens == 256)
    # launches above 64 KB of LDS (the dynamic-LDS limit is raised first): the 256-token case, and the biggest tiles
    big = {q[:6] for q in CASES if _lds_bytes(q[0], q[1], q[2], q[5]) > 64 * 1024}
    assert big == {(64, 7, 15, 12, 8, 256), (256, 7, 15, 12, 32, cf.TOKENS)}
    assert _lds_bytes(256, 7, 15, cf.TOKENS) == 86880
    assert _lds_bytes(64, 7, 15, 256) == 102688  # 4000 + 2 * (3088 floats + 9248 ints) * 4: below the 160 KiB refusal
    assert max(_lds_bytes(q[0], q[1], q[2], q[5]) for q in CASES) <= 160 * 1024


def test_the_proof_notices_a_shared_word_in_a_batched_corpus(hub_libs):
    """one word of sentence 0 put into sentence 1: two sentences change its rows"""
    for hub in (0, cf.V_WORDS + 4):
        case = cf.batched_case(hub_libs.hub, 64, 5, 5, 4, hub_rows=hub)
        case.walks[1, 7] = case.walks[0, 3]
        with pytest.raises(AssertionError):
            cf.prove(case)
