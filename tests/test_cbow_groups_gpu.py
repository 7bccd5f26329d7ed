"""The CBOW kernel's groups of target rows, groups of context rows and batches of negative draws, bit for
bit against the CPU restatement in deterministic mode (node2vec_amd/csrc/n2v_cbow.hip).

The kernel takes the 1 + negative targets of a position kTG at a time (6 for VEC 1, 2 and 4; 3 for
VEC 8; 2 for VEC 16): the first group is requested before the context rows are summed, further groups
run in a loop of their own, a first group with fewer than kTG targets and a last group with fewer are
padded with "nothing to train", and a target equal to an earlier one must see that one's stored update
-- inside a group by a second load, across groups because the group is loaded after the stores of the
one before.  It sums and updates the context rows kCG at a time with the same care for a repeated word,
and draws the negatives of 64 / negative positions at once.  test_cbow_gpu.py tries all of that at
negative = 5 (and once at 20, dim 32); here `negative` stands on every edge of the grouping for every
VEC, and the batches of draws at their extremes.

Every case first asserts from the integer replay tests/cbow_groups.py (held to the restatement's own
counters by test_cbow_host.py) that it reaches what it is there for; a case that does not is wrongly
built and fails before anything runs on the GPU.  No tolerance: bits and an integer count.
"""
import numpy as np
import pytest
import torch

import cbow_groups
from test_cbow_gpu import _case, _check_bits
from test_cbow_host import cbow_cpu  # noqa: F401  (the session fixture that builds the restatement)

pytestmark = pytest.mark.gpu

# VEC 1; VEC 2 full (agent-scope loads); VEC 4 ragged and full; VEC 8; VEC 16 ragged and full
GROUP_DIMS = [48, 128, 200, 256, 512, 1000, 1024]


def _negatives(ktg):
    """`negative` on the edges of groups of ktg targets (1 + negative targets per position): one target
    short of a full first group and two short, exactly one group, one short of two groups and exactly
    two (ktg, 2 ktg - 1: a further group of one target, and a full one), and the draw batches of 3
    positions with one idle lane (21) and of 2 positions with none (32)"""
    return sorted(k for k in {1, ktg - 2, ktg - 1, ktg, 2 * ktg - 1, 2 * ktg, 21, 32} if k >= 1)


# (dim, negative, window, cbow_mean, sample): window and subsampling rotate over the cases as in
# test_cbow_gpu.BIT_CASES
GROUP_CASES = [(dim, k, (5, 1, 32)[j % 3], mean, (0.0, 1e-2)[(j + mean) % 2])
               for j, (dim, k) in enumerate((dim, k) for dim in GROUP_DIMS
                                            for k in _negatives(cbow_groups.KTG[cbow_groups.vec_of(dim)]))
               for mean in (0, 1)]


def test_group_cases_cover_what_they_claim():
    assert {c[2] for c in GROUP_CASES} == {1, 5, 32} and {c[4] for c in GROUP_CASES} == {0.0, 1e-2}
    assert {cbow_groups.vec_of(d) for d in GROUP_DIMS} == {1, 2, 4, 8, 16}
    assert _negatives(6) == [1, 4, 5, 6, 11, 12, 21, 32] and _negatives(3) == [1, 2, 3, 5, 6, 21, 32]
    assert _negatives(2) == [1, 2, 3, 4, 21, 32]
    for dim in GROUP_DIMS:
        ktg = cbow_groups.KTG[cbow_groups.vec_of(dim)]
        for mean in (0, 1):
            mine = [c for c in GROUP_CASES if c[0] == dim and c[3] == mean]
            assert [c[1] for c in mine] == _negatives(ktg)
            assert len({c[2] for c in mine}) == 3 and len({c[4] for c in mine}) == 2


def _nonzero_outputs(m):
    """syn1neg starts at zero, and then a pass this short with one or two negatives moves syn0 by less than
    the 1e-4 that _check_bits asks of a case: start from outputs of size 0.05, as
    test_cbow_gpu.test_offsets_past_2_31_elements does.  f matters from the first position on"""
    gen = torch.Generator(device="cuda").manual_seed(m.seed)
    m.syn1neg.copy_(0.05 * torch.randn(m.syn1neg.shape, generator=gen, device="cuda"))


def _replay(m, idx, bases):
    vec = cbow_groups.vec_of(m.dim)
    return cbow_groups.replay(idx.cpu().numpy(), m.cum_table.cpu().numpy().view(np.uint32),
                              None if m.sample_int is None else m.sample_int.cpu().numpy().view(np.uint32),
                              len(m.vocab), m.seed, bases, m.window, m.negative, cbow_groups.KTG[vec],
                              cbow_groups.KCG[vec])


def group_claims(negative, ktg, rep):
    """what a (kTG, negative) case must reach, asserted from the replay alone"""
    assert rep["positions"] > 0
    assert rep["centre_draws"] > 0, "no draw equals its centre word"
    # the centre word and a draw never repeat each other (such a draw is skipped): a group needs two draws
    if negative >= (2 if ktg >= 3 else 3):
        assert rep["dup_in_group"] > 0, "no target repeats one of its own group"
    else:
        assert rep["dup_in_group"] == 0
    if negative >= ktg:
        assert rep["dup_across_groups"] > 0, "no target repeats one of an earlier group"
    else:
        assert rep["dup_across_groups"] == 0
    assert rep["padded_last_group"] == (rep["positions"] if (1 + negative) % ktg else 0)


@pytest.mark.parametrize("dim,negative,window,cbow_mean,sample", GROUP_CASES)
def test_negative_on_the_edges_of_the_target_groups(cbow_cpu, dim, negative, window, cbow_mean, sample):
    sgns, m, idx = _case(60, 12, 21, dim, window, negative, seed=5 + dim, sample=sample, cbow_mean=cbow_mean)
    rows = idx.shape[0]
    bases = (0, rows)
    _nonzero_outputs(m)
    rep = _replay(m, idx, bases)
    print(dim, negative, window, cbow_mean, sample, rep)
    group_claims(negative, cbow_groups.KTG[cbow_groups.vec_of(dim)], rep)
    n = _check_bits(cbow_cpu, m, idx, ((bases[0], 0.025), (bases[1], 0.02)))
    assert n == rep["positions"]


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("dim", [64, 300])
def test_one_negative_and_a_second_batch_of_draws(cbow_cpu, dim, cbow_mean):
    """negative = 1: 64 positions per batch of draws, so only a sentence of more than 64 kept tokens
    draws a second time"""
    sgns, m, idx = _case(60, 3, 150, dim, 5, 1, seed=5 + dim, sample=0.0, cbow_mean=cbow_mean)
    bases = (0, idx.shape[0])
    _nonzero_outputs(m)
    rep = _replay(m, idx, bases)
    print(dim, cbow_mean, rep)
    assert rep["max_kept"] > 64 and rep["max_position"] >= 64 and rep["centre_draws"] > 0
    assert _check_bits(cbow_cpu, m, idx, ((bases[0], 0.025), (bases[1], 0.02))) == rep["positions"]


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("negative", [22, 31])
def test_two_positions_per_batch_with_idle_lanes(cbow_cpu, negative, cbow_mean):
    """negative 22 .. 31: batches of 2 positions, lanes 2 * negative .. 63 idle; positions of both
    parities train, so both halves of a batch are read"""
    dim = 128
    sgns, m, idx = _case(60, 12, 21, dim, 5, negative, seed=5 + dim, sample=0.0, cbow_mean=cbow_mean)
    bases = (0, idx.shape[0])
    _nonzero_outputs(m)
    rep = _replay(m, idx, bases)
    print(negative, cbow_mean, rep)
    assert 64 // negative == 2 and 2 * negative < 64
    assert rep["odd_positions"] > 0 and rep["even_positions"] > 0
    group_claims(negative, cbow_groups.KTG[cbow_groups.vec_of(dim)], rep)
    assert _check_bits(cbow_cpu, m, idx, ((bases[0], 0.025), (bases[1], 0.02))) == rep["positions"]


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("dim", [48, 256, 1024])
def test_context_groups_at_window_32(cbow_cpu, dim, cbow_mean):
    """windows of more than 16 context rows: more than two groups of kCG even at VEC 1 (kCG 8), with a
    word repeated inside a group and across groups (VEC 16, kCG 1: across only)"""
    sgns, m, idx = _case(60, 6, 40, dim, 32, 5, seed=5 + dim, sample=0.0, cbow_mean=cbow_mean)
    bases = (0, idx.shape[0])
    _nonzero_outputs(m)
    rep = _replay(m, idx, bases)
    print(dim, cbow_mean, rep)
    kcg = cbow_groups.KCG[cbow_groups.vec_of(dim)]
    assert rep["max_count"] > 16 and rep["max_count"] > 2 * kcg
    assert rep["ctx_dup_across_groups"] > 0
    assert (rep["ctx_dup_in_group"] > 0) == (kcg > 1)
    assert _check_bits(cbow_cpu, m, idx, ((bases[0], 0.025), (bases[1], 0.02))) == rep["positions"]
