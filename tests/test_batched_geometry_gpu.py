"""The batched skip-gram trainer's hogwild launch on many waves, bit for bit (n2v_sgns_batched.hip,
SgnsModel.batched = True).

On one wave the kernel is pinned twice (test_sgns_batched_gpu.py: the store form against its oracle;
test_hub_form_gpu.py: the hogwild form against the hub restatement).  One wave is one block and
wave_in_block == 0.  What only exists on more waves is run here: the per-wave LDS carve-up
(mine = smem + exp + wave_in_block * (per_wave_floats + per_wave_ints) * 4) and its agreement with the
launcher's per_wave expression, each with its own term for the raw draws' area; blocks of two waves and
blockIdx > 0; the shared row counter; the occupancy cap of the launch; and the launch above 64 KB of LDS
with two waves in it.

The corpora are conflict_free.batched_case: sentences over disjoint words, every negative one of a few
saturated sinks.  This kernel writes every target row of a position back, the sinks included -- but with
the bits they hold (G is the literal 0.0f there), so any schedule computes what the hub restatement
computes in order: the argument of tests/conflict_free.py, whose premises tests/test_batched_geometry_host.py
proves for every case run here.  Three launches with deterministic=False, then the pair count and the bits
of syn0 and syn1neg must equal the joint run of conflict_free.prove.  One run each: the argument does not
depend on the schedule.  The wave count is asked of the library (SgnsModel.hogwild_waves) and asserted.

Real races (two waves on one row) stay a statistical claim (test_sgns_batched_gpu.py).
"""
import pytest
import torch

from same_bits import same_bits
from test_batched_geometry_host import CASES, IDS, _hub, proved
from test_cbow_host import cbow_cpu  # noqa: F401  (session fixture behind hub_libs)
from test_hub_form_gpu import _identity_vocab, _model
from test_hub_form_host import hub_libs  # noqa: F401  (session fixture: the restatements)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_batched_hogwild_bit_identical_on_conflict_free_corpus(hub_libs, p):
    """32 x 40 tokens under the library's rule: 32 waves in 16 blocks of 2, both tile heights and ring
    sizes, hub_rows 0 / all / 513.  64 sentences with -1 tokens on 16 waves: a wave takes about four through
    the counter, and the ring and plan of one sentence must not leak into the next.  max_waves = 3: rounded
    up to two blocks of two.  8 x 256 tokens at 15 negatives: the raw draws in their own area, 100 KB of LDS
    per block (the dynamic-LDS limit raised first), 8 waves."""
    import conflict_free as cf

    dim, window, negative, sinks, sentences, tokens, oov, _, max_waves, waves = p
    case, want0, want1, pairs = proved(hub_libs, p)
    n = cf.V_WORDS + sinks
    m = _model(_identity_vocab(n), n, dim, window, negative, cf.SEED, case.m0, case.m1, case.extra["cum"], None)
    m.batched, m.hub_rows, m.max_waves = True, _hub(p), max_waves
    idx = torch.from_numpy(case.walks).cuda()
    got = m.hogwild_waves(*idx.shape)
    print(case.name, "waves", got)
    assert got == waves
    for base, alpha in case.launches():
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == pairs
    same_bits(case.name + " syn0", m.syn0.cpu().numpy(), want0)
    same_bits(case.name + " syn1neg", m.syn1neg.cpu().numpy(), want1)
