"""The trainers' atomic-add row updates, bit for bit against restatements of the hub form.

In hogwild mode rows below hub_rows -- and every row leaving an LDS ring -- go back to memory as fp32
atomic adds instead of stores: the form the library runs by default (SgnsModel.hub_rows = None resolves
to auto_hub_rows).  Every such update is a short, fixed sequence of fp32 operations, so on ONE wave, and
on MANY waves where no two of them touch a row, the schedule cannot change its result and the kernels are
held to the exact bits of tests/cpu_sgns_hub/n2v_sgns_hub_cpu.c (default and batched skip-gram) and of
tests/cpu_cbow/n2v_cbow_cpu.c with hub_rows (CBOW): syn0, syn1neg and the pair count.

tests/test_hub_form_host.py proves, without a GPU and for every case run here, what makes that sound:
at hub_rows = 0 the restatements are the pinned store-form ones; at hub_rows > 0 they differ from those in
bits in both matrices (a kernel that stores where it should add, or the reverse, fails here); no atomic
add has a subnormal operand (a hardware atomic need not honour the denormal mode); a delta added twice,
fmaf for the rounded product, the boundary row taken as a hub and a lane that skips its adds each change
bits on these cases; and the many-wave corpora are conflict-free under the hub form (conflict_free.prove).

One wave (max_waves = 1, deterministic = False), the 40 x 21 corpora over 60 tokens of the existing bit
tests, two launches so that differences carry over.  Many waves: the library's own wave rule (at least 8
waves) on the conflict-free corpora of conflict_free.py with every row a hub and with a cut that splits
every sentence's words, three launches, one run each -- schedule independence is the argument of
conflict_free.py, proved for the hub form by the host test.

The batched trainer's hogwild mode on many waves is pinned by tests/test_batched_geometry_gpu.py (32 / 16 /
4 / 8 waves in blocks of two, hub_rows 0 / all / 513).  Its kernel writes EVERY target row of a position
back, the saturated sinks included, so "shared rows are never written" does not hold for it; what schedule
independence needs is weaker and does hold: a shared row is only ever rewritten with the bits it already
holds (a store of old + sum(0 * x), or an add of +0 + sum(0 * x), finite x, no -0 in the row:
tests/conflict_free.py, proved per case by tests/test_batched_geometry_host.py).
Real races (two waves on one row) stay a statistical claim.
"""
import numpy as np
import pytest
import torch

import conflict_free as cf
import hub_form_cases as hc
from same_bits import same_bits
from test_cbow_host import cbow_cpu  # noqa: F401  (session fixture behind hub_libs)
from test_hub_form_host import hub_libs  # noqa: F401  (session fixture: the restatements)

pytestmark = pytest.mark.gpu

MIN_WAVES = 8  # at least two blocks of 4 waves, as in test_train_geometry_gpu.py


def _model(vocab, n_vocab, dim, window, negative, seed, m0, m1, cum, sample_int, sg=1, cbow_mean=1):
    """a model on the GPU holding exactly the arrays the restatement starts from"""
    from node2vec_amd import _lib, sgns

    m = sgns.SgnsModel(vocab, dim, window, negative, seed=seed, sample=0.0, sg=sg, cbow_mean=cbow_mean)
    m.syn0.copy_(torch.from_numpy(m0))
    m.syn1neg.copy_(torch.from_numpy(m1))
    m.cum_table.copy_(torch.from_numpy(np.ascontiguousarray(cum).view(np.int32)))
    m.sample_int = None if sample_int is None else torch.from_numpy(sample_int).cuda()
    _lib.check(_lib.load().n2v_cum_index_build(m.cum_table.data_ptr(), n_vocab, m.cum_index_bits,
                                               m.cum_index.data_ptr(), _lib.current_stream_ptr()),
               "n2v_cum_index_build")
    return m


def _one_wave(libs, case):
    from node2vec_amd import sgns

    want0, want1, pairs = case.run(libs)
    v = case.vocab
    m = _model(sgns.Vocab(v.ids.cuda(), v.counts.cuda(), v.index_of.cuda()), case.n_vocab, case.dim, case.window,
               case.negative, case.seed, case.m0, case.m1, case.cum, case.sample_int,
               sg=0 if case.kind == "cbow" else 1, cbow_mean=case.cbow_mean)
    m.batched = case.kind == "batched"
    m.window_cache, m.hub_rows, m.max_waves = case.window_cache, case.hub_rows, 1
    idx = torch.from_numpy(case.walks).cuda()
    assert m.hogwild_waves(*idx.shape) == 1
    for base, alpha in case.launches:
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == pairs > 0, case.name
    same_bits(case.name + " syn0", m.syn0.cpu().numpy(), want0)
    same_bits(case.name + " syn1neg", m.syn1neg.cpu().numpy(), want1)


@pytest.mark.parametrize("dim,negative,sample,hub,window_cache", hc.SGNS_PARAMS)
def test_default_trainer_hub_form_on_one_wave(hub_libs, dim, negative, sample, hub, window_cache):
    """n2v_sgns.hip: negative targets, context rows and the centre row below hub_rows as atomic adds, rows at
    or above it as stores in the same position (hub_rows 7), the guarded tail lanes of dim 200, VEC 8 at
    512, the further target groups at negative 12, and the window cache's write-back add"""
    _one_wave(hub_libs, hc.sgns_case(dim, negative, sample, hub, window_cache))


@pytest.mark.parametrize("dim,window,negative,hub", hc.BATCHED_PARAMS)
def test_batched_trainer_hogwild_form_on_one_wave(hub_libs, dim, window, negative, hub):
    """n2v_sgns_batched.hip: every context row leaves the ring as an add of its delta (hub_rows 0 too), hub
    targets take their accumulated delta; both tile heights and both k-step counts over the ring"""
    _one_wave(hub_libs, hc.batched_case(dim, window, negative, hub))


@pytest.mark.parametrize("dim,window,cbow_mean,sample,hub", hc.cbow_params())
def test_cbow_hub_form_on_one_wave(hub_libs, dim, window, cbow_mean, sample, hub):
    """n2v_cbow.hip over the cases of test_cbow_gpu.BIT_CASES: beside test_hub_rows_on_one_wave, which
    bounds the distance from the STORE form, this asks for the hub form's bits"""
    _one_wave(hub_libs, hc.cbow_case(dim, window, cbow_mean, sample, hub))


def _many_waves(case, m):
    want0, want1, pairs = cf.prove(case)
    idx = torch.from_numpy(case.walks).cuda()
    waves = m.hogwild_waves(*idx.shape)
    print(case.name, "waves", waves)
    assert MIN_WAVES <= waves <= 32, waves
    for base, alpha in case.launches():
        m.train_block(idx, alpha, base, deterministic=False)
    torch.cuda.synchronize()
    assert int(m.pairs.item()) == pairs
    same_bits(case.name + " syn0", m.syn0.cpu().numpy(), want0)
    same_bits(case.name + " syn1neg", m.syn1neg.cpu().numpy(), want1)


def _identity_vocab(n):
    from node2vec_amd import sgns

    return sgns.Vocab(torch.arange(n).cuda(), torch.full((n,), 7, dtype=torch.int64).cuda(),
                      torch.arange(n, dtype=torch.int32).cuda())


@pytest.mark.parametrize("hub", hc.MANY_HUBS)
@pytest.mark.parametrize("dim", hc.MANY_DIMS)
def test_default_trainer_hub_form_on_many_waves(hub_libs, dim, hub):
    n = cf.V_WORDS + 1
    h = n if hub == hc.ALL else hub
    case = cf.sgns_case(hub_libs.oracle, dim, hub_rows=h, hub_cpu=hub_libs.hub)
    m = _model(_identity_vocab(n), n, dim, cf.WINDOW, cf.NEGATIVE, cf.SEED, case.m0, case.m1, cf.sgns_cum_table(), None)
    m.hub_rows = h
    _many_waves(case, m)


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("hub", hc.MANY_HUBS)
@pytest.mark.parametrize("dim", hc.MANY_DIMS)
def test_cbow_hub_form_on_many_waves(hub_libs, dim, hub, cbow_mean):
    n = cf.V_WORDS + 1
    h = n if hub == hc.ALL else hub
    case = cf.cbow_case(hub_libs.cbow, dim, cbow_mean=cbow_mean, hub_rows=h)
    m = _model(_identity_vocab(n), n, dim, cf.WINDOW, cf.NEGATIVE, cf.SEED, case.m0, case.m1, cf.sgns_cum_table(), None,
               sg=0, cbow_mean=cbow_mean)
    m.hub_rows = h
    _many_waves(case, m)
