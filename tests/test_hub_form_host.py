"""The hub-form restatements, with no GPU: tests/cpu_sgns_hub/n2v_sgns_hub_cpu.c (the default and the
batched skip-gram trainer) and the hub_rows argument of tests/cpu_cbow/n2v_cbow_cpu.c state what the
kernels compute in hogwild mode, where rows below hub_rows -- and every row leaving an LDS ring -- go
back as fp32 atomic adds.  tests/test_hub_form_gpu.py holds the kernels to their bits; this file proves,
on every case that test takes to the GPU (hub_form_cases.py), that the comparison means something:

  * with hub_rows = 0 (and stores for the batched ring) each restatement equals the pinned one bit for
    bit: oracle.sgns_train, oracle.sgns_train(batched=True), the CBOW restatement's store form;
  * with hub_rows > 0 (or the window cache) it differs in bits from that store-form twin in both matrices,
    so a kernel that stores where it should add, or adds where it should store, fails the GPU test; the
    largest |difference| per case is printed;
  * no atomic add of any case has a nonzero subnormal addend, memory operand or result (a hardware fp32
    atomic need not honour the denormal mode: bit equality with a CPU addition is only claimed where that
    cannot matter);
  * seeded mutations of the restatement -- the centre delta added twice, fmaf for the rounded product,
    row hub_rows treated as a hub, the last lane of a ragged row skipping its adds -- each change bits on
    GPU cases: what a subtly wrong kernel would show;
  * the many-wave corpora are conflict-free under the hub restatement (conflict_free.prove).
"""
import types

import numpy as np
import pytest

import conflict_free as cf
import hub_form_cases as hc
from test_cbow_host import cbow_cpu  # noqa: F401  (session fixture: the CBOW restatement)


@pytest.fixture(scope="session")
def hub_libs(tmp_path_factory, oracle, cbow_cpu):
    """the restatements: .hub / .cbow as the GPU test uses them, .hub_checked / .cbow_checked with the
    subnormal-operand counter compiled in, .oracle"""
    return types.SimpleNamespace(hub=hc.load_hub(tmp_path_factory.mktemp("hub_cpu")),
                                 hub_checked=hc.load_hub(tmp_path_factory.mktemp("hub_cpu_checked"), checked=True),
                                 cbow=cbow_cpu,
                                 cbow_checked=hc.load_cbow_checked(tmp_path_factory.mktemp("cbow_cpu_checked")),
                                 oracle=oracle)


def _bits(a):
    return a.view(np.uint32)


def _equal(a, b):
    return a[2] == b[2] and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _checked(libs, case, **kw):
    """the case under the instrumented build: (result, subnormal operands)"""
    libs.hub_checked.n2v_sgns_hub_cpu_subnormals()
    libs.cbow_checked.n2v_cbow_cpu_subnormals()
    out = case.run(libs, hub=libs.hub_checked, cbow=libs.cbow_checked, **kw)
    return out, libs.hub_checked.n2v_sgns_hub_cpu_subnormals() + libs.cbow_checked.n2v_cbow_cpu_subnormals()


def _check_case(libs, case):
    """what every one-wave GPU case must satisfy; returns the hub form's result"""
    store = case.run(libs, store_form=True)
    assert store[2] > 0 and np.abs(store[1]).max() > 0
    # hub_rows = 0: the new code states what the pinned restatement states
    if case.kind == "batched":
        zero = (case.m0.copy(), case.m1.copy(), 0)
        for base, alpha in case.launches:
            zero = zero[:2] + (zero[2] + hc.hub_batched_train(
                libs.hub, case.walks, zero[0], zero[1], case.cum, case.sample_int, case.n_vocab, base, case.seed,
                case.dim, case.window, case.negative, alpha, 0, ctx_store=1),)
    elif case.kind == "sgns":
        saved, case.window_cache = case.window_cache, 0
        zero = case.run(libs, hub_rows=0)
        case.window_cache = saved
    else:
        zero = store  # CBOW: hub_rows = 0 IS the pinned restatement
    assert _equal(zero, store), f"{case.name}: the hub restatement at hub_rows = 0 is not the pinned restatement"
    # the case's own form: same pairs, other bits in both matrices, no subnormal operand
    hub, subnormals = _checked(libs, case)
    assert _equal(hub, case.run(libs)), "the instrumented build computes something else"
    assert subnormals == 0, f"{case.name}: {subnormals} subnormal operands of atomic adds"
    assert hub[2] == store[2]
    d0, d1 = float(np.abs(hub[0] - store[0]).max()), float(np.abs(hub[1] - store[1]).max())
    n0, n1 = int((_bits(hub[0]) != _bits(store[0])).sum()), int((_bits(hub[1]) != _bits(store[1])).sum())
    print(f"{case.name}: hub form vs store form: syn0 {n0} elements, max |diff| {d0:.3e}; syn1neg {n1} elements, "
          f"max |diff| {d1:.3e}")
    assert n0 > 0 and n1 > 0, f"{case.name}: the hub form and the store form agree: the case cannot tell them apart"
    return hub


@pytest.mark.parametrize("dim,negative,sample,hub,window_cache", hc.SGNS_PARAMS)
def test_default_trainer_cases(hub_libs, dim, negative, sample, hub, window_cache):
    case = hc.sgns_case(dim, negative, sample, hub, window_cache)
    if window_cache and case.hub_rows == 0:
        # only the ring's write-back adds: hub_rows = 0 with the cache must still differ from the stores
        assert case.window == 5
    _check_case(hub_libs, case)
    if case.hub_rows == 7:
        # rows 6 (the last hub) and 7 (the first plain row) both take every role in this case
        roles = np.zeros((3, case.n_vocab), np.int64)
        case.run(hub_libs, roles=roles)
        assert roles[:, 6].min() > 0 and roles[:, 7].min() > 0, roles[:, 6:8].tolist()


@pytest.mark.parametrize("dim,window,negative,hub", hc.BATCHED_PARAMS)
def test_batched_trainer_cases(hub_libs, dim, window, negative, hub):
    """hub_rows = 0 included: every context row leaves the ring as an atomic add of its delta"""
    _check_case(hub_libs, hc.batched_case(dim, window, negative, hub))


@pytest.mark.parametrize("dim,window,cbow_mean,sample,hub", hc.cbow_params())
def test_cbow_cases(hub_libs, dim, window, cbow_mean, sample, hub):
    _check_case(hub_libs, hc.cbow_case(dim, window, cbow_mean, sample, hub))


def _assert_detected(libs, cases, mutation, expected):
    """the mutated restatement differs in bits from the true one on the `expected` cases and on no other.  A
    row of fewer than 16 elements may hide a mutation that only moves a rounding (at dim 1 a single element's
    two roundings can coincide with the one): there it may go unnoticed, everywhere else it must not."""
    got = {c.name for c in cases if not _equal(c.run(libs, mutation=mutation), c.run(libs))}
    assert got <= {c.name for c in expected}, sorted(got - {c.name for c in expected})
    must = {c.name for c in expected if c.dim >= 16}
    assert must and must <= got, sorted(must - got)


def test_every_seeded_mutation_changes_bits(hub_libs):
    """one wrong kernel per branch, stated as a mutation of the restatement: each must differ in bits on the
    GPU cases that exercise its branch, and on those alone"""
    sgns = [hc.sgns_case(*p) for p in hc.SGNS_PARAMS]
    cbow = [hc.cbow_case(*p) for p in hc.cbow_params()]
    batched = [hc.batched_case(*p) for p in hc.BATCHED_PARAMS]
    hubbed = [c for c in sgns if c.hub_rows > 0]
    # the centre delta added twice: every case with a hub row
    _assert_detected(hub_libs, sgns, hc.MUT_CENTRE_TWICE, hubbed)
    # fmaf for the rounded product, in both trainers that have the branch
    _assert_detected(hub_libs, sgns, hc.MUT_NEG_FMA, hubbed)
    _assert_detected(hub_libs, cbow, hc.MUT_NEG_FMA, cbow)
    # the boundary: only where a row hub_rows exists (hub_rows < n_vocab), and there in every trainer
    for cases in (sgns, cbow, batched):
        _assert_detected(hub_libs, cases, hc.MUT_BOUNDARY, [c for c in cases if c.hub_rows < c.n_vocab])
    # the last lane of a ragged row: dim 200 of the default trainer, every ragged dim of CBOW
    _assert_detected(hub_libs, sgns, hc.MUT_LAST_LANE, [c for c in hubbed if c.dim == 200])
    _assert_detected(hub_libs, cbow, hc.MUT_LAST_LANE, [c for c in cbow if c.dim not in (64, 128, 256, 512, 1024)])


def _split_by(case, cut):
    """every sentence has words on both sides of `cut`"""
    return all((w[w >= 0] < cut).any() and (w[w >= 0] >= cut).any() for w in case.walks)


@pytest.mark.parametrize("hub", hc.MANY_HUBS)
@pytest.mark.parametrize("dim", hc.MANY_DIMS)
def test_many_wave_sgns_corpus_is_conflict_free_under_the_hub_form(hub_libs, dim, hub):
    h = cf.V_WORDS + 1 if hub == hc.ALL else hub
    case = cf.sgns_case(hub_libs.oracle, dim, hub_rows=h, hub_cpu=hub_libs.hub)
    assert _split_by(case, h) == (hub != hc.ALL)
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() >= 1.0  # f >= 8 at the sink throughout
    # other bits than the store form, in both matrices; no subnormal operand
    s0, s1, n = cf.prove(cf.sgns_case(hub_libs.oracle, dim))
    assert n == pairs and (_bits(s0) != _bits(j0)).any() and (_bits(s1) != _bits(j1)).any()
    hub_libs.hub_checked.n2v_sgns_hub_cpu_subnormals()
    c0, c1 = case.m0.copy(), case.m1.copy()
    for base, alpha in case.launches():
        hc.hub_sgns_train(hub_libs.hub_checked, case.walks, c0, c1, cf.sgns_cum_table(), None, cf.V_WORDS + 1, base,
                          cf.SEED, dim, cf.WINDOW, cf.NEGATIVE, alpha, h)
    assert hub_libs.hub_checked.n2v_sgns_hub_cpu_subnormals() == 0
    assert np.array_equal(_bits(c0), _bits(j0)) and np.array_equal(_bits(c1), _bits(j1))
    print(case.name, "pairs", pairs, "max |hub - store|", float(np.abs(s0 - j0).max()), float(np.abs(s1 - j1).max()))


@pytest.mark.parametrize("cbow_mean", [0, 1])
@pytest.mark.parametrize("hub", hc.MANY_HUBS)
@pytest.mark.parametrize("dim", hc.MANY_DIMS)
def test_many_wave_cbow_corpus_is_conflict_free_under_the_hub_form(hub_libs, dim, hub, cbow_mean):
    h = cf.V_WORDS + 1 if hub == hc.ALL else hub
    case = cf.cbow_case(hub_libs.cbow, dim, cbow_mean=cbow_mean, hub_rows=h)
    assert _split_by(case, h) == (hub != hc.ALL)
    j0, j1, pairs = cf.prove(case)
    assert j0[:, 0].min() >= 1.0
    # CBOW's context add is the store's value in order: the forms differ in syn1neg, and through it in syn0
    s0, s1, n = cf.prove(cf.cbow_case(hub_libs.cbow, dim, cbow_mean=cbow_mean))
    assert n == pairs and (_bits(s0) != _bits(j0)).any() and (_bits(s1) != _bits(j1)).any()
    checked = cf.cbow_case(hub_libs.cbow_checked, dim, cbow_mean=cbow_mean, hub_rows=h)
    hub_libs.cbow_checked.n2v_cbow_cpu_subnormals()
    c0, c1 = checked.m0.copy(), checked.m1.copy()
    for base, alpha in checked.launches():
        checked.run(checked.walks, c0, c1, base, alpha)
    assert hub_libs.cbow_checked.n2v_cbow_cpu_subnormals() == 0
    assert np.array_equal(_bits(c0), _bits(j0)) and np.array_equal(_bits(c1), _bits(j1))
    print(case.name, "positions", pairs, "max |hub - store|", float(np.abs(s0 - j0).max()), float(np.abs(s1 - j1).max()))


def test_the_proof_notices_a_shared_word_under_the_hub_form(hub_libs):
    """one word of sentence 0 put into sentence 1: two sentences add to its rows"""
    n = cf.V_WORDS + 1
    for case in (cf.sgns_case(hub_libs.oracle, 64, hub_rows=n, hub_cpu=hub_libs.hub),
                 cf.cbow_case(hub_libs.cbow, 64, hub_rows=n)):
        case.walks[1, 7] = case.walks[0, 3]
        with pytest.raises(AssertionError):
            cf.prove(case)
