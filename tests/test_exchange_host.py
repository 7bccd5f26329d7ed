"""The host form of the replica exchange (the CPU branches of sgns.DeltaSync and shard._rank_ordered_reduce:
what gloo runs on host tensors) against tests/exchange_restatement.py, bit for bit, over the world sizes,
shapes and values that tests/test_exchange_edges_gpu.py holds the HIP passes to.  No GPU needed: these
define what the kernels are compared with."""
import numpy as np
import pytest
import torch

import exchange_cases as X
import exchange_restatement as R


def _sync(world, wire, like):
    from node2vec_amd.sgns import DeltaSync

    s = DeltaSync([like], wire=wire, overlap=False)
    s.active, s.world = True, world
    return s


# -- the restatement itself ----------------------------------------------------------------------------------

def test_restated_bf16_rounding_on_known_values():
    f = lambda *w: np.array(w, dtype=np.uint32).view(np.float32)
    got = R.f32_to_bf16(f(0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF,
                          0x00008000, 0x00018000, 0x00000001, 0x80000000, 0x7F800000, 0x3FFF8000))
    assert got.tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF82, 0x7F80, 0xFF80,
                            0x0000, 0x0002, 0x0000, 0x8000, 0x7F80, 0x4000]
    nan = R.f32_to_bf16(f(0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0xFF80FFFF))
    assert R.is_nan16(nan).all()
    back = R.bf16_to_f32(np.array([0x3F80, 0xC040, 0x0001, 0x7F80], dtype=np.uint16))
    assert back.view(np.uint32).tolist() == [0x3F800000, 0xC0400000, 0x00010000, 0x7F800000]
    # every bf16 value survives the round trip (NaNs as NaNs)
    every = np.arange(1 << 16, dtype=np.uint16)
    R.assert_same_bits(R.f32_to_bf16(R.bf16_to_f32(every)), every, "bf16 round trip")


def test_restated_bf16_rounding_is_the_nearest_with_ties_to_even():
    """against exact arithmetic: the two bf16 neighbours of x in float64, the nearer wins, the even one on a tie"""
    v = R.special_values()
    v = v[np.isfinite(v)]
    got = R.f32_to_bf16(v)
    lo = (v.view(np.uint32) >> 16).astype(np.uint16)  # truncation: the neighbour towards zero
    hi = (lo + 1).astype(np.uint16)                   # the next one away from zero (may be inf: 2^128 in float64)
    x = v.astype(np.float64)
    with np.errstate(all="ignore"):
        a = R.bf16_to_f32(lo).astype(np.float64)
        b = R.bf16_to_f32(hi).astype(np.float64)
    b = np.where(np.isinf(b), np.sign(x) * 2.0 ** 128, b)
    da, db = np.abs(x - a), np.abs(b - x)
    want = np.where(da < db, lo, np.where(db < da, hi, np.where(lo & 1, hi, lo))).astype(np.uint16)
    assert np.array_equal(got, want)


def test_mean_by_division_and_by_reciprocal_differ_off_powers_of_two():
    """why world 2 cannot pin the mean: x / w and x * (1 / w) are the same operation only for w = 1, 2, 4, 8"""
    x = np.random.default_rng(0).standard_normal(100000).astype(np.float32)
    for w in X.WORLDS + (4,):
        differ = int((x / np.float32(w) != x * (np.float32(1) / np.float32(w))).sum())
        assert (differ == 0) == (w in (1, 2, 4, 8)), (w, differ)


# -- the single passes on CPU tensors -------------------------------------------------------------------------

@pytest.mark.parametrize("world", X.WORLDS)
def test_host_passes_equal_the_restatement_on_special_values(world):
    from node2vec_amd.shard import _rank_ordered_reduce

    curs, ref, mids = R.edge_case(world)
    n = curs[0].size
    # ref_init
    s = _sync(world, "bf16", X.f32_tensor(curs[0]).view(n, 1))
    for c in curs[:2]:
        R.assert_same_bits(X.bf16_bits(s._ref_init(X.f32_tensor(c))), R.ref_init(c), "ref_init")
    for wire in ("fp32", "bf16"):
        s = _sync(world, wire, X.f32_tensor(curs[0]).view(n, 1))
        wdt = torch.float32 if wire == "fp32" else torch.bfloat16
        to_np = X.f32_array if wire == "fp32" else X.bf16_bits
        wires = []
        for r in range(world):  # pack, with and without a snapshot
            for snap in (False, True):
                cur, before, w = X.f32_tensor(curs[r]), torch.full((n,), 7.0), torch.zeros(n, dtype=wdt)
                s._pack(cur, X.bf16_tensor(ref) if wire == "bf16" else None, before if snap else None, w)
                want_w, want_b = R.pack(curs[r], ref if wire == "bf16" else None, snap)
                R.assert_same_bits(to_np(w), want_w, f"pack {wire} rank {r}")
                R.assert_same_bits(X.f32_array(before), want_b if snap else np.full(n, 7.0, np.float32), "snapshot")
                R.assert_same_bits(X.f32_array(cur), curs[r], "pack left cur alone")
            wires.append(want_w)
        # the rank-ordered sum
        total = R.rank_sum(wires)
        parts = (X.f32_tensor if wire == "fp32" else X.bf16_tensor)(np.concatenate(wires))
        got = _rank_ordered_reduce(parts, world, n, torch.empty(n, dtype=wdt))
        R.assert_same_bits(to_np(got), total, f"sum {wire}")
        # apply, set form and add form
        for add in (False, True):
            cur = X.f32_tensor(mids[0] if add else curs[0])
            rf = X.bf16_tensor(ref) if wire == "bf16" else None
            summed = (X.f32_tensor if wire == "fp32" else X.bf16_tensor)(total)
            s._apply(cur, rf, X.f32_tensor(curs[0]) if add else None, summed)
            want_c, want_r = R.apply(mids[0] if add else curs[0], ref if wire == "bf16" else None,
                                     curs[0] if add else None, total, world)
            R.assert_same_bits(X.f32_array(cur), want_c, f"apply {wire} add={add}")
            if wire == "bf16":
                R.assert_same_bits(X.bf16_bits(rf), want_r, f"apply {wire} add={add}: reference")


@pytest.mark.parametrize("world", X.WORLDS)
def test_host_apply_equals_the_restatement_on_every_bf16_sum(world):
    """all 65 536 bf16 bit patterns as the summed wire, against references that run through them at another pace"""
    total = np.arange(1 << 16, dtype=np.uint16)
    ref = (total * np.uint16(40503) + np.uint16(world)).astype(np.uint16)  # a permutation of the patterns
    n = total.size
    s = _sync(world, "bf16", torch.zeros(n, 1))
    cur, rf = torch.zeros(n), X.bf16_tensor(ref)
    s._apply(cur, rf, None, X.bf16_tensor(total))
    want_c, want_r = R.apply(np.zeros(n, np.float32), ref, None, total, world)
    R.assert_same_bits(X.f32_array(cur), want_c, "apply")
    R.assert_same_bits(X.bf16_bits(rf), want_r, "reference")


# -- whole exchanges through DeltaSync._exchange ----------------------------------------------------------------

@pytest.mark.parametrize("exact", [True, False], ids=["set", "add"])
@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", X.WORLDS)
def test_host_exchange_equals_the_restatement(world, wire, exact):
    for case, block_rows in ((X.random_case(world, [(33, 5)], 11), 2),
                             (X.random_case(world, [(37, 7), (5, 3)], 12), 256),
                             (X.special_case(world), 97)):
        bad, _, _ = X.check_exchange("cpu", world, wire, case, block_rows, exact)
        assert bad == 0, (world, wire, exact, block_rows, bad)


@pytest.mark.parametrize("exact", [True, False], ids=["set", "add"])
@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", [2, 3])
def test_host_exchange_in_blocks_off_16_bytes(world, wire, exact):
    """(1000, 7) in blocks of 3 rows: 334 blocks, their bases at multiples of 84 bytes"""
    case = X.random_case(world, [(1000, 7)], 13)
    bad, _, _ = X.check_exchange("cpu", world, wire, case, 3, exact, ranks=(0, world - 1))
    assert bad == 0, (world, wire, exact, bad)


def test_replicas_end_identical_after_a_blocking_exchange():
    for world in (3, 7):
        for wire in ("fp32", "bf16"):
            _, got, _ = X.check_exchange("cpu", world, wire, X.random_case(world, [(33, 5)], 14), 2, True)
            for r in range(1, world):
                R.assert_same_bits(got[r][0][0], got[0][0][0], "replicas")
