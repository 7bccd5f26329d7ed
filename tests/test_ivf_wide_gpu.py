"""The launch geometry of the two inverted-file scans on the GPU (csrc/n2v_ivf.hip, csrc/n2v_ivfpq.hip, their
n2v_ivf_group.h and n2v_topk_select.h) on the cases of tests/ivf_wide_cases.py: up to 1024 lists with long runs of
empty ones, 1 .. 1024 probes a query, 1 .. 3072 slots for the merge, chunks of 128 and 256 rows and lists that end
chunks before max_list_rows, code rows that m does not fill, and a list that a query names twice.

The reference is the restatement the hand-made tests already use (ivf_cases.expect, ivfpq_cases.scan_expect and
lut_expect), unchanged.  Everything goes through ann._topk / ann._pq_topk with the caller's probes; rows are compared
with array_equal and scores by their int32 bit patterns (ivf_cases.same).  There is no tolerance anywhere.  The plan
values the cases rely on (tile, chunk, chunks, code stride) are asserted in tests/test_ivf_wide_host.py."""
import numpy as np
import pytest
import torch

import ivf_cases as ic
import ivf_wide_cases as wc
import ivfpq_cases as pc
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)

pytestmark = pytest.mark.gpu

WIDE_K = 10
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(a, aligned=True):
    """a float32 numpy array on the device; aligned=False: its base 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if aligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _probes(p):
    return _dev(np.asarray(p).astype(np.int32))


def _flat_index(ann, idx, dim):
    return ann.IVFIndex(torch.zeros(idx.nlist, dim, device="cuda"), torch.ones(idx.nlist, device="cuda"),
                        _dev(idx.list_off), _dev(idx.row_ids), idx.max_list_rows, idx.n, dim, 1)


def _pq_index(ann, idx, codes, cb, dim):
    return ann.IVFPQIndex(_flat_index(ann, idx, dim), _dev(cb), _dev(codes), cb.shape[0], cb.shape[2])


def _flat(ann, Xd, inv, index, Q, probes, k):
    """n2v_ivf_topk as it is: the caller's probes"""
    return _host(ann._topk(Xd, inv, index, _dev(Q), None, _probes(probes), k))


def _pq(ann, index, Q, probes, coarse, k):
    """n2v_ivfpq_topk as it is: the caller's probes and first terms"""
    return _host(ann._pq_topk(index, None, None, _dev(Q), None, _probes(probes), _dev(coarse), k))


def _flat_problem(seed, n, dim, nq):
    """mixed rows (hub copies: ties; zero rows) and Gaussian queries, one of them zero and one a row of X"""
    rng = np.random.default_rng(seed)
    X = ic.mixed_rows(rng, n, dim)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q[1], Q[2] = 0.0, X[n // 2]
    return X, Q


class _FlatSide:
    """X on the device beside one index, and the search through ann._topk"""

    def __init__(self, ann, idx, X, aligned=True):
        from node2vec_amd import similarity

        self.ann, self.X = ann, X
        self.Xd = _device(X, aligned)
        self.inv = similarity.inv_norms(self.Xd)
        self.index = _flat_index(ann, idx, X.shape[1])

    def search(self, Q, probes, k):
        return _flat(self.ann, self.Xd, self.inv, self.index, Q, probes, k)


# ---- 1. wide indexes: many lists, many probes, runs of empty lists ----------------------------------------------------

def _wide_flat_want(oracle, nlist, dim):
    """name -> (probes, expected result) of every table, computed once for the aligned and the unaligned run"""
    key = ("flat", nlist, dim)
    if key not in _cache:
        idx = wc.wide_index(nlist)
        X, Q = _flat_problem(8000 + nlist + dim, idx.n, dim, wc.MAX_NQ)
        want = {name: (p, ic.expect(oracle, X, idx.lists, p, WIDE_K, queries=Q[:len(p)]))
                for name, p in wc.wide_probes(idx).items()}
        _cache[key] = idx, X, Q, want
    return _cache[key]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dim", [17, 64])
@pytest.mark.parametrize("nlist", wc.WIDE_NLISTS)
def test_wide_index_flat(oracle, nlist, dim, aligned):
    from node2vec_amd import ann

    idx, X, Q, want = _wide_flat_want(oracle, nlist, dim)
    side = _FlatSide(ann, idx, X, aligned)
    for name, (p, expected) in want.items():
        ic.same(side.search(Q[:len(p)], p, WIDE_K), expected, name)
        assert (expected[0] >= 0).any(), name  # (the table finds something)
    if nlist > 2:
        r, _ = want["one empty run and the long list"][1]
        assert np.isin(r, idx.lists[idx.long_list]).all()  # nothing but the long list's rows


def _wide_pq_problem(oracle, nlist, m, dim=24):
    idx = wc.wide_index(nlist)
    rng = np.random.default_rng(8100 + nlist + m)
    cb, Q, _ = pc.gaussian_problem(rng, dim, m, wc.MAX_NQ, 1)
    codes = pc.hand_codes(rng, len(idx.row_ids), m)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    return idx, rng, cb, Q, codes, lut


@pytest.mark.parametrize("m", [4, 12])
@pytest.mark.parametrize("nlist", wc.WIDE_NLISTS)
def test_wide_index_pq(oracle, nlist, m):
    from node2vec_amd import ann

    idx, rng, cb, Q, codes, lut = _wide_pq_problem(oracle, nlist, m)
    index = _pq_index(ann, idx, codes, cb, 24)
    for name, p in wc.wide_probes(idx).items():
        nq = len(p)
        coarse = rng.standard_normal(p.shape).astype(np.float32)
        expected = pc.scan_expect(lut[:nq], codes, idx.list_off, idx.row_ids, p, coarse, WIDE_K)
        ic.same(_pq(ann, index, Q[:nq], p, coarse, WIDE_K), expected, name)
        assert (expected[0] >= 0).any(), name


def test_a_query_alone_and_in_a_batch_of_1024_lists(oracle):
    """257 queries x 64 probes are more than 16 x 1024 pairs (the 64-wide tile of the flat scan), one of them alone
    is not (the 16-wide one): the same bits from both, and from the PQ scan"""
    from node2vec_amd import ann

    idx, X, Q, want = _wide_flat_want(oracle, 1024, 64)
    p, expected = want["just above the narrow tile"]
    assert p.shape == (257, 64)
    side = _FlatSide(ann, idx, X)
    batch = side.search(Q[:257], p, WIDE_K)
    ic.same(batch, expected, "the batch")
    for q in (0, 3, 256):
        alone = side.search(Q[q:q + 1], p[q:q + 1], WIDE_K)
        assert (alone[0] >= 0).any()
        ic.same(alone, (batch[0][q:q + 1], batch[1][q:q + 1]), f"flat, query {q}")
    idx, rng, cb, Q, codes, _ = _wide_pq_problem(oracle, 1024, 12)
    index = _pq_index(ann, idx, codes, cb, 24)
    coarse = rng.standard_normal(p.shape).astype(np.float32)
    batch = _pq(ann, index, Q[:257], p, coarse, WIDE_K)
    for q in (0, 3, 256):
        alone = _pq(ann, index, Q[q:q + 1], p[q:q + 1], coarse[q:q + 1], WIDE_K)
        assert (alone[0] >= 0).any()
        ic.same(alone, (batch[0][q:q + 1], batch[1][q:q + 1]), f"pq, query {q}")


# ---- 2. the merge at other slot counts --------------------------------------------------------------------------------

def _slot_flat(chunks):
    key = ("slot flat", chunks)
    if key not in _cache:
        idx = wc.slot_index(wc.FLAT, chunks)
        _cache[key] = (idx,) + _flat_problem(8200 + chunks, idx.n, 16, wc.SLOT_NQ)
    return _cache[key]


@pytest.mark.parametrize("k", wc.SLOT_KS)
@pytest.mark.parametrize("nprobe,chunks", wc.SLOT_CASES)
def test_slot_counts_flat(oracle, nprobe, chunks, k):
    from node2vec_amd import ann

    idx, X, Q = _slot_flat(chunks)
    p = wc.slot_probes(np.random.default_rng(100 * nprobe + chunks + k), nprobe)
    expected = ic.expect(oracle, X, idx.lists, p, k, queries=Q)
    ic.same(_FlatSide(ann, idx, X).search(Q, p, k), expected, f"{nprobe} x {chunks} slots")
    if k == 128 and nprobe * chunks > 1:
        assert ((expected[0] >= 0).sum(axis=1) == k).any()  # full results that more than one slot fed


@pytest.mark.parametrize("k", wc.SLOT_KS)
@pytest.mark.parametrize("nprobe,chunks", wc.SLOT_CASES)
def test_slot_counts_pq(oracle, nprobe, chunks, k):
    """exact arithmetic, heavily tied: the merge orders equal scores from different slots by original row"""
    from node2vec_amd import ann

    idx = wc.slot_index(wc.PQ, chunks)
    rng = np.random.default_rng(8300 + 100 * nprobe + chunks + k)
    dim, m = 16, 4
    cb, Q, coarse = pc.exact_problem(rng, dim, m, wc.SLOT_NQ, nprobe)
    codes = pc.hand_codes(rng, len(idx.row_ids), m)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    p = wc.slot_probes(rng, nprobe)
    expected = pc.scan_expect(lut, codes, idx.list_off, idx.row_ids, p, coarse, k)
    ic.same(_pq(ann, _pq_index(ann, idx, codes, cb, dim), Q, p, coarse, k), expected, f"{nprobe} x {chunks} slots")
    if k == 128:
        assert (expected[1][::2, 0] == expected[1][::2, 1]).any()  # tied scores at the very top


# ---- 3. the chunk plan away from three chunks ---------------------------------------------------------------------------

def _small_cases(scan):
    return [wc.small_index(mlr) for mlr in wc.SMALL_CHUNKS] + [wc.sparse_index(scan)]


@pytest.mark.parametrize("case", range(5))
def test_small_chunks_flat(oracle, case):
    from node2vec_amd import ann

    idx = _small_cases(wc.FLAT)[case]
    X, Q = _flat_problem(8400 + case, idx.n, 16, 30)
    side = _FlatSide(ann, idx, X)
    for k in (1, 10, 128):
        for name, p in wc.small_probes().items():
            ic.same(side.search(Q, p, k), ic.expect(oracle, X, idx.lists, p, k, queries=Q),
                    f"max_list_rows {idx.max_list_rows}, k {k}, {name}")


@pytest.mark.parametrize("case", range(5))
def test_small_chunks_pq(oracle, case):
    from node2vec_amd import ann

    idx = _small_cases(wc.PQ)[case]
    rng = np.random.default_rng(8500 + case)
    dim, m = 16, 4
    codes = pc.hand_codes(rng, len(idx.row_ids), m)
    for k, problem in ((1, pc.gaussian_problem), (10, pc.exact_problem), (128, pc.gaussian_problem)):
        cb, Q, coarse = problem(rng, dim, m, 30, 3)
        index = _pq_index(ann, idx, codes, cb, dim)
        lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
        for name, p in wc.small_probes().items():
            c = np.ascontiguousarray(coarse[:, :p.shape[1]])
            ic.same(_pq(ann, index, Q, p, c, k), pc.scan_expect(lut, codes, idx.list_off, idx.row_ids, p, c, k),
                    f"max_list_rows {idx.max_list_rows}, k {k}, {name}")


# ---- 4. code rows that m does not fill -------------------------------------------------------------------------------

def _ragged_case(rng, m, long_kind):
    list_off, row_ids = pc.hand_lists(rng, ic.long_rows(long_kind, pc.HAND_CHUNK))
    return list_off, row_ids, pc.hand_codes(rng, len(row_ids), m)  # the bytes past m are random


def _hand_pq_index(ann, list_off, row_ids, codes, cb, dim):
    nlist = len(list_off) - 1
    base = ann.IVFIndex(torch.zeros(nlist, dim, device="cuda"), torch.ones(nlist, device="cuda"), _dev(list_off),
                        _dev(row_ids), pc.HAND_MAX_LIST_ROWS, pc.HAND_N, dim, 1)
    return ann.IVFPQIndex(base, _dev(cb), _dev(codes), cb.shape[0], cb.shape[2])


@pytest.mark.parametrize("dim,m,k,long_kind,nq", wc.RAGGED_CASES)
def test_ragged_m_exact_arithmetic(oracle, dim, m, k, long_kind, nq):
    """every score is exact in fp32 and heavily tied: indexing and selection, whatever the order of summation"""
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 1000 + 10 * m + k)
    list_off, row_ids, codes = _ragged_case(rng, m, long_kind)
    cb, Q, coarse = pc.exact_problem(rng, dim, m, nq, 4)
    index = _hand_pq_index(ann, list_off, row_ids, codes, cb, dim)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    assert np.array_equal(lut.astype(np.float64), pc.lut_float64(Q, cb, dim)[0])
    for name, probes in ic.probe_sets(rng, nq, wc.tile_pairs(m)).items():
        c = np.ascontiguousarray(coarse[:, :probes.shape[1]])
        want = pc.scan_expect(lut, codes, list_off, row_ids, probes, c, k)
        ic.same(_pq(ann, index, Q, probes, c, k), want, name)
        if name == "all on the long list" and k > 1:
            assert (np.diff(want[1], axis=1) == 0).any()  # tied scores: the original row decides


@pytest.mark.parametrize("dim,m,k,long_kind,nq", wc.RAGGED_CASES)
def test_ragged_m_gaussian(oracle, dim, m, k, long_kind, nq):
    """Gaussian codebooks, queries and first terms: the chosen order of summation, bit for bit"""
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 1000 + 10 * m + k + 1)
    list_off, row_ids, codes = _ragged_case(rng, m, long_kind)
    cb, Q, coarse = pc.gaussian_problem(rng, dim, m, nq, 4)
    index = _hand_pq_index(ann, list_off, row_ids, codes, cb, dim)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    for name, probes in ic.probe_sets(rng, nq, wc.tile_pairs(m)).items():
        c = np.ascontiguousarray(coarse[:, :probes.shape[1]])
        ic.same(_pq(ann, index, Q, probes, c, k), pc.scan_expect(lut, codes, list_off, row_ids, probes, c, k), name)


@pytest.mark.parametrize("dim,m", [(dim, m) for dim, m, *_ in wc.RAGGED_CASES])
def test_ragged_m_table_bits(oracle, dim, m):
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 100 + m)
    cb, Q, _ = pc.gaussian_problem(rng, dim, m, 33, 1)
    Q[4] = 0.0
    Q[9, dim // 2] = np.nan
    want = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    got = ann.pq_lut(_dev(cb), dim, queries=_dev(Q)).cpu().numpy()
    assert got.shape == want.shape == (33, m, 256)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan[9].any() and not nan[:9].any() and not nan[10:].any()
    assert np.array_equal(ic.bits(got)[~nan], ic.bits(want)[~nan])  # (a NaN's payload is not part of the contract)
    assert (got[4] == 0).all()
    dsub = pc.dsub_of(dim, m)
    for j in range(m):
        if j * dsub >= dim:
            assert (got[:9, j] == 0).all() and not np.signbit(got[:9, j]).any()  # a sub-space past dim: +0


# ---- 5. a list that a query names twice is refused ---------------------------------------------------------------------

def _raw(ann, call, sizes, extra, Qd, Pd, k, bytes_fn):
    """the C entry point itself: (its return value, the status word, rows, scores); every buffer is a live
    allocation of the documented size until the stream is idle"""
    nq, nprobe = Pd.shape
    ws = torch.empty(max(int(bytes_fn(*sizes, nq, nprobe, k)), 16), dtype=torch.uint8, device="cuda")
    out_r = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
    out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = call(Qd.data_ptr(), None, nq, Pd.data_ptr(), *extra, nprobe, k, out_r.data_ptr(), out_s.data_ptr(),
              status.data_ptr(), ws.data_ptr(), ws.numel(), ann._lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, int(status), out_r.cpu().numpy(), out_s.cpu().numpy()


def _duplicate_index(where):
    return wc.slot_index(wc.FLAT, 1) if where == "slots" else wc.wide_index(1024)


@pytest.mark.parametrize("table", range(3))
def test_a_repeated_probe_is_refused_flat(oracle, table):
    from node2vec_amd import _lib, ann

    name, where, p, bad, fixed = wc.duplicate_tables()[table]
    idx = _duplicate_index(where)
    dim, k = 16, 20
    X, Q = _flat_problem(8600 + table, idx.n, dim, len(p))
    side = _FlatSide(ann, idx, X)
    valid = p.copy()
    valid[bad] = fixed  # the repeat taken out: what the device must make of the row
    good = side.search(Q, valid, k)
    ic.same(good, ic.expect(oracle, X, idx.lists, valid, k, queries=Q), "the valid table")
    with pytest.raises(ValueError, match="probe"):
        side.search(Q, p, k)
    L = _lib.load()
    Qd, Pd = _dev(Q), _probes(p)
    index = side.index
    sizes = (idx.n, dim, idx.nlist, idx.max_list_rows)

    def call(*tail):
        return L.n2v_ivf_topk(side.Xd.data_ptr(), side.inv.data_ptr(), idx.n, dim, index.list_off.data_ptr(),
                              index.row_ids.data_ptr(), idx.nlist, idx.max_list_rows, *tail)

    rc, status, r, s = _raw(ann, call, sizes, (), Qd, Pd, k, L.n2v_ivf_workspace_bytes)
    assert rc == _lib.OK and status & _lib.ST_RANGE, name
    ic.same((r, s), good, "the repeat is skipped like a probe out of range")
    rc, status, r, s = _raw(ann, call, sizes, (), Qd, _probes(valid), k, L.n2v_ivf_workspace_bytes)
    assert rc == _lib.OK and status == 0
    ic.same((r, s), good, "the entry point on the valid table")
    ic.same(side.search(Q, valid, k), good, "after the refusal")  # the device is as it was


@pytest.mark.parametrize("table", range(3))
def test_a_repeated_probe_is_refused_pq(oracle, table):
    from node2vec_amd import _lib, ann

    name, where, p, bad, fixed = wc.duplicate_tables()[table]
    idx = _duplicate_index(where)
    dim, m, k = 16, 12, 20
    rng = np.random.default_rng(8700 + table)
    cb, Q, coarse = pc.gaussian_problem(rng, dim, m, len(p), p.shape[1])
    codes = pc.hand_codes(rng, len(idx.row_ids), m)
    index = _pq_index(ann, idx, codes, cb, dim)
    valid = p.copy()
    valid[bad] = fixed
    good = _pq(ann, index, Q, valid, coarse, k)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    ic.same(good, pc.scan_expect(lut, codes, idx.list_off, idx.row_ids, valid, coarse, k), "the valid table")
    with pytest.raises(ValueError, match="probe"):
        _pq(ann, index, Q, p, coarse, k)
    L = _lib.load()
    Qd, Pd, Cd = _dev(Q), _probes(p), _dev(coarse)
    sizes = (idx.n, dim, m, idx.nlist, idx.max_list_rows)

    def call(q, qr, nq, probes, *tail):
        return L.n2v_ivfpq_topk(index.codes.data_ptr(), index.codebooks.data_ptr(), m, None, None, idx.n, dim,
                                index.list_off.data_ptr(), index.row_ids.data_ptr(), idx.nlist, idx.max_list_rows,
                                q, qr, nq, probes, *tail)

    rc, status, r, s = _raw(ann, call, sizes, (Cd.data_ptr(),), Qd, Pd, k, L.n2v_ivfpq_workspace_bytes)
    assert rc == _lib.OK and status & _lib.ST_RANGE, name
    ic.same((r, s), good, "the repeat is skipped like a probe out of range")
    rc, status, r, s = _raw(ann, call, sizes, (Cd.data_ptr(),), Qd, _probes(valid), k, L.n2v_ivfpq_workspace_bytes)
    assert rc == _lib.OK and status == 0
    ic.same((r, s), good, "the entry point on the valid table")
    ic.same(_pq(ann, index, Q, valid, coarse, k), good, "after the refusal")  # the device is as it was
