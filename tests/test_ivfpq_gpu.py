"""Product-quantised codes for the inverted-file index on the GPU (csrc/n2v_ivfpq.hip through node2vec_amd.ann)
against the numpy restatement of its fixed order (tests/ivfpq_cases.py), bit for bit: rows with array_equal, scores
by their int32 bit patterns.  The table and scan tests use hand-made codebooks and codes, so nothing in them rests on
training; build_pq, the re-rank and the KeyedVectors interface come after."""
import numpy as np
import pytest
import torch

import ivf_cases as ic
import ivfpq_cases as pc
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _hand_index(ann, list_off, row_ids, codes, cb, dim, mlr=pc.HAND_MAX_LIST_ROWS, n=pc.HAND_N):
    nlist = len(list_off) - 1
    base = ann.IVFIndex(torch.zeros(nlist, dim, device="cuda"), torch.ones(nlist, device="cuda"), _dev(list_off),
                        _dev(row_ids), mlr, n, dim, 1)
    return ann.IVFPQIndex(base, _dev(cb), _dev(codes), cb.shape[0], cb.shape[2])


def _scan(ann, idx, Q, probes, coarse, k, X=None, inv=None, rows=None):
    """n2v_ivfpq_topk as it is: the caller's probes and first terms"""
    return _host(ann._pq_topk(idx, X, inv, None if Q is None else _dev(Q), rows, _dev(probes.astype(np.int32)),
                              _dev(coarse), k))


# ---- (a) the tables ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,m", pc.LUT_CASES)
def test_table_bits(oracle, dim, m):
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
    # the same tables for queries given as rows of a matrix
    X = rng.standard_normal((50, dim)).astype(np.float32)
    R = rng.integers(0, 50, 33)
    got = ann.pq_lut(_dev(cb), dim, rows=_dev(R), X=_dev(X)).cpu().numpy()
    assert np.array_equal(ic.bits(got), ic.bits(pc.lut_expect(pc.qhat(oracle, X[R]), cb, dim)))


# ---- (b), (c) the scan on hand-made lists -------------------------------------------------------------------------

def _hand_case(ann, rng, dim, m, k, long_kind, nq):
    t, chunk, chunks, _, stride = ann.plan_pq(pc.HAND_N, dim, m, ic.NLIST, pc.HAND_MAX_LIST_ROWS, nq, 1, k)
    assert (chunk, chunks) == (pc.HAND_CHUNK, 3) and stride == pc.code_stride(m)
    list_off, row_ids = pc.hand_lists(rng, ic.long_rows(long_kind, chunk))
    codes = pc.hand_codes(rng, len(row_ids), m)
    return t, list_off, row_ids, codes


@pytest.mark.parametrize("dim,m,k,long_kind,nq", pc.HAND_CASES)
def test_scan_exact_arithmetic(oracle, dim, m, k, long_kind, nq):
    """every score is exact in fp32 and heavily tied: indexing and selection, whatever the order of summation"""
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 1000 + 10 * m + k)
    t, list_off, row_ids, codes = _hand_case(ann, rng, dim, m, k, long_kind, nq)
    cb, Q, coarse = pc.exact_problem(rng, dim, m, nq, 4)
    idx = _hand_index(ann, list_off, row_ids, codes, cb, dim)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    assert np.array_equal(lut.astype(np.float64), pc.lut_float64(Q, cb, dim)[0])
    for name, probes in ic.probe_sets(rng, nq, t).items():
        c = np.ascontiguousarray(coarse[:, :probes.shape[1]])
        want = pc.scan_expect(lut, codes, list_off, row_ids, probes, c, k)
        ic.same(_scan(ann, idx, Q, probes, c, k), want, name)
        if name == "all on the long list" and k > 1:
            assert (np.diff(want[1], axis=1) == 0).any()  # tied scores: the original row decides


@pytest.mark.parametrize("dim,m,k,long_kind,nq", pc.HAND_CASES)
def test_scan_gaussian(oracle, dim, m, k, long_kind, nq):
    """Gaussian codebooks, queries and first terms: the chosen order of summation, bit for bit"""
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 1000 + 10 * m + k + 1)
    t, list_off, row_ids, codes = _hand_case(ann, rng, dim, m, k, long_kind, nq)
    cb, Q, coarse = pc.gaussian_problem(rng, dim, m, nq, 4)
    idx = _hand_index(ann, list_off, row_ids, codes, cb, dim)
    lut = pc.lut_expect(pc.qhat(oracle, Q), cb, dim)
    for name, probes in ic.probe_sets(rng, nq, t).items():
        c = coarse[:, :probes.shape[1]].copy()
        if name == "random":
            probes[3] = -1  # every slot unused: the tail alone
            probes[5] = [ic.LONG_LIST, 7, -1, -1]
            c[5, 0] = np.nan  # that probe contributes nothing
        want = pc.scan_expect(lut, codes, list_off, row_ids, probes, c, k)
        got = _scan(ann, idx, Q, probes, c, k)
        ic.same(got, want, name)
        if name == "random":
            assert (got[0][3] == -1).all() and (got[1][3] == -np.inf).all()
            assert np.isin(got[0][5][got[0][5] >= 0], row_ids[list_off[7]:list_off[8]]).all()
            assert not np.isnan(got[1]).any()
            # a query's result does not depend on the batch around it
            for batch in (slice(7, 8), slice(0, 16)):
                part = _scan(ann, idx, Q[batch], probes[batch], np.ascontiguousarray(c[batch]), k)
                at = 7 - batch.start
                assert np.array_equal(part[0][at], got[0][7])
                assert np.array_equal(ic.bits(part[1][at]), ic.bits(got[1][7]))


def test_scan_with_query_rows_and_identical_code_rows(oracle):
    """queries given as rows of X (the only use of X), and a list of identical code rows: every score ties and the
    rows come back in ascending original order whatever their positions"""
    from node2vec_amd import ann

    rng = np.random.default_rng(12)
    dim, m, k, nq = 24, 8, 20, 40
    t, list_off, row_ids, codes = _hand_case(ann, rng, dim, m, k, "c+1", nq)
    codes[list_off[7]:list_off[8], :m] = codes[0, :m]
    cb, _, coarse = pc.gaussian_problem(rng, dim, m, nq, 2)
    X = rng.standard_normal((pc.HAND_N, dim)).astype(np.float32)
    R = rng.integers(0, pc.HAND_N, nq)
    idx = _hand_index(ann, list_off, row_ids, codes, cb, dim)
    lut = pc.lut_expect(pc.qhat(oracle, X[R]), cb, dim)
    probes = np.tile(np.array([7, ic.LONG_LIST]), (nq, 1))
    want = pc.scan_expect(lut, codes, list_off, row_ids, probes, coarse, k)
    Xd = _dev(X)
    inv = _dev(oracle.knn_inv_norms(X))
    ic.same(_scan(ann, idx, None, probes, coarse, k, X=Xd, inv=inv, rows=_dev(R)), want, "rows")
    only7 = np.full((nq, 1), 7)
    r, s = _scan(ann, idx, None, only7, np.ascontiguousarray(coarse[:, :1]), k, X=Xd, inv=inv, rows=_dev(R))
    assert (r == np.sort(row_ids[list_off[7]:list_off[8]])[:k]).all() and (s == s[:, :1]).all()


def test_status_word_raises_and_the_run_ends_normally():
    from node2vec_amd import ann

    rng = np.random.default_rng(13)
    dim, m, k, nq = 16, 4, 5, 9
    _, list_off, row_ids, codes = _hand_case(ann, rng, dim, m, k, "c", nq)
    cb, Q, coarse = pc.gaussian_problem(rng, dim, m, nq, 2)
    idx = _hand_index(ann, list_off, row_ids, codes, cb, dim)
    probes = np.tile(np.array([ic.LONG_LIST, 3]), (nq, 1))
    good = _scan(ann, idx, Q, probes, coarse, k)
    idx.max_list_rows = pc.HAND_CHUNK - 1
    with pytest.raises(ValueError, match="max_list_rows"):
        _scan(ann, idx, Q, probes, coarse, k)
    idx.max_list_rows = pc.HAND_MAX_LIST_ROWS
    for bad in (ic.NLIST, -2):
        p = probes.copy()
        p[4, 1] = bad
        with pytest.raises(ValueError, match="probe"):
            _scan(ann, idx, Q, p, coarse, k)
    ids = row_ids.copy()
    ids[list_off[3]] = pc.HAND_N
    with pytest.raises(ValueError, match="row id"):
        _scan(ann, _hand_index(ann, list_off, ids, codes, cb, dim), Q, probes, coarse, k)
    again = _scan(ann, idx, Q, probes, coarse, k)  # the device is as it was
    ic.same(again, good, "after the refusals")


# ---- (d) encoding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,m", [(17, 4), (17, 16), (64, 4), (64, 16)])
def test_build_pq_encodes_every_listed_row_with_its_nearest_codeword(oracle, dim, m):
    from node2vec_amd import ann, cluster

    n, nlist = 2000, 8
    X = pc.mixture_rows(np.random.default_rng(dim + m), n, dim)
    X[11, 2] = np.nan  # k-means leaves it in no list: it has no code
    Xd = _dev(X)
    index = ann.build_index(Xd, nlist=nlist, seed=1, max_iter=10)
    kw = dict(seed=2, max_iter=8, init="random") if m == 16 else dict(seed=2, max_iter=8)
    pq = ann.build_pq(Xd, index, m, **kw)
    dsub = pc.dsub_of(dim, m)
    n_listed = n - 1
    assert isinstance(pq, ann.IVFIndex) and (pq.m, pq.dsub, pq.n, pq.dim, pq.nlist) == (m, dsub, n, dim, nlist)
    assert pq.codebooks.shape == (m, 256, dsub) and pq.codebooks.dtype == torch.float32
    assert pq.codes.shape == (n_listed, pc.code_stride(m)) and pq.codes.dtype == torch.uint8
    assert pq.row_ids is index.row_ids and pq.list_off is index.list_off and len(index.row_ids) == n_listed
    codes, cb = pq.codes.cpu().numpy(), pq.codebooks.cpu().numpy()
    assert (codes[:, m:] == 0).all()
    # two builds: identical bits
    again = ann.build_pq(Xd, index, m, **kw)
    assert torch.equal(again.codes, pq.codes) and torch.equal(again.codebooks.view(torch.int32),
                                                              pq.codebooks.view(torch.int32))
    # the rows of codes follow row_ids: position p is row row_ids[p], its residual against its own list's centroid
    row_ids, list_off = index.row_ids.cpu().numpy(), index.list_off.cpu().numpy()
    lists = np.searchsorted(list_off, np.arange(n_listed), side="right") - 1
    inv = oracle.knn_inv_norms(X)
    res = np.zeros((n_listed, m * dsub), np.float32)
    res[:, :dim] = X[row_ids] * inv[row_ids][:, None] - index.centroids.cpu().numpy()[lists]
    got_res = ann._residuals(Xd, _dev(inv), index, torch.arange(n_listed, device="cuda"), m * dsub)
    assert np.array_equal(ic.bits(got_res.cpu().numpy()), ic.bits(res))
    for j in range(m):
        for t in range(dsub):
            if j * dsub + t >= dim:
                assert (cb[j, :, t] == 0).all()  # the padding of the last sub-spaces stays zero
    dp = -(-dsub // 16) * 16
    err = 0.0
    for j in range(m):
        sub = res[:, j * dsub:(j + 1) * dsub]
        # the codes are cluster.assign's labels on the same sub-matrix
        labels, _ = cluster.assign(_dev(sub), pq.codebooks[j], "euclidean")
        assert np.array_equal(labels.cpu().numpy(), codes[:, j].astype(np.int32)), j
        # and the chosen codeword is the nearest in float64, up to the rounding of the fp32 distance
        # t(c) = fmaf(-2, dot(c, r), |c|^2): the dot is a chain of dp fmas (error <= dp u |c||r|, doubled), |c|^2 a
        # sum of at most ceil(dsub / 64) fmas and 6 adds (<= (dp + 7) u |c|^2), the last fma u |t|; with u = 2^-24
        # that is within 2^-23 (dp + 8) (|c|^2 + 2 |c||r|) / 2, the other half covers the second-order terms
        w = cb[j].astype(np.float64)
        r64 = sub.astype(np.float64)
        d = ((r64[:, None, :] - w[None]) ** 2).sum(axis=2)
        cn, rn = np.sqrt((w ** 2).sum(axis=1)), np.sqrt((r64 ** 2).sum(axis=1))
        slack = 2.0 ** -23 * (dp + 8) * (cn[None, :] ** 2 + 2 * cn[None, :] * rn[:, None])
        best = d.argmin(axis=1)
        at = np.arange(n_listed)
        chosen = codes[:, j]
        assert (d[at, chosen] <= d[at, best] + slack[at, chosen] + slack[at, best]).all(), j
        err += d[at, chosen].sum()
    # the codes say something: the mean squared quantisation error is below the mean squared residual norm (a
    # float64 numpy PQ on the same seeded data leaves under 1 % of it, so the margin is wide)
    assert err / n_listed < (res.astype(np.float64) ** 2).sum() / n_listed


def test_build_pq_with_fewer_than_256_training_rows():
    """spare codewords are copies of used ones; a copy never wins a tie, so every code names the lowest of its
    equals"""
    from node2vec_amd import ann

    rng = np.random.default_rng(14)
    X = rng.standard_normal((100, 8)).astype(np.float32)
    Xd = _dev(X)
    index = ann.build_index(Xd, nlist=2, seed=0, max_iter=5)
    pq = ann.build_pq(Xd, index, 2, seed=1, max_iter=4)
    cb, codes = pq.codebooks.cpu().numpy(), pq.codes.cpu().numpy()
    for j in range(2):
        distinct = np.unique(cb[j], axis=0)
        assert len(distinct) <= 100
        for c in np.unique(codes[:, j]):
            same = np.nonzero((cb[j] == cb[j][c]).all(axis=1))[0]
            assert c == same[0]
    r, s = ann.search_pq(pq, 5, queries=_dev(X[:7]), nprobe=2)
    assert (r[:, 0].cpu().numpy() == np.arange(7)).all()  # 100 rows, 256 codewords: a row's code is the row


# ---- (e) the re-rank --------------------------------------------------------------------------------------------

def test_refine_rescored_results(oracle):
    from node2vec_amd import ann

    rng = np.random.default_rng(15)
    n, dim, nlist, k = 250, 32, 8, 5
    X = rng.standard_normal((n, dim)).astype(np.float32)  # no clusters: lists of about n / nlist rows
    Xd = _dev(X)
    pq = ann.build_pq(Xd, ann.build_index(Xd, nlist=nlist, seed=3, max_iter=10), 8, seed=4, max_iter=5)
    assert 2 * pq.max_list_rows <= 128  # two probed lists fit into the re-rank's 128 candidates
    Q = rng.standard_normal((30, dim)).astype(np.float32)
    R = rng.integers(0, n, 30)
    Qd, Rd = _dev(Q), _dev(R)
    probes = ann.probe(pq, queries=Qd, nprobe=2)
    # every probed row is rescored: IVF-flat's result, rows and score bits
    ic.same(_host(ann.search_pq(pq, k, queries=Qd, X=Xd, probes=probes, refine=26)),
            _host(ann.search(Xd, pq, k, queries=Qd, probes=probes)), "queries, given probes")
    ic.same(_host(ann.search_pq(pq, k, queries=Qd, X=Xd, nprobe=2, refine=26)),
            _host(ann.search(Xd, pq, k, queries=Qd, nprobe=2)), "queries")
    ic.same(_host(ann.search_pq(pq, k, rows=Rd, X=Xd, nprobe=2, refine=26)),
            _host(ann.search(Xd, pq, k, rows=Rd, nprobe=2)), "rows")
    ic.same(_host(ann.search_pq(pq, k, rows=Rd, X=Xd, nprobe=2, refine=22, exclude_self=True)),
            _host(ann.search(Xd, pq, k, rows=Rd, nprobe=2, exclude_self=True)), "exclude_self")
    # any refine: exact scores, ordered, out of the approximate top refine * k
    exact = oracle.knn_scores(X, queries=Q)
    for f in (1, 2, 4):
        r, s = _host(ann.search_pq(pq, k, queries=Qd, X=Xd, nprobe=2, refine=f))
        approx, _ = _host(ann.search_pq(pq, f * k, queries=Qd, nprobe=2))
        for q in range(len(Q)):
            assert (r[q] >= 0).all()
            assert np.array_equal(ic.bits(s[q]), ic.bits(exact[q, r[q]]))
            keys = list(zip(-s[q], r[q]))
            assert keys == sorted(keys) and set(r[q]) <= set(approx[q])
            # the best k of those candidates by the exact score
            cand = approx[q][approx[q] >= 0]
            order = np.lexsort((cand, -exact[q, cand]))[:k]
            assert np.array_equal(r[q], cand[order])
    r0, _ = _host(ann.search_pq(pq, k, rows=Rd, X=Xd, nprobe=2, exclude_self=True))
    r4, _ = _host(ann.search_pq(pq, k, rows=Rd, X=Xd, nprobe=2, refine=4, exclude_self=True))
    assert not (r0 == R[:, None]).any() and not (r4 == R[:, None]).any()
    with pytest.raises(ValueError, match="needs X"):
        ann.search_pq(pq, k, queries=Qd, refine=2)
    # the approximate scores: the probe's centroid score plus the tables, as the restatement sums them
    r, s = _host(ann.search_pq(pq, k, queries=Qd, probes=probes))
    from node2vec_amd import similarity

    coarse = torch.gather(similarity.scores(pq.centroids, queries=Qd, inv_norm=pq.centroid_inv_norm), 1,
                          probes.long()).cpu().numpy()
    lut = pc.lut_expect(pc.qhat(oracle, Q), pq.codebooks.cpu().numpy(), dim)
    want = pc.scan_expect(lut, pq.codes.cpu().numpy(), pq.list_off.cpu().numpy(), pq.row_ids.cpu().numpy(),
                          probes.cpu().numpy(), coarse, k)
    ic.same((r, s), want, "approximate scores")
    ic.same(_host(ann.search_pq(pq, k, queries=Qd, nprobe=2)), want, "the probe's own centroid scores")


def test_search_pq_splits_a_batch_to_fit_the_workspace(monkeypatch):
    from node2vec_amd import ann, similarity

    rng = np.random.default_rng(16)
    n, dim = 1500, 16
    Xd = _dev(pc.mixture_rows(rng, n, dim))
    pq = ann.build_pq(Xd, ann.build_index(Xd, nlist=6, seed=1, max_iter=5), 4, seed=1, max_iter=4)
    Qd = _dev(rng.standard_normal((300, dim)).astype(np.float32))
    whole = ann.search_pq(pq, 10, queries=Qd, nprobe=3)
    need = ann._lib.load().n2v_ivfpq_workspace_bytes(n, dim, 4, 6, pq.max_list_rows, 40, 3, 10)
    monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", int(need))
    parts = ann.search_pq(pq, 10, queries=Qd, nprobe=3)
    ic.same(_host(parts), _host(whole), "split")


# ---- (f) the API ------------------------------------------------------------------------------------------------

def test_keyed_vectors_with_a_pq_index():
    from node2vec_amd import ann
    from node2vec_amd.embedding import KeyedVectors

    rng = np.random.default_rng(17)
    n, dim = 3000, 16
    ids = rng.permutation(n).astype(np.int64) + 100
    Xd = _dev(pc.mixture_rows(rng, n, dim, centres=100, noise=0.3))
    kv = KeyedVectors(ids, Xd)
    idx = kv.build_index(nlist=12, seed=2, max_iter=5, pq=8)
    assert isinstance(idx, ann.IVFPQIndex) and (idx.m, idx.nlist, idx.nprobe, idx.refine) == (8, 12, 8, 4)
    token, row = str(int(ids[40])), 40
    for refine in (4, 0):
        idx.refine = refine
        hits = kv.most_similar(token, topn=7, indexer=idx)
        q = torch.from_numpy(kv._query([token], None)[0]).cuda()
        r, s = _host(ann.search_pq(idx, 8, queries=q, X=Xd, refine=refine, inv_norm=kv._inv_norm))
        want = [(str(int(ids[a])), float(b)) for a, b in zip(r[0], s[0]) if a >= 0 and a != row][:7]
        assert hits == want and len(hits) == 7
        assert kv.similar_by_word(token, topn=7, indexer=idx) == hits
        rows = torch.arange(0, 200, device="cuda")
        a = kv.nearest(rows, 6, indexer=idx)
        b = ann.search_pq(idx, 6, rows=rows, X=Xd, refine=refine, inv_norm=kv._inv_norm, exclude_self=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert not (a[0] == rows[:, None]).any()
    idx.refine = 4
    exact = dict(kv.most_similar(token, topn=n))
    assert all(exact[t] == s for t, s in kv.most_similar(token, topn=7, indexer=idx))  # re-ranked: true cosines
    # an IVFIndex handed over the same way is searched as before
    flat = kv.build_index(nlist=12, seed=2, max_iter=5)
    assert type(flat) is ann.IVFIndex
    q = torch.from_numpy(kv._query([token], None)[0]).cuda()
    r, s = _host(ann.search(Xd, flat, 8, queries=q, inv_norm=kv._inv_norm))
    want = [(str(int(ids[a])), float(b)) for a, b in zip(r[0], s[0]) if a >= 0 and a != row][:7]
    assert kv.most_similar(token, topn=7, indexer=flat) == want
    a, b = kv.nearest(rows, 6, indexer=flat), ann.search(Xd, flat, 6, rows=rows, inv_norm=kv._inv_norm,
                                                         exclude_self=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    with pytest.raises(ValueError):
        kv.nearest(rows, 128, indexer=idx)
