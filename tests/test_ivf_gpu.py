"""The inverted-file index on the GPU (csrc/n2v_ivf.hip through node2vec_amd.ann) against its restatement
(tests/ivf_cases.py, numpy around oracle/n2v_oracle_knn.c) and against similarity.knn, bit for bit: rows with
array_equal, scores by their int32 bit patterns.  What is approximate about the index is which lists a query probes;
every score and the selection among the probed rows are exact, so every comparison here is an equality."""
import numpy as np
import pytest
import torch

import ivf_cases as ic
from conftest import ROOT  # noqa: F401  (puts the repository and oracle/ on sys.path)

pytestmark = pytest.mark.gpu


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


def _same_as_knn(got, want, what):
    ic.same(_host(got), _host(want), what)


def _random_index(ann, Xd, rng, nlist, lowest=-1, **kw):
    labels = rng.integers(lowest, nlist, Xd.shape[0])
    C = torch.from_numpy(rng.standard_normal((nlist, Xd.shape[1])).astype(np.float32)).cuda()
    return ann.from_labels(Xd, C, torch.from_numpy(labels).cuda(), **kw), labels


# ---- 1. every list probed: the exact result ----------------------------------------------------------------------

@pytest.mark.parametrize("n,dim,nlist,k", [(3000, 32, 20, 10), (2500, 129, 7, 127), (700, 1024, 5, 10)])
def test_every_list_probed_equals_knn(n, dim, nlist, k):
    from node2vec_amd import ann, similarity

    rng = np.random.default_rng(n + dim)
    X = ic.mixed_rows(rng, n, dim)
    Xd = _device(X)
    Q = _device(rng.standard_normal((65, dim)))
    R = torch.from_numpy(rng.integers(0, n, 100)).cuda()
    built = ann.build_index(Xd, nlist=nlist, seed=3, max_iter=5)
    hand, _ = _random_index(ann, Xd, rng, nlist, lowest=0)
    for name, idx in (("build_index", built), ("from_labels", hand)):
        assert int(idx.list_off[-1]) == n  # every row is in a list
        _same_as_knn(ann.search(Xd, idx, k, queries=Q, nprobe=nlist), similarity.knn(Xd, k, queries=Q), name)
        _same_as_knn(ann.search(Xd, idx, k, rows=R, nprobe=nlist), similarity.knn(Xd, k, rows=R), name)
        _same_as_knn(ann.search(Xd, idx, k, rows=R, nprobe=nlist, exclude_self=True),
                     similarity.knn(Xd, k, rows=R, exclude_self=True), name)


# ---- 2. hand-made lists against the restatement -------------------------------------------------------------------

@pytest.mark.parametrize("dim,k,long_kind,nq,aligned", ic.HAND_CASES)
def test_hand_made_lists(oracle, dim, k, long_kind, nq, aligned):
    from node2vec_amd import ann

    rng = np.random.default_rng(dim * 1000 + k + nq)
    mlr = ic.HAND_MAX_LIST_ROWS
    long_len = ic.long_rows(long_kind, 1792)
    labels = ic.hand_labels(rng, long_len)
    n = len(labels)
    qt, chunk_rows, chunks = ann.plan(n, dim, ic.NLIST, mlr, nq, 1, k)
    assert (chunk_rows, chunks) == (1792, 3) and qt == (64 if nq == 200 else 16) and mlr <= n <= 6000
    X = ic.mixed_rows(rng, n, dim)
    Xd = _device(X, aligned)
    C = torch.from_numpy(rng.standard_normal((ic.NLIST, dim)).astype(np.float32)).cuda()
    idx = ann.from_labels(Xd, C, torch.from_numpy(labels).cuda())
    assert idx.max_list_rows == long_len
    counts = (idx.list_off[1:] - idx.list_off[:-1]).tolist()
    assert counts == list(ic.SMALL_LISTS) + [long_len]
    idx.max_list_rows = mlr  # an upper bound is enough: the long list now ends at the edge of a chunk the plan fixes
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q[0], Q[1] = 0.0, X[n // 2]
    R = rng.integers(0, n, nq)
    Qd, Rd = _device(Q), torch.from_numpy(R).cuda()
    for name, probes in ic.probe_sets(rng, nq, qt).items():
        Pd = torch.from_numpy(probes).cuda()
        ic.same(_host(ann.search(Xd, idx, k, queries=Qd, probes=Pd)),
                ic.expect(oracle, X, labels, probes, k, queries=Q), f"{name}, queries")
        ic.same(_host(ann.search(Xd, idx, k, rows=Rd, probes=Pd)),
                ic.expect(oracle, X, labels, probes, k, rows=R), f"{name}, rows")
    if k < 128:
        probes = ic.probe_sets(rng, nq, qt)["random"]
        got = ann.search(Xd, idx, k, rows=Rd, probes=torch.from_numpy(probes).cuda(), exclude_self=True)
        want = ic.expect(oracle, X, labels, probes, k + 1, rows=R)  # ask for k + 1, drop the own row or the last
        wr, ws = want
        out_r, out_s = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
        for q in range(nq):
            keep = np.nonzero(wr[q] != R[q])[0][:k]
            out_r[q], out_s[q] = wr[q][keep], ws[q][keep]
        ic.same(_host(got), (out_r, out_s), "exclude_self")


def test_three_chunks_of_the_long_list(oracle):
    """the long list fills max_list_rows: three full chunks, every query on it, k above a chunk's share"""
    from node2vec_amd import ann

    rng = np.random.default_rng(5)
    dim, k, nq = 24, 100, 80
    labels = ic.hand_labels(rng, ic.HAND_MAX_LIST_ROWS)
    n = len(labels)
    assert ann.plan(n, dim, ic.NLIST, ic.HAND_MAX_LIST_ROWS, nq, 2, k) == (64, 1792, 3)
    X = ic.mixed_rows(rng, n, dim)
    Xd = _device(X)
    idx = ann.from_labels(Xd, torch.ones(ic.NLIST, dim).cuda(), torch.from_numpy(labels).cuda())
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    probes = np.tile(np.array([ic.LONG_LIST, 7]), (nq, 1))
    got = ann.search(Xd, idx, k, queries=_device(Q), probes=torch.from_numpy(probes).cuda())
    ic.same(_host(got), ic.expect(oracle, X, labels, probes, k, queries=Q), "three chunks")


# ---- 3. ties across lists and chunks ------------------------------------------------------------------------------

def test_ties_come_back_in_original_row_order(oracle):
    from node2vec_amd import ann

    rng = np.random.default_rng(6)
    dim, long_len = 16, 2 * 1792 + 1
    labels = ic.hand_labels(rng, long_len)
    n = len(labels)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    long_members = np.nonzero(labels == ic.LONG_LIST)[0]
    # copies of one row: in each chunk of the long list (by position in the list) and in three other lists
    copies = [long_members[5], long_members[1791], long_members[1792], long_members[3583], long_members[3584]]
    copies += [np.nonzero(labels == l)[0][0] for l in (1, 4, 7)]
    copies = np.sort(np.array(copies))
    X[copies] = X[copies[0]]
    Xd = _device(X)
    idx = ann.from_labels(Xd, torch.ones(ic.NLIST, dim).cuda(), torch.from_numpy(labels).cuda())
    idx.max_list_rows = ic.HAND_MAX_LIST_ROWS
    Q = np.tile(X[copies[0]], (3, 1))
    probes = np.array([[8, 1, 4, 7], [7, 4, 1, 8], [4, 8, -1, 7]])
    for k in (3, 8, 20):
        got = _host(ann.search(Xd, idx, k, queries=_device(Q), probes=torch.from_numpy(probes).cuda()))
        ic.same(got, ic.expect(oracle, X, labels, probes, k, queries=Q), f"k={k}")
        assert got[0][0].tolist()[:min(k, 8)] == copies[:min(k, 8)].tolist()
        assert got[0][1].tolist() == got[0][0].tolist()  # the order of the probes does not matter
        mine = [c for c in copies if labels[c] != 1]
        assert got[0][2].tolist()[:min(k, 7)] == mine[:min(k, 7)]


# ---- 4. zero and non-finite values --------------------------------------------------------------------------------

def test_zero_and_non_finite_values(oracle):
    from node2vec_amd import ann

    rng = np.random.default_rng(7)
    n, dim, nlist, k = 1500, 20, 6, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[::7] = 0.0
    X[3, 5] = np.nan
    X[900, 1] = np.inf
    labels = rng.integers(0, nlist, n)
    Q = rng.standard_normal((5, dim)).astype(np.float32)
    Q[1] = 0.0
    Q[2, 0] = np.nan
    Xd = _device(X)
    idx = ann.from_labels(Xd, torch.ones(nlist, dim).cuda(), torch.from_numpy(labels).cuda())
    probes = np.tile(np.arange(nlist), (5, 1))
    r, s = _host(ann.search(Xd, idx, k, queries=_device(Q), probes=torch.from_numpy(probes).cuda()))
    ic.same((r, s), ic.expect(oracle, X, labels, probes, k, queries=Q), "queries")
    assert not np.isin(r, (3, 900)).any() and not np.isnan(s).any()
    # a zero query scores 0 against every row it can score (a zero row included): the first rows, in order
    assert (s[1] == 0).all() and r[1].tolist() == [i for i in range(k + 1) if i != 3]
    assert (r[2] == -1).all() and (s[2] == -np.inf).all()  # a NaN query: only the tail
    zero = np.nonzero(~X.any(axis=1))[0]
    R = np.array([zero[0], 3, 900, 10])
    r, s = _host(ann.search(Xd, idx, k, rows=torch.from_numpy(R).cuda(), probes=torch.from_numpy(probes[:4]).cuda()))
    ic.same((r, s), ic.expect(oracle, X, labels, probes[:4], k, rows=R), "rows")
    assert (s[0] == 0).all() and (r[1:3] == -1).all()  # a zero query row; query rows holding NaN and inf
    # probe() gives a NaN query no list at all
    assert (ann.probe(idx, queries=_device(Q), nprobe=3)[2] == -1).all()


# ---- 5. the status word -------------------------------------------------------------------------------------------

def test_status_word_raises_and_the_run_ends_normally():
    from node2vec_amd import ann

    rng = np.random.default_rng(8)
    n, dim, nlist = 2000, 16, 5
    Xd = _device(rng.standard_normal((n, dim)))
    idx, labels = _random_index(ann, Xd, rng, nlist)
    Q = _device(rng.standard_normal((9, dim)))
    good = ann.search(Xd, idx, 5, queries=Q, nprobe=nlist)
    longest = idx.max_list_rows
    idx.max_list_rows = longest - 1
    with pytest.raises(ValueError, match="max_list_rows"):
        ann.search(Xd, idx, 5, queries=Q, nprobe=nlist)
    idx.max_list_rows = 1
    with pytest.raises(ValueError, match="max_list_rows"):
        ann.search(Xd, idx, 5, queries=Q, nprobe=nlist)
    idx.max_list_rows = longest
    probes = torch.zeros((9, 2), dtype=torch.int32, device="cuda")
    probes[4, 1] = nlist
    with pytest.raises(ValueError, match="probe"):
        ann.search(Xd, idx, 5, queries=Q, probes=probes)
    probes[4, 1] = -2
    with pytest.raises(ValueError, match="probe"):
        ann.search(Xd, idx, 5, queries=Q, probes=probes)
    again = ann.search(Xd, idx, 5, queries=Q, nprobe=nlist)  # the device is as it was
    assert torch.equal(again[0], good[0]) and torch.equal(again[1].view(torch.int32), good[1].view(torch.int32))


# ---- 6. build_index -----------------------------------------------------------------------------------------------

def test_build_index_is_reproducible_and_follows_kmeans():
    from node2vec_amd import ann, cluster

    rng = np.random.default_rng(9)
    n, dim = 4000, 24
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[17, 3] = np.nan  # k-means leaves it unassigned
    Xd = _device(X)
    a = ann.build_index(Xd, nprobe=100, seed=4, max_iter=8)
    b = ann.build_index(Xd, nprobe=100, seed=4, max_iter=8)
    assert a.nlist == round(np.sqrt(n)) == 63 and a.nprobe == 63 and (a.n, a.dim) == (n, dim)
    for name in ("centroids", "centroid_inv_norm", "list_off", "row_ids"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta.dtype == tb.dtype and torch.equal(ta.view(torch.int32) if ta.dtype == torch.float32 else ta,
                                                    tb.view(torch.int32) if tb.dtype == torch.float32 else tb), name
    assert a.max_list_rows == b.max_list_rows == int((a.list_off[1:] - a.list_off[:-1]).max())
    assert a.list_off.dtype == torch.int64 and a.row_ids.dtype == torch.int32
    labels, _ = cluster.assign(Xd, a.centroids, "cosine")
    labels = labels.cpu().numpy()
    assert labels[17] == -1
    rows, off = a.row_ids.cpu().numpy(), a.list_off.cpu().numpy()
    assert np.array_equal(np.sort(rows), np.nonzero(labels >= 0)[0])  # a permutation of the assigned rows
    for l in range(a.nlist):
        assert np.array_equal(rows[off[l]:off[l + 1]], np.nonzero(labels == l)[0]), l
    other = ann.build_index(Xd, nlist=10, nprobe=3, seed=5, max_iter=3)
    assert other.nlist == 10 and other.nprobe == 3


# ---- 7. nested probes ---------------------------------------------------------------------------------------------

def test_more_probes_never_lower_a_score():
    from node2vec_amd import ann, similarity

    rng = np.random.default_rng(10)
    n, dim, nlist, k = 5000, 32, 24, 10
    centres = rng.standard_normal((40, dim)).astype(np.float32)
    X = centres[rng.integers(0, 40, n)] + 0.5 * rng.standard_normal((n, dim)).astype(np.float32)
    Xd = _device(X)
    idx = ann.build_index(Xd, nlist=nlist, seed=1, max_iter=10)
    R = torch.from_numpy(rng.integers(0, n, 150)).cuda()
    full = ann.probe(idx, rows=R, X=Xd, nprobe=nlist)
    assert full.dtype == torch.int32 and full.shape == (150, nlist)
    assert (full.sort(dim=1)[0] == torch.arange(nlist, device="cuda", dtype=torch.int32)).all()
    prev = None
    for nprobe in (1, 2, 5, 23, 24):
        assert torch.equal(ann.probe(idx, rows=R, X=Xd, nprobe=nprobe), full[:, :nprobe])  # nested
        idx.nprobe = nprobe
        r, s = ann.search(Xd, idx, k, rows=R)
        if prev is not None:
            assert (s >= prev).all(), nprobe
        prev = s
    _same_as_knn((r, s), similarity.knn(Xd, k, rows=R), "nprobe = nlist")


# ---- 8. query batches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,by_rows", [(40, False), (37, True)])  # steps of 5: eight launches | seven and a ragged one
def test_search_splits_a_batch_to_fit_the_workspace(monkeypatch, nq, by_rows):
    from node2vec_amd import ann, similarity

    rng = np.random.default_rng(70)
    n, dim, nlist, nprobe, k = 70, 8, 4, 3, 10
    Xd = _device(ic.mixed_rows(rng, n, dim))
    idx = ann.build_index(Xd, nlist=nlist, seed=1, max_iter=5)
    who = {"rows": torch.from_numpy(rng.integers(0, n, nq)).cuda()} if by_rows else \
        {"queries": _device(rng.standard_normal((nq, dim)))}
    L = ann._lib.load()
    real, scans = L.n2v_ivf_topk, []  # the queries of every launch: n2v_ivf_topk's eleventh argument
    monkeypatch.setattr(L, "n2v_ivf_topk", lambda *args: scans.append(args[10]) or real(*args))
    whole = ann.search(Xd, idx, k, nprobe=nprobe, **who)
    need = L.n2v_ivf_workspace_bytes(n, dim, nlist, idx.max_list_rows, 6, nprobe, k)
    monkeypatch.setattr(similarity, "WORKSPACE_LIMIT", int(need))
    parts = ann.search(Xd, idx, k, nprobe=nprobe, **who)
    ic.same(_host(parts), _host(whole), "split")
    assert scans[0] == nq and len(scans) > 2 and sum(scans[1:]) == nq


# ---- 9. the API ---------------------------------------------------------------------------------------------------

def test_keyed_vectors_indexer():
    from node2vec_amd.embedding import KeyedVectors

    rng = np.random.default_rng(11)
    n, dim = 3000, 16
    ids = rng.permutation(n).astype(np.int64) + 100
    kv = KeyedVectors(ids, _device(rng.standard_normal((n, dim))))
    idx = kv.build_index(nlist=12, seed=2, max_iter=5)
    assert idx.nlist == 12 and idx.nprobe == 8
    idx.nprobe = idx.nlist
    token = str(int(ids[40]))
    assert kv.most_similar(token, topn=7, indexer=idx) == kv.most_similar(token, topn=7)
    assert kv.similar_by_word(token, topn=3, indexer=idx) == kv.similar_by_word(token, topn=3)
    v = rng.standard_normal(dim).astype(np.float32)
    assert kv.similar_by_vector(v, topn=5, indexer=idx) == kv.similar_by_vector(v, topn=5)
    assert kv.most_similar([token, str(int(ids[41]))], [str(int(ids[42]))], topn=9, indexer=idx) == \
        kv.most_similar([token, str(int(ids[41]))], [str(int(ids[42]))], topn=9)
    rows = torch.arange(0, 200, device="cuda")
    a, b = kv.nearest(rows, 6, indexer=idx), kv.nearest(rows, 6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    a, b = kv.nearest(rows, 6, exclude_self=False, indexer=idx), kv.nearest(rows, 6, exclude_self=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    idx.nprobe = 1  # fewer lists: still the same tokens' scores, never better than the exact ones
    approx = kv.most_similar(token, topn=7, indexer=idx)
    exact = dict(kv.most_similar(token, topn=n))
    assert approx and all(exact[t] == s for t, s in approx)
    for call in (lambda: kv.most_similar(token, restrict_vocab=100, indexer=idx),
                 lambda: kv.most_similar(token, topn=None, indexer=idx),
                 lambda: kv.nearest(rows, 6, restrict_vocab=100, indexer=idx),
                 lambda: kv.nearest(rows, 128, indexer=idx)):
        with pytest.raises(ValueError):
            call()
