"""Nearest-neighbour queries on the GPU (csrc/n2v_knn.hip through node2vec_amd.similarity and
KeyedVectors.most_similar) against a float64 brute force over the same fp32 matrix.

A score may differ from its float64 cosine by tol = dim * 2^-22; the top k are right when every
returned score is within tol, every row clearly above the k-th float64 score is returned and no row
clearly below it is."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _cos64(X, Q):
    """float64 cosines [nq, n] of fp32 X and Q (norm 0 -> 0), on the device"""
    X64, Q64 = X.double(), Q.double()
    nx, nq = X64.norm(dim=1), Q64.norm(dim=1)
    S = (Q64 @ X64.T) / (nq[:, None] * nx[None, :])
    return torch.nan_to_num(S, nan=0.0)


def _check_topk(rows, scores, ref, k, tol):
    nq, n = ref.shape
    assert rows.shape == (nq, k) and scores.shape == (nq, k)
    keep = min(k, n)
    assert (rows[:, keep:] == -1).all() and torch.isinf(scores[:, keep:]).all()
    r, s = rows[:, :keep], scores[:, :keep]
    assert (r >= 0).all() and (r < n).all()
    assert all(len(set(x)) == keep for x in r.tolist())
    got = torch.gather(ref, 1, r)
    assert (got - s.double()).abs().max() <= tol
    kth = torch.topk(ref, keep, dim=1).values[:, -1:]
    assert (got >= kth - tol).all()  # nothing clearly below the k-th
    must = ref > kth + tol  # everything clearly above it is there
    hit = torch.zeros_like(must)
    hit.scatter_(1, r, True)
    assert (hit | ~must).all()
    # best first, ties by row
    assert (s[:, 1:] <= s[:, :-1]).all()
    tie = s[:, 1:] == s[:, :-1]
    assert (r[:, 1:][tie] > r[:, :-1][tie]).all()


CASES = [  # n, dim, nq, k
    (1, 1, 1, 1), (1, 3, 5, 10), (17, 3, 5, 10), (17, 128, 64, 100), (1000, 1, 5, 10), (1000, 3, 64, 100),
    (1000, 100, 64, 1000), (1000, 128, 1000, 10), (1000, 300, 5, 2000), (1000, 1024, 5, 100),
    (100003, 128, 64, 10), (100003, 100, 5, 1000), (100003, 128, 1000, 100), (100003, 300, 1, 10),
    (100003, 1024, 5, 10), (100003, 128, 5, 2000), (17, 1024, 1000, 1), (1000, 128, 64, 200), (100003, 64, 40, 500),
]


@pytest.mark.parametrize("n,dim,nq,k", CASES)
def test_knn_equals_float64_brute_force(n, dim, nq, k):
    from node2vec_amd import similarity

    g = torch.Generator(device="cuda").manual_seed(n * 7 + dim * 3 + nq + k)
    X = torch.randn(n, dim, device="cuda", generator=g)
    Q = torch.randn(nq, dim, device="cuda", generator=g)
    tol = dim * 2.0 ** -22
    rows, scores = similarity.knn(X, k, queries=Q)
    _check_topk(rows, scores, _cos64(X, Q), k, tol)
    # rows= : queries drawn from X itself
    qr = torch.randint(0, n, (nq,), device="cuda", generator=g)
    rows2, scores2 = similarity.knn(X, k, rows=qr)
    _check_topk(rows2, scores2, _cos64(X, X[qr]), k, tol)
    # the same rows passed as vectors: bit for bit
    rows3, scores3 = similarity.knn(X, k, queries=X[qr])
    assert torch.equal(rows2, rows3) and torch.equal(scores2, scores3)
    # restrict: the first rows only
    cut = max(1, n // 3)
    rows4, scores4 = similarity.knn(X, k, queries=Q, restrict=cut)
    _check_topk(rows4, scores4, _cos64(X[:cut], Q), k, tol)


def test_knn_is_bitwise_reproducible_and_batch_independent():
    from node2vec_amd import similarity

    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn(50000, 128, device="cuda", generator=g)
    Q = torch.randn(300, 128, device="cuda", generator=g)
    for k in (10, 100, 500, 1000, 1500):
        r1, s1 = similarity.knn(X, k, queries=Q)
        r2, s2 = similarity.knn(X, k, queries=Q)
        assert torch.equal(r1, r2) and torch.equal(s1, s2)
        for i in (0, 17, 299):
            ri, si = similarity.knn(X, k, queries=Q[i:i + 1])
            assert torch.equal(ri[0], r1[i]) and torch.equal(si[0], s1[i]), (k, i)
        ri, si = similarity.knn(X, k, queries=Q[40:90])
        assert torch.equal(ri, r1[40:90]) and torch.equal(si, s1[40:90])
        # the selected scores are the full-score kernel's values, bit for bit
        full = similarity.scores(X, queries=Q)
        assert torch.equal(torch.gather(full, 1, r1), s1)


def test_duplicates_in_row_order_and_zero_rows():
    from node2vec_amd import similarity

    g = torch.Generator(device="cuda").manual_seed(9)
    X = torch.randn(3000, 64, device="cuda", generator=g)
    X[[40, 700, 2999]] = X[5].clone()
    X[100] = 0.0
    for k in (4, 300):
        rows, scores = similarity.knn(X, k, rows=torch.tensor([5], device="cuda"))
        assert rows[0, :4].tolist() == [5, 40, 700, 2999]
        assert (scores[0, :4] == scores[0, 0]).all() and abs(float(scores[0, 0]) - 1) <= 64 * 2 ** -22
    full = similarity.scores(X, queries=X[:3])
    assert (full[:, 100] == 0).all()
    assert (similarity.scores(X, queries=torch.zeros(1, 64, device="cuda")) == 0).all()
    assert float(similarity.inv_norms(X)[100]) == 0.0
    r, s = similarity.knn(X, 3, rows=torch.tensor([5, 40], device="cuda"), exclude_self=True)
    assert r[0].tolist() == [40, 700, 2999] and r[1].tolist() == [5, 700, 2999]


def test_offsets_past_2_to_the_32_elements():
    """n = 2^22 + 5 rows of dim 1024 (17 GB): copies of the queries planted in the last rows are found"""
    from node2vec_amd import similarity

    n, dim = (1 << 22) + 5, 1024
    g = torch.Generator(device="cuda").manual_seed(11)
    X = torch.empty(n, dim, device="cuda")
    for lo in range(0, n, 1 << 20):
        X[lo:lo + (1 << 20)].normal_(generator=g)
    Q = torch.randn(4, dim, device="cuda", generator=g)
    X[n - 4:] = Q
    tol = dim * 2.0 ** -22
    inv = similarity.inv_norms(X)
    rows, scores = similarity.knn(X, 3, queries=Q, inv_norm=inv)
    assert rows[:, 0].tolist() == list(range(n - 4, n))
    assert ((scores[:, 0] - 1).abs() <= tol).all() and (scores[:, 1] < 0.5).all()
    rows2, scores2 = similarity.knn(X, 3, rows=torch.arange(n - 4, n, device="cuda"), inv_norm=inv)
    assert torch.equal(rows2[:, 0], rows[:, 0]) and ((scores2[:, 0] - 1).abs() <= tol).all()
    full = similarity.scores(X, queries=Q[:1], inv_norm=inv)
    assert abs(float(full[0, n - 4]) - 1) <= tol and torch.equal(full[0, rows[0]], scores[0])
    del X, full
    torch.cuda.empty_cache()


def _gensim_most_similar(V, index2word, positive, negative, topn, restrict=None):
    """gensim 3.8 KeyedVectors.most_similar restated in float64: [(token, score)], all scores"""
    V = V.astype(np.float64)
    vn = V / np.linalg.norm(V, axis=1, keepdims=True)
    vocab = {t: i for i, t in enumerate(index2word)}
    items = [(w, 1.0) if isinstance(w, (str, np.ndarray)) else w for w in positive]
    items += [(w, -1.0) if isinstance(w, (str, np.ndarray)) else w for w in negative]
    mean, own = [], set()
    for w, wt in items:
        if isinstance(w, np.ndarray):
            mean.append(wt * w.astype(np.float64))
        else:
            mean.append(wt * vn[vocab[w]])
            own.add(vocab[w])
    mean = np.mean(mean, axis=0)
    mean /= np.linalg.norm(mean)
    lim = vn if restrict is None else vn[:restrict]
    dists = lim @ mean
    return dists, own


def _check_hits(hits, dists, own, index2word, topn, tol):
    allowed = np.array([i not in own for i in range(len(dists))])
    ref = np.where(allowed, dists, -np.inf)
    keep = min(topn, int(allowed.sum()))
    assert len(hits) == keep
    kth = np.sort(ref)[::-1][keep - 1]
    idx = {t: i for i, t in enumerate(index2word)}
    got = [idx[t] for t, _ in hits]
    assert len(set(got)) == keep and not set(got) & own
    for (t, s), i in zip(hits, got):
        assert abs(s - dists[i]) <= tol and dists[i] >= kth - tol
    assert set(np.nonzero(ref > kth + tol)[0]) <= set(got)


@pytest.mark.parametrize("held", ["device", "text"])
def test_most_similar_matches_gensim(tmp_path, held):
    from node2vec_amd.embedding import KeyedVectors

    rng = np.random.default_rng(3)
    n, dim = 500, 48
    V = rng.standard_normal((n, dim)).astype(np.float32)
    kv = KeyedVectors(np.arange(100, 100 + n, dtype=np.int64), torch.from_numpy(V).cuda())
    if held == "text":
        kv.save_word2vec_format(str(tmp_path / "v.txt"))
        kv = KeyedVectors.load_word2vec_format(str(tmp_path / "v.txt"))
        V = kv.vectors
    words = list(kv.index2word)
    tol = dim * 2.0 ** -22 + 1e-6  # + the host-side mean in fp32
    vec = rng.standard_normal(dim).astype(np.float32)
    for pos, neg, topn, restrict in ((["105"], [], 10, None), (["105", "230"], ["400"], 25, None),
                                     ([("101", 0.3), "102"], [("555", 2.0)], 7, 300), ([vec], [], 12, None),
                                     (["105"], [], 2000, None), ([vec, "150"], ["151"], 5, 50)):
        hits = kv.most_similar(positive=pos, negative=neg, topn=topn, restrict_vocab=restrict)
        dists, own = _gensim_most_similar(V, words, pos, neg, topn, restrict)
        _check_hits(hits, dists, own, words, topn, tol)
    full = kv.most_similar("105", topn=None)
    dists, _ = _gensim_most_similar(V, words, ["105"], [], None)
    assert full.dtype == np.float32 and full.shape == (n,) and np.abs(full - dists).max() <= tol
    _check_hits(kv.most_similar(105, topn=4), dists, {5}, words, 4, tol)
    _check_hits(kv.similar_by_word("105", topn=4), dists, {5}, words, 4, tol)
    dv, _ = _gensim_most_similar(V, words, [vec], [], None)
    _check_hits(kv.similar_by_vector(vec, topn=6), dv, set(), words, 6, tol)
    a, b = V[3].astype(np.float64), V[9].astype(np.float64)
    assert abs(kv.similarity("103", "109") - a @ b / np.linalg.norm(a) / np.linalg.norm(b)) <= tol
    rows, scores = kv.nearest([5, 6], topn=3)
    assert rows.is_cuda and rows.shape == (2, 3) and 5 not in rows[0].tolist() and 6 not in rows[1].tolist()
    assert rows[0].tolist() == [words.index(t) for t, _ in kv.most_similar("105", topn=3)]


@pytest.mark.parametrize("with_names", [False, True])
def test_node2vec_most_similar_end_to_end(with_names):
    from node2vec_amd.embedding import Node2VecHIP
    from node2vec_amd.fugue import random_walk

    df = pd.DataFrame(load_golden("karate_edges.json"), columns=["src", "dst", "weight"])
    params = {"num_walks": 10, "walk_length": 10, "return_param": 1.0, "inout_param": 1.0}
    walks = random_walk("hip", df, params, random_seed=42)
    name_id = pd.DataFrame({"name": [f"v{i}" for i in range(34)], "id": list(range(34))}) if with_names else None
    n2v = Node2VecHIP(walks, {"min_count": 0, "iter": 5, "size": 32, "negative": 5, "deterministic": True},
                      name_id=name_id, random_seed=1000)
    n2v.fit()
    out = n2v.most_similar(0, topn=5)
    assert list(out.columns) == ["name" if with_names else "id", "similarity"] and len(out) == 5
    wv = n2v.model.wv
    V = np.stack([wv.rows(i, i + 1)[0] for i in range(len(wv))])
    words = list(wv.index2word)
    dists, own = _gensim_most_similar(V, words, ["0"], [], 5)
    ids = out["name"].str[1:].astype(int).tolist() if with_names else out["id"].tolist()
    _check_hits(list(zip(map(str, ids), out["similarity"])), dists, own, words, 5, 32 * 2.0 ** -22 + 1e-6)
    assert 0 not in ids
