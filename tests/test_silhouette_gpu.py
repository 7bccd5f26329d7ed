"""Silhouette scores on the GPU (csrc/n2v_silhouette.hip through node2vec_amd.cluster) against the CPU restatement,
tests/cpu_silhouette/n2v_silhouette_cpu.c, bit for bit: a, b and s by their fp64 bit patterns (NaN positions as
positions), nearest and counts with array_equal.  The shapes sit on the kernel's edges: both load paths (dim % 4,
base alignment), a ragged last 16-block and a ragged batch of eight loads (dim), segments that end before, on and
after a tile of 16 (cluster sizes), the loop over clusters (k), a ragged tile, wave and block of scored rows (m)."""
import numpy as np
import pandas as pd
import pytest
import torch

import silhouette_cases as sc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return sc.build(tmp_path_factory.mktemp("silhouette_cpu"))


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


def _same(got, want, what):
    """a SilhouetteResult of device tensors against a restated sc.Sil"""
    for name in ("s", "a", "b"):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.dtype == np.float64 and sc.same_bits(g, w), (what, name, np.nonzero(~(g == w) & ~np.isnan(w))[0][:8])
    assert np.array_equal(got.nearest.cpu().numpy(), want.nearest), what
    assert got.nearest.dtype == torch.int32 and got.counts.dtype == torch.int64
    assert np.array_equal(got.counts.cpu().numpy(), want.counts), what


def _check(cpu, X, labels, k, metric, rows=None, aligned=True):
    from node2vec_amd import cluster

    inv = sc.inv_norms(cpu, X)
    want = sc.restated(cpu, X, labels, k, metric, rows=rows, inv=inv)
    got = cluster.silhouette_samples(_device(X, aligned), torch.from_numpy(np.asarray(labels)).cuda(), metric, k,
                                     None if rows is None else torch.from_numpy(np.asarray(rows)),
                                     inv_norm=_device(inv))
    _same(got, want, (metric, X.shape, k, aligned, None if rows is None else len(rows)))
    return got, want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 4, 15, 16, 17, 64, 100, 128, 129, 1024])
def test_bitwise_over_the_dimensions_and_both_load_paths(cpu, dim, metric):
    X, labels = sc.normal_case(83, dim, 3, 31 * dim)
    X[5] = 0.0           # a zero row: at cosine distance 1 from everything
    X[7] = X[6]          # duplicates, in one cluster and across two
    X[9] = X[8]
    labels[6] = labels[7] = 0
    labels[8], labels[9] = 1, 2
    labels[[11, 40]] = -1
    for aligned in (True, False):
        _check(cpu, X, labels, 3, metric, aligned=aligned)


@pytest.mark.parametrize("metric", METRICS)
def test_bitwise_over_the_segment_padding_edges(cpu, metric):
    sizes = [1, 15, 16, 17, 0, 31, 33]  # an empty id inside [0, k); 5 rows of no cluster
    labels = sc.sized_labels(sizes, extra_none=5, seed=3)
    labels[labels == -1] = [-1, 7, -5, 1 << 30, -(1 << 31)]  # not labels: as -1
    X, _ = sc.normal_case(len(labels), 20, 7, 5)
    got, want = _check(cpu, X, labels, 7, metric)
    assert want.counts.tolist() == sizes
    s = got.s.cpu().numpy()
    assert s[labels == 0].tolist() == [0.0]  # the singleton
    member = (labels >= 0) & (labels < 7)
    assert np.isnan(s[~member]).all() and not np.isnan(s[member]).any()
    assert not (got.nearest.cpu().numpy() == 4).any()  # the empty cluster is nobody's neighbour


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [2, 3, 16, 17, 64, 65, 1024])
def test_bitwise_over_the_cluster_counts(cpu, k, metric):
    n = 1100 if k == 1024 else 210
    X, labels = sc.normal_case(n, 24, k, k)
    _check(cpu, X, labels, k, metric)


@pytest.fixture(scope="module")
def full(cpu):
    """one case and its restated full result per metric, shared by the subset tests"""
    X, labels = sc.normal_case(300, 36, 5, 77)
    labels[::17] = -1
    inv = sc.inv_norms(cpu, X)
    return X, labels, inv, {m: sc.restated(cpu, X, labels, 5, m, inv=inv) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_bitwise_over_the_scored_row_counts(cpu, full, metric):
    from node2vec_amd import cluster

    X, labels, inv, want = full
    Xd, ld, invd = _device(X), torch.from_numpy(labels).cuda(), _device(inv)
    whole = cluster.silhouette_samples(Xd, ld, metric, 5, inv_norm=invd)
    _same(whole, want[metric], (metric, "every row"))
    rng = np.random.default_rng(1)
    for m in (1, 15, 16, 17, 63, 64, 65, 255, 257):
        # every row of a smaller matrix (rows=None: m == n)
        _check(cpu, X[:m], labels[:m], 5, metric)
        # an unsorted subset with a repeated index: the same bits as those rows of the full call
        rows = rng.integers(0, 300, m)
        rows[-1] = rows[0]
        part = cluster.silhouette_samples(Xd, ld, metric, 5, torch.from_numpy(rows), inv_norm=invd)
        for name in ("s", "a", "b"):
            assert sc.same_bits(getattr(part, name).cpu().numpy(), getattr(want[metric], name)[rows]), (m, name)
            assert sc.same_bits(getattr(part, name).cpu().numpy(), getattr(whole, name).cpu().numpy()[rows])
        assert np.array_equal(part.nearest.cpu().numpy(), want[metric].nearest[rows])
        assert torch.equal(part.counts, whole.counts)


@pytest.mark.parametrize("metric", METRICS)
def test_rows_that_are_no_rows_score_nan_and_read_nothing(cpu, full, metric):
    X, labels, _, _ = full
    rows = np.array([5, -1, 300, 1 << 40, -(1 << 62), 0, 17, 299], np.int64)  # row 0 and 17 have no cluster
    got, _ = _check(cpu, X, labels, 5, metric, rows=rows)
    assert np.isnan(got.s.cpu().numpy()).tolist() == [False, True, True, True, True, True, True, False]


def test_a_run_on_another_stream_and_the_same_call_twice(cpu, full):
    from node2vec_amd import cluster

    X, labels, inv, want = full
    Xd, ld, invd = _device(X), torch.from_numpy(labels).cuda(), _device(inv)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = cluster.silhouette_samples(Xd, ld, "cosine", 5, inv_norm=invd)
    stream.synchronize()
    _same(got, want["cosine"], "side stream")
    again = cluster.silhouette_samples(Xd, ld, "cosine", 5, inv_norm=invd)
    assert torch.equal(again.s.view(torch.int64), got.s.view(torch.int64))


def test_score_is_the_mean_of_the_samples_and_the_sample_is_exact(cpu, full):
    from node2vec_amd import cluster

    X, labels, inv, want = full
    Xd, ld = _device(X), torch.from_numpy(labels).cuda()
    member = labels >= 0
    for metric in METRICS:
        res = cluster.silhouette_samples(Xd, ld, metric)  # k = labels.max() + 1, inv_norm computed
        _same(res, want[metric], metric)
        score = cluster.silhouette_score(Xd, ld, metric)
        assert score == float(res.s[torch.from_numpy(member).cuda()].mean())
        assert abs(score - want[metric].s[member].mean()) <= 1e-12
        rows = cluster.sample_rows(ld, 5, 40, seed=9)
        sampled = cluster.silhouette_score(Xd, ld, metric, sample_size=40, seed=9)
        assert sampled == cluster.silhouette_score(Xd, ld, metric, sample_size=40, seed=9)
        assert sampled == float(res.s[rows.cuda()].mean())  # each sampled value is the row's exact silhouette
        assert cluster.silhouette_score(Xd, ld, metric, sample_size=10 ** 6) == score
    blobs = np.concatenate([np.random.default_rng(c).standard_normal((50, 8)) * 0.05 + 4.0 * c for c in range(3)])
    planted = np.repeat(np.arange(3), 50).astype(np.int32)
    good = cluster.silhouette_score(_device(blobs), torch.from_numpy(planted).cuda())
    bad = cluster.silhouette_score(_device(blobs), torch.from_numpy(np.roll(planted, 25)).cuda())
    assert good > 0.9 > bad


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_keyedvectors_and_model_classes_score_their_clusters(cpu):
    from node2vec_amd import cluster
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    rng = np.random.default_rng(6)
    centres = rng.standard_normal((2, 8)) * 4.0
    planted = rng.integers(0, 2, 40)
    X = (centres[planted] + rng.standard_normal((40, 8)) * 0.05).astype(np.float32)
    ids = np.arange(40)[::-1] + 100  # vocabulary order is not id order
    wv = KeyedVectors(ids, X)
    res = wv.kmeans(2, seed=1)
    sil = wv.silhouette(res)  # cosine over the cached norms, as kmeans
    want = sc.restated(cpu, X, res.labels.cpu().numpy(), 2, "cosine", inv=sc.inv_norms(cpu, X))
    _same(sil, want, "KeyedVectors")
    same = wv.silhouette(res.labels)  # a label tensor: k = labels.max() + 1
    assert torch.equal(same.s.view(torch.int64), sil.s.view(torch.int64))
    part = wv.silhouette(res.labels[:25], metric="euclidean", restrict_vocab=25)
    _same(part, sc.restated(cpu, X[:25], res.labels[:25].cpu().numpy(), 2, "euclidean"), "restrict_vocab")
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((40, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((39, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.silhouette()
        n2v.model = model(KeyedVectors(ids, X))
        with pytest.raises(ValueError):
            n2v.silhouette()
        for metric in ("cosine", "euclidean"):
            clusters = n2v.cluster(2, metric=metric, seed=1)
            assert list(clusters.columns) == ["id", "cluster"]  # cluster() itself is unchanged
            df = n2v.silhouette()
            assert list(df.columns) == ["id", "cluster", "silhouette"] and n2v.clusters is clusters
            assert df["id"].tolist() == ids.tolist() and df["cluster"].tolist() == clusters["cluster"].tolist()
            labels = n2v.kmeans_result.labels
            direct = cluster.silhouette_samples(_device(X), labels, metric, 2)
            assert sc.same_bits(df["silhouette"].to_numpy(), direct.s.cpu().numpy())
            assert n2v.silhouette_score == cluster.silhouette_score(_device(X), labels, metric, k=2)
            assert n2v.silhouette_score > 0.9  # two blobs far apart
