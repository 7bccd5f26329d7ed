"""DBSCAN on the GPU (csrc/n2v_dbscan.hip through node2vec_amd.cluster) against the CPU restatement,
tests/cpu_dbscan/n2v_dbscan_cpu.c: counts, core mask, labels, n_clusters and sizes, all exactly; on gapped cases
against scikit-learn's brute-force DBSCAN as well.  The shapes sit on the kernels' edges: ragged tiles, waves and
chunks of rows (n), a ragged last 16-block and both load paths (dim), components that cross every tile and block,
the highest contention the union-find can see, and every launch geometry a block cap gives."""
import numpy as np
import pandas as pd
import pytest
import torch

import dbscan_cases as dc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return dc.build(tmp_path_factory.mktemp("dbscan_cpu"))


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
    """a DBSCANResult of device tensors against a dc.Db"""
    assert got.labels.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.sizes.dtype == torch.int64
    assert got.core_mask.dtype == torch.bool
    n = len(want.labels)
    assert got.labels.shape == got.counts.shape == got.core_mask.shape == (n,)
    counts, core, labels = got.counts.cpu().numpy(), got.core_mask.cpu().numpy(), got.labels.cpu().numpy()
    assert np.array_equal(counts, want.counts), (what, np.nonzero(counts != want.counts)[0][:8])
    assert np.array_equal(core, want.core), what
    assert np.array_equal(labels, want.labels), (what, np.nonzero(labels != want.labels)[0][:8])
    assert got.n_clusters == want.n_clusters, what
    assert np.array_equal(got.sizes.cpu().numpy(), np.bincount(want.labels[want.labels >= 0],
                                                               minlength=want.n_clusters)), what


def _check(cpu, X, eps, min_samples, metric, want=None, max_blocks=0, aligned=True):
    from node2vec_amd import cluster

    inv = dc.inv_norms(cpu, X) if metric == "cosine" else None
    if want is None:
        want = dc.restated(cpu, X, eps, min_samples, metric, inv=inv)
    got = cluster.dbscan(_device(X, aligned), eps, min_samples, metric, inv_norm=None if inv is None else _device(inv),
                         max_blocks=max_blocks)
    _same(got, want, (metric, X.shape, eps, min_samples, max_blocks, aligned))
    return got, want


def _random_case(n, dim, seed):
    """normal rows with a duplicate pair; eps at the 15 % point of the float64 distances (not gapped: against the
    restatement alone)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 4:
        X[3] = X[1]
    eps = {}
    for metric in METRICS:
        D = dc.distances64(X, metric)
        eps[metric] = float(np.quantile(D, 0.15)) if n > 1 else 0.5
    return X, eps


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 16, 17, 128, 130])
def test_exact_over_the_tile_and_dimension_edges(cpu, dim, metric):
    kinds = set()
    for n in (1, 15, 16, 17, 63, 65, 257):
        X, eps = _random_case(n, dim, 1000 * dim + n)
        for min_samples in (1, 4):
            got, want = _check(cpu, X, eps[metric], min_samples, metric)
        if dim % 4 == 0:  # the same rows from a base that is not 16-byte aligned: the scalar load path
            _check(cpu, X, eps[metric], 4, metric, want=want, aligned=False)
        kinds |= {"noise"} if (want.labels == -1).any() else set()
        kinds |= {"border"} if (~want.core & (want.labels >= 0)).any() else set()
        kinds |= {"clusters"} if want.n_clusters > 1 else set()
    assert kinds >= {"noise", "border"}, kinds


def test_a_chain_that_crosses_every_tile_and_block_and_falls_apart_one_step_below_eps(cpu):
    """700 points a distance of exactly 1 apart, eps = 1: every pair of the chain sits on the threshold"""
    X = dc.chain(700, 4)
    got, _ = _check(cpu, X, 1.0, 2, "euclidean")
    assert got.n_clusters == 1 and bool((got.labels == 0).all())
    assert got.counts.cpu().tolist() == [2] + [3] * 698 + [2]
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    got, _ = _check(cpu, X, below, 2, "euclidean")
    assert got.n_clusters == 0 and bool((got.labels == -1).all()) and bool((got.counts == 1).all())


def test_two_chains_interleaved_by_index(cpu):
    """even rows are one cluster and odd rows the other: every tile mixes the two components"""
    got, _ = _check(cpu, dc.chain(700, 4, interleaved=True), 1.0, 2, "euclidean")
    assert got.labels.cpu().tolist() == [0, 1] * 350 and got.sizes.cpu().tolist() == [350, 350]


def test_one_dense_cluster_is_the_highest_contention_on_parent():
    """n = 4096 rows all within eps of each other: every pair is a union"""
    from node2vec_amd import cluster

    rng = np.random.default_rng(4)
    X = (rng.integers(-8, 9, (4096, 16)) / 16.0).astype(np.float32)
    for metric, eps in (("euclidean", 100.0), ("cosine", 2.5)):
        got = cluster.dbscan(torch.from_numpy(X).cuda(), eps, 5, metric)
        assert got.n_clusters == 1 and bool((got.labels == 0).all()) and bool((got.counts == 4096).all())
        assert bool(got.core_mask.all()) and got.sizes.cpu().tolist() == [4096]


def test_contested_border_cases_among_far_away_noise(cpu):
    rng = np.random.default_rng(6)
    for X, eps, min_samples, labels in dc.CONTESTED:
        far = (1000.0 + 10.0 * np.arange(300 - len(X)))[:, None] * np.array([[1.0, -1.0]])
        order = rng.permutation(300)
        padded = np.concatenate([X, far.astype(np.float32)])
        got, want = _check(cpu, padded, eps, min_samples, "euclidean")
        assert want.labels[:len(X)].tolist() == labels and (want.labels[len(X):] == -1).all()
        sk_labels, sk_core = dc.sklearn_dbscan(padded, eps, min_samples, "euclidean")
        assert np.array_equal(sk_labels, want.labels) and np.array_equal(sk_core, want.core)
        # the same rows in another order: the same partition, renumbered by the lowest core row
        got2, want2 = _check(cpu, padded[order], eps, min_samples, "euclidean")
        sk2, _ = dc.sklearn_dbscan(padded[order], eps, min_samples, "euclidean")
        assert np.array_equal(sk2, want2.labels)


@pytest.mark.parametrize("metric", METRICS)
def test_min_samples_extremes_duplicates_and_zero_rows(cpu, metric):
    X, eps = _random_case(130, 20, 77)
    X[10:20] = X[9]          # ten duplicates
    X[40] = X[41] = 0.0      # zero rows: at cosine distance 1 from everything, at Euclidean distance 0 from each other
    n = len(X)
    got, want = _check(cpu, X, eps[metric], 1, metric)
    assert bool(got.core_mask.all()) and bool((got.labels >= 0).all())  # every row is core
    got, want = _check(cpu, X, eps[metric], n + 1, metric)
    assert got.n_clusters == 0 and bool((got.labels == -1).all()) and got.sizes.numel() == 0
    got, want = _check(cpu, X, eps[metric], 5, metric)
    assert bool((got.counts[9:20] >= 11).all()) and len(set(got.labels[9:20].cpu().tolist())) == 1
    if metric == "cosine":
        assert got.counts[40].item() == got.counts[41].item() == 1  # 1 <= eps is false for every eps below 1
        got, _ = _check(cpu, X, 1.0, 5, metric)  # and at eps = 1 a zero row is within eps of every row
        assert got.counts[40].item() == n
    got, _ = _check(cpu, X, 0.0, 2, metric)  # eps = 0: the duplicates alone (Euclidean: exactly; cosine: as rounded)
    assert got.counts[40].item() == (2 if metric == "euclidean" else 1)


BLOBS = {}


def _blobs(cpu, metric, dim):
    """n = 5000: three blobs and 500 rows of noise, gapped by construction; the restatement and scikit-learn computed
    once and shared by the block caps"""
    key = (metric, dim)
    if key not in BLOBS:
        if metric == "euclidean":
            X, eps = dc.dyadic_blobs(1500, 500, dim, 3 + dim, *((500, 1 / 16) if dim == 16 else (1100, 1 / 8)))
        else:
            X, eps = dc.cosine_blobs(1500, 500, dim, 5 + dim, 0.02, sigma=0.01)
        min_samples = 300
        want = dc.restated(cpu, X, eps, min_samples, metric)
        sk_labels, sk_core = dc.sklearn_dbscan(X, eps, min_samples, metric)
        assert np.array_equal(sk_labels, want.labels) and np.array_equal(sk_core, want.core)
        assert want.n_clusters == 3 and (want.labels == -1).sum() >= 200
        if metric == "euclidean":
            assert (~want.core & (want.labels >= 0)).sum() >= 100  # border rows
        BLOBS[key] = (X, eps, min_samples, want)
    return BLOBS[key]


@pytest.mark.parametrize("max_blocks", [0, 1, 7])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [16, 130])
def test_blobs_and_noise_are_sklearn_on_every_launch_geometry(cpu, dim, metric, max_blocks):
    X, eps, min_samples, want = _blobs(cpu, metric, dim)
    _check(cpu, X, eps, min_samples, metric, want=want, max_blocks=max_blocks)


@pytest.mark.parametrize("metric", METRICS)
def test_neighbor_counts_alone_are_the_restated_counts(cpu, metric):
    from node2vec_amd import cluster

    X, eps = _random_case(300, 33, 9)
    want = dc.restated(cpu, X, eps[metric], 1, metric)
    for max_blocks in (0, 3):
        got = cluster.neighbor_counts(_device(X), eps[metric], metric, max_blocks=max_blocks)  # its own inv_norm
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want.counts)


def test_the_python_layer_on_the_device():
    from node2vec_amd import cluster

    X = torch.zeros((0, 8), device="cuda")
    res = cluster.dbscan(X, 0.5)
    assert res.n_clusters == 0 and res.labels.shape == (0,) and res.sizes.shape == (0,)
    assert cluster.neighbor_counts(X, 0.5).shape == (0,)
    bad = torch.ones((4, 8), device="cuda")
    bad[2, 3] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        cluster.dbscan(bad, 0.5)
    with pytest.raises(ValueError, match="float32"):
        cluster.dbscan(torch.ones((4, 8), device="cuda", dtype=torch.float64), 0.5)


def test_labels_go_into_the_silhouette_unchanged(cpu):
    from node2vec_amd import cluster

    X, eps = dc.dyadic_blobs(70, 50, 16, 11 * 16, 500)
    Xd = _device(X)
    res = cluster.dbscan(Xd, eps, 8)
    assert res.n_clusters >= 2 and bool((res.labels == -1).any())
    sil = cluster.silhouette_samples(Xd, res.labels, "euclidean", k=res.n_clusters)
    noise = (res.labels == -1)
    assert bool(torch.isnan(sil.s[noise]).all()) and bool(torch.isfinite(sil.s[~noise]).all())
    assert torch.equal(sil.counts, res.sizes)
    assert cluster.silhouette_score(Xd, res.labels) > 0.3  # blobs: the clustering is a good one


def test_front_ends_are_cluster_dbscan_on_the_same_vectors():
    from node2vec_amd import cluster, similarity
    from node2vec_amd.embedding import HipW2V, KeyedVectors, Node2VecHIP

    X, _ = dc.cosine_blobs(40, 20, 12, 3, 0.06)
    Xe, eps_e = dc.dyadic_blobs(40, 20, 12, 3, 300)
    for vectors, metric, eps in ((X, "cosine", 0.06), (Xe, "euclidean", eps_e)):
        ids = np.arange(len(vectors)) + 100
        wv = KeyedVectors(ids, vectors)
        Xd = torch.from_numpy(vectors).cuda()
        want = cluster.dbscan(Xd, eps, 4, metric, inv_norm=similarity.inv_norms(Xd) if metric == "cosine" else None)
        assert want.n_clusters >= 2
        got = wv.dbscan(eps, 4, metric=metric)
        for name in ("labels", "core_mask", "counts", "sizes"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (metric, name)
        assert got.n_clusters == want.n_clusters
        part = wv.dbscan(eps, 4, metric=metric, restrict_vocab=50)
        assert part.labels.shape == (50,)
        n2v = Node2VecHIP(pd.DataFrame.from_dict({"walk": [[100, 101]]}), {})
        n2v.model = HipW2V(wv, np.zeros_like(vectors), {}, 0)
        frame = n2v.dbscan(eps, 4, metric=metric)
        assert list(frame.columns) == ["id", "cluster"] and frame["id"].tolist() == ids.tolist()
        assert frame["cluster"].tolist() == want.labels.cpu().tolist()
        assert torch.equal(n2v.dbscan_result.labels, want.labels)
    assert wv.dbscan(eps_e, 4).n_clusters >= 0  # the default metric is cosine, as for kmeans
