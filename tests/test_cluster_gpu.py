"""k-means on the GPU (csrc/n2v_kmeans.hip through node2vec_amd.cluster) against its CPU restatement,
tests/cpu_kmeans/n2v_kmeans_cpu.c, bit for bit: labels and counts with array_equal, distances and centroids by
their bit patterns.  The shapes sit on the kernel's edges: both load paths (dim % 4, base alignment), a ragged
last 16-block and a ragged batch of eight loads (dim), the edges of a centroid tile (16, 64) and of the loop over
tiles (k), a ragged wave, step and slab (n)."""
import numpy as np
import pandas as pd
import pytest
import torch

import kmeans_cases as kc
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return kc.build(tmp_path_factory.mktemp("kmeans_cpu"))


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


def _check_assign(cpu, X, Cm, metric, aligned=True):
    from node2vec_amd import cluster

    inv = kc.inv_norms(cpu, X)
    Cu = kc.unit(cpu, Cm) if metric == "cosine" else Cm
    want_l, want_d = kc.assign(cpu, X, inv, Cu, metric)
    got_l, got_d = cluster.assign(_device(X, aligned), _device(Cu), metric, inv_norm=_device(inv))
    got_l, got_d = got_l.cpu().numpy(), got_d.cpu().numpy()
    bad = np.nonzero(got_l != want_l)[0]
    assert len(bad) == 0, (metric, aligned, bad[:5], got_l[bad[:5]], want_l[bad[:5]])
    assert kc.same_bits(got_d, want_d), (metric, aligned)
    return got_l


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 4, 15, 16, 17, 64, 100, 128, 129, 256, 1000, 1024])
def test_assign_bitwise_over_the_dimensions(cpu, dim, metric):
    for k, aligned in ((15, True), (17, True), (17, False)):
        X, Cm = kc.normal_case(81, dim, k, 31 * dim + k)
        X[5] = 0.0
        _check_assign(cpu, X, Cm, metric, aligned)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 63, 64, 65, 1024])
def test_assign_bitwise_over_the_centroid_tiles(cpu, k, metric):
    for dim in (64, 17):
        X, Cm = kc.normal_case(65, dim, k, 7 * k + dim)
        Cm[k - 1] = Cm[0]  # an exact tie of the first and the last centroid, for both metrics: the first wins
        labels = _check_assign(cpu, X, Cm, metric)
        assert k == 1 or not (labels == k - 1).any()


def _three_slabs_and_a_tail(dim, k):
    from node2vec_amd import cluster

    slab = cluster.slab_rows(300, dim, k)  # read from the library
    n = 3 * slab + 37
    assert cluster.slab_rows(n, dim, k) == slab and n // slab == 3 and n % slab
    return n


@pytest.mark.parametrize("metric", METRICS)
def test_assign_bitwise_over_the_row_counts(cpu, metric):
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 257, _three_slabs_and_a_tail(20, 18)):
        X, Cm = kc.normal_case(n, 20, 18, n)
        _check_assign(cpu, X, Cm, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [5, 64])
def test_assign_bitwise_on_signed_zeros_denormals_and_inf(cpu, dim, metric):
    X = kc.special_rows(dim, dim)
    _, Cm = kc.normal_case(1, dim, 20, dim + 1)
    Cm[3] = 0.0
    Cm[4] = X[10]
    for aligned in (True, False):
        labels = _check_assign(cpu, X, Cm, metric, aligned)
        assert labels[9] == -1  # the NaN row


@pytest.mark.parametrize("metric", METRICS)
def test_the_best_centroid_at_every_tile_edge(cpu, metric):
    """row i is centroid place[i] itself: it wins wherever it sits in the tiles of 64 and the groups of 16"""
    place = [0, 15, 16, 63, 64, 65, 127, 128, 129]
    _, Cm = kc.normal_case(1, 48, 130, 9)
    X = Cm[place].copy()
    labels = _check_assign(cpu, X, Cm, metric)
    assert labels.tolist() == place


def _skewed_labels(n, k, kind, rng):
    if kind == "one":
        return np.full(n, k - 1, np.int32)
    labels = rng.integers(0, k, n).astype(np.int32)
    labels[labels == 1] = 0            # cluster 1 is empty
    labels[labels == 2] = 3 % k        # cluster 2 has one member, in the last slab
    labels[n - 2] = 2
    labels[rng.integers(0, n, n // 10)] = -1
    labels[:3] = (k, -7, 1 << 30)      # not labels: as -1
    return labels


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,k,big", [(3, 5, False), (64, 5, False), (260, 17, False), (8, 4, True)])
def test_update_bitwise_on_skewed_labels(cpu, dim, k, big, metric):
    from node2vec_amd import cluster

    n = 150001 if big else _three_slabs_and_a_tail(dim, k)  # big: slabs of more than one step of 64 rows
    if big:
        assert cluster.slab_rows(n, dim, k) > 64 and n // cluster.slab_rows(n, dim, k) >= 3
    rng = np.random.default_rng(dim + k)
    X, prev = kc.normal_case(n, dim, k, dim * k)
    inv = kc.inv_norms(cpu, X)
    for kind in ("one", "skewed"):
        labels = _skewed_labels(n, k, kind, rng)
        want_c, want_n = kc.update(cpu, X, inv, labels, k, metric, prev)
        for aligned in (True, False):
            got_c, got_n = cluster.update(_device(X, aligned), torch.from_numpy(labels).cuda(), k, metric,
                                          _device(prev), inv_norm=_device(inv))
            assert np.array_equal(got_n.cpu().numpy(), want_n), (kind, aligned)
            assert kc.same_bits(got_c.cpu().numpy(), want_c), (kind, aligned)
        if kind == "skewed":
            assert want_n[1] == 0 and want_n[2] == 1
            assert kc.same_bits(want_c[1], prev[1])


def _step(X, inv, Cm, metric, labels):
    """n2v_kmeans_step through the binding -> (labels, dist, centroids, counts, stats), device tensors"""
    from node2vec_amd import _lib, cluster

    L = _lib.load()
    n, dim = X.shape
    k = Cm.shape[0]
    labels = labels.clone()
    dist = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.empty_like(Cm)
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    ws = cluster.alloc_workspace(n, dim, k, X.device)
    _lib.check(L.n2v_kmeans_step(X.data_ptr(), None if inv is None else inv.data_ptr(), n, dim, Cm.data_ptr(), k,
                                 cluster.METRICS[metric], labels.data_ptr(), dist.data_ptr(), out.data_ptr(),
                                 counts.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _lib.current_stream_ptr()), "n2v_kmeans_step")
    return labels, dist, out, counts, stats


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,dim,k", [(229, 20, 18), (229, 64, 3), (150001, 8, 4), (1000, 129, 65)])
def test_step_is_assign_then_update_and_the_same_twice(cpu, n, dim, k, metric):
    from node2vec_amd import cluster

    X, Cm = kc.normal_case(n, dim, k, n + dim + k)
    X[n // 2] = np.nan
    inv = kc.inv_norms(cpu, X)
    Cu = kc.unit(cpu, Cm) if metric == "cosine" else Cm
    prev = np.random.default_rng(1).integers(-1, k, n).astype(np.int32)
    Xd, invd, Cd, prevd = _device(X), _device(inv), _device(Cu), torch.from_numpy(prev).cuda()
    labels, dist, out, counts, stats = _step(Xd, invd, Cd, metric, prevd)
    a_l, a_d = cluster.assign(Xd, Cd, metric, inv_norm=invd)
    u_c, u_n = cluster.update(Xd, a_l, k, metric, Cd, inv_norm=invd)
    assert torch.equal(labels, a_l) and torch.equal(counts, u_n)
    assert kc.same_bits(dist.cpu().numpy(), a_d.cpu().numpy()) and kc.same_bits(out.cpu().numpy(), u_c.cpu().numpy())
    assert stats.tolist() == [int((labels != prevd).sum()), int((labels < 0).sum())] and stats[1] >= 1
    # the restatement
    w_l, w_d, w_c, w_n, w_s = kc.step(cpu, X, inv, Cu, metric, prev)
    assert np.array_equal(labels.cpu().numpy(), w_l) and np.array_equal(counts.cpu().numpy(), w_n)
    assert kc.same_bits(dist.cpu().numpy(), w_d) and kc.same_bits(out.cpu().numpy(), w_c)
    assert stats.tolist() == w_s.tolist()
    # the same call twice
    again = _step(Xd, invd, Cd, metric, prevd)
    assert torch.equal(again[0], labels) and torch.equal(again[3], counts) and torch.equal(again[4], stats)
    assert torch.equal(again[2].view(torch.int32), out.view(torch.int32))


def test_exact_by_construction_past_32_bit_offsets():
    """n dim > 2^31 elements: every row is one of k integer-valued centroids, so every dot, partial sum (at most
    slab_rows * 8 < 2^24) and mean is exact; the planted labels and the centroids come back exactly, the rows past
    element 2^31 included"""
    from node2vec_amd import cluster

    n, dim, k = (1 << 23) + 5, 260, 4
    assert n * dim > 1 << 31 and cluster.slab_rows(n, dim, k) * 8 < 1 << 24
    gen = torch.Generator(device="cuda").manual_seed(3)
    Cm = torch.randint(-8, 9, (k, dim), generator=gen, device="cuda").float()
    Cm[:, 0] = torch.arange(k, device="cuda") * 4.0 - 6.0  # distinct
    r = torch.arange(n, device="cuda")
    planted = ((r * 7 + r // 1000) % k).to(torch.int32)
    planted[-3:] = torch.tensor([3, 0, 2], dtype=torch.int32, device="cuda")
    X = Cm[planted.long()]
    del r
    start = Cm + 0.25  # not the answer itself
    labels, dist, out, counts, stats = _step(X, None, start.contiguous(), "euclidean",
                                             torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    assert torch.equal(labels, planted)
    assert torch.equal(out, Cm)
    assert torch.equal(counts, torch.bincount(planted.long(), minlength=k))
    assert stats.tolist() == [n, 0]
    assert torch.equal(dist, torch.full_like(dist, dim * 0.0625))  # 260 / 16: exact


@pytest.mark.parametrize("metric,init", [("euclidean", "k-means++"), ("euclidean", "random"), ("cosine", "k-means++"),
                                         ("cosine", "random")])
def test_kmeans_recovers_planted_blobs_and_equals_the_restated_loop(cpu, metric, init):
    from node2vec_amd import cluster

    X, planted, _ = kc.blobs(2000, 32, 5, 11)
    Xd = _device(X)
    inv = kc.inv_norms(cpu, X)
    seed = 0
    res = None
    for seed in range(8):  # "random" may start two centres in one blob: Lloyd then stops in a local optimum
        C0 = cluster.init_centroids(Xd, 5, metric, seed, init)
        res = cluster.kmeans(Xd, 5, metric=metric, init=init, seed=seed)
        # the restatement's loop from the same initial centroids
        w_c, w_l, w_d, w_it, w_conv = kc.lloyd(cpu, X, inv, C0.cpu().numpy(), metric)
        assert res.n_iter == w_it and res.converged and w_conv
        assert np.array_equal(res.labels.cpu().numpy(), w_l)
        assert kc.same_bits(res.centroids.cpu().numpy(), w_c) and kc.same_bits(res.dist.cpu().numpy(), w_d)
        # Lloyd never raises the float64 inertia of the initial assignment
        first = cluster.assign(Xd, C0, metric)[1].double().sum().item()
        assert res.inertia <= first and res.inertia == res.dist.double().sum().item()
        assert res.n_unassigned == 0 and res.counts.sum().item() == 2000
        again = cluster.kmeans(Xd, 5, metric=metric, init=init, seed=seed)
        assert torch.equal(again.labels, res.labels) and torch.equal(again.centroids, res.centroids)
        assert again.n_iter == res.n_iter and again.inertia == res.inertia
        got = res.labels.cpu().numpy()
        table = {(int(p), int(g)) for p, g in zip(planted, got)}
        if len(table) == 5 and len({g for _, g in table}) == 5:  # a permutation of the planted labels
            break
    else:
        pytest.fail(f"no seed in 0..7 recovered the blobs with init={init}")
    if init == "k-means++":
        assert seed == 0  # D^2 seeding separates blobs this far apart at once


def test_n_init_keeps_the_best_run():
    from node2vec_amd import cluster

    X, _, _ = kc.blobs(600, 8, 6, 5, spread=1.5)
    Xd = _device(X)
    runs = [cluster.kmeans(Xd, 6, init="random", seed=20 + i, max_iter=3) for i in range(3)]
    best = cluster.kmeans(Xd, 6, init="random", seed=20, n_init=3, max_iter=3)
    pick = min(range(3), key=lambda i: (runs[i].inertia, i))
    assert best.inertia == runs[pick].inertia and torch.equal(best.labels, runs[pick].labels)
    assert not best.converged or best.n_iter <= 3


def test_keyedvectors_kmeans_on_host_and_device_vectors():
    from node2vec_amd import cluster
    from node2vec_amd.embedding import KeyedVectors

    X, _, _ = kc.blobs(300, 16, 3, 2)
    ids = np.arange(1000, 1300)
    host = KeyedVectors(ids, X).kmeans(3, seed=4)
    dev = KeyedVectors(ids, _device(X)).kmeans(3, seed=4)
    direct = cluster.kmeans(_device(X), 3, metric="cosine", seed=4)
    for res in (host, dev):
        assert torch.equal(res.labels, direct.labels) and torch.equal(res.centroids, direct.centroids)
        assert res.labels.shape == (300,) and res.converged
    part = KeyedVectors(ids, X).kmeans(3, metric="euclidean", restrict_vocab=100, seed=4)
    want = cluster.kmeans(_device(X[:100]), 3, metric="euclidean", seed=4)
    assert part.labels.shape == (100,) and torch.equal(part.labels, want.labels)
    assert torch.equal(part.centroids, want.centroids)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_model_classes_cluster_their_vocabulary():
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    X, planted, _ = kc.blobs(40, 8, 2, 6)
    ids = np.arange(40)[::-1] + 100  # vocabulary order is not id order
    names = pd.DataFrame({"id": list(ids) + [139, 500], "name": [f"v{i}" for i in ids] + ["last", "unused"]})
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((40, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((39, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.cluster(2)
        n2v.model = model(KeyedVectors(ids, X))
        df = n2v.cluster(2, seed=1)
        assert list(df.columns) == ["id", "cluster"] and df["id"].tolist() == ids.tolist()
        got = df["cluster"].to_numpy()
        assert set(got) == {0, 1} and len({(int(p), int(g)) for p, g in zip(planted, got)}) == 2
        assert n2v.clusters is df and torch.equal(n2v.kmeans_result.labels.cpu(), torch.from_numpy(got))
        assert n2v.cluster(2, metric="euclidean", seed=1)["cluster"].isin([0, 1]).all()
        n2v.name_id = names
        named = n2v.cluster(2, seed=1)
        assert list(named.columns) == ["name", "cluster"] and named["cluster"].tolist() == got.tolist()
        assert named["name"].tolist() == ["last"] + [f"v{i}" for i in ids[1:]]  # id 139: its last name wins
        n2v.name_id = names[names["id"] != 105]
        with pytest.raises(KeyError):
            n2v.cluster(2)
