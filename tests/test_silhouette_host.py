"""Silhouette scores (node2vec_amd/cluster.py, csrc/n2v_silhouette.hip), the parts that need no GPU: the CPU
restatement (tests/cpu_silhouette/n2v_silhouette_cpu.c) against a brute-force float64 silhouette within bounds
derived from the fp32 unit roundoff, against the cosine sum's linear identity, and on the definition's edges worked
by hand; the C ABI's argument checks, the header and the binding, and the Python layer's checks and sampling."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import silhouette_cases as sc
from conftest import ROOT


@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def cpu(tmp_path_factory):
    return sc.build(tmp_path_factory.mktemp("silhouette_cpu"))


CASES = [(200, 3, 4), (300, 16, 7), (257, 33, 16), (150, 100, 5), (120, 129, 33)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("n,dim,k", CASES)
def test_restated_silhouette_is_the_float64_one_within_the_rounding_bound(cpu, n, dim, k, metric):
    """Every fp32 distance is within sc.distance_bound of the exact one (derived there from U = 2^-24, dim_pad and
    the magnitudes; the rows are at least 0.5 apart, which bounds what the square root amplifies).  A mean of
    distances is then within the mean of their bounds (sc.mean_bounds): Ba for a; for b, a minimum of means, the
    largest bound Bb of the candidates.  s = f(a, b) = (b - a) / max(a, b) has |df/da|, |df/db| <= 1 / max(a, b),
    and max(a, b) moves by at most Ba + Bb, so |s' - s| <= (Ba + Bb) / (max(a, b) - Ba - Bb), plus four fp64
    roundings.  nearest is the float64 one wherever the float64 gap between the best and the second best mean
    exceeds twice the bound; at most 5 % of the rows may lie inside it."""
    X, labels = sc.lattice_case(n, dim, k, 13 * dim + k)
    got = sc.restated(cpu, X, labels, k, metric)
    s, a, b, nearest, means, D = sc.brute(X, labels, k, metric)
    if metric == "euclidean":
        apart = D[~np.eye(n, dtype=bool)].min()
        assert apart >= 0.5, apart  # the inputs' own property, in float64
    E = sc.distance_bound(X, metric, D)
    B = sc.mean_bounds(E, labels, k)
    Ba = B[np.arange(n), labels]
    other = np.where(np.isnan(means), -np.inf, B)
    Bb = other.max(1)
    assert np.array_equal(got.counts, np.bincount(labels, minlength=k))
    mx = np.maximum(a, b)
    scored = np.isfinite(b)
    assert scored.all()  # every row has a cluster and another one to compare with
    Bs = np.where(s == 0.0, 0.0, (Ba + Bb) / (mx - Ba - Bb) + 4 * 2.0 ** -53)
    ea, eb, es = np.abs(got.a - a), np.abs(got.b - b), np.abs(got.s - s)
    print(f"{metric} n={n} dim={dim} k={k}: error / bound  a {np.max(ea[Ba > 0] / Ba[Ba > 0]):.3f}  "
          f"b {np.max(eb / Bb):.3f}  s {np.max(es[Bs > 0] / Bs[Bs > 0]):.3f}  "
          f"(bounds a {Ba.max():.2e} b {Bb.max():.2e} s {Bs.max():.2e})")
    assert (ea <= Ba).all() and (eb <= Bb).all() and (es <= Bs).all()
    order = np.sort(np.where(np.isnan(means), np.inf, means), axis=1)
    decided = (order[:, 1] - order[:, 0]) > 2.0 * Bb
    assert (~decided).sum() <= 0.05 * n, (~decided).sum()  # the float64 reference itself: the inputs are fit
    assert np.array_equal(got.nearest[decided], nearest[decided])


@pytest.mark.parametrize("n,dim,k", CASES)
def test_restated_cosine_sums_are_the_linear_identity(cpu, n, dim, k):
    """S(i, c) = n_c' - inv_i dot(x_i, sum over j in c, j != i, of x_j / |x_j|) in float64, n_c' the rows summed:
    n_c' distances, each within the cosine bound of sc.distance_bound"""
    X, labels = sc.normal_case(n, dim, k, 7 * dim + k)
    X[3] = 0.0  # a zero row: at distance 1 from everything, on both sides
    got = sc.restated(cpu, X, labels, k, "cosine", sums=True)
    X64 = X.astype(np.float64)
    norm = np.sqrt((X64 ** 2).sum(1))
    inv = np.divide(1.0, norm, out=np.zeros_like(norm), where=norm > 0)
    unit = X64 * inv[:, None]
    E = 2.0 * sc.gamma((dim + 15) // 16 * 16 + 2 * (dim + 8) + 4)
    worst = 0.0
    for c in range(k):
        col = labels == c
        total = unit[col].sum(0)
        for i in range(n):
            own = labels[i] == c
            cnt = int(col.sum()) - int(own)
            want = cnt - unit[i] @ (total - (unit[i] if own else 0.0))
            tol = cnt * E * (1.0 + 2.0 ** -40)
            err = abs(got.sums[i, c] - want)
            worst = max(worst, err / tol if tol else err)
            assert err <= tol, (i, c, err, tol)
    print(f"cosine identity n={n} dim={dim} k={k}: largest error / bound {worst:.3f}")


def test_definition_edges_worked_by_hand(cpu):
    """integer rows whose distances are exact (3-4-5): a singleton, an exact tie of two clusters' means, a
    duplicate in another cluster, an empty id inside [0, k), rows of no cluster"""
    X = np.array([[0, 0], [3, 4], [0, 0], [6, 8], [0, 0], [100, 0]], np.float32)
    labels = np.array([0, 0, 1, 3, -1, 7], np.int32)
    got = sc.restated(cpu, X, labels, 4, "euclidean", sums=True)
    assert got.counts.tolist() == [2, 1, 0, 1]
    # row 0: a = 5; cluster 1 is its duplicate (mean 0), cluster 3 at 10.  row 1: clusters 1 and 3 both at 5: 1 wins
    # rows 2, 3: alone in their clusters, s = 0, b from cluster 0: (0 + 5) / 2 and (10 + 5) / 2
    assert got.a[:4].tolist() == [5.0, 5.0, 0.0, 0.0]
    assert got.b[:4].tolist() == [0.0, 5.0, 2.5, 7.5]
    assert got.s[:4].tolist() == [-1.0, 0.0, 0.0, 0.0]
    assert got.nearest.tolist() == [1, 1, 0, 0, -1, -1]
    assert np.isnan(got.a[4:]).all() and np.isnan(got.b[4:]).all() and np.isnan(got.s[4:]).all()
    assert got.sums[1].tolist() == [5.0, 5.0, 0.0, 5.0] and got.sums[0].tolist() == [5.0, 0.0, 0.0, 10.0]
    # asked for by row number: repeats, any order, a row of no cluster, numbers that are no rows
    rows = np.array([3, 0, 0, 5, -1, 6, 1 << 40, 1], np.int64)
    part = sc.restated(cpu, X, labels, 4, "euclidean", rows=rows)
    for q, r in enumerate(rows):
        if 0 <= r < 4:
            assert (part.a[q], part.b[q], part.s[q], part.nearest[q]) == (got.a[r], got.b[r], got.s[r], got.nearest[r])
        else:
            assert np.isnan([part.a[q], part.b[q], part.s[q]]).all() and part.nearest[q] == -1
    assert np.array_equal(part.counts, got.counts)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_duplicate_rows_and_a_lone_cluster(cpu, metric):
    X = np.array([[2, 0]] * 4, np.float32)  # inv_norm = 0.5 and every product exact: all distances are 0
    got = sc.restated(cpu, X, np.array([0, 0, 1, 1], np.int32), 2, metric)
    assert got.a.tolist() == [0.0] * 4 and got.b.tolist() == [0.0] * 4 and got.s.tolist() == [0.0] * 4
    assert got.nearest.tolist() == [1, 1, 0, 0]
    # one cluster with rows: nothing to compare with
    X = np.array([[2, 0], [0, 2], [4, 0]], np.float32)
    got = sc.restated(cpu, X, np.array([1, 1, 1], np.int32), 3, metric)
    assert got.s.tolist() == [0.0] * 3 and got.nearest.tolist() == [-1] * 3 and np.isinf(got.b).all()
    assert got.counts.tolist() == [0, 3, 0]


def test_cosine_by_hand_with_a_zero_row(cpu):
    X = np.array([[1, 0], [0, 2], [-4, 0], [0, 0]], np.float32)  # norms 1, 2, 4: every inv_norm and product exact
    got = sc.restated(cpu, X, np.array([0, 0, 1, 1], np.int32), 2, "cosine")
    # row 0: a = d(0, 1) = 1; b = (d(0, 2) + d(0, zero)) / 2 = (2 + 1) / 2
    assert got.a[0] == 1.0 and got.b[0] == 1.5 and got.s[0] == (1.5 - 1.0) / 1.5
    # the zero row is at 1 from everything: a = 1, b = 1, s = 0
    assert got.a[3] == 1.0 and got.b[3] == 1.0 and got.s[3] == 0.0


def test_the_list_pads_every_segment_to_tiles_of_one_cluster(cpu):
    labels = sc.sized_labels([1, 15, 16, 17, 0, 31, 33], extra_none=5, seed=2)
    counts, seg_off, lst = sc.row_list(cpu, labels, 7)
    assert counts.tolist() == [1, 15, 16, 17, 0, 31, 33]
    assert seg_off.tolist() == [0, 16, 32, 48, 80, 80, 112, 160]
    for c in range(7):
        seg = lst[seg_off[c]:seg_off[c + 1]]
        assert seg[:counts[c]].tolist() == np.nonzero(labels == c)[0].tolist()  # ascending rows
        assert (seg[counts[c]:] == -1).all()


def test_a_row_scores_the_same_bits_whatever_comes_with_it(cpu):
    X, labels = sc.normal_case(90, 20, 5, 4)
    labels[::11] = -1
    for metric in ("euclidean", "cosine"):
        full = sc.restated(cpu, X, labels, 5, metric)
        rows = np.array([70, 3, 3, 11, 89, 0], np.int64)
        part = sc.restated(cpu, X, labels, 5, metric, rows=rows)
        for name in ("s", "a", "b"):
            assert sc.same_bits(getattr(part, name), getattr(full, name)[rows]), (metric, name)
        assert np.array_equal(part.nearest, full.nearest[rows])


def test_silhouette_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; n == 0 or m == 0 is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    big = 1 << 40

    def call(X=p, inv=p, n=10, dim=16, labels=p, k=4, metric=1, rows=p, m=5, a=p, b=p, s=p, nearest=p, counts=p,
             ws=p, ws_bytes=big):
        return lib.n2v_silhouette(X, inv, n, dim, labels, k, metric, rows, m, a, b, s, nearest, counts, ws, ws_bytes,
                                  None)

    assert call(n=0, m=0) == _lib.OK and call(n=0, m=0, rows=None) == _lib.OK and call(m=0) == _lib.OK
    assert call(n=0, m=0, dim=1024, k=1024) == _lib.OK and call(n=0, m=0, metric=0, inv=None) == _lib.OK
    need = lib.n2v_silhouette_workspace_bytes(10, 16, 4, 5)
    assert need > 0
    for kw in (dict(dim=0), dict(dim=1025), dict(k=0), dict(k=1025), dict(n=-1), dict(n=1 << 31), dict(m=-1),
               dict(m=1 << 31), dict(metric=-1), dict(metric=2), dict(inv=None), dict(rows=None),  # m != n
               dict(X=None), dict(labels=None), dict(a=None), dict(b=None), dict(s=None), dict(nearest=None),
               dict(ws=None), dict(ws=p + 4), dict(ws_bytes=0), dict(ws_bytes=need - 1)):
        assert call(**kw) == _lib.EINVAL, kw
    for kw in (dict(dim=0), dict(k=1025), dict(metric=2), dict(inv=None)):
        assert call(n=0, m=0, **kw) == _lib.EINVAL, kw  # refused before the empty input returns
    # the size query: -1 for what the call refuses, 0 for nothing to do, the documented parts otherwise
    q = lib.n2v_silhouette_workspace_bytes
    assert q(10, 0, 4, 5) == q(10, 16, 0, 5) == q(10, 16, 1025, 5) == q(-1, 16, 4, 5) == q(10, 16, 4, -1) == -1
    assert q(0, 16, 4, 0) == 0 and q(10, 16, 4, 0) == 0

    def up(x):
        return (x + 255) // 256 * 256

    for n, dim, k, m in ((10, 16, 4, 5), (1000, 100, 17, 1000), (10 ** 6, 128, 1024, 4096), (2 ** 31 - 1, 1, 1, 1)):
        slab = (max(1, -(-n // 2048)) + 1023) // 1024 * 1024
        want = (up((m + 63) // 64 * 64 * ((dim + 15) // 16 * 16) * 4) + up(4 * n) + up(4 * k * -(-n // slab)) +
                up(4 * k) + up(8 * (k + 1)) + up(4 * (n + 16 * k)))
        assert q(n, dim, k, m) == want, (n, dim, k, m)


def test_header_and_binding_name_the_silhouette_entry_points(lib):
    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("n2v_silhouette_workspace_bytes", "n2v_silhouette"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code) and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15


def test_python_layer_checks_its_arguments_before_the_gpu():
    """on host tensors: the message names the bad argument, so it was found before the device check"""
    from node2vec_amd import cluster

    X = torch.zeros((10, 8))
    labels = torch.tensor([0, 1] * 5)
    for call in (cluster.silhouette_samples, cluster.silhouette_score):
        with pytest.raises(ValueError, match="metric"):
            call(X, labels, metric="manhattan")
        with pytest.raises(ValueError, match=r"labels must be a \[10\] tensor"):
            call(X, labels[:9])
        with pytest.raises(ValueError, match="labels must be integers"):
            call(X, labels.float())
        for k in (0, -1, 1025):
            with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
                call(X, labels, k=k)
        with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
            call(X, labels * 5000)  # k = labels.max() + 1
        with pytest.raises(ValueError, match="HIP device"):  # everything else was fine: no CPU path
            call(X, labels)
    with pytest.raises(ValueError, match="rows must be"):
        cluster.silhouette_samples(X, labels, rows=torch.zeros(3))
    for lone in (torch.zeros(10, dtype=torch.int32), torch.full((10,), -1), torch.tensor([3] * 9 + [-1])):
        with pytest.raises(ValueError, match="at least two clusters"):
            cluster.silhouette_score(X, lone)
    with pytest.raises(ValueError, match="at least two clusters"):
        cluster.silhouette_score(X, labels, k=1)  # label 1 is no cluster of k = 1
    with pytest.raises(ValueError, match="sample_size"):
        cluster.silhouette_score(X, labels, sample_size=0)


def test_the_sample_is_seeded_without_replacement_and_of_clustered_rows():
    from node2vec_amd import cluster

    rng = np.random.default_rng(0)
    labels = torch.from_numpy(rng.integers(-1, 6, 500).astype(np.int32))  # 5 is no cluster of k = 5
    have = np.nonzero((labels.numpy() >= 0) & (labels.numpy() < 5))[0]
    a = cluster.sample_rows(labels, 5, 100, seed=3)
    assert torch.equal(a, cluster.sample_rows(labels, 5, 100, seed=3))
    assert not torch.equal(a, cluster.sample_rows(labels, 5, 100, seed=4))
    assert a.dtype == torch.int64 and len(a) == 100 and len(set(a.tolist())) == 100 and set(a.tolist()) <= set(have)
    want = np.sort(have[np.random.default_rng(3).choice(len(have), size=100, replace=False)])
    assert a.tolist() == want.tolist()
    assert cluster.sample_rows(labels, 5, None) is None and cluster.sample_rows(labels, 5, len(have)) is None


def test_model_classes_refuse_silhouette_before_fit_and_before_cluster():
    import pandas as pd

    from node2vec_amd.embedding import HipW2V, KeyedVectors, Node2VecHIP

    walks = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4]]})
    n2v = Node2VecHIP(walks, {})
    with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
        n2v.silhouette()
    n2v.model = HipW2V(KeyedVectors(np.arange(5), np.ones((5, 4), np.float32)), np.zeros((5, 4), np.float32), {}, 0)
    with pytest.raises(ValueError, match="Please run cluster()"):
        n2v.silhouette()
    assert n2v.silhouette_score is None
