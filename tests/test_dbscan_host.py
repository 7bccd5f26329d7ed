"""DBSCAN (node2vec_amd/cluster.py, csrc/n2v_dbscan.hip), the parts that need no GPU: the CPU restatement
(tests/cpu_dbscan/n2v_dbscan_cpu.c) against scikit-learn's brute-force DBSCAN and a float64 brute force, labels and
core set exactly, on gapped cases and on integer grids where distances sit exactly on eps; the contested-border
cases; the pair test's symmetry bit for bit; csrc/n2v_unionfind.h compiled into a stand-alone host program against
scipy's connected components; the C ABI's argument checks and the Python layer's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dbscan_cases as dc
from conftest import ROOT


@pytest.fixture(scope="session")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def cpu(tmp_path_factory):
    return dc.build(tmp_path_factory.mktemp("dbscan_cpu"))


def _agree(cpu, X, eps, min_samples, metric, sklearn_too=True):
    got = dc.restated(cpu, X, eps, min_samples, metric)
    want = dc.brute(X, eps, min_samples, metric)
    what = (metric, X.shape, eps, min_samples)
    assert np.array_equal(got.counts, want.counts), what
    assert np.array_equal(got.core, want.core), what
    assert np.array_equal(got.labels, want.labels) and got.n_clusters == want.n_clusters, what
    if sklearn_too:
        labels, core = dc.sklearn_dbscan(X, eps, min_samples, metric)
        assert np.array_equal(got.core, core), what
        assert np.array_equal(got.labels, labels), what
    return got


@pytest.mark.parametrize("dim,steps,quantum", [(1, 2, 1 / 16), (3, 40, 1 / 16), (16, 500, 1 / 16), (17, 560, 1 / 16),
                                               (130, 1100, 1 / 8)])
def test_restatement_is_sklearn_and_the_brute_force_on_gapped_blobs(cpu, dim, steps, quantum):
    X, eps = dc.dyadic_blobs(70, 50, dim, 11 * dim, steps, quantum)
    for min_samples in (3, 8):
        got = _agree(cpu, X, eps, min_samples, "euclidean")
    assert dim == 1 or (got.n_clusters >= 2 and (got.labels == -1).any())  # (min_samples = 8)


@pytest.mark.parametrize("dim", [3, 16, 17, 130])
def test_restatement_is_sklearn_and_the_brute_force_on_gapped_cosine_bundles(cpu, dim):
    X, eps = dc.cosine_blobs(70, 50, dim, 5 * dim, 0.06)
    for min_samples in (3, 8):
        got = _agree(cpu, X, eps, min_samples, "cosine")
    assert got.n_clusters >= 2


@pytest.mark.parametrize("eps", [1.0, 2.0])
def test_restatement_is_sklearn_on_integer_grids_with_distances_on_the_boundary(cpu, eps):
    """everything is exact in fp32 and in fp64, so d2 == eps2 is decided the same way everywhere"""
    on_boundary = 0
    for seed in range(24):
        dim = (2, 3, 5)[seed % 3]
        X = dc.grid_case(90 + 7 * seed, dim, (9, 6, 3)[seed % 3], seed)
        D = dc.distances64(X, "euclidean")
        on_boundary += int((D == eps).sum())
        _agree(cpu, X, eps, 2 + seed % 5, "euclidean")
    assert on_boundary > 1000


def test_contested_border_rows_take_the_lowest_cluster_not_the_lowest_neighbour(cpu):
    for X, eps, min_samples, labels in dc.CONTESTED:
        got = _agree(cpu, X, eps, min_samples, "euclidean")
        assert got.labels.tolist() == labels
    # the second case tells the two rules apart: its row 3 has core neighbours in both clusters
    X, eps, min_samples, labels = dc.CONTESTED[1]
    wrong = dc.lowest_neighbour_rule(X, eps, min_samples).tolist()
    assert wrong != labels and wrong[3] == 1 and labels[3] == 0


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("dim", [1, 3, 16, 17, 130])
def test_the_restated_pair_test_is_symmetric_bit_for_bit(cpu, dim, metric):
    """within(i, j) == within(j, i) and dot(i, j) == dot(j, i) on random fp32 rows, rows of very different
    lengths included (xn_i >> xn_j), at thresholds that cut through the pairs"""
    rng = np.random.default_rng(100 * dim + len(metric))
    n = 48
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[::3] *= np.float32(4096.0)  # xn_i ~ 2^24 xn_j
    X[1::7] *= np.float32(1.0 / 1024.0)
    X[5] = 0.0
    aux = dc.inv_norms(cpu, X) if metric == "cosine" else dc.sumsq(cpu, X)
    D = dc.distances64(X, metric)
    thresholds = np.quantile(D[~np.eye(n, dtype=bool)], [0.1, 0.5, 0.9]).tolist() + [0.0, 1.0]
    px, pa = X.ctypes.data, aux.ctypes.data
    seen = set()
    for i in range(n):
        for j in range(i + 1, n):
            a = cpu.n2v_dbscan_cpu_dot(px + 4 * dim * i, px + 4 * dim * j, dim)
            b = cpu.n2v_dbscan_cpu_dot(px + 4 * dim * j, px + 4 * dim * i, dim)
            assert np.float32(a).tobytes() == np.float32(b).tobytes(), (i, j)
            for eps in thresholds:
                w = cpu.n2v_dbscan_cpu_within(px, pa, dim, dc.METRICS[metric], eps, i, j)
                assert w == cpu.n2v_dbscan_cpu_within(px, pa, dim, dc.METRICS[metric], eps, j, i), (i, j, eps)
                seen.add(w)
    assert seen == {0, 1}


UF_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#define N2V_UF_FN static inline
#define N2V_UF_LOAD(p) (*(p))
static inline int32_t cas(int32_t *p, int32_t e, int32_t v) { const int32_t o = *p; if (o == e) *p = v; return o; }
static inline void lower(int32_t *p, int32_t v) { if (v < *p) *p = v; }
#define N2V_UF_CAS(p, e, v) cas((p), (e), (v))
#define N2V_UF_MIN(p, v) lower((p), (v))
#include "n2v_unionfind.h"
// stdin: n m, then m pairs.  stdout: "ok" or "bad <step>", then find(v) of every v
int main() {
  long n, m;
  if (scanf("%ld %ld", &n, &m) != 2) return 2;
  std::vector<int32_t> parent(n), before(n);
  for (long v = 0; v < n; ++v) parent[v] = (int32_t)v;
  long bad = -1;
  for (long s = 0; s < m; ++s) {
    long a, b;
    if (scanf("%ld %ld", &a, &b) != 2) return 2;
    before = parent;
    uf_unite(parent.data(), (int32_t)a, (int32_t)b);
    for (long v = 0; v < n; ++v)  // parent[v] <= v, and a value only ever decreases
      if ((parent[v] > v || parent[v] < 0 || parent[v] > before[v]) && bad < 0) bad = s;
    if (uf_find(parent.data(), (int32_t)a) != uf_find(parent.data(), (int32_t)b) && bad < 0) bad = s;
  }
  if (bad < 0) printf("ok\n"); else printf("bad %ld\n", bad);
  for (long v = 0; v < n; ++v) printf("%d\n", uf_find(parent.data(), (int32_t)v));
  return 0;
}
"""


def test_unionfind_header_on_the_host_against_scipy_components(tmp_path):
    """the text the union scan runs, single-threaded: random union sequences, the invariant after every union, the
    final root of every vertex the minimum of its scipy component"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    src, exe = tmp_path / "uf_main.cpp", tmp_path / "uf_main"
    src.write_text(UF_MAIN)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "node2vec_amd", "csrc"),
                           "-o", str(exe), str(src)])
    rng = np.random.default_rng(8)
    for n, m in ((1, 0), (2, 1), (50, 200), (3000, 1500), (3000, 2600), (2500, 9000)):
        a, b = rng.integers(0, n, m), rng.integers(0, n, m)
        if n > 100:  # some long paths: chains hooked from the far end
            a[:50], b[:50] = np.arange(n - 50, n), np.arange(n - 51, n - 1)
        text = f"{n} {m}\n" + "".join(f"{x} {y}\n" for x, y in zip(a, b))
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        assert out[0] == "ok", out[0]
        roots = np.array([int(v) for v in out[1:n + 1]])
        _, comp = connected_components(coo_matrix((np.ones(m), (a, b)), shape=(n, n)).tocsr(), directed=False)
        lowest = np.full(comp.max() + 1, n)
        np.minimum.at(lowest, comp, np.arange(n))
        assert np.array_equal(roots, lowest[comp]), (n, m)


def test_dbscan_abi_refuses_bad_arguments_without_a_gpu(lib):
    """argument errors come back as N2V_EINVAL before anything is launched; n == 0 is N2V_OK"""
    from node2vec_amd import _lib

    buf = (C.c_int64 * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    big = 1 << 40

    def count(X=p, inv=p, n=10, dim=16, metric=1, eps=0.5, min_samples=3, counts=p, core=p, ws=p, ws_bytes=big,
              max_blocks=0):
        return lib.n2v_dbscan_count(X, inv, n, dim, metric, eps, min_samples, counts, core, ws, ws_bytes, max_blocks,
                                    None)

    def union(X=p, inv=p, n=10, dim=16, metric=1, eps=0.5, core=p, n_core=4, root=p, ws=p, ws_bytes=big,
              max_blocks=0):
        return lib.n2v_dbscan_union(X, inv, n, dim, metric, eps, core, n_core, root, ws, ws_bytes, max_blocks, None)

    def border(X=p, inv=p, n=10, dim=16, metric=1, eps=0.5, core=p, n_core=4, rows=p, n_border=6, labels=p, ws=p,
               ws_bytes=big, max_blocks=0):
        return lib.n2v_dbscan_border(X, inv, n, dim, metric, eps, core, n_core, rows, n_border, labels, ws, ws_bytes,
                                     max_blocks, None)

    need = lib.n2v_dbscan_workspace_bytes(10, 16)
    assert need > 0
    shared = (dict(dim=0), dict(dim=1025), dict(n=-1), dict(n=1 << 31), dict(metric=-1), dict(metric=2),
              dict(inv=None), dict(eps=-0.5), dict(eps=float("nan")), dict(eps=float("inf")), dict(max_blocks=-1))
    late = (dict(X=None), dict(ws=None), dict(ws=p + 4), dict(ws_bytes=0), dict(ws_bytes=need - 1))
    empties = {count: dict(n=0), union: dict(n=0, n_core=0), border: dict(n=0, n_core=0, n_border=0)}
    for call, empty in empties.items():
        assert call(**empty) == _lib.OK and call(metric=0, inv=None, **empty) == _lib.OK
        assert call(dim=1024, eps=0.0, **empty) == _lib.OK
        for kw in shared:
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
            if "n" not in kw:
                assert call(**empty, **kw) == _lib.EINVAL, (call.__name__, kw)  # refused before the empty input returns
        for kw in late:
            assert call(**kw) == _lib.EINVAL, (call.__name__, kw)
    for kw in (dict(min_samples=0), dict(min_samples=-3), dict(counts=None)):
        assert count(**kw) == _lib.EINVAL, kw
    assert count(n=0, min_samples=0) == _lib.EINVAL
    for kw in (dict(n_core=-1), dict(n_core=11), dict(core=None), dict(root=None)):
        assert union(**kw) == _lib.EINVAL, kw
    for kw in (dict(n_core=-1), dict(n_core=11), dict(n_border=-1), dict(n_border=11), dict(core=None),
               dict(rows=None), dict(labels=None)):
        assert border(**kw) == _lib.EINVAL, kw
    assert border(n_core=0) == _lib.OK and border(n_border=0) == _lib.OK  # nothing to scan: nothing launched
    # the size query: -1 for what the calls refuse, 0 for nothing to do, the documented parts otherwise
    q = lib.n2v_dbscan_workspace_bytes
    assert q(10, 0) == q(10, 1025) == q(-1, 16) == q(1 << 31, 16) == -1 and q(0, 16) == 0

    def up(x):
        return (x + 255) // 256 * 256

    for n, dim in ((10, 16), (1000, 100), (10 ** 6, 128), (2 ** 31 - 1, 1)):
        assert q(n, dim) == up((n + 63) // 64 * 64 * ((dim + 15) // 16 * 16) * 4) + up(4 * n), (n, dim)


def test_header_and_binding_name_the_dbscan_entry_points(lib):
    from node2vec_amd import _lib

    text = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("n2v_dbscan_workspace_bytes", "n2v_dbscan_count", "n2v_dbscan_union", "n2v_dbscan_border"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code) and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.n2v_abi_version() == 15


def test_python_layer_checks_its_arguments_before_the_gpu():
    """on host tensors: the message names the bad argument, so it was found before the device check"""
    from node2vec_amd import cluster

    X = torch.zeros((10, 8))
    for call in (cluster.dbscan, cluster.neighbor_counts):
        with pytest.raises(ValueError, match="metric"):
            call(X, 0.5, metric="manhattan")
        for eps in (-1.0, float("nan"), float("inf"), 1e39):  # 1e39 is inf in fp32
            with pytest.raises(ValueError, match="eps"):
                call(X, eps)
        with pytest.raises(ValueError, match="max_blocks"):
            call(X, 0.5, max_blocks=-1)
        with pytest.raises(ValueError, match="2-D tensor"):
            call(torch.zeros(10), 0.5)
        with pytest.raises(ValueError, match="HIP device"):  # everything else was fine: no CPU path
            call(X, 0.5)
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="min_samples"):
            cluster.dbscan(X, 0.5, min_samples=bad)


def test_a_result_has_the_documented_fields_and_goes_into_the_silhouette_unchanged():
    from node2vec_amd import cluster

    assert cluster.DBSCANResult._fields == ("labels", "core_mask", "n_clusters", "counts", "sizes")
    labels = torch.tensor([0, 0, -1, 1, 1, -1, 0], dtype=torch.int32)
    res = cluster.DBSCANResult(labels, labels >= 0, 2, torch.ones(7, dtype=torch.int32), torch.tensor([3, 2]))
    # what silhouette_samples makes of them on the host: the same labels, noise still -1 (no cluster), k = n_clusters
    kept, k = cluster._labels(res.labels, 7, res.n_clusters)
    assert kept.dtype == torch.int32 and torch.equal(kept, labels) and k == 2
    assert cluster._labels(res.labels, 7, None)[1] == 2


def test_model_classes_refuse_dbscan_before_fit():
    import pandas as pd

    from node2vec_amd.embedding import KeyedVectors, Node2VecHIP

    n2v = Node2VecHIP(pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4]]}), {})
    with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
        n2v.dbscan(0.5)
    assert n2v.dbscan_result is None
    with pytest.raises(ValueError, match="metric"):
        KeyedVectors(np.arange(5), np.ones((5, 4), np.float32)).dbscan(0.5, metric="manhattan")
