"""The size entry points of the dense tasks (n2v_knn, n2v_kmeans, n2v_logreg) are host code: slab rows and workspace
bytes over a grid of shapes, the -1 rejections included, against tests/golden/dense_plans.json.  The fixture was
recorded from the library as it stood before the three files got one plan, carver and launch core (every value of
the full cross product, in itertools.product order); `python tests/test_dense_plans_host.py <file>` writes one from
the library that N2V_HIP_LIB names."""
import itertools
import json
import sys

import pytest

from conftest import ROOT, load_golden  # noqa: F401  (puts the repository on sys.path)

GRID = {
    "n": [0, 1, 63, 64, 65, 130, 131072, 131073, 2 ** 31 - 1, 2 ** 31],
    "dim": [0, 1, 3, 16, 17, 1024, 1025],
    "k": [0, 1, 16, 17, 64, 65, 1024, 1025],  # clusters, classes
    "knn_nq": [1, 16, 17, 64, 65, 1000],
    "knn_k": [0, 1, 10, 1024],
}


def measure(L):
    slabs = list(itertools.product(GRID["n"], GRID["dim"], GRID["k"]))
    knn = list(itertools.product(GRID["n"], GRID["dim"], GRID["knn_nq"], GRID["knn_k"]))
    return {
        "grid": GRID,
        "knn_workspace_bytes": [L.n2v_knn_workspace_bytes(*a) for a in knn],
        "kmeans_slab_rows": [L.n2v_kmeans_slab_rows(*a) for a in slabs],
        "kmeans_workspace_bytes": [L.n2v_kmeans_workspace_bytes(*a) for a in slabs],
        "logreg_slab_rows": [L.n2v_logreg_slab_rows(*a) for a in slabs],
        "logreg_workspace_bytes": [L.n2v_logreg_workspace_bytes(*a) for a in slabs],
    }


@pytest.fixture(scope="module")
def measured():
    import __graft_entry__ as ge

    ge.build()
    from node2vec_amd import _lib

    return measure(_lib.load())


@pytest.mark.parametrize("name", ["knn_workspace_bytes", "kmeans_slab_rows", "kmeans_workspace_bytes",
                                  "logreg_slab_rows", "logreg_workspace_bytes"])
def test_sizes_are_the_recorded_ones(measured, name):
    want = load_golden("dense_plans.json")
    assert want["grid"] == GRID
    axes = ("n", "dim", "knn_nq", "knn_k") if name.startswith("knn") else ("n", "dim", "k")
    cases = list(itertools.product(*(GRID[a] for a in axes)))
    assert len(want[name]) == len(measured[name]) == len(cases)
    differ = [(c, w, g) for c, w, g in zip(cases, want[name], measured[name]) if w != g]
    assert not differ, f"{name}{axes}: (case, recorded, now) {differ[:5]} and {max(len(differ) - 5, 0)} more"
    assert -1 in want[name] and any(v > 0 for v in want[name])  # the grid holds rejections and sizes


if __name__ == "__main__":
    from node2vec_amd import _lib

    with open(sys.argv[1], "w") as f:
        json.dump(measure(_lib.load()), f, separators=(",", ":"))
        f.write("\n")
