"""The link-prediction classifier on the GPU (node2vec_amd/linkpred.py, csrc/n2v_edge_logreg.hip): scores, loss and
gradient bit for bit against the CPU restatement (tests/cpu_edge_logreg/n2v_edge_logreg_cpu.c) at every lane-group
instance and on the ragged path, their symmetry and independence of place, an index outside the rows through the raw
call, the whole fit against the fit on the restatement, and the public interface end to end on the karate club."""
import numpy as np
import pandas as pd
import pytest
import torch

import edge_logreg_cases as ec
from conftest import load_golden

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 63, 64, 65, 128, 129, 256, 300, 1024)  # every (G, K) instance, full and ragged
N_PAIRS = (1, 63, 64, 65, 257, 10007)
# 131 073: the smallest count whose slabs hold two groups of 64 pairs (two waves of a block at work); a block steps
# over 256 pairs at a time, so 524 289 is the smallest count at which a slab (320 pairs) holds two block steps and a
# wave's chains run over two groups
N_TWO_GROUPS, N_TWO_STEPS = 2048 * 64 + 1, 2048 * 256 + 1
ROWS = 300
ZERO_ROW = 5


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return ec.build(tmp_path_factory.mktemp("edge_logreg_cpu"))


def _matrix(dim):
    """300 seeded normal rows, one of them zero; no NaN (a NaN row would make every sum NaN)"""
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((ROWS, dim)).astype(np.float32)
    X[ZERO_ROW] = 0.0
    return X


def _pair_list(n=N_PAIRS[-1]):
    """pairs over the 300 rows as tests/test_linkpred_gpu.py builds them: a == b, the zero row, a repeated pair, then
    random ones (with more repeats); every prefix of length >= 7 holds the special ones.  With labels."""
    rng = np.random.default_rng(99)
    a, b = rng.integers(0, ROWS, n), rng.integers(0, ROWS, n)
    head = [(3, 3), (ZERO_ROW, 9), (9, ZERO_ROW), (2, 17), (ZERO_ROW, ZERO_ROW), (11, 12), (11, 12)]
    a[:len(head)], b[:len(head)] = zip(*head)
    if n >= 5100:
        a[5000:5100], b[5000:5100] = a[100:200], b[100:200]
    y = (rng.random(n) < 0.4).astype(np.uint8)
    return a.astype(np.int64), b.astype(np.int64), y


def _weights(dim):
    rng = np.random.default_rng(1000 + dim)
    return (rng.standard_normal(dim) * 0.5 / np.sqrt(dim)).astype(np.float32), np.float32(rng.standard_normal())


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _gpu_loss_grad(Xd, a, b, y, w, b0, op):
    from node2vec_amd import linkpred

    loss, gw, gb = linkpred.edge_loss_grad(Xd, _t(a), _t(b), _t(y), _t(w), float(b0), op)
    assert loss.dtype == gw.dtype == gb.dtype == torch.float64 and loss.is_cuda
    assert tuple(loss.shape) == (1,) and tuple(gw.shape) == (Xd.shape[1],) and tuple(gb.shape) == (1,)
    return loss.cpu().numpy(), gw.cpu().numpy(), gb.cpu().numpy()


@pytest.mark.parametrize("dim", DIMS)
def test_scores_loss_and_gradient_equal_the_restatement_bit_for_bit(cpu, dim):
    from node2vec_amd import linkpred

    X = _matrix(dim)
    Xd = _t(X)
    a, b, y = _pair_list()
    w, b0 = _weights(dim)
    for op in ec.OPS:
        want_z = ec.scores(cpu, X, a, b, w, b0, op)
        assert np.isfinite(want_z).all()
        for n in N_PAIRS:
            got = linkpred.edge_scores(Xd, _t(a[:n]), _t(b[:n]), _t(w), float(b0), op)
            assert got.dtype == torch.float32 and got.shape == (n,)
            assert ec.same_bits(got.cpu().numpy(), want_z[:n]), (dim, op, n)
            got = _gpu_loss_grad(Xd, a[:n], b[:n], y[:n], w, b0, op)
            want = ec.loss_grad(cpu, X, a[:n], b[:n], y[:n], w, b0, op)
            for name, g, wnt in zip(("loss", "gw", "gb"), got, want):
                assert ec.same_bits(g, wnt), (dim, op, n, name)
    assert linkpred.edge_scores(Xd, [], [], _t(w), float(b0)).shape == (0,)
    # lists and numpy arrays are taken as indices, labels and weights; a workspace may be passed in
    ws = linkpred.alloc_edge_workspace(65, dim, Xd.device)
    got = linkpred.edge_loss_grad(Xd, a[:65].tolist(), b[:65], y[:65].astype(bool), w, b0, "l1", workspace=ws)
    want = ec.loss_grad(cpu, X, a[:65], b[:65], y[:65], w, b0, "l1")
    assert all(ec.same_bits(g.cpu().numpy(), wnt) for g, wnt in zip(got, want))


@pytest.mark.parametrize("n", [N_TWO_GROUPS, N_TWO_STEPS])
def test_slabs_of_more_than_one_group(cpu, n):
    from node2vec_amd import linkpred

    dim = 64
    assert linkpred.edge_slab_pairs(n, dim) == ec.slab_pairs(cpu, n, dim) == (128 if n == N_TWO_GROUPS else 320)
    X = _matrix(dim)
    a, b, y = _pair_list(n)
    w, b0 = _weights(dim)
    got = _gpu_loss_grad(_t(X), a, b, y, w, b0, "hadamard")
    want = ec.loss_grad(cpu, X, a, b, y, w, b0, "hadamard")
    for name, g, wnt in zip(("loss", "gw", "gb"), got, want):
        assert ec.same_bits(g, wnt), (n, name)


@pytest.mark.parametrize("dim", (64, 129, 300))
def test_symmetry_and_independence_of_place(cpu, dim):
    from node2vec_amd import linkpred

    X = _matrix(dim)
    Xd = _t(X)
    a, b, y = _pair_list()
    w, b0 = _weights(dim)
    for op in ec.OPS:
        z = linkpred.edge_scores(Xd, _t(a), _t(b), _t(w), float(b0), op).cpu().numpy()
        assert ec.same_bits(linkpred.edge_scores(Xd, _t(b), _t(a), _t(w), float(b0), op).cpu().numpy(), z), op
        tail = linkpred.edge_scores(Xd, _t(a[4001:]), _t(b[4001:]), _t(w), float(b0), op)  # a prefix removed
        assert ec.same_bits(tail.cpu().numpy(), z[4001:]), op
        for n in (257, 10007):
            fwd = _gpu_loss_grad(Xd, a[:n], b[:n], y[:n], w, b0, op)
            swp = _gpu_loss_grad(Xd, b[:n], a[:n], y[:n], w, b0, op)
            assert all(ec.same_bits(g, h) for g, h in zip(fwd, swp)), (op, n)


def test_a_base_off_the_16_byte_grid_takes_the_element_path(cpu):
    """dim % 4 == 0, but X starts 4 bytes past a 16-byte boundary: the same bits as the aligned copy"""
    from node2vec_amd import linkpred

    dim, n = 64, 257
    X = _matrix(dim)
    Xd = _t(X)
    Xs = torch.empty(ROWS * dim + 1, device="cuda")[1:].view(ROWS, dim).copy_(Xd)
    assert Xs.data_ptr() % 16 == 4 and Xs.is_contiguous()
    a, b, y = _pair_list(n)
    w, b0 = _weights(dim)
    for op in ("average", "l2"):
        want = linkpred.edge_scores(Xd, _t(a), _t(b), _t(w), float(b0), op).cpu().numpy()
        assert ec.same_bits(linkpred.edge_scores(Xs, _t(a), _t(b), _t(w), float(b0), op).cpu().numpy(), want)
        assert ec.same_bits(want, ec.scores(cpu, X, a, b, w, b0, op))
        aligned, shifted = _gpu_loss_grad(Xd, a, b, y, w, b0, op), _gpu_loss_grad(Xs, a, b, y, w, b0, op)
        assert all(ec.same_bits(g, h) for g, h in zip(aligned, shifted)), op


def test_an_index_outside_the_rows_is_nan_through_the_raw_call():
    """The Python layer raises first, so the index goes through the library's own entry points.  The kernels never
    dereference it: load_pair turns it into row -1, which load_step reads as a dead pair (no load is issued)."""
    from node2vec_amd import _lib, linkpred

    dim, n = 20, 70
    X = _t(_matrix(dim))
    a, b, y = _pair_list(n)
    w, b0 = _weights(dim)
    with pytest.raises(IndexError):
        linkpred.edge_scores(X, _t(np.r_[a[:-1], ROWS]), _t(b), _t(w), float(b0))
    for bad_a, bad_b in ((ROWS, 0), (0, -1), (1 << 40, 3)):
        aa, bb = a.copy(), b.copy()
        aa[66], bb[66] = bad_a, bad_b
        ta, tb, ty, tw, tb0 = _t(aa), _t(bb), _t(y), _t(w), _t(np.array([b0], np.float32))
        z = torch.empty(n, device="cuda")
        out = torch.zeros(dim + 2, dtype=torch.float64, device="cuda")
        ws = linkpred.alloc_edge_workspace(n, dim, X.device)
        L = _lib.load()
        _lib.check(L.n2v_edge_logreg_scores(X.data_ptr(), ROWS, dim, ta.data_ptr(), tb.data_ptr(), n, 1, tw.data_ptr(),
                                            tb0.data_ptr(), z.data_ptr(), _lib.current_stream_ptr()), "scores")
        _lib.check(L.n2v_edge_logreg_loss_grad(X.data_ptr(), ROWS, dim, ta.data_ptr(), tb.data_ptr(), ty.data_ptr(), n,
                                               1, tw.data_ptr(), tb0.data_ptr(), out.data_ptr(), out[1:].data_ptr(),
                                               out[1 + dim:].data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.current_stream_ptr()), "loss_grad")
        z = z.cpu().numpy()
        assert np.isnan(z[66]) and np.isfinite(np.delete(z, 66)).all()
        assert np.isnan(out.cpu().numpy()).all()  # loss, every element of gw, gb


def test_fit_on_the_gpu_equals_the_fit_on_the_restatement(cpu):
    from node2vec_amd import linkpred

    X, a, b, y = ec.planted()
    T = torch.from_numpy
    for op in ("hadamard", "l2"):
        fn = ec.torch_loss_grad_fn(cpu, X, a, b, y, op)
        want = linkpred.fit_edges(T(X), T(a), T(b), T(y), op=op, loss_grad_fn=fn)
        assert want.converged and want.reason == "gradient"
        for _ in range(2):  # a second call repeats it
            got = linkpred.fit_edges(_t(X), _t(a), _t(b), _t(y), op=op)
            assert got.w.is_cuda and got.op == op and got.converged and got.reason == "gradient"
            assert torch.equal(got.w.cpu(), want.w) and torch.equal(got.b.cpu(), want.b)
            assert (got.n_evals, got.n_iter, got.loss, got.grad_max) == (want.n_evals, want.n_iter, want.loss,
                                                                         want.grad_max)


@pytest.fixture(scope="module")
def karate():
    from node2vec_amd.fugue import random_walk
    from node2vec_amd.graph import DeviceGraph

    e = load_golden("karate_edges.json")
    df = pd.DataFrame(e, columns=["src", "dst", "weight"])
    params = {"num_walks": 10, "walk_length": 10, "return_param": 1.0, "inout_param": 1.0}
    walks = random_walk("hip", df, params, random_seed=42)
    g = DeviceGraph.from_edges(df["src"].to_numpy(), df["dst"].to_numpy(), n_vertices=34, device="cuda")
    return df[["src", "dst"]], walks, g


def test_end_to_end_on_the_karate_club(karate, cpu):
    """no AUC threshold: what this tiny graph gives has not been measured"""
    from node2vec_amd import linkpred
    from node2vec_amd.embedding import Node2VecHIP

    df_edges, walks, g = karate
    n2v = Node2VecHIP(walks, {"min_count": 0, "iter": 3, "size": 16, "negative": 5, "deterministic": True},
                      random_seed=1000)
    n2v.fit()
    wv = n2v.model.wv
    n = 200
    res = linkpred.link_classifier_auc(g, wv, n, seed=5, op="hadamard", train_fraction=0.5)
    assert set(res) == {"auc", "train_pairs", "test_pairs", "dropped", "result"}
    print("karate link-classifier AUC", res["auc"], res["result"].n_iter, res["result"].n_evals)
    assert 0.0 <= res["auc"] <= 1.0
    assert res["train_pairs"] + res["test_pairs"] + res["dropped"] == 2 * n and res["dropped"] == 0
    assert res["train_pairs"] == n and res["result"].converged and res["result"].op == "hadamard"
    # link_classifier / link_classifier_scores round-trip a DataFrame
    pos, neg = linkpred.sample_edges(g, 60, 7), linkpred.sample_non_edges(g, 60, 8)
    df_pairs = pd.DataFrame({"src": torch.cat([pos[0], neg[0]]).cpu().numpy(),
                             "dst": torch.cat([pos[1], neg[1]]).cpu().numpy(), "label": [1] * 60 + [0] * 60})
    result = n2v.link_classifier(df_pairs, "l2")
    assert result is n2v.edge_classifier and result.op == "l2" and result.converged
    out = n2v.link_classifier_scores(df_edges, result)
    assert list(out.columns) == ["src", "dst", "score"] and len(out) == len(df_edges)
    src, dst = df_edges["src"].to_numpy(), df_edges["dst"].to_numpy()
    assert np.array_equal(out["src"].to_numpy(), src) and np.array_equal(out["dst"].to_numpy(), dst)
    direct = wv.edge_scores(src, dst, result)
    assert direct.dtype == np.float32 and ec.same_bits(out["score"].to_numpy(), direct)
    assert ec.same_bits(n2v.link_classifier_scores(df_edges)["score"].to_numpy(), direct)  # the kept classifier
    rows_a = np.array([wv.vocab[str(v)] for v in src])
    rows_b = np.array([wv.vocab[str(v)] for v in dst])
    assert ec.same_bits(direct, ec.scores(cpu, wv.vectors, rows_a, rows_b, result.w.cpu().numpy(),
                                          float(result.b[0]), "l2"))
    # the fit of the frame is the fit of its rows
    ra = np.array([wv.vocab[str(v)] for v in df_pairs["src"]])
    rb = np.array([wv.vocab[str(v)] for v in df_pairs["dst"]])
    again = linkpred.fit_edges(wv._device_vectors(), ra, rb, df_pairs["label"].to_numpy(), op="l2")
    assert torch.equal(again.w, result.w) and torch.equal(again.b, result.b)
    with pytest.raises(KeyError):
        n2v.link_classifier(pd.DataFrame({"src": [0, 99], "dst": [1, 2], "label": [1, 0]}))
    with pytest.raises(ValueError):
        n2v.link_classifier(df_edges)  # no labels
