"""Node classification on the GPU (csrc/n2v_logreg.hip through node2vec_amd.classify) against its CPU restatement,
tests/cpu_logreg/n2v_logreg_cpu.c, bit for bit: the fp32 scores and the float64 loss and gradient by their bit
patterns.  The shapes sit on the kernel's edges: both load paths (dim % 4, base alignment), a ragged last 16-block
(dim), the edges of a class tile (16, 64), of a label word (32) and of the loop over chunks (c), a ragged wave, step
and slab (n)."""
import numpy as np
import pandas as pd
import pytest
import torch

import logreg_cases as lc
from conftest import ROOT  # noqa: F401
from kmeans_cases import special_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return lc.build(tmp_path_factory.mktemp("logreg_cpu"))


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


def _check(cpu, X, Y, W, b, aligned=True, scores=True):
    from node2vec_amd import classify

    Xd, Wd, bd = _device(X, aligned), _device(W), _device(b)
    if scores:
        got = classify.decision_function(Xd, Wd, bd).cpu().numpy()
        assert lc.same_bits(got, lc.scores(cpu, X, W, b)), ("scores", X.shape, W.shape, aligned)
    yb = classify.pack_labels(torch.from_numpy(np.asarray(Y)).cuda())
    loss, gW, gb = (t.cpu().numpy() for t in classify.loss_grad(Xd, yb, Wd, bd))
    w_loss, w_gW, w_gb = lc.loss_grad(cpu, X, Y, W, b)
    assert lc.same_bits(gW, w_gW), ("gW", X.shape, W.shape, aligned, np.abs(gW - w_gW).max())
    assert lc.same_bits(gb, w_gb), ("gb", X.shape, W.shape, aligned)
    assert lc.same_bits(loss, w_loss), ("loss", X.shape, W.shape, aligned, loss, w_loss)
    return loss, gW, gb


@pytest.mark.parametrize("dim", [1, 3, 4, 15, 16, 17, 64, 100, 128, 129, 1000, 1024])
def test_bitwise_over_the_dimensions(cpu, dim):
    for c, aligned in ((15, True), (15, False), (17, True), (17, False)):
        X, W, b, Y = lc.normal_case(81, dim, c, 31 * dim + c, scale=0.5 / np.sqrt(dim))
        _check(cpu, X, Y, W, b, aligned)


@pytest.mark.parametrize("c", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1024])
def test_bitwise_over_the_class_tiles(cpu, c):
    for dim in (64, 17):
        X, W, b, Y = lc.normal_case(65, dim, c, 7 * c + dim, scale=0.2)
        _check(cpu, X, Y, W, b)


def _three_slabs_and_a_tail(dim, c):
    from node2vec_amd import classify

    slab = classify.slab_rows(300, dim, c)  # read from the library
    n = 3 * slab + 37
    assert classify.slab_rows(n, dim, c) == slab and n // slab == 3 and n % slab
    return n


def test_bitwise_over_the_row_counts(cpu):
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 257, _three_slabs_and_a_tail(20, 18)):
        X, W, b, Y = lc.normal_case(n, 20, 18, n)
        _check(cpu, X, Y, W, b)


def test_bitwise_on_slabs_longer_than_one_step_and_the_same_twice(cpu):
    from node2vec_amd import classify

    n, dim, c = 150001, 8, 4
    assert classify.slab_rows(n, dim, c) > 64 and n // classify.slab_rows(n, dim, c) >= 3
    X, W, b, Y = lc.normal_case(n, dim, c, 3)
    for aligned in (True, False):
        first = _check(cpu, X, Y, W, b, aligned)
    again = _check(cpu, X, Y, W, b, False, scores=False)
    for a, g in zip(first, again):
        assert lc.same_bits(a, g)


@pytest.mark.parametrize("pattern", ["ones", "zeros", "single"])
def test_bitwise_on_label_patterns(cpu, pattern):
    n = _three_slabs_and_a_tail(20, 35)
    X, W, b, Y = lc.normal_case(n, 20, 35, 12)
    if pattern == "ones":
        Y[:] = True
    elif pattern == "zeros":
        Y[:] = False
    else:
        Y[:, 33] = False
        Y[n - 2, 33] = True  # one positive, in the last slab
    _check(cpu, X, Y, W, b, scores=False)


@pytest.mark.parametrize("dim", [5, 64])
def test_scores_bitwise_on_signed_zeros_denormals_and_inf(cpu, dim):
    from node2vec_amd import classify

    X = special_rows(dim, dim)
    _, W, b, _ = lc.normal_case(1, dim, 20, dim + 1)
    W[3] = 0.0
    W[4] = X[10]
    b[3] = -0.0
    for aligned in (True, False):
        got = classify.decision_function(_device(X, aligned), _device(W), _device(b)).cpu().numpy()
        assert lc.same_bits(got, lc.scores(cpu, X, W, b)), aligned
        assert np.isnan(got[9]).all()


def test_a_nan_row_poisons_exactly_what_the_restatement_says(cpu):
    n = _three_slabs_and_a_tail(20, 18)
    X, W, b, Y = lc.normal_case(n, 20, 18, 4)
    X[70, 3] = np.nan
    loss, gW, gb = _check(cpu, X, Y, W, b)
    assert np.isnan(loss[0]) and np.isnan(gW).all() and np.isnan(gb).all()


def test_saturated_scores(cpu):
    """|z| so large that p is exactly 0 or 1: res is exactly -y or 1 - y"""
    X, W, b, Y = lc.normal_case(130, 16, 6, 9)
    W *= np.float32(400.0)
    Z = lc.scores(cpu, X, W, b)
    assert (np.abs(Z) > 104).mean() > 0.5
    _check(cpu, X, Y, W, b)


def test_loss_grad_at_zero_weights(cpu):
    n, dim, c = 333, 12, 5
    X, _, _, Y = lc.normal_case(n, dim, c, 6)
    X = np.round(X * 8)  # small integers: every partial sum is exact
    W, b = np.zeros((c, dim), np.float32), np.zeros(c, np.float32)
    loss, gW, gb = _check(cpu, X, Y, W, b)
    l0 = np.float64(lc.points(cpu, np.zeros(1, np.float32), 0)[0, 3])
    assert loss[0] == n * c * l0
    assert np.array_equal(gW, (0.5 - Y.astype(np.float64)).T @ X.astype(np.float64))
    assert np.array_equal(gb, (0.5 - Y.astype(np.float64)).sum(0))


def test_exact_by_construction_past_32_bit_offsets():
    """n dim > 2^31 elements, X integer-valued: with W = 0 every residual is +-0.5 and every slab partial (at most
    slab_rows * 8 / 2 < 2^24) is exact, so the gradient is the float64 torch sum; with small integer W the scores of
    sampled rows are float64 matmul's, the last three rows included"""
    from node2vec_amd import classify

    n, dim, c = (1 << 23) + 5, 260, 4
    assert n * dim > 1 << 31 and classify.slab_rows(n, dim, c) * 8 < 1 << 24
    gen = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randint(-8, 9, (n, dim), generator=gen, device="cuda", dtype=torch.int8).float()
    r = torch.arange(n, device="cuda")
    Y = torch.stack([(r * 7 + r // 1000 + k) % 3 == 0 for k in range(c)], 1)
    Y[-3:] = torch.tensor([[1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 1]], dtype=torch.bool, device="cuda")
    del r
    zero_W, zero_b = torch.zeros((c, dim), device="cuda"), torch.zeros(c, device="cuda")
    loss, gW, gb = classify.loss_grad(X, classify.pack_labels(Y), zero_W, zero_b)
    res = 0.5 - Y.double()
    want = torch.stack([(X * res[:, k:k + 1].float()).sum(0, dtype=torch.float64) for k in range(c)])
    assert torch.equal(gW, want)
    assert torch.equal(gb, res.sum(0))
    W = torch.randint(-3, 4, (c, dim), generator=gen, device="cuda").float()
    b = torch.tensor([1.0, -2.0, 0.0, 5.0], device="cuda")
    Z = classify.decision_function(X, W, b)
    rows = torch.cat([torch.arange(0, n, 65537, device="cuda"), torch.arange(n - 3, n, device="cuda")])
    assert torch.equal(Z[rows].double(), X[rows].double() @ W.double().t() + b.double())


def test_fit_on_the_gpu_equals_the_restated_loop(cpu):
    from node2vec_amd import classify

    X, Y = lc.planted()
    want = classify.fit(torch.from_numpy(X), torch.from_numpy(Y), C=1.0, loss_grad_fn=lc.torch_loss_grad_fn(cpu, X, Y))
    got = classify.fit(_device(X), torch.from_numpy(Y).cuda(), C=1.0)
    assert (got.n_iter, got.n_evals, got.reason, got.converged) == (want.n_iter, want.n_evals, want.reason, True)
    assert got.W.is_cuda and lc.same_bits(got.W.cpu().numpy(), want.W.numpy())
    assert lc.same_bits(got.b.cpu().numpy(), want.b.numpy())
    assert got.loss == want.loss and got.grad_max == want.grad_max
    bad = _device(X).clone()
    bad[7, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        classify.fit(bad, torch.from_numpy(Y).cuda())


def test_evaluate_is_reproducible_and_trains_on_the_stated_rows():
    from node2vec_amd import classify

    X, Y = lc.planted(n=300, seed=8)
    Xd, Yd = _device(X), torch.from_numpy(Y).cuda()
    res, f1 = classify.evaluate(Xd, Yd, train_fraction=0.4, seed=5)
    again, f1_again = classify.evaluate(Xd, Yd, train_fraction=0.4, seed=5)
    assert torch.equal(res.W, again.W) and torch.equal(res.b, again.b) and f1["micro"] == f1_again["micro"]
    perm = np.random.default_rng(5).permutation(300)
    train, test = perm[:120], perm[120:]
    assert [a.tolist() for a in classify.split_rows(300, 0.4, 5)] == [train.tolist(), test.tolist()]
    direct = classify.fit(_device(X[train]), torch.from_numpy(Y[train]).cuda())
    assert torch.equal(direct.W, res.W) and torch.equal(direct.b, res.b)
    scores = classify.decision_function(_device(X[test]), res.W, res.b)
    truth = torch.from_numpy(Y[test]).cuda()
    want = classify.f1_scores(truth, classify.predict_top(scores, truth.sum(1)))
    assert f1["micro"] == want["micro"] and f1["macro"] == want["macro"] and f1["micro"] > 0.5
    other, _ = classify.evaluate(Xd, Yd, train_fraction=0.4, seed=6)
    assert not torch.equal(other.W, res.W)


def test_keyedvectors_logreg_on_host_and_device_vectors():
    from node2vec_amd import classify
    from node2vec_amd.embedding import KeyedVectors

    X, Y = lc.planted(n=200, seed=2)
    ids = np.arange(1000, 1200)
    direct = classify.fit(_device(X), torch.from_numpy(Y).cuda())
    for kv in (KeyedVectors(ids, X), KeyedVectors(ids, _device(X))):
        res = kv.logreg(Y)
        assert torch.equal(res.W, direct.W) and torch.equal(res.b, direct.b) and res.converged
        scores = kv.label_scores(res)
        assert torch.equal(scores, classify.decision_function(_device(X), res.W, res.b))
    part = KeyedVectors(ids, X).logreg(Y, restrict_vocab=100, C=0.5)
    want = classify.fit(_device(X[:100]), torch.from_numpy(Y[:100]).cuda(), C=0.5)
    assert torch.equal(part.W, want.W)


WALKS = pd.DataFrame.from_dict({"walk": [[0, 1, 1, 0, 3, 4], [1, 2, 3, 2, 0, 4], [2, 3, 1, 0, 4, 4]]})


def test_model_classes_classify_their_vocabulary():
    from node2vec_amd import classify
    from node2vec_amd.embedding import HipW2V, HsW2VModel, KeyedVectors, Node2VecHIP, Node2VecSpark

    X, Y = lc.planted(n=60, seed=6)
    ids = np.arange(60)[::-1] + 100  # vocabulary order is not id order
    rows, cols = np.nonzero(Y)
    labels = pd.DataFrame({"id": ids[rows], "label": np.array(["a", "b", "c"])[cols]})
    names = pd.DataFrame({"id": list(ids) + [159, 500], "name": [f"v{i}" for i in ids] + ["last", "unused"]})
    for cls, model in ((Node2VecHIP, lambda wv: HipW2V(wv, np.zeros((60, 8), np.float32), {}, 0)),
                       (Node2VecSpark, lambda wv: HsW2VModel(wv, np.zeros((59, 8), np.float32), {}, 0, {}))):
        n2v = cls(WALKS, {})
        with pytest.raises(ValueError, match="Model is not available. Please run fit()"):
            n2v.classify(labels)
        n2v.model = model(KeyedVectors(ids, X))
        df = n2v.classify(labels, train_fraction=0.5, seed=1)
        assert list(df.columns) == ["id", "label", "score", "predicted", "train"] and len(df) == 60 * 3
        assert df["id"].tolist() == np.repeat(ids, 3).tolist() and df["label"].tolist() == ["a", "b", "c"] * 60
        assert df["train"].sum() == 30 * 3 and df["predicted"].dtype == bool
        train = classify.split_rows(60, 0.5, 1)[0]
        assert sorted(set(df["id"][df["train"]])) == sorted(ids[train].tolist())
        want = classify.fit(_device(X[train]), torch.from_numpy(Y[train]).cuda())
        assert torch.equal(n2v.classifier.W, want.W) and set(n2v.label_f1) == {"micro", "macro", "per_class"}
        assert df["predicted"].to_numpy().reshape(60, 3).sum(1).tolist() == Y.sum(1).tolist()  # the paper's protocol
        n2v.name_id = names
        named = n2v.classify(labels, train_fraction=0.5, seed=1)
        assert list(named.columns) == ["name", "label", "score", "predicted", "train"]
        assert named["name"].tolist()[:6] == ["last"] * 3 + [f"v{ids[1]}"] * 3  # id 159: its last name wins
        assert named["score"].tolist() == df["score"].tolist()
        n2v.name_id = names[names["id"] != 105]
        with pytest.raises(KeyError):
            n2v.classify(labels)
        n2v.name_id = None
        with pytest.raises(KeyError):
            n2v.classify(pd.DataFrame({"id": [100, 7], "label": ["a", "b"]}))
