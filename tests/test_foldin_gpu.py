"""Fold-in on the GPU (csrc/n2v_foldin.hip, node2vec_amd/foldin.py, Node2VecHIP.infer_vertices): the pair listing
must equal the records of the CPU restatement tests/cpu_foldin/n2v_foldin_cpu.c exactly and the trained rows must
equal its rows BIT FOR BIT, on every case of tests/foldin_cases.py; the frozen model must be byte-identical before
and after.  What each case reaches is asserted from the restatement alone in test_foldin_host.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

import foldin_cases as fc
from test_foldin_host import cases, foldin_cpu  # noqa: F401  (session fixtures: the case list and the restatement)

pytestmark = pytest.mark.gpu


def _model(case):
    """the frozen model of a case on the GPU, as fold_in takes it"""
    from node2vec_amd import _lib, sgns

    dev = _lib.require_gpu()
    t = lambda a: torch.from_numpy(np.array(a).view(np.int32) if a.dtype == np.uint32 else  # noqa: E731
                                   np.array(a)).to(dev)  # (copies: the cases are read-only)
    m = SimpleNamespace(syn0=t(case["syn0"]), syn1neg=t(case["syn1neg"]), cum_table=t(case["cum_table"]),
                        sample_int=None if case["sample_int"] is None else t(case["sample_int"]),
                        exp_table=torch.from_numpy(sgns.exp_table()).to(dev), window=case["window"],
                        negative=case["negative"], seed=case["seed"], cum_index=None, cum_index_bits=0)
    if case["cum_index"]:
        m.cum_index_bits = 10
        m.cum_index = torch.empty((1 << 10) + 1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().n2v_cum_index_build(m.cum_table.data_ptr(), case["n_vocab"], 10, m.cum_index.data_ptr(),
                                                   _lib.current_stream_ptr()), "n2v_cum_index_build")
    return m, t(case["walks"]), t(case["init"]), None if case["row_alpha"] is None else t(case["row_alpha"])


def _frozen(m):
    keep = [m.syn0, m.syn1neg, m.cum_table, m.exp_table] + ([] if m.sample_int is None else [m.sample_int])
    return [x.cpu().numpy().tobytes() for x in keep]


def _gpu_pass(case, max_waves=0):
    """listing + one training pass on the GPU; returns (records, vertex_off, rows) as numpy"""
    from node2vec_amd import foldin

    m, walks, rows, row_alpha = _model(case)
    before = _frozen(m)
    records, off = foldin.pair_records(m, walks, case["n_new"], case["sentence_base"])
    foldin.train_pass(m, records, off, rows, walks.shape[0], walks.shape[1], case["alpha"], case["sentence_base"],
                      row_alpha=row_alpha, max_waves=max_waves)
    torch.cuda.synchronize()
    assert _frozen(m) == before, "fold-in wrote to the frozen model"
    return records.cpu().numpy(), off.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("name", fc.NAMES)
def test_records_and_rows_equal_the_restatement(foldin_cpu, cases, name):
    case = cases[name]
    want = case["init"].copy()
    n, rec = fc.cpu_pass(foldin_cpu, case, want, records=True)
    want_rec, want_off = fc.group_by_vertex(rec, case["n_new"])
    records, off, rows = _gpu_pass(case)
    assert records.shape == (n, 4) and n > 0
    assert np.array_equal(off, want_off) and np.array_equal(records, want_rec)
    assert np.isfinite(rows).all()
    assert np.array_equal(rows, want), float(np.abs(rows - want).max())
    if case["never"] is not None:  # the vertex that never occurs keeps its row
        assert off[case["never"]] == off[case["never"] + 1]
        assert np.array_equal(rows[case["never"]], case["init"][case["never"]])


@pytest.mark.parametrize("name", ["many_vertices_dim64", "dim128_window32_row_alpha", "dim1024_k6"])
def test_geometry_independence(foldin_cpu, cases, name):
    """the same case on one block, on a grid capped below n_new and on the default grid: the same bits"""
    case = cases[name]
    assert case["n_new"] > 4
    want = case["init"].copy()
    fc.cpu_pass(foldin_cpu, case, want)
    default = _gpu_pass(case)[2]
    for waves in (1, 4, 12):
        assert waves < case["n_new"] or waves == 12
        assert np.array_equal(_gpu_pass(case, max_waves=waves)[2], default), waves
    assert np.array_equal(default, want)


def test_three_epochs_through_fold_in(foldin_cpu, cases):
    from node2vec_amd import foldin

    case = cases["ragged_dim100_two_passes"]
    assert case["row_alpha"] is None
    m, walks, init, _ = _model(case)
    before = _frozen(m)
    epochs, alpha, min_alpha, base = 3, 0.05, 1e-3, 40
    rows, pairs = foldin.fold_in(m, walks, case["n_new"], epochs, alpha, min_alpha, init=init, sentence_base=base)
    torch.cuda.synchronize()
    assert _frozen(m) == before
    assert rows.data_ptr() != init.data_ptr() and np.array_equal(init.cpu().numpy(), case["init"])  # copied
    want, n = case["init"].copy(), 0
    for ep in range(epochs):
        a = max(min_alpha, alpha - (alpha - min_alpha) * (ep / epochs))
        n += fc.cpu_pass(foldin_cpu, case, want, alpha=a, sentence_base=base + ep * walks.shape[0])[0]
    assert pairs == n > 0
    assert np.array_equal(rows.cpu().numpy(), want)
    # init=None: the seeded rows, the same on every call, and not the trainer's
    from node2vec_amd import sgns

    r0, _ = foldin.fold_in(m, walks, case["n_new"], 0)
    assert torch.equal(r0, sgns.init_syn0(case["n_new"], case["dim"], case["seed"] ^ foldin.INIT_SEED_XOR, r0.device))
    r1, _ = foldin.fold_in(m, walks, case["n_new"], 1)
    r2, _ = foldin.fold_in(m, walks, case["n_new"], 1)
    assert torch.equal(r1, r2) and not torch.equal(r1, r0)


def test_fold_in_on_a_trained_sgns_model(foldin_cpu):
    """fold_in takes an sgns.SgnsModel as it stands after training (its own cum_index, sample_int)"""
    from node2vec_amd import foldin, sgns
    from test_sgns_gpu import _setup

    _, m, idx = _setup(60, 40, 21, 64, 5, 1e-2, 1, False)
    m.train_block(idx, 0.025, 0, deterministic=True)
    n_vocab, n_new = len(m.vocab), 5
    gen = torch.Generator().manual_seed(3)
    walks = idx.clone()
    mask = (torch.rand(idx.shape, generator=gen) < 0.2).to(idx.device)
    walks[mask] = (n_vocab + torch.randint(0, n_new, idx.shape, generator=gen)).to(idx.device, torch.int32)[mask]
    s0, s1 = m.syn0.clone(), m.syn1neg.clone()
    rows, pairs = foldin.fold_in(m, walks, n_new, 1, alpha=0.03, sentence_base=9)
    torch.cuda.synchronize()
    assert torch.equal(m.syn0, s0) and torch.equal(m.syn1neg, s1)
    case = {"walks": walks.cpu().numpy(), "n_vocab": n_vocab, "n_new": n_new, "dim": 64, "window": m.window,
            "negative": m.negative, "syn1neg": s1.cpu().numpy(), "cum_table": m.cum_table.cpu().numpy().view(np.uint32),
            "sample_int": m.sample_int.cpu().numpy().view(np.uint32), "row_alpha": None, "alpha": 0.03, "seed": m.seed,
            "sentence_base": 9}
    want = sgns.init_syn0(n_new, 64, m.seed ^ foldin.INIT_SEED_XOR, "cuda").cpu().numpy()
    n, _ = fc.cpu_pass(foldin_cpu, case, want)
    assert pairs == n > 0 and np.array_equal(rows.cpu().numpy(), want)


def test_argument_errors_leave_new_rows_untouched(cases):
    from node2vec_amd import _lib, foldin

    case = cases["dim128_window32_row_alpha"]
    m, walks, rows, _ = _model(case)
    records, off = foldin.pair_records(m, walks, case["n_new"], case["sentence_base"])
    before = rows.clone()
    L = _lib.load()

    def train(n_new=case["n_new"], new_rows=rows.data_ptr(), **kw):
        P = foldin._params(m, case["n_vocab"], 0, 0.025, None, 0)
        for k, v in kw.items():
            setattr(P, k, v)
        return L.n2v_foldin_train(records.data_ptr(), off.data_ptr(), n_new, walks.shape[0], walks.shape[1], new_rows,
                                  m.syn1neg.data_ptr(), m.cum_table.data_ptr(), m.exp_table.data_ptr(), P,
                                  _lib.current_stream_ptr())

    assert train(n_new=-1) == _lib.EINVAL and train(new_rows=None) == _lib.EINVAL
    assert train(n_vocab=2 ** 31 - 3) == _lib.EINVAL and train(negative=33) == _lib.EINVAL
    assert train(dim=0) == _lib.EINVAL and train(window=0) == _lib.EINVAL and train(batched=1) == _lib.EINVAL
    assert train(n_new=0) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(rows, before)
    with pytest.raises(ValueError):
        foldin.fold_in(m, walks, -1, 1)
    with pytest.raises(ValueError):
        foldin.fold_in(m, walks, case["n_new"], 1, init=rows[:, :5])
    with pytest.raises(TypeError):
        foldin.fold_in(m, walks.long(), case["n_new"], 1)


def _ring_walks(ids, rows, ln, seed):
    """walks on a ring of communities: a step goes to a vertex of the same block of ten with probability 0.9"""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids)
    out = np.empty((rows, ln), np.int64)
    out[:, 0] = ids[rng.integers(0, len(ids), rows)]
    for t in range(1, ln):
        block = out[:, t - 1] // 10
        block = np.where(rng.random(rows) < 0.9, block, rng.integers(0, 6, rows))
        cand = block * 10 + rng.integers(0, 10, rows)
        ok = np.isin(cand, ids)
        out[:, t] = np.where(ok, cand, out[:, t - 1])
    return out


def test_infer_vertices_end_to_end():
    """60 vertices in six blocks of ten; vertices 7, 23 and 58 are held out of the fit, then folded in from walks
    over all sixty.  The model is untouched, the frame has embedding()'s shape, with_rows extends the queries, and
    each folded-in vertex finds its own block"""
    from node2vec_amd.embedding import Node2VecHIP

    held = [7, 23, 58]
    known = [v for v in range(60) if v not in held]
    train = pd.DataFrame({"walk": _ring_walks(known, 600, 20, 1).tolist()})
    params = {"negative": 5, "min_count": 0, "iter": 3, "deterministic": True}
    n2v = Node2VecHIP(train, params, vector_size=32, window_size=5, random_seed=11)
    model = n2v.fit()
    vectors, syn1neg = model.wv.vectors.copy(), model.syn1neg.copy()
    grown = _ring_walks(list(range(60)), 600, 20, 2)
    df = n2v.infer_vertices(pd.DataFrame({"walk": grown.tolist()}))
    assert list(df.columns) == ["id", "vector"] and df["id"].tolist() == held
    assert all(len(v) == 32 and np.isfinite(v).all() for v in df["vector"])
    assert np.array_equal(model.wv.vectors, vectors) and np.array_equal(model.syn1neg, syn1neg) and len(model.wv) == 57
    again = n2v.infer_vertices(torch.from_numpy(grown))  # a tensor of walks: the same bits
    assert again["vector"].tolist() == df["vector"].tolist()
    rows = np.array(df["vector"].tolist(), np.float32)
    ext = model.wv.with_rows(np.array(held), rows)
    assert len(ext) == 60 and len(model.wv) == 57 and np.array_equal(ext["23"], rows[1])
    for v in held:
        hits = ext.most_similar(str(v), topn=5)
        assert len(hits) == 5 and all(t != str(v) for t, _ in hits)
        # its own block holds 9 of the other 59 vertices (chance: < 1 of 5 hits): more of it than of all the rest
        assert sum(int(t) // 10 == v // 10 for t, _ in hits) >= 3, (v, hits)
    # epochs=0 returns the seeded starting rows; another corpus is refused
    zero = n2v.infer_vertices(pd.DataFrame({"walk": grown.tolist()}), epochs=0)
    assert not np.array_equal(np.array(zero["vector"].tolist(), np.float32), rows)
    n2v.walks = pd.DataFrame({"walk": grown.tolist()})
    with pytest.raises(RuntimeError):
        n2v.infer_vertices(pd.DataFrame({"walk": grown.tolist()}))
