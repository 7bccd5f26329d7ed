"""Fold-in: rows for NEW vertices against a frozen skip-gram negative-sampling model (csrc/n2v_foldin.hip,
DESIGN.md "Fold-in"; doc2vec's infer_vector is the same idea).

The trained model is only read.  Walks over the grown graph name known words by their vocabulary index and new
vertices by n_vocab + new index; a pair of the trainer whose context word is new and whose centre word is known is
trained on the new vertex's row as the trainer would train it, minus the updates of syn1neg.  The pairs of one new
vertex form one sequential chain, independent of every other vertex: the result is a pure function of the inputs
and does not depend on launch geometry.  torch is plumbing here (the prefix over rows, the stable sort that groups
records by vertex); listing and training are the HIP kernels.
"""
import math
from typing import Optional, Tuple

import torch

from node2vec_amd import _lib, sgns

INIT_SEED_XOR = 0x666f6c64  # "fold": the seeded starting rows are not the trainer's own


def _params(model, n_vocab: int, sentence_base: int, alpha: float, row_alpha, max_waves: int) -> "_lib.SgnsParams":
    cum_index = getattr(model, "cum_index", None)
    bits = int(getattr(model, "cum_index_bits", 0) or 0)
    if cum_index is not None and not bits:
        bits = int(math.log2(cum_index.numel() - 1))
    return _lib.SgnsParams(n_vocab, int(sentence_base), int(model.seed) & (2 ** 64 - 1), int(model.syn1neg.shape[1]),
                           int(model.window), int(model.negative), float(alpha), 0, bits,
                           0 if cum_index is None else cum_index.data_ptr(), int(max_waves), 0, 0, 0,
                           0 if row_alpha is None else row_alpha.data_ptr())


def _check(model, walks_idx: torch.Tensor, n_new: int) -> torch.Tensor:
    if getattr(model, "sg", 1) != 1 or getattr(model, "batched", False):
        raise ValueError("fold-in is defined for skip-gram negative sampling only (sg=1, not batched): the other "
                         "trainers' pair definitions differ")
    if walks_idx.dtype != torch.int32 or walks_idx.dim() != 2 or not walks_idx.is_cuda:
        raise TypeError("fold-in wants a CUDA int32 [rows, len] tensor")
    if walks_idx.shape[1] > sgns.MAX_SENTENCE:
        raise ValueError(f"walks longer than {sgns.MAX_SENTENCE}: split rows first (sgns.split_rows)")
    if int(n_new) < 0:
        raise ValueError("n_new must not be negative")
    return walks_idx.contiguous()


def pair_records(model, walks_idx: torch.Tensor, n_new: int, sentence_base: int = 0
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The trainable pairs of `walks_idx` (int32 [rows, len]; tokens >= n_vocab are new vertices) as records
    int32 [n, 4] = {new index, row, i | rel << 16, centre word}, grouped by new vertex and inside a vertex in
    (row, i, j) order, and vertex_off int64 [n_new + 1]: vertex u owns records[vertex_off[u]:vertex_off[u + 1]]."""
    walks_idx = _check(model, walks_idx, n_new)
    L = _lib.load()
    _lib.require_gpu()
    dev = walks_idx.device
    rows, ln = walks_idx.shape
    n_vocab = int(model.syn1neg.shape[0])
    si = getattr(model, "sample_int", None)
    P = _params(model, n_vocab, sentence_base, 0.0, None, 0)
    counts = torch.zeros(rows, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.n2v_foldin_pair_counts(walks_idx.data_ptr(), rows, ln, int(n_new),
                                            0 if si is None else si.data_ptr(), P, counts.data_ptr(),
                                            _lib.current_stream_ptr()), "n2v_foldin_pair_counts")
        off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=off[1:])
        total = int(off[-1].item())
        records = torch.empty((total, 4), dtype=torch.int32, device=dev)
        if total:
            _lib.check(L.n2v_foldin_pair_records(walks_idx.data_ptr(), rows, ln, int(n_new),
                                                 0 if si is None else si.data_ptr(), P, off.data_ptr(),
                                                 records.data_ptr(), _lib.current_stream_ptr()),
                       "n2v_foldin_pair_records")
    # grouping by vertex: a STABLE sort on the new index keeps the (row, i, j) order inside a vertex
    order = torch.sort(records[:, 0], stable=True).indices
    records = records[order].contiguous()
    vertex_off = torch.zeros(int(n_new) + 1, dtype=torch.int64, device=dev)
    if total:
        torch.cumsum(torch.bincount(records[:, 0].long(), minlength=int(n_new)), 0, out=vertex_off[1:])
    return records, vertex_off


def train_pass(model, records: torch.Tensor, vertex_off: torch.Tensor, new_rows: torch.Tensor, rows: int, length: int,
               alpha: float, sentence_base: int = 0, row_alpha: Optional[torch.Tensor] = None,
               max_waves: int = 0) -> None:
    """One pass of n2v_foldin_train over the records of pair_records(model, walks [rows, length], ...,
    sentence_base): new_rows fp32 [n_new, dim] is updated in place.  max_waves > 0 caps the waves of the launch
    (the result does not depend on it)."""
    L = _lib.load()
    _lib.require_gpu()
    n_new = int(vertex_off.numel()) - 1
    if new_rows.dtype != torch.float32 or not new_rows.is_contiguous() or \
            tuple(new_rows.shape) != (n_new, int(model.syn1neg.shape[1])):
        raise TypeError("new_rows must be a contiguous float32 [n_new, dim] tensor")
    n_vocab = int(model.syn1neg.shape[0])
    P = _params(model, n_vocab, sentence_base, alpha, row_alpha, max_waves)
    with torch.cuda.device(new_rows.device):
        _lib.check(L.n2v_foldin_train(records.data_ptr(), vertex_off.data_ptr(), n_new, int(rows), int(length),
                                      new_rows.data_ptr(), model.syn1neg.data_ptr(), model.cum_table.data_ptr(),
                                      model.exp_table.data_ptr(), P, _lib.current_stream_ptr()), "n2v_foldin_train")


def fold_in(model, walks_idx: torch.Tensor, n_new: int, epochs: int, alpha: float = 0.025, min_alpha: float = 1e-4,
            init: Optional[torch.Tensor] = None, sentence_base: int = 0) -> Tuple[torch.Tensor, int]:
    """Trains rows for `n_new` new vertices and returns (new_rows fp32 [n_new, dim], trained pairs).

    `model`: an sgns.SgnsModel, or any object with its syn0, syn1neg, cum_table, cum_index, sample_int, exp_table,
    window, negative and seed; nothing of it is written.  `walks_idx`: int32 [rows, len] over the grown graph, a
    known word by its vocabulary index, new vertex k as n_vocab + k, anything else dropped.  Epoch e of `epochs`
    uses the sentences sentence_base + e * rows + r and the rate max(min_alpha, alpha - (alpha - min_alpha) * e /
    epochs), as SgnsModel.train does with one launch per epoch.  `init`: the starting rows (copied, never
    aliased); None: sgns.init_syn0(n_new, dim, seed ^ INIT_SEED_XOR)."""
    walks_idx = _check(model, walks_idx, n_new)
    dev = walks_idx.device
    n_new, dim = int(n_new), int(model.syn1neg.shape[1])
    if init is None:
        new_rows = sgns.init_syn0(n_new, dim, (int(model.seed) ^ INIT_SEED_XOR) & (2 ** 64 - 1), dev)
    else:
        if tuple(init.shape) != (n_new, dim):
            raise ValueError(f"init must be [n_new, dim] = [{n_new}, {dim}], not {tuple(init.shape)}")
        new_rows = init.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
    rows, ln = walks_idx.shape
    pairs = 0
    epochs = int(epochs)
    for ep in range(epochs):
        base = int(sentence_base) + ep * rows
        a = max(min_alpha, alpha - (alpha - min_alpha) * (ep / max(epochs, 1)))
        records, vertex_off = pair_records(model, walks_idx, n_new, base)
        pairs += int(records.shape[0])
        if records.shape[0]:
            train_pass(model, records, vertex_off, new_rows, rows, ln, a, base)
    return new_rows, pairs
