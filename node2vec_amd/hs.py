"""Skip-gram hierarchical-softmax trainer: host logic around n2v_hs_train (csrc/n2v_hs.hip).

What Spark ML's Word2Vec does around its training loop (the reference's Node2VecSpark,
embedding.py:182-285; DESIGN.md "Hierarchical softmax"): the vocabulary of sgns.build_vocab, the
Huffman tree of word2vec.c (n2v_hs_tree_build, host C++), sentences cut into rows of at most
maxSentenceLength in-vocabulary tokens, (rand - 0.5) / dim initialisation of syn0, a zero syn1,
and Spark's learning-rate rule per row.  Tensors live on the GPU; the arithmetic of training is
the HIP kernel.
"""
from typing import Optional

import numpy as np
import torch

from node2vec_amd import _lib
from node2vec_amd.sgns import MAX_SENTENCE, Vocab, default_block_rows, exp_table, init_syn0, split_rows

RATE_REFRESH_WORDS = 10000  # Spark refreshes the learning rate every 10 000 words
MIN_RATE_SHARE = 1e-4       # ... and never below stepSize * 1e-4
# hogwild: plain stores on every syn1 row.  Atomic adds on the top inner nodes (n2v_hs_params.hot_nodes)
# were measured slower and worse (profiles/hs_bench.json) and are refused by the library.
HOT_NODES = 0


class HsTree:
    """The Huffman tree of a vocabulary: word w's path is points[path_off[w]:path_off[w + 1]] (syn1
    rows, root first) and its code bit d is (codes[w] >> d) & 1."""

    def __init__(self, path_off: np.ndarray, codes: np.ndarray, points: np.ndarray):
        self.path_off, self.codes, self.points = path_off, codes, points

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.path_off)

    def code(self, w: int):
        return [int((int(self.codes[w]) >> d) & 1) for d in range(int(self.lengths[w]))]

    def path(self, w: int) -> np.ndarray:
        return self.points[self.path_off[w]:self.path_off[w + 1]]


def build_tree(counts) -> HsTree:
    """word2vec.c CreateBinaryTree over `counts` (descending: the vocabulary's order), in the
    library's host code.  ValueError for counts that are not descending or a code longer than 64."""
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().numpy()
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    n = int(counts.shape[0])
    if n < 1:
        raise ValueError("the Huffman tree needs at least one word")
    L = _lib.load()
    off = np.zeros(n + 1, np.int64)
    codes = np.empty(n, np.uint64)
    # one pass: points sized for ceil(log2 V) + 8 levels per word (pages past the real total are never
    # touched); a second pass only for a tree deeper on average than that
    cap = n * min(64, max(1, int(n - 1).bit_length()) + 8)
    points = np.empty(max(cap, 1), np.int32)
    rc = L.n2v_hs_tree_build(counts.ctypes.data, n, off.ctypes.data, codes.ctypes.data, points.ctypes.data, cap)
    if rc == _lib.EINVAL and int(off[-1]) > cap:
        cap = int(off[-1])
        points = np.empty(cap, np.int32)
        rc = L.n2v_hs_tree_build(counts.ctypes.data, n, off.ctypes.data, codes.ctypes.data, points.ctypes.data,
                                 cap)
    _lib.check(rc, "n2v_hs_tree_build")
    total = int(off[-1])
    return HsTree(off, codes, points[:total])


def spark_row_alpha(words_per_row, epoch: int, epochs: int, step_size: float,
                    train_words: Optional[int] = None) -> np.ndarray:
    """Spark ML Word2Vec's learning rate (one partition), the fp32 rate of every row of one epoch:

        alpha = stepSize * max(1e-4, 1 - words_done / (maxIter * train_words + 1))

    `train_words` is the number of in-vocabulary words of one epoch (default: the sum of
    `words_per_row`), and words_done = epoch * train_words + the in-vocabulary words of the rows
    before this one in the epoch, rounded down to a multiple of 10 000 (Spark refreshes the rate every
    10 000 words).  Computed in float64, rounded to fp32 once."""
    w = np.asarray(words_per_row, dtype=np.int64).reshape(-1)
    if train_words is None:
        train_words = int(w.sum())
    before = np.concatenate([np.zeros(1, np.int64), np.cumsum(w)[:-1]]) if w.size else w
    done = float(epoch) * float(train_words) + (before // RATE_REFRESH_WORDS * RATE_REFRESH_WORDS).astype(np.float64)
    share = 1.0 - done / (float(epochs) * float(train_words) + 1.0)
    return (float(step_size) * np.maximum(MIN_RATE_SHARE, share)).astype(np.float32)


def sentences(idx: torch.Tensor, max_sentence_length: int) -> torch.Tensor:
    """Spark's sentences from rows of vocabulary indices (-1 = outside the vocabulary): the
    out-of-vocabulary tokens are dropped, then every row is cut into chunks of at most
    max_sentence_length tokens (and at most MAX_SENTENCE, the kernel's row buffer).  Rows left
    empty are dropped.  int32 [rows, len], -1 padded."""
    if max_sentence_length < 1:
        raise ValueError("maxSentenceLength must be positive")
    keep = idx >= 0
    width = max(1, int(keep.sum(1).max().item())) if idx.numel() else 1
    out = torch.full((idx.shape[0], width), -1, dtype=torch.int32, device=idx.device)
    if idx.numel():
        pos = torch.cumsum(keep.to(torch.int64), 1) - 1
        rows = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand_as(idx)
        out[rows[keep], pos[keep]] = idx[keep].to(torch.int32)
    out = split_rows(out, min(int(max_sentence_length), MAX_SENTENCE))
    return out[(out >= 0).any(1)].contiguous()


class HsModel:
    """The trained state of skip-gram HS: syn0 [V, dim] (the vectors), syn1 [V - 1, dim] (the inner
    nodes of the tree; one unused row when V = 1)."""

    def __init__(self, vocab: Vocab, dim: int, window: int, seed: int, device=None):
        device = device or vocab.ids.device
        n = len(vocab)
        if n == 0:
            raise RuntimeError("you must first build vocabulary before training the model")
        self.vocab, self.dim, self.window = vocab, int(dim), int(window)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.tree = tree = build_tree(vocab.counts)
        self.syn0 = init_syn0(n, self.dim, self.seed, device)
        self.syn1 = torch.zeros((max(n - 1, 1), self.dim), dtype=torch.float32, device=device)
        self.path_off = torch.from_numpy(tree.path_off).to(device)
        pts = tree.points if tree.points.size else np.zeros(1, np.int32)
        self.points = torch.from_numpy(np.ascontiguousarray(pts)).to(device)
        self.codes = torch.from_numpy(tree.codes.view(np.int64)).to(device)  # the uint64 code bits
        self.exp_table = torch.from_numpy(exp_table()).to(device)
        c = vocab.counts.cpu().numpy().astype(np.float64)
        # frequency-weighted mean code length: the path nodes one pair trains on average
        self.mean_code_length = float((c * tree.lengths).sum() / c.sum()) if c.sum() > 0 else 0.0
        self.hot_nodes: Optional[int] = None  # None = HOT_NODES
        self.path_cache = True
        self.max_waves = 0
        self.hogwild_waves_used: Optional[int] = None  # waves in flight of the first hogwild launch
        self._counters = torch.zeros(2, dtype=torch.int64, device=device)
        self.pairs = self._counters[:1]
        self.sentences_seen = 0

    def _params(self, sentence_base: int, alpha: float, deterministic: bool, row_alpha) -> "_lib.HsParams":
        hot = HOT_NODES if self.hot_nodes is None else int(self.hot_nodes)
        return _lib.HsParams(len(self.vocab), int(sentence_base), self.seed, self.dim, self.window, float(alpha),
                             int(bool(deterministic)), 0 if row_alpha is None else row_alpha.data_ptr(),
                             int(self.max_waves), hot, int(bool(self.path_cache)), 0)

    def hogwild_waves(self, rows: int, length: int) -> int:
        """the waves n2v_hs_train keeps in flight for such a launch on this device"""
        L = _lib.load()
        with torch.cuda.device(self.syn0.device):
            w = int(L.n2v_hs_hogwild_waves(self._params(0, 0.025, False, None), int(rows), int(length)))
        if w < 0:
            _lib.check(w, "n2v_hs_hogwild_waves")
        return w

    def train_block(self, rows_idx: torch.Tensor, alpha: float = 0.025, sentence_base: int = 0,
                    deterministic: bool = False, row_alpha: Optional[torch.Tensor] = None):
        """rows_idx: CUDA int32 [rows, len <= MAX_SENTENCE] vocabulary indices (-1 = none); `alpha` is
        the rate of every row unless `row_alpha` (fp32, one per row) is given."""
        L = _lib.load()
        _lib.require_gpu()
        if rows_idx.dtype != torch.int32 or rows_idx.dim() != 2 or not rows_idx.is_cuda:
            raise TypeError("train_block wants a CUDA int32 [rows, len] tensor")
        if rows_idx.shape[1] > MAX_SENTENCE:
            raise ValueError(f"rows longer than {MAX_SENTENCE}: cut them first (sentences / split_rows)")
        rows_idx = rows_idx.contiguous()
        if row_alpha is not None:
            row_alpha = row_alpha.to(device=rows_idx.device, dtype=torch.float32).contiguous()
            if row_alpha.numel() != rows_idx.shape[0]:
                raise ValueError("row_alpha needs one rate per row")
        P = self._params(sentence_base, alpha, deterministic, row_alpha)
        if not deterministic and rows_idx.shape[0] > 0 and self.hogwild_waves_used is None:
            self.hogwild_waves_used = self.hogwild_waves(rows_idx.shape[0], rows_idx.shape[1])
        with torch.cuda.device(rows_idx.device):
            rc = L.n2v_hs_train(rows_idx.data_ptr(), rows_idx.shape[0], rows_idx.shape[1], self.syn0.data_ptr(),
                                self.syn1.data_ptr(), self.path_off.data_ptr(), self.points.data_ptr(),
                                self.codes.data_ptr(), self.exp_table.data_ptr(), P, self.pairs.data_ptr(),
                                _lib.current_stream_ptr())
        _lib.check(rc, "n2v_hs_train")

    def train(self, rows_idx: torch.Tensor, epochs: int, step_size: float = 0.025, sentence_base: int = 0,
              deterministic: bool = False, block_rows: Optional[int] = None):
        """`epochs` passes over the rows (Spark's maxIter) at Spark's rate per row (spark_row_alpha);
        row r of epoch e is sentence sentence_base + e * rows + r of the random stream."""
        rows = rows_idx.shape[0]
        words = (rows_idx >= 0).sum(1).cpu().numpy()
        train_words = int(words.sum())
        if block_rows is None:
            block_rows = default_block_rows(rows)
        for ep in range(int(epochs)):
            ra = torch.from_numpy(spark_row_alpha(words, ep, epochs, step_size, train_words)).to(rows_idx.device)
            for lo in range(0, rows, block_rows):
                hi = min(rows, lo + block_rows)
                self.train_block(rows_idx[lo:hi], step_size, sentence_base + ep * rows + lo, deterministic,
                                 row_alpha=ra[lo:hi])
        self.sentences_seen += rows * int(epochs)
        return self
