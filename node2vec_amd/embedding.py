"""Embedding plugin API: the reference's node2vec/embedding.py with a HIP trainer.

`Node2VecBase` is the reference's abstract plugin interface (embedding.py:22-66:
fit / embedding / get_vector / save_model / load_model, all NotImplementedError).
`Node2VecHIP` mirrors `Node2VecGensim` (embedding.py:70-178): same constructor
arguments, same in-place filling of the caller's w2v_params from GENSIM_PARAMS,
same ValueErrors, same DataFrame shapes -- with the gensim.models.Word2Vec call of
embedding.py:126 replaced by the SGNS kernel.  `Node2VecGensim` is exported as an
alias so `from node2vec.embedding import Node2VecGensim` ports by changing the
package name only.

The one behavioural decision (SURVEY.md finding 4): the reference's defaults
(negative=0 with gensim's sg=0, hs=0) perform no weight updates at all; this
trainer uses negative sampling, so a missing/zero `negative` becomes 5 and a missing `sg`
means 1, skip-gram (constants.HIP_SGNS_PARAMS).  sg=0 trains CBOW with negative sampling,
gensim's own default objective (csrc/n2v_cbow.hip; `cbow_mean` 1 or 0 as in gensim).  hs=1 is
rejected with ValueError.
"""
import logging
import os
import time
from typing import Any, Dict, List, Optional, Union

import numpy as np
import pandas as pd
import torch

from node2vec_amd import corpus, sgns
from node2vec_amd.constants import GENSIM_PARAMS, HIP_SGNS_PARAMS, WORD2VEC_PARAMS


class Node2VecBase(object):
    """Base class for conducting Node2Vec in various computing frameworks
    (embedding.py:22-66)."""

    def __init__(self):
        pass

    def fit(self):
        raise NotImplementedError()

    def embedding(self):
        raise NotImplementedError()

    def get_vector(self, vertex_id: Union[str, int]):
        raise NotImplementedError()

    def save_model(self, file_path: str, file_name: str):
        raise NotImplementedError()

    def load_model(self, file_path: str, file_name: str):
        raise NotImplementedError()


class _Tokens:
    """index -> token, lazily: the tokens of a fitted model are the decimal strings of its vertex
    ids (embedding.py:125); at BASELINE cfg 4 a list of 10^8 Python strings is ~6 GB of objects
    nobody reads, so the ids stay an int64 array and strings are made on access."""

    def __init__(self, ids: np.ndarray):
        self.ids = ids

    def __len__(self):
        return int(self.ids.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [str(int(x)) for x in self.ids[i]]
        return str(int(self.ids[i]))

    def __iter__(self):
        for lo in range(0, len(self), 1 << 16):
            yield from map(str, self.ids[lo:lo + (1 << 16)].tolist())

    def __eq__(self, other):
        return len(self) == len(other) and all(a == b for a, b in zip(self, other))


class _Vocab:
    """token -> row, lazily (what callers of the reference do with model.wv.vocab: `in`, `[]`,
    `len`, iteration in index order -- embedding.py:135-136).  Lookup through a sorted copy of the
    id array, built on first use (searchsorted): no 10^8-entry dict."""

    def __init__(self, ids: np.ndarray):
        self.ids = ids
        self._sorted = None

    def _row(self, token) -> int:
        try:
            v = int(token)
        except (TypeError, ValueError):
            return -1
        if str(v) != str(token):  # "07", " 7": not a token this vocabulary ever produced
            return -1
        if self._sorted is None:
            order = np.argsort(self.ids, kind="stable")
            self._sorted = (self.ids[order], order)
        keys, order = self._sorted
        k = int(np.searchsorted(keys, v))
        return int(order[k]) if k < keys.shape[0] and keys[k] == v else -1

    def __contains__(self, token):
        return self._row(token) >= 0

    def __getitem__(self, token):
        r = self._row(token)
        if r < 0:
            raise KeyError(token)
        return r

    def get(self, token, default=None):
        r = self._row(token)
        return default if r < 0 else r

    def __len__(self):
        return int(self.ids.shape[0])

    def __iter__(self):
        return iter(_Tokens(self.ids))

    def keys(self):
        return iter(self)

    def items(self):
        return ((t, i) for i, t in enumerate(self))


class KeyedVectors:
    """What callers of the reference touch on model.wv: `vocab` (token -> row; tokens
    are decimal strings of vertex ids, embedding.py:125), `wv[token]`, `index2word`, `vectors`
    and the word2vec text format.

    `tokens`: a list of strings (a loaded text file), or an integer id array / tensor (a fitted
    model: tokens and the token -> row map are then lazy).  `vectors`: numpy [n, dim], or the
    trainer's device tensor -- it stays in HBM; `wv[token]` copies one row, `.vectors` converts
    the whole matrix to numpy on first access (51 GB at cfg 4: ask for rows or chunks instead,
    `rows(lo, hi)`)."""

    def __init__(self, tokens, vectors):
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.cpu().numpy()
        if isinstance(tokens, np.ndarray) and tokens.dtype.kind in "iu":
            self.ids: Optional[np.ndarray] = tokens.astype(np.int64, copy=False)
            self.index2word = _Tokens(self.ids)
            self.vocab = _Vocab(self.ids)
        else:
            self.ids = None
            self.index2word = list(tokens)
            self.vocab = {t: i for i, t in enumerate(self.index2word)}
        self._vectors = vectors
        self.vector_size = int(vectors.shape[1]) if vectors.ndim == 2 else 0
        # query caches (never saved): the matrix on the GPU, its inverse row norms (init_sims)
        self._dev = vectors if isinstance(vectors, torch.Tensor) and vectors.is_cuda else None
        self._inv_norm: Optional[torch.Tensor] = None

    @property
    def vectors(self) -> np.ndarray:
        if isinstance(self._vectors, torch.Tensor):
            self._vectors = self._vectors.cpu().numpy()
        return self._vectors

    def rows(self, lo: int, hi: int) -> np.ndarray:
        """vectors[lo:hi] as numpy without converting the whole matrix"""
        v = self._vectors[lo:hi]
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else v

    def __len__(self):
        return len(self.index2word)

    def __getitem__(self, token: str) -> np.ndarray:
        r = self.vocab[token]
        return self.rows(r, r + 1)[0]

    def __contains__(self, token: str) -> bool:
        return token in self.vocab

    def save_word2vec_format(self, fname: str, chunk_rows: int = 1 << 16) -> None:
        with open(fname, "w") as f:
            f.write(f"{len(self.index2word)} {self.vector_size}\n")
            for lo in range(0, len(self), chunk_rows):
                block = self.rows(lo, lo + chunk_rows).astype(np.float64).tolist()
                toks = self.index2word[lo:lo + chunk_rows]
                f.writelines(t + " " + " ".join(map(repr, v)) + "\n" for t, v in zip(toks, block))

    # -- similarity queries (gensim 3.8 KeyedVectors; csrc/n2v_knn.hip) -----------------------
    def _device_vectors(self) -> torch.Tensor:
        """the matrix on the GPU: the trainer's tensor, or a copy of host vectors made on the first query"""
        if self._dev is None:
            from node2vec_amd import _lib

            v = self._vectors
            v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
            self._dev = v.to(device=_lib.require_gpu(), dtype=torch.float32).contiguous()
        return self._dev

    def init_sims(self, replace: bool = False) -> None:
        """Caches 1 / ||v|| of every row on the GPU (the normalised copy gensim builds is never made)."""
        if replace:
            raise NotImplementedError("init_sims(replace=True): the vectors are kept as trained")
        if self._inv_norm is None:
            from node2vec_amd import similarity

            self._inv_norm = similarity.inv_norms(self._device_vectors())

    def _row_of(self, token) -> int:
        if isinstance(token, (int, np.integer)) and not isinstance(token, bool):
            token = str(int(token))  # as get_vector
        return self.vocab[token]  # KeyError for an unknown token

    def _query(self, positive, negative):
        """gensim 3.8 most_similar's mean: (unit query fp32 [dim], rows of the input tokens).  Tokens are
        looked up (KeyError) and the input checked (ValueError) before the GPU is touched."""
        def items(arg, weight):
            if arg is None:
                return []
            if isinstance(arg, (str, int, np.integer, np.ndarray)):
                arg = [arg]  # a bare token (or vector)
            out = []
            for it in arg:
                if isinstance(it, tuple) and len(it) == 2 and not isinstance(it[0], tuple):
                    out.append((it[0], float(it[1])))
                else:
                    out.append((it, weight))
            return out

        parsed = []
        for item, weight in items(positive, 1.0) + items(negative, -1.0):
            if isinstance(item, (np.ndarray, torch.Tensor)):
                vec = np.asarray(item.cpu() if isinstance(item, torch.Tensor) else item, dtype=np.float32)
                if vec.shape != (self.vector_size,):
                    raise ValueError(f"a query vector must have {self.vector_size} values")
                parsed.append((None, vec, weight))
            else:
                parsed.append((self._row_of(item), None, weight))
        if not parsed:
            raise ValueError("cannot compute similarity with no input")
        mean = []
        for row, vec, weight in parsed:
            if row is not None:  # a token: its unit vector (gensim's vectors_norm row)
                v = self.rows(row, row + 1)[0].astype(np.float32)
                norm = np.float32(np.sqrt(np.dot(v, v)))
                vec = v / norm if norm > 0 else v
            mean.append(np.float32(weight) * vec)
        mean = np.mean(np.asarray(mean, dtype=np.float32), axis=0, dtype=np.float32)
        norm = np.float32(np.sqrt(np.dot(mean, mean)))
        query = mean / norm if norm > 0 else mean
        return query.astype(np.float32), sorted({row for row, _, _ in parsed if row is not None})

    def build_index(self, nlist: Optional[int] = None, nprobe: int = 8, seed: int = 0, pq: Optional[int] = None,
                    refine: int = 4, **kw):
        """An inverted-file index over the vectors for approximate queries (node2vec_amd.ann.build_index, whose other
        arguments pass through): spherical k-means into nlist lists over the cached init_sims norms.  Hand it to
        most_similar / similar_by_* / nearest as indexer=; its nprobe (lists scanned per query) may be set at any
        time.  It indexes the vectors as they are now.  pq=m: an IVFPQIndex (ann.build_pq: m bytes per vector,
        trained with the same seed), searched by ann.search_pq -- approximate scores over the codes, the best
        refine * topn of them scored exactly again (index.refine, settable; 0: the approximate scores as they
        are)."""
        from node2vec_amd import ann

        self.init_sims()
        X = self._device_vectors()
        index = ann.build_index(X, nlist=nlist, nprobe=nprobe, seed=seed, inv_norm=self._inv_norm, **kw)
        if pq is None:
            return index
        if int(refine) < 0:
            raise ValueError("refine must be >= 0")
        index = ann.build_pq(X, index, pq, seed=seed, inv_norm=self._inv_norm)
        index.refine = int(refine)
        return index

    def _index_search(self, indexer, k: int, **kw):
        """ann.search, or ann.search_pq for an index with product-quantised codes"""
        from node2vec_amd import ann

        X = self._device_vectors()
        if isinstance(indexer, ann.IVFPQIndex):
            return ann.search_pq(indexer, k, X=X, refine=indexer.refine, inv_norm=self._inv_norm, **kw)
        return ann.search(X, indexer, k, inv_norm=self._inv_norm, **kw)

    @staticmethod
    def _check_indexer(topn, restrict_vocab) -> None:
        if restrict_vocab is not None:
            raise ValueError("restrict_vocab cannot be combined with indexer=: the index covers every row")
        if topn is None:
            raise ValueError("topn=None (every score) cannot be combined with indexer=")

    def most_similar(self, positive=None, negative=None, topn: Optional[int] = 10,
                     restrict_vocab: Optional[int] = None, indexer=None):
        """gensim 3.8 KeyedVectors.most_similar: [(token, cosine)] of the topn nearest rows to the unit mean of
        weight * unit(token vector) (weight +1 for positive, -1 for negative, or given as (item, weight));
        a vector given as such enters as it is, as in gensim.  The input tokens are not returned.
        topn=None: the whole fp32 score array.  restrict_vocab: only the first rows are searched.
        A row holding inf or NaN (or a query that does) scores NaN: it is never returned, for every topn, so
        fewer than topn pairs may come back; topn=None returns the NaN scores.
        indexer (gensim's argument; an index from build_index): only the lists the index probes are searched --
        the same scores, the nearest rows among those lists; not with restrict_vocab or topn=None."""
        if indexer is not None:
            self._check_indexer(topn, restrict_vocab)
        if topn is not None and topn < 1:
            return []
        query, own = self._query(positive, negative)
        from node2vec_amd import similarity

        self.init_sims()
        X = self._device_vectors()
        q = torch.from_numpy(query).to(X.device)
        if topn is None:
            return similarity.scores(X, queries=q, restrict=restrict_vocab, inv_norm=self._inv_norm)[0].cpu().numpy()
        if indexer is not None:
            rows, scores = self._index_search(indexer, int(topn) + len(own), queries=q)
        else:
            rows, scores = similarity.knn(X, int(topn) + len(own), queries=q, restrict=restrict_vocab,
                                          inv_norm=self._inv_norm)
        rows, scores = rows[0].cpu().numpy(), scores[0].cpu().numpy()
        own = set(own)
        out = [(self.index2word[int(r)], float(s)) for r, s in zip(rows, scores) if r >= 0 and int(r) not in own]
        return out[:int(topn)]

    def similar_by_word(self, word, topn: Optional[int] = 10, restrict_vocab: Optional[int] = None, indexer=None):
        return self.most_similar(positive=[word], topn=topn, restrict_vocab=restrict_vocab, indexer=indexer)

    def similar_by_vector(self, vector, topn: Optional[int] = 10, restrict_vocab: Optional[int] = None, indexer=None):
        return self.most_similar(positive=[np.asarray(vector, dtype=np.float32)], topn=topn,
                                 restrict_vocab=restrict_vocab, indexer=indexer)

    def similarity(self, w1, w2) -> float:
        """cosine of two tokens (gensim: dot(unitvec(wv[w1]), unitvec(wv[w2])))"""
        a, b = (self.rows(r, r + 1)[0].astype(np.float32) for r in (self._row_of(w1), self._row_of(w2)))
        na, nb = np.float32(np.sqrt(np.dot(a, a))), np.float32(np.sqrt(np.dot(b, b)))
        return float(np.dot(a / na if na > 0 else a, b / nb if nb > 0 else b))

    def nearest(self, rows, topn: int = 10, exclude_self: bool = True, restrict_vocab: Optional[int] = None,
                indexer=None):
        """The batched form: for every row number in `rows`, its topn nearest rows -- device tensors
        (rows int64 [len(rows), topn], cosines fp32), best first, a query's own row left out.  indexer (an index
        from build_index): the nearest among the lists the index probes; not with restrict_vocab."""
        from node2vec_amd import similarity

        if indexer is not None:
            self._check_indexer(topn, restrict_vocab)
        self.init_sims()
        if indexer is not None:
            return self._index_search(indexer, topn, rows=rows, exclude_self=exclude_self)
        return similarity.knn(self._device_vectors(), topn, rows=rows, restrict=restrict_vocab,
                              inv_norm=self._inv_norm, exclude_self=exclude_self)

    def _rows_of_tokens(self, tokens) -> np.ndarray:
        """rows int64 of a sequence of tokens (ints stand for their decimal strings); KeyError for an unknown one"""
        if isinstance(tokens, (str, int, np.integer)):
            tokens = [tokens]
        return np.fromiter((self._row_of(t) for t in tokens), dtype=np.int64)

    def _pair_rows(self, tokens_a, tokens_b):
        """the rows of two token lists of one length: looked up (KeyError) and checked (ValueError) before the GPU
        is touched"""
        ra, rb = self._rows_of_tokens(tokens_a), self._rows_of_tokens(tokens_b)
        if ra.shape[0] != rb.shape[0]:
            raise ValueError(f"tokens_a and tokens_b must have the same length, not {ra.shape[0]} and {rb.shape[0]}")
        return ra, rb

    def pair_scores(self, tokens_a, tokens_b, metric: str = "cosine") -> np.ndarray:
        """score of every pair (tokens_a[i], tokens_b[i]), fp32 [n]: "cosine" (gensim's similarity, over the cached
        init_sims norms) or "dot" (csrc/n2v_pairs.hip; every score in one fixed order, symmetric in the pair)"""
        from node2vec_amd import linkpred

        if metric not in linkpred.METRICS:
            raise ValueError(f"metric {metric!r}: " + " | ".join(linkpred.METRICS))
        ra, rb = self._pair_rows(tokens_a, tokens_b)
        X = self._device_vectors()
        if metric == "cosine":
            self.init_sims()
        return linkpred.pair_scores(X, torch.from_numpy(ra), torch.from_numpy(rb), metric,
                                    inv_norm=self._inv_norm).cpu().numpy()

    def edge_features(self, tokens_a, tokens_b, op: str = "hadamard") -> np.ndarray:
        """the node2vec paper's edge feature of every pair, fp32 [n, dim]: "average" | "hadamard" | "l1" | "l2" """
        from node2vec_amd import linkpred

        if op not in linkpred.OPERATORS:
            raise ValueError(f"operator {op!r}: " + " | ".join(linkpred.OPERATORS))
        ra, rb = self._pair_rows(tokens_a, tokens_b)
        return linkpred.pair_features(self._device_vectors(), torch.from_numpy(ra), torch.from_numpy(rb),
                                      op).cpu().numpy()

    def fit_edges(self, tokens_a, tokens_b, y, op: str = "hadamard", **kw):
        """the node2vec paper's link-prediction classifier on the pairs (tokens_a[i], tokens_b[i]) with labels y
        (nonzero: an edge): linkpred.fit_edges on the vectors, whose other arguments pass through -> EdgeClassifier"""
        from node2vec_amd import linkpred

        if op not in linkpred.OPERATORS:
            raise ValueError(f"operator {op!r}: " + " | ".join(linkpred.OPERATORS))
        ra, rb = self._pair_rows(tokens_a, tokens_b)
        return linkpred.fit_edges(self._device_vectors(), torch.from_numpy(ra), torch.from_numpy(rb),
                                  torch.as_tensor(np.asarray(y)), op=op, **kw)

    def edge_scores(self, tokens_a, tokens_b, result) -> np.ndarray:
        """the score of every pair under a fitted EdgeClassifier, fp32 [n]: dot(w, op(x_a, x_b)) + b (> 0: an edge)"""
        from node2vec_amd import linkpred

        ra, rb = self._pair_rows(tokens_a, tokens_b)
        return linkpred.edge_scores(self._device_vectors(), torch.from_numpy(ra), torch.from_numpy(rb), result.w,
                                    result.b, result.op).cpu().numpy()

    def target_ranks(self, tokens_a, tokens_b, graph=None, metric: str = "cosine"):
        """where tokens_b[i] stands among the whole vocabulary as a partner of tokens_a[i]: (greater, equal int64 [n],
        thr fp32 [n]) -- how many tokens score above, and equal to, tokens_b[i] against tokens_a[i], and that score
        (linkpred.target_ranks; csrc/n2v_linkrank.hip: no [n, vocabulary] score matrix is made).  graph: a DeviceGraph
        over vertex ids, for tokens that are vertex ids: the neighbours tokens_a[i] has in it are not candidates."""
        from node2vec_amd import linkpred

        if metric not in linkpred.METRICS:
            raise ValueError(f"metric {metric!r}: " + " | ".join(linkpred.METRICS))
        ra, rb = self._pair_rows(tokens_a, tokens_b)
        X = self._device_vectors()
        if metric == "cosine":
            self.init_sims()
        filt = None if graph is None else linkpred.rows_graph(graph.to(X.device), self)
        greater, equal, thr = linkpred.target_ranks(X, torch.from_numpy(ra), torch.from_numpy(rb), graph=filt,
                                                    metric=metric, inv_norm=self._inv_norm)
        return greater.cpu().numpy(), equal.cpu().numpy(), thr.cpu().numpy()

    def kmeans(self, k: int, metric: str = "cosine", restrict_vocab: Optional[int] = None, **kw):
        """k-means of the vectors on the GPU (node2vec_amd.cluster.kmeans, whose other arguments pass through):
        a KMeansResult whose labels[i] is the cluster of row i (token index2word[i]).  The default metric is
        cosine (spherical k-means over the cached init_sims norms), as every similarity of this class is a
        cosine; cluster.kmeans itself defaults to "euclidean" as scikit-learn does.  restrict_vocab: only the
        first rows are clustered."""
        from node2vec_amd import cluster

        cluster.check_metric(metric)
        cluster.check_k(k, self._first_rows(restrict_vocab))
        X, inv_norm = self._window(restrict_vocab, metric == "cosine")
        return cluster.kmeans(X, k, metric=metric, inv_norm=inv_norm, **kw)

    def dbscan(self, eps: float, min_samples: int = 5, metric: str = "cosine", restrict_vocab: Optional[int] = None,
               **kw):
        """DBSCAN of the vectors on the GPU (node2vec_amd.cluster.dbscan, whose other arguments pass through): a
        DBSCANResult whose labels[i] is the cluster of row i (token index2word[i]), -1 for noise.  The default
        metric is cosine (1 - cosine <= eps over the cached init_sims norms), as for kmeans; cluster.dbscan itself
        defaults to "euclidean" as scikit-learn does.  restrict_vocab: only the first rows are clustered."""
        from node2vec_amd import cluster

        cluster.check_metric(metric)
        X, inv_norm = self._window(restrict_vocab, metric == "cosine")
        return cluster.dbscan(X, eps, min_samples, metric=metric, inv_norm=inv_norm, **kw)

    def silhouette(self, labels_or_result, metric: str = "cosine", restrict_vocab: Optional[int] = None, **kw):
        """the silhouette of every vector under a clustering, on the GPU (node2vec_amd.cluster.silhouette_samples,
        whose other arguments pass through): a SilhouetteResult.  labels_or_result: a label tensor (one per row,
        or per row of restrict_vocab) or a KMeansResult.  The default metric is cosine over the cached init_sims
        norms, as for kmeans: score a clustering by the metric it was made with."""
        from node2vec_amd import cluster

        cluster.check_metric(metric)
        X, inv_norm = self._window(restrict_vocab, metric == "cosine")
        return cluster.silhouette_samples(X, labels_or_result, metric=metric, inv_norm=inv_norm, **kw)

    def logreg(self, Y, restrict_vocab: Optional[int] = None, **kw):
        """one-vs-rest logistic regression of the vectors on the GPU (node2vec_amd.classify.fit, whose other
        arguments pass through): a LogRegResult; row i of Y (bool or 0/1 [n, c]) holds the labels of token
        index2word[i].  restrict_vocab: only the first rows are used."""
        from node2vec_amd import classify

        n = self._first_rows(restrict_vocab)
        Y = torch.as_tensor(Y)
        if Y.ndim != 2 or Y.shape[0] < n:
            raise ValueError(f"Y must hold one row of labels per vector: [{n}, c]")
        return classify.fit(self._window(restrict_vocab, False)[0], Y[:n], **kw)

    def label_scores(self, result) -> torch.Tensor:
        """fp32 [n, c] on the device: the decision function of a LogRegResult for every vector"""
        from node2vec_amd import classify

        return classify.decision_function(self._device_vectors(), result.W, result.b)

    def _first_rows(self, restrict_vocab: Optional[int]) -> int:
        n = len(self)
        if restrict_vocab is not None:
            if int(restrict_vocab) < 0:
                raise ValueError("restrict_vocab must be >= 0")
            n = min(n, int(restrict_vocab))
        return n

    def _window(self, restrict_vocab: Optional[int], cosine: bool):
        """(the first rows of the matrix on the GPU, their cached init_sims norms -- None unless cosine)"""
        n = self._first_rows(restrict_vocab)
        if cosine:
            self.init_sims()
        return self._device_vectors()[:n], self._inv_norm[:n] if cosine else None

    def pca(self, n_components: Optional[int] = 2, metric: str = "cosine", restrict_vocab: Optional[int] = None,
            **kw):
        """principal components of the vectors on the GPU (node2vec_amd.pca.fit, whose other arguments pass
        through): a PCAResult.  metric "cosine" (the default, as for kmeans) takes the rows as unit vectors over
        the cached init_sims norms; "euclidean" takes them as trained.  restrict_vocab: only the first rows are
        fitted."""
        from node2vec_amd import cluster, pca

        cluster.check_metric(metric)
        self._first_rows(restrict_vocab)  # its ValueError first, as before
        pca.check_components(n_components, self.vector_size)
        X, inv_norm = self._window(restrict_vocab, metric == "cosine")
        return pca.fit(X, n_components, unit=metric == "cosine", inv_norm=inv_norm, **kw)

    def project(self, result, restrict_vocab: Optional[int] = None) -> torch.Tensor:
        """fp32 [n, k] on the device: row i is token index2word[i] on the components of a PCAResult
        (node2vec_amd.pca.transform); NaN for a vector that holds a non-finite value"""
        from node2vec_amd import pca

        X, inv_norm = self._window(restrict_vocab, result.unit)
        return pca.transform(X, result, inv_norm=inv_norm)

    def tsne(self, perplexity: float = 30.0, restrict_vocab: Optional[int] = None, **kw):
        """the t-SNE map of the vectors on the GPU (node2vec_amd.tsne.fit, whose other arguments pass through): a
        TSNEResult whose embedding[i] is the 2-D point of token index2word[i].  The neighbours are cosine over the
        cached init_sims norms.  The exact gradient costs O(n^2) per iteration: restrict_vocab fits only the first
        rows."""
        from node2vec_amd import tsne

        X, inv_norm = self._window(restrict_vocab, True)
        return tsne.fit(X, perplexity=perplexity, inv_norm=inv_norm, **kw)

    def umap(self, n_neighbors: int = 15, restrict_vocab: Optional[int] = None, **kw):
        """the UMAP layout of the vectors on the GPU (node2vec_amd.umap.fit, whose other arguments pass through): a
        UMAPResult whose embedding[i] is the 2-D point of token index2word[i].  The neighbours are cosine over the
        cached init_sims norms.  An epoch costs O(n n_neighbors): this is the map for vocabularies past t-SNE's
        reach.  restrict_vocab fits only the first rows."""
        from node2vec_amd import umap

        X, inv_norm = self._window(restrict_vocab, True)
        return umap.fit(X, n_neighbors=n_neighbors, inv_norm=inv_norm, **kw)

    def with_rows(self, tokens, rows) -> "KeyedVectors":
        """A new KeyedVectors holding this one's rows followed by `rows` [m, dim] under `tokens` (m vertex ids or
        strings: the vertices Node2VecHIP.infer_vertices folded in), so that most_similar, build_index, kmeans and
        the rest run on the extended set.  This object is untouched and shares no memory with the result."""
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.cpu().numpy()
        tokens = np.asarray(tokens) if not isinstance(tokens, np.ndarray) else tokens
        if rows.ndim != 2 or rows.shape[0] != tokens.shape[0] or int(rows.shape[1]) != self.vector_size:
            raise ValueError(f"with_rows wants {tokens.shape[0]} rows of {self.vector_size} values, "
                             f"not {tuple(rows.shape)}")
        if self.ids is not None and tokens.dtype.kind in "iu":
            names = np.concatenate([self.ids, tokens.astype(np.int64)])
        else:
            names = list(self.index2word) + [str(t) for t in tokens.tolist()]
        if len(set(names.tolist() if isinstance(names, np.ndarray) else names)) != len(names):
            raise ValueError("with_rows: a token is already in the vocabulary, or is given twice")
        old = self._vectors
        if isinstance(old, torch.Tensor):
            new = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows))
            vectors = torch.cat([old, new.to(device=old.device, dtype=old.dtype)], 0)
        else:
            new = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
            vectors = np.concatenate([old, new.astype(old.dtype, copy=False)], 0)
        return KeyedVectors(names, vectors)

    @classmethod
    def load_word2vec_format(cls, fname: str) -> "KeyedVectors":
        with open(fname) as f:
            n, dim = (int(x) for x in f.readline().split())
            tokens, rows = [], np.zeros((n, dim), np.float32)
            for i in range(n):
                parts = f.readline().rstrip("\n").split(" ")
                tokens.append(parts[0])
                rows[i] = np.asarray(parts[1:1 + dim], dtype=np.float32)
        return cls(tokens, rows)


class HipW2V:
    """The fitted model object returned by fit() (stands where gensim's Word2Vec
    object stands): .wv plus the output matrix and the training parameters.  The matrices may be
    the trainer's device tensors (they are converted when saved or read as numpy)."""

    def __init__(self, wv: KeyedVectors, syn1neg, params: Dict[str, Any], pairs: int):
        self.wv, self._syn1neg, self.params, self.pairs_trained = wv, syn1neg, dict(params), pairs

    @property
    def syn1neg(self) -> np.ndarray:
        if isinstance(self._syn1neg, torch.Tensor):
            self._syn1neg = self._syn1neg.cpu().numpy()
        return self._syn1neg

    def save(self, fname: str) -> None:
        tokens = self.wv.ids if self.wv.ids is not None else self.wv.index2word
        torch.save({"tokens": tokens, "vectors": self.wv.vectors,
                    "syn1neg": self.syn1neg, "params": self.params,
                    "pairs": self.pairs_trained}, fname)

    @classmethod
    def load(cls, fname: str) -> "HipW2V":
        d = torch.load(fname, weights_only=False)
        return cls(KeyedVectors(d["tokens"], d["vectors"]), d["syn1neg"], d["params"], d["pairs"])


def _check_objective(p: Dict[str, Any]) -> None:
    """hs=1 is not trained by this class; sg=0 is CBOW, which has no batched variant"""
    if p.get("hs", 0):
        raise ValueError("the HIP trainer implements hs=0 (negative sampling): sg=1 skip-gram, sg=0 CBOW")
    if p.get("sg", 1) not in (0, 1, False, True):
        raise ValueError(f"sg must be 0 (CBOW) or 1 (skip-gram), not {p['sg']!r}")
    if p.get("cbow_mean", 1) not in (0, 1, False, True):
        raise ValueError(f"cbow_mean must be 0 (sum) or 1 (mean), not {p['cbow_mean']!r}")
    if not p.get("sg", 1) and p.get("batched", False):
        raise ValueError("batched is a skip-gram trainer: not available with sg=0 (CBOW)")


class _ModelQueries:
    """The queries of a fitted model that Node2VecHIP and Node2VecSpark share: link_scores() / edge_embedding(),
    link_classifier() / link_classifier_scores(), cluster() / silhouette(), classify(), project(), tsne() and umap().  They
    answer per vertex in vocabulary order, under ["id"], or ["name"] through name_id: a repeated id keeps its last
    name, and an id of the vocabulary that name_id does not list is a KeyError -- raised before any GPU work."""

    model = None
    name_id = None
    clusters = None
    kmeans_result = None
    silhouette_score = None
    _cluster_metric = "cosine"
    classifier = None
    edge_classifier = None
    label_f1 = None
    pca_result = None
    tsne_result = None
    umap_result = None
    dbscan_result = None

    def _wv(self) -> KeyedVectors:
        if self.model is None:
            raise ValueError("Model is not available. Please run fit()")
        return self.model.wv

    @staticmethod
    def _vocab_ids(wv: KeyedVectors, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """the vertex ids of rows [lo, hi), int64"""
        if wv.ids is not None:
            return wv.ids[lo:hi]
        return np.array([int(t) for t in wv.index2word[lo:hi]], dtype=np.int64)

    def _names(self) -> Optional[pd.Series]:
        """name_id as id -> name (embedding.py:139-140 builds a dict: a repeated id keeps its LAST name)"""
        if self.name_id is None:
            return None
        return self.name_id.drop_duplicates("id", keep="last").set_index("id")["name"]

    def _who(self, ids: np.ndarray, names=False):
        """("id", ids), or ("name", their names); KeyError: the first of `ids` that name_id does not list.
        names: self._names(), for a caller that asks more than once"""
        names = self._names() if names is False else names
        if names is None:
            return "id", ids
        missing = ~pd.Index(ids).isin(names.index)
        if missing.any():
            raise KeyError(int(np.asarray(ids)[missing][0]))
        return "name", names.reindex(ids).to_numpy()

    def _edge_ids(self, df_edges: pd.DataFrame):
        """`df_edges` holds vertex ids in columns "src" and "dst"; an id outside the vocabulary is a KeyError"""
        self._wv()
        if "src" not in df_edges.columns or "dst" not in df_edges.columns:
            raise ValueError('df_edges must have the columns "src" and "dst"')
        return df_edges["src"].to_numpy(), df_edges["dst"].to_numpy()

    def link_scores(self, df_edges: pd.DataFrame, metric: str = "cosine") -> pd.DataFrame:
        """["src", "dst", "score"]: the score of every row's pair of vertices (model.wv.pair_scores)"""
        src, dst = self._edge_ids(df_edges)
        return pd.DataFrame({"src": src, "dst": dst, "score": self.model.wv.pair_scores(src, dst, metric)})

    def edge_embedding(self, df_edges: pd.DataFrame, operator: str = "hadamard") -> pd.DataFrame:
        """["src", "dst", "vector"]: the edge feature of every row's pair of vertices (model.wv.edge_features)"""
        src, dst = self._edge_ids(df_edges)
        vectors = corpus.list_column(self.model.wv.edge_features(src, dst, operator))
        return pd.DataFrame({"src": src, "dst": dst, "vector": vectors})

    def link_classifier(self, df_pairs: pd.DataFrame, operator: str = "hadamard", **kw):
        """The node2vec paper's link-prediction classifier (section 4.4): logistic regression on the edge feature of
        every row's pair of vertices, df_pairs holding ["src", "dst", "label"] (label nonzero: an edge)
        (model.wv.fit_edges, whose other arguments pass through).  Returns the EdgeClassifier, kept as
        self.edge_classifier."""
        src, dst = self._edge_ids(df_pairs)
        if "label" not in df_pairs.columns:
            raise ValueError('df_pairs must have the column "label"')
        self.edge_classifier = self.model.wv.fit_edges(src, dst, df_pairs["label"].to_numpy(), op=operator, **kw)
        return self.edge_classifier

    def link_classifier_scores(self, df_edges: pd.DataFrame, result=None) -> pd.DataFrame:
        """["src", "dst", "score"]: the score of every row's pair of vertices under `result` (an EdgeClassifier;
        default: the one link_classifier() kept) (model.wv.edge_scores)"""
        src, dst = self._edge_ids(df_edges)
        result = self.edge_classifier if result is None else result
        if result is None:
            raise ValueError("No classifier is available. Please run link_classifier()")
        return pd.DataFrame({"src": src, "dst": dst, "score": self.model.wv.edge_scores(src, dst, result)})

    def link_ranking(self, df_test_edges: pd.DataFrame, df_train_edges: Optional[pd.DataFrame] = None,
                     ks=(1, 10, 50, 100), metric: str = "cosine", both: bool = True) -> pd.DataFrame:
        """One row ["mrr", "mean_rank", "hits@k" for every k of ks, "n", "dropped"]: the filtered ranking of the
        held-out edges of df_test_edges (["src", "dst"], vertex ids) among every vocabulary vertex
        (linkpred.link_ranking: with `both`, dst among the partners of src and src among those of dst).
        df_train_edges (["src", "dst"], the arcs as stored: both directions of an undirected edge): the graph the
        vectors were trained on, whose edges are not candidates; None: nothing is filtered.  A test vertex outside the
        vocabulary is dropped and counted."""
        from node2vec_amd import linkpred
        from node2vec_amd.graph import DeviceGraph

        wv = self._wv()
        src, dst = self._edge_ids(df_test_edges)
        train = None
        if df_train_edges is not None:
            tsrc, tdst = self._edge_ids(df_train_edges)
            train = DeviceGraph.from_edges(tsrc, tdst, device=wv._device_vectors().device)
        out = linkpred.link_ranking(train, wv, src, dst, ks=ks, metric=metric, both=both)
        return pd.DataFrame([out])

    def cluster(self, k: int, metric: str = "cosine", **kw) -> pd.DataFrame:
        """["id" | "name", "cluster"]: the k-means cluster of every vocabulary vertex, in vocabulary order
        (model.wv.kmeans, whose other arguments pass through; -1: a vertex whose vector holds NaN).  The default
        metric is cosine, as in the rest of this class; node2vec_amd.cluster.kmeans defaults to "euclidean".
        Names go through name_id as in most_similar(): a repeated id keeps its last name, an id that name_id does
        not list is a KeyError.  The DataFrame is kept as self.clusters, the KMeansResult as self.kmeans_result."""
        wv = self._wv()
        column, who = self._who(self._vocab_ids(wv))
        self.kmeans_result = wv.kmeans(k, metric=metric, **kw)
        self.clusters = pd.DataFrame({column: who, "cluster": self.kmeans_result.labels.cpu().numpy()})
        self._cluster_metric = metric
        return self.clusters

    def dbscan(self, eps: float, min_samples: int = 5, metric: str = "cosine", **kw) -> pd.DataFrame:
        """["id" | "name", "cluster"]: the DBSCAN cluster of every vocabulary vertex, in vocabulary order, -1 for a
        noise vertex (model.wv.dbscan, whose other arguments pass through).  The default metric is cosine, as in
        cluster().  Names go through name_id as in cluster().  The DBSCANResult is kept as self.dbscan_result;
        self.clusters and self.kmeans_result stay those of cluster()."""
        wv = self._wv()
        column, who = self._who(self._vocab_ids(wv))
        self.dbscan_result = wv.dbscan(eps, min_samples, metric=metric, **kw)
        labels = self.dbscan_result.labels.cpu().numpy()
        return pd.DataFrame({column: who[:len(labels)], "cluster": labels})

    def silhouette(self) -> pd.DataFrame:
        """self.clusters plus a "silhouette" column: how well every vertex sits in the cluster cluster() gave it
        (model.wv.silhouette of self.kmeans_result, by the metric it was clustered with; NaN for a vertex of no
        cluster).  The mean over the clustered vertices is kept as self.silhouette_score.  cluster() first."""
        wv = self._wv()
        if self.kmeans_result is None:
            raise ValueError("Clusters are not available. Please run cluster()")
        res = wv.silhouette(self.kmeans_result, metric=self._cluster_metric, restrict_vocab=len(self.clusters))
        member = self.kmeans_result.labels >= 0
        self.silhouette_score = float(res.s[member.to(res.s.device)].mean())
        return self.clusters.assign(silhouette=res.s.cpu().numpy())

    def classify(self, df_labels: pd.DataFrame, train_fraction: float = 0.5, seed: int = 0, **kw) -> pd.DataFrame:
        """The node2vec paper's multi-label classification (section 4.3): one-vs-rest logistic regression on
        train_fraction of the vocabulary vertices (node2vec_amd.classify.evaluate, whose other arguments pass
        through), df_labels holding one ["id", "label"] row per (vertex, label).  Returns one row per (vertex,
        class), in vocabulary order: ["id" | "name", "label", "score", "predicted", "train"].  Names go through
        name_id as in cluster().  The LogRegResult is kept as self.classifier, the F1 of the held-out vertices as
        self.label_f1."""
        wv = self._wv()
        from node2vec_amd import classify

        ids = self._vocab_ids(wv)
        column, who = self._who(ids)
        Y, classes = classify.labels_from_frame(df_labels, ids)
        top = kw.pop("top", True)
        X = wv._device_vectors()
        self.classifier, self.label_f1 = classify.evaluate(X, Y, train_fraction, seed, top=top, **kw)
        scores = wv.label_scores(self.classifier)
        truth = Y.to(scores.device)
        pred = classify.predict_top(scores, truth.sum(1)) if top else classify.predict(scores)
        train = np.zeros(len(ids), dtype=bool)
        train[classify.split_rows(len(ids), train_fraction, seed)[0]] = True
        c = len(classes)
        return pd.DataFrame({column: np.repeat(who, c), "label": np.tile(classes, len(ids)),
                             "score": scores[:, :c].cpu().numpy().reshape(-1),
                             "predicted": pred[:, :c].cpu().numpy().reshape(-1), "train": np.repeat(train, c)})

    def project(self, n_components: int = 2, metric: str = "cosine", **kw) -> pd.DataFrame:
        """["id" | "name", "x0", "x1", ..]: every vocabulary vertex on the leading principal components of the
        vectors, in vocabulary order (model.wv.pca and model.wv.project, whose other arguments pass through; NaN:
        a vertex whose vector holds a non-finite value).  The default metric is cosine, as in cluster().  Names go
        through name_id as in cluster().  The PCAResult is kept as self.pca_result."""
        wv = self._wv()
        column, who = self._who(self._vocab_ids(wv))
        self.pca_result = wv.pca(n_components, metric=metric, **kw)
        coords = wv.project(self.pca_result).cpu().numpy()
        return pd.DataFrame({column: who, **{f"x{j}": coords[:, j] for j in range(coords.shape[1])}})

    def tsne(self, **kw) -> pd.DataFrame:
        """["id" | "name", "x0", "x1"]: every vocabulary vertex on the t-SNE map of the vectors, in vocabulary order
        (model.wv.tsne, whose arguments pass through).  Names go through name_id as in project().  The TSNEResult
        is kept as self.tsne_result."""
        wv = self._wv()
        column, who = self._who(self._vocab_ids(wv))  # the whole vocabulary, whatever restrict_vocab leaves
        self.tsne_result = wv.tsne(**kw)
        coords = self.tsne_result.embedding.cpu().numpy()
        return pd.DataFrame({column: who[:coords.shape[0]], "x0": coords[:, 0], "x1": coords[:, 1]})

    def umap(self, **kw) -> pd.DataFrame:
        """["id" | "name", "x0", "x1"]: every vocabulary vertex on the UMAP layout of the vectors, in vocabulary order
        (model.wv.umap, whose arguments pass through).  Names go through name_id as in project().  The UMAPResult
        is kept as self.umap_result."""
        wv = self._wv()
        column, who = self._who(self._vocab_ids(wv))  # the whole vocabulary, whatever restrict_vocab leaves
        self.umap_result = wv.umap(**kw)
        coords = self.umap_result.embedding.cpu().numpy()
        return pd.DataFrame({column: who[:coords.shape[0]], "x0": coords[:, 0], "x1": coords[:, 1]})


class Node2VecHIP(Node2VecBase, _ModelQueries):
    """Drop-in for Node2VecGensim (embedding.py:70-178) on one MI355X."""

    def __init__(
        self,
        df_walks: pd.DataFrame,
        w2v_params: Dict[str, Any],
        name_id: Optional[pd.DataFrame] = None,
        window_size: Optional[int] = None,
        vector_size: Optional[int] = None,
        random_seed: Optional[int] = None,
    ) -> None:
        super().__init__()
        self.walks = df_walks
        self.name_id = name_id
        self.model: Optional[HipW2V] = None

        for param in GENSIM_PARAMS:  # embedding.py:105-107: fills the caller's dict
            if param not in w2v_params:
                w2v_params[param] = GENSIM_PARAMS[param]
        w2v_params["seed"] = random_seed if random_seed else int(time.time()) // 60  # :108
        if window_size is not None:
            if window_size < 5 or window_size > 30:  # :110-111
                raise ValueError(f"Inappropriate context window size {window_size}!")
            w2v_params["window"] = window_size
        if vector_size is not None:
            if vector_size < 32 or vector_size > 1024:  # :114-115
                raise ValueError(f"Inappropriate vector dimension {vector_size}!")
            w2v_params["size"] = vector_size
        _check_objective(w2v_params)
        logging.info(f"__init__(): w2v params: {w2v_params}")
        self.w2v_params = w2v_params

    # -- training ---------------------------------------------------------------
    def _walk_tensor(self, device, walks=None) -> torch.Tensor:
        walks = self.walks if walks is None else walks
        if isinstance(walks, torch.Tensor):
            return walks.to(device=device, dtype=torch.int32)
        from node2vec_amd import corpus

        dev_walks = corpus.lookup(walks)  # the frame random_walk() returned, unchanged
        if dev_walks is not None:
            return dev_walks.to(device=device, dtype=torch.int32)
        arr = corpus.arrow_rows(walks["walk"])  # an Arrow-backed column: no Python object per vertex
        if arr is not None:
            return torch.from_numpy(np.array(arr, dtype=np.int32)).to(device)  # (a copy: the Arrow buffer is read-only)
        # embedding.py:125 requires equal-length walks (np.array(walks.tolist()))
        arr = np.array(walks["walk"].tolist())
        if arr.ndim != 2:
            raise ValueError("walks must all have the same length")
        return torch.from_numpy(arr.astype(np.int32)).to(device)

    def fit(self, device=None, sync=None, sentence_base: int = 0) -> HipW2V:
        """Trains and returns the model (embedding.py:120-127).

        Under an initialised torch.distributed process group (one process per GPU) the
        walks held by this object are this rank's shard: the vocabulary is built from
        globally summed counts, every rank starts from the same seeded model, trains on its
        own walks with disjoint sentence ids, and the replicas are averaged (RCCL) every
        `sync_every` launches (sgns.DeltaSync; w2v_params["sync_every"], default: chosen so that
        the exchange takes <= 10 % of the time; w2v_params["sync_wire"] "fp32" | "bf16"), with a
        final blocking exchange, so all ranks return the same vectors.  Ranks may hold
        different numbers of walks (or none): the block grid is laid over the largest shard."""
        import torch.distributed as dist

        from node2vec_amd import _lib

        dev = device or _lib.require_gpu()
        p = dict(HIP_SGNS_PARAMS)
        p.update(self.w2v_params)
        negative = int(p["negative"]) if p["negative"] else int(HIP_SGNS_PARAMS["negative"])
        walks = self._walk_tensor(dev)
        vocab = sgns.build_vocab(walks, int(p["min_count"]))
        if len(vocab) == 0:
            raise RuntimeError("you must first build vocabulary before training the model")
        m = sgns.SgnsModel(vocab, int(p["size"]), int(p["window"]), negative, int(p["seed"]),
                           sample=float(p["sample"] or 0.0), ns_exponent=float(p["ns_exponent"]),
                           device=dev, sg=int(bool(p["sg"])), cbow_mean=int(p["cbow_mean"]))
        # opt-in, not gensim's sampling: w2v_params["batched"] = True shares the k negatives of a
        # centre position among its pairs (csrc/n2v_sgns_batched.hip; dim 64 / 128 / 256,
        # window <= 7, negative <= 15)
        m.batched = bool(p.get("batched", False))
        m.hub_rows = None if p.get("hub_rows") is None else int(p["hub_rows"])  # hogwild: atomic adds on the top rows
        # tokens < 0 (rows of dropped walkers in an on-device corpus, fugue.random_walk_tensors)
        # stay outside the vocabulary; a negative index must not wrap around
        idx = torch.where(walks >= 0, vocab.index_of[walks.clamp(min=0).long()],
                          torch.full_like(walks, -1))
        idx = sgns.split_rows(idx)
        rows_max = None
        if sync is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from node2vec_amd.shard import all_reduce, sentence_base as rank_base

            rows = torch.tensor([idx.shape[0]], device=dev)
            all_reduce(rows, dist.ReduceOp.MAX)
            rows_max = int(rows.item())  # every rank lays the same block grid over this
            sentence_base = rank_base(dist.get_rank(), dist.get_world_size(),
                                      rows_max * max(int(p["iter"]), 1))
            sync = sgns.DeltaSync(m, sync_every=p.get("sync_every"), wire=p.get("sync_wire", "fp32"))
        # the rate falls per job of batch_words words as in gensim (constants.py:58; a corpus whose
        # walks had to be split into sentences keeps one rate per launch)
        split = idx.shape[0] != walks.shape[0]
        m.train(idx, int(p["iter"]), float(p["alpha"]), float(p["min_alpha"]),
                sentence_base=sentence_base, sync=sync, rows_global_max=rows_max,
                deterministic=bool(p.get("deterministic", False)),
                batch_words=None if split else int(p.get("batch_words") or 0) or None)
        torch.cuda.synchronize(dev)
        p["negative"], p["sg"], p["cbow_mean"] = negative, m.sg, m.cbow_mean
        # what the trainer really ran with (hub_rows None = chosen from the corpus: recorded, so that a
        # parity run can pin it -- hub_rows = 0 is gensim's code as written)
        p["hub_rows"], p["hub_rows_auto"], p["hub_waves"] = m.hub_rows, m.hub_rows_auto, m.hub_waves
        # the matrices stay in HBM and the tokens stay integer ids (lazy strings): at cfg 4 the
        # host copies would be 2 x 51 GB + 10^8 Python strings that most callers never read
        self.model = HipW2V(KeyedVectors(vocab.ids, m.syn0), m.syn1neg, p, int(m.pairs.item()))
        return self.model

    # -- fold-in: vertices the model has never seen ---------------------------------
    def infer_vertices(self, df_walks_or_tensor, epochs: Optional[int] = None, init=None) -> pd.DataFrame:
        """Embeds the vertices of `df_walks_or_tensor` (walks over the grown graph, as fit() takes them) that are
        not in model.wv, against the fitted model, which stays exactly as it is (node2vec_amd/foldin.py, DESIGN.md
        "Fold-in").  The new vertices are numbered in ascending id.  Returns a DataFrame ["id" | "name", "vector"]
        shaped like embedding(); model.wv.with_rows(ids, vectors) gives a KeyedVectors over old and new.

        The negative table is rebuilt from the walks this object was fitted on (the fitted model keeps no counts):
        RuntimeError if they no longer give the model's vocabulary.  epochs: default w2v_params["iter"]; init:
        the starting rows [n_new, dim], default seeded.  Skip-gram negative sampling only: ValueError for a model
        fitted with sg=0 or batched=True."""
        from types import SimpleNamespace

        from node2vec_amd import _lib, foldin

        wv = self._wv()
        p = self.model.params
        if not p.get("sg", 1) or p.get("batched", False):
            raise ValueError("infer_vertices is defined for skip-gram negative sampling only (sg=1, not batched)")
        dev = _lib.require_gpu()
        vocab = sgns.build_vocab(self._walk_tensor(dev), int(p["min_count"]))
        if wv.ids is None or not np.array_equal(vocab.ids.cpu().numpy(), wv.ids):
            raise RuntimeError("the walks of this object do not give the vocabulary of its model: infer_vertices "
                               "rebuilds the negative-sampling table from the walks the model was fitted on")
        n_vocab = len(vocab)
        walks = self._walk_tensor(dev, df_walks_or_tensor).long()
        seen = torch.unique(walks[walks >= 0])  # ascending
        inside = seen < vocab.index_of.numel()
        known = torch.zeros_like(inside)
        known[inside] = vocab.index_of[seen[inside]] >= 0
        new_ids = seen[~known]
        n_new = int(new_ids.numel())
        if n_vocab + n_new > 2 ** 31:
            raise ValueError("vocabulary and new vertices together exceed the int32 tokens of the kernels")
        # token -> vocabulary index, n_vocab + new index, or -1
        index = torch.cat([vocab.index_of[seen[known]].long(), n_vocab + torch.arange(n_new, device=dev)])
        keys, order = torch.sort(torch.cat([seen[known], new_ids]))
        index = index[order]
        at = torch.searchsorted(keys, walks.clamp(min=0)).clamp(max=max(keys.numel() - 1, 0))
        idx = torch.where(walks >= 0, index[at], torch.full_like(walks, -1)).to(torch.int32)
        idx = sgns.split_rows(idx)
        syn1neg = self.model._syn1neg
        syn1neg = syn1neg if isinstance(syn1neg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(syn1neg))
        sample_int = sgns.make_sample_int(vocab.counts, float(p["sample"] or 0.0))
        frozen = SimpleNamespace(syn0=wv._device_vectors(), syn1neg=syn1neg.to(device=dev, dtype=torch.float32),
                                 cum_table=sgns.make_cum_table(vocab.counts, float(p["ns_exponent"])).to(dev),
                                 cum_index=None, sample_int=None if sample_int is None else sample_int.to(dev),
                                 exp_table=torch.from_numpy(sgns.exp_table()).to(dev), window=int(p["window"]),
                                 negative=int(p["negative"]), seed=int(p["seed"]))
        rows, _ = foldin.fold_in(frozen, idx, n_new, int(p["iter"]) if epochs is None else int(epochs),
                                 float(p["alpha"]), float(p["min_alpha"]), init=init)
        column, who = self._who(new_ids.cpu().numpy())
        return pd.DataFrame({column: who, "vector": corpus.list_column(rows.cpu().numpy(), "list")})

    # -- results ------------------------------------------------------------------
    def iter_embedding(self, chunk_rows: int = 1 << 18, vector_column: str = "auto"):
        """embedding() in chunks of `chunk_rows` rows: DataFrames ["id" | "name", "vector"] of the
        reference's shape, made without ever holding the whole model as Python objects.  `vector_column`:
        "list" = Python lists of floats, "rows" = one read-only ndarray view per row, "arrow" = an Arrow-backed
        list<float> column, "auto" = lists up to corpus.LIST_COLUMN_MAX_VALUES values per chunk, rows beyond
        (corpus.list_column)"""
        from node2vec_amd import corpus
        wv = self._wv()
        names = self._names()
        for lo in range(0, len(wv), chunk_rows):
            hi = min(len(wv), lo + chunk_rows)
            vectors = corpus.list_column(wv.rows(lo, hi), vector_column)
            column, who = self._who(self._vocab_ids(wv, lo, hi), names)  # a chunk's KeyError comes with the chunk
            yield pd.DataFrame({column: who, "vector": vectors})

    def embedding(self) -> pd.DataFrame:
        """embedding.py:129-143.  One DataFrame of Python lists, as the reference returns: fine
        up to a few million vertices; beyond 2^31 vector elements use iter_embedding()."""
        wv = self._wv()
        if len(wv) * max(wv.vector_size, 1) >= 2 ** 31:
            raise MemoryError(f"embedding(): {len(wv)} x {wv.vector_size} values as Python lists do "
                              "not fit a DataFrame; use iter_embedding(chunk_rows) or model.wv.rows()")
        big = len(wv) * max(wv.vector_size, 1) > corpus.LIST_COLUMN_MAX_VALUES
        parts = list(self.iter_embedding(len(wv) if big else 1 << 18, str(self.w2v_params.get("vector_column", "auto"))))
        if not parts:
            return pd.DataFrame({("name" if self.name_id is not None else "id"): [], "vector": []})
        return parts[0] if len(parts) == 1 else pd.concat(parts, ignore_index=True)

    def get_vector(self, vertex_id: Union[str, int]) -> List[float]:
        """embedding.py:145-151"""
        if isinstance(vertex_id, int):
            vertex_id = str(vertex_id)
        return list(self.model.wv[vertex_id])  # type: ignore

    def most_similar(self, vertex_id: Union[str, int], topn: int = 10, indexer=None) -> pd.DataFrame:
        """The topn vertices nearest to vertex_id by cosine of their vectors (model.wv.most_similar):
        a DataFrame ["id" | "name", "similarity"], names mapped through name_id as in embedding().
        indexer: an index from model.wv.build_index() for an approximate search."""
        hits = self._wv().most_similar(str(vertex_id), topn=topn, indexer=indexer)
        column, who = self._who(np.array([int(t) for t, _ in hits], dtype=np.int64))
        return pd.DataFrame({column: who, "similarity": np.array([s for _, s in hits], dtype=np.float64)})

    def save_model(self, file_path: str, file_name: str) -> None:
        """embedding.py:153-157: "<path>/<name>.model" """
        self.model.save(os.path.join(file_path, file_name + ".model"))  # type: ignore

    def load_model(self, file_path: str, file_name: str) -> HipW2V:
        """embedding.py:159-164"""
        self.model = HipW2V.load(os.path.join(file_path, file_name + ".model"))
        return self.model

    def save_vectors(self, file_path: str, file_name: str) -> None:
        """embedding.py:166-170: word2vec text format"""
        self.model.wv.save_word2vec_format(os.path.join(file_path, file_name))  # type: ignore

    @staticmethod
    def load_vectors(file_path: str, file_name: str) -> KeyedVectors:
        """embedding.py:172-178"""
        return KeyedVectors.load_word2vec_format(os.path.join(file_path, file_name))


class HsW2VModel:
    """The fitted model of Node2VecSpark (stands where Spark's Word2VecModel stands): .wv over syn0
    (so most_similar works), the inner-node matrix syn1, the parameters and what the trainer did."""

    FILE = "model.pt"

    def __init__(self, wv: KeyedVectors, syn1, params: Dict[str, Any], pairs: int, stats: Dict[str, Any]):
        self.wv, self._syn1, self.params, self.pairs_trained = wv, syn1, dict(params), pairs
        self.stats = dict(stats)

    @property
    def syn1(self) -> np.ndarray:
        if isinstance(self._syn1, torch.Tensor):
            self._syn1 = self._syn1.cpu().numpy()
        return self._syn1

    def getVectors(self) -> pd.DataFrame:
        """Spark's Word2VecModel.getVectors: ["word", "vector"], one row per vocabulary word (words are
        the int64 vertex ids, where Spark has the strings of its array<string> cast)"""
        from node2vec_amd import corpus

        wv = self.wv
        return pd.DataFrame({"word": _ModelQueries._vocab_ids(wv),
                             "vector": corpus.list_column(wv.rows(0, len(wv)), "list")})

    def save(self, path: str) -> None:
        """a directory (Spark writes one), overwritten"""
        os.makedirs(path, exist_ok=True)
        tokens = self.wv.ids if self.wv.ids is not None else self.wv.index2word
        torch.save({"tokens": tokens, "vectors": self.wv.vectors, "syn1": self.syn1, "params": self.params,
                    "pairs": self.pairs_trained, "stats": self.stats}, os.path.join(path, self.FILE))

    @classmethod
    def load(cls, path: str) -> "HsW2VModel":
        d = torch.load(os.path.join(path, cls.FILE), weights_only=False)
        return cls(KeyedVectors(d["tokens"], d["vectors"]), d["syn1"], d["params"], d["pairs"], d["stats"])


# the keyword arguments Spark's Word2Vec takes besides inputCol / outputCol (the reference sets those),
# and the options of the HIP trainer
_SPARK_KEYS = frozenset(WORD2VEC_PARAMS)
HIP_HS_PARAMS: Dict[str, Any] = {
    "deterministic": False,  # True: one wave, sentences in order -- reproducible bit for bit (for tests)
}


class Node2VecSpark(Node2VecBase, _ModelQueries):
    """Drop-in for the reference's Node2VecSpark (embedding.py:182-285) on one MI355X: skip-gram with
    hierarchical softmax, what Spark ML's Word2Vec trains (node2vec_amd/hs.py, csrc/n2v_hs.hip).

    Deviations: words are int64 vertex ids where Spark casts the walks to array<string>; numPartitions
    is validated but not replayed (Spark trains that many replicas per iteration and averages them:
    this trainer keeps one model); Spark's vocabSize * vectorSize < 2^31 cap is not replayed; sentences
    longer than 256 tokens are cut at 256 (the kernel's row buffer)."""

    def __init__(
        self,
        df_walks,
        w2v_params: Dict[str, Any],
        name_id: Optional[pd.DataFrame] = None,
        window_size: Optional[int] = None,
        vector_size: Optional[int] = None,
        random_seed: Optional[int] = None,
    ) -> None:
        super().__init__()
        self.walks = df_walks
        self.name_id = name_id
        self.model: Optional[HsW2VModel] = None

        for param in WORD2VEC_PARAMS:  # embedding.py:234-236: fills the caller's dict
            if param not in w2v_params:
                w2v_params[param] = WORD2VEC_PARAMS[param]
        w2v_params["seed"] = random_seed if random_seed else int(time.time())  # :237
        if window_size is not None:
            if window_size < 5 or window_size > 30:  # :238-241
                raise ValueError(f"Inappropriate context window size {window_size}!")
            w2v_params["windowSize"] = window_size
        if vector_size is not None:
            if vector_size < 32 or vector_size > 1024:  # :242-245
                raise ValueError(f"Inappropriate vector dimension {vector_size}!")
            w2v_params["vectorSize"] = vector_size
        unknown = sorted(k for k in w2v_params if k not in _SPARK_KEYS and k not in HIP_HS_PARAMS)
        if unknown:  # Spark's keyword-only constructor
            raise TypeError(f"Word2Vec got an unexpected keyword argument {unknown[0]!r}")
        for k in ("vectorSize", "windowSize", "stepSize", "numPartitions", "maxSentenceLength"):
            if not w2v_params[k] > 0:
                raise ValueError(f"{k} must be positive, got {w2v_params[k]!r}")
        for k in ("maxIter", "minCount"):
            if w2v_params[k] < 0:
                raise ValueError(f"{k} must be >= 0, got {w2v_params[k]!r}")
        if w2v_params["vectorSize"] > 1024 or w2v_params["windowSize"] > 32:
            raise ValueError("the HIP trainer supports vectorSize <= 1024 and windowSize <= 32")
        logging.info(f"__init__(): w2v params: {w2v_params}")
        self.w2v_params = w2v_params

    def fit(self, device=None) -> HsW2VModel:
        """Trains and returns the model (embedding.py:247-256).  One GPU: under a process group of more
        than one rank it raises NotImplementedError."""
        import torch.distributed as dist

        from node2vec_amd import _lib, hs

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("Node2VecSpark trains on one GPU: there is no multi-GPU hierarchical softmax")
        dev = device or _lib.require_gpu()
        p = dict(HIP_HS_PARAMS)
        p.update(self.w2v_params)
        walks = Node2VecHIP._walk_tensor(self, dev)
        vocab = sgns.build_vocab(walks, int(p["minCount"]))
        if len(vocab) == 0:
            raise RuntimeError("you must first build vocabulary before training the model")
        idx = torch.where(walks >= 0, vocab.index_of[walks.clamp(min=0).long()], torch.full_like(walks, -1))
        rows = hs.sentences(idx, int(p["maxSentenceLength"]))
        m = hs.HsModel(vocab, int(p["vectorSize"]), int(p["windowSize"]), int(p["seed"]), device=dev)
        m.train(rows, int(p["maxIter"]), float(p["stepSize"]), deterministic=bool(p.get("deterministic")))
        torch.cuda.synchronize(dev)
        stats = {"hogwild_waves": m.hogwild_waves_used,
                 "hot_nodes": hs.HOT_NODES,
                 "mean_code_length": m.mean_code_length, "sentences": int(rows.shape[0])}
        self.model = HsW2VModel(KeyedVectors(vocab.ids, m.syn0), m.syn1, p, int(m.pairs.item()), stats)
        logging.info("model fitting done!")
        return self.model

    def embedding(self) -> pd.DataFrame:
        """embedding.py:258-267: ["id", "vector"], or ["name", "vector"] through an inner join with
        name_id (ids that name_id does not list are dropped, as Spark's join drops them)"""
        self._wv()
        df = self.model.getVectors().rename(columns={"word": "id"})
        if self.name_id is not None:
            df = df.merge(self.name_id, on="id", how="inner")[["name", "vector"]]
        return df

    def get_vector(self, vertex_id: Union[str, int]) -> pd.DataFrame:
        """embedding.py:269-274: the ["word", "vector"] rows of word == vertex_id (0 or 1 row)"""
        wv = self._wv()
        row = wv.vocab.get(str(vertex_id))
        if row is None:
            return pd.DataFrame({"word": np.array([], np.int64), "vector": []})
        word = int(wv.ids[row]) if wv.ids is not None else int(wv.index2word[row])
        return pd.DataFrame({"word": np.array([word], np.int64), "vector": [wv.rows(row, row + 1)[0].tolist()]})

    def infer_vertices(self, df_walks_or_tensor, epochs: Optional[int] = None, init=None):
        """Not available: fold-in (Node2VecHIP.infer_vertices) is defined for skip-gram negative sampling; the
        pairs of hierarchical softmax are trained against tree nodes, another definition."""
        raise ValueError("infer_vertices is defined for skip-gram negative sampling only (Node2VecHIP, sg=1)")

    def save_model(self, cloud_path: str, model_name: str) -> None:
        """embedding.py:276-285: "<path>/<name>.sparkml", a directory"""
        if not model_name.endswith(".sparkml"):
            model_name += ".sparkml"
        self.model.save(os.path.join(cloud_path, model_name))  # type: ignore

    def load_model(self, cloud_path: str, model_name: str) -> HsW2VModel:
        if not model_name.endswith(".sparkml"):
            model_name += ".sparkml"
        self.model = HsW2VModel.load(os.path.join(cloud_path, model_name))
        return self.model


# import-compatible names
Node2VecGensim = Node2VecHIP
GensimW2V = HipW2V
