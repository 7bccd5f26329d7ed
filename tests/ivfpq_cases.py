"""Shared by tests/test_ivfpq_host.py and tests/test_ivfpq_gpu.py: what csrc/n2v_ivfpq.hip must compute, restated in
numpy, and the case tables.

The restatement is the fixed order of the kernel word for word (DESIGN.md "Product-quantised codes").  numpy's
float32 `*` and `+` are one IEEE rounding each and never fused, which is what __fmul_rn / __fadd_rn are:
  q_hat         = q * inv, inv = 1 / sqrtf(sum q^2) in n2v_knn.hip's order (oracle.knn_inv_norms), 0 for a sum that
                  is not > 0
  lut[q][j][c]  = (..((+0 + q_hat[j dsub] * w_j[c][0]) + q_hat[j dsub + 1] * w_j[c][1]) + ..), over j dsub + t < dim
  score         = (..((coarse + lut[q][0][code_0]) + lut[q][1][code_1]) + ..)
  result        = NaN dropped, (score descending, original row ascending), the tail (-1, -inf)
Nothing in it knows about tiles, chunks or groups."""
import numpy as np

import ivf_cases as ic

CODEWORDS = 256
# max_list_rows the hand-made indexes are searched with: three chunks of 3584 positions by the plan's rule
# (asserted where used); the matrix the row numbers belong to has HAND_N rows
HAND_MAX_LIST_ROWS = 10752
HAND_CHUNK = 3584
HAND_N = 11000

# dim, m, k, the long list's length in terms of the plan's chunk c, n_queries.  m = 1, 4, 7: 16 pairs a tile
# (4- and 8-byte code rows); 8, 16: 8 pairs (8- and 16-byte rows); 32: 4 pairs; 64: 2 pairs.  dim 129 with m 16 has
# a ragged last sub-space and one that lies wholly past dim; 17 with 7 and 20 with 4 are ragged too
HAND_CASES = [
    (64, 1, 1, "c-1", 200), (64, 8, 10, "c", 200), (64, 16, 127, "c+1", 100), (64, 64, 128, "2c+1", 200),
    (129, 16, 10, "2c+1", 100), (17, 7, 128, "c", 200), (20, 4, 10, "c+1", 100), (64, 32, 10, "c-1", 100),
]

LUT_CASES = [(3, 2), (16, 16), (64, 8), (129, 16), (128, 64), (1024, 1)]


def dsub_of(dim, m):
    return -(-dim // m)


def code_stride(m):
    return next(s for s in (4, 8, 16, 32, 64) if m <= s)


def qhat(oracle, Q):
    """the normalised queries n2v_knn.hip's query kernel builds, fp32 [nq, dim]"""
    Q = np.ascontiguousarray(Q, np.float32)
    inv = oracle.knn_inv_norms(Q)
    with np.errstate(invalid="ignore", over="ignore"):
        return (Q * inv[:, None]).astype(np.float32)


def lut_expect(qh, codebooks, dim):
    """fp32 [nq, m, 256] from q_hat [nq, dim] and codebooks [m, 256, dsub]"""
    qh = np.ascontiguousarray(qh, np.float32)
    cb = np.ascontiguousarray(codebooks, np.float32)
    m, _, dsub = cb.shape
    out = np.zeros((qh.shape[0], m, CODEWORDS), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            acc = np.zeros((qh.shape[0], CODEWORDS), np.float32)
            for t in range(dsub):
                d = j * dsub + t
                if d >= dim:
                    break
                acc = acc + qh[:, d:d + 1] * cb[j, :, t][None, :]
            out[:, j, :] = acc
    return out


def lut_float64(qh, codebooks, dim):
    """(the same sums in float64, the sums of the terms' absolute values)"""
    m, _, dsub = codebooks.shape
    q = np.zeros((qh.shape[0], m * dsub))
    q[:, :dim] = qh
    q = q.reshape(qh.shape[0], m, dsub)
    cb = np.array(codebooks, np.float64)
    live = (np.arange(m * dsub) < dim).reshape(m, dsub)
    cb = cb * live[:, None, :]
    return np.einsum("qjt,jct->qjc", q, cb), np.einsum("qjt,jct->qjc", np.abs(q), np.abs(cb))


def scores_expect(lut, codes, positions, coarse):
    """fp32 [nq', len(positions)]: the scores of queries lut [nq', m, 256] with first terms coarse [nq'] against
    the code rows at `positions`"""
    m = lut.shape[1]
    s = np.repeat(np.asarray(coarse, np.float32)[:, None], len(positions), axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            s = s + lut[:, j, :][:, codes[positions, j]]
    return s


def scan_expect(lut, codes, list_off, row_ids, probes, coarse, k):
    """(rows int64 [nq, k], scores fp32 [nq, k]) of n2v_ivfpq_topk; probes [nq, nprobe] list numbers, -1 unused"""
    probes = np.asarray(probes, np.int64)
    nq = probes.shape[0]
    cand_r = [[] for _ in range(nq)]
    cand_s = [[] for _ in range(nq)]
    for l in np.unique(probes[probes >= 0]):
        positions = np.arange(list_off[l], list_off[l + 1])
        qs, os_ = np.nonzero(probes == l)
        if len(positions) == 0:
            continue
        s = scores_expect(lut[qs], codes, positions, coarse[qs, os_])
        for i, q in enumerate(qs):
            cand_r[q].append(row_ids[positions].astype(np.int64))
            cand_s[q].append(s[i])
    out_r = np.full((nq, k), -1, np.int64)
    out_s = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        if not cand_r[q]:
            continue
        r, s = np.concatenate(cand_r[q]), np.concatenate(cand_s[q])
        r, s = r[~np.isnan(s)], s[~np.isnan(s)]
        order = np.lexsort((r, -s))[:k]  # score descending, then row ascending (-0.0 == 0.0, as in the kernel)
        out_r[q, :len(order)] = r[order]
        out_s[q, :len(order)] = s[order]
    return out_r, out_s


def hand_lists(rng, long_len):
    """(list_off int64 [NLIST + 1], row_ids int32): ivf_cases' list lengths, the rows a seeded permutation of
    HAND_N row numbers -- not ascending inside a list, so that "by original row" is not "by position" """
    lens = list(ic.SMALL_LISTS) + [long_len]
    list_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert list_off[-1] <= HAND_N
    return list_off, rng.permutation(HAND_N)[:list_off[-1]].astype(np.int32)


def hand_codes(rng, n_positions, m, repeats=True):
    """uint8 [n_positions, stride]: random codes, the bytes past m random too (they must not be looked at); with
    `repeats` a tenth of the rows are copies of the first three rows' codes (ties between rows)"""
    codes = rng.integers(0, 256, (n_positions, code_stride(m)), dtype=np.uint8)
    if repeats and n_positions >= 30:
        for i, p in enumerate(rng.choice(n_positions, n_positions // 10, replace=False)):
            codes[p, :m] = codes[i % 3, :m]
    return codes


def exact_problem(rng, dim, m, nq, nprobe):
    """codebooks (multiples of 1/8 in [-2, 2]), unit queries of s in {1, 4, 16, 64} entries of +-1 / sqrt(s) (their
    sum of squares is 1 and q_hat = q exactly) and coarse scores (multiples of 1/8): every table entry and score is
    exact in fp32 in any order of summation"""
    dsub = dsub_of(dim, m)
    cb = (rng.integers(-16, 17, (m, CODEWORDS, dsub)) / 8.0).astype(np.float32)
    Q = np.zeros((nq, dim), np.float32)
    for q in range(nq):
        s = int(rng.choice([c for c in (1, 4, 16, 64) if c <= dim]))
        at = rng.choice(dim, s, replace=False)
        Q[q, at] = rng.choice([-1.0, 1.0], s) / np.sqrt(np.float32(s))
    coarse = (rng.integers(-8, 9, (nq, nprobe)) / 8.0).astype(np.float32)
    return cb, Q, coarse


def gaussian_problem(rng, dim, m, nq, nprobe):
    dsub = dsub_of(dim, m)
    cb = rng.standard_normal((m, CODEWORDS, dsub)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    coarse = rng.standard_normal((nq, nprobe)).astype(np.float32)
    return cb, Q, coarse


def mixture_rows(rng, n, dim, centres=48, noise=0.1):
    """rows around `centres` Gaussian centres: with 8 coarse lists the residuals still gather around a few points
    per list, which 256 codewords per sub-space resolve"""
    C = rng.standard_normal((centres, dim)).astype(np.float32)
    return (C[rng.integers(0, centres, n)] + noise * rng.standard_normal((n, dim))).astype(np.float32)
