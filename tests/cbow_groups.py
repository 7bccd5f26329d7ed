"""Which rows a position of the CBOW trainer touches, replayed in integers: the kept tokens, the reduced
windows and the per-position draws of node2vec_amd/csrc/n2v_cbow.hip (its header comment; the float64
restatement test_cbow_host.reference_cbow makes the same draws), and from them how often the kernel's
grouping of targets (kTG at a time) and of context rows (kCG at a time) meets the cases it has code for.

  sentence r of a launch:  hs = mix64(seed ^ mix64(base + r + 0xA0761D6478BD642F)),
                           draw(idx) = mix64(hs + (idx + 1) * 0xE7037ED1A0B428DB)
  raw position t is kept unless it is < 0 or >= n_vocab, or sample_int[tok] < draw(2t) >> 32;
  its reduced window is b = (draw(2t + 1) >> 32) % window;
  kept position i with centre c trains when count = hi - lo - 1 > 0, lo = max(0, i - window + b),
  hi = min(nf, i + window + 1 - b); its targets are e = 0: c, and e = 1 .. negative:
  bisect_left(cum_table, (draw(2 * walk_len + i * negative + e - 1) >> 16) % cum_table[-1]), none
  when that equals c.

No floats are involved, so the tests can assert from the replay alone that a case reaches the path it
is meant to reach before they compare anything on the GPU.

Not a test module: a helper of test_cbow_host.py and test_cbow_groups_gpu.py.
"""
from bisect import bisect_left

# targets in flight / context rows summed per group, by the kernel's VEC (tgt_group, ctx_group)
KTG = {1: 6, 2: 6, 4: 6, 8: 3, 16: 2}
KCG = {1: 8, 2: 8, 4: 4, 8: 2, 16: 1}

M64 = (1 << 64) - 1


def vec_of(dim):
    v = 1
    while 64 * v < dim:
        v *= 2
    return v


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def replay(walks, cum_table, sample_int, n_vocab, seed, bases, window, negative, ktg, kcg):
    """walks: [rows, len] integers; cum_table / sample_int: the uint32 VALUES (sample_int or None);
    bases: the sentence_base of every launch over `walks`.  Returns a dict of counts."""
    cum = [int(x) for x in cum_table]
    assert len(cum) == n_vocab and all(0 <= x < 1 << 32 for x in cum)
    si = None if sample_int is None else [int(x) for x in sample_int]
    assert si is None or all(0 <= x < 1 << 32 for x in si)
    domain = cum[-1]
    ln = len(walks[0])
    out = dict(positions=0, centre_draws=0, dup_in_group=0, dup_across_groups=0, padded_last_group=0,
               ctx_dup_in_group=0, ctx_dup_across_groups=0, windows_twice=0, max_count=0, max_kept=0,
               max_position=-1, odd_positions=0, even_positions=0)
    for base in bases:
        for r, row in enumerate(walks):
            hs = mix64(seed ^ mix64(base + r + 0xA0761D6478BD642F))

            def draw(idx):
                return mix64(hs + (idx + 1) * 0xE7037ED1A0B428DB)

            sent, red = [], []
            for t in range(ln):
                tok = int(row[t])
                if tok < 0 or tok >= n_vocab:
                    continue
                if si is not None and si[tok] < (draw(2 * t) >> 32):
                    continue
                sent.append(tok)
                red.append((draw(2 * t + 1) >> 32) % window)
            nf = len(sent)
            out["max_kept"] = max(out["max_kept"], nf)
            for i in range(nf):
                centre = sent[i]
                lo, hi = max(0, i - window + red[i]), min(nf, i + window + 1 - red[i])
                ctx = [sent[m] for m in range(lo, hi) if m != i]
                if not ctx:
                    continue
                out["positions"] += 1
                out["max_count"] = max(out["max_count"], len(ctx))
                out["max_position"] = max(out["max_position"], i)
                out["odd_positions" if i & 1 else "even_positions"] += 1
                # the targets, -1 where there is nothing to train: a draw equal to the centre, or the
                # padding of the last group
                tg = [centre]
                for d in range(negative):
                    x = (draw(2 * ln + i * negative + d) >> 16) % domain
                    t = bisect_left(cum, x)
                    if t == centre:
                        out["centre_draws"] += 1
                        t = -1
                    tg.append(t)
                if len(tg) % ktg:
                    out["padded_last_group"] += 1
                    tg += [-1] * (ktg - len(tg) % ktg)
                for g0 in range(0, len(tg), ktg):
                    earlier = set(tg[:g0]) - {-1}
                    for e in range(g0, g0 + ktg):
                        if tg[e] < 0:
                            continue
                        if tg[e] in tg[g0:e]:
                            out["dup_in_group"] += 1
                        if tg[e] in earlier:
                            out["dup_across_groups"] += 1
                # the context rows, in position order
                out["windows_twice"] += len(set(ctx)) < len(ctx)
                for g0 in range(0, len(ctx), kcg):
                    earlier = set(ctx[:g0])
                    for e in range(g0, min(g0 + kcg, len(ctx))):
                        if ctx[e] in ctx[g0:e]:
                            out["ctx_dup_in_group"] += 1
                        if ctx[e] in earlier:
                            out["ctx_dup_across_groups"] += 1
    return out
