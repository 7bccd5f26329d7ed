"""The sample behind the hogwild tolerances of tests/test_cbow_gpu.py.

    python scripts/cbow_stat_runs.py [--runs 30] [--out profiles/cbow_stat_runs.log]

The planted-partition case of tests/test_sgns_gpu.planted_case (50 communities x 40 vertices, dim 64,
window 5, negative 5, 3 epochs) trained with sg=0: the community-separation AUC of one deterministic
run (one wave: bit for bit the CPU restatement) and of --runs hogwild runs on one GPU, then their
mean, standard deviation and mean -+ 5 sd.  The test's bounds are set looser than that."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from node2vec_amd import sgns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from test_sgns_gpu import planted_case

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    case = planted_case()
    model, waves = sgns.SgnsModel, []

    def cbow_model(*args, **kw):
        m = model(*args, sg=0, **kw)
        waves.append(m.hogwild_waves(20000, 41))
        return m

    sgns.SgnsModel = cbow_model  # planted_case builds its models through the module
    t0 = time.perf_counter()
    det = case["auc"](case["train"](True))
    say("planted partition, CBOW (sg=0, cbow_mean=1), dim 64, window 5, negative 5, 3 epochs")
    say("deterministic: community AUC %.6f (%.1f s)" % (det, time.perf_counter() - t0))
    aucs = []
    for r in range(a.runs):
        aucs.append(case["auc"](case["train"](False)))
        say("hogwild run %2d: community AUC %.6f  |hogwild - deterministic| %.6f" % (r, aucs[-1], abs(aucs[-1] - det)))
    x, d = np.array(aucs), np.abs(np.array(aucs) - det)
    say("waves in flight (hogwild): %d" % waves[-1])
    say("hogwild AUC: mean %.6f sd %.6f min %.6f max %.6f; mean - 5 sd %.6f" %
        (x.mean(), x.std(ddof=1), x.min(), x.max(), x.mean() - 5 * x.std(ddof=1)))
    say("|hogwild - deterministic|: mean %.6f sd %.6f max %.6f; mean + 5 sd %.6f" %
        (d.mean(), d.std(ddof=1), d.max(), d.mean() + 5 * d.std(ddof=1)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
