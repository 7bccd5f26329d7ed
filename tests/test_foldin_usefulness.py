"""Fold-in is useful: on a planted-partition graph the held-out vertices land in their own community about as often
after fold-in as after a full retrain (scripts/foldin_usefulness.py, CPU only: the restatement and the oracle's
deterministic SGNS -- the GPU kernels equal the restatement bit for bit, test_foldin_gpu.py).

MEASURED here, seeds 1 .. 5 (DESIGN.md "Fold-in"): fold-in 1.000 / 1.000 / 1.000 / 0.950 / 1.000, full retrain
0.975 / 0.900 / 0.975 / 0.850 / 0.950 -- a spread of 0.125 over the seeds.  The test runs seed 1 and asserts only
that fold-in is no worse than the retrain minus that spread."""
import os
import sys

from conftest import ROOT
from test_foldin_host import foldin_cpu  # noqa: F401  (the session fixture that builds the restatement)

SPREAD_OVER_FIVE_SEEDS = 0.125


def test_fold_in_is_no_worse_than_a_retrain_minus_the_spread(oracle, foldin_cpu):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import foldin_usefulness as fu

    fold, retrain = fu.measure(1, oracle, foldin_cpu)
    print("fold-in usefulness, seed 1: fold-in %.3f, full retrain %.3f" % (fold, retrain))
    assert retrain > 0.5  # the statistic discriminates: chance is 0.25
    assert fold >= retrain - SPREAD_OVER_FIVE_SEEDS, (fold, retrain)
