"""GPU: ff_mat learns.  One run of tools/mat_bench.py's CURVE - ff_mat and ff_mappo (network=mlp) on env=lbf
2s-8x8-2p-2f-coop for the same number of env-steps and the same seed; the measured curves are profiles/mat_learning_curve.json.
The bar is set by ff_mappo in the same run, not by ff_mat's own curve."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ff_mat_learns_lbf_against_ff_mappo(dev):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mat_bench as mb

    run = mb.learning_run(dev, log=print)
    mappo, mat = run["ff_mappo"], run["ff_mat"]
    print("ff_mappo gain", mappo["gain"], "final sem", mappo["final_sem"], "| ff_mat gain", mat["gain"], "bar", run["bar"])
    # the budget shows something only if ff_mappo's own gain stands clear of the noise of its final evaluation
    assert mappo["gain"] > 5.0 * mappo["final_sem"], (mappo["gain"], mappo["final_sem"])
    assert mat["gain"] >= run["bar"], f"ff_mat gained {mat['gain']:.4f}, the bar is {run['bar']:.4f} ({mb.BAR_FACTOR} x ff_mappo's {mappo['gain']:.4f})"
