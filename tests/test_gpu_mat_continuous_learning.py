"""GPU: ff_mat with the continuous head learns.  One run of tools/mat_bench.py's CONT_CURVE - ff_mappo (network=continuous_mlp) and
ff_mat (network=continuous_transformer) on env=spread spread-2a for the same 655 360 env-steps and the same seed; the measured curves
are profiles/mat_continuous_learning_curve.json.  The bar is set by ff_mappo in the same run (BAR_FACTOR of its eval-return gain), not
by ff_mat's own curve.  Measured: ff_mappo gains 9.3, ff_mat 5.1 against a bar of 3.7.  spread-3a is not this test's scenario: there
ff_mat at its default hyper-parameters stays flat at this budget (DESIGN.md 3.25 says why; the profile records that run too)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ff_mat_learns_spread_against_ff_mappo(dev):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mat_bench as mb

    assert mb.CONT_CURVE["calls"] == mb.CURVE["calls"] and mb.CONT_CURVE["overrides"]["ff_mat"] == ["network=continuous_transformer"]
    run = mb.learning_run(dev, log=print, curve=mb.CONT_CURVE)
    mappo, mat = run["ff_mappo"], run["ff_mat"]
    print("ff_mappo gain", mappo["gain"], "final sem", mappo["final_sem"], "| ff_mat gain", mat["gain"], "bar", run["bar"])
    # the budget shows something only if ff_mappo's own gain stands clear of the noise of its final evaluation
    assert mappo["gain"] > 5.0 * mappo["final_sem"], (mappo["gain"], mappo["final_sem"])
    assert mat["gain"] >= run["bar"], f"ff_mat gained {mat['gain']:.4f}, the bar is {run['bar']:.4f} ({mb.BAR_FACTOR} x ff_mappo's {mappo['gain']:.4f})"
