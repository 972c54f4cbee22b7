"""GPU: rec_qmix and rec_vdn learn Level-Based Foraging.  The run is rec_iql's learning run (the overrides of
profiles/iql_learning_curve.json, unchanged) and the yardstick is rec_iql's committed measurement in that file, not the
new systems' own curves (those are recorded in profiles/qmix_learning_curve.json by tools/qmix_bench.py --curve)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
def test_value_decomposition_learns_lbf(dev, mixer):
    import importlib

    from mava_amd.config import compose

    system = importlib.import_module(f"mava_amd.systems.q_learning.rec_{mixer}")
    with open(os.path.join(ROOT, "profiles", "iql_learning_curve.json")) as f:
        curve = json.load(f)
    measured = curve["measured_gain"]  # rec_iql's gain on this run: 0.1798
    assert measured > 0.1
    recs = []
    system.run_experiment(compose(f"default_rec_{mixer}", curve["overrides"]), log=recs.append)
    ev = [r["episode_return"] for r in recs if r["event"] == "EVAL"]
    got = sum(ev[-3:]) / 3.0 - ev[0]  # tools/iql_bench.py gain()
    print(f"rec_{mixer}: gain {got:.4f}, curve {[round(v, 4) for v in ev]}")
    assert got > 0.4 * measured, (ev, measured)  # the margin of tests/test_gpu_iql.py::test_rec_iql_learns_lbf
