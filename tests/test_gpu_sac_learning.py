"""GPU: ff_isac learns env=spread (against two baselines the NumPy model plays on the CPU), and ff_isac / ff_masac through
run_experiment: every event, finite losses, log_alpha moving with autotune and staying without."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from tests import spread_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_isac_learns_spread(dev):
    """One fixed-seed ff_isac run on spread-3a with the default networks (tools/sac_learning.py's CURVE; the measured
    curve is profiles/sac_learning_curve.json: the midpoint is crossed after about 12 s, this run takes about 15 s): the
    final mean eval return (320 episodes) exceeds the midpoint between the uniform-random policy and the scripted policy
    "agent i walks to landmark i", both played by the NumPy model over 320 episodes."""
    p = m.Params(3)
    rand = m.mean_episode_return(p, lambda st, rng: m.uniform_actions(rng, st["agent_pos"].shape[0], p.A), 320, seed=7)
    walk = m.mean_episode_return(p, lambda st, rng: m.scripted_actions(st), 320, seed=7)
    assert walk > rand + 8.0, (rand, walk)
    spec = importlib.util.spec_from_file_location("sac_learning", os.path.join(ROOT, "tools", "sac_learning.py"))
    sl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sl)
    curve = sl.learning_curve(dev)
    rec = {"random": rand, "scripted": walk, "midpoint": 0.5 * (rand + walk), "eval_return_before": curve[0][2],
           "eval_return_after": curve[-1][2], "env_steps": curve[-1][0], "seconds": curve[-1][1]}
    print(json.dumps(rec))
    assert curve[-1][2] > 0.5 * (rand + walk), rec


@pytest.mark.parametrize("system,autotune", [("ff_isac", True), ("ff_masac", True), ("ff_masac", False)])
def test_run_experiment(dev, system, autotune):
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.sac.{system}")
    cfg = compose(f"default_{system}_spread", ["arch.num_envs=16", "system.num_updates=8", "arch.num_evaluation=2", "arch.num_eval_episodes=16",
                                        "arch.num_absolute_metric_eval_episodes=32", "system.explore_steps=400", "system.epochs=2",
                                        "system.buffer_size=1024", f"system.autotune={str(autotune).lower()}"])
    recs = []
    ret = mod.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    assert events[:2] == ["MISC", "ACT"] and events.count("TRAIN") == 2 and events.count("EVAL") == 2 and events[-1] == "ABSOLUTE"
    assert recs[0]["step"] == 400 and recs[1]["episode_length"] == 25  # 25 explore steps of 16 envs: one episode each
    evals = [r for r in recs if r["event"] == "EVAL"]
    lo, hi = -25 * (2 * math.sqrt(2) + 0.5), 0.0  # every landmark a diagonal away and every pair colliding, for 25 steps
    assert all(lo <= r["episode_return"] <= hi for r in evals) and ret == evals[-1]["episode_return"]
    assert [r["timestep"] for r in evals] == [400 + 128, 400 + 256]
    trains = [r for r in recs if r["event"] == "TRAIN"]
    for r in trains:
        for k in ("q1_loss", "q2_loss", "loss", "q1_a_vals", "q2_a_vals", "actor_loss", "alpha_loss", "log_alpha"):
            assert np.isfinite(r[k]), (k, r)
        assert r["q1_loss"] > 0 and r["actor_loss"] != 0
    if autotune:  # starts at 0 and moves
        assert trains[0]["log_alpha"] != 0.0 and trains[1]["log_alpha"] != trains[0]["log_alpha"] and trains[0]["alpha_loss"] != 0
    else:  # stays at log(init_alpha), no alpha loss
        assert all(abs(r["log_alpha"] - math.log(0.1)) < 1e-6 and r["alpha_loss"] == 0 for r in trains)
    assert lo <= recs[-1]["episode_return"] <= hi
