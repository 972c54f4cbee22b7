#!/usr/bin/env python3
"""rec_qmix / rec_vdn measurements on Level-Based Foraging next to rec_iql in the same run (bench.py's
headline is not involved).

    python tools/qmix_bench.py [--out profiles/qmix_bench.json]
    python tools/qmix_bench.py --curve [--out profiles/qmix_learning_curve.json]

Default mode: tools/iql_bench.py's two shapes - the reference defaults (16 envs, B = 32, L = 20) and the wide one (1024
envs, B = 256) - for rec_qmix, rec_vdn and rec_iql, each past the train gate: the median time of one update, env-steps/s and
the library calls per update; then the per-launch time of the two new kernels at each shape (HIP events around the learner's
own launches).  --curve: the learning runs of tests/test_gpu_qmix_learning.py (rec_iql's overrides, unchanged).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.iql_bench import CURVE_OVERRIDES, SCENARIO, SHAPES, LaunchCounter, gain  # noqa: E402

SYSTEMS = ("rec_qmix", "rec_vdn", "rec_iql")


def _setup(system, overrides, updates):
    from mava_amd import envs
    from mava_amd.config import compose

    if system == "rec_iql":
        from mava_amd.iql_learner import learner_setup
    else:
        from mava_amd.qmix_learner import learner_setup
    cfg = compose(f"default_{system}", [f"env/scenario={SCENARIO}", *overrides, f"system.num_updates_per_eval={updates}"])
    env, _ = envs.make(cfg)
    learn, _, state = learner_setup(env, (1, 2), cfg)
    L = learn.learner
    while not L.can_train():  # fill the buffer past the train gate (untimed)
        state = learn(state).learner_state
    state = learn(state).learner_state  # warm-up
    torch.cuda.synchronize()
    return learn, L, state


def bench_shape(system, name, overrides, updates, repeats):
    from mava_amd import _lib

    learn, L, state = _setup(system, overrides, updates)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        state = learn(state).learner_state
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / updates)
    cnt = LaunchCounter()
    state = learn(state).learner_state
    torch.cuda.synchronize()
    cnt.close()
    # per-launch time of the named launches (events around every launch() call: the update itself runs slower here)
    _lib.TIMERS = {}
    learn(state)
    torch.cuda.synchronize()
    timers, _lib.TIMERS = _lib.TIMERS, None
    per_launch = {k: round(1e3 * statistics.median(a.elapsed_time(b) for a, b in v), 2) for k, v in timers.items()
                  if k in ("qmix_td", "qmix_state", "q_td_loss")}
    med = statistics.median(times)
    res = {"system": system, "shape": name, "num_envs": L.E, "num_agents": L.A, "rollout_length": L.T, "epochs": L.K,
           "sample_batch_size": L.B, "sample_sequence_length": L.L, "matmul_mode": L.matmul_mode, "params": int(L.p.numel()),
           "median_update_ms": round(med * 1e3, 3), "update_ms_all": [round(x * 1e3, 3) for x in times],
           "env_steps_per_s": round(L.E * L.T / med, 1), "launches_per_update": cnt.n / updates,
           "median_launch_us": per_launch}
    if system != "rec_iql":
        res["mixer_rows"], res["mixer_state_dim"], res["td_blocks"] = L.mrows, L.Ds, L.td_blocks
    return res


def curve(out_path):
    import importlib

    from mava_amd.config import compose

    res = {"overrides": CURVE_OVERRIDES, "yardstick": "profiles/iql_learning_curve.json measured_gain (rec_iql)"}
    for system in ("rec_qmix", "rec_vdn"):
        mod = importlib.import_module(f"mava_amd.systems.q_learning.{system}")
        recs = []
        t0 = time.time()
        mod.run_experiment(compose(f"default_{system}", CURVE_OVERRIDES), log=recs.append)
        ev = [(r["timestep"], round(r["episode_return"], 4)) for r in recs if r["event"] == "EVAL"]
        res[system] = {"seconds": round(time.time() - t0, 1), "curve [timestep, mean eval return]": ev,
                       "measured_gain": round(gain([r for _, r in ev]), 4)}
        print(json.dumps({system: res[system]}), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.curve:
        curve(a.out or os.path.join(ROOT, "profiles", "qmix_learning_curve.json"))
        return
    res = {"device": torch.cuda.get_device_name(0), "scenario": SCENARIO, "results": []}
    for name, ov in SHAPES.items():
        for system in SYSTEMS:
            r = bench_shape(system, name, ov, a.updates, a.repeats)
            print(json.dumps(r), flush=True)
            res["results"].append(r)
    with open(a.out or os.path.join(ROOT, "profiles", "qmix_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
