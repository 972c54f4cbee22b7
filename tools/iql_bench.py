#!/usr/bin/env python3
"""rec_iql measurements on Level-Based Foraging (DESIGN.md "rec_iql"; bench.py's headline is not involved).

    python tools/iql_bench.py [--out profiles/iql_bench.json]
    python tools/iql_bench.py --curve [--out profiles/iql_learning_curve.json]

Default mode: two shapes - the reference defaults (16 envs, rollout 2, 2 epochs, B = 32, L = 20) and a wide one (1024
envs, B = 256) - each past the train gate: the median time of one update (one learn() call of `updates` updates,
synchronised, divided), env-steps/s and the HIP launches per update (every call into the library counted).
--curve: the learning run of tests/test_gpu_iql.py::test_rec_iql_learns_lbf (eval return after every evaluation
interval), the measurement its threshold is set from.
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

SCENARIO = "10x10-3p-3f"
SHAPES = {
    "reference_defaults": ["arch.num_envs=16"],
    "wide": ["arch.num_envs=1024", "system.sample_batch_size=256", "system.buffer_size=1000"],
}
# tests/test_gpu_iql.py::test_rec_iql_learns_lbf runs exactly these overrides
CURVE_OVERRIDES = [f"env/scenario={SCENARIO}", "arch.num_envs=64", "system.total_timesteps=500000", "arch.num_evaluation=20",
                   "system.eps_decay=100000", "arch.num_eval_episodes=128", "arch.absolute_metric=false", "system.seed=3"]


def gain(returns) -> float:
    """Learning gain of a curve: mean of the last three eval returns minus the first (taken after 25k env steps, while
    epsilon is still above 0.7)."""
    return sum(returns[-3:]) / 3.0 - returns[0]


class LaunchCounter:
    """Counts every call of a library entry point (wraps the ctypes functions of the loaded library)."""

    def __init__(self):
        from mava_amd import _lib

        self.lib, self.n, self.saved = _lib.lib(), 0, {}
        for name in _lib._SIGNATURES:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def wrap(*a, _fn=fn):
                self.n += 1
                return _fn(*a)

            setattr(self.lib, name, wrap)

    def close(self):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def bench_shape(name, overrides, updates, repeats):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup

    cfg = compose("default_rec_iql", [f"env/scenario={SCENARIO}", *overrides, f"system.num_updates_per_eval={updates}"])
    env, _ = envs.make(cfg)
    learn, _, state = learner_setup(env, (1, 2), cfg)
    L = learn.learner
    while not L.can_train():  # fill the buffer past the train gate (untimed)
        state = learn(state).learner_state
    state = learn(state).learner_state  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        state = learn(state).learner_state
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / updates)
    cnt = LaunchCounter()
    learn(state)
    torch.cuda.synchronize()
    cnt.close()
    med = statistics.median(times)
    E, T = L.E, L.T
    buf_bytes = sum(t.numel() * t.element_size() for f in L.buf for t in (f if isinstance(f, tuple) else (f,)))
    return {"shape": name, "num_envs": E, "num_agents": L.A, "rollout_length": T, "epochs": L.K, "sample_batch_size": L.B,
            "sample_sequence_length": L.L, "buffer_size": L.cap, "matmul_mode": L.matmul_mode,
            "median_update_ms": round(med * 1e3, 3), "update_ms_all": [round(x * 1e3, 3) for x in times],
            "env_steps_per_s": round(E * T / med, 1), "launches_per_update": cnt.n / updates,
            "replay_buffer_MB": round(buf_bytes / 2**20, 1)}


def curve(out_path):
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    recs = []
    t0 = time.time()
    rec_iql.run_experiment(compose("default_rec_iql", CURVE_OVERRIDES), log=recs.append)
    ev = [(r["timestep"], round(r["episode_return"], 4)) for r in recs if r["event"] == "EVAL"]
    res = {"overrides": CURVE_OVERRIDES, "seconds": round(time.time() - t0, 1), "curve [timestep, mean eval return]": ev,
           "measured_gain": round(gain([r for _, r in ev]), 4)}
    print(json.dumps(res))
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
        curve(a.out or os.path.join(ROOT, "profiles", "iql_learning_curve.json"))
        return
    res = {"device": torch.cuda.get_device_name(0), "scenario": SCENARIO, "shapes": []}
    for name, ov in SHAPES.items():
        r = bench_shape(name, ov, a.updates, a.repeats)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    with open(a.out or os.path.join(ROOT, "profiles", "iql_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
