#!/usr/bin/env python3
"""Soft actor-critic timings (DESIGN.md "Soft actor-critic"; bench.py's headline is not involved).

    python tools/sac_bench.py [--out profiles/sac_bench.json]

For ff_isac and ff_masac on spread-3a with the reference's system defaults (batch 32, epochs 32, rollout_length 2, policy
delay 4 - at num_envs 16 every epoch trains the actor four times): wall ms per update step and per train step (epoch),
env-steps/s through learn(), and the kernel launches of one update step counted through the library's launch hook.
Warm-up first, median of 3 timed repeats of `--updates` update steps each, the device synchronised around every repeat.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def measure(system: str, dev, updates: int, overrides=()) -> dict:
    from mava_amd import _lib, envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.sac.{system}")
    cfg = compose(f"default_{system}_spread", ["system.buffer_size=100000", "system.explore_steps=1024", *overrides])
    cfg.system.num_updates_per_eval = updates
    env, _ = envs.make(cfg, add_global_state=system == "ff_masac", device=dev)
    learn, _net, state = mod.learner_setup(env, [1, 2, 3, 4, 5, 6], cfg, device=dev)
    L = learn.learner
    learn.explore()
    state = learn(state).learner_state  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        state = learn(state).learner_state
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # launches of one update step: every product and kernel goes through _lib.launch or a checked direct call; count the
    # timed ones (TIMERS brackets each launch() call with an event pair)
    L.n_upd = 1
    _lib.TIMERS = {}
    L.update(0)
    torch.cuda.synchronize()
    counted = {k: len(v) for k, v in _lib.TIMERS.items()}
    _lib.TIMERS = None
    el = statistics.median(times)
    return {"workload": f"{system} env=spread spread-3a network=continuous_mlp", "overrides": list(overrides), "envs": L.E,
            "rollout_length": L.T, "epochs": L.K, "batch_size": L.B, "policy_update_delay": L.delay, "matmul_mode": L.matmul_mode,
            "updates": updates, "repeats": 3, "ms_per_update": 1e3 * el / updates, "ms_per_train_step": 1e3 * el / updates / L.K,
            "ms_per_update_all": [round(1e3 * t / updates, 3) for t in times], "env_steps_per_s": updates * L.T * L.E / el,
            "launch_calls_per_update_step": counted, "launch_calls_per_update_step_total": sum(counted.values())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sac_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0),
           "results": [measure("ff_isac", dev, args.updates), measure("ff_masac", dev, args.updates),
                       measure("ff_isac", dev, args.updates, ["arch.num_envs=64", "system.batch_size=256", "system.epochs=2",
                                                              "system.policy_update_delay=2"])]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
