#!/usr/bin/env python3
"""The learning curve of ff_isac / ff_masac on env=spread (DESIGN.md "Soft actor-critic").

    python tools/sac_learning.py [--system ff_masac] [--calls N --envs E --epochs K --batch B] [--out profiles/sac_learning_curve.json]

Explores with random actions, then alternates learn() calls with an evaluation of the sampled policy on the evaluation
envs (their own Philox key).  tests/test_gpu_sac_learning.py runs CURVE as it stands and compares the last evaluation
with the random and the scripted policy of tests/spread_model.py; the options override single entries of CURVE.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# tests/test_gpu_sac_learning.py::test_isac_learns_spread runs exactly this configuration
CURVE = dict(system="ff_isac", scenario="spread-3a", envs=64, rollout=2, epochs=2, batch=256, delay=2, explore=5120,
             updates_per_call=100, calls=28, seed=1, eval_envs=320)


def learning_curve(dev, log=None, **override) -> list:
    """[(env steps, seconds of explore + learn, mean eval return)] of CURVE's configuration (entries replaced by
    `override`), fixed seeds; the first entry is the untrained policy."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.evaluator import get_eval_fn, make_ff_eval_act_fn

    c = dict(CURVE, **override)
    system = importlib.import_module(f"mava_amd.systems.sac.{c['system']}")
    cfg = compose(f"default_{c['system']}_spread", [f"env/scenario={c['scenario']}", f"arch.num_envs={c['envs']}",
                                             f"system.rollout_length={c['rollout']}", f"system.epochs={c['epochs']}",
                                             f"system.batch_size={c['batch']}", f"system.policy_update_delay={c['delay']}",
                                             f"system.explore_steps={c['explore']}", f"system.seed={c['seed']}",
                                             f"arch.num_eval_episodes={c['eval_envs']}", "system.buffer_size=100000"])
    cfg.system.num_updates_per_eval = c["updates_per_call"]
    central = c["system"] == "ff_masac"
    env, eval_env = envs.make(cfg, add_global_state=central, device=dev)
    learn, actor_network, state = system.learner_setup(env, [c["seed"] + i for i in range(6)], cfg, device=dev)
    evaluator = get_eval_fn(eval_env, make_ff_eval_act_fn(actor_network.apply, cfg), cfg, absolute_metric=False)
    ev = lambda i: float(evaluator(state.params.actor, 1000)["episode_return"].float().mean())  # the same eval seed every time
    curve = [(0, 0.0, ev(0))]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    learn.explore()
    for i in range(c["calls"]):
        state = learn(state).learner_state
        torch.cuda.synchronize()
        secs = round(time.perf_counter() - t0, 2)
        if i + 1 == c["calls"] or log:  # the evaluations in between are the curve's, not the test's
            curve.append((learn.learner.t, secs, ev(i + 1)))
            if log:
                log(f"  {curve[-1]} log_alpha={learn.learner.log_alpha.tolist()}")
    return curve


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default=None)
    for k in ("calls", "envs", "epochs", "batch", "delay", "updates_per_call"):
        ap.add_argument(f"--{k}", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sac_learning.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ov = {k: v for k, v in vars(args).items() if k != "out" and v is not None}
    curve = learning_curve(dev, log=lambda m: print(m, file=sys.stderr, flush=True), **ov)
    out = {"device": torch.cuda.get_device_name(0), "config": dict(CURVE, **ov), "curve [env steps, seconds, mean eval return]": curve,
           "measured_gain": curve[-1][2] - curve[0][2], "seconds": curve[-1][1]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
