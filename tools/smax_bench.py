#!/usr/bin/env python3
"""SMAX measurements (DESIGN.md "SMAX"; bench.py's headline is not involved).

    python tools/smax_bench.py [--out profiles/smax_bench.json] [--skip-learners]
    python tools/smax_bench.py --curve [--calls N --lr X --envs E --rollout T] [--out profiles/smax_learning_curve.json]

Default mode, in one run: the device time of one mava_smax_step launch, graph-replayed, at 2048 envs of 3s5z (20 launches
per graph, warm-up, median of 5) under uniform random action values - an attack that is not possible executes as a stop,
episodes end and reset along the way - with the compulsory bytes per launch and the GB/s they give; next to it the same
figures of mava_cleaner_step at 2048 envs of clean-10x10x10a and of a device copy of the same number of bytes.  Then
env-steps/s through learn() of ff_mappo and rec_mappo on 3s5z at 2048 envs, native (env=smax_native) and on the synthetic
stand-in of the same shape (env=smax, the configuration BASELINE.json's config 4 was measured on).
--curve: the learning curve of tests/test_gpu_smax.py::test_ppo_learns_smax (mean eval return and win rate after every
learn() call); the options override single entries of CURVE.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

# tests/test_gpu_smax.py::test_ppo_learns_smax runs exactly this configuration
CURVE = dict(system="ff_mappo", scenario="3m", network="mlp", envs=256, rollout=32, updates_per_call=10, calls=3, seed=42,
             lr=1e-3, eval_envs=128)


def env_step_bytes(Na: int, Ne: int, real: bool = False) -> dict:
    """Bytes one environment moves per step launch (compulsory traffic: state read + written, action, outputs)."""
    U = Na + Ne
    state = 20 * U + 4 * Na + 16  # pos, health, cd, last_action; step_count; 4 metric words
    view, mask = 4 * Na * (Na + 11 * (U - 1) + 10), Na * (5 + Ne)
    out = view + 48 * U + mask + 4 * Na + 4 * Na + Na + 10  # view, global state, mask, step_count, reward, done, info
    if real:
        out += view + mask + 1
    return {"read": state + 4 * Na, "written": state + out, "total": 2 * state + 4 * Na + out}


def _compose(system: str, env: str, scenario: str, network: str, extra):
    from mava_amd.config import compose

    return compose(f"default_{system}", [f"env={env}", f"env/scenario={scenario}", f"network={network}"] + list(extra))


def learning_curve(dev, log=None, **override) -> list:
    """[(updates, seconds, mean eval return, eval win rate in %)] of CURVE's configuration (entries replaced by
    `override`), fixed seeds."""
    from mava_amd import envs
    from mava_amd.evaluator import get_eval_fn, make_ff_eval_act_fn

    c = dict(CURVE, **override)
    system = importlib.import_module(f"mava_amd.systems.ppo.{c['system']}")
    cfg = _compose(c["system"], "smax_native", c["scenario"], c["network"],
                   [f"arch.num_envs={c['envs']}", f"system.rollout_length={c['rollout']}", "system.update_batch_size=1",
                    f"system.seed={c['seed']}", f"system.actor_lr={c['lr']}", f"system.critic_lr={c['lr']}",
                    f"arch.num_eval_episodes={c['eval_envs']}"])
    cfg.system.num_updates_per_eval = c["updates_per_call"]
    central = c["system"].endswith("mappo")
    env, eval_env = envs.make(cfg, add_global_state=central, device=dev)
    learn, actor_network, state = system.learner_setup(env, (c["seed"], c["seed"] + 2, c["seed"] + 3), cfg, device=dev)
    evaluator = get_eval_fn(eval_env, make_ff_eval_act_fn(actor_network.apply, cfg), cfg, absolute_metric=False)

    def ev(i):
        out = evaluator(state.params.actor_params, 1000 + i)
        return float(out["episode_return"].float().mean()), 100.0 * float(out["won_episode"].float().mean())

    curve = [(0, 0.0, *ev(0))]
    t0 = time.perf_counter()
    for i in range(c["calls"]):
        state = learn(state).learner_state
        torch.cuda.synchronize()
        secs = round(time.perf_counter() - t0, 2)
        if i + 1 == c["calls"] or log:  # the evaluations in between are the curve's, not the test's
            curve.append(((i + 1) * c["updates_per_call"], secs, *ev(i + 1)))
            if log:
                log(f"  {curve[-1]}")
    return curve


def throughput(system: str, network: str, env_name: str, scenario: str, E: int, steps: int, warmup: int, dev) -> dict:
    import bench
    from mava_amd import envs

    cfg = _compose(system, env_name, scenario, network, [f"arch.num_envs={E}", "system.update_batch_size=1"])
    cfg.system.num_updates_per_eval = steps
    cfg.system.num_updates = 4 * steps + warmup
    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    env, _ = envs.make(cfg, add_global_state=system.endswith("mappo"), device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    times, _ = bench.time_learn(learn, state, L, steps, warmup, 3, 1)
    el = bench._median(times)
    res = {"workload": f"{system} env={env_name} {scenario} network={network}", "envs": E, "rollout_length": L.T, "agents": L.A,
           "obs_dim": L.Oa, "state_dim": L.Oc, "steps": steps, "repeats": 3,
           "env_steps_per_s": steps * L.T * L.U * L.E / el, "ms_per_update": 1e3 * el / steps,
           "ms_per_update_all": [round(1e3 * t / steps, 3) for t in times]}
    del learn, state, L
    torch.cuda.empty_cache()
    return res


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _time_step(env, dev) -> dict:
    """Median device us per launch over graph replays of 20 consecutive steps with uniform random action values."""
    import bench

    E, A = env.num_envs, env.num_agents
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, A, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    acts = torch.randint(0, env.action_dim, (23, E, A), device=dev, generator=gen, dtype=torch.int32)
    calls = [0]

    def step(_i):
        env.step_into(st, 1 + calls[0], obs, *tr, action=acts[calls[0] % 23])
        calls[0] += 1

    us = bench._graph_time_us(step, 1, dev)
    return {"us_per_launch": us, "episode_ends_in_the_last_launch": int(tr[4].sum())}


def step_device_times(dev) -> dict:
    import cleaner_bench
    import connector_bench
    from mava_amd import envs

    out = {}
    E = 2048
    env, _ = envs.make(_compose("ff_mappo", "smax_native", "3s5z", "mlp", [f"arch.num_envs={E}"]), add_global_state=True, device=dev)
    res = _time_step(env, dev)
    b = env_step_bytes(env.num_agents, env.num_enemies)["total"] * E
    cp = connector_bench._time_copy(b, dev)
    out[f"smax_step {E} x 3s5z"] = {**res, "bytes_per_launch": b, "GBps": b / res["us_per_launch"] / 1e3,
                                    "same_bytes_copy_us": cp, "same_bytes_copy_GBps": b / cp / 1e3}
    del env
    torch.cuda.empty_cache()
    cl = cleaner_bench._make("clean-10x10x10a", E, dev, cleaner_bench.NEVER)
    us = cleaner_bench._time_no_reset(cl, dev)
    b = cleaner_bench.env_step_bytes(cl.num_rows, cl.num_cols, cl.num_agents)["total"] * E
    out[f"cleaner_step {E} x clean-10x10x10a"] = {"us_per_launch": us, "bytes_per_launch": b, "GBps": b / us / 1e3}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--skip-learners", action="store_true")
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--rollout", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smax_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.curve:
        ov = {k: v for k, v in (("calls", args.calls), ("lr", args.lr), ("envs", args.envs), ("rollout", args.rollout)) if v is not None}
        curve = learning_curve(dev, log=lambda m: print(m, file=sys.stderr, flush=True), **ov)
        out = {"config": dict(CURVE, **ov), "curve [updates, seconds, mean eval return, eval win rate %]": curve,
               "measured_gain": curve[-1][2] - curve[0][2], "win_rate_at_end": curve[-1][3]}
    else:
        out = {"device": torch.cuda.get_device_name(0), "env_step_graph_timed": step_device_times(dev)}
        if not args.skip_learners:
            out["results"] = [throughput("ff_mappo", "mlp", "smax_native", "3s5z", 2048, 10, 3, dev),
                              throughput("ff_mappo", "mlp", "smax", "3s5z", 2048, 10, 3, dev),
                              throughput("rec_mappo", "rnn", "smax_native", "3s5z", 2048, 5, 2, dev),
                              throughput("rec_mappo", "rnn", "smax", "3s5z", 2048, 5, 2, dev)]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
