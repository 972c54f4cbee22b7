#!/usr/bin/env python3
"""Connector measurements (DESIGN.md "Connector"; bench.py's headline is not involved).

    python tools/connector_bench.py [--out profiles/connector_bench.json] [--skip-learners]
    python tools/connector_bench.py --curve [--calls N --lr X --envs E --rollout T] [--out profiles/connector_learning_curve.json]

Default mode: the device time of one env step launch, graph-replayed (20 launches per graph, warm-up, median of 5), for
mava_connector_step without and with its real_view / real_mask / terminated outputs at 4096 envs x con-5x5x3a and 1024 envs x con-10x10x10a, with the
compulsory bytes per launch and the GB/s they give; in the same run mava_rware_step at 4096 envs x tiny-4ag and a
device-to-device copy of the same number of bytes as each Connector step moves.  Then env-steps/s through learn() of
ff_mappo (network=mlp and network=cnn) and rec_mappo on con-5x5x3a.
--curve: the learning curve of tests/test_gpu_connector.py::test_ppo_learns_connector (mean eval return after every
learn() call), the measurement its threshold is set from; the options override single entries of CURVE.
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

# tests/test_gpu_connector.py::test_ppo_learns_connector runs exactly this configuration
CURVE = dict(system="ff_mappo", scenario="con-5x5x3a", network="mlp", envs=1024, rollout=64, updates_per_call=10, calls=12,
             seed=42, lr=5e-4, eval_envs=256)


def env_step_bytes(G: int, A: int, real: bool = False) -> dict:
    """Bytes one environment moves per step launch (compulsory traffic: state read + written, action, outputs)."""
    state = 4 * (2 * A + 2 * A) + A + G * G + 4 * A + 16  # head, target, connected, grid, step_count, 4 metric words
    view, mask = 4 * A * G * G * 5, 5 * A
    out = view + 4 * G * G * 3 + mask + 4 * A + 4 * A + A + 9  # view, global state, mask, step_count, reward, done, info
    if real:
        out += view + mask + 1
    return {"read": state + 4 * A, "written": state + out, "total": 2 * state + 4 * A + out}


def _compose(system: str, scenario: str, network: str, extra):
    from mava_amd.config import compose

    return compose(f"default_{system}", ["env=connector", f"env/scenario={scenario}", f"network={network}"] + list(extra))


def learning_curve(dev, log=None, **override) -> list:
    """[(updates, seconds, mean eval return)] of CURVE's configuration (entries replaced by `override`), fixed seeds."""
    from mava_amd import envs
    from mava_amd.evaluator import get_eval_fn, make_ff_eval_act_fn

    c = dict(CURVE, **override)
    system = importlib.import_module(f"mava_amd.systems.ppo.{c['system']}")
    cfg = _compose(c["system"], c["scenario"], c["network"],
                   [f"arch.num_envs={c['envs']}", f"system.rollout_length={c['rollout']}", "system.update_batch_size=1",
                    f"system.seed={c['seed']}", f"system.actor_lr={c['lr']}", f"system.critic_lr={c['lr']}",
                    f"arch.num_eval_episodes={c['eval_envs']}"])
    cfg.system.num_updates_per_eval = c["updates_per_call"]
    central = c["system"].endswith("mappo")
    env, eval_env = envs.make(cfg, add_global_state=central, device=dev)
    learn, actor_network, state = system.learner_setup(env, (c["seed"], c["seed"] + 2, c["seed"] + 3), cfg, device=dev)
    evaluator = get_eval_fn(eval_env, make_ff_eval_act_fn(actor_network.apply, cfg), cfg, absolute_metric=False)

    def ev(i):
        return float(evaluator(state.params.actor_params, 1000 + i)["episode_return"].float().mean())

    curve = [(0, 0.0, ev(0))]
    t0 = time.perf_counter()
    for i in range(c["calls"]):
        state = learn(state).learner_state
        torch.cuda.synchronize()
        curve.append(((i + 1) * c["updates_per_call"], round(time.perf_counter() - t0, 2), ev(i + 1)))
        if log:
            log(f"  {curve[-1]}")
    return curve


def gain(curve) -> float:
    """Mean eval return of the last three evaluations minus the untrained policy's."""
    return sum(c[2] for c in curve[-3:]) / 3.0 - curve[0][2]


def throughput(system: str, network: str, scenario: str, E: int, steps: int, warmup: int, dev) -> dict:
    import bench
    from mava_amd import envs

    cfg = _compose(system, scenario, network, [f"arch.num_envs={E}", "system.update_batch_size=1"])
    cfg.system.num_updates_per_eval = steps
    cfg.system.num_updates = 4 * steps + warmup
    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    env, _ = envs.make(cfg, add_global_state=system.endswith("mappo"), device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    times, _ = bench.time_learn(learn, state, L, steps, warmup, 3, 1)
    el = bench._median(times)
    res = {"workload": f"{system} connector {scenario} network={network}", "envs": E, "rollout_length": L.T, "agents": L.A,
           "obs_dim": L.Oa, "state_dim": L.Oc, "steps": steps, "repeats": 3,
           "env_steps_per_s": steps * L.T * L.U * L.E / el, "ms_per_update": 1e3 * el / steps,
           "ms_per_update_all": [round(1e3 * t / steps, 3) for t in times]}
    del learn, state, L
    torch.cuda.empty_cache()
    return res


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _time_step(env, real: bool, dev) -> float:
    """Median device us per launch of env.step_into: random actions, mid-episode states, 20 launches per graph."""
    import bench

    E, A = env.num_envs, env.num_agents
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, A, dev)
    act = torch.randint(0, env.action_dim, (E, A), dtype=torch.int32, device=dev)
    kw = {}
    if real:
        kw = dict(real_obs={"agents_view": torch.empty_like(obs["agents_view"]), "action_mask": torch.empty_like(obs["action_mask"])},
                  terminated=torch.empty(E, dtype=torch.uint8, device=dev))
    for t in range(1, 11):  # off the reset state
        env.step_into(st, t, obs, *tr, action=act, **kw)
    return bench._graph_time_us(lambda i: env.step_into(st, 11 + i, obs, *tr, action=act, **kw), 1, dev)


def _time_copy(nbytes: int, dev) -> float:
    """A device-to-device copy that moves `nbytes` in total (half read, half written), timed the same way."""
    import bench

    n = max(nbytes // 8, 1)
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    return bench._graph_time_us(lambda i: dst.copy_(src), 1, dev)


def step_device_times(dev) -> dict:
    import rware_bench
    from mava_amd import envs
    from mava_amd.config import compose

    out = {}
    for scenario, E in (("con-5x5x3a", 4096), ("con-10x10x10a", 1024)):
        env, _ = envs.make(_compose("ff_mappo", scenario, "mlp", [f"arch.num_envs={E}"]), add_global_state=True, device=dev)
        G, A = env.grid_size, env.num_agents
        # (row names, not symbols: "_real_next" = mava_connector_step with its real-next outputs; the committed profiles keep them)
        for name, real in (("connector_step", False), ("connector_step_real_next", True)):
            us = _time_step(env, real, dev)
            b = env_step_bytes(G, A, real)["total"] * E
            cp = _time_copy(b, dev)
            out[f"{name} {E} x {scenario}"] = {"us_per_launch": us, "bytes_per_launch": b, "GBps": b / us / 1e3,
                                               "same_bytes_copy_us": cp, "same_bytes_copy_GBps": b / cp / 1e3}
    E = 4096
    rw, _ = envs.make(compose("default_ff_mappo", ["env=rware_native", "env/scenario=tiny-4ag", f"arch.num_envs={E}"]),
                      add_global_state=True, device=dev)
    us = _time_step(rw, False, dev)
    b = rware_bench.env_step_bytes(rw.num_agents, rw.num_shelves, rw.request_queue_size, rw.sensor_range)["total"] * E
    out[f"rware_step {E} x tiny-4ag"] = {"us_per_launch": us, "bytes_per_launch": b, "GBps": b / us / 1e3}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--skip-learners", action="store_true")
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--rollout", type=int, default=None)
    ap.add_argument("--network", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("connector_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.curve:
        ov = {k: v for k, v in (("calls", args.calls), ("lr", args.lr), ("envs", args.envs), ("rollout", args.rollout),
                                ("network", args.network)) if v is not None}
        curve = learning_curve(dev, log=lambda m: print(m, file=sys.stderr, flush=True), **ov)
        out = {"config": dict(CURVE, **ov), "curve [updates, seconds, mean eval return]": curve, "measured_gain": gain(curve)}
    else:
        out = {"device": torch.cuda.get_device_name(0), "env_step_graph_timed": step_device_times(dev)}
        if not args.skip_learners:
            out["results"] = [throughput("ff_mappo", "mlp", "con-5x5x3a", 4096, 10, 3, dev),
                              throughput("ff_mappo", "cnn", "con-5x5x3a", 1024, 3, 1, dev),
                              throughput("rec_mappo", "rnn", "con-5x5x3a", 4096, 5, 2, dev)]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
