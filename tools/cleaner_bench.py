#!/usr/bin/env python3
"""Cleaner measurements (DESIGN.md "Cleaner"; bench.py's headline is not involved).

    python tools/cleaner_bench.py [--out profiles/cleaner_bench.json] [--skip-learners]
    python tools/cleaner_bench.py --curve [--calls N --lr X --envs E --rollout T] [--out profiles/cleaner_learning_curve.json]

Default mode: the device time of one env step launch, graph-replayed, at 1024 envs of clean-5x5x5a, clean-10x10x10a and
clean-30x30x30a, with the compulsory bytes per launch and the GB/s they give.  These launches reset nothing: the agents
step onto the first open neighbour of the start and back, under a time limit that is never reached (20 launches per
graph, warm-up, median of 5).  In the same run: mava_connector_step at 1024 envs x con-10x10x10a, a launch that resets
every env, and for clean-10x10x10a the two numbers that say what the maze generator costs:
  (a) no_reset_us      - the launch above, in which no env resets;
  (b) steady_state_us  - the mean launch of 2 * time_limit consecutive steps of masked-random actions (the policy's mask
                         makes invalid moves impossible, so episodes end at the time limit or by a win).  The actions are
                         drawn in an untimed run, the state is restored, and the same steps are replayed from one graph.
Then env-steps/s through learn() of ff_mappo and rec_mappo on clean-5x5x5a.
--curve: the learning curve of tests/test_gpu_cleaner.py::test_ppo_learns_cleaner (mean eval return and win rate after
every learn() call), the measurement its threshold is set from; the options override single entries of CURVE.
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

# tests/test_gpu_cleaner.py::test_ppo_learns_cleaner runs exactly this configuration
CURVE = dict(system="ff_mappo", scenario="clean-5x5x5a", network="mlp", envs=1024, rollout=64, updates_per_call=10, calls=12,
             seed=42, lr=5e-4, eval_envs=256)
NEVER = 1 << 30  # a time limit no run reaches


def env_step_bytes(R: int, C: int, A: int, real: bool = False) -> dict:
    """Bytes one environment moves per step launch (compulsory traffic: state read + written, action, outputs)."""
    state = 8 * A + R * C + 4 * A + 16  # pos, grid, step_count, 4 metric words
    view, mask = 16 * A * R * C, 4 * A
    out = view + 12 * R * C + mask + 4 * A + 4 * A + A + 9  # view, global state, mask, step_count, reward, done, info
    if real:
        out += view + mask + 1
    return {"read": state + 4 * A, "written": state + out, "total": 2 * state + 4 * A + out}


def _compose(system: str, scenario: str, network: str, extra):
    from mava_amd.config import compose

    return compose(f"default_{system}", ["env=cleaner", f"env/scenario={scenario}", f"network={network}"] + list(extra))


def learning_curve(dev, log=None, **override) -> list:
    """[(updates, seconds, mean eval return, eval win rate in %)] of CURVE's configuration (entries replaced by
    `override`), fixed seeds."""
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
        out = evaluator(state.params.actor_params, 1000 + i)
        return float(out["episode_return"].float().mean()), 100.0 * float(out["won_episode"].float().mean())

    curve = [(0, 0.0, *ev(0))]
    t0 = time.perf_counter()
    for i in range(c["calls"]):
        state = learn(state).learner_state
        torch.cuda.synchronize()
        curve.append(((i + 1) * c["updates_per_call"], round(time.perf_counter() - t0, 2), *ev(i + 1)))
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
    res = {"workload": f"{system} cleaner {scenario} network={network}", "envs": E, "rollout_length": L.T, "agents": L.A,
           "obs_dim": L.Oa, "state_dim": L.Oc, "steps": steps, "repeats": 3,
           "env_steps_per_s": steps * L.T * L.U * L.E / el, "ms_per_update": 1e3 * el / steps,
           "ms_per_update_all": [round(1e3 * t / steps, 3) for t in times]}
    del learn, state, L
    torch.cuda.empty_cache()
    return res


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _make(scenario: str, E: int, dev, time_limit=None):
    from mava_amd import envs

    extra = [f"arch.num_envs={E}"] + ([f"env.kwargs.time_limit={time_limit}"] if time_limit else [])
    return envs.make(_compose("ff_mappo", scenario, "mlp", extra), add_global_state=True, device=dev)[0]


def _masked_random(mask: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    return (torch.rand(mask.shape, device=mask.device, generator=gen) * mask).argmax(-1).to(torch.int32)


def _time_no_reset(env, dev) -> float:
    """Median device us per launch when no env resets: there (the first legal move of the reset state) and back."""
    import bench

    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(env.num_envs, env.num_agents, dev)
    there = obs["action_mask"].float().argmax(-1).to(torch.int32)
    acts = (there, (there + 2) % 4)
    calls = [0]

    def step(_i):  # alternates over the warm-up calls, the capture and every replay (an even number of launches per graph)
        env.step_into(st, 1 + calls[0], obs, *tr, action=acts[calls[0] % 2])
        calls[0] += 1

    us = bench._graph_time_us(step, 1, dev)
    assert int(st.run_length.min()) > 0 and int(st.step_count.min()) > 0  # nothing ended, nothing was reset
    return us


def _time_all_reset(env, dev) -> float:
    import bench

    st, obs = env.alloc_state(), env.alloc_obs()
    return bench._graph_time_us(lambda i: env.step_into(st, i, obs, is_reset=True), 20, dev)


def _time_steady_state(env, dev, reps: int = 5) -> dict:
    """Mean device us per launch over 2 * time_limit consecutive steps of masked-random actions, resets included."""
    E, A, n = env.num_envs, env.num_agents, 2 * env.time_limit
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, A, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for t in range(1, env.time_limit // 2 + 1):  # off the reset state
        env.step_into(st, t, obs, *tr, action=_masked_random(obs["action_mask"], gen))
    t0 = env.time_limit // 2
    saved = [x.clone() for x in st]
    acts = torch.empty((n, E, A), dtype=torch.int32, device=dev)
    ends = 0
    for i in range(n):  # the untimed run that draws the actions
        acts[i] = _masked_random(obs["action_mask"], gen)
        env.step_into(st, t0 + 1 + i, obs, *tr, action=acts[i])
        ends += int(tr[4].sum())

    def restore():
        for x, y in zip(st, saved):
            x.copy_(y)

    restore()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for i in range(n):
                env.step_into(st, t0 + 1 + i, obs, *tr, action=acts[i])
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps + 1):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / n)
    ts = sorted(ts[1:])
    return {"steady_state_us": ts[len(ts) // 2], "launches": n, "episode_ends_per_launch": ends / n, "all": ts}


def step_device_times(dev) -> dict:
    import connector_bench
    from mava_amd import envs
    from mava_amd.config import compose

    out = {}
    E = 1024
    for scenario in ("clean-5x5x5a", "clean-10x10x10a", "clean-30x30x30a"):
        env = _make(scenario, E, dev, NEVER)
        us = _time_no_reset(env, dev)
        b = env_step_bytes(env.num_rows, env.num_cols, env.num_agents)["total"] * E
        cp = connector_bench._time_copy(b, dev)
        out[f"cleaner_step {E} x {scenario}"] = {"us_per_launch": us, "bytes_per_launch": b, "GBps": b / us / 1e3,
                                                 "same_bytes_copy_us": cp, "same_bytes_copy_GBps": b / cp / 1e3,
                                                 "all_envs_reset_us": _time_all_reset(env, dev)}
        del env
        torch.cuda.empty_cache()
    con, _ = envs.make(compose("default_ff_mappo", ["env=connector", "env/scenario=con-10x10x10a", f"arch.num_envs={E}"]),
                       add_global_state=True, device=dev)
    us = connector_bench._time_step(con, False, dev)
    b = connector_bench.env_step_bytes(con.grid_size, con.num_agents)["total"] * E
    out[f"connector_step {E} x con-10x10x10a"] = {"us_per_launch": us, "bytes_per_launch": b, "GBps": b / us / 1e3}
    a_us = out[f"cleaner_step {E} x clean-10x10x10a"]["us_per_launch"]
    steady = _time_steady_state(_make("clean-10x10x10a", E, dev), dev)
    out[f"reset_cost {E} x clean-10x10x10a"] = {"no_reset_us": a_us, **steady,
                                                "steady_minus_no_reset_over_no_reset": (steady["steady_state_us"] - a_us) / a_us}
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
        raise SystemExit("cleaner_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.curve:
        ov = {k: v for k, v in (("calls", args.calls), ("lr", args.lr), ("envs", args.envs), ("rollout", args.rollout),
                                ("network", args.network)) if v is not None}
        curve = learning_curve(dev, log=lambda m: print(m, file=sys.stderr, flush=True), **ov)
        out = {"config": dict(CURVE, **ov), "curve [updates, seconds, mean eval return, eval win rate %]": curve,
               "measured_gain": gain(curve), "win_rate_at_end": curve[-1][3]}
    else:
        out = {"device": torch.cuda.get_device_name(0), "env_step_graph_timed": step_device_times(dev)}
        if not args.skip_learners:
            out["results"] = [throughput("ff_mappo", "mlp", "clean-5x5x5a", 4096, 10, 3, dev),
                              throughput("rec_mappo", "rnn", "clean-5x5x5a", 4096, 5, 2, dev)]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
