#!/usr/bin/env python3
"""Robot Warehouse measurements (DESIGN.md "Robot Warehouse"; bench.py's headline is not involved).

    python tools/rware_bench.py [--envs 4096] [--scenario tiny-4ag] [--out profiles/rware_bench.json]
    python tools/rware_bench.py --curve [--scenario S --collision-mode M --calls N ...] [--out profiles/rware_learning_curve.json]

Default mode: the device time of one env step launch (graph-replayed; the LBF step and the synthetic RWARE step at the
same number of envs next to it, same box, same run), then ff_mappo and rec_mappo on RWARE: env-steps/s through learn()
(median of 3 calls, timed like bench.py's secondary workloads with its own build_learner / time_learn), one
instrumented pass for the per-launch times of the env step and the acting (policy) step from the learners' HIP-event
timers (these include the Python launch cost), and the env step's bytes per launch.
--curve: the learning curve of tests/test_gpu_rware.py::test_ppo_learns_rware (mean eval return after every learn()
call), the measurement its threshold is set from; the options override single entries of CURVE for trying other settings.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# tests/test_gpu_rware.py::test_ppo_learns_rware runs exactly this configuration
CURVE = dict(system="ff_mappo", scenario="tiny-2ag", collision_mode="terminate", envs=1024, rollout=128,
             updates_per_call=10, calls=30, seed=42, lr=5e-4, eval_envs=256)


def env_step_bytes(A: int, S: int, R: int, sensor_range: int = 1) -> dict:
    """Bytes one environment moves per step launch (compulsory traffic: state read + written, action, outputs)."""
    state = 4 * (2 * A + A + A + S + R + A + 4)  # position, direction, carry, shelves, queue, step_count, 4 metric words
    raw = 8 + 7 * (2 * sensor_range + 1) ** 2
    out = 4 * A * (A + raw) + 4 * A * raw + 5 * A + 4 * A + 4 * A + A + 9  # view, state, mask, step_count, reward, done, info
    return {"read": state + 4 * A, "written": state + out, "total": 2 * state + 4 * A + out}


def learning_curve(dev, log=None, **override) -> list:
    """[(updates, seconds, mean eval return)] of CURVE's configuration (entries replaced by `override`), fixed seeds."""
    import importlib

    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.evaluator import get_eval_fn, make_ff_eval_act_fn

    c = dict(CURVE, **override)
    system = importlib.import_module(f"mava_amd.systems.ppo.{c['system']}")
    cfg = compose(f"default_{c['system']}", ["env=rware_native", f"env/scenario={c['scenario']}",
                                             f"env.kwargs.collision_mode={c['collision_mode']}", f"arch.num_envs={c['envs']}",
                                             f"system.rollout_length={c['rollout']}", "system.update_batch_size=1",
                                             f"system.seed={c['seed']}", f"system.actor_lr={c['lr']}",
                                             f"system.critic_lr={c['lr']}", f"arch.num_eval_episodes={c['eval_envs']}"])
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


def throughput(system: str, scenario: str, envs_per_gpu: int, steps: int, warmup: int, dev) -> dict:
    import bench

    learn, state, L, cfg = bench.build_learner(system, "rware_native", scenario, envs_per_gpu, 1, "f16x2", steps, warmup, dev)
    times, _ = bench.time_learn(learn, state, L, steps, warmup, 3, 1)
    el = bench._median(times)
    ff_t, rec_t, n = bench.instrumented_pass(L, 2, 1)
    tm = ff_t or rec_t
    per = {k: bench._median(bench._ev_ms(v)) * 1e3 for k, v in tm.items()}  # median us per launch
    env0 = L.reps[0].env
    b = env_step_bytes(env0.num_agents, env0.num_shelves, env0.request_queue_size, env0.sensor_range)
    env_us = per["env_step"]
    policy_key = "policy_step" if ff_t else "rec_step"
    res = {"workload": f"{system} rware_native {scenario}", "envs": envs_per_gpu, "rollout_length": L.T, "agents": L.A,
           "obs_dim": L.Oa, "state_dim": L.Oc, "steps": steps, "repeats": 3,
           "env_steps_per_s": steps * L.T * L.U * L.E / el, "ms_per_update": 1e3 * el / steps,
           "ms_per_update_all": [round(1e3 * t / steps, 3) for t in times],
           "env_step_us_per_launch": env_us, "policy_step_us_per_launch": per[policy_key], "policy_kernel": policy_key,
           "env_step_bytes_per_env": b, "env_step_bytes_per_launch": b["total"] * L.E,
           "env_step_achieved_GBps": b["total"] * L.E / (env_us * 1e-6) / 1e9,
           "per_launch_us": {k: round(v, 2) for k, v in sorted(per.items())}}
    del learn, state, L
    torch.cuda.empty_cache()
    return res


def step_device_times(scenario: str, E: int, dev) -> dict:
    """Device time per launch (us) of the RWARE step (plain and with the pre-reset observation) and, on the same box in
    the same run, of the LBF step (15x15-4p-5f) and the synthetic RWARE step at the same number of envs and agents:
    20 launches replayed from one HIP graph, so that the Python launch cost (~10 us) is not in the number.  Random
    actions, mid-episode states."""
    import bench
    from mava_amd import envs
    from mava_amd.config import compose

    cfg = compose("default_ff_mappo", ["env=rware_native", f"env/scenario={scenario}", f"arch.num_envs={E}"])
    rw, _ = envs.make(cfg, add_global_state=True, device=dev)
    A = rw.num_agents
    lbf_env, _ = envs.make(compose("default_ff_mappo", ["env=lbf", "env/scenario=15x15-4p-5f", f"arch.num_envs={E}"]),
                           add_global_state=True, device=dev)
    syn = envs.SyntheticRware(E, A, obs_dim=66, num_actions=5, add_global_state=True, device=dev)
    out = {}
    # (row names, not symbols: "_real_next" = mava_rware_step with its real-next outputs; the committed profiles keep these keys)
    for name, env, real in (("rware_step", rw, False), ("rware_step_real_next", rw, True), ("lbf_step", lbf_env, False),
                            ("synth_rware_step", syn, False)):
        A = env.num_agents
        st, obs = env.alloc_state(), env.alloc_obs()
        env.step_into(st, 0, obs, is_reset=True)
        tr = (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
              torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
        act = torch.randint(0, env.action_dim, (E, A), dtype=torch.int32, device=dev)
        kw = {}
        if real:
            kw = dict(real_obs={"agents_view": torch.empty_like(obs["agents_view"]), "action_mask": torch.empty_like(obs["action_mask"])},
                      terminated=torch.empty(E, dtype=torch.uint8, device=dev))
        for t in range(1, 31):  # off the reset state
            env.step_into(st, t, obs, *tr, action=act, **kw)
        out[name] = bench._graph_time_us(lambda i: env.step_into(st, 31 + i, obs, *tr, action=act, **kw), 1, dev)
    return {"envs": E, "agents": rw.num_agents, "scenario": scenario, "device_us_per_launch": out}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--scenario", default=None)
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--system", default=None)
    ap.add_argument("--collision-mode", default=None)
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--rollout", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rware_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.curve:
        ov = {k: v for k, v in (("system", args.system), ("scenario", args.scenario), ("collision_mode", args.collision_mode),
                                ("calls", args.calls), ("lr", args.lr), ("envs", args.envs), ("rollout", args.rollout))
              if v is not None}
        curve = learning_curve(dev, log=lambda m: print(m, file=sys.stderr, flush=True), **ov)
        out = {"config": dict(CURVE, **ov), "curve [updates, seconds, mean eval return]": curve, "measured_gain": gain(curve)}
    else:
        scenario, E = args.scenario or "tiny-4ag", args.envs or 4096
        out = {"device": torch.cuda.get_device_name(0), "env_step_graph_timed": step_device_times(scenario, E, dev),
               "results": [
            throughput("ff_mappo", scenario, E, 10, 3, dev),
            throughput("rec_mappo", scenario, E, 5, 2, dev)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
