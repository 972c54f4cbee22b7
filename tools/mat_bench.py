#!/usr/bin/env python3
"""ff_mat measurements (bench.py's headline is not involved).

    python tools/mat_bench.py [--envs 1024] [--acting layerwise|fused] [--out profiles/mat_bench_fused.json]
    python tools/mat_bench.py --curve [--acting fused] [--out profiles/mat_learning_curve_fused.json]
    python tools/mat_bench.py --continuous [--envs 1024] [--out profiles/mat_continuous_bench.json]
    python tools/mat_bench.py --continuous --curve [--out profiles/mat_continuous_learning_curve.json]

Default mode: ms per update and library calls per update of ff_mat at its defaults on env=rware tiny-4ag, ff_mappo
(update_batch_size 1) in the same run for scale, and the per-launch HIP-event times of the attention and LayerNorm kernels at
rows = envs * 4 next to the bytes each launch moves.  Without --acting both settings of network.acting run in the same
process (the layer-wise path is the yardstick of the fused one), with the fused step's per-launch time, the library calls per
update the code implies and the fused step's maximum differences from the float64 model on the shapes of
tests/test_gpu_mat_fused_act.py; with --acting only that setting runs.
--curve: the learning run of tests/test_gpu_mat_learning.py - ff_mat and ff_mappo (network=mlp) for the same number of
env-steps and the same seed - with the bar the test holds ff_mat to.
--continuous: the same two measurements for the continuous action head on env=spread (CONT_CURVE): ff_mat
network=continuous_transformer against ff_mappo network=continuous_mlp, update cost layer-wise against fused.
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

# tests/test_gpu_mat_learning.py runs exactly this configuration
CURVE = dict(env="lbf", scenario="2s-8x8-2p-2f-coop", envs=256, rollout=32, updates_per_call=10, calls=8, seed=42, lr=1e-3,
             eval_envs=256)
# a curve may carry extra config overrides per system ("overrides": {system: [...]}); none by default
# tests/test_gpu_mat_continuous_learning.py runs exactly CONT_CURVE: spread-2a, the smaller of the two scenarios at which ff_mappo's
# gain stands clear of its noise at CURVE's budget.  --continuous --curve also records spread-3a (CONT_CURVE_3A), where ff_mat at its
# default hyper-parameters misses the bar: see DESIGN.md 3.25.
CONT_CURVE = dict(CURVE, env="spread", scenario="spread-2a",
                  overrides={"ff_mappo": ["network=continuous_mlp"], "ff_mat": ["network=continuous_transformer"]})
CONT_CURVE_3A = dict(CONT_CURVE, scenario="spread-3a")
BAR_FACTOR = 0.4  # of ff_mappo's eval-return gain in the same run: the factor rec_qmix was held to against rec_iql


def _setup(system: str, dev, c=CURVE):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.evaluator import get_eval_fn, make_ff_eval_act_fn
    from mava_amd.systems.ppo import ff_mappo, ff_mat

    mod = {"ff_mat": ff_mat, "ff_mappo": ff_mappo}[system]
    cfg = compose(f"default_{system}", [f"env={c['env']}", f"env/scenario={c['scenario']}", f"arch.num_envs={c['envs']}",
                                        f"system.rollout_length={c['rollout']}", "system.update_batch_size=1", f"system.seed={c['seed']}",
                                        f"system.actor_lr={c['lr']}", f"system.critic_lr={c['lr']}",
                                        f"arch.num_eval_episodes={c['eval_envs']}"]
                  + list(c.get("overrides", {}).get(system, []))
                  + ([f"network.acting={c['acting']}"] if system == "ff_mat" and c.get("acting") else []))
    cfg.system.num_updates_per_eval = c["updates_per_call"]
    env, eval_env = envs.make(cfg, add_global_state=system == "ff_mappo", device=dev)
    learn, actor_network, state = mod.learner_setup(env, (c["seed"], c["seed"] + 2, c["seed"] + 3), cfg, device=dev)
    evaluator = get_eval_fn(eval_env, make_ff_eval_act_fn(actor_network.apply, cfg), cfg, absolute_metric=False)
    return cfg, learn, state, evaluator


def learning_curve(system: str, dev, log=None, c=CURVE) -> dict:
    """{"curve": [(env steps, seconds, mean eval return)], "final_sem": standard error of the last evaluation}."""
    _, learn, state, evaluator = _setup(system, dev, c)

    def ev(i):
        r = evaluator(state.params.actor_params, 1000 + i)["episode_return"].float()
        return float(r.mean()), float(r.std() / r.numel() ** 0.5)

    steps_per_call = c["updates_per_call"] * c["rollout"] * c["envs"]
    curve = [(0, 0.0, ev(0)[0])]
    sem = 0.0
    t0 = time.perf_counter()
    for i in range(c["calls"]):
        state = learn(state).learner_state
        torch.cuda.synchronize()
        mean, sem = ev(i + 1)
        curve.append(((i + 1) * steps_per_call, round(time.perf_counter() - t0, 2), mean))
        if log:
            log(f"  {system} {curve[-1]}")
    return {"curve": curve, "final_sem": sem}


def learning_run(dev, log=None, acting=None, curve=CURVE) -> dict:
    """Both systems on `curve`, and the bar: ff_mat's gain must reach BAR_FACTOR of ff_mappo's."""
    c = curve if acting is None else dict(curve, acting=acting)
    out = {"config": c, "bar_factor": BAR_FACTOR, "env_steps": c["calls"] * c["updates_per_call"] * c["rollout"] * c["envs"]}
    for system in ("ff_mappo", "ff_mat"):
        t0 = time.perf_counter()
        out[system] = learning_curve(system, dev, log, c)
        out[system]["wall_s"] = round(time.perf_counter() - t0, 2)
        cv = out[system]["curve"]
        out[system]["gain"] = cv[-1][2] - cv[0][2]
    out["bar"] = BAR_FACTOR * out["ff_mappo"]["gain"]
    return out


class _CallCounter:
    """Counts every call into libmavahip.so while active (the entry points are attributes of the CDLL object)."""

    def __init__(self):
        from mava_amd import _lib

        self.lib, self.names, self.n, self.by = _lib.lib(), list(_lib._SIGNATURES), 0, {}

    def __enter__(self):
        self.saved = {k: getattr(self.lib, k) for k in self.names}
        for k, fn in self.saved.items():
            def wrapped(*a, _fn=fn, _k=k):
                self.n += 1
                self.by[_k] = self.by.get(_k, 0) + 1
                return _fn(*a)
            setattr(self.lib, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(self.lib, k, fn)


ACT_SYMBOLS = ("mava_transformer_act_f32", "mava_transformer_act_continuous_f32")


def update_cost(system: str, envs_: int, dev, steps: int = 3, acting=None, continuous: bool = False) -> dict:
    base = dict(CONT_CURVE_3A) if continuous else dict(CURVE, env="rware", scenario="tiny-4ag")
    c = dict(base, envs=envs_, rollout=128, updates_per_call=1, lr=2.5e-4, eval_envs=32)
    if acting is not None:
        c["acting"] = acting
    cfg, learn, state, _ = _setup(system, dev, c)
    state = learn(state).learner_state  # warm-up (and ff_mappo's graph capture needs two calls)
    state = learn(state).learner_state
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        state = learn(state).learner_state
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    with _CallCounter() as cc:
        learn(state)
        torch.cuda.synchronize()
    L = learn.learner
    extra = {}
    if system == "ff_mat":
        extra["acting"] = L.acting
        # what MATPass.act launches layer by layer (its docstring), and what an update must then cost with the fused step:
        # T x (1 act + 1 env step) + the bootstrap's gather and encoder + the training calls
        per_act = 1 + len(L.roll.enc) + L.A * (2 + len(L.roll.dec))
        by = cc.by
        rollout_calls = sum(by.get(k, 0) for k in ACT_SYMBOLS) + by.get(L.rep.env.step_symbol, 0) if L.acting == "fused" else L.T * (per_act + 1)
        extra["layerwise_calls_per_act"] = per_act
        extra["library_calls_outside_rollout"] = cc.n - rollout_calls
        if L.acting == "fused":
            extra["fused_act_us_per_launch"] = _fused_step_us(L)
    return {"system": system, "envs": envs_, **extra, "agents": L.A, "rollout_length": L.T, "ms_per_update": round(1e3 * sorted(times)[len(times) // 2], 3),
            "ms_per_update_all": [round(1e3 * t, 3) for t in times], "env_steps_per_s": round(L.T * L.E / sorted(times)[len(times) // 2]),
            "library_calls_per_update": cc.n, "library_calls_by_symbol": dict(sorted(cc.by.items(), key=lambda kv: -kv[1]))}


def _fused_step_us(L, reps: int = 30) -> float:
    """Median HIP-event time (us, includes the Python launch cost) of one fused acting step of the learner's rollout pass."""
    rep = L.rep
    act = lambda: L.roll.act(L.p, rep.agents_view[0], rep.action_mask[0], rep.action[0], rep.log_prob[0], L.seed, 0, 0, False,
                             value_out=rep.value[0])
    act()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        act()
        b.record()
    torch.cuda.synchronize()
    return round(sorted(1e3 * a.elapsed_time(b) for a, b in ev)[reps // 2], 2)


def fused_accuracy(dev) -> dict:
    """The fused step against the float64 model on the shapes of tests/test_gpu_mat_fused_act.py (that module's cases and
    comparison): rows compared and the maximum log-prob and value differences over the sampled and the greedy run."""
    from tests import test_gpu_mat_fused_act as t

    cases, worst_lp, worst_v = [], 0.0, 0.0
    for shape in t.SHAPES + [t.MANY_GROUPS]:
        for greedy in (False, True):
            n, rows, e, v = t.measure(dev, shape, greedy)
            cases.append({"shape": list(shape), "greedy": greedy, "rows_compared": n, "rows": rows, "max_log_prob_error": e,
                          "max_value_error": v})
            worst_lp, worst_v = max(worst_lp, e), max(worst_v, v)
    return {"bound": 1e-5, "max_log_prob_error": worst_lp, "max_value_error": worst_v, "cases": cases}


def kernel_times(rows: int, dev, A: int = 4, D: int = 64, H: int = 1, reps: int = 30) -> dict:
    """Median HIP-event time per launch (us, includes the Python launch cost) and compulsory bytes per launch."""
    from mava_amd._lib import check, lib, ptr, stream_ptr

    L, B = lib(), rows // A
    f = lambda n: torch.randn(n, device=dev)
    q, k, v, dy, y, dq, dk, dv, xh = (f(rows * D) for _ in range(9))
    P, rstd, sc, bi = f(rows * H * A), f(rows), f(D), f(D)
    nb = min(256, rows // 32)
    slab = torch.zeros((nb, 2 * D), device=dev)
    s = stream_ptr()
    calls = {
        "attn_fwd": (lambda: L.mava_mat_attn_fwd_f32(ptr(q), ptr(k), ptr(v), rows, D, B, A, H, 1, ptr(y), ptr(P), nb, s),
                     4 * rows * (4 * D + H * A)),
        "attn_bwd": (lambda: L.mava_mat_attn_bwd_f32(ptr(dy), ptr(q), ptr(k), ptr(v), rows, D, B, A, H, 1, ptr(dq), ptr(dk), ptr(dv), nb, s),
                     4 * rows * 7 * D),
        "ln_fwd": (lambda: L.mava_mat_ln_fwd_f32(ptr(q), ptr(k), ptr(sc), ptr(bi), D, rows, rows, ptr(y), ptr(xh), ptr(rstd), nb, s),
                   4 * rows * (4 * D + 1)),
        "ln_bwd": (lambda: L.mava_mat_ln_bwd_f32(ptr(dy), ptr(xh), ptr(rstd), ptr(sc), D, rows, rows, 1.0, ptr(dq), ptr(slab), 2 * D, nb, s),
                   4 * rows * (3 * D + 1) + 4 * nb * 2 * D),
    }
    out = {}
    for name, (fn, nbytes) in calls.items():
        check(fn(), name)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)[reps // 2]
        out[name] = {"us_per_launch": round(us, 2), "bytes_per_launch": nbytes, "achieved_GBps": round(nbytes / us / 1e3, 1)}
    return {"rows": rows, "A": A, "D": D, "n_head": H, "kernels": out}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--continuous", action="store_true", help="the continuous action head on env=spread (CONT_CURVE)")
    ap.add_argument("--calls", type=int, default=None, help="--curve: learn() calls (the budget), default the curve's")
    ap.add_argument("--acting", choices=("layerwise", "fused"), default=None, help="network.acting of ff_mat (default: the "
                    "config's in --curve mode, both settings otherwise)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mat_bench.py measures on the GPU; no GPU found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.continuous and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mat_continuous_learning_curve.json" if args.curve else "mat_continuous_bench.json")
    if args.curve:
        curve = CONT_CURVE if args.continuous else CURVE
        if args.calls:
            curve = dict(curve, calls=args.calls)
        out = learning_run(dev, log=lambda m: print(m, file=sys.stderr, flush=True), acting=args.acting, curve=curve)
        out["device"] = torch.cuda.get_device_name(0)
        if args.continuous:
            log = lambda m: print(m, file=sys.stderr, flush=True)
            out["spread-3a"] = learning_run(dev, log=log, acting=args.acting, curve=dict(CONT_CURVE_3A, calls=curve["calls"]))
            vf = dict(CONT_CURVE_3A, calls=curve["calls"])
            vf["overrides"] = dict(vf["overrides"], ff_mat=vf["overrides"]["ff_mat"] + ["system.vf_coef=0.05"])
            out["spread-3a, ff_mat at system.vf_coef=0.05"] = learning_curve("ff_mat", dev, log, vf)
    elif args.continuous:
        settings = [args.acting] if args.acting else ["layerwise", "fused"]
        results = [update_cost("ff_mat", args.envs, dev, acting=a, continuous=True) for a in settings]
        results.append(update_cost("ff_mappo", args.envs, dev, continuous=True))
        out = {"device": torch.cuda.get_device_name(0), "workload": f"env=spread spread-3a x {args.envs} envs, continuous head, defaults",
               "results": results}
        by = {r.get("acting"): r for r in results if r["system"] == "ff_mat"}
        if len(by) == 2:
            out["fused_speedup_per_update"] = round(by["layerwise"]["ms_per_update"] / by["fused"]["ms_per_update"], 2)
    else:
        settings = [args.acting] if args.acting else ["layerwise", "fused"]
        results = [update_cost("ff_mat", args.envs, dev, acting=a) for a in settings] + [update_cost("ff_mappo", args.envs, dev)]
        out = {"device": torch.cuda.get_device_name(0), "workload": f"env=rware tiny-4ag x {args.envs} envs, defaults",
               "results": results, "kernel_times": kernel_times(args.envs * 4, dev)}
        by = {r.get("acting"): r for r in results if r["system"] == "ff_mat"}
        if "fused" in by:
            f = by["fused"]
            # T x (1 act + 1 env step) + everything the layer-wise update calls outside its rollout (bootstrap + training)
            outside = by["layerwise"]["library_calls_outside_rollout"] if "layerwise" in by else f["library_calls_outside_rollout"]
            f["library_calls_implied"] = 2 * f["rollout_length"] + outside
            f["library_calls_as_implied"] = f["library_calls_per_update"] == f["library_calls_implied"]
            out["fused_accuracy"] = fused_accuracy(dev)
        if len(by) == 2:
            out["fused_speedup_per_update"] = round(by["layerwise"]["ms_per_update"] / by["fused"]["ms_per_update"], 2)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
