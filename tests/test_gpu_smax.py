"""GPU: SMAX (mava_smax_step, csrc/smax.hip) against the NumPy rules of tests/smax_model.py, bit for bit; the hand-worked
cases and the golden file; captured-graph replay; the four PPO systems, run_experiment with its win rate, rec_iql and
learning on SMAX."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import smax_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = m.STATE_FIELDS
OBS = ("agents_view", "global_state", "action_mask", "step_count")
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")
# name: (scenario, E, model keywords, env seed).  A ragged last workgroup (8 envs each) in all three; Na != Ne and no wall
# deaths / hidden enemy actions in the second; the widest row (8 x 201 floats) and several workgroups in the third.  The
# env seeds were chosen on the model's event counts alone (test_model_runs_cover_the_rules).
CASES = {"2s3z": ("2s3z", 5, {}, 14), "5m_vs_6m": ("5m_vs_6m", 3, dict(walls_cause_death=False, see_enemy_actions=False), 10),
         "3s5z_vs_3s6z": ("3s5z_vs_3s6z", 33, {}, 1)}
STEPS = 121  # past the time limit of 100: every env auto-resets at least once


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import Smax

    return Smax(E, p.ally_types, p.enemy_types, p.time_limit, p.see_enemy_actions, p.walls_cause_death, add_global_state=True,
                seed=seed, env_offset=env_offset, device=dev)


def _host_state(st) -> dict:
    return {k: getattr(st, k).cpu().numpy().copy() for k in STATE_FIELDS}


def _load_state(st, host: dict) -> None:
    for k in STATE_FIELDS:
        getattr(st, k).copy_(torch.from_numpy(host[k]))


def _eq(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint8) if got.dtype == np.float32 else got,
                          want.astype(got.dtype).view(np.uint8) if got.dtype == np.float32 else want):
        bad = np.argwhere(got != want)
        where = tuple(bad[0]) if len(bad) else ()
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {bad[:3].tolist()}: got {got[where]!r} want {want[where]!r}")


def _check_obs(obs: dict, want: dict, what: str):
    for k in OBS:
        _eq(obs[k], want[k], f"{what} {k}")


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _real(env, dev):
    E, A = env.num_envs, env.num_agents
    return ({"agents_view": torch.empty((E, A, env.obs_dim), device=dev),
             "action_mask": torch.empty((E, A, env.action_dim), dtype=torch.uint8, device=dev)},
            torch.empty(E, dtype=torch.uint8, device=dev))


_MODEL_RUNS = {}


def model_run(name: str):
    """The model's side of test_kernel_matches_model, computed once per case and shared by its two variants: the reset
    at t = 0, then STEPS steps of the fixed action mix.  [(action, step result, state after)], the reset first."""
    if name not in _MODEL_RUNS:
        scen, E, kw, seed = CASES[name]
        p = m.scenario(scen, **kw)
        off = 12345
        hst, hobs = m.reset(p, E, seed, off, 0)
        run = [(None, (hobs,), {k: v.copy() for k, v in hst.items()})]
        rng = np.random.default_rng(5)
        mask = hobs["action_mask"]
        total = {k: 0 for k in m.EVENTS}
        ends = np.zeros(E, np.int64)
        for t in range(1, STEPS + 1):
            a = m.mixed_actions(rng, mask)
            want = m.step(p, hst, a, seed, off, t)
            mask = want[0]["action_mask"]
            for k in m.EVENTS:
                total[k] += want[6]["events"][k]
            ends += want[5]
            run.append((a, want, {k: v.copy() for k, v in hst.items()}))
        total["min_ends"] = int(ends.min())
        _MODEL_RUNS[name] = (p, seed, off, run, total)
    return _MODEL_RUNS[name]


def test_model_runs_cover_the_rules():
    """Counted in the model's outputs alone: the three runs of test_kernel_matches_model together contain a win, a loss, a
    time-limit end, a wall death and an attack on a dead target; every run has losses, shots, attacks on dead and on far
    targets, and every env of every run auto-reset."""
    totals = {name: model_run(name)[4] for name in CASES}
    print(totals)
    for name, tot in totals.items():
        assert all(tot[k] > 0 for k in ("losses", "shots", "dead_target_attacks", "far_target_attacks", "min_ends")), (name, tot)
    for k in ("wins", "losses", "truncations", "wall_deaths", "dead_target_attacks"):
        assert sum(tot[k] for tot in totals.values()) > 0, (k, totals)
    assert totals["2s3z"]["wins"] > 0 and totals["2s3z"]["wall_deaths"] > 0 and totals["5m_vs_6m"]["truncations"] > 0
    assert totals["5m_vs_6m"]["wall_deaths"] == 0  # walls_cause_death off


@pytest.mark.parametrize("real_obs", [False, True], ids=["plain", "real"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_model(dev, name, real_obs):
    p, seed, off, run, _total = model_run(name)
    E = CASES[name][1]
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, p.Na, dev)
    won = torch.empty(E, dtype=torch.uint8, device=dev)
    ro, term = _real(env, dev) if real_obs else (None, None)
    for t, (a, want, hst) in enumerate(run):
        if t == 0:
            env.step_into(st, 0, obs, is_reset=True)
            _check_obs(obs, want[0], "reset")
        else:
            env.step_into(st, t, obs, *tr, action=torch.from_numpy(a).to(dev), real_obs=ro, terminated=term, info_won=won)
            _check_obs(obs, want[0], f"t={t}")
            for nm, got, w in zip(TRANSITION, tr, want[1:6]):
                _eq(got, w, f"t={t} {nm}")
            _eq(won, want[6]["won"], f"t={t} info_won")
            if real_obs:
                _eq(ro["agents_view"], want[6]["real_view"], f"t={t} real_view")
                _eq(ro["action_mask"], want[6]["real_mask"], f"t={t} real_mask")
                _eq(term, want[6]["terminated"], f"t={t} terminated")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")


def test_golden_on_gpu(dev):
    """The kernel driven by the recorded actions of tests/golden/smax_2s3z.npz against the stored arrays."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "smax_2s3z.npz"))
    E, steps, seed, off = (int(v) for v in g["params"])
    p = m.scenario("2s3z")
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, p.Na, dev)
    won = torch.empty(E, dtype=torch.uint8, device=dev)
    ro, term = _real(env, dev)
    env.step_into(st, 0, obs, is_reset=True)
    for k in OBS:
        _eq(obs[k], g[f"reset_obs_{k}"], f"reset {k}")
    for k in STATE_FIELDS:
        _eq(getattr(st, k), g[f"reset_{k}"], f"reset {k}")
    kept = {int(t): n for n, t in enumerate(g["obs_steps"])}
    for t in range(steps):
        env.step_into(st, t + 1, obs, *tr, action=torch.from_numpy(g["action"][t]).to(dev), real_obs=ro, terminated=term,
                      info_won=won)
        for k in ("action_mask", "step_count"):
            _eq(obs[k], g[f"obs_{k}"][t], f"t={t} {k}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), g[k][t], f"t={t} {k}")
        for k, got in zip(TRANSITION, tr):
            _eq(got, g[k][t], f"t={t} {k}")
        _eq(won, g["won"][t], f"t={t} won")
        _eq(term, g["terminated"][t], f"t={t} terminated")
        _eq(ro["action_mask"], g["real_mask"][t], f"t={t} real_mask")
        if t in kept:
            _eq(ro["agents_view"], g["real_view"][kept[t]], f"t={t} real_view")
            for k in ("agents_view", "global_state"):
                _eq(obs[k], g[f"obs_{k}"][kept[t]], f"t={t} {k}")


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule_on_gpu(dev, case):
    _name, p, host, actions, t, expect = case
    env = _env(p, 1, dev, seed=m.SCRIPT_SEED)
    want = m.run_case(p, host, actions, t)
    for real_obs in (True, False):
        st, obs = env.alloc_state(), env.alloc_obs()
        _load_state(st, host)
        tr = _transition(1, p.Na, dev)
        won = torch.empty(1, dtype=torch.uint8, device=dev)
        ro, term = _real(env, dev) if real_obs else (None, None)
        results = []
        for n, action in enumerate(actions):
            env.step_into(st, t + n, obs, *tr, action=torch.from_numpy(action[None]).to(dev), real_obs=ro, terminated=term,
                          info_won=won)
            got = {"state": _host_state(st), "obs": {k: v.cpu().numpy() for k, v in obs.items()}, "won": won.cpu().numpy()}
            got.update({k: v.cpu().numpy() for k, v in zip(TRANSITION, tr)})
            if real_obs:
                got.update(real_view=ro["agents_view"].cpu().numpy(), real_mask=ro["action_mask"].cpu().numpy(),
                           terminated=term.cpu().numpy())
                for k in ("real_view", "real_mask", "terminated"):
                    _eq(got[k], want[n][k], f"step {n} {k}")
            _check_obs(obs, want[n]["obs"], f"step {n} obs")
            for k in TRANSITION + ("won",):
                _eq(got[k], want[n][k], f"step {n} {k}")
            for k in STATE_FIELDS:
                _eq(got["state"][k], want[n]["state"][k], f"step {n} {k}")
            results.append(got)
        if real_obs:
            expect(results)


def test_graph_replay_with_moving_t_base(dev):
    p = m.scenario("3m", time_limit=6)
    E, seed, off = 20, 7, 64
    env = _env(p, E, dev, seed=seed, env_offset=off)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, p.Na, dev)
    hst, hobs = m.reset(p, E, seed, off, 0)
    action = torch.zeros((E, p.Na), dtype=torch.int32, device=dev)
    t_base = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_into(st, 1, obs, *tr, t_base=t_base, action=action)
    # capture does not run the kernel: the state is still the reset state
    rng = np.random.default_rng(1)
    resets = np.zeros(E, np.int64)
    mask = hobs["action_mask"]
    for t in range(1, 21):
        a = m.mixed_actions(rng, mask)
        action.copy_(torch.from_numpy(a))
        t_base.fill_(t - 1)
        g.replay()
        torch.cuda.synchronize()
        want = m.step(p, hst, a, seed, off, t)
        mask = want[0]["action_mask"]
        _check_obs(obs, want[0], f"t={t}")
        for nm, got, w in zip(TRANSITION, tr, want[1:6]):
            _eq(got, w, f"t={t} {nm}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
        resets += want[5]
    assert (resets >= 1).all()  # every env auto-reset at least once inside the replayed graph


@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo", "rec_ippo", "rec_mappo"])
def test_learners_record_smax_trajectories(dev, system):
    """Two learn() calls (the feed-forward learner replays its captured rollout in the second): every recorded
    observation slot, reward, done flag and episode metric equals the model driven by the learner's own actions."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 32, 16  # E * A = 160 rows: a multiple of 32, as the recurrent path needs of every minibatch (so it takes one)
    M = 1 if system.startswith("rec") else 2
    cfg = compose(f"default_{system}", ["env=smax_native", "env/scenario=2s3z", f"arch.num_envs={E}", f"system.rollout_length={T}",
                                        "system.update_batch_size=2", "system.ppo_epochs=2", f"system.num_minibatches={M}",
                                        "env.kwargs.time_limit=12"])
    cfg.system.num_updates_per_eval = 1
    central = system.endswith("mappo")
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    assert len(L.reps) == 2 and L.reps[1].env.env_offset == E and L.Oa == 5 + 99 + 10 and L.Oc == (120 if central else 114)
    p = m.params_of(env)
    ends = 0
    for _call in range(2):
        before = [_host_state(rep.state) for rep in L.reps]
        t0 = L.t_global
        state = learn(state).learner_state
        torch.cuda.synchronize()
        for rep, hst in zip(L.reps, before):
            acts = rep.action.cpu().numpy()
            for t in range(T):
                want = m.step(p, hst, acts[t], env.seed, rep.env.env_offset, t0 + t + 1)
                _check_obs(rep.obs_slot(t + 1), want[0], f"{system} t={t}")
                _eq(rep.reward[t], want[1], f"{system} t={t} reward")
                _eq(rep.done[t], want[2], f"{system} t={t} done")
                _eq(rep.info_return[0, t], want[3], f"{system} t={t} info_return")
                _eq(rep.info_length[0, t], want[4], f"{system} t={t} info_length")
                _eq(rep.info_terminal[0, t], want[5], f"{system} t={t} info_terminal")
                ends += int(want[5].sum())
            for k in STATE_FIELDS:
                _eq(getattr(rep.state, k), hst[k], f"{system} end state {k}")
    assert ends > 0


def test_run_experiment_on_smax_logs_win_rate(dev):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import rec_mappo

    cfg = compose("default_rec_mappo", ["env=smax_native", "env/scenario=3m", "arch.num_envs=64", "system.rollout_length=16",
                                        "system.num_updates=4", "arch.num_evaluation=2", "arch.num_eval_episodes=32",
                                        "arch.num_absolute_metric_eval_episodes=64", "system.update_batch_size=1"])
    assert cfg.env.log_win_rate is True
    recs = []
    ret = rec_mappo.run_experiment(cfg, log=recs.append)
    evals = [r for r in recs if "eval_episode_return" in r]
    lo, hi = 0.0, 2.0  # every enemy's whole health plus the win bonus
    assert len(evals) == 2 and all(lo <= r["eval_episode_return"] <= hi for r in evals) and ret == evals[-1]["eval_episode_return"]
    assert all(np.isfinite(r["win_rate"]) and 0.0 <= r["win_rate"] <= 100.0 for r in evals)
    last = recs[-1]
    assert "absolute_episode_return" in last and lo <= last["absolute_episode_return"] <= hi
    assert np.isfinite(last["win_rate"]) and 0.0 <= last["win_rate"] <= 100.0


def test_rec_iql_on_smax(dev):
    """One rec_iql learn() call on SMAX: the replay buffer's stored next observation and terminal flag are the model's
    real_obs / terminated."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup

    cfg = compose("default_rec_iql", ["env=smax_native", "env/scenario=3m", "arch.num_envs=32", "system.sample_sequence_length=4",
                                      "system.min_buffer_size=4", "system.buffer_size=64", "env.kwargs.time_limit=6",
                                      "system.num_updates_per_eval=6"])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    p = m.params_of(env)
    E, A = 32, 3
    hst, hobs = m.reset(p, E, env.seed, env.env_offset, 0)
    for k in STATE_FIELDS:
        _eq(getattr(L.state, k), hst[k], f"learner reset {k}")
    learn(state)
    torch.cuda.synchronize()
    n_steps = len(L.debug["actions"])
    assert n_steps == 12 and L.n_added == n_steps
    n_end = 0
    prev_obs, prev_term = hobs, np.zeros(E, np.uint8)
    for k in range(n_steps):
        a = L.debug["actions"][k].cpu().numpy()
        want = m.step(p, hst, a, env.seed, env.env_offset, k + 1)
        _eq(L.buf.obs[0][:, k], prev_obs["agents_view"], f"step {k} obs")
        _eq(L.buf.action[:, k], a, f"step {k} action")
        _eq(L.buf.reward[:, k], want[1], f"step {k} reward")
        _eq(L.buf.next_obs[0][:, k], want[6]["real_view"], f"step {k} next_obs")
        _eq(L.buf.next_obs[1][:, k], want[6]["real_mask"], f"step {k} next mask")
        _eq(L.buf.terminal[:, k], np.repeat(prev_term[:, None], A, 1), f"step {k} terminal (of the step that produced obs)")
        prev_obs, prev_term = want[0], want[6]["terminated"]
        n_end += int(want[5].sum())
    _eq(L.term[L.cur], prev_term, "terminated flag of the last step")
    assert n_end >= E  # the time limit of 6 ended every env at least once
    for k in STATE_FIELDS:
        _eq(getattr(L.state, k), hst[k], f"end state {k}")


def test_ppo_learns_smax(dev):
    """One fixed-seed ff_mappo run on 3m: the mean eval return of the trained policy exceeds the untrained policy's.
    The configuration is tools/smax_bench.py's CURVE; the measured curve is profiles/smax_learning_curve.json, and this
    run writes its before / after return and win rate to profiles/smax_learning.json."""
    spec = importlib.util.spec_from_file_location("smax_bench", os.path.join(ROOT, "tools", "smax_bench.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    curve = sb.learning_curve(dev)
    before, after = curve[0], curve[-1]
    rec = {"config": sb.CURVE, "eval_return_before": before[2], "eval_return_after": after[2], "win_rate_before": before[3],
           "win_rate_after": after[3]}
    print(json.dumps(rec))
    try:
        with open(os.path.join(ROOT, "profiles", "smax_learning.json"), "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    except OSError:
        pass  # a read-only checkout still runs the check
    assert after[2] > before[2], curve
