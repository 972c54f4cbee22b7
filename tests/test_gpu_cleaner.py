"""GPU: Cleaner (mava_cleaner_step, csrc/cleaner.hip) against the NumPy rules of tests/cleaner_model.py, bit for bit;
the golden file; captured-graph replay; the four PPO systems on the flat and on the image observation, run_experiment
with its win rate, rec_iql and learning on Cleaner."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import cleaner_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = m.STATE_FIELDS
OBS = ("agents_view", "global_state", "action_mask", "step_count")
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")
# (R, C, A, E, time_limit): the smallest board with E no multiple of the four environments of a workgroup; a reference
# scenario at a short limit; even sizes and a rectangle; mixed parity; odd row length 675 in global_state; the maxima; a
# single agent on one row of rooms
CASES = {"3x3x2a": (3, 3, 2, 65, 8), "5x5x5a": (5, 5, 5, 37, 10), "4x6x3a": (4, 6, 3, 33, 9), "10x7x10a": (10, 7, 10, 9, 12),
         "15x15x15a": (15, 15, 15, 5, 6), "32x32x32a": (32, 32, 32, 3, 5), "3x32x1a": (3, 32, 1, 66, 7)}


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import Cleaner

    return Cleaner(E, p.R, p.C, p.A, p.time_limit, add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


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
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {bad[:3].tolist()}: got {got[tuple(bad[0])]} "
                             f"want {want[tuple(bad[0])]}")


def _check_obs(obs: dict, want: dict, what: str):
    for k in OBS:
        _eq(obs[k], want[k], f"{what} {k}")


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _real(env, dev):
    E, A = env.num_envs, env.num_agents
    return ({"agents_view": torch.empty((E, A, env.obs_dim), device=dev),
             "action_mask": torch.empty((E, A, 4), dtype=torch.uint8, device=dev)}, torch.empty(E, dtype=torch.uint8, device=dev))


def _actions(rng, mask, p_free=0.03):
    """Masked-random actions; each agent draws without the mask with probability p_free (walls, the board's edge)."""
    u = rng.random(mask.shape) * np.where(rng.random(mask.shape[:2] + (1,)) < p_free, 1.0, mask)
    return u.argmax(-1).astype(np.int32)


_MODEL_RUNS = {}


def model_run(name: str):
    """The model's side of test_kernel_matches_model, computed once per case and shared by its two variants: the reset
    at t = 0, then 3 * time_limit + 1 steps.  [(action, step result, state after)], the reset first."""
    if name not in _MODEL_RUNS:
        R, C, A, E, tl = CASES[name]
        p = m.Params(R, C, A, tl)
        seed, off = 0x5EED0000ABCD, 12345
        hst, hobs = m.reset(p, E, seed, off, 0)
        run = [(None, (hobs,), {k: v.copy() for k, v in hst.items()})]
        rng = np.random.default_rng(5)  # chosen on the model's event counts alone: 32x32x32a needs a truncation
        mask = hobs["action_mask"]
        total = {k: 0 for k in m.EVENTS}
        total["ends"] = 0
        for t in range(1, 3 * tl + 2):
            assert mask.any(-1).all()  # every agent always has a legal move
            a = _actions(rng, mask)
            want = m.step(p, hst, a, seed, off, t)
            mask = want[0]["action_mask"]
            for k in m.EVENTS:
                total[k] += want[6]["events"][k]
            total["ends"] += int(want[5].sum())
            run.append((a, want, {k: v.copy() for k, v in hst.items()}))
        _MODEL_RUNS[name] = (p, seed, off, run, total)
    return _MODEL_RUNS[name]


@pytest.mark.parametrize("real_obs", [False, True], ids=["plain", "real"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_model(dev, name, real_obs):
    p, seed, off, run, total = model_run(name)
    E = CASES[name][3]
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, p.A, dev)
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
    # counted in the model's outputs only: the run really exercised the rules, and every env reset
    assert all(total[k] > 0 for k in ("cleaned", "blocked", "invalid_ends", "truncations")) and total["ends"] >= E, total
    assert total["shared_cleans"] > 0 or p.A == 1, total
    assert total["wins"] > 0 or name != "3x3x2a", total


def test_unaligned_slots_take_the_scalar_ends(dev):
    """agents_view / global_state slots that start 4, 8 and 12 bytes past a 16-byte boundary."""
    p = m.Params(5, 7, 3, 6)
    E, seed, off = 9, 21, 7
    env = _env(p, E, dev, seed, off)
    for shift in (1, 2, 3):
        st, obs = env.alloc_state(), env.alloc_obs()
        for k in ("agents_view", "global_state"):
            flat = torch.full((obs[k].numel() + 8,), -7.0, device=dev)
            obs[k] = flat[shift:shift + obs[k].numel()].view(obs[k].shape)
            obs[k + "_store"] = flat
        env.step_into(st, 0, obs, is_reset=True)
        hst, hobs = m.reset(p, E, seed, off, 0)
        _check_obs(obs, hobs, f"shift {shift} reset")
        tr = _transition(E, p.A, dev)
        rng = np.random.default_rng(shift)
        for t in range(1, 8):
            a = _actions(rng, hobs["action_mask"], 0.1)
            env.step_into(st, t, obs, *tr, action=torch.from_numpy(a).to(dev))
            hobs = m.step(p, hst, a, seed, off, t)[0]
            _check_obs(obs, hobs, f"shift {shift} t={t}")
        for k in ("agents_view", "global_state"):  # nothing outside the slot was written
            flat, n = obs[k + "_store"].cpu().numpy(), obs[k].numel()
            assert (flat[:shift] == -7.0).all() and (flat[shift + n:] == -7.0).all()


def test_golden_on_gpu(dev):
    """The kernel driven by the recorded actions of tests/golden/cleaner_5x5x5a.npz against the stored arrays."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "cleaner_5x5x5a.npz"))
    R, C, A, tl, E, steps, seed, off = (int(v) for v in g["params"])
    env = _env(m.Params(R, C, A, tl), E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, A, dev)
    won = torch.empty(E, dtype=torch.uint8, device=dev)
    ro, term = _real(env, dev)
    env.step_into(st, 0, obs, is_reset=True)
    for k in OBS:
        _eq(obs[k], g[f"reset_obs_{k}"], f"reset {k}")
    for k in STATE_FIELDS:
        _eq(getattr(st, k), g[f"reset_{k}"], f"reset {k}")
    for t in range(steps):
        env.step_into(st, t + 1, obs, *tr, action=torch.from_numpy(g["action"][t]).to(dev), real_obs=ro, terminated=term,
                      info_won=won)
        for k in OBS:
            _eq(obs[k], g[f"obs_{k}"][t], f"t={t} {k}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), g[k][t], f"t={t} {k}")
        for k, got in zip(TRANSITION, tr):
            _eq(got, g[k][t], f"t={t} {k}")
        _eq(won, g["won"][t], f"t={t} won")
        _eq(term, g["terminated"][t], f"t={t} terminated")
        _eq(ro["agents_view"], g["real_view"][t], f"t={t} real_view")
        _eq(ro["action_mask"], g["real_mask"][t], f"t={t} real_mask")


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule_on_gpu(dev, case):
    _name, p, host, action, t, expect = case
    env = _env(p, 1, dev, seed=m.SCRIPT_SEED)
    want = m.run_case(p, host, action, t)
    for real_obs in (True, False):
        st, obs = env.alloc_state(), env.alloc_obs()
        _load_state(st, host)
        tr = _transition(1, p.A, dev)
        won = torch.empty(1, dtype=torch.uint8, device=dev)
        ro, term = _real(env, dev) if real_obs else (None, None)
        env.step_into(st, t, obs, *tr, action=torch.from_numpy(action[None]).to(dev), real_obs=ro, terminated=term, info_won=won)
        got = {"state": _host_state(st), "obs": {k: v.cpu().numpy() for k, v in obs.items()}, "won": won.cpu().numpy()}
        got.update({k: v.cpu().numpy() for k, v in zip(TRANSITION, tr)})
        if real_obs:
            got.update(real_view=ro["agents_view"].cpu().numpy(), real_mask=ro["action_mask"].cpu().numpy(),
                       terminated=term.cpu().numpy())
            expect(got)
            for k in ("real_view", "real_mask", "terminated"):
                _eq(got[k], want[k], k)
        _check_obs(obs, want["obs"], "obs")
        for k in TRANSITION + ("won",):
            _eq(got[k], want[k], k)
        for k in STATE_FIELDS:
            _eq(got["state"][k], want["state"][k], k)


def test_graph_replay_with_moving_t_base(dev):
    p = m.Params(5, 5, 3, time_limit=5)
    E, seed, off = 64, 7, 64
    env = _env(p, E, dev, seed=seed, env_offset=off)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, p.A, dev)
    hst, hobs = m.reset(p, E, seed, off, 0)
    action = torch.zeros((E, p.A), dtype=torch.int32, device=dev)
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
        a = _actions(rng, mask)
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


@pytest.mark.parametrize("image", [False, True], ids=["flat", "image"])
@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo", "rec_ippo", "rec_mappo"])
def test_learners_record_cleaner_trajectories(dev, system, image):
    """Three learn() calls (the feed-forward learner replays its captured rollout from the second on): every recorded
    observation slot, reward, done flag and episode metric equals the model driven by the learner's own actions.  Once on
    the flat observation (network=mlp / rnn, the fused kernels) and once on the image (network=cnn / rcnn)."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 64, 16  # E * A is a multiple of 32, as the general network path needs
    rec = system.startswith("rec")
    network = ("rcnn" if rec else "cnn") if image else ("rnn" if rec else "mlp")
    cfg = compose(f"default_{system}", ["env=cleaner", "env/scenario=clean-5x5x5a", f"network={network}", f"arch.num_envs={E}",
                                        f"system.rollout_length={T}", "system.update_batch_size=2", "system.ppo_epochs=2",
                                        "system.num_minibatches=2", "env.kwargs.time_limit=12"])
    cfg.system.num_updates_per_eval = 1
    central = system.endswith("mappo")
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    assert len(L.reps) == 2 and L.reps[1].env.env_offset == E and L.Oa == 100 and L.Oc == (75 if central else 100)
    p = m.params_of(env)
    ends = 0
    for _call in range(3):
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


def test_run_experiment_on_cleaner_logs_win_rate(dev):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    cfg = compose("default_ff_mappo", ["env=cleaner", "network=cnn", "arch.num_envs=64", "system.rollout_length=16",
                                       "system.num_updates=6", "arch.num_evaluation=2", "arch.num_eval_episodes=32",
                                       "arch.num_absolute_metric_eval_episodes=64", "system.update_batch_size=1"])
    assert cfg.env.log_win_rate is True
    recs = []
    ret = ff_mappo.run_experiment(cfg, log=recs.append)
    evals = [r for r in recs if "eval_episode_return" in r]
    # clean-5x5x5a: 2 * 3 * 3 - 1 = 17 open cells, 16 of them dirty after the reset, 25 steps at -0.5
    lo, hi = -0.5 * 25, 16 - 0.5
    assert len(evals) == 2 and all(lo <= r["eval_episode_return"] <= hi for r in evals) and ret == evals[-1]["eval_episode_return"]
    assert all(np.isfinite(r["win_rate"]) and 0.0 <= r["win_rate"] <= 100.0 for r in evals)
    last = recs[-1]
    assert "absolute_episode_return" in last and lo <= last["absolute_episode_return"] <= hi
    assert np.isfinite(last["win_rate"]) and 0.0 <= last["win_rate"] <= 100.0


def test_rec_iql_on_cleaner(dev):
    """rec_iql.run_experiment completes on Cleaner and reports a win rate; and for a few act steps of its learner the
    replay buffer's stored next observation and terminal flag are the model's real_obs / terminated."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup
    from mava_amd.systems.q_learning import rec_iql

    small = ["env=cleaner", "env/scenario=clean-5x5x5a", "arch.num_envs=16", "system.sample_sequence_length=4",
             "system.min_buffer_size=4", "system.buffer_size=64", "env.kwargs.time_limit=6"]
    cfg = compose("default_rec_iql", small + ["system.total_timesteps=512", "arch.num_evaluation=2",
                                              "arch.num_eval_episodes=16", "arch.num_absolute_metric_eval_episodes=16"])
    recs = []
    ret = rec_iql.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    assert all(ev in events for ev in ("MISC", "TRAIN", "EVAL", "ABSOLUTE")) and np.isfinite(ret) and -3.0 <= ret <= 15.5
    for r in recs:
        if r["event"] in ("EVAL", "ABSOLUTE"):
            assert "won_episode" not in r and np.isfinite(r["win_rate"]) and 0.0 <= r["win_rate"] <= 100.0

    cfg = compose("default_rec_iql", small + ["system.num_updates_per_eval=6"])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    p = m.params_of(env)
    E, A = 16, 5
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


def test_ppo_learns_cleaner(dev):
    """One fixed-seed PPO run on clean-5x5x5a: the mean eval return of the trained policy rises above the initial
    policy's by at least one extra tile per episode.  The configuration and its measured curve are
    profiles/cleaner_learning_curve.json (tools/cleaner_bench.py --curve); the bar is half the measured gain."""
    spec = importlib.util.spec_from_file_location("cleaner_bench", os.path.join(ROOT, "tools", "cleaner_bench.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    with open(os.path.join(ROOT, "profiles", "cleaner_learning_curve.json")) as f:
        rec = json.load(f)
    assert rec["config"] == cb.CURVE
    measured = rec["measured_gain"]
    assert measured >= 1.0  # one more tile per episode than the untrained policy: the run showed learning
    curve = cb.learning_curve(dev)
    got = cb.gain(curve)
    print(f"eval return {curve[0][2]:.3f} -> {got + curve[0][2]:.3f}, gain {got:.3f} (measured {measured:.3f})")
    assert got > 0.5 * measured, (curve, measured)
