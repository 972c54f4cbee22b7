"""GPU: Robot Warehouse (mava_rware_step, csrc/rware.hip) against the plain-Python rules of tests/rware_model.py, bit
for bit; captured-graph replay; the four PPO systems, run_experiment, rec_iql and learning on RWARE."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import rware_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = m.STATE_FIELDS
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")
# name: (scenario, sensor range, collision mode, with real_obs)
CASES = {"tiny-2ag": ("tiny-2ag", 1, "terminate", False), "tiny-2ag-real": ("tiny-2ag", 1, "overlap", True),
         "tiny-4ag-real": ("tiny-4ag", 1, "terminate", True), "tiny-4ag-easy-overlap": ("tiny-4ag-easy", 1, "overlap", False),
         "small-4ag-real": ("small-4ag", 1, "terminate", True), "tiny-4ag-s2": ("tiny-4ag", 2, "overlap", True),
         "small-4ag-s2": ("small-4ag", 2, "terminate", False)}
N_ENVS, N_STEPS, TIME_LIMIT, N_CRAFT = 403, 64, 12, 16


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import RobotWarehouse

    return RobotWarehouse(E, p.column_height, p.shelf_rows, p.shelf_columns, p.A, p.sensor_range, p.R, p.time_limit,
                          p.collision_mode, add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


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
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        _eq(obs[k], want[k], f"{what} {k}")


def _transition(E, A, dev):
    return (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
            torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))


def _real(env, dev):
    E, A = env.num_envs, env.num_agents
    return ({"agents_view": torch.empty((E, A, env.obs_dim), device=dev),
             "action_mask": torch.empty((E, A, 5), dtype=torch.uint8, device=dev)}, torch.empty(E, dtype=torch.uint8, device=dev))


def case_params(name: str) -> m.Params:
    scen, s, mode, _real_obs = CASES[name]
    ch, rows, cols, A, _, R = m.SCENARIOS[scen]
    return m.Params(ch, rows, cols, A, s, R, time_limit=TIME_LIMIT, collision_mode=mode)


def model_run(name: str, on_step=None, seed=0x5EED0000ABCD, off=12345):
    """The model's side of test_kernel_matches_model (no GPU): reset at t = 0, the first environments overwritten with
    crafted starts, then masked-random actions (one in ten drawn without the mask).  `on_step(t, state before, action,
    model result, state after)` sees every step; returns the summed event counts."""
    p = case_params(name)
    E = N_ENVS
    hst, hobs = m.reset(p, E, seed, off, 0)
    m.craft(p, hst, range(0, N_CRAFT), "deliver")
    m.craft(p, hst, range(N_CRAFT, 2 * N_CRAFT), "collide")
    hobs = m.observe(p, hst)
    if on_step:
        on_step(0, None, None, (hobs,), hst)
    rng = np.random.default_rng(3)
    total = {k: 0 for k in m.EVENTS}
    mask = hobs["action_mask"]
    for t in range(1, N_STEPS + 1):
        u = rng.random((E, p.A, 5)) * np.where(rng.random((E, p.A, 1)) < 0.1, 1.0, mask)
        a = u.argmax(-1).astype(np.int32)
        if t == 1:
            a[:N_CRAFT, 0] = m.FORWARD        # onto the goal
            a[N_CRAFT: 2 * N_CRAFT, :2] = m.FORWARD  # into each other
        want = m.step(p, hst, a, seed, off, t)
        mask = want[0]["action_mask"]
        for k in m.EVENTS:
            total[k] += want[6]["events"][k]
        if on_step:
            on_step(t, None, a, want, hst)
    return total


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_model(dev, name):
    real_obs = CASES[name][3]
    p = case_params(name)
    E, off, seed = N_ENVS, 12345, 0x5EED0000ABCD  # a ragged last workgroup; global env ids start at env_offset
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, p.A, dev)
    ro, term = _real(env, dev) if real_obs else (None, None)

    def on_step(t, _before, a, want, hst):
        if t == 0:
            env.step_into(st, 0, obs, is_reset=True)
            fresh, fobs = m.reset(p, E, seed, off, 0)
            _check_obs(obs, fobs, "reset")
            for k in STATE_FIELDS:
                _eq(getattr(st, k), fresh[k], f"reset {k}")
            _load_state(st, hst)  # the crafted starts
            return
        env.step_into(st, t, obs, *tr, action=torch.from_numpy(a).to(dev), real_obs=ro, terminated=term)
        _check_obs(obs, want[0], f"t={t}")
        for nm, got, w in zip(TRANSITION, tr, want[1:6]):
            _eq(got, w, f"t={t} {nm}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
        if real_obs:
            _eq(ro["agents_view"], want[6]["real_view"], f"t={t} real_view")
            _eq(ro["action_mask"], want[6]["real_mask"], f"t={t} real_mask")
            _eq(term, want[6]["terminated"], f"t={t} terminated")

    total = model_run(name, on_step, seed, off)
    # counted in the model's outputs only: every kind of event really happened
    assert all(total[k] > 0 for k in m.EVENTS), total


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule_on_gpu(dev, case):
    _name, p, host, action, t, expect = case
    env = _env(p, 1, dev, seed=m.SCRIPT_SEED)
    want = m.run_case(p, host, action, t)
    for real_obs in (True, False):
        st, obs = env.alloc_state(), env.alloc_obs()
        _load_state(st, host)
        tr = _transition(1, p.A, dev)
        ro, term = _real(env, dev) if real_obs else (None, None)
        env.step_into(st, t, obs, *tr, action=torch.from_numpy(action).to(dev), real_obs=ro, terminated=term)
        got = {"state": _host_state(st), "obs": {k: v.cpu().numpy() for k, v in obs.items()}}
        got.update({k: v.cpu().numpy() for k, v in zip(TRANSITION, tr)})
        if real_obs:
            got.update(real_view=ro["agents_view"].cpu().numpy(), real_mask=ro["action_mask"].cpu().numpy(),
                       terminated=term.cpu().numpy())
            expect(got)
            for k in ("real_view", "real_mask", "terminated"):
                _eq(got[k], want[k], k)
        _check_obs(obs, want["obs"], "obs")
        for k in TRANSITION:
            _eq(got[k], want[k], k)
        for k in STATE_FIELDS:
            _eq(got["state"][k], want["state"][k], k)


def test_graph_replay_with_moving_t_base(dev):
    p = m.Params(8, 1, 3, 2, 1, 2, time_limit=5)
    E, seed, off = 64, 7, 64
    env = _env(p, E, dev, seed=seed, env_offset=off)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, 2, dev)
    hst, _ = m.reset(p, E, seed, off, 0)
    action = torch.zeros((E, 2), dtype=torch.int32, device=dev)
    t_base = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_into(st, 1, obs, *tr, t_base=t_base, action=action)
    # capture does not run the kernel: the state is still the reset state
    rng = np.random.default_rng(1)
    resets = np.zeros(E, np.int64)
    for t in range(1, 31):
        a = rng.integers(0, 5, (E, 2)).astype(np.int32)
        action.copy_(torch.from_numpy(a))
        t_base.fill_(t - 1)
        g.replay()
        torch.cuda.synchronize()
        want = m.step(p, hst, a, seed, off, t)
        _check_obs(obs, want[0], f"t={t}")
        for nm, got, w in zip(TRANSITION, tr, want[1:6]):
            _eq(got, w, f"t={t} {nm}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
        resets += want[5]
    assert (resets >= 1).all()  # every env auto-reset at least once inside the replayed graph


@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo", "rec_ippo", "rec_mappo"])
def test_learners_record_rware_trajectories(dev, system):
    """Three learn() calls (the feed-forward learner replays its captured rollout from the second on): every recorded
    observation slot, reward, done flag and episode metric equals the model driven by the learner's own actions."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 64, 16
    cfg = compose(f"default_{system}", ["env=rware_native", "env/scenario=tiny-2ag", f"arch.num_envs={E}",
                                        f"system.rollout_length={T}", "system.update_batch_size=2", "system.ppo_epochs=2",
                                        "system.num_minibatches=2", "env.kwargs.time_limit=12"])
    cfg.system.num_updates_per_eval = 1
    central = system.endswith("mappo")
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    assert len(L.reps) == 2 and L.reps[1].env.env_offset == E
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


def test_run_experiment_on_rware(dev):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    cfg = compose("default_ff_mappo", ["env=rware_native", "env/scenario=tiny-4ag", "arch.num_envs=64",
                                       "system.rollout_length=16", "system.num_updates=6", "arch.num_evaluation=2",
                                       "arch.num_eval_episodes=32", "arch.num_absolute_metric_eval_episodes=64",
                                       "system.update_batch_size=1", "env.kwargs.time_limit=60"])
    recs = []
    ret = ff_mappo.run_experiment(cfg, log=recs.append)
    evals = [r["eval_episode_return"] for r in recs if "eval_episode_return" in r]
    assert len(evals) == 2 and all(v >= 0.0 and np.isfinite(v) for v in evals) and ret == evals[-1]
    assert "absolute_episode_return" in recs[-1] and recs[-1]["absolute_episode_return"] >= 0.0


def test_rec_iql_on_rware(dev):
    """rec_iql.run_experiment completes on the native env; and for a few act steps of its learner the replay buffer's
    stored next observation and terminal flag are the model's real_obs / terminated."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup
    from mava_amd.systems.q_learning import rec_iql

    small = ["env=rware_native", "env/scenario=tiny-2ag", "arch.num_envs=16", "system.sample_sequence_length=4",
             "system.min_buffer_size=4", "system.buffer_size=64", "env.kwargs.time_limit=6"]
    cfg = compose("default_rec_iql", small + ["system.total_timesteps=512", "arch.num_evaluation=2",
                                              "arch.num_eval_episodes=16", "arch.num_absolute_metric_eval_episodes=16"])
    recs = []
    ret = rec_iql.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    assert all(ev in events for ev in ("MISC", "TRAIN", "EVAL", "ABSOLUTE")) and np.isfinite(ret) and ret >= 0.0

    cfg = compose("default_rec_iql", small + ["system.num_updates_per_eval=6"])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    p = m.params_of(env)
    E, A = 16, 2
    hst, hobs = m.reset(p, E, env.seed, env.env_offset, 0)
    for k in STATE_FIELDS:
        _eq(getattr(L.state, k), hst[k], f"learner reset {k}")
    learn(state)
    torch.cuda.synchronize()
    n_steps = len(L.debug["actions"])
    assert n_steps == 12 and L.n_added == n_steps
    n_term = n_end = 0
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
        n_term += int(prev_term.sum())
        n_end += int(want[5].sum())
    _eq(L.term[L.cur], prev_term, "terminated flag of the last step")
    assert n_end >= E  # the time limit of 6 ended every env at least once (truncations: terminal stays 0 for those)
    for k in STATE_FIELDS:
        _eq(getattr(L.state, k), hst[k], f"end state {k}")


def test_ppo_learns_rware(dev):
    """One fixed-seed PPO run on Robot Warehouse: the mean eval return of the trained policy rises above the initial
    policy's by deliveries per episode.  The configuration and its measured curve are profiles/rware_learning_curve.json
    (tools/rware_bench.py --curve); the bar is under half the measured gain."""
    spec = importlib.util.spec_from_file_location("rware_bench", os.path.join(ROOT, "tools", "rware_bench.py"))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    with open(os.path.join(ROOT, "profiles", "rware_learning_curve.json")) as f:
        rec = json.load(f)
    assert rec["config"] == rb.CURVE
    measured = rec["measured_gain"]
    assert measured >= 1.0  # at least one delivery per episode more than the untrained policy: the run showed learning
    curve = rb.learning_curve(dev)
    got = rb.gain(curve)
    print(f"eval return {curve[0][2]:.3f} -> {got + curve[0][2]:.3f}, gain {got:.3f} (measured {measured:.3f})")
    assert got > 0.5 * measured, (curve, measured)
