"""GPU: Connector (mava_connector_step, csrc/connector.hip) against the NumPy rules of tests/connector_model.py, bit for
bit; captured-graph replay; the four PPO systems on the flat and on the image observation, run_experiment, rec_iql and
learning on Connector."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import connector_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = m.STATE_FIELDS
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")
# (G, A, E, time_limit): E is no multiple of the four environments of a workgroup; 15 x 15 has odd row lengths (1125 and
# 675 floats); 16 x 16 x 32 are the maxima; 4 x 4 x 7 reaches the generator's no-candidate fallback
CASES = {"5x5x3a": (5, 3, 37, 8), "7x7x5a": (7, 5, 33, 9), "15x15x23a": (15, 23, 5, 6), "16x16x32a": (16, 32, 3, 5),
         "3x3x3a": (3, 3, 65, 6), "4x4x7a": (4, 7, 41, 5)}


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import Connector

    return Connector(E, p.G, p.A, p.time_limit, add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


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


def _actions(rng, mask):
    """Masked-random actions; one agent in five draws without the mask (walls, blocked cells, connected agents)."""
    u = rng.random(mask.shape) * np.where(rng.random(mask.shape[:2] + (1,)) < 0.2, 1.0, mask)
    return u.argmax(-1).astype(np.int32)


_MODEL_RUNS = {}


def model_run(name: str):
    """The model's side of test_kernel_matches_model, computed once per case and shared by its two variants: the reset
    at t = 0, then about three time limits of steps.  [(action, step result, state after)], the reset first."""
    if name not in _MODEL_RUNS:
        G, A, E, tl = CASES[name]
        p = m.Params(G, A, tl)
        seed, off = 0x5EED0000ABCD, 12345
        hst, hobs = m.reset(p, E, seed, off, 0)
        run = [(None, (hobs,), {k: v.copy() for k, v in hst.items()})]
        rng = np.random.default_rng(3)
        mask = hobs["action_mask"]
        total = {k: 0 for k in m.EVENTS}
        for t in range(1, 3 * tl + 2):
            a = _actions(rng, mask)
            want = m.step(p, hst, a, seed, off, t)
            mask = want[0]["action_mask"]
            for k in m.EVENTS:
                total[k] += want[6]["events"][k]
            run.append((a, want, {k: v.copy() for k, v in hst.items()}))
        _MODEL_RUNS[name] = (p, seed, off, run, total)
    return _MODEL_RUNS[name]


@pytest.mark.parametrize("real_obs", [False, True], ids=["plain", "real"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_model(dev, name, real_obs):
    p, seed, off, run, total = model_run(name)
    E = CASES[name][2]
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, p.A, dev)
    ro, term = _real(env, dev) if real_obs else (None, None)
    for t, (a, want, hst) in enumerate(run):
        if t == 0:
            env.step_into(st, 0, obs, is_reset=True)
            _check_obs(obs, want[0], "reset")
        else:
            env.step_into(st, t, obs, *tr, action=torch.from_numpy(a).to(dev), real_obs=ro, terminated=term)
            _check_obs(obs, want[0], f"t={t}")
            for nm, got, w in zip(TRANSITION, tr, want[1:6]):
                _eq(got, w, f"t={t} {nm}")
            if real_obs:
                _eq(ro["agents_view"], want[6]["real_view"], f"t={t} real_view")
                _eq(ro["action_mask"], want[6]["real_mask"], f"t={t} real_mask")
                _eq(term, want[6]["terminated"], f"t={t} terminated")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
    # counted in the model's outputs only: the run really exercised the rules, and every env reset
    assert total["moves"] > 0 and total["connections"] > 0 and total["truncations"] + total["terminations"] >= E, total
    assert total["contested"] > 0 or name == "16x16x32a", total
    assert total["fallbacks"] > 0 or name != "4x4x7a", total


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
        env.step_into(st, t, obs, *tr, action=torch.from_numpy(action[None]).to(dev), real_obs=ro, terminated=term)
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
    p = m.Params(5, 3, time_limit=5)
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
def test_learners_record_connector_trajectories(dev, system, image):
    """Three learn() calls (the feed-forward learner replays its captured rollout from the second on): every recorded
    observation slot, reward, done flag and episode metric equals the model driven by the learner's own actions.  Once on
    the flat observation (network=mlp / rnn, the fused kernels) and once on the image (network=cnn / rcnn)."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 64, 16  # E * A is a multiple of 32, as the general network path needs
    rec = system.startswith("rec")
    network = ("rcnn" if rec else "cnn") if image else ("rnn" if rec else "mlp")
    cfg = compose(f"default_{system}", ["env=connector", "env/scenario=con-5x5x3a", f"network={network}", f"arch.num_envs={E}",
                                        f"system.rollout_length={T}", "system.update_batch_size=2", "system.ppo_epochs=2",
                                        "system.num_minibatches=2", "env.kwargs.time_limit=12"])
    cfg.system.num_updates_per_eval = 1
    central = system.endswith("mappo")
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    assert len(L.reps) == 2 and L.reps[1].env.env_offset == E and L.Oa == 125 and L.Oc == (75 if central else 125)
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


def test_run_experiment_on_connector_with_cnn(dev):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    cfg = compose("default_ff_mappo", ["env=connector", "network=cnn", "arch.num_envs=64", "system.rollout_length=16",
                                       "system.num_updates=6", "arch.num_evaluation=2", "arch.num_eval_episodes=32",
                                       "arch.num_absolute_metric_eval_episodes=64", "system.update_batch_size=1"])
    recs = []
    ret = ff_mappo.run_experiment(cfg, log=recs.append)
    evals = [r["eval_episode_return"] for r in recs if "eval_episode_return" in r]
    # a Connector episode of con-5x5x3a returns between 25 steps x 3 agents x -0.03 and 3 connections
    assert len(evals) == 2 and all(-2.25 - 1e-4 <= v <= 3.0 and np.isfinite(v) for v in evals) and ret == evals[-1]
    assert "absolute_episode_return" in recs[-1] and -2.25 - 1e-4 <= recs[-1]["absolute_episode_return"] <= 3.0


def test_rec_iql_on_connector(dev):
    """rec_iql.run_experiment completes on Connector; and for a few act steps of its learner the replay buffer's stored
    next observation and terminal flag are the model's real_obs / terminated."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup
    from mava_amd.systems.q_learning import rec_iql

    small = ["env=connector", "env/scenario=con-5x5x3a", "arch.num_envs=16", "system.sample_sequence_length=4",
             "system.min_buffer_size=4", "system.buffer_size=64", "env.kwargs.time_limit=6"]
    cfg = compose("default_rec_iql", small + ["system.total_timesteps=512", "arch.num_evaluation=2",
                                              "arch.num_eval_episodes=16", "arch.num_absolute_metric_eval_episodes=16"])
    recs = []
    ret = rec_iql.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    assert all(ev in events for ev in ("MISC", "TRAIN", "EVAL", "ABSOLUTE")) and np.isfinite(ret) and -0.54 - 1e-4 <= ret <= 3.0

    cfg = compose("default_rec_iql", small + ["system.num_updates_per_eval=6"])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    p = m.params_of(env)
    E, A = 16, 3
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


def test_ppo_learns_connector(dev):
    """One fixed-seed PPO run on con-5x5x3a: the mean eval return of the trained policy rises above the initial policy's
    by at least one connection per episode.  The configuration and its measured curve are
    profiles/connector_learning_curve.json (tools/connector_bench.py --curve); the bar is half the measured gain."""
    spec = importlib.util.spec_from_file_location("connector_bench", os.path.join(ROOT, "tools", "connector_bench.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    with open(os.path.join(ROOT, "profiles", "connector_learning_curve.json")) as f:
        rec = json.load(f)
    assert rec["config"] == cb.CURVE
    measured = rec["measured_gain"]
    assert measured >= 1.0  # one more connection per episode than the untrained policy: the run showed learning
    curve = cb.learning_curve(dev)
    got = cb.gain(curve)
    print(f"eval return {curve[0][2]:.3f} -> {got + curve[0][2]:.3f}, gain {got:.3f} (measured {measured:.3f})")
    assert got > 0.5 * measured, (curve, measured)
