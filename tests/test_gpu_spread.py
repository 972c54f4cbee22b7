"""GPU: Spread (mava_spread_step, csrc/spread.hip) against the NumPy rules of tests/spread_model.py, bit for bit, with
and without the agent id; captured-graph replay; and the PPO learners handing their continuous action to the env."""
import importlib

import numpy as np
import pytest
import torch

from tests import spread_model as m

pytestmark = pytest.mark.gpu

F = np.float32
STATE_FIELDS = m.STATE_FIELDS
OBS = ("agents_view", "global_state", "action_mask", "step_count")
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")
# (E, A): one ragged workgroup (32 envs each), a second workgroup of one env, a third of one env at the widest row
SHAPES = [(3, 2), (33, 5), (65, 8)]
STEPS = 60  # two auto-resets at time_limit = 25


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import Spread

    return Spread(E, p.A, p.time_limit, p.add_agent_id, add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


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


def mixed_actions(rng, st: dict, t: int) -> np.ndarray:
    """The fixed action mix of the kernel tests, by env e: uniform in [-1.5, 1.5], a third of it outside the action range
    (e % 4 == 0); everybody walks to landmark 0, which ends in collisions (1); everybody walks into the corner (1, -1),
    into the walls and each other (2); agent i walks to landmark i, with a large and an infinite component thrown in (3)."""
    E, A = st["agent_pos"].shape[:2]
    a = rng.uniform(-1.5, 1.5, (E, A, 2)).astype(F)
    e = np.arange(E)
    to_first = ((st["landmark_pos"][:, :1] - st["agent_pos"]) / m.STEP_SIZE).astype(F)
    a[e % 4 == 1] = to_first[e % 4 == 1]
    a[e % 4 == 2] = np.array([3.0, -3.0], F)
    own = m.scripted_actions(st)
    own[:, 0, 0] *= F(1e30)
    if t % 7 == 0:
        own[:, 0, 1] = F(-np.inf)
    a[e % 4 == 3] = own[e % 4 == 3]
    return a


_MODEL_RUNS = {}


def model_run(E: int, A: int, add_id: bool):
    """The model's side of test_kernel_matches_model, computed once per case and shared by its two variants: the reset
    at t = 0, then STEPS steps of the fixed action mix.  [(action, step result, state after)], the reset first."""
    key = (E, A, add_id)
    if key not in _MODEL_RUNS:
        p = m.Params(A, add_agent_id=add_id)
        seed, off = 17 + A, 12345
        hst, hobs = m.reset(p, E, seed, off, 0)
        run = [(None, (hobs,), {k: v.copy() for k, v in hst.items()})]
        rng = np.random.default_rng(5)
        tot = {"pairs": 0, "ends": np.zeros(E, np.int64), "walls": 0, "outside": 0}
        for t in range(1, STEPS + 1):
            a = mixed_actions(rng, hst, t)
            want = m.step(p, hst, a, seed, off, t)
            tot["pairs"] += int(want[6]["pairs"].sum())
            tot["ends"] += want[5]
            tot["outside"] += int((np.abs(a) > 1).sum())
            run.append((a, want, {k: v.copy() for k, v in hst.items()}))
            tot["walls"] += int((np.abs(hst["agent_pos"]) == 1).sum())
        _MODEL_RUNS[key] = (p, seed, off, run, tot)
    return _MODEL_RUNS[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"E{s[0]}xA{s[1]}")
def test_model_runs_cover_the_rules(shape):
    """Counted in the model's outputs alone: every run has collisions, agents at a wall, actions outside [-1, 1], and
    every env auto-reset twice."""
    tot = model_run(*shape, False)[4]
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in tot.items()})
    assert tot["pairs"] > 0 and tot["walls"] > 0 and tot["outside"] > 0 and (tot["ends"] == 2).all()


@pytest.mark.parametrize("real_obs", [False, True], ids=["plain", "real"])
@pytest.mark.parametrize("add_id", [False, True], ids=["noid", "id"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"E{s[0]}xA{s[1]}")
def test_kernel_matches_model(dev, shape, add_id, real_obs):
    E, A = shape
    p, seed, off, run, _tot = model_run(E, A, add_id)
    env = _env(p, E, dev, seed, off)
    assert env.obs_dim == p.obs_dim
    st, obs = env.alloc_state(), env.alloc_obs()
    tr = _transition(E, A, dev)
    ro, term = _real(env, dev) if real_obs else (None, None)
    truncations = 0
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
                _eq(term, np.zeros(E, np.uint8), f"t={t} terminated")
                if want[5].any():  # the truncation step: real_view holds the pre-reset observation
                    truncations += 1
                    assert not np.array_equal(want[6]["real_view"], want[0]["agents_view"])
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
    assert not real_obs or truncations == 2


def test_allocating_step_takes_the_float_action(dev):
    p = m.Params(3)
    E, seed = 5, 3
    env = _env(p, E, dev, seed)
    state, ts = env.reset()
    hst, hobs = m.reset(p, E, seed)
    _eq(ts.observation.agents_view, hobs["agents_view"], "reset view")
    rng = np.random.default_rng(0)
    for t in range(1, 27):
        a = m.uniform_actions(rng, E, 3, -1.2, 1.2)
        state, ts = env.step(state, torch.from_numpy(a).to(dev))
        want = m.step(p, hst, a, seed, 0, t)
        _eq(ts.observation.agents_view, want[0]["agents_view"], f"t={t} view")
        _eq(ts.reward, want[1], f"t={t} reward")
        _eq(ts.extras["episode_metrics"]["episode_return"], want[3], f"t={t} episode_return")
        assert ts.last().cpu().numpy().tolist() == want[5].astype(bool).tolist()


def test_graph_replay_with_moving_t_base(dev):
    p = m.Params(3, time_limit=6)
    E, seed, off = 40, 7, 64
    env = _env(p, E, dev, seed=seed, env_offset=off)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(E, p.A, dev)
    hst, _ = m.reset(p, E, seed, off, 0)
    action = torch.zeros((E, p.A, 2), device=dev)
    t_base = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_into(st, 1, obs, *tr, t_base=t_base, action=action)
    rng = np.random.default_rng(1)
    resets = np.zeros(E, np.int64)
    for t in range(1, 14):
        a = mixed_actions(rng, hst, t)
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
    assert (resets == 2).all()


def test_argument_errors(dev):
    from mava_amd._lib import MavaHipError

    env = _env(m.Params(2), 4, dev)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    tr = _transition(4, 2, dev)
    with pytest.raises(ValueError, match="float32"):
        env.step_into(st, 1, obs, *tr, action=torch.zeros((4, 2), dtype=torch.int32, device=dev))
    env.num_agents = 9  # past the kernel's bound: refused on the host, before any launch
    with pytest.raises(MavaHipError, match="bad shape"):
        env.step_into(st, 1, obs, *tr, action=torch.zeros((4, 9, 2), device=dev))


@pytest.mark.parametrize("system,network", [("ff_ippo", "continuous_mlp"), ("ff_mappo", "continuous_mlp"),
                                            ("rec_ippo", "rnn"), ("rec_mappo", "rnn")])
def test_ppo_learners_hand_the_action_to_the_env(dev, system, network):
    """Two learn() calls with a ContinuousActionHead on env=spread: the losses are finite, every recorded slot equals the
    model driven by the learner's own actions, and the agents have moved - a run fed zero actions keeps them where the
    reset put them (fewer steps than the time limit: no auto-reset in between)."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 32, 8  # E * A = 96 rows: a multiple of 32, as the recurrent path needs of every minibatch (so it takes one)
    M = 1 if system.startswith("rec") else 2
    cfg = compose(f"default_{system}", ["env=spread", f"network={network}", f"arch.num_envs={E}", f"system.rollout_length={T}",
                                        "system.update_batch_size=2", "system.ppo_epochs=2", f"system.num_minibatches={M}",
                                        "network.action_head._target_=mava.networks.ContinuousActionHead"])
    cfg.system.num_updates_per_eval = 1
    central = system.endswith("mappo")
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _net, state = mod.learner_setup(env, (42, 43, 44), cfg, device=dev)
    L = learn.learner
    assert L.continuous and len(L.reps) == 2
    p = m.params_of(env)
    assert p.add_agent_id and L.Oa == p.obs_dim
    start = [{k: getattr(rep.state, k).cpu().numpy().copy() for k in STATE_FIELDS} for rep in L.reps]
    for _call in range(2):
        before = [{k: getattr(rep.state, k).cpu().numpy().copy() for k in STATE_FIELDS} for rep in L.reps]
        t0 = L.t_global
        out = learn(state)
        state = out.learner_state
        torch.cuda.synchronize()
        for k, v in out.train_metrics.items():
            assert bool(torch.isfinite(torch.as_tensor(v)).all()), k
        for rep, hst in zip(L.reps, before):
            acts = rep.action.cpu().numpy()
            assert acts.shape == (T, E, p.A, 2) and acts.dtype == F and np.abs(acts).max() < 1
            for t in range(T):
                want = m.step(p, hst, acts[t], env.seed, rep.env.env_offset, t0 + t + 1)
                _check_obs(rep.obs_slot(t + 1), want[0], f"{system} t={t}")
                _eq(rep.reward[t], want[1], f"{system} t={t} reward")
                _eq(rep.done[t], want[2], f"{system} t={t} done")
            for k in STATE_FIELDS:
                _eq(getattr(rep.state, k), hst[k], f"{system} end state {k}")
    for rep, s0 in zip(L.reps, start):  # 16 steps < 25: the same episode; zero actions would have left agent_pos alone
        _eq(rep.state.landmark_pos, s0["landmark_pos"], "landmarks of the running episode")
        assert not (rep.state.agent_pos.cpu().numpy() == s0["agent_pos"]).all(-1).any()
