"""GPU: Level-Based Foraging (mava_lbf_step, csrc/lbf.hip) against the NumPy rules of tests/lbf_model.py, bit for bit;
captured-graph replay; the four PPO systems, run_experiment and learning on LBF."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import lbf_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = ("agent_pos", "agent_level", "food_pos", "food_level", "food_alive", "total_food_level", "step_count",
                "run_return", "run_length", "ep_return", "ep_length")
SCEN = {"2s-8x8-2p-2f-coop": (8, 2, 2, 2, 2, True), "10x10-3p-3f": (10, 10, 3, 3, 2, False),
        "15x15-4p-5f": (15, 15, 4, 5, 2, False)}


def _env(p: m.Params, E: int, dev, seed=99, env_offset=0):
    from mava_amd.envs import LevelBasedForaging

    return LevelBasedForaging(E, p.G, p.fov, p.A, p.F, p.max_level, p.force_coop, p.time_limit, p.individual,
                              add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


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


@pytest.mark.parametrize("scenario", list(SCEN))
def test_kernel_matches_model(dev, scenario):
    G, fov, A, F, ml, coop = SCEN[scenario]
    p = m.Params(G, fov, A, F, ml, coop, time_limit=20)
    E, off, seed = 1000, 12345, 0x5EED0000ABCD  # a ragged last workgroup; global env ids start at env_offset
    env = _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    hst, hobs = m.reset(p, E, seed, off, 0)
    _check_obs(obs, hobs, "reset")
    for k in STATE_FIELDS:
        _eq(getattr(st, k), hst[k], f"reset {k}")
    rng = np.random.default_rng(3)
    rew = torch.empty((E, A), device=dev)
    done = torch.empty((E, A), dtype=torch.uint8, device=dev)
    ir, il, it = torch.empty(E, device=dev), torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)
    n_term = n_eat = 0
    for t in range(1, 301):
        a = rng.integers(0, 6, (E, A)).astype(np.int32)  # masked-invalid actions included
        env.step_into(st, t, obs, rew, done, ir, il, it, action=torch.from_numpy(a).to(dev))
        want = m.step(p, hst, a, seed, off, t)
        _check_obs(obs, want[0], f"t={t}")
        for name, got, w in zip(("reward", "done", "info_return", "info_length", "info_terminal"), (rew, done, ir, il, it), want[1:]):
            _eq(got, w, f"t={t} {name}")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), hst[k], f"t={t} {k}")
        n_term += int(want[5].sum())
        n_eat += int((want[1] > 0).any(-1).sum())
    assert n_term > E and n_eat > 0  # resets and eating really happened


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule_on_gpu(dev, case):
    _name, p, host, action, t, expect = case
    env = _env(p, 1, dev, seed=m.SCRIPT_SEED)
    st, obs = env.alloc_state(), env.alloc_obs()
    _load_state(st, host)
    rew = torch.empty((1, p.A), device=dev)
    done = torch.empty((1, p.A), dtype=torch.uint8, device=dev)
    ir, il, it = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.uint8, device=dev)
    env.step_into(st, t, obs, rew, done, ir, il, it, action=torch.from_numpy(action).to(dev))
    got = {"state": _host_state(st), "obs": {k: v.cpu().numpy() for k, v in obs.items()}, "reward": rew.cpu().numpy(),
           "done": done.cpu().numpy(), "info_return": ir.cpu().numpy(), "info_length": il.cpu().numpy(),
           "info_terminal": it.cpu().numpy()}
    expect(got)
    want = m.run_case(p, host, action, t)
    _check_obs(obs, want["obs"], "obs")
    for k in ("reward", "done", "info_return", "info_length", "info_terminal"):
        _eq(got[k], want[k], k)
    for k in STATE_FIELDS:
        _eq(got["state"][k], want["state"][k], k)


def test_graph_replay_with_moving_t_base(dev):
    p = m.Params(8, 2, 2, 2, 2, False, time_limit=5)
    E = 64
    env = _env(p, E, dev, seed=7, env_offset=64)
    bufs = []
    for _ in range(2):
        st, obs = env.alloc_state(), env.alloc_obs()
        env.step_into(st, 0, obs, is_reset=True)
        tr = (torch.empty((E, 2), device=dev), torch.empty((E, 2), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
              torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
        bufs.append((st, obs, tr))
    (gs, gobs, gtr), (es, eobs, etr) = bufs
    action = torch.zeros((E, 2), dtype=torch.int32, device=dev)
    t_base = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_into(gs, 1, gobs, *gtr, t_base=t_base, action=action)
    # capture does not run the kernel: both copies are still at the reset state
    rng = np.random.default_rng(1)
    resets = 0
    for t in range(1, 41):
        action.copy_(torch.from_numpy(rng.integers(0, 6, (E, 2)).astype(np.int32)))
        t_base.fill_(t - 1)
        g.replay()
        env.step_into(es, t, eobs, *etr, action=action)
        torch.cuda.synchronize()
        for k in gobs:
            _eq(gobs[k], eobs[k].cpu().numpy(), f"t={t} {k}")
        for a_, b_ in zip(gtr, etr):
            _eq(a_, b_.cpu().numpy(), f"t={t} transition")
        for k in STATE_FIELDS:
            _eq(getattr(gs, k), getattr(es, k).cpu().numpy(), f"t={t} {k}")
        resets += int(etr[4].sum())
    assert resets >= E  # every env auto-reset at least once inside the replayed graph


@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo", "rec_ippo", "rec_mappo"])
def test_learners_record_lbf_trajectories(dev, system):
    """Three learn() calls (the feed-forward learner replays its captured rollout from the second on): every recorded
    observation slot, reward, done flag and episode metric equals the NumPy rules driven by the learner's own actions."""
    from mava_amd import envs
    from mava_amd.config import compose

    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    E, T = 64, 16
    cfg = compose(f"default_{system}", ["env=lbf", "env/scenario=2s-8x8-2p-2f-coop", f"arch.num_envs={E}",
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


def test_run_experiment_on_lbf(dev):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    cfg = compose("default_ff_mappo", ["env=lbf", "env/scenario=2s-10x10-3p-3f", "arch.num_envs=64",
                                       "system.rollout_length=16", "system.num_updates=6", "arch.num_evaluation=2",
                                       "arch.num_eval_episodes=32", "arch.num_absolute_metric_eval_episodes=64",
                                       "system.update_batch_size=1"])
    recs = []
    ret = ff_mappo.run_experiment(cfg, log=recs.append)
    evals = [r["eval_episode_return"] for r in recs if "eval_episode_return" in r]
    assert len(evals) == 2 and all(0.0 <= v <= 1.0 for v in evals) and ret == evals[-1]
    assert "absolute_episode_return" in recs[-1] and 0.0 <= recs[-1]["absolute_episode_return"] <= 1.0


def test_ff_ippo_learns_lbf(dev):
    """ff_ippo on 10x10-3p-3f (no forced cooperation): the mean eval return of the trained policy rises well above the
    initial policy's.  The curve of this exact configuration is in profiles/lbf_learning_curve.json."""
    spec = importlib.util.spec_from_file_location("lbf_bench", os.path.join(ROOT, "tools", "lbf_bench.py"))
    lb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lb)
    curve = lb.learning_curve(dev)
    ev0 = curve[0][2]
    last = float(np.mean([c[2] for c in curve[-3:]]))
    # measured: 0.157 -> 0.95 (mean of the last three evaluations) in 300 updates; the bar is under half that gain
    assert ev0 < 0.3 and last > ev0 + 0.3, curve
