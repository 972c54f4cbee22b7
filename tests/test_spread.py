"""CPU: the Spread rules of tests/spread_model.py (the contract of mava_spread_step) on their own, and the configuration
surface of `env=spread`."""
import numpy as np
import pytest
import torch

from tests import spread_model as m

F = np.float32
CPU = torch.device("cpu")


def _state(p, agents, landmarks, step_count=0):
    st = m.alloc_state(p, 1)
    st["agent_pos"][0] = np.asarray(agents, F)
    st["landmark_pos"][0] = np.asarray(landmarks, F)
    st["step_count"][0] = step_count
    return st


def test_reset_is_a_function_of_seed_step_and_env_id():
    p = m.scenario("spread-5a")
    a, oa = m.reset(p, 6, seed=11, env_offset=3, t=17)
    b, ob = m.reset(p, 6, seed=11, env_offset=3, t=17)
    for k in m.STATE_FIELDS:
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(oa["agents_view"], ob["agents_view"])
    pos = np.concatenate([a["agent_pos"], a["landmark_pos"]], 1)
    assert pos.dtype == F and (pos >= -1).all() and (pos < 1).all() and len(np.unique(pos)) == pos.size
    # env id: env e of offset 3 is env e - 2 of offset 5
    c, _ = m.reset(p, 4, seed=11, env_offset=5, t=17)
    assert np.array_equal(c["agent_pos"], a["agent_pos"][2:]) and np.array_equal(c["landmark_pos"], a["landmark_pos"][2:])
    # seed and step each change every env
    for kw in (dict(seed=12, env_offset=3, t=17), dict(seed=11, env_offset=3, t=18)):
        d, _ = m.reset(p, 6, **kw)
        assert not (d["agent_pos"] == a["agent_pos"]).all(-1).all(-1).any()
    # the draws: agent i takes 2i, 2i + 1, landmark l takes 2A + 2l, 2A + 2l + 1
    w = m.draws(11, np.array([3], np.uint32), 17, 4 * p.A)[0]
    want = F(2) * ((w >> np.uint32(8)).astype(F) * F(2.0 ** -24)) - F(1)
    assert np.array_equal(a["agent_pos"][0].ravel(), want[:2 * p.A]) and np.array_equal(a["landmark_pos"][0].ravel(), want[2 * p.A:])


def test_step_is_deterministic_and_resets_at_the_steps_counter():
    p = m.scenario("spread-2a", time_limit=3)
    runs = []
    for _ in range(2):
        st, _ = m.reset(p, 5, seed=7, env_offset=2)
        rng = np.random.default_rng(3)
        out = [m.step(p, st, m.uniform_actions(rng, 5, 2, -1.5, 1.5), 7, 2, t) for t in range(1, 8)]
        runs.append((out, {k: v.copy() for k, v in st.items()}))
    for x, y in zip(runs[0][0], runs[1][0]):
        for k in x[0]:
            assert np.array_equal(x[0][k], y[0][k])
        assert all(np.array_equal(u, v) for u, v in zip(x[1:6], y[1:6]))
    # step 3 ends every env: the state is the reset of (seed, t = 3, env id)
    st, _ = m.reset(p, 5, seed=7, env_offset=2)
    for t in range(1, 4):
        obs, *_ = m.step(p, st, np.zeros((5, 2, 2), F), 7, 2, t)
    fresh, fobs = m.reset(p, 5, seed=7, env_offset=2, t=3)
    assert np.array_equal(st["agent_pos"], fresh["agent_pos"]) and np.array_equal(st["landmark_pos"], fresh["landmark_pos"])
    assert np.array_equal(obs["agents_view"], fobs["agents_view"]) and (obs["step_count"] == 0).all()


def test_actions_and_positions_are_clamped():
    p = m.Params(2)
    st = _state(p, [(0.95, -0.95), (0.0, 0.0)], [(0.5, 0.5), (-0.5, -0.5)])
    m.step(p, st, np.array([[(1.0, -1.0), (7.0, -0.25)]], F), 1, 0, 1)
    assert st["agent_pos"][0, 0].tolist() == [1.0, -1.0]  # the walls
    assert st["agent_pos"][0, 1].tolist() == [F(0.1) * F(1), F(0.1) * F(-0.25)]  # 7 counts as 1
    m.step(p, st, np.array([[(0.5, -0.5), (-np.inf, np.nan)]], F), 1, 0, 2)
    assert st["agent_pos"][0, 0].tolist() == [1.0, -1.0]
    assert st["agent_pos"][0, 1, 0] == F(0.1) * F(1) + F(0.1) * F(-1)
    assert st["agent_pos"][0, 1, 1] == F(0.1) * F(-0.25) + F(0.1) * F(-1)  # a NaN component counts as -1


def test_reward_by_hand_with_and_without_a_collision():
    p = m.Params(2)
    zero = np.zeros((1, 2, 2), F)
    # agents (0, 0) and (0.6, 0); landmarks (0, 0.3) and (1, 0): nearest 0.3 and 0.4, no pair within 0.15
    st = _state(p, [(0, 0), (0.6, 0)], [(0, 0.3), (1, 0)])
    _, reward, done, _, _, _, extra = m.step(p, st, zero, 1, 0, 1)
    d0, d1 = np.sqrt(F(0.3) * F(0.3)), np.sqrt((F(0.6) - F(1)) * (F(0.6) - F(1)))
    want = -((d0 + d1) * F(0.5))
    assert extra["pairs"].tolist() == [0] and reward.shape == (1, 2) and (reward == want).all()
    assert abs(float(want) + 0.35) < 1e-6 and not done.any()
    # agents (0, 0) and (0.1, 0): nearest 0.3 and 0.9, one pair at distance 0.1 -> a fine of 0.5 / 2
    st = _state(p, [(0, 0), (0.1, 0)], [(0, 0.3), (1, 0)])
    _, reward, _, _, _, _, extra = m.step(p, st, zero, 1, 0, 1)
    d1 = np.sqrt((F(0.1) - F(1)) * (F(0.1) - F(1)))
    want = -((d0 + d1) * F(0.5)) - (F(0.5) * F(1)) * F(0.5)
    assert extra["pairs"].tolist() == [1] and (reward == want).all() and abs(float(want) + 0.85) < 1e-6
    # the action moves first: agent 1 steps from 0.2 to 0.1 and collides
    st = _state(p, [(0, 0), (0.2, 0)], [(0, 0.3), (1, 0)])
    _, _, _, _, _, _, extra = m.step(p, st, np.array([[(0, 0), (-1, 0)]], F), 1, 0, 1)
    assert extra["pairs"].tolist() == [1]
    # three agents on one spot: three pairs
    p3 = m.Params(3)
    st = _state(p3, [(0, 0)] * 3, [(0, 0)] * 3)
    _, reward, _, _, _, _, extra = m.step(p3, st, np.zeros((1, 3, 2), F), 1, 0, 1)
    assert extra["pairs"].tolist() == [3] and (reward == -(F(1.5) * (F(1) / F(3)))).all()


def test_time_limit_truncates_and_never_terminates():
    p = m.Params(3)
    assert p.time_limit == 25
    st, _ = m.reset(p, 4, seed=2)
    total = np.zeros(4, F)
    for t in range(1, 26):
        obs, reward, done, ir, il, it, extra = m.step(p, st, np.zeros((4, 3, 2), F), 2, 0, t)
        total = total + reward[:, 0]
        assert not extra["terminated"].any() and extra["terminated"].dtype == np.uint8
        assert (done == (t == 25)).all() and (it == (t == 25)).all()
        assert (obs["step_count"] == (t % 25)).all()
    assert il.tolist() == [25] * 4 and np.array_equal(ir, total) and (st["run_length"] == 0).all()
    # the pre-reset view on the truncation step observes the state the rules produced, not the regenerated one
    assert not np.array_equal(extra["real_view"], obs["agents_view"])
    fresh, fobs = m.reset(p, 4, seed=2, t=25)
    assert np.array_equal(obs["agents_view"], fobs["agents_view"])


@pytest.mark.parametrize("add_id", [False, True])
def test_observation_layout(add_id):
    p = m.Params(3, add_agent_id=add_id)
    pos = np.array([(0.1, 0.2), (-0.3, 0.4), (0.5, -0.6)], F)
    land = np.array([(0.7, 0.7), (-0.8, 0.0), (0.0, 0.9)], F)
    obs = m.observe(p, _state(p, pos, land))
    w = 3 if add_id else 0
    assert p.obs_dim == w + 2 + 6 + 4 and obs["agents_view"].shape == (1, 3, p.obs_dim) and obs["agents_view"].dtype == F
    for i in range(3):
        row = obs["agents_view"][0, i]
        if add_id:
            assert row[:3].tolist() == np.eye(3)[i].tolist()
        assert np.array_equal(row[w:w + 2], pos[i])
        assert np.array_equal(row[w + 2:w + 8], (land - pos[i]).ravel())
        others = [j for j in range(3) if j != i]
        assert np.array_equal(row[w + 8:], (pos[others] - pos[i]).ravel())
    assert obs["global_state"].shape == (1, 1, 12)
    assert np.array_equal(obs["global_state"][0, 0], np.concatenate([pos.ravel(), land.ravel()]))
    assert obs["action_mask"].shape == (1, 3, 2) and obs["action_mask"].dtype == np.uint8 and obs["action_mask"].all()


def test_eval_and_train_streams_are_disjoint():
    from mava_amd.envs.base import EVAL_KEY_TAG

    p = m.Params(3)
    seed = 42
    train, _ = m.reset(p, 64, seed)
    evale, _ = m.reset(p, 64, seed ^ EVAL_KEY_TAG)
    both = np.concatenate([train["agent_pos"].ravel(), train["landmark_pos"].ravel(), evale["agent_pos"].ravel(),
                           evale["landmark_pos"].ravel()])
    # 24-bit draws: a shared stream would repeat all 768 values, chance repeats at most a few
    assert len(np.unique(both)) > both.size - 4


def test_the_scripted_policy_beats_random():
    p = m.Params(3)
    rand = m.mean_episode_return(p, lambda st, rng: m.uniform_actions(rng, st["agent_pos"].shape[0], p.A), 64, seed=1)
    walk = m.mean_episode_return(p, lambda st, rng: m.scripted_actions(st), 64, seed=1)
    assert walk > rand + 5.0, (rand, walk)


def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cfg = compose("default_ff_ippo", ["env=spread", "network=continuous_mlp"])
    assert cfg.env.env_name == "Spread" and cfg.env.log_win_rate is False and cfg.env.implicit_agent_id is False
    assert cfg.env.scenario.task_name == "spread-3a"
    for name, A in m.SCENARIOS.items():
        for add_id in (True, False):
            cfg = compose("default_ff_mappo", ["env=spread", "network=continuous_mlp", f"env/scenario={name}",
                                               f"system.add_agent_id={str(add_id).lower()}"])
            env, ev = envs.make(cfg, add_global_state=True, device=CPU)
            p = m.params_of(env)
            assert type(env) is envs.Spread and env.continuous_actions and env.emits_real_next_obs
            assert (p.A, p.time_limit, p.add_agent_id) == (A, 25, add_id)
            assert env.obs_dim == p.obs_dim and env.state_dim == p.state_dim and env.action_dim == 2
            spec = env.observation_spec()
            assert spec.agents_view == (A, p.obs_dim) and spec.action_mask == (A, 2) and spec.global_state == (A, 4 * A)
            assert ev.seed == env.seed ^ envs.base.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
    env, _ = envs.make(compose("default_ff_ippo", ["env=spread", "network=continuous_mlp", "env.kwargs.time_limit=9"]), device=CPU)
    assert env.time_limit == 9
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.time_limit, c.add_agent_id) == (8, 64, 9, env.add_agent_id)


def test_make_refuses_a_discrete_head_and_bad_shapes():
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.envs import Spread

    with pytest.raises(ValueError, match="continuous actions only"):
        envs.make(compose("default_ff_ippo", ["env=spread"]), device=CPU)  # network=mlp: a DiscreteActionHead
    for A in (1, 9):
        with pytest.raises(ValueError, match="num_agents"):
            Spread(4, num_agents=A, device=CPU)
        with pytest.raises(ValueError, match="num_agents"):
            m.Params(A)
    with pytest.raises(ValueError, match="time_limit"):
        Spread(4, time_limit=0, device=CPU)
    env = Spread(4, num_agents=2, device=CPU)
    with pytest.raises(ValueError, match="float32"):
        env._action_ptr(torch.zeros((4, 2), dtype=torch.int32), False)
    with pytest.raises(ValueError, match="float32"):
        env._action_ptr(torch.zeros((4, 2, 3)), False)
    assert env._action_ptr(None, True) is None and env._action_ptr(torch.zeros((4, 2, 2)), False) is not None


def test_spread_step_argument_errors_without_a_gpu():
    from mava_amd import _lib

    lib = _lib.lib()

    def call(is_reset=1, ptrs=True, trans=False, action=None, real=(None,) * 4, E=4, A=3, tl=25):
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        return lib.mava_spread_step(E, A, 1, tl, 1, 0, None, 0, is_reset, *([p] * 11), *([p if trans else None] * 5), action,
                                    *real, None)

    err = lib.mava_last_error
    assert call(A=9) <= -1000 and b"mava_spread_step: bad shape" in err()
    assert call(A=1) <= -1000 and call(E=-1) <= -1000
    assert call(tl=0) <= -1000 and b"time_limit" in err()
    assert call(E=2**24, A=8) <= -1000 and b"32-bit" in err()
    assert call(ptrs=False) <= -1000 and b"null state" in err()
    assert call(is_reset=0) <= -1000 and b"transition" in err()
    # real_view / real_mask / terminated: none of them on a step reaches the later checks, one or two are rejected (on a
    # reset too), real_state comes only with them, and none of the four may alias the observation
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in err() and b"real_view" not in err()
    assert call(A=9, real=(16, 16, 16, 16)) <= -1000 and b"mava_spread_step: bad shape" in err()
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        for state in (None, 16):
            assert call(is_reset=0, trans=True, action=16, real=(*part, state)) <= -1000 and b"real_view" in err()
            assert call(is_reset=1, real=(*part, state)) <= -1000 and b"real_view" in err()
    assert call(is_reset=0, trans=True, action=16, real=(None, None, None, 16)) <= -1000 and b"real_state only with them" in err()
    assert call(is_reset=1, real=(None, None, None, 16)) <= -1000 and b"real_state only with them" in err()
    assert call(is_reset=0, trans=True, action=16, real=(16, 16, 16, None)) <= -1000 and b"alias" in err()
    assert call(is_reset=0, trans=True, action=16, real=(32, 48, 64, 16)) <= -1000 and b"alias" in err()
    assert call(E=0) == 0  # nothing to do, nothing launched
