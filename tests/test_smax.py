"""CPU: the SMAX rules (tests/smax_model.py, the NumPy statement the kernel is checked against on the GPU by
tests/test_gpu_smax.py): hand-worked cases, rollout invariants, auto-reset, the golden file and learnability; the
`env=smax_native` configuration and dispatch (`env=smax` stays synthetic); what envs/base.py gives the Smax class (its
attributes, clone, shapes and the argument list of step_into against a recorder); the mava_smax_step argument checks,
which return before any launch."""
import os

import numpy as np
import pytest
import torch

from tests import smax_model as m

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smax_2s3z.npz")
CPU = torch.device("cpu")
SHAPES = {"3m": (3, 3), "2s3z": (5, 5), "3s5z": (8, 8), "3s5z_vs_3s6z": (8, 9), "5m_vs_6m": (5, 6), "10m_vs_11m": (10, 11),
          "3s_vs_5z": (3, 5), "6h_vs_8z": (6, 8)}


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule(case):
    _name, p, st, actions, t, expect = case
    expect(m.run_case(p, st, actions, t))


def test_unit_table_and_scenarios():
    assert m.HEALTH.tolist() == [45, 125, 160, 150, 35, 80] and m.DAMAGE.tolist() == [9, 10, 13, 8, 5, 12]
    assert m.RANGE.tolist() == [5, 6, 6, 2, 2, 5] and m.SIGHT.tolist() == [9, 10, 10, 9, 8, 9]
    assert m.COOLDOWN.tolist() == [10, 18, 30, 14, 8, 10]
    assert (m.STEP_LEN * m.F(16) == m.SPEED).all()  # speed / 16 is a power-of-two scaling: exact
    assert set(m.SCENARIOS) == set(SHAPES)
    for name, (na, ne) in SHAPES.items():
        p = m.scenario(name)
        assert (p.Na, p.Ne, p.n_actions, p.raw_obs_dim, p.state_dim) == (na, ne, 5 + ne, 11 * (na + ne - 1) + 10, 12 * (na + ne))
        assert p.time_limit == 100 and na <= m.MAX_SIDE and ne <= m.MAX_SIDE
    assert m.scenario("3s5z").ally_types == (2, 2, 2, 3, 3, 3, 3, 3)  # stalkers before zealots
    assert m.scenario("3s5z_vs_3s6z").enemy_types == (2,) * 3 + (3,) * 6 and m.scenario("6h_vs_8z").ally_types == (5,) * 6
    assert (m.scenario("3s5z").n_actions, m.scenario("3s5z_vs_3s6z").n_actions) == (13, 14)  # the project's shapes


def test_reset_positions_and_draws():
    p = m.scenario("5m_vs_6m")
    st, obs = m.reset(p, 7, seed=11, env_offset=3, t=17)
    x, y = st["pos"][..., 0], st["pos"][..., 1]
    assert (x[:, :5] >= 6).all() and (x[:, :5] < 10).all() and (x[:, 5:] >= 22).all() and (x[:, 5:] < 26).all()
    assert (y >= 14).all() and (y < 18).all() and (st["health"] == 45).all() and not st["cd"].any() and (st["last_action"] == 4).all()
    w = m.draws(11, [5], 17, 22)[0]  # env 2 is global env 5; unit j uses draws 2j and 2j + 1
    u = (w >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    assert st["pos"][2, 6, 0] == np.float32(22) + np.float32(4) * u[12] and st["pos"][2, 6, 1] == np.float32(14) + np.float32(4) * u[13]
    assert len({tuple(r) for r in st["pos"].reshape(7, -1)}) == 7  # the envs differ
    assert obs["agents_view"].shape == (7, 5, 5 + 11 * 10 + 10) and obs["global_state"].shape == (7, 1, 132)
    assert obs["action_mask"].shape == (7, 5, 11) and not obs["action_mask"][..., 5:].any() and obs["action_mask"][..., :5].all()


def _direct_view(p, st, e, i):
    """The agents_view row of ally i, written out float by float."""
    ty, f = p.types, np.float32
    row = [f(j == i) for j in range(p.Na)]
    pos, hp, cd, la = st["pos"][e], st["health"][e], st["cd"][e], st["last_action"][e]
    if hp[i] <= 0:
        return np.array(row + [0] * p.raw_obs_dim, f)
    for j in range(p.U):
        if j == i:
            continue
        dx, dy = pos[j, 0] - pos[i, 0], pos[j, 1] - pos[i, 1]
        if hp[j] <= 0 or dx * dx + dy * dy > m.SIGHT2[ty[i]]:
            row += [f(0)] * 11
            continue
        act = f(0) if (j >= p.Na and not p.see_enemy_actions) else f(la[j] + 1) * p.inv_act
        row += [hp[j] * m.INV_HEALTH[ty[j]], dx * m.INV_SIGHT[ty[i]], dy * m.INV_SIGHT[ty[i]], act, f(cd[j]) * m.INV_CD[ty[j]]]
        row += [f(ty[j] == k) for k in range(6)]
    row += [hp[i] * m.INV_HEALTH[ty[i]], pos[i, 0] / f(32), pos[i, 1] / f(32), f(cd[i]) * m.INV_CD[ty[i]]]
    row += [f(ty[i] == k) for k in range(6)]
    return np.array(row, f)


@pytest.mark.parametrize("see", [True, False], ids=["see-enemy-actions", "blind"])
def test_random_rollout_invariants(see):
    p = m.scenario("2s3z", see_enemy_actions=see)
    E = 12
    st, obs = m.reset(p, E, seed=5)
    rng = np.random.default_rng(0)
    total = {k: 0 for k in m.EVENTS}
    ended = np.zeros(E, bool)
    for t in range(1, 102):
        mask = obs["action_mask"]
        alive0, h0 = st["health"] > 0, st["health"].copy()
        assert (mask[..., 4] == 1).all() and (mask[..., :4] == alive0[:, :p.Na, None]).all()
        a = m.mixed_actions(rng, mask)
        obs, r, done, ir, il, it, extra = m.step(p, st, a, 5, 0, t)
        cont = it == 0
        assert (st["health"][cont] <= h0[cont]).all() and not ((st["health"] > 0) & ~alive0)[cont].any()  # the dead stay dead
        assert (st["health"] == np.round(st["health"])).all() and (st["health"] >= 0).all() and (st["cd"] >= 0).all()
        assert (st["pos"] >= 0).all() and (st["pos"] <= 32).all()
        assert (r[:, :1] == r).all() and (r >= 0).all() and (r <= 2).all()
        assert (extra["won"] <= it).all() and (extra["terminated"] <= it).all() and (extra["won"] <= extra["terminated"]).all()
        assert ((r[:, 0] >= 1) == (extra["won"] == 1)).all()  # the reference's won_episode: last & all(reward >= 1)
        assert (il[it == 1] <= 100).all() and (obs["step_count"][it == 1] == 0).all()
        # the mask's attack bits are alive & in range, a dead ally may only stop
        alive = st["health"] > 0
        for e in range(E):
            for i in range(p.Na):
                d2 = ((st["pos"][e, p.Na:] - st["pos"][e, i]) ** 2).sum(-1)
                want = alive[e, i] & alive[e, p.Na:] & (d2 <= m.RANGE2[p.types[i]])
                assert (obs["action_mask"][e, i, 5:] == want).all()
                if not alive[e, i]:
                    assert obs["action_mask"][e, i].tolist() == [0, 0, 0, 0, 1] + [0] * p.Ne
            if t % 10 == 0 or it[e]:
                for i in range(p.Na):
                    assert np.array_equal(obs["agents_view"][e, i], _direct_view(p, st, e, i)), (t, e, i)
                gs = obs["global_state"][e, 0].reshape(p.U, 12)
                assert not gs[~alive[e]].any() and (gs[alive[e], 10] == (np.arange(p.U) < p.Na)[alive[e]]).all()
                assert (gs[alive[e], 0] == (st["health"][e] * m.INV_HEALTH[p.types])[alive[e]]).all()
        ended |= it == 1
        for k in m.EVENTS:
            total[k] += extra["events"][k]
    assert ended.all()  # every episode ends by step 100
    assert all(total[k] > 0 for k in ("losses", "wall_deaths", "shots", "far_target_attacks")), total


def test_auto_reset_observation_and_real_obs():
    """A terminal step returns the observation of the environment regenerated at that step's counter; real_view keeps
    the view of the state the rules produced."""
    p = m.scenario("3m", time_limit=3)
    st, first = m.reset(p, 4, seed=7, env_offset=100)
    for t in (1, 2, 3):
        obs, _r, done, _ir, il, it, extra = m.step(p, st, np.full((4, 3), m.EAST, np.int32), 7, 100, t)
    assert done.all() and it.all() and (il == 3).all() and not extra["terminated"].any() and not extra["won"].any()
    _, want = m.reset(p, 4, seed=7, env_offset=100, t=3)
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], want[k]), k
    assert not np.array_equal(want["agents_view"], first["agents_view"])
    # the pre-reset view: the allies have walked east three steps (x / 32 in the own block)
    x_own = extra["real_view"][:, :, 3 + 11 * 5 + 1]
    assert (x_own * 32 > 6 + 3 * 8 * m.STEP_LEN[0] - 1e-3).all() and not np.array_equal(extra["real_view"], obs["agents_view"])


def test_model_reproduces_the_golden_file():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    E, steps, seed, off = (int(v) for v in g["params"])
    assert (E, steps) == (4, 120)
    p = m.scenario("2s3z")
    st, obs = m.reset(p, E, seed, off, 0)
    for k in m.STATE_FIELDS:
        assert np.array_equal(st[k], g[f"reset_{k}"]), k
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], g[f"reset_obs_{k}"]), k
    kept = {int(t): n for n, t in enumerate(g["obs_steps"])}
    for t in range(steps):
        out = m.step(p, st, g["action"][t], seed, off, t + 1)
        for k in m.STATE_FIELDS:
            assert np.array_equal(st[k], g[k][t]), (t, k)
        for k in ("action_mask", "step_count"):
            assert np.array_equal(out[0][k], g[f"obs_{k}"][t]), (t, k)
        for k, v in zip(("reward", "done", "info_return", "info_length", "info_terminal"), out[1:6]):
            assert np.array_equal(v, g[k][t]), (t, k)
        for k in ("won", "terminated", "real_mask"):
            assert np.array_equal(out[6][k], g[k][t]), (t, k)
        if t in kept:
            assert np.array_equal(out[6]["real_view"], g["real_view"][kept[t]]), t
            for k in ("agents_view", "global_state"):
                assert np.array_equal(out[0][k], g[f"obs_{k}"][kept[t]]), (t, k)
    assert (g["info_terminal"].sum(0) >= 1).all() and g["terminated"].sum() > 0 and len(kept) >= 5


def test_the_task_is_learnable():
    """3m, 64 episodes each: focusing fire on the lowest-index enemy in range (else walking east) wins strictly more
    often than uniform-random valid actions."""
    p = m.scenario("3m")

    def wins(policy):
        E = 64
        st, obs = m.reset(p, E, seed=3)
        rng = np.random.default_rng(0)
        won, ended = np.zeros(E, bool), np.zeros(E, bool)
        for t in range(1, 101):
            obs, _r, _d, _ir, _il, it, extra = m.step(p, st, policy(rng, obs["action_mask"]), 3, 0, t)
            first = (it == 1) & ~ended
            won[first] = extra["won"][first] == 1
            ended |= it == 1
        assert ended.all()
        return int(won.sum())

    scripted, rand = wins(lambda rng, mask: m.attack_else_east(mask)), wins(m.random_valid)
    print(f"wins of 64 episodes: scripted {scripted}, random {rand}")
    assert scripted > rand


# ---- the host side ----------------------------------------------------------------------------------------------------
def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cfg = compose("default_rec_mappo", ["env=smax_native"])
    assert cfg.env.env_name == "Smax" and cfg.env.native is True and cfg.env.log_win_rate is True
    assert cfg.env.eval_metric == "episode_return" and cfg.env.implicit_agent_id is False and cfg.env.scenario.task_name == "2s3z"
    assert dict(cfg.env.kwargs) == {"see_enemy_actions": True, "walls_cause_death": True, "attack_mode": "closest"}
    for name, (na, ne) in SHAPES.items():
        cfg = compose("default_ff_mappo", ["env=smax_native", f"env/scenario={name}"])
        assert cfg.env.scenario.name == "HeuristicEnemySMAX" and cfg.env.scenario.task_name == name
        assert dict(cfg.env.scenario.task_config) == {"num_agents": na, "num_enemies": ne}
        env, ev = envs.make(cfg, add_global_state=True, device=CPU)
        assert isinstance(env, envs.Smax) and (env.num_agents, env.num_enemies, env.time_limit) == (na, ne, 100)
        assert env.see_enemy_actions and env.walls_cause_death
        assert (env.obs_dim, env.state_dim, env.action_dim) == (na + 11 * (na + ne - 1) + 10, 12 * (na + ne), 5 + ne)
        assert m.params_of(env) == m.scenario(name) and m.params_of(env).obs_dim == env.obs_dim
        assert ev.seed == env.seed ^ envs.base.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
        assert env.observation_spec() == envs.base.ObsSpec((na, env.obs_dim), (na, 5 + ne), (na, env.state_dim), (na,))
    # `env=smax` is still the synthetic generator with SMAX's shape
    for scen in ("3s5z", "3s5z_vs_3s6z"):
        cfg = compose("default_rec_mappo", ["env=smax", f"env/scenario={scen}"])
        env, _ = envs.make(cfg, add_global_state=True, device=CPU)
        assert type(env) is envs.SyntheticRware and not cfg.env.get("native", False)
    env, _ = envs.make(compose("default_rec_ippo", ["env=smax_native", "env/scenario=5m_vs_6m", "env.kwargs.time_limit=9",
                                                   "env.kwargs.walls_cause_death=false", "env.kwargs.see_enemy_actions=false"]), device=CPU)
    assert (env.time_limit, env.walls_cause_death, env.see_enemy_actions) == (9, False, False)
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.obs_dim, c.seed, c.time_limit, c.walls_cause_death) == (8, 64, env.obs_dim, env.seed, 9, False)


def test_refused_scenarios_and_kwargs():
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.envs import Smax, smax

    for name in ("27m_vs_30m", "smacv2_5_units", "smacv2_10_units"):
        with pytest.raises(ValueError, match="out of scope"):
            smax.scenario_units(name)
    with pytest.raises(ValueError, match="unknown SMAX scenario"):
        smax.scenario_units("4q")
    with pytest.raises(ValueError, match="attack_mode"):
        envs.make(compose("default_ff_ippo", ["env=smax_native", "env.kwargs.attack_mode=random"]), device=CPU)
    with pytest.raises(ValueError, match="does not know"):
        envs.make(compose("default_ff_ippo", ["env=smax_native", "env.kwargs.num_obstacles=3"]), device=CPU)
    with pytest.raises(ValueError, match="agent one-hot id"):
        envs.make(compose("default_ff_ippo", ["env=smax_native", "system.add_agent_id=false"]), device=CPU)
    with pytest.raises(ValueError, match="discrete"):
        envs.make(compose("default_ff_ippo", ["env=smax_native", "network=continuous_mlp"]), device=CPU)
    ok = dict(num_envs=4, ally_types=(0, 0, 0), enemy_types=(0, 0, 0), device=CPU)
    Smax(**ok)
    Smax(**dict(ok, ally_types=(5,) * 16, enemy_types=(4,) * 16))
    for kw in (dict(ally_types=()), dict(enemy_types=()), dict(ally_types=(0,) * 17), dict(enemy_types=(0,) * 17),
               dict(ally_types=(0, 6)), dict(enemy_types=(-1,)), dict(time_limit=0), dict(attack_mode="random")):
        with pytest.raises(ValueError):
            Smax(**dict(ok, **kw))
    env = Smax(**ok)
    st, obs = env.alloc_state(), env.alloc_obs()
    with pytest.raises(ValueError, match="int32"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="go together"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int32), terminated=torch.zeros(4, dtype=torch.uint8))


def test_rec_iql_accepts_smax():
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    rec_iql._check_config(compose("default_rec_iql", ["env=smax_native"]))


E, STREAM = 4, 0x5157
PREFIX = ("step_count", "run_return", "run_length", "ep_return", "ep_length", "t")


def _make(**over):
    from mava_amd.envs import Smax

    kw = dict(num_envs=E, ally_types=(2, 3, 3), enemy_types=(0, 4), time_limit=30, see_enemy_actions=False, add_global_state=True,
              seed=11, env_offset=3, device=CPU)
    return Smax(**dict(kw, **over))


def test_attributes_clone_and_shapes():
    from mava_amd.envs import base

    env = _make()
    assert isinstance(env, base.BatchedEnv)
    want = dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=False, emits_real_next_obs=True, implicit_agent_id=False,
                reports_win=True)
    for k, v in want.items():
        assert getattr(env, k) == v, k
    assert not {"gs_tiles", "global_state_shared"} & set(vars(env))
    A, O, S, nA = 3, 3 + 11 * 4 + 10, 60, 7
    assert (env.num_agents, env.obs_dim, env.state_dim, env.action_dim) == (A, O, S, nA)
    assert env.observation_spec() == base.ObsSpec((A, O), (A, nA), (A, S), (A,))
    assert _make(add_global_state=False).observation_spec().global_state is None
    c = env.clone(7, 2)
    assert type(c) is type(env) and (c.env_offset, c.num_envs) == (7, 2) and (env.env_offset, env.num_envs) == (3, E)
    assert set(vars(c)) == set(vars(env))
    for k, v in vars(env).items():
        if k not in ("env_offset", "num_envs") and not isinstance(v, dict):
            assert getattr(c, k) == v, k
    assert env.clone(9).num_envs == E and c.clone(0).num_envs == 2
    obs = env.alloc_obs()
    shapes = {"agents_view": ((E, A, O), torch.float32), "global_state": ((E, 1, S), torch.float32),
              "action_mask": ((E, A, nA), torch.uint8), "step_count": ((E, A), torch.int32)}
    assert list(obs) == list(shapes)
    for k, (shape, dtype) in shapes.items():
        assert tuple(obs[k].shape) == shape and obs[k].dtype == dtype and obs[k].device == CPU, k
    st = env.alloc_state()
    assert type(st) is env.State and st._fields == PREFIX + ("pos", "health", "cd", "last_action")
    i32, f32 = torch.int32, torch.float32
    for f, shape, dtype in zip(st._fields, ((E, A), (E,), (E,), (E,), (E,), (), (E, 5, 2), (E, 5), (E, 5), (E, 5)),
                               (i32, f32, i32, f32, i32, torch.int64, f32, f32, i32, i32)):
        x = getattr(st, f)
        assert tuple(x.shape) == shape and x.dtype == dtype and not x.any(), f


class _Recorder:
    """Stands in for the library: every symbol it is asked for records its arguments and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        return lambda *args: self.calls.append((symbol, args)) or 0


def test_step_into_argument_list(monkeypatch):
    """Position by position in the order of include/mava_hip.h."""
    from mava_amd.envs import base

    rec = _Recorder()
    monkeypatch.setattr(base, "lib", lambda: rec)
    monkeypatch.setattr(base, "stream_ptr", lambda: STREAM)
    env = _make()
    st, obs, A = env.alloc_state(), env.alloc_obs(), 3
    tr = dict(reward=torch.empty((E, A)), done=torch.empty((E, A), dtype=torch.uint8), info_return=torch.empty(E),
              info_length=torch.empty(E, dtype=torch.int32), info_terminal=torch.empty(E, dtype=torch.uint8))
    real = dict(real_obs={"agents_view": torch.empty_like(obs["agents_view"]), "action_mask": torch.empty_like(obs["action_mask"])},
                terminated=torch.empty(E, dtype=torch.uint8))
    action, t_base, won = torch.zeros((E, A), dtype=torch.int32), torch.zeros((), dtype=torch.int32), torch.empty(E, dtype=torch.uint8)
    p = torch.Tensor.data_ptr
    # Ne = 2; allies stalker zealot zealot = nibbles 2 3 3; enemies marine zergling = 0 4; time limit 30; blind; walls kill
    scenario = [2, 0x332, 0x40, 30, 0, 1]

    def want(t, off, is_reset, tb=None, with_tr=True, with_real=False, info_won=None, act=None):
        trs = [p(tr[k]) if with_tr else None for k in ("reward", "done", "info_return", "info_length", "info_terminal")]
        return ([E, A] + scenario + [11, t, tb, off, is_reset] + [p(st.pos), p(st.health), p(st.cd), p(st.last_action)]
                + [p(st.step_count), p(st.run_return), p(st.run_length), p(st.ep_return), p(st.ep_length)]
                + [p(obs["agents_view"]), p(obs["global_state"]), p(obs["action_mask"]), p(obs["step_count"])] + trs
                + [info_won, act]
                + ([p(real["real_obs"]["agents_view"]), p(real["real_obs"]["action_mask"]), p(real["terminated"])] if with_real
                   else [None, None, None])
                + [STREAM])

    def last():
        symbol, args = rec.calls[-1]
        return symbol, list(args)

    name = "mava_smax_step"  # one entry point: the three real slots are always passed, None without real_obs
    env.step_into(st, 0, obs, is_reset=True, action=action)
    assert last() == (name, want(0, 3, 1, with_tr=False))
    env.step_into(st, 0, obs, is_reset=True, **real)
    assert last() == (name, want(0, 3, 1, with_tr=False, with_real=True))
    env.step_into(st, (1 << 32) + 7, obs, action=action, **tr)
    assert last() == (name, want(7, 3, 0, act=p(action)))
    env.step_into(st, 8, obs, tr["reward"], tr["done"], tr["info_return"], tr["info_length"], tr["info_terminal"], False, 21,
                  t_base, action, **real)
    assert last() == (name, want(8, 21, 0, tb=p(t_base), with_real=True, act=p(action)))
    env.step_into(st, 9, obs, action=action, info_won=won, **tr)
    assert last() == (name, want(9, 3, 0, info_won=p(won), act=p(action)))
    env.step_into(st, 9, obs, action=action, info_won=won, **tr, **real)
    assert last() == (name, want(9, 3, 0, with_real=True, info_won=p(won), act=p(action)))
    assert len(last()[1]) == len(__import__("mava_amd._lib", fromlist=["_SIGNATURES"])._SIGNATURES[name])
    ptrs = [a for a in last()[1] if isinstance(a, int) and a > (1 << 16)]
    assert len(set(ptrs)) == len(ptrs) >= 22  # every pointer of a call is a different one
    n = len(rec.calls)
    with pytest.raises(ValueError, match="Smax.step_into needs the .* int32"):
        env.step_into(st, 1, obs, **tr)
    assert len(rec.calls) == n
    # the allocating API goes through the same call and carries won_episode
    st2, ts = env.reset()
    assert rec.calls[-1][0] == name and rec.calls[-1][1][-5:-1] == (None,) * 4 and ts.extras["won_episode"].dtype == torch.bool
    st3, ts = env.step(st2, action.long())
    symbol, args = rec.calls[-1]
    i_t = 2 + len(scenario) + 1
    assert symbol == name and args[i_t] == 1 and args[i_t + 3] == 0 and int(st3.t) == 1 and args[-6] is not None
    assert args[-4:-1] == (None, None, None)
    assert ts.extras["won_episode"].dtype == torch.bool


def test_smax_step_argument_errors_without_a_gpu():
    from mava_amd import _lib

    lib = _lib.lib()
    ok = dict(E=4, A=3, Ne=4, at=0x000, et=0x3332, tl=100)

    def call(fn=lib.mava_smax_step, is_reset=1, ptrs=True, trans=False, action=None, extra=(None,) * 3, **kw):
        a = dict(ok, **kw)
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        return fn(a["E"], a["A"], a["Ne"], a["at"], a["et"], a["tl"], 1, 1, 1, 0, None, 0, is_reset, *([p] * 13),
                  *([p if trans else None] * 5), None, action, *extra, None)

    err = lib.mava_last_error
    assert call(A=17) <= -1000 and b"mava_smax_step: bad shape" in err()
    assert call(Ne=17) <= -1000 and call(A=0) <= -1000 and call(Ne=0) <= -1000 and call(E=-1) <= -1000
    assert call(tl=0) <= -1000 and b"time_limit" in err()
    assert call(at=0x060) <= -1000 and b"unit type" in err()
    assert call(et=0x7000) <= -1000 and call(E=0, et=0x70000) == call(E=0) == 0  # nibbles beyond Ne are not read; E = 0 launches nothing
    assert call(E=2**22, A=16, Ne=16, at=0, et=0) <= -1000 and b"32-bit" in err()
    assert call(ptrs=False) <= -1000 and b"null state" in err()
    assert call(is_reset=0) <= -1000 and b"transition" in err()
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in err()
    # real_view / real_mask / terminated: none of them on a step reaches the later checks (the line above), one or two are
    # rejected, all three must not alias the observation
    assert b"real_view" not in err()
    assert call(A=17, extra=(16, 16, 16)) <= -1000 and b"mava_smax_step: bad shape" in err()
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        assert call(is_reset=0, trans=True, action=16, extra=part) <= -1000 and b"real_view" in err()
        assert call(is_reset=1, extra=part) <= -1000 and b"real_view" in err()
    assert call(is_reset=0, trans=True, action=16, extra=(16, 16, 16)) <= -1000 and b"alias" in err()
