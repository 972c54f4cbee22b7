"""CPU: the Connector rules (tests/connector_model.py, the NumPy statement the kernel is checked against on the GPU by
tests/test_gpu_connector.py), the generator's and the rollout's invariants, the `env=connector` configuration and the
mava_connector_step argument checks, which return before any launch."""
import numpy as np
import pytest
import torch

from tests import connector_model as m

GENERATOR_CASES = {**{k: v[:2] for k, v in m.SCENARIOS.items()}, "max-16x16x32a": (16, 32), "min-3x3x3a": (3, 3)}


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule(case):
    _name, p, st, action, t, expect = case
    expect(m.run_case(p, st, action, t))


def test_team_reward_is_one_rounded_division():
    for c in range(4):
        for o in range(c, 33):
            r = m.team_reward(c, o)
            assert r.dtype == np.float32 and abs(float(r) - (c - 0.03 * o)) < 1e-6
    assert m.rel_table(3).tolist() == [0.0, np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), 1.0]


def _check_board(p, gen):
    heads, targets = [tuple(h) for h in gen["head"]], [tuple(t) for t in gen["target"]]
    assert len(set(heads + targets)) == 2 * p.A  # pairwise distinct cells, and head != target
    grid = gen["grid"]
    assert (grid > 0).sum() == 2 * p.A  # the grid holds exactly them
    for k in range(p.A):
        assert grid[heads[k]] == m.HEAD + 3 * k and grid[targets[k]] == m.TARGET + 3 * k
    seen = set()
    for k, w in enumerate(gen["walks"]):  # disjoint, 4-connected from head to target: the board is solvable
        assert w[0] == heads[k] and w[-1] == targets[k] and 2 <= len(w) <= p.lmax + 1
        assert not (set(w) & seen) and len(set(w)) == len(w)
        seen |= set(w)
        for a, b in zip(w, w[1:]):
            assert abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 or gen["fallbacks"]


@pytest.mark.parametrize("name", list(GENERATOR_CASES))
def test_generator_invariants(name):
    G, A = GENERATOR_CASES[name]
    p = m.Params(G, A)
    n = 300 if G < 15 else 40
    dr = m.draws(11, np.arange(n) + 3, 17, p.n_draws)
    lengths = set()
    for i in range(n):
        gen = m.generate(p, dr[i])
        assert gen["fallbacks"] == 0
        _check_board(p, gen)
        lengths |= {len(w) for w in gen["walks"]}
    assert len(lengths) > 1 or p.lmax == 1
    st, obs = m.reset(p, 3, seed=11, env_offset=3, t=17)  # reset() is generate() on those draws
    assert np.array_equal(st["grid"][2], m.generate(p, dr[2])["grid"]) and (st["connected"] == 0).all()
    assert obs["agents_view"].shape == (3, A, G * G * 5) and obs["global_state"].shape == (3, 1, G * G * 3)


def test_generator_fallback_without_a_candidate():
    """4 x 4 with 7 agents (Lmax 1: dominoes): after six dominoes the four empty cells can be pairwise apart, and then
    the seventh agent takes the first two empty cells in row-major order."""
    p = m.Params(4, 7)
    assert p.lmax == 1 and 2 * p.A <= p.G * p.G - 2
    dr = m.draws(11, np.arange(2000), 3, p.n_draws)
    hit = [m.generate(p, d) for d in dr]
    hit = [g for g in hit if g["fallbacks"]]
    assert hit
    for gen in hit:
        heads, targets = [tuple(h) for h in gen["head"]], [tuple(t) for t in gen["target"]]
        assert len(set(heads + targets)) == 14 and (gen["grid"] > 0).sum() == 14
        k = next(k for k, w in enumerate(gen["walks"]) if abs(w[0][0] - w[1][0]) + abs(w[0][1] - w[1][1]) != 1)
        before = {c for w in gen["walks"][:k] for c in w}
        empty = [(r, c) for r in range(4) for c in range(4) if (r, c) not in before]
        assert gen["walks"][k] == empty[:2]


def _direct_view(p, grid, j):
    """agents_view of agent j, one cell at a time."""
    out = np.zeros((p.G, p.G, 5), np.float32)
    for r in range(p.G):
        for c in range(p.G):
            v = int(grid[r, c])
            if v == 0:
                continue
            k, kind = (v - 1) // 3, (v - 1) % 3
            rel = np.float32(((k - j) % p.A) + 1) / np.float32(p.A)
            if kind == 1:
                out[r, c, 0] = rel
                out[r, c, 3] = k == j
            elif kind == 2:
                out[r, c, 1] = rel
                out[r, c, 4] = k == j
            else:
                out[r, c, 2] = 1
    return out


def test_random_rollout_invariants():
    p = m.Params(5, 3, time_limit=15)
    E = 24
    st, obs = m.reset(p, E, seed=5)
    rng = np.random.default_rng(0)
    total = {k: 0 for k in m.EVENTS}
    for t in range(1, 61):
        mask = obs["action_mask"]
        u = rng.random((E, p.A, 5)) * np.where(rng.random((E, p.A, 1)) < 0.2, 1.0, mask)
        a = u.argmax(-1).astype(np.int32)
        was_open = (st["connected"] == 0).sum(1)
        obs, r, done, ir, il, it, extra = m.step(p, st, a, 5, 0, t)
        assert (r[:, :1] == r).all() and (r <= 3).all() and (r >= -0.09 - 1e-6).all()
        assert ((r[:, 0] + 0.03 * was_open) > -1e-6).all()
        for e in range(E):
            grid, head, target, conn = st["grid"][e], st["head"][e], st["target"][e], st["connected"][e]
            for k in range(p.A):  # grid, head and connected stay consistent
                assert grid[tuple(head[k])] == m.HEAD + 3 * k and (grid == m.HEAD + 3 * k).sum() == 1
                assert bool(conn[k]) == (tuple(head[k]) == tuple(target[k]))
                assert (grid == m.TARGET + 3 * k).sum() == (0 if conn[k] else 1)
                if not conn[k]:
                    assert grid[tuple(target[k])] == m.TARGET + 3 * k
                for mv, (dr, dc) in m._MOVE.items():  # the mask is rule 1
                    rr, cc = head[k][0] + dr, head[k][1] + dc
                    ok = (not conn[k]) and 0 <= rr < p.G and 0 <= cc < p.G and grid[rr, cc] in (0, m.TARGET + 3 * k)
                    assert obs["action_mask"][e, k, mv] == ok
                assert obs["action_mask"][e, k, 0] == 1
                assert np.array_equal(obs["agents_view"][e, k].reshape(p.G, p.G, 5), _direct_view(p, grid, k))
            assert np.array_equal(obs["global_state"][e, 0].reshape(p.G, p.G, 3), _direct_view(p, grid, 0)[..., :3])
        assert (il[it == 1] <= 15).all() and (obs["step_count"][it == 1] == 0).all()
        for k in m.EVENTS:
            total[k] += extra["events"][k]
    assert all(total[k] > 0 for k in ("moves", "connections", "contested", "terminations", "truncations")), total


def test_auto_reset_observation_and_real_obs():
    """A terminal step returns the observation of the environment regenerated at that step's counter; real_view keeps
    the view of the state the rules produced."""
    p = m.Params(5, 3, time_limit=3)
    st, _ = m.reset(p, 4, seed=7, env_offset=100)
    noop = np.zeros((4, 3), np.int32)
    for t in (1, 2):
        before = m.step(p, st, noop, 7, 100, t)[0]
    obs, _r, done, _ir, il, it, extra = m.step(p, st, noop, 7, 100, 3)
    assert done.all() and it.all() and (il == 3).all() and not extra["terminated"].any()
    _, want_obs = m.reset(p, 4, seed=7, env_offset=100, t=3)
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], want_obs[k]), k
    assert not np.array_equal(want_obs["agents_view"], m.reset(p, 4, seed=7, env_offset=100, t=0)[1]["agents_view"])
    assert np.array_equal(extra["real_view"], before["agents_view"])  # nobody moved: the pre-reset view is the old one
    assert np.array_equal(extra["real_mask"], before["action_mask"])


def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cpu = torch.device("cpu")
    for name, (G, A, tl) in m.SCENARIOS.items():
        cfg = compose("default_ff_mappo", ["env=connector", f"env/scenario={name}", "network=cnn"])
        assert cfg.env.env_name == "MaConnector" and cfg.env.implicit_agent_id is True and cfg.env.log_win_rate is False
        assert cfg.env.kwargs == {} and cfg.env.eval_metric == "episode_return" and cfg.env.scenario.task_name == name
        assert cfg.env.scenario.env_kwargs.time_limit == tl
        env, ev = envs.make(cfg, add_global_state=True, device=cpu)
        assert isinstance(env, envs.Connector) and (env.grid_size, env.num_agents, env.time_limit) == (G, A, tl)
        assert env.obs_dim == G * G * 5 and env.state_dim == G * G * 3 and env.action_dim == 5
        assert env.obs_shape == (G, G, 5) and env.state_shape == (G, G, 3) and env.implicit_agent_id
        assert env.gs_tiles == 1 and env.global_state_shared and not env.supports_fused_rollout and env.emits_real_next_obs
        assert ev.seed == env.seed ^ envs.synthetic_rware.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
        spec = env.observation_spec()
        assert spec[0] == (A, G * G * 5) and spec[1] == (A, 5) and spec[2] == (A, G * G * 3)
        assert m.params_of(env) == m.Params(G, A, tl)
    assert compose("default_rec_ippo", ["env=connector"]).env.scenario.task_name == "con-5x5x3a"
    rc = compose("default_rec_mappo", ["env=connector", "network=rcnn"]).network
    assert "CNNTorso" in rc.actor_network.pre_torso._target_ and "MLPTorso" in rc.critic_network.post_torso._target_
    # system.add_agent_id is ignored (implicit ids), env.kwargs.time_limit overrides the scenario's
    env, _ = envs.make(compose("default_ff_ippo", ["env=connector", "system.add_agent_id=false", "env.kwargs.time_limit=9"]),
                       device=cpu)
    assert env.obs_dim == 125 and env.time_limit == 9
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.obs_dim, c.seed, c.time_limit, c.obs_shape) == (8, 64, 125, env.seed, 9, (5, 5, 5))
    with pytest.raises(ValueError, match="discrete"):
        envs.make(compose("default_ff_ippo", ["env=connector", "network=continuous_mlp"]), device=cpu)


def test_rec_iql_accepts_connector():
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    rec_iql._check_config(compose("default_rec_iql", ["env=connector"]))
    for name in ("rware", "smax"):
        with pytest.raises(ValueError, match="pre-reset observation"):
            rec_iql._check_config(compose("default_rec_iql", [f"env={name}"]))


def test_bad_scenarios_are_refused():
    from mava_amd.envs import Connector

    cpu = torch.device("cpu")
    ok = dict(num_envs=4, grid_size=5, num_agents=3, device=cpu)
    Connector(**ok)
    Connector(**dict(ok, grid_size=16, num_agents=32))
    Connector(**dict(ok, grid_size=3, num_agents=3))
    for kw in (dict(grid_size=2, num_agents=1), dict(grid_size=17), dict(num_agents=0), dict(grid_size=16, num_agents=33),
               dict(grid_size=3, num_agents=4), dict(num_agents=12), dict(time_limit=0)):
        with pytest.raises(ValueError):
            Connector(**dict(ok, **kw))
    env = Connector(**ok)
    st, obs = env.alloc_state(), env.alloc_obs()
    with pytest.raises(ValueError, match="int32"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="go together"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int32), terminated=torch.zeros(4, dtype=torch.uint8))


def test_connector_step_argument_errors_without_a_gpu():
    from mava_amd import _lib

    lib = _lib.lib()
    ok = dict(E=4, A=3, G=5, tl=25)

    def call(fn=lib.mava_connector_step, is_reset=1, ptrs=True, trans=False, action=None, extra=(None,) * 3, **kw):
        a = dict(ok, **kw)
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        return fn(a["E"], a["A"], a["G"], a["tl"], 1, 0, None, 0, is_reset, *([p] * 13), *([p if trans else None] * 5),
                  action, *extra, None)

    err = lib.mava_last_error
    assert call(A=33) <= -1000 and b"mava_connector_step: bad shape" in err()
    assert call(G=17) <= -1000 and call(G=2, A=1) <= -1000 and call(A=0) <= -1000 and call(E=-1) <= -1000
    assert call(A=12) <= -1000 and b"bad scenario" in err()
    assert call(G=3, A=4) <= -1000 and call(tl=0) <= -1000 and b"time_limit" in err()
    assert call(ptrs=False) <= -1000 and b"null state" in err()
    assert call(is_reset=0) <= -1000 and b"transition" in err()
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in err()
    # real_view / real_mask / terminated: none of them on a step reaches the later checks (the line above), one or two are
    # rejected, all three must not alias the observation
    assert b"real_view" not in err()
    assert call(A=33, extra=(16, 16, 16)) <= -1000 and b"mava_connector_step: bad shape" in err()
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        assert call(is_reset=0, trans=True, action=16, extra=part) <= -1000 and b"real_view" in err()
        assert call(is_reset=1, extra=part) <= -1000 and b"real_view" in err()
    assert call(is_reset=0, trans=True, action=16, extra=(16, 16, 16)) <= -1000 and b"alias" in err()
    assert call(E=0) == 0  # nothing to do, nothing launched
