"""CPU: the Cleaner rules (tests/cleaner_model.py, the NumPy statement the kernel is checked against on the GPU by
tests/test_gpu_cleaner.py), the maze generator's and the rollout's invariants, the golden file, the `env=cleaner`
configuration, the evaluator's win rate and the mava_cleaner_step argument checks, which return before any launch."""
import os

import numpy as np
import pytest
import torch

from tests import cleaner_model as m

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cleaner_5x5x5a.npz")
# (R, C): the shapes of tests/test_gpu_cleaner.py and the reference's scenarios
MAZE_CASES = {"3x3": (3, 3), "5x5": (5, 5), "4x6": (4, 6), "10x7": (10, 7), "15x15": (15, 15), "32x32": (32, 32), "3x32": (3, 32),
              "10x10": (10, 10), "20x20": (20, 20), "30x30": (30, 30), "32x3": (32, 3)}


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule(case):
    _name, p, st, action, t, expect = case
    expect(m.run_case(p, st, action, t))


def _flood(grid):
    """The open cells reachable from (0, 0)."""
    R, C = grid.shape
    seen, todo = {(0, 0)}, [(0, 0)]
    while todo:
        r, c = todo.pop()
        for dr, dc in m._MOVE.values():
            n = (r + dr, c + dc)
            if 0 <= n[0] < R and 0 <= n[1] < C and grid[n] != m.WALL and n not in seen:
                seen.add(n)
                todo.append(n)
    return seen


@pytest.mark.parametrize("name", list(MAZE_CASES))
def test_maze_properties(name):
    R, C = MAZE_CASES[name]
    p = m.Params(R, C, 2)
    n_env = 12 if R * C > 400 else 40
    trees = set()
    for t in (0, 1, 17, 2**32 - 1):
        dr = m.draws(11, np.arange(n_env) + 3, t, p.n_draws)
        for i in range(n_env):
            gen = m.generate(p, dr[i])
            grid = gen["grid"]
            assert (grid[0::2, 0::2] != m.WALL).all()  # even / even cells are never wall
            assert (grid[1::2, 1::2] == m.WALL).all()  # odd / odd cells always are
            assert (grid != m.WALL).sum() == p.n_open == 2 * p.nr * p.nc - 1 and (grid == m.CLEAN).sum() == 0
            assert len(_flood(grid)) == p.n_open  # connected: a spanning tree of the rooms
            assert len(gen["tree"]) == p.nr * p.nc - 1 and len(set(gen["tree"])) == len(gen["tree"])
            if R % 2 == 0:
                assert (grid[R - 1] == m.WALL).all()  # an even R leaves a solid last row
            if C % 2 == 0:
                assert (grid[:, C - 1] == m.WALL).all()
            trees.add(tuple(sorted(gen["tree"])))
    assert len(trees) > 1 or p.nr * p.nc <= 2  # the maze really is random
    st, obs = m.reset(p, 3, seed=11, env_offset=3, t=17)  # reset() is generate() on those draws, (0, 0) cleaned
    want = m.generate(p, m.draws(11, [5], 17, p.n_draws)[0])["grid"]
    want[0, 0] = m.CLEAN
    assert np.array_equal(st["grid"][2], want) and (st["pos"] == 0).all()
    assert obs["agents_view"].shape == (3, 2, R * C * 4) and obs["global_state"].shape == (3, 1, R * C * 3)


def test_the_tree_is_the_minimum_spanning_tree():
    """Against a second algorithm: Prim from room (0, 0) under the same weights gives the same edge set."""
    p = m.Params(9, 12, 1)
    for dr in m.draws(3, np.arange(20), 5, p.n_draws):
        es = {n: (a, b) for n, a, b, _cell in m.edges(p)}
        inside, tree = {(0, 0)}, set()
        while len(inside) < p.nr * p.nc:
            n = min((n for n, (a, b) in es.items() if (a in inside) != (b in inside)), key=lambda n: (int(dr[n]), n))
            tree.add(n)
            inside |= set(es[n])
        assert tree == set(m.generate(p, dr)["tree"])


def test_draws_skip_the_ids_of_missing_edges():
    """Edge n keeps draw n: the last column's horizontal ids and the last row's vertical ids are unused, not renumbered."""
    p = m.Params(5, 5, 1)
    ids = [n for n, *_ in m.edges(p)]
    assert len(ids) == 12 and 4 not in ids and 17 not in ids and max(ids) < p.n_draws == 18
    assert {n: cell for n, _a, _b, cell in m.edges(p)}[7] == (3, 0)  # room (1, 0) = q 3, vertical: through cell (3, 0)


def _direct_view(p, grid, pos, j):
    out = np.zeros((p.R, p.C, 4), np.float32)
    for r in range(p.R):
        for c in range(p.C):
            out[r, c] = [grid[r, c] == m.DIRTY, grid[r, c] == m.WALL, sum(tuple(q) == (r, c) for q in pos), tuple(pos[j]) == (r, c)]
    return out


def test_random_rollout_invariants():
    p = m.Params(5, 7, 3, time_limit=15)
    E = 24
    st, obs = m.reset(p, E, seed=5)
    rng = np.random.default_rng(0)
    total = {k: 0 for k in m.EVENTS}
    for t in range(1, 81):
        mask = obs["action_mask"]
        assert mask.any(-1).all()  # every agent has a legal move in every observation
        u = rng.random((E, p.A, 4)) * np.where(rng.random((E, p.A, 1)) < 0.05, 1.0, mask)
        a = u.argmax(-1).astype(np.int32)
        dirty_before = (st["grid"] == m.DIRTY).sum((1, 2))
        obs, r, done, ir, il, it, extra = m.step(p, st, a, 5, 0, t)
        assert (r[:, :1] == r).all() and (r >= -0.5).all() and (r <= p.A - 0.5).all() and (r * 2 == np.round(r * 2)).all()
        cont = it == 0
        assert ((dirty_before - (st["grid"] == m.DIRTY).sum((1, 2)))[cont] == (r[:, 0] + 0.5)[cont]).all()
        assert (extra["won"] <= it).all() and (extra["terminated"] <= it).all() and (extra["won"] <= extra["terminated"]).all()
        for e in range(E):
            grid, pos = st["grid"][e], st["pos"][e]
            assert (grid != m.WALL).sum() == p.n_open
            for k in range(p.A):
                assert grid[tuple(pos[k])] == m.CLEAN  # an agent's cell is clean
                assert np.array_equal(obs["agents_view"][e, k].reshape(p.R, p.C, 4), _direct_view(p, grid, pos, k))
            assert np.array_equal(obs["global_state"][e, 0].reshape(p.R, p.C, 3), _direct_view(p, grid, pos, 0)[..., :3])
        assert (il[it == 1] <= 15).all() and (obs["step_count"][it == 1] == 0).all() and (st["pos"][it == 1] == 0).all()
        for k in m.EVENTS:
            total[k] += extra["events"][k]
    assert all(total[k] > 0 for k in ("cleaned", "shared_cleans", "blocked", "invalid_ends", "truncations")), total


def test_a_small_maze_can_be_won():
    """Following the mask greedily towards dirt wins 3 x 3 (seven open cells); `won` is reported on that step only."""
    p = m.Params(3, 3, 1, time_limit=40)
    st, obs = m.reset(p, 8, seed=2)
    rng = np.random.default_rng(1)
    wins = 0
    for t in range(1, 200):
        a = (rng.random((8, 1, 4)) * obs["action_mask"]).argmax(-1).astype(np.int32)
        obs, _r, _d, _ir, _il, it, extra = m.step(p, st, a, 2, 0, t)
        assert not extra["events"]["blocked"] and (extra["won"] == (it & extra["terminated"])).all()
        wins += int(extra["won"].sum())
    assert wins > 0


def test_auto_reset_observation_and_real_obs():
    """A terminal step returns the observation of the environment regenerated at that step's counter; real_view keeps
    the view of the state the rules produced."""
    p = m.Params(5, 5, 2, time_limit=3)
    st, first = m.reset(p, 4, seed=7, env_offset=100)
    for t in (1, 2, 3):
        a = first["action_mask"].argmax(-1).astype(np.int32) if t == 1 else back
        back = (a + 2) % 4  # there and back again: always valid
        obs, _r, done, _ir, il, it, extra = m.step(p, st, a, 7, 100, t)
    assert done.all() and it.all() and (il == 3).all() and not extra["terminated"].any() and not extra["won"].any()
    _, want_obs = m.reset(p, 4, seed=7, env_offset=100, t=3)
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], want_obs[k]), k
    assert not np.array_equal(want_obs["agents_view"], first["agents_view"])
    assert not np.array_equal(extra["real_view"], obs["agents_view"]) and (extra["real_view"].reshape(4, 2, 5, 5, 4)[:, :, 0, 0, 3] == 0).all()


def test_model_reproduces_the_golden_file():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    R, C, A, tl, E, steps, seed, off = (int(v) for v in g["params"])
    assert (R, C, A, steps) == (5, 5, 5, 20)
    p = m.Params(R, C, A, tl)
    st, obs = m.reset(p, E, seed, off, 0)
    for k in m.STATE_FIELDS:
        assert np.array_equal(st[k], g[f"reset_{k}"]), k
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], g[f"reset_obs_{k}"]), k
    for t in range(steps):
        out = m.step(p, st, g["action"][t], seed, off, t + 1)
        for k in m.STATE_FIELDS:
            assert np.array_equal(st[k], g[k][t]), (t, k)
        for k in ("agents_view", "global_state", "action_mask", "step_count"):
            assert np.array_equal(out[0][k], g[f"obs_{k}"][t]), (t, k)
        for k, v in zip(("reward", "done", "info_return", "info_length", "info_terminal"), out[1:6]):
            assert np.array_equal(v, g[k][t]), (t, k)
        for k in ("won", "terminated", "real_view", "real_mask"):
            assert np.array_equal(out[6][k], g[k][t]), (t, k)
    assert g["info_terminal"].sum() >= E and g["terminated"].sum() > 0 and (g["info_terminal"] > g["terminated"]).any()


def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cpu = torch.device("cpu")
    assert compose("default_ff_mappo", ["env=cleaner"]).env.scenario.task_name == "clean-5x5x5a"
    for name, (N, tl) in m.SCENARIOS.items():
        cfg = compose("default_ff_mappo", ["env=cleaner", f"env/scenario={name}", "network=cnn"])
        assert cfg.env.env_name == "Cleaner" and cfg.env.implicit_agent_id is True and cfg.env.log_win_rate is True
        assert cfg.env.kwargs == {} and cfg.env.eval_metric == "episode_return" and cfg.env.scenario.task_name == name
        assert cfg.env.scenario.name == "Cleaner-v0" and cfg.env.scenario.env_kwargs.time_limit == tl
        assert dict(cfg.env.scenario.task_config) == {"num_rows": N, "num_cols": N, "num_agents": N}
        env, ev = envs.make(cfg, add_global_state=True, device=cpu)
        assert isinstance(env, envs.Cleaner) and (env.num_rows, env.num_cols, env.num_agents, env.time_limit) == (N, N, N, tl)
        assert env.obs_dim == N * N * 4 and env.state_dim == N * N * 3 and env.action_dim == 4
        assert env.obs_shape == (N, N, 4) and env.state_shape == (N, N, 3) and env.implicit_agent_id
        assert env.gs_tiles == 1 and env.global_state_shared and not env.supports_fused_rollout and env.emits_real_next_obs
        assert ev.seed == env.seed ^ envs.synthetic_rware.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
        spec = env.observation_spec()
        assert spec[0] == (N, N * N * 4) and spec[1] == (N, 4) and spec[2] == (N, N * N * 3)
        assert m.params_of(env) == m.Params(N, N, N, tl)
    assert compose("default_rec_ippo", ["env=cleaner"]).env.scenario.task_name == "clean-5x5x5a"
    # system.add_agent_id is ignored (implicit ids), env.kwargs.time_limit overrides the scenario's
    env, _ = envs.make(compose("default_ff_ippo", ["env=cleaner", "system.add_agent_id=false", "env.kwargs.time_limit=9"]),
                       device=cpu)
    assert env.obs_dim == 100 and env.time_limit == 9
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.obs_dim, c.seed, c.time_limit, c.obs_shape) == (8, 64, 100, env.seed, 9, (5, 5, 4))
    with pytest.raises(ValueError, match="discrete"):
        envs.make(compose("default_ff_ippo", ["env=cleaner", "network=continuous_mlp"]), device=cpu)


def test_rec_iql_accepts_cleaner():
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    rec_iql._check_config(compose("default_rec_iql", ["env=cleaner"]))


class _StubEnv:
    """Scripted episode ends on the CPU: env e ends at step ends[e] with won_episode wons[e], and (like an auto-reset
    env) again one step later with the opposite flag, which the evaluator must not take."""

    def __init__(self, ends, wons, with_key=True):
        self.ends, self.wons = torch.tensor(ends), torch.tensor(wons)
        self.num_envs, self.num_agents, self.device, self.with_key = len(ends), 2, torch.device("cpu"), with_key
        self.time_limit = max(ends) + 3

    def _ts(self, t):
        from mava_amd.types import Observation, TimeStep

        E, A = self.num_envs, self.num_agents
        first, again = self.ends == t, self.ends + 1 == t
        last = first | again
        extras = {"episode_metrics": {"episode_return": torch.full((E,), float(t)), "is_terminal_step": last,
                                      "episode_length": torch.full((E,), t, dtype=torch.int32)}}
        if self.with_key:
            extras["won_episode"] = (first & self.wons) | (again & ~self.wons)
        obs = Observation(torch.zeros((E, A, 3)), torch.ones((E, A, 4), dtype=torch.bool), torch.full((E, A), t, dtype=torch.int32))
        return TimeStep(torch.where(last, 2, 1).to(torch.int8), torch.zeros((E, A)), torch.ones((E, A)), obs, extras)

    def reset(self, key=None):
        return 0, self._ts(0)

    def step(self, state, action):
        return state + 1, self._ts(state + 1)


def test_evaluator_forwards_won_episode():
    from mava_amd.config import compose
    from mava_amd.evaluator import get_eval_fn

    ends, wons = [3, 1, 4, 1, 5, 2], [True, False, True, True, False, False]

    def act(params, ts, key, act_state):
        return torch.zeros((6, 2), dtype=torch.int32), act_state

    over = ["arch.num_eval_episodes=6", "arch.num_absolute_metric_eval_episodes=18"]
    cfg = compose("default_ff_mappo", ["env=cleaner"] + over)
    assert cfg.env.log_win_rate is True
    out = get_eval_fn(_StubEnv(ends, wons), act, cfg, absolute_metric=False)(None, 0)
    assert set(out) == {"episode_return", "episode_length", "won_episode"}
    assert out["won_episode"].dtype == torch.bool and out["won_episode"].tolist() == wons and int(out["won_episode"].sum()) == 3
    assert out["episode_length"].tolist() == ends and out["episode_return"].tolist() == [float(e) for e in ends]
    out = get_eval_fn(_StubEnv(ends, wons), act, cfg, absolute_metric=True)(None, 0)  # three loops of six episodes
    assert out["won_episode"].tolist() == wons * 3 and out["episode_length"].tolist() == ends * 3
    # the logger turns it into a percentage
    from mava_amd.utils.logger import LogEvent, MavaLogger

    lg = MavaLogger.__new__(MavaLogger)
    lg.cfg = cfg
    assert lg.calc_winrate({"won_episode": out["won_episode"][:6]}, LogEvent.EVAL) == {"win_rate": 50.0}
    # no key: the env lacks it (env=smax: log_win_rate on a synthetic env), or log_win_rate is off
    smax = compose("default_ff_mappo", ["env=smax"] + over)
    assert smax.env.log_win_rate is True
    out = get_eval_fn(_StubEnv(ends, wons, with_key=False), act, smax, absolute_metric=False)(None, 0)
    assert set(out) == {"episode_return", "episode_length"} and out["episode_length"].tolist() == ends
    off = compose("default_ff_mappo", ["env=cleaner", "env.log_win_rate=false"] + over)
    assert off.env.log_win_rate is False
    out = get_eval_fn(_StubEnv(ends, wons), act, off, absolute_metric=False)(None, 0)
    assert set(out) == {"episode_return", "episode_length"} and out["episode_length"].tolist() == ends


def test_bad_scenarios_are_refused():
    from mava_amd.envs import Cleaner

    cpu = torch.device("cpu")
    ok = dict(num_envs=4, num_rows=5, num_cols=5, num_agents=3, device=cpu)
    Cleaner(**ok)
    Cleaner(**dict(ok, num_rows=32, num_cols=32, num_agents=32))
    Cleaner(**dict(ok, num_rows=3, num_cols=32, num_agents=1))
    for kw in (dict(num_rows=2), dict(num_cols=2), dict(num_rows=33), dict(num_cols=33), dict(num_agents=0), dict(num_agents=33),
               dict(time_limit=0)):
        with pytest.raises(ValueError):
            Cleaner(**dict(ok, **kw))
    env = Cleaner(**ok)
    st, obs = env.alloc_state(), env.alloc_obs()
    assert st.grid.shape == (4, 5, 5) and st.pos.shape == (4, 3, 2) and obs["action_mask"].shape == (4, 3, 4)
    with pytest.raises(ValueError, match="int32"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="go together"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 3), dtype=torch.int32), terminated=torch.zeros(4, dtype=torch.uint8))


def test_cleaner_step_argument_errors_without_a_gpu():
    from mava_amd import _lib

    lib = _lib.lib()
    ok = dict(E=4, A=3, R=5, C=7, tl=25)

    def call(fn=lib.mava_cleaner_step, is_reset=1, ptrs=True, trans=False, action=None, extra=(None,) * 3, **kw):
        a = dict(ok, **kw)
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        return fn(a["E"], a["A"], a["R"], a["C"], a["tl"], 1, 0, None, 0, is_reset, *([p] * 11), *([p if trans else None] * 5),
                  None, action, *extra, None)

    err = lib.mava_last_error
    assert call(A=33) <= -1000 and b"mava_cleaner_step: bad shape" in err()
    assert call(R=33) <= -1000 and call(C=33) <= -1000 and call(R=2) <= -1000 and call(C=2) <= -1000
    assert call(A=0) <= -1000 and call(E=-1) <= -1000
    assert call(tl=0) <= -1000 and b"time_limit" in err()
    assert call(E=2**20, R=32, C=32, A=32) <= -1000 and b"32-bit" in err()
    assert call(ptrs=False) <= -1000 and b"null state" in err()
    assert call(is_reset=0) <= -1000 and b"transition" in err()
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in err()
    # real_view / real_mask / terminated: none of them on a step reaches the later checks (the line above), one or two are
    # rejected, all three must not alias the observation
    assert b"real_view" not in err()
    assert call(A=33, extra=(16, 16, 16)) <= -1000 and b"mava_cleaner_step: bad shape" in err()
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        assert call(is_reset=0, trans=True, action=16, extra=part) <= -1000 and b"real_view" in err()
        assert call(is_reset=1, extra=part) <= -1000 and b"real_view" in err()
    assert call(is_reset=0, trans=True, action=16, extra=(16, 16, 16)) <= -1000 and b"alias" in err()
    assert call(E=0) == 0  # nothing to do, nothing launched
