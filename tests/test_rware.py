"""CPU: the Robot Warehouse rules (tests/rware_model.py, the plain-Python statement the kernel is checked against on the
GPU by tests/test_gpu_rware.py), the layout, the generator's and the rollout's invariants, the `env=rware_native`
configuration and the mava_rware_step argument checks, which return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rware_model as m


def test_layout_facts():
    from mava_amd.envs.rware import warehouse_layout

    for name, H, W, S in (("tiny-2ag", 11, 10, 32), ("small-4ag", 20, 10, 80)):
        ch, rows, cols, A, s, R = m.SCENARIOS[name]
        p = m.Params(ch, rows, cols, A, s, R)
        assert (p.H, p.W, p.S) == (H, W, S) and p.goals == [(4, H - 1), (5, H - 1)]
        assert all(g in p.highway for g in p.goals) and not any(h in p.highway for h in p.homes)
        assert len(p.highway) + p.S == H * W
        for x in range(W):  # the column highways, the top and bottom rows, the corridor above the goals
            assert (x, 0) in p.highway and (x, H - 1) in p.highway and (x, H - 2) in p.highway
        assert all((x, y) in p.highway for y in range(H) for x in (0, 3, 6, 9))
        assert all(((4, y) in p.highway) == (y > H - 11 or y % 9 == 0) for y in range(H))
        # the product's own layout (bit masks) states the same warehouse
        lay = warehouse_layout(ch, rows, cols)
        assert (lay.height, lay.width) == (H, W) and list(lay.goals) == p.goals
        assert lay.shelf_home == [p.cell(x, y) for x, y in p.homes]
        assert {(x, y) for y in range(H) for x in range(W) if (lay.highway_rows[y] >> x) & 1} == p.highway
    tiny = m.Params(8, 1, 3, 2, 1, 2)
    assert tiny.homes[:5] == [(1, 1), (2, 1), (7, 1), (8, 1), (1, 2)] and tiny.shelf_of_home(8, 8) == 31
    assert tiny.raw_dim == 71 and m.Params(8, 1, 3, 2, 2, 2).raw_dim == 183


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule(case):
    _name, p, st, action, t, expect = case
    expect(m.run_case(p, st, action, t))


def test_auto_reset_observation_and_real_obs():
    """A terminal step returns the observation of the environment regenerated at that step's counter; real_view keeps
    the view of the state the rules produced."""
    p = m.Params(8, 1, 3, 2, 1, 2, time_limit=3)
    st, _ = m.reset(p, 4, seed=7, env_offset=100)
    noop = np.zeros((4, 2), np.int32)
    for t in (1, 2):
        before = m.step(p, st, noop, 7, 100, t)[0]
    obs, _r, done, _ir, il, it, extra = m.step(p, st, noop, 7, 100, 3)
    assert done.all() and it.all() and (il == 3).all() and not extra["terminated"].any()
    _, want_obs = m.reset(p, 4, seed=7, env_offset=100, t=3)
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], want_obs[k]), k
    assert not np.array_equal(want_obs["agents_view"], m.reset(p, 4, seed=7, env_offset=100, t=0)[1]["agents_view"])
    assert np.array_equal(extra["real_view"], before["agents_view"])  # nobody moved: the pre-reset view is the old one


@pytest.mark.parametrize("name", list(m.SCENARIOS))
def test_generator_invariants(name):
    p = m.Params(*m.SCENARIOS[name])
    n = 1500
    st, obs = m.reset(p, n, seed=11, env_offset=3, t=17)
    ap = st["agent_pos"]
    assert ((ap >= 0) & (ap[..., 0] < p.W)[..., None] & (ap[..., 1] < p.H)[..., None]).all()
    for j in range(p.A):
        for k in range(j):
            assert (ap[:, j] != ap[:, k]).any(-1).all()  # agents on distinct cells
    q = np.sort(st["request_queue"], -1)
    assert ((q >= 0) & (q < p.S)).all() and (q[:, 1:] != q[:, :-1]).all()  # queue distinct
    assert (st["shelf_pos"] == np.array([p.cell(x, y) for x, y in p.homes])).all()  # shelves on their homes
    assert (st["agent_carry"] == -1).all() and (st["step_count"] == 0).all()
    assert set(np.unique(st["agent_dir"])) == {0, 1, 2, 3}
    assert obs["agents_view"].shape == (n, p.A, p.A + 71) and obs["action_mask"][:, :, [0, 2, 3, 4]].all()
    # over many resets agents start on every cell (under shelves too) and every shelf is requested
    assert len({(int(x), int(y)) for x, y in ap.reshape(-1, 2)}) == p.H * p.W
    assert set(np.unique(st["request_queue"])) == set(range(p.S))


@pytest.mark.parametrize("mode", ["terminate", "overlap"])
def test_random_rollout_invariants(mode):
    p = m.Params(8, 1, 3, 4, 1, 4, time_limit=40, collision_mode=mode)
    E = 48
    st, obs = m.reset(p, E, seed=5)
    m.craft(p, st, range(0, 8), "deliver")
    rng = np.random.default_rng(0)
    total = {k: 0 for k in m.EVENTS}
    for t in range(1, 121):
        a = rng.integers(0, 5, (E, p.A)).astype(np.int32)
        if t == 1:
            a[:8, 0] = m.FORWARD
        obs, r, done, ir, il, it, extra = m.step(p, st, a, 5, 0, t)
        assert (r >= 0).all() and (r == np.round(r)).all() and (r[:, :1] == r).all()
        for e in range(E):
            sp, carry = st["shelf_pos"][e], st["agent_carry"][e]
            assert sp.shape == (p.S,) and ((sp >= 0) & (sp < p.H * p.W)).all()
            ground = [int(sp[s]) for s in range(p.S) if s not in carry]
            assert len(ground) == len(set(ground))  # no two ground shelves on a cell
            for j in range(p.A):
                if carry[j] >= 0:
                    assert sp[carry[j]] == p.cell(*st["agent_pos"][e, j])  # a carried shelf is on its carrier's cell
            assert len({c for c in carry if c >= 0}) == sum(c >= 0 for c in carry)
            assert len(set(st["request_queue"][e].tolist())) == p.R
            assert all((c % p.W, c // p.W) not in p.highway for c in ground)
        assert (il[it == 1] <= 40).all()
        if mode == "overlap":
            assert not extra["terminated"].any()
        for k in m.EVENTS:
            total[k] += extra["events"][k]
    assert total["deliveries"] >= 8 and total["pickups"] > 0 and total["putdowns"] > 0 and total["truncations"] > 0


def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cpu = torch.device("cpu")
    cfg = compose("default_ff_mappo", ["env=rware_native", "env/scenario=tiny-4ag"])
    assert cfg.env.env_name == "RobotWarehouse" and cfg.env.native and cfg.env.kwargs.time_limit == 500
    assert cfg.env.kwargs.collision_mode == "terminate" and cfg.env.eval_metric == "episode_return"
    env, ev = envs.make(cfg, add_global_state=True, device=cpu)
    assert isinstance(env, envs.RobotWarehouse) and env.obs_dim == 75 and env.action_dim == 5 and env.state_dim == 284
    assert (env.height, env.width, env.num_shelves, env.request_queue_size) == (11, 10, 32, 4)
    assert env.gs_tiles == 1 and env.global_state_shared and not env.supports_fused_rollout and env.emits_real_next_obs
    assert ev.seed == env.seed ^ envs.synthetic_rware.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
    spec = env.observation_spec()
    assert spec[0] == (4, 75) and spec[1] == (4, 5) and spec[2] == (4, 284)
    assert compose("default_rec_ippo", ["env=rware_native"]).env.scenario.task_name == "tiny-2ag"
    easy = compose("default_ff_ippo", ["env=rware_native", "env/scenario=tiny-4ag-easy"]).env.scenario.task_config
    assert (easy.num_agents, easy.request_queue_size, easy.shelf_columns) == (4, 8, 3)
    small, _ = envs.make(compose("default_rec_mappo", ["env=rware_native", "env/scenario=small-4ag"]), device=cpu)
    assert (small.height, small.width, small.num_shelves) == (20, 10, 80)
    ov, _ = envs.make(compose("default_ff_ippo", ["env=rware_native", "env.kwargs.collision_mode=overlap"]), device=cpu)
    assert ov.collision_mode == "overlap" and ov.num_agents == 2 and ov.obs_dim == 73
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.obs_dim, c.seed, c.collision_mode) == (8, 64, 75, env.seed, "terminate")
    assert m.params_of(c) == m.Params(8, 1, 3, 4, 1, 4)
    # env=rware is still the synthetic stand-in
    rw, _ = envs.make(compose("default_ff_mappo", ["env=rware"]), add_global_state=True, device=cpu)
    assert isinstance(rw, envs.SyntheticRware) and rw.obs_dim == 68
    with pytest.raises(ValueError, match="discrete"):
        envs.make(compose("default_ff_ippo", ["env=rware_native", "network=continuous_mlp"]), device=cpu)
    with pytest.raises(ValueError, match="agent one-hot"):
        envs.make(compose("default_ff_ippo", ["env=rware_native", "system.add_agent_id=false"]), device=cpu)


def test_rec_iql_accepts_the_native_env_only():
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    rec_iql._check_config(compose("default_rec_iql", ["env=rware_native"]))
    for name in ("rware", "smax"):
        with pytest.raises(ValueError, match="pre-reset observation"):
            rec_iql._check_config(compose("default_rec_iql", [f"env={name}"]))


def test_bad_scenarios_are_refused():
    from mava_amd.envs import RobotWarehouse

    cpu = torch.device("cpu")
    ok = dict(num_envs=4, column_height=8, shelf_rows=1, shelf_columns=3, num_agents=2, sensor_range=1,
              request_queue_size=2, device=cpu)
    RobotWarehouse(**ok)
    for kw in (dict(shelf_columns=11), dict(shelf_rows=4), dict(num_agents=17), dict(num_agents=0),
               dict(column_height=20, shelf_columns=10), dict(request_queue_size=0), dict(request_queue_size=32),
               dict(request_queue_size=17), dict(sensor_range=0), dict(sensor_range=3), dict(time_limit=0),
               dict(collision_mode="bounce")):
        with pytest.raises(ValueError):
            RobotWarehouse(**dict(ok, **kw))
    env = RobotWarehouse(**ok)
    st, obs = env.alloc_state(), env.alloc_obs()
    with pytest.raises(ValueError, match="int32"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="go together"):
        env.step_into(st, 1, obs, action=torch.zeros((4, 2), dtype=torch.int32), terminated=torch.zeros(4, dtype=torch.uint8))


def test_rware_step_argument_errors_without_a_gpu():
    from mava_amd import _lib
    from mava_amd.envs.rware import warehouse_layout

    lib = _lib.lib()
    lay = warehouse_layout(8, 1, 3)
    ok = dict(E=4, A=2, S=32, R=2, H=11, W=10, sr=1, tl=500, coll=1)

    def call(fn=lib.mava_rware_step, is_reset=1, ptrs=True, trans=False, action=None, rows=lay.highway_rows,
             home=lay.shelf_home, extra=(None,) * 3, **kw):
        a = dict(ok, **kw)
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        hr = (C.c_uint32 * len(rows))(*rows) if rows is not None else None
        hm = (C.c_int32 * len(home))(*home) if home is not None else None
        return fn(a["E"], a["A"], a["S"], a["R"], a["H"], a["W"], a["sr"], a["tl"], a["coll"], hr, hm, 1, 0, None, 0,
                  is_reset, *([p] * 14), *([p if trans else None] * 5), action, *extra, None)

    err = lib.mava_last_error
    assert call(A=17) <= -1000 and b"mava_rware_step: bad shape" in err()
    assert call(W=33) <= -1000 and call(H=33) <= -1000 and call(S=257) <= -1000 and call(E=-1) <= -1000 and call(A=0) <= -1000
    assert call(R=0) <= -1000 and b"bad scenario" in err()
    assert call(R=32) <= -1000 and call(R=17) <= -1000 and call(sr=0) <= -1000 and call(sr=3) <= -1000
    assert call(tl=0) <= -1000 and call(coll=2) <= -1000
    assert call(rows=None) <= -1000 and b"null layout" in err()
    assert call(home=[5] + lay.shelf_home[1:]) <= -1000 and b"bad layout" in err()  # (5, 0) is a highway
    assert call(home=lay.shelf_home[:1] + lay.shelf_home[:-1]) <= -1000 and b"increasing" in err()
    assert call(rows=[0] * 11) <= -1000 and b"goal" in err()
    assert call(ptrs=False) <= -1000 and b"null state" in err()
    assert call(is_reset=0) <= -1000 and b"transition" in err()
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in err()
    # real_view / real_mask / terminated: none of them on a step reaches the later checks (the line above), one or two are
    # rejected, all three must not alias the observation
    assert b"real_view" not in err()
    assert call(A=17, extra=(16, 16, 16)) <= -1000 and b"mava_rware_step: bad shape" in err()
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        assert call(is_reset=0, trans=True, action=16, extra=part) <= -1000 and b"real_view" in err()
        assert call(is_reset=1, extra=part) <= -1000 and b"real_view" in err()
    assert call(is_reset=0, trans=True, action=16, extra=(16, 16, 16)) <= -1000 and b"alias" in err()
    assert call(E=0) == 0  # nothing to do, nothing launched
