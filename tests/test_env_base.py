"""What the five environments inherit from envs/base.py, checked without a GPU: the class attributes, clone, the shapes of
alloc_obs / alloc_state, and - with the library symbols replaced by a recorder - the argument list step_into hands to the
step kernels, position by position in the order of include/mava_hip.h (a swapped pair of same-typed pointers is the one
mistake no other GPU-free test would see)."""
import sys

import pytest
import torch

from mava_amd import envs
from mava_amd.envs import base

CPU = torch.device("cpu")
E = 4
STREAM = 0x5157
PREFIX = ("step_count", "run_return", "run_length", "ep_return", "ep_length", "t")

# class -> (constructor keywords, attributes, (obs_dim, state_dim, action_dim), the state's own fields)
CASES = {
    "lbf": (envs.LevelBasedForaging,
            dict(grid_size=8, fov=3, num_agents=2, num_food=2, max_agent_level=4, force_coop=True, time_limit=30),
            dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=False, emits_real_next_obs=True, implicit_agent_id=False),
            (14, 24, 6), ("agent_pos", "agent_level", "food_pos", "food_level", "food_alive", "total_food_level")),
    "rware": (envs.RobotWarehouse,
              dict(column_height=8, shelf_rows=1, shelf_columns=3, num_agents=2, sensor_range=1, request_queue_size=2,
                   time_limit=40, collision_mode="overlap"),
              dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=False, emits_real_next_obs=True, implicit_agent_id=False),
              (73, 142, 5), ("agent_pos", "agent_dir", "agent_carry", "shelf_pos", "request_queue")),
    "connector": (envs.Connector, dict(grid_size=5, num_agents=3, time_limit=20),
                  dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=False, emits_real_next_obs=True, implicit_agent_id=True),
                  (125, 75, 5), ("head", "target", "connected", "grid")),
    "cleaner": (envs.Cleaner, dict(num_rows=5, num_cols=5, num_agents=3, time_limit=25),
                dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=False, emits_real_next_obs=True, implicit_agent_id=True),
                (100, 75, 4), ("pos", "grid")),
    "synthetic": (envs.SyntheticRware, dict(num_agents=3, obs_dim=7, time_limit=50, state_dim=0, reward_mode="match"),
                  dict(gs_tiles=1, global_state_shared=True, supports_fused_rollout=True, emits_real_next_obs=False, implicit_agent_id=False),
                  (10, 21, 5), ()),
    "synthetic-tiled": (envs.SyntheticRware, dict(num_agents=3, obs_dim=7, tile_global_state=True),
                        dict(gs_tiles=3, global_state_shared=False, supports_fused_rollout=True, emits_real_next_obs=False,
                             implicit_agent_id=False),
                        (10, 21, 5), ()),
}


def _make(name, **over):
    cls, kw = CASES[name][:2]
    return cls(**dict(dict(kw, num_envs=E, add_global_state=True, seed=11, env_offset=3, device=CPU), **over))


def _plain(v):
    return list(v) if type(v).__module__ == "ctypes" or hasattr(v, "_length_") else v


@pytest.mark.parametrize("name", list(CASES))
def test_attributes_clone_and_shapes(name):
    _, _, attrs, (O, S, nA), own = CASES[name]
    env = _make(name)
    assert isinstance(env, base.BatchedEnv)
    for k, v in attrs.items():
        assert getattr(env, k) == v, k
    if not env.supports_fused_rollout:  # the native envs leave the defaults to the class
        assert not {"gs_tiles", "global_state_shared"} & set(vars(env))
    assert (env.obs_dim, env.state_dim, env.action_dim) == (O, S, nA)
    A = env.num_agents
    assert env.observation_spec() == base.ObsSpec((A, O), (A, nA), (A, S), (A,))
    assert _make(name, add_global_state=False).observation_spec().global_state is None

    if name.startswith("synthetic"):  # make() sets the image shapes on the object: a clone must carry them over
        env.obs_shape, env.state_shape = (2, 5, 1), (3, 7, 1)
    c = env.clone(7, 2)
    assert type(c) is type(env) and (c.env_offset, c.num_envs) == (7, 2) and (env.env_offset, env.num_envs) == (3, E)
    assert set(vars(c)) == set(vars(env))
    for k, v in vars(env).items():
        if k not in ("env_offset", "num_envs") and not isinstance(v, dict):  # (the dict: the recorded constructor keywords)
            assert _plain(getattr(c, k)) == _plain(v), k
    assert env.clone(9).num_envs == E and c.clone(0).num_envs == 2

    obs = env.alloc_obs()
    want = {"agents_view": ((E, A, O), torch.float32), "global_state": ((E, attrs["gs_tiles"], S), torch.float32),
            "action_mask": ((E, A, nA), torch.uint8), "step_count": ((E, A), torch.int32)}
    assert list(obs) == list(want)
    for k, (shape, dtype) in want.items():
        assert tuple(obs[k].shape) == shape and obs[k].dtype == dtype and obs[k].device == CPU, k

    st = env.alloc_state()
    assert type(st) is env.State and issubclass(env.State, tuple) and st._fields == PREFIX + own
    i32, f32 = torch.int32, torch.float32
    for f, shape, dtype in zip(PREFIX, ((E, A), (E,), (E,), (E,), (E,), ()), (i32, f32, i32, f32, i32, torch.int64)):
        x = getattr(st, f)
        assert tuple(x.shape) == shape and x.dtype == dtype and not x.any(), f
    assert int(st._replace(t=torch.tensor(5)).t) == 5
    if name == "rware":
        assert (st.agent_carry == -1).all() and st.shelf_pos.shape == (E, env.num_shelves) and st.request_queue.shape == (E, 2)
    if name == "lbf":
        assert st.food_alive.dtype == torch.uint8 and st.total_food_level.dtype == f32 and st.food_pos.shape == (E, 2, 2)


def _line_tracer(frame, event, arg):
    return _line_tracer  # local line events too: they are what re-syncs f_locals


@pytest.mark.parametrize("name", list(CASES))
def test_clone_of_an_env_built_under_a_trace_function(name):
    """A Python trace function (a debugger, a line-coverage tool) keeps a frame's locals() dict in step with the frame: the
    constructor keywords must be a snapshot taken before the constructor's own locals exist."""
    old = sys.gettrace()
    sys.settrace(_line_tracer)
    try:
        env = _make(name)
        c = env.clone(7, 2)
    finally:
        sys.settrace(old)
    assert type(c) is type(env) and (c.env_offset, c.num_envs, c.num_agents, c.time_limit) == (7, 2, env.num_agents, env.time_limit)
    assert c.clone(1).num_envs == 2 and c.obs_dim == env.obs_dim and c.state_dim == env.state_dim


class _Recorder:
    """Stands in for the library: every symbol it is asked for records its arguments and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        return lambda *args: self.calls.append((symbol, args)) or 0


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(base, "lib", lambda: rec)
    monkeypatch.setattr(envs.synthetic_rware, "lib", lambda: rec)  # its own check(...) call
    monkeypatch.setattr(base, "stream_ptr", lambda: STREAM)
    return rec


def _buffers(env):
    A = env.num_agents
    tr = dict(reward=torch.empty((E, A)), done=torch.empty((E, A), dtype=torch.uint8), info_return=torch.empty(E),
              info_length=torch.empty(E, dtype=torch.int32), info_terminal=torch.empty(E, dtype=torch.uint8))
    obs = env.alloc_obs()
    real = dict(real_obs={"agents_view": torch.empty_like(obs["agents_view"]), "action_mask": torch.empty_like(obs["action_mask"])},
                terminated=torch.empty(E, dtype=torch.uint8))
    return obs, tr, real, torch.zeros((E, A), dtype=torch.int32), torch.zeros((), dtype=torch.int32)


def _scenario_and_state(name, env, st):
    """The arguments between A and seed, and the names of the state tensors between is_reset and step_count."""
    if name == "lbf":
        return [2, 8, 3, 4, 1, 0, 30], ["agent_pos", "agent_level", "food_pos", "food_level", "food_alive", "total_food_level"]
    if name == "rware":  # S = 32 shelves, R = 2, H = 11, W = 10, sensor range 1, time limit 40, collision mode "overlap"
        return ([32, 2, 11, 10, 1, 40, 0, env._highway_rows, env._shelf_home],
                ["agent_pos", "agent_dir", "agent_carry", "shelf_pos", "request_queue"])
    if name == "connector":
        return [5, 20], ["head", "target", "connected", "grid"]
    return [5, 5, 25], ["pos", "grid"]


@pytest.mark.parametrize("name", ["lbf", "rware", "connector", "cleaner"])
def test_step_into_argument_list(name, recorder):
    env = _make(name)
    st = env.alloc_state()
    obs, tr, real, action, t_base = _buffers(env)
    won = torch.empty(E, dtype=torch.uint8)
    scenario, own = _scenario_and_state(name, env, st)
    symbol = f"mava_{name}_step"  # one entry point: the three real slots are always passed, None without real_obs
    p = torch.Tensor.data_ptr

    def want(t, off, is_reset, tb=None, with_tr=True, with_real=False, info_won=None, act=None):
        trs = [p(tr[k]) if with_tr else None for k in ("reward", "done", "info_return", "info_length", "info_terminal")]
        return ([E, env.num_agents] + scenario + [11, t, tb, off, is_reset] + [p(getattr(st, f)) for f in own]
                + [p(st.step_count), p(st.run_return), p(st.run_length), p(st.ep_return), p(st.ep_length)]
                + [p(obs["agents_view"]), p(obs["global_state"]), p(obs["action_mask"]), p(obs["step_count"])] + trs
                + ([info_won] if name == "cleaner" else []) + [act]
                + ([p(real["real_obs"]["agents_view"]), p(real["real_obs"]["action_mask"]), p(real["terminated"])] if with_real
                   else [None, None, None])
                + [STREAM])

    def last():
        sym, args = recorder.calls[-1]
        return sym, list(args)

    # a reset passes no action (even when one is given) and no transition slots
    env.step_into(st, 0, obs, is_reset=True, action=action)
    assert last() == (symbol, want(0, 3, 1, with_tr=False))
    env.step_into(st, 0, obs, is_reset=True, **real)
    assert last() == (symbol, want(0, 3, 1, with_tr=False, with_real=True))
    # a step; t is passed modulo 2^32, env_offset= overrides the object's, t_base is the device word
    env.step_into(st, (1 << 32) + 7, obs, action=action, **tr)
    assert last() == (symbol, want(7, 3, 0, act=p(action)))
    env.step_into(st, 8, obs, tr["reward"], tr["done"], tr["info_return"], tr["info_length"], tr["info_terminal"], False, 21,
                  t_base, action, **real)
    assert last() == (symbol, want(8, 21, 0, tb=p(t_base), with_real=True, act=p(action)))
    if name == "cleaner":
        env.step_into(st, 9, obs, action=action, info_won=won, **tr)
        assert last() == (symbol, want(9, 3, 0, info_won=p(won), act=p(action)))
        env.step_into(st, 9, obs, action=action, info_won=won, **tr, **real)
        assert last() == (symbol, want(9, 3, 0, with_real=True, info_won=p(won), act=p(action)))
    else:
        with pytest.raises(ValueError, match="reports no win"):
            env.step_into(st, 9, obs, action=action, info_won=won, **tr)
    # every pointer of a call is a different one: no position above can pass by standing in for its neighbour
    ptrs = [a for a in last()[1] if isinstance(a, int) and a > (1 << 16)]
    assert len(set(ptrs)) == len(ptrs) >= 17

    n = len(recorder.calls)
    cls = type(env).__name__
    with pytest.raises(ValueError, match=f"{cls}.step_into needs the .* int32"):
        env.step_into(st, 1, obs, action=action.long(), **tr)
    with pytest.raises(ValueError, match=f"{cls}.step_into needs the .* int32"):
        env.step_into(st, 1, obs, **tr)
    with pytest.raises(ValueError, match=f"{cls}.step_into: real_obs and terminated go together"):
        env.step_into(st, 1, obs, action=action, real_obs=real["real_obs"], **tr)
    assert len(recorder.calls) == n

    # the allocating API goes through the same call: reset at t = 0, a step at state.t + 1 with the action as int32
    st2, ts = env.reset()
    assert recorder.calls[-1][0] == symbol and recorder.calls[-1][1][-5:-1] == (None, None, None, None)
    assert ("won_episode" in ts.extras) == (name == "cleaner")
    st3, ts = env.step(st2, action.long())
    sym, args = recorder.calls[-1]
    i_t = 2 + len(scenario) + 1
    assert sym == symbol and args[i_t] == 1 and args[i_t + 3] == 0 and int(st3.t) == 1 and int(st2.t) == 0
    assert args[-4:-1] == (None, None, None) and isinstance(args[-5], int) and args[-5] != p(action)
    assert ("won_episode" in ts.extras) == (name == "cleaner") and set(ts.extras["episode_metrics"]) == {
        "episode_return", "episode_length", "is_terminal_step"}
    if name == "cleaner":
        assert args[-6] is not None and ts.extras["won_episode"].dtype == torch.bool


@pytest.mark.parametrize("mode", ["random", "match"])
def test_synthetic_step_arguments(mode, recorder):
    env = _make("synthetic", reward_mode=mode)
    st = env.alloc_state()
    obs, tr, real, action, _ = _buffers(env)
    p = torch.Tensor.data_ptr
    match = int(mode == "match")
    # no real-next outputs here: asked for, the call is refused before the library is reached
    with pytest.raises(ValueError, match="SyntheticRware.step_into: this environment emits no real next observation"):
        env.step_into(st, 5, obs, action=action, **tr, **real)
    assert recorder.calls == []

    def want(t, is_reset, act):
        trs = [None if is_reset else p(tr[k]) for k in ("reward", "done", "info_return", "info_length", "info_terminal")]
        return ([E, 3, 7, 5, 1, 0, 50, 11, t, None, 3, is_reset, p(st.step_count), p(st.run_return), p(st.run_length),
                 p(st.ep_return), p(st.ep_length), p(obs["agents_view"]), p(obs["global_state"]), p(obs["action_mask"]),
                 p(obs["step_count"])] + trs + [act, match, STREAM])

    env.step_into(st, 0, obs, is_reset=True)
    assert recorder.calls[-1] == ("mava_synth_rware_step", tuple(want(0, 1, None)))
    env.step_into(st, 5, obs, action=action, **tr)
    assert recorder.calls[-1] == ("mava_synth_rware_step", tuple(want(5, 0, p(action) if match else None)))
    if match:
        with pytest.raises(ValueError, match="int32"):
            env.step_into(st, 6, obs, **tr)
    else:
        env.step_into(st, 6, obs, **tr)  # "random" reads no action
        assert recorder.calls[-1][1][-3] is None
    _, ts = env.step(st, action.long())
    assert (recorder.calls[-1][1][-3] is not None) == bool(match) and "won_episode" not in ts.extras
    tiled = _make("synthetic-tiled")
    tiled.step_into(tiled.alloc_state(), 0, tiled.alloc_obs(), is_reset=True)
    assert recorder.calls[-1][1][2:7] == (7, 5, 3, 0, 500) and recorder.calls[-1][1][-2] == 0


def test_make_pair_and_public_names():
    from mava_amd.config import compose
    from mava_amd.envs import cleaner, connector, lbf, rware, synthetic_rware

    assert synthetic_rware.EVAL_KEY_TAG == base.EVAL_KEY_TAG == 0x4556414C4556414C
    assert synthetic_rware.ObsSpec is base.ObsSpec and synthetic_rware.SynthState._fields == PREFIX
    for mod, state in ((lbf, "LBFState"), (rware, "RwareState"), (connector, "ConnectorState"), (cleaner, "CleanerState")):
        assert getattr(mod, state)._fields[:6] == PREFIX and mod.NUM_ACTIONS and callable(mod.make)
    over = ["arch.num_envs=6", "arch.num_eval_episodes=2", "system.seed=5"]
    for env_name, cls in (("lbf", envs.LevelBasedForaging), ("rware_native", envs.RobotWarehouse), ("connector", envs.Connector),
                          ("cleaner", envs.Cleaner), ("rware", envs.SyntheticRware)):
        cfg = compose("default_ff_mappo", [f"env={env_name}"] + over)
        train, evale = envs.make(cfg, add_global_state=True, device=CPU, env_offset=12)
        assert type(train) is cls and type(evale) is cls
        assert (train.num_envs, evale.num_envs, train.env_offset, evale.env_offset) == (6, 2, 12, 12)
        assert train.seed == 5 and evale.seed == 5 ^ base.EVAL_KEY_TAG and train.add_global_state and evale.device == CPU
        cont = compose("default_ff_mappo", [f"env={env_name}", "network.action_head._target_=mava.networks.heads.ContinuousActionHead"] + over)
        if cls is envs.SyntheticRware:
            envs.make(cont, device=CPU)
        else:
            with pytest.raises(ValueError, match=f"{cls.__name__} has discrete actions only"):
                envs.make(cont, device=CPU)
