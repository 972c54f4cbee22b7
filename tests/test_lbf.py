"""CPU: the Level-Based Foraging rules (tests/lbf_model.py, the NumPy statement the kernel is checked against on the GPU
by tests/test_gpu_lbf.py), the generator's invariants, the `env=lbf` configuration and the mava_lbf_step argument
checks, which return before any launch."""
import numpy as np
import pytest
import torch

from tests import lbf_model as m

SCENARIOS = {  # name: (G, fov, A, F, max level, force_coop)
    "2s-8x8-2p-2f-coop": (8, 2, 2, 2, 2, True), "8x8-2p-2f-coop": (8, 8, 2, 2, 2, True),
    "2s-10x10-3p-3f": (10, 2, 3, 3, 2, False), "10x10-3p-3f": (10, 10, 3, 3, 2, False),
    "15x15-3p-5f": (15, 15, 3, 5, 2, False), "15x15-4p-3f": (15, 15, 4, 3, 2, False),
    "15x15-4p-5f": (15, 15, 4, 5, 2, False),
}


@pytest.mark.parametrize("case", m.scripted_cases(), ids=lambda c: c[0])
def test_scripted_rule(case):
    _name, p, st, action, t, expect = case
    expect(m.run_case(p, st, action, t))


def test_auto_reset_observation():
    """A terminal step returns the observation of the environment regenerated at that step's counter."""
    p = m.Params(G=8, fov=2, A=2, F=2, max_level=2, force_coop=False, time_limit=3)
    st, _ = m.reset(p, 4, seed=7, env_offset=100)
    for t in (1, 2):
        m.step(p, st, np.zeros((4, 2), np.int32), 7, 100, t)
    obs, _r, done, *_ = m.step(p, st, np.zeros((4, 2), np.int32), 7, 100, 3)
    assert done.all()
    _, want_obs = m.reset(p, 4, seed=7, env_offset=100, t=3)
    for k in ("agents_view", "global_state", "action_mask", "step_count"):
        assert np.array_equal(obs[k], want_obs[k]), k
    assert not np.array_equal(want_obs["agents_view"], m.reset(p, 4, seed=7, env_offset=100, t=0)[1]["agents_view"])


@pytest.mark.parametrize("name", ["2s-8x8-2p-2f-coop", "10x10-3p-3f", "15x15-3p-5f", "15x15-4p-5f"])
def test_generator_invariants(name):
    G, fov, A, F, ml, coop = SCENARIOS[name]
    p = m.Params(G, fov, A, F, ml, coop)
    n = 2500  # 10^4 resets over the four scenarios
    st, obs = m.reset(p, n, seed=11, env_offset=3, t=17)
    fp, ap = st["food_pos"], st["agent_pos"]
    assert ((fp >= 1) & (fp <= G - 2)).all()  # foods interior
    for i in range(F):
        for k in range(i):
            assert (np.abs(fp[:, i] - fp[:, k]).max(-1) >= 2).all()  # no two foods adjacent (diagonals included)
    assert ((ap >= 0) & (ap < G)).all()
    for j in range(A):
        for i in range(F):
            assert (np.abs(ap[:, j] - fp[:, i]).max(-1) > 0).all()  # agents off foods
        for k in range(j):
            assert (np.abs(ap[:, j] - ap[:, k]).max(-1) > 0).all()  # agents on distinct cells
    al, fl = st["agent_level"], st["food_level"]
    assert ((al >= 1) & (al <= ml)).all() and set(np.unique(al)) == set(range(1, ml + 1))
    max_food = np.sort(al, -1)[:, ::-1][:, : min(3, A)].sum(-1)
    if coop:
        assert (fl == max_food[:, None]).all()
    else:
        assert ((fl >= 1) & (fl <= max_food[:, None])).all() and (fl < max_food[:, None]).any()
    assert np.array_equal(st["total_food_level"], fl.sum(-1).astype(np.float32))
    assert st["food_alive"].all() and (st["step_count"] == 0).all()
    assert obs["agents_view"].shape == (n, A, A + 3 * (F + A)) and obs["action_mask"][:, :, 0].all()
    # foods sit on every interior cell over many resets, agents anywhere (the draws cover the candidate lists)
    assert len({(int(r), int(c)) for r, c in fp.reshape(-1, 2)}) == (G - 2) ** 2


def test_random_rollout_invariants():
    """300 random steps (invalid actions included): returns stay in [0, 1], rewards are non-negative, episodes end at
    the time limit or when every food is eaten."""
    p = m.Params(10, 10, 3, 3, 2, False, time_limit=20)
    E = 200
    st, obs = m.reset(p, E, seed=5)
    rng = np.random.default_rng(0)
    eaten = 0
    for t in range(1, 301):
        a = rng.integers(0, 6, (E, 3)).astype(np.int32)
        obs, r, done, ir, il, it = m.step(p, st, a, 5, 0, t)
        assert (r >= 0).all() and (r[:, :1] == r).all()
        assert (ir[it == 1] >= 0).all() and (ir[it == 1] <= 1.0 + 1e-6).all() and (il[it == 1] <= 20).all()
        eaten += int((r > 0).any(-1).sum())
    assert eaten > 0


def test_config_and_dispatch():
    from mava_amd import envs
    from mava_amd.config import compose

    cpu = torch.device("cpu")
    cfg = compose("default_ff_mappo", ["env=lbf", "env/scenario=15x15-4p-5f"])
    assert cfg.env.env_name == "LevelBasedForaging" and cfg.env.kwargs.time_limit == 100
    env, ev = envs.make(cfg, add_global_state=True, device=cpu)
    assert isinstance(env, envs.LevelBasedForaging) and env.obs_dim == 31 and env.action_dim == 6
    assert env.state_dim == 4 * 27 and env.gs_tiles == 1 and env.global_state_shared and not env.supports_fused_rollout
    assert ev.seed == env.seed ^ envs.synthetic_rware.EVAL_KEY_TAG and ev.num_envs == cfg.arch.num_eval_episodes
    assert compose("default_rec_ippo", ["env=lbf"]).env.scenario.task_name == "2s-8x8-2p-2f-coop"
    for name, (G, fov, A, F, ml, coop) in SCENARIOS.items():
        tc = compose("default_ff_ippo", ["env=lbf", f"env/scenario={name}"]).env.scenario.task_config
        assert (tc.grid_size, tc.fov, tc.num_agents, tc.num_food, tc.max_agent_level, tc.force_coop) == (G, fov, A, F, ml, coop)
    c = env.clone(env_offset=64, num_envs=8)
    assert (c.num_envs, c.env_offset, c.obs_dim, c.seed) == (8, 64, 31, env.seed)
    rw, _ = envs.make(compose("default_ff_mappo", ["env=rware"]), add_global_state=True, device=cpu)
    assert isinstance(rw, envs.SyntheticRware)
    cfg_c = compose("default_ff_ippo", ["env=lbf", "network=continuous_mlp"])
    with pytest.raises(ValueError, match="discrete"):
        envs.make(cfg_c, device=cpu)


def test_bad_scenarios_are_refused():
    from mava_amd.envs import LevelBasedForaging

    cpu = torch.device("cpu")
    for kw in (dict(grid_size=33), dict(num_agents=17), dict(num_food=17), dict(grid_size=5, num_food=2),
               dict(max_agent_level=0)):
        args = dict(num_envs=4, grid_size=8, fov=2, num_agents=2, num_food=2, max_agent_level=2, force_coop=False, device=cpu)
        args.update(kw)
        with pytest.raises(ValueError):
            LevelBasedForaging(**args)


def test_lbf_step_argument_errors_without_a_gpu():
    from mava_amd import _lib

    lib = _lib.lib()
    ok = dict(E=4, A=2, F=2, G=8, fov=2, lvl=2, coop=0, ind=0, tl=100)

    def call(is_reset=1, ptrs=True, trans=False, action=None, **kw):
        a = dict(ok, **kw)
        p = 16 if ptrs else None  # never dereferenced: every call below is rejected on the host
        return lib.mava_lbf_step(a["E"], a["A"], a["F"], a["G"], a["fov"], a["lvl"], a["coop"], a["ind"], a["tl"], 1, 0,
                                 None, 0, is_reset, *([p] * 15), *([p if trans else None] * 5), action, None, None, None,
                                 None)  # no real_view / real_mask / terminated (tests/test_iql.py has them)

    assert call(A=17) <= -1000 and b"bad shape" in lib.mava_last_error()
    assert call(G=33) <= -1000 and call(F=0) <= -1000 and call(E=-1) <= -1000
    assert call(G=5, F=2) <= -1000 and b"cannot place" in lib.mava_last_error()
    assert call(lvl=0) <= -1000 and call(coop=2) <= -1000 and call(tl=0) <= -1000
    assert call(ptrs=False) <= -1000 and b"null state" in lib.mava_last_error()
    assert call(is_reset=0) <= -1000 and b"transition" in lib.mava_last_error()
    assert call(is_reset=0, trans=True) <= -1000 and b"action array" in lib.mava_last_error()
