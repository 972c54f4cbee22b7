"""mava_rollout_ff_f32 (csrc/rollout_h2.hip) called directly: every one of its six template instances at its edges against the
NumPy float64 model of one launch (tests/rollout_model.py: the model, the case table and the restatement of the dispatch).
Each case asserts through mava_debug_rollout_last_instance() WHICH instance it ran.  What the environment phase writes is
compared bit for bit; sampled actions may differ from the model's own draw only at near-ties of the Gumbel-max, which
tests/test_rollout_model.py caps on the reference alone; value / log_prob / last_val / adv / tgt are held to 5e-5, the figure
tests/test_gpu_learner.py holds this kernel to.  The remaining tests compare launches with each other and need no tolerance."""
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests import rollout_model as M
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

OBS = ("agents_view", "global_state", "action_mask", "obs_step_count")  # (T + 1, E, ...): slot 0 is the caller's
STEP = ("action", "value", "reward", "log_prob", "done", "info_return", "info_length", "info_terminal")  # (T, E, ...)
STATE = ("state.step_count", "state.run_return", "state.run_length", "state.ep_return", "state.ep_length")  # (E, ...)
FLOATS = ("value", "log_prob", "last_val", "adv", "tgt")
SENTINEL = {torch.float32: float("nan"), torch.int32: -7, torch.uint8: 0xAB, torch.float16: float("nan")}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _instance():
    from mava_amd._lib import lib

    return lib().mava_debug_rollout_last_instance()


def _buffers(dev, c, init, with_gae=True):
    """Output buffers as tests/test_gpu_x16.py::_run_rollout allocates them, filled with sentinels (an entry the launch does not
    write shows up in every bit-exact comparison), slot 0 and the env-state words from `init`."""
    E, A, T, W, AO, nA = c.E, c.A, c.T, c.A + c.O, c.A * c.O, c.nA
    f = lambda shape, dt=torch.float32: torch.full(shape, SENTINEL[dt], dtype=dt, device=dev)  # noqa: E731
    b = dict(agents_view=f((T + 1, E, A, W)), global_state=f((T + 1, E, 1, AO)) if c.shared else None,
             action_mask=f((T + 1, E, A, nA), torch.uint8), obs_step_count=f((T + 1, E, A), torch.int32),
             action=f((T, E, A), torch.int32), value=f((T, E, A)), reward=f((T, E, A)), log_prob=f((T, E, A)),
             done=f((T, E, A), torch.uint8), last_val=f((E, A)), info_return=f((T, E)), info_length=f((T, E), torch.int32),
             info_terminal=f((T, E), torch.uint8))
    if with_gae:
        b.update(adv=f((T, E, A)), tgt=f((T, E, A)))
    b["agents_view"][0] = _t(np.asarray(init["agents_view"], np.float32), dev)
    if c.shared:
        b["global_state"][0] = _t(np.asarray(init["global_state"], np.float32), dev)
    b["action_mask"][0] = _t(np.asarray(init["action_mask"]).astype(np.uint8), dev)
    b["obs_step_count"][0] = _t(np.asarray(init["step_count"], np.int32), dev)
    st = SimpleNamespace(**{k: _t(init[k], dev).clone() for k in ("step_count", "run_return", "run_length", "ep_return", "ep_length")})
    return b, st


def _run(c, pa, pc, b, st, **opt):
    from mava_amd import ops

    ok = ops.rollout_ff(pa, pc, n_actions=c.nA, critic_shared=c.shared, E=c.E, A=c.A, O=c.O, T=c.T, time_limit=c.time_limit,
                        policy_seed=c.policy_seed, env_seed=c.env_seed, t0=c.t0, row_offset=c.row_offset, env_offset=c.env_offset,
                        reward_mode=c.reward_mode, env_state=st, gamma=M.GAMMA, gae_lambda=M.LAMBDA, **opt, **b)
    torch.cuda.synchronize()
    return ok


def _numpy(b, st):
    out = {k: v.cpu().numpy() for k, v in b.items() if v is not None}
    out.update({f"state.{k}": v.cpu().numpy() for k, v in vars(st).items()})
    return out


def _launch(dev, c, params, init, with_gae=True, **opt):
    b, st = _buffers(dev, c, init, with_gae)
    assert _run(c, _t(params[0], dev), _t(params[1], dev), b, st, **opt), f"{c.name}: the fused rollout does not instantiate this shape"
    return _numpy(b, st)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _rel_err(got, want):
    """The largest |got - want| / (|want| + rms(want)): assert_close(got, want, rtol) holds exactly when this is <= rtol."""
    want = np.asarray(want, np.float64)
    err, den = np.abs(np.asarray(got, np.float64) - want), np.abs(want) + np.sqrt(np.mean(want * want))
    with np.errstate(divide="ignore", invalid="ignore"):  # (an all-zero reference: the one-action case's log-probs)
        return float(np.where(err == 0.0, 0.0, err / den).max())


def _check_against_model(c, out, ref, init, tol):
    """`out`: one launch; `ref`: the model run with the launch's actions forced.  Returns the number of rows at which the model's
    own draw differs."""
    T = c.T
    # ---- bit-exact: what the environment phase writes, and slot 0 left as the caller wrote it
    slot0 = {"agents_view": np.asarray(init["agents_view"], np.float32), "global_state": np.asarray(init["global_state"], np.float32),
             "action_mask": np.asarray(init["action_mask"]).astype(np.uint8), "obs_step_count": np.asarray(init["step_count"], np.int32)}
    for k in OBS:
        if k == "global_state" and not c.shared:
            continue
        assert _same_bits(out[k][0], slot0[k].reshape(out[k][0].shape)), f"{c.name}: slot 0 of {k} belongs to the caller"
        assert np.array_equal(out[k][1:].astype(np.float64), ref[k][1:].astype(np.float64)), f"{c.name}: {k} in slots 1 .. T"
    assert np.array_equal(out["reward"], ref["reward"].astype(np.float32)), f"{c.name}: reward"
    for k in ("done", "info_terminal"):
        assert np.array_equal(out[k].astype(bool), ref[k]), f"{c.name}: {k}"
        assert set(np.unique(out[k])) <= {0, 1}
    assert np.array_equal(out["info_return"], ref["info_return"]) and out["info_return"].dtype == ref["info_return"].dtype
    assert np.array_equal(out["info_length"], ref["info_length"])
    for k in STATE:
        assert np.array_equal(out[k], ref[k]) and out[k].dtype == ref[k].dtype, f"{c.name}: {k} after the launch"
    # ---- actions: legal, and different from the model's own draw only at a near-tie
    act = out["action"].astype(np.int64)
    assert act.min() >= 0 and act.max() < c.nA
    mask = ref["action_mask"][:T]
    legal = np.take_along_axis(mask, act[..., None], 3)[..., 0]
    assert (legal | ~mask.any(-1)).all(), f"{c.name}: an illegal action was sampled"
    diff = ref["own_action"] != out["action"]
    assert (ref["action_margin"][diff] < M.NEAR_TIE).all(), f"{c.name}: actions differ beyond a near-tie: {ref['action_margin'][diff]}"
    assert not (diff & ~(ref["runner_up_gap"] < M.NEAR_TIE)).any(), "a disagreeing row is not among the reference's near-ties"
    assert diff.sum() <= M.NEAR_TIE_CAP * diff.size
    # ---- floats against float64, and the kernel's GAE on its own inputs
    errs = {k: _rel_err(out[k], ref[k]) for k in FLOATS}
    print(f"{c.name}: instance {c.inst}, {int(diff.sum())}/{diff.size} action disagreements, rel err "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {tol:.1e})")
    for k in FLOATS:  # (the buffers were filled with NaN, and assert_close lets NaN through: an entry not written fails here)
        assert np.isfinite(out[k]).all(), f"{c.name}: {k} has {int((~np.isfinite(out[k])).sum())} entries that are not finite"
        assert_close(out[k], ref[k], tol, f"{c.name}: {k}")
    a64, t64 = po.gae(out["reward"], out["value"], out["done"].astype(bool), out["last_val"], M.GAMMA, M.LAMBDA)
    assert_close(out["adv"], a64, 1e-5, f"{c.name}: advantages on identical inputs")
    assert_close(out["tgt"], t64, 1e-5, f"{c.name}: targets on identical inputs")
    return int(diff.sum())


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_rollout_case_matches_model(dev, c):
    params, init = M.case_params(c), M.case_init(c)
    out = _launch(dev, c, params, init)
    assert _instance() == c.inst, f"rollout instance {_instance()} ran, wanted {c.inst}"
    ref = M.rollout(c, *params, init, forced_action=out["action"])
    _check_against_model(c, out, ref, init, M.float_tolerance(c.name))


@pytest.mark.parametrize("name", ["s-A8-O3-n8", "d-A2-O13-n8"])
def test_slot0_mask_is_honoured(dev, name):
    """A caller-written slot-0 mask over eight actions: rows with a single legal action (2 .. 7: neither action 0, which wins
    every exact tie, nor action 1, the only one the environment ever masks), rows with all but one, alternating rows."""
    c = M.CASE_BY_NAME[name]
    assert c.nA == 8
    params, init = M.case_params(c), dict(M.case_init(c))
    R = c.E * c.A
    mask = np.ones((R, 8), np.uint8)
    rows = np.arange(R)
    single, but_one, alt = rows % 3 == 0, rows % 3 == 1, rows % 3 == 2
    only = 2 + (rows // 3) % 6  # (every one of 2 .. 7 is some row's only action: the last lane of NO = 8 among them)
    mask[single] = 0
    mask[rows[single], only[single]] = 1
    mask[rows[but_one], (rows % 8)[but_one]] = 0
    mask[alt] = ((np.arange(8)[None, :] + rows[alt, None]) % 2).astype(np.uint8)
    init["action_mask"] = mask.reshape(c.E, c.A, 8)
    out = _launch(dev, c, params, init)
    assert _instance() == c.inst
    assert _same_bits(out["action_mask"][0], init["action_mask"]), "slot 0 of the mask belongs to the caller"
    a0, lp0 = out["action"][0].reshape(-1), out["log_prob"][0].reshape(-1)
    assert (mask[rows, a0] == 1).all(), "an action the caller masked was sampled at t = 0"
    assert np.array_equal(a0[single], only[single]) and (lp0[single] == 0.0).all()
    assert set(only[single].tolist()) == set(range(2, 8))
    assert len(np.unique(a0[but_one])) > 2 and len(np.unique(a0[alt])) > 2
    ref = M.rollout(c, *params, init, forced_action=out["action"])
    _check_against_model(c, out, ref, init, M.float_tolerance(c.name))


@pytest.mark.parametrize("name", ["s-A8-O17-n4", "d-A16-O48-n3"])
def test_inexact_slot0_takes_the_low_plane(dev, name):
    """Slot-0 observations with non-zero low f16 terms (1/3, 0.1, ...): the first step's values and log-probs still meet the
    bound against float64 of those inputs (without the low plane they miss by about 2^-11), the f16 records report themselves
    invalid, and the later steps - whose observations are exact again - match the model like any other launch."""
    c = M.CASE_BY_NAME[name]
    params, init = M.case_params(c), dict(M.case_init(c))
    rng = np.random.default_rng(c.O)
    raw = rng.choice(np.array([1 / 3, 0.1, 0.7, 2.3, 0.0, 1.0], np.float32), size=(c.E, c.A, c.O))
    assert (raw.astype(np.float16).astype(np.float32) != raw).mean() > 0.5
    av = np.array(init["agents_view"], np.float32)
    av[:, :, c.A :] = raw
    init["agents_view"], init["global_state"] = av, raw.reshape(c.E, 1, c.A * c.O)
    W = c.A + c.O
    opt = dict(view16=torch.zeros((c.T + 1, c.E, c.A, 8 * ((W + 8) // 8)), dtype=torch.float16, device=dev),
               view16_valid=torch.ones((1,), dtype=torch.int32, device=dev))
    if c.shared:
        assert (c.A * c.O) % 8 == 0
        opt.update(state16=torch.zeros((c.T + 1, c.E, 1, c.A * c.O), dtype=torch.float16, device=dev),
                   state16_valid=torch.ones((1,), dtype=torch.int32, device=dev))
    out = _launch(dev, c, params, init, **opt)
    assert _instance() == c.inst
    assert int(opt["view16_valid"].item()) == 0, "agents_view has low terms in slot 0: its word must read 0"
    if c.shared:
        assert int(opt["state16_valid"].item()) == 0, "the global state has low terms in slot 0: its word must read 0"
        assert _same_bits(out["global_state"][0], init["global_state"])
    ref = M.rollout(c, *params, init, forced_action=out["action"])
    tol = M.float_tolerance(c.name)
    print(f"{c.name}: t = 0 rel err value {_rel_err(out['value'][0], ref['value'][0]):.2e}, "
          f"log_prob {_rel_err(out['log_prob'][0], ref['log_prob'][0]):.2e}; t >= 1 value "
          f"{_rel_err(out['value'][1:], ref['value'][1:]):.2e}, log_prob {_rel_err(out['log_prob'][1:], ref['log_prob'][1:]):.2e}")
    assert_close(out["value"][0], ref["value"][0], tol, "value at t = 0")
    assert_close(out["log_prob"][0], ref["log_prob"][0], tol, "log_prob at t = 0")
    assert_close(out["value"][1:], ref["value"][1:], tol, "value at t >= 1")
    assert_close(out["log_prob"][1:], ref["log_prob"][1:], tol, "log_prob at t >= 1")
    _check_against_model(c, out, ref, init, tol)


# a shared case of three blocks (16 environments each: the 17-step instance) and a decentralised one (4 each), cut inside a block
@pytest.mark.parametrize("name,E,E1", [("s-A4-O64-n8", 37, 21), ("d-A16-O48-n3", 11, 3)])
def test_split_launches_equal_one_launch(dev, name, E, E1):
    """One launch over E environments against two over [0, E1) and [E1, E) with env_offset + E1 and row_offset + E1 * A: every
    output, adv and tgt included, bit for bit - environments land in other blocks and other tile rows, nothing else changes."""
    c = replace(M.CASE_BY_NAME[name], E=E)
    assert E1 % c.envs_per_block != 0 and -(-E // c.envs_per_block) >= 3
    params, init = M.case_params(c), M.case_init(c)
    whole = _launch(dev, c, params, init)
    assert _instance() == c.inst
    c1 = replace(c, E=E1)
    c2 = replace(c, E=E - E1, env_offset=c.env_offset + E1, row_offset=c.row_offset + E1 * c.A)
    p1 = _launch(dev, c1, params, M.slice_init(init, 0, E1))
    p2 = _launch(dev, c2, params, M.slice_init(init, E1, E))
    assert _instance() == c.inst
    assert not np.isnan(whole["adv"]).any() and whole["done"].max() == 1
    for k, v in whole.items():
        axis = 0 if (k in STATE or k == "last_val") else 1
        assert _same_bits(v, np.concatenate([p1[k], p2[k]], axis)), f"{k} differs between one launch and two"


@pytest.mark.parametrize("name", ["s-A32-O4-n7", "d-A1-O70-n5"])
def test_two_half_rollouts_equal_one(dev, name):
    """T = 8 in one launch against two launches of 4, the second with t0 + 4 after mava_rollout_carry moved slot 4 to slot 0:
    everything but adv / tgt (the first half bootstraps from another value) bit for bit."""
    from mava_amd import ops

    c = M.CASE_BY_NAME[name]
    params, init = M.case_params(c), M.case_init(c)
    whole = _launch(dev, c, params, init)
    h = replace(c, T=c.T // 2)
    pa, pc = _t(params[0], dev), _t(params[1], dev)
    b, st = _buffers(dev, h, init)
    assert _run(h, pa, pc, b, st)
    first = _numpy(b, st)
    ops.rollout_carry(b["agents_view"], b["global_state"], b["action_mask"], b["obs_step_count"])
    assert _run(replace(h, t0=c.t0 + h.T), pa, pc, b, st)
    second = _numpy(b, st)
    assert _instance() == c.inst
    for k in OBS:
        if k in whole:
            assert _same_bits(second[k][0], first[k][h.T]), f"{k}: slot T was not carried to slot 0"
            assert _same_bits(whole[k], np.concatenate([first[k], second[k][1:]], 0)), f"{k} differs"
    for k in STEP:
        assert _same_bits(whole[k], np.concatenate([first[k], second[k]], 0)), f"{k} differs"
    for k in STATE:
        assert _same_bits(whole[k], second[k]), f"{k} differs"
    assert _same_bits(whole["last_val"], second["last_val"])


@pytest.mark.parametrize("name", ["s-A4-O15-n5", "d-A64-O15-n6"])
def test_gae_outputs_are_optional(dev, name):
    c = M.CASE_BY_NAME[name]
    params, init = M.case_params(c), M.case_init(c)
    full = _launch(dev, c, params, init)
    bare = _launch(dev, c, params, init, with_gae=False)
    assert _instance() == c.inst and "adv" not in bare and not np.isnan(full["tgt"]).any()
    for k, v in bare.items():
        assert _same_bits(v, full[k]), f"{k} differs from the launch that also wrote adv / tgt"


@pytest.mark.parametrize("shape", M.REFUSED, ids=lambda s: "{}-A{}-O{}-n{}".format("s" if s[0] else "d", *s[1:]))
def test_refused_shapes_launch_nothing(dev, shape):
    """Shapes without an instance: rollout_ff returns False, every buffer keeps its sentinels and the caller's slot 0, and the
    instance diagnostic keeps its previous value."""
    shared, A, O, nA = shape
    assert M.predict_instance(*shape) is None
    c = M.Case("refused", shared, A, O, nA, 3, 0, t0=3, row_offset=37, env_offset=11, reward_mode=1, policy_seed=(5 << 32) | 42,
               env_seed=(9 << 32) | 7, T=2)
    init = M.case_init(c)
    rng = np.random.default_rng(0)
    pa = _t(rng.standard_normal(po.mlp_param_count(A + O, nA)).astype(np.float32), dev)
    pc = _t(rng.standard_normal(po.mlp_param_count(A * O if shared else A + O, 1)).astype(np.float32), dev)
    b, st = _buffers(dev, c, init)
    before, inst = _numpy(b, st), _instance()
    assert _run(c, pa, pc, b, st) is False
    assert _instance() == inst
    after = _numpy(b, st)
    for k, v in before.items():
        assert _same_bits(v, after[k]), f"{k} was written"
