"""The f16 record of the shared global state: written by the fused rollout (rollout_h2.hip, state16 / state16_valid), read by
the wide f16x2 critic gradient kernel's second staging path (ppo_train_h2.hip, TrainTask::x16) and plumbed through the learner
(MAVA_X16).  The record changes no bit of any result: every check here is torch.equal against the same launch without it, and
the handle's counters say which path ran."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

A = 4
WIDE18, WIDE12 = 2401184, 2401124  # ppo_train_h2_kernel<1, 18 | 12, critic, wide, XV = 4> (ppo_train_task.h train_instance_id)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _critic_inputs(rng, din, TE, exact=True):
    """Exact inputs: 0 / 1 flags and two small integers per row; otherwise normal-distributed (low f16 terms everywhere)."""
    if exact:
        gs = (rng.random((TE, din)) < 0.2).astype(np.float32)
        gs[:, :2] = rng.integers(0, 10, (TE, 2)).astype(np.float32)
    else:
        gs = rng.standard_normal((TE, din)).astype(np.float32)
    old_v = rng.standard_normal(TE * A).astype(np.float32)
    tgt = (old_v + rng.standard_normal(TE * A)).astype(np.float32)
    return gs, old_v, tgt


def _launch(dev, ctx, flat, gs, old_v, tgt, idx, idx_base, Rb, n_slab, x16=None, word=None):
    """One critic gradient launch on `ctx`; returns (slab, kernel instance, exact-loop tiles, launches on the f16 copy)."""
    from mava_amd import ops
    from mava_amd._lib import Ctx, lib

    ctx.set(Ctx.EXACT_TILES, 0)
    ctx.set(Ctx.X16_LAUNCHES, 0)
    slab = torch.zeros((n_slab, flat.size + 2), device=dev)
    valid = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
    ops.ppo_critic_grad(_t(flat, dev), _t(gs, dev), A, _t(old_v, dev), _t(tgt, dev), None if idx is None else _t(idx, dev),
                        idx_base, Rb, A, 0.2, 0.5, slab, ctx=ctx, input16=x16, input16_valid=valid)
    torch.cuda.synchronize()
    return slab, lib().mava_debug_train_last_instance(), ctx.get(Ctx.EXACT_TILES), ctx.get(Ctx.X16_LAUNCHES)


# (din, instance, Rb, n_slab, index vector?, idx_base): 264 / 261 rows = 9 tiles with a ragged last one - three per block (steady
# state, early layer 1 and tail all run) and 16 blocks (seven without a tile); the 12-step instance; consecutive rows from a base
CRITIC_CASES = [(264, WIDE18, 261, 3, True, 0), (264, WIDE18, 261, 16, True, 0), (176, WIDE12, 96, 2, True, 0),
                (264, WIDE18, 261, 3, False, 37)]


@pytest.mark.parametrize("din,instance,Rb,n_slab,use_idx,idx_base", CRITIC_CASES)
def test_critic_f16_path_equals_f32_path(dev, din, instance, Rb, n_slab, use_idx, idx_base):
    """Staging from the f16 copy against staging from the f32 rows: slabs (gradient rows and loss sums) bit for bit, the sum
    within the critic gradient tests' tolerance of the float64 model, the counters say the f16 path and the exact loop ran."""
    from mava_amd._lib import Ctx

    TE = 400
    rng = np.random.default_rng(din * 100 + Rb + n_slab)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    gs, _, _ = _critic_inputs(rng, din, TE)
    idx = rng.permutation(TE)[:Rb].astype(np.int32) if use_idx else None
    v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), gs.astype(np.float64))[:, 0]
    old_v = (np.repeat(v_now, A) + rng.standard_normal(TE * A) * 0.2).astype(np.float32)
    tgt = (np.repeat(v_now, A) + rng.standard_normal(TE * A)).astype(np.float32)
    x16 = _t(gs, dev).half()
    assert torch.equal(x16.float(), _t(gs, dev))
    ntiles = -(-Rb // 32)
    ctx = Ctx("f16x2")
    ref, inst_r, tiles_r, n16_r = _launch(dev, ctx, flat, gs, old_v, tgt, idx, idx_base, Rb, n_slab)
    got, inst_g, tiles_g, n16_g = _launch(dev, ctx, flat, gs, old_v, tgt, idx, idx_base, Rb, n_slab, x16, 1)
    ctx.close()
    assert inst_r == instance and inst_g == instance, "the wide f16x2 critic instantiation took both launches"
    assert (tiles_r, n16_r) == (ntiles, 0), "the f32 launch: every tile in the exact loop, the copy not read"
    assert n16_g == 1, "the launch with a valid copy did not take the f16 path"
    assert tiles_g == ntiles, f"{tiles_g} exact-loop tiles on the f16 path, {ntiles} tiles"
    assert torch.equal(got, ref), "slabs of the f16 path differ from the f32 path's"
    Pn = flat.size
    p_rows = idx.astype(np.int64) if use_idx else idx_base + np.arange(Rb, dtype=np.int64)
    rows = np.repeat(p_rows, A) * A + np.tile(np.arange(A), Rb)  # agent rows in launch order
    total = got.double().sum(0).cpu().numpy()
    _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, gs[rows // A].astype(np.float64),
                                          old_v[rows].astype(np.float64), tgt[rows].astype(np.float64), 0.2, 0.5)
    assert_close(total[:Pn], want, 1e-4, "critic grad")
    assert_close(total[Pn : Pn + 1], np.array([vl]), 1e-5, "value loss", scale=1.0)


@pytest.mark.parametrize("case", ["word0", "force_xlo", "din260"])
def test_copy_is_not_read_when_it_must_not_be(dev, case):
    """A copy full of NaN beside f32 rows that are not exact in f16: word 0, forced x_lo products (TRAIN_VARIANT bit 1) with word
    1, and an input width that is no multiple of 8 with word 1 all give the bits of a launch without the copy."""
    from mava_amd._lib import Ctx

    din = 260 if case == "din260" else 264
    TE, Rb, n_slab = 400, 261, 3
    rng = np.random.default_rng(din + len(case))
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    gs, old_v, tgt = _critic_inputs(rng, din, TE, exact=False)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    x16 = torch.full((TE, din), float("nan"), dtype=torch.float16, device=dev)
    ctx = Ctx("f16x2")
    if case == "force_xlo":
        ctx.set(Ctx.TRAIN_VARIANT, 2)
    ref, inst_r, _, _ = _launch(dev, ctx, flat, gs, old_v, tgt, idx, 0, Rb, n_slab)
    got, inst_g, _, n16 = _launch(dev, ctx, flat, gs, old_v, tgt, idx, 0, Rb, n_slab, x16, 0 if case == "word0" else 1)
    ctx.close()
    assert inst_r == WIDE18 and inst_g == WIDE18
    assert n16 == 0, "the f16 path ran"
    assert torch.isfinite(got).all() and torch.equal(got, ref), "the copy was read"


# ------------------------------------------------------------------------------------------------ rollout record
E_R, O_R, T_R, NA_R = 24, 66, 6, 5  # 16 envs per block: two blocks, the second half-full
GUARD = 64  # halves in front of and behind the record


def _rollout_init(rng):
    """Slot-0 observations of the synthetic env's kind (0 / 1 flags, counters 0..9, one-hot agent ids) and a fresh env state."""
    W, AO = A + O_R, A * O_R
    raw = (rng.random((E_R, A, O_R)) < 0.2).astype(np.float32)
    raw[:, :, :2] = rng.integers(0, 10, (E_R, A, 2)).astype(np.float32)
    av = np.zeros((E_R, A, W), np.float32)
    av[:, :, :A] = np.eye(A, dtype=np.float32)[None]
    av[:, :, A:] = raw
    gs = raw.reshape(E_R, 1, AO)
    mask = np.ones((E_R, A, NA_R), np.uint8)
    return av, gs, mask


def _run_rollout(dev, pa, pc, init, with16, poison=None):
    from mava_amd import ops

    av0, gs0, mask0 = init
    W, AO, T, E = A + O_R, A * O_R, T_R, E_R
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    b = dict(agents_view=z((T + 1, E, A, W)), global_state=z((T + 1, E, 1, AO)), action_mask=z((T + 1, E, A, NA_R), torch.uint8),
             obs_step_count=z((T + 1, E, A), torch.int32), action=z((T, E, A), torch.int32), value=z((T, E, A)), reward=z((T, E, A)),
             log_prob=z((T, E, A)), done=z((T, E, A), torch.uint8), last_val=z((E, A)), info_return=z((T, E)),
             info_length=z((T, E), torch.int32), info_terminal=z((T, E), torch.uint8), adv=z((T, E, A)), tgt=z((T, E, A)),
             last_reward=z((E, A)), last_done=z((E, A), torch.uint8))
    b["agents_view"][0] = _t(av0, dev)
    b["global_state"][0] = _t(gs0, dev)
    b["action_mask"][0] = _t(mask0, dev)
    if poison is not None:
        b["global_state"][0, poison[0], 0, poison[1]] = 0.1
    st = SimpleNamespace(step_count=z((E, A), torch.int32), run_return=z((E,)), run_length=z((E,), torch.int32), ep_return=z((E,)),
                         ep_length=z((E,), torch.int32))
    rec = valid = flat16 = None
    n16 = (T + 1) * E * AO
    if with16:
        flat16 = torch.full((n16 + 2 * GUARD,), float("nan"), dtype=torch.float16, device=dev)
        rec = flat16[GUARD : GUARD + n16].view(T + 1, E, 1, AO)
        valid = torch.zeros((1,), dtype=torch.int32, device=dev)
    ok = ops.rollout_ff(pa, pc, n_actions=NA_R, critic_shared=True, E=E, A=A, O=O_R, T=T, time_limit=4, policy_seed=42, env_seed=7,
                        t0=3, row_offset=0, env_offset=0, reward_mode=0, env_state=st, gamma=0.99, gae_lambda=0.95,
                        state16=rec, state16_valid=valid, **b)
    torch.cuda.synchronize()
    assert ok, "the fused rollout does not instantiate this shape"
    out = dict(b)
    out.update({f"state.{k}": v for k, v in vars(st).items()})
    return out, rec, valid, flat16


@pytest.fixture(scope="module")
def rollout_runs(dev):
    rng = np.random.default_rng(11)
    pa = _t(po.mlp_flatten(po.init_mlp(rng, A + O_R, NA_R, 1.0)).astype(np.float32), dev)
    pc = _t(po.mlp_flatten(po.init_mlp(rng, A * O_R, 1, 1.0)).astype(np.float32), dev)
    init = _rollout_init(rng)
    runs = {"plain": _run_rollout(dev, pa, pc, init, False), "x16": _run_rollout(dev, pa, pc, init, True)}
    poison = (19, 137)  # (env of the second block, state column)
    runs["plain_poisoned"] = _run_rollout(dev, pa, pc, init, False, poison)
    runs["x16_poisoned"] = _run_rollout(dev, pa, pc, init, True, poison)
    return runs


def test_rollout_record_equals_the_f32_state(dev, rollout_runs):
    from mava_amd._lib import lib

    assert lib().mava_debug_rollout_last_instance() == 805171  # rollout_h2_kernel<8, 5, 17, shared>: the headline instance
    out, rec, valid, flat16 = rollout_runs["x16"]
    n16 = rec.numel()
    assert int(valid.item()) == 1, "exact slot-0 state: the word must read 1"
    assert torch.equal(rec[:T_R].float(), out["global_state"][:T_R]), "float(state16) != global_state in slots 0 .. T-1"
    assert out["global_state"][:T_R].abs().sum().item() > 0
    assert torch.isnan(flat16[:GUARD]).all() and torch.isnan(flat16[GUARD + n16 :]).all(), "stores outside the record"
    ref = rollout_runs["plain"][0]
    for k, v in ref.items():
        assert torch.equal(v, out[k]), f"{k} differs from the launch without the record"


def test_rollout_word_is_zero_for_an_inexact_initial_state(dev, rollout_runs):
    out, rec, valid, flat16 = rollout_runs["x16_poisoned"]
    assert int(valid.item()) == 0, "0.1 in slot 0 of the f32 state: the word must read 0"
    assert torch.isnan(flat16[:GUARD]).all() and torch.isnan(flat16[GUARD + rec.numel() :]).all(), "stores outside the record"
    ref = rollout_runs["plain_poisoned"][0]
    for k, v in ref.items():
        assert torch.equal(v, out[k]), f"{k} differs from the launch without the record"
    assert float(out["global_state"][0, 19, 0, 137]) == pytest.approx(0.1), "slot 0 of the f32 state belongs to the caller"


# ------------------------------------------------------------------------------------------------ optional argument groups
E_C, T_C = 32, 8  # the learner test's shape below: 32 envs x 4 agents, T = 8
COMBOS = {"none": (False, False, False), "tail": (True, False, False), "tail+state16": (True, True, False),
          "tail+state16+view16": (True, True, True)}


def _run_combo(dev, pa, pc, init, tail, s16, v16):
    from mava_amd import ops

    av0, gs0, mask0 = init
    W, AO, T, E = A + O_R, A * O_R, T_C, E_C
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    b = dict(agents_view=z((T + 1, E, A, W)), global_state=z((T + 1, E, 1, AO)), action_mask=z((T + 1, E, A, NA_R), torch.uint8),
             obs_step_count=z((T + 1, E, A), torch.int32), action=z((T, E, A), torch.int32), value=z((T, E, A)), reward=z((T, E, A)),
             log_prob=z((T, E, A)), done=z((T, E, A), torch.uint8), last_val=z((E, A)), info_return=z((T, E)),
             info_length=z((T, E), torch.int32), info_terminal=z((T, E), torch.uint8), adv=z((T, E, A)), tgt=z((T, E, A)))
    b["agents_view"][0], b["global_state"][0], b["action_mask"][0] = _t(av0, dev), _t(gs0, dev), _t(mask0, dev)
    st = SimpleNamespace(step_count=z((E, A), torch.int32), run_return=z((E,)), run_length=z((E,), torch.int32), ep_return=z((E,)),
                         ep_length=z((E,), torch.int32))
    opt = {}
    if tail:
        opt.update(last_reward=z((E, A)), last_done=z((E, A), torch.uint8), step_counter=z((1,), torch.int32))
    if s16:
        opt.update(state16=z((T + 1, E, 1, AO), torch.float16), state16_valid=z((1,), torch.int32))
    if v16:
        opt.update(view16=z((T + 1, E, A, 8 * ((W + 8) // 8)), torch.float16), view16_valid=z((1,), torch.int32))
    ok = ops.rollout_ff(pa, pc, n_actions=NA_R, critic_shared=True, E=E, A=A, O=O_R, T=T, time_limit=4, policy_seed=42, env_seed=7,
                        t0=3, row_offset=0, env_offset=0, reward_mode=0, env_state=st, gamma=0.99, gae_lambda=0.95, **opt, **b)
    torch.cuda.synchronize()
    assert ok, "the fused rollout does not instantiate this shape"
    return dict(b, **opt, **{f"state.{k}": v for k, v in vars(st).items()})


@pytest.fixture(scope="module")
def combo_runs(dev):
    rng = np.random.default_rng(13)
    pa = _t(po.mlp_flatten(po.init_mlp(rng, A + O_R, NA_R, 1.0)).astype(np.float32), dev)
    pc = _t(po.mlp_flatten(po.init_mlp(rng, A * O_R, 1, 1.0)).astype(np.float32), dev)
    raw = (rng.random((E_C, A, O_R)) < 0.2).astype(np.float32)
    raw[:, :, :2] = rng.integers(0, 10, (E_C, A, 2)).astype(np.float32)
    av = np.concatenate([np.broadcast_to(np.eye(A, dtype=np.float32), (E_C, A, A)), raw], axis=2)
    init = (av, raw.reshape(E_C, 1, A * O_R), np.ones((E_C, A, NA_R), np.uint8))
    return {name: _run_combo(dev, pa, pc, init, *flags) for name, flags in COMBOS.items()}


@pytest.mark.parametrize("name", [n for n in COMBOS if n != "tail+state16+view16"])
def test_rollout_optional_groups_change_no_common_output(combo_runs, name):
    """mava_rollout_ff_f32 with each subset of its optional output groups that a caller passes - none, the tail outputs, the tail
    and state16 - against the launch with all of them: every output both launches write is the same bit for bit."""
    full, out = combo_runs["tail+state16+view16"], combo_runs[name]
    assert int(full["step_counter"].item()) == T_C and int(full["state16_valid"].item()) == int(full["view16_valid"].item()) == 1
    assert full["reward"].abs().sum().item() > 0 and full["done"].sum().item() > 0 and full["agents_view"][1:].abs().sum().item() > 0
    assert torch.equal(full["last_reward"], full["reward"][T_C - 1]) and torch.equal(full["last_done"], full["done"][T_C - 1])
    assert len(out) == 20 + 3 * COMBOS[name][0] + 2 * COMBOS[name][1]
    for k, v in out.items():
        assert torch.equal(v, full[k]), f"{k} differs from the launch with every optional group"


# ------------------------------------------------------------------------------------------------ one learner update
def _update_once(dev, monkeypatch, x16, U):
    from mava_amd import envs
    from mava_amd._lib import Ctx
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    monkeypatch.setenv("MAVA_X16", x16)
    monkeypatch.setenv("MAVA_FUSED_ROLLOUT", "1")
    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    E, T, K, M = 32, 8, 2, 2
    cfg = compose("default_ff_mappo", [f"arch.num_envs={E}", f"system.rollout_length={T}", f"system.ppo_epochs={K}",
                                       f"system.num_minibatches={M}", f"system.update_batch_size={U}"])
    cfg.env.scenario.task_config.num_agents = A
    cfg.system.num_updates_per_eval = 1
    cfg.env.kwargs.time_limit = 5
    env, _ = envs.make(cfg, add_global_state=True, device=dev)
    learn, _, state = ff_mappo.learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    assert L.fused_rollout and L.x16 == (x16 == "1") and L.Oc == 264
    L.update(0)
    torch.cuda.synchronize()
    assert L.fused_rollout, "the fused rollout served the update"
    n16 = L.ctx.get(Ctx.X16_LAUNCHES)
    if x16 == "1":
        for rep in L.reps:
            assert int(rep.state16_valid.item()) == 1
            # (slot 0 of the f32 state already holds the next rollout's first observation: update() ends with the carry)
            assert torch.equal(rep.state16[1:T].float(), rep.global_state[1:T])
    return {"p": L.p.clone(), "m": L.m.clone(), "v": L.v.clone(), "train_metrics": L.train_metrics.clone()}, n16, K * M * U


@pytest.mark.parametrize("U", [1, 2])
def test_learner_update_same_bits_with_and_without_the_record(dev, monkeypatch, U):
    """One ff_mappo update (two epochs x two minibatches) from the same state with MAVA_X16=0 and =1: parameters, both Adam
    moments and the train metrics bit for bit; every critic launch of the =1 run on the f16 path, none of the =0 run."""
    off, n_off, _ = _update_once(dev, monkeypatch, "0", U)
    on, n_on, launches = _update_once(dev, monkeypatch, "1", U)
    assert n_off == 0, "MAVA_X16=0: a critic launch read an f16 copy"
    assert n_on == launches, f"MAVA_X16=1: {n_on} of {launches} critic launches on the f16 path"
    for k in off:
        assert torch.equal(off[k], on[k]), f"{k} differs between MAVA_X16=0 and =1"
