"""The f16 record of agents_view: written by the fused rollout (rollout_h2.hip, view16 / view16_valid), read by the eight-wave
f16x2 gradient kernel's second staging body (ppo_train_w8.hip, TrainTask::x16 with x16_ld) and plumbed through the learner
(MAVA_X16_ACTOR).  The record changes no bit of any result: every check here is torch.equal against the same launch without it,
and the handle's counter says which body ran."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

A = 4
TE = 400


def _w8_id(actor, no_pad, s1, xv):
    """ppo_train_w8_kernel<NO, S1, XV, ., ACTOR> as mava_debug_train_last_instance() reports it (ppo_train_task.h)."""
    return 3000000 + (100000 if actor else 0) + no_pad * 1000 + s1 * 10 + xv


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rp(din):
    return 8 * ((din + 8) // 8)


def _exact_rows(rng, rows, din):
    """Rows of the synthetic env's kind, exact in f16: a one-hot agent id, two integers 0..9, 0 / 1 flags."""
    x = (rng.random((rows, din)) < 0.2).astype(np.float32)
    x[:, :A] = np.eye(A, dtype=np.float32)[np.arange(rows) % A]
    x[:, A : A + 2] = rng.integers(0, 10, (rows, 2)).astype(np.float32)
    return x


def _record(x, dev, fill=None):
    """The record of x as the rollout writes it: din halves, 1.0, zeros up to RP (or `fill` everywhere)."""
    rows, din = x.shape
    rec = torch.zeros((rows, _rp(din)), dtype=torch.float16, device=dev)
    if fill is not None:
        rec.fill_(fill)
        return rec
    rec[:, :din] = _t(x, dev).half()
    rec[:, din] = 1.0
    assert torch.equal(rec[:, :din].float(), _t(x, dev))
    return rec


def _actor_data(rng, din, nA, exact=True):
    rows = TE * A
    av = _exact_rows(rng, rows, din) if exact else rng.standard_normal((rows, din)).astype(np.float32)
    flat = po.mlp_flatten(po.init_mlp(rng, din, nA, 0.01)).astype(np.float32)
    mask = np.ones((rows, nA), np.uint8)
    mask[:, 1] = rng.random(rows) > 0.2
    y = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, nA), av.astype(np.float64))
    logp = po.log_softmax(po.masked_logits(y, mask))
    action = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int32)
    old_lp = (logp[np.arange(rows), action] + rng.standard_normal(rows) * 0.1).astype(np.float32)
    adv = rng.standard_normal(rows).astype(np.float32)
    return SimpleNamespace(din=din, nA=nA, av=av, flat=flat, mask=mask, action=action, old_lp=old_lp, adv=adv)


def _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab, rec=None, word=None):
    """One actor gradient launch on `ctx`; returns (slab, kernel instance, eight-wave launches on the record)."""
    from mava_amd import ops
    from mava_amd._lib import Ctx, lib

    ctx.set(Ctx.X16_W8_LAUNCHES, 0)
    slab = torch.zeros((n_slab, d.flat.size + 2), device=dev)
    valid = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
    adv, idx_d = _t(d.adv, dev), None if idx is None else _t(idx, dev)
    stats = ops.adv_stats(adv, idx_d, idx_base, Rb, A)
    ops.ppo_actor_grad(_t(d.flat, dev), _t(d.av, dev), _t(d.mask, dev), _t(d.action, dev), _t(d.old_lp, dev), adv, stats, idx_d,
                       idx_base, Rb, A, d.nA, 0.2, 0.01, slab, ctx=ctx, input16=rec, input16_valid=valid)
    torch.cuda.synchronize()
    return slab, lib().mava_debug_train_last_instance(), ctx.get(Ctx.X16_W8_LAUNCHES)


def _launch_rows(idx, idx_base, Rb):
    p_rows = idx.astype(np.int64) if idx is not None else idx_base + np.arange(Rb, dtype=np.int64)
    return np.repeat(p_rows, A) * A + np.tile(np.arange(A), Rb)  # agent rows in launch order


# (din, actions, instance, Rb, n_slab, index vector?, idx_base): 65 x 4 = 260 rows = 9 tiles with a ragged last one - three per
# block, or 16 blocks of which seven have none; consecutive rows from a base; one, two (exactly eight chunks: no second load),
# three and four 32-input steps; 11 actions: sixteen loss lanes, every thread stages (ROLE 0)
ACTOR_CASES = [
    (70, 5, _w8_id(True, 8, 3, 2), 65, 3, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 16, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 3, False, 37),
    (30, 5, _w8_id(True, 8, 1, 2), 65, 3, True, 0),
    (62, 5, _w8_id(True, 8, 2, 2), 65, 3, True, 0),
    (94, 5, _w8_id(True, 8, 3, 2), 65, 3, True, 0),
    (126, 5, _w8_id(True, 8, 4, 2), 65, 3, True, 0),
    (70, 11, _w8_id(True, 16, 3, 2), 65, 3, True, 0),
]


@pytest.mark.parametrize("din,nA,instance,Rb,n_slab,use_idx,idx_base", ACTOR_CASES)
def test_actor_f16_path_equals_f32_path(dev, din, nA, instance, Rb, n_slab, use_idx, idx_base):
    """Staging from the f16 record against staging from the f32 rows: slabs (gradient rows and loss sums) bit for bit, the sum
    within the actor gradient tests' tolerance of the float64 model, the counter says the record was read."""
    from mava_amd._lib import Ctx

    rng = np.random.default_rng(din * 100 + nA + n_slab + idx_base)
    d = _actor_data(rng, din, nA)
    idx = rng.permutation(TE)[:Rb].astype(np.int32) if use_idx else None
    rec = _record(d.av, dev)
    ctx = Ctx("f16x2")
    ref, inst_r, n16_r = _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab)
    got, inst_g, n16_g = _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab, rec, 1)
    ctx.close()
    assert inst_r == instance and inst_g == instance, "the eight-wave instantiation took both launches"
    assert n16_r == 0, "a launch without a record counted one"
    assert n16_g == 1, "the launch with a valid record did not stage from it"
    assert torch.equal(got, ref), "slabs of the f16 path differ from the f32 path's"
    rows = _launch_rows(idx, idx_base, Rb)
    P = d.flat.size
    total = got.double().sum(0).cpu().numpy()
    _, la, ent, want = po.actor_loss_and_grad(d.flat.astype(np.float64), din, nA, d.av[rows].astype(np.float64), d.mask[rows],
                                              d.action[rows], d.old_lp[rows].astype(np.float64), d.adv[rows].astype(np.float64),
                                              0.2, 0.01)
    assert_close(total[:P], want, 1e-4, "actor grad")
    assert_close(total[P : P + 2], np.array([la, ent]), 1e-5, "actor loss sums", scale=1.0)


def _launch_critic(dev, ctx, flat, x, old_v, tgt, idx, Rb, n_slab, rec=None, word=None):
    from mava_amd import ops
    from mava_amd._lib import Ctx, lib

    ctx.set(Ctx.X16_W8_LAUNCHES, 0)
    slab = torch.zeros((n_slab, flat.size + 2), device=dev)
    valid = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
    ops.ppo_critic_grad(_t(flat, dev), _t(x, dev), 1, _t(old_v, dev), _t(tgt, dev), _t(idx, dev), 0, Rb, A, 0.2, 0.5, slab, ctx=ctx,
                        input16=rec, input16_valid=valid)
    torch.cuda.synchronize()
    return slab, lib().mava_debug_train_last_instance(), ctx.get(Ctx.X16_W8_LAUNCHES)


def test_narrow_critic_f16_path_equals_f32_path(dev):
    """The value network on agents_view (one input row per agent row: x_share = 1) runs on the same kernel and reads the same
    record."""
    from mava_amd._lib import Ctx

    din, Rb, n_slab = 70, 65, 3
    rng = np.random.default_rng(7070)
    rows = TE * A
    x = _exact_rows(rng, rows, din)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), x.astype(np.float64))[:, 0]
    old_v = (v_now + rng.standard_normal(rows) * 0.2).astype(np.float32)
    tgt = (v_now + rng.standard_normal(rows)).astype(np.float32)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    ctx = Ctx("f16x2")
    ref, inst_r, n16_r = _launch_critic(dev, ctx, flat, x, old_v, tgt, idx, Rb, n_slab)
    got, inst_g, n16_g = _launch_critic(dev, ctx, flat, x, old_v, tgt, idx, Rb, n_slab, _record(x, dev), 1)
    ctx.close()
    assert inst_r == inst_g == _w8_id(False, 8, 3, 2), "the eight-wave critic instantiation took both launches"
    assert (n16_r, n16_g) == (0, 1)
    assert torch.equal(got, ref), "slabs of the f16 path differ from the f32 path's"
    r = _launch_rows(idx, 0, Rb)
    Pn = flat.size
    total = got.double().sum(0).cpu().numpy()
    _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, x[r].astype(np.float64), old_v[r].astype(np.float64),
                                          tgt[r].astype(np.float64), 0.2, 0.5)
    assert_close(total[:Pn], want, 1e-4, "critic grad")
    assert_close(total[Pn : Pn + 1], np.array([vl]), 1e-5, "value loss", scale=1.0)


@pytest.mark.parametrize("case", ["word0", "force_xlo", "odd_din", "base_plus_8_bytes"])
def test_record_is_not_read_when_it_must_not_be(dev, case):
    """A record full of NaN beside f32 rows that are not exact in f16: word 0, forced x_lo products (TRAIN_VARIANT bit 1) with
    word 1, an odd input width (the XV = 1 instance) with word 1 and a record base 8 bytes off a 16-byte boundary with word 1 all
    give the bits of a launch without the record."""
    from mava_amd._lib import Ctx

    din = 69 if case == "odd_din" else 70
    Rb, n_slab = 65, 3
    rng = np.random.default_rng(din + len(case))
    d = _actor_data(rng, din, 5, exact=False)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    rows, rp = TE * A, _rp(din)
    if case == "base_plus_8_bytes":
        store = torch.full((rows * rp + 8,), float("nan"), dtype=torch.float16, device=dev)
        rec = store[4 : 4 + rows * rp].view(rows, rp)
        assert rec.data_ptr() % 16 == 8
    else:
        rec = _record(d.av, dev, fill=float("nan"))
        assert rec.data_ptr() % 16 == 0
    ctx = Ctx("f16x2")
    if case == "force_xlo":
        ctx.set(Ctx.TRAIN_VARIANT, 2)
    ref, inst_r, _ = _launch_actor(dev, ctx, d, idx, 0, Rb, n_slab)
    got, inst_g, n16 = _launch_actor(dev, ctx, d, idx, 0, Rb, n_slab, rec, 0 if case == "word0" else 1)
    ctx.close()
    want_inst = _w8_id(True, 8, 3, 1 if case == "odd_din" else 2)
    assert inst_r == want_inst and inst_g == want_inst
    assert n16 == 0, "the record was staged"
    assert torch.isfinite(got).all() and torch.equal(got, ref), "the record was read"


# ------------------------------------------------------------------------------------------------ rollout record
E_R, O_R, T_R, NA_R = 24, 66, 6, 5
GUARD = 64  # halves in front of and behind the record
ROLLOUT_CASES = {"shared_A4": (4, True, 805171), "shared_A2": (2, True, 805091), "decentralised_A4": (4, False, 805050)}


def _rollout_init(rng, Ar):
    W = Ar + O_R
    raw = (rng.random((E_R, Ar, O_R)) < 0.2).astype(np.float32)
    raw[:, :, :2] = rng.integers(0, 10, (E_R, Ar, 2)).astype(np.float32)
    av = np.zeros((E_R, Ar, W), np.float32)
    av[:, :, :Ar] = np.eye(Ar, dtype=np.float32)[None]
    av[:, :, Ar:] = raw
    return av, raw.reshape(E_R, 1, Ar * O_R), np.ones((E_R, Ar, NA_R), np.uint8)


def _run_rollout(dev, pa, pc, init, Ar, shared, state16=False, view16=False, word_in=0, plant=None):
    from mava_amd import ops

    av0, gs0, mask0 = init
    W, AO, T, E = Ar + O_R, Ar * O_R, T_R, E_R
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    b = dict(agents_view=z((T + 1, E, Ar, W)), action_mask=z((T + 1, E, Ar, NA_R), torch.uint8),
             obs_step_count=z((T + 1, E, Ar), torch.int32), action=z((T, E, Ar), torch.int32), value=z((T, E, Ar)),
             reward=z((T, E, Ar)), log_prob=z((T, E, Ar)), done=z((T, E, Ar), torch.uint8), last_val=z((E, Ar)),
             info_return=z((T, E)), info_length=z((T, E), torch.int32), info_terminal=z((T, E), torch.uint8), adv=z((T, E, Ar)),
             tgt=z((T, E, Ar)), last_reward=z((E, Ar)), last_done=z((E, Ar), torch.uint8))
    b["global_state"] = z((T + 1, E, 1, AO)) if shared else None
    b["agents_view"][0] = _t(av0, dev)
    b["action_mask"][0] = _t(mask0, dev)
    if shared:
        b["global_state"][0] = _t(gs0, dev)
    if plant is not None:
        b["agents_view"][0, plant[0], plant[1], plant[2]] = 1.0 + 2.0 ** -12
    st = SimpleNamespace(step_count=z((E, Ar), torch.int32), run_return=z((E,)), run_length=z((E,), torch.int32), ep_return=z((E,)),
                         ep_length=z((E,), torch.int32))
    kw, rec, valid, store = {}, None, None, None
    if state16:
        kw["state16"] = torch.zeros((T + 1, E, 1, AO), dtype=torch.float16, device=dev)
        kw["state16_valid"] = z((1,), torch.int32)
    if view16:
        rp = _rp(W)
        n16 = (T + 1) * E * Ar * rp
        store = torch.full((n16 + 2 * GUARD,), float("nan"), dtype=torch.float16, device=dev)
        rec = store[GUARD : GUARD + n16].view(T + 1, E, Ar, rp)
        valid = torch.full((1,), word_in, dtype=torch.int32, device=dev)
        kw["view16"], kw["view16_valid"] = rec, valid
    ok = ops.rollout_ff(pa, pc, n_actions=NA_R, critic_shared=shared, E=E, A=Ar, O=O_R, T=T, time_limit=4, policy_seed=42, env_seed=7,
                        t0=3, row_offset=0, env_offset=0, reward_mode=0, env_state=st, gamma=0.99, gae_lambda=0.95, **kw, **b)
    torch.cuda.synchronize()
    assert ok, "the fused rollout does not instantiate this shape"
    out = {k: v for k, v in b.items() if v is not None}
    out.update({f"state.{k}": v for k, v in vars(st).items()})
    if state16:
        out["state16"], out["state16_valid"] = kw["state16"], kw["state16_valid"]
    return out, rec, valid, store


@pytest.mark.parametrize("name", list(ROLLOUT_CASES))
def test_rollout_record(dev, name):
    """view16 holds the halves of agents_view in all T + 1 slots, then 1.0, then zeros; its word is 1; nothing is stored outside
    it; every other output equals the launch without it and the launch with state16 alone; a slot-0 value with a low f16 term in the
    last block turns an entry word of 1 into 0, exact inputs turn an entry word of 0 into 1."""
    from mava_amd._lib import lib

    Ar, shared, instance = ROLLOUT_CASES[name]
    W = Ar + O_R
    rng = np.random.default_rng(11 + Ar)
    pa = _t(po.mlp_flatten(po.init_mlp(rng, W, NA_R, 1.0)).astype(np.float32), dev)
    pc = _t(po.mlp_flatten(po.init_mlp(rng, Ar * O_R if shared else W, 1, 1.0)).astype(np.float32), dev)
    init = _rollout_init(rng, Ar)
    s16 = shared and (Ar * O_R) % 8 == 0  # (state16 needs whole 16-byte chunks of the shared state: not with two agents)
    plain, _, _, _ = _run_rollout(dev, pa, pc, init, Ar, shared)
    out, rec, valid, store = _run_rollout(dev, pa, pc, init, Ar, shared, state16=s16, view16=True, word_in=0)
    assert lib().mava_debug_rollout_last_instance() == instance
    n16 = rec.numel()
    assert int(valid.item()) == 1, "exact slot-0 observations and an entry word of 0: the word must read 1"
    assert torch.equal(rec[..., :W].float(), out["agents_view"]), "float(view16) != agents_view"
    assert out["agents_view"][1:].abs().sum().item() > 0
    assert (rec[..., W] == 1).all(), "the ones column"
    assert (rec[..., W + 1 :] == 0).all(), "the padding behind the ones column"
    assert torch.isnan(store[:GUARD]).all() and torch.isnan(store[GUARD + n16 :]).all(), "stores outside the record"
    for k, v in plain.items():
        assert torch.equal(v, out[k]), f"{k} differs from the launch without the records"
    if s16:
        only_s16, _, _, _ = _run_rollout(dev, pa, pc, init, Ar, shared, state16=True)
        assert int(only_s16["state16_valid"].item()) == 1
        for k, v in only_s16.items():
            assert torch.equal(v, out[k]), f"{k} differs from the launch with state16 alone"
        alone, rec_a, valid_a, _ = _run_rollout(dev, pa, pc, init, Ar, shared, view16=True)  # (each pair is nullable on its own)
        assert int(valid_a.item()) == 1 and torch.equal(rec_a, rec)
        for k, v in plain.items():
            assert torch.equal(v, alone[k]), f"{k} differs between view16 alone and no record"
    # a low f16 term in slot 0, in the last block (env 19 of 24: 16 or 32 envs per block), agent 1, a flag column
    bad, rec_b, valid_b, store_b = _run_rollout(dev, pa, pc, init, Ar, shared, state16=s16, view16=True, word_in=1,
                                                plant=(19, 1, Ar + 9))
    assert int(valid_b.item()) == 0, "1 + 2^-12 in slot 0 of agents_view: the word must read 0"
    assert torch.isnan(store_b[:GUARD]).all() and torch.isnan(store_b[GUARD + n16 :]).all(), "stores outside the record"
    assert float(bad["agents_view"][0, 19, 1, Ar + 9]) == 1.0 + 2.0 ** -12, "slot 0 of agents_view belongs to the caller"


# ------------------------------------------------------------------------------------------------ learner
def _leaves(prefix, x):
    if isinstance(x, torch.Tensor):
        yield prefix, x
    elif hasattr(x, "_fields"):
        for k in x._fields:
            yield from _leaves(f"{prefix}.{k}", getattr(x, k))
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _leaves(f"{prefix}.{k}", v)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(f"{prefix}.{i}", v)


def _learn_three_updates(dev, monkeypatch, system, actor_switch):
    import importlib

    from mava_amd import envs
    from mava_amd._lib import Ctx
    from mava_amd.config import compose

    monkeypatch.setenv("MAVA_X16", "1")
    monkeypatch.setenv("MAVA_X16_ACTOR", actor_switch)
    monkeypatch.setenv("MAVA_FUSED_ROLLOUT", "1")
    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    E, T, K, M, N = 32, 4, 2, 2, 3
    cfg = compose(f"default_{system}", [f"arch.num_envs={E}", f"system.rollout_length={T}", f"system.ppo_epochs={K}",
                                        f"system.num_minibatches={M}", "system.update_batch_size=1"])
    cfg.env.scenario.task_config.num_agents = A
    cfg.system.num_updates_per_eval = N
    cfg.env.kwargs.time_limit = 5
    mod = importlib.import_module(f"mava_amd.systems.ppo.{system}")
    env, _ = envs.make(cfg, add_global_state=system == "ff_mappo", device=dev)
    learn, _, state = mod.learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    assert L.fused_rollout and L.view16 == (actor_switch == "1") and L.Oa == 70
    out = learn(state)
    torch.cuda.synchronize()
    assert L.fused_rollout, "the fused rollout served the updates"
    if actor_switch == "1":
        for rep in L.reps:
            assert int(rep.view16_valid.item()) == 1
    leaves = {k: v.clone() for k, v in _leaves("out", out)}
    assert len(leaves) > 10
    return leaves, L.ctx.get(Ctx.X16_W8_LAUNCHES), N * K * M


@pytest.mark.parametrize("system", ["ff_mappo", "ff_ippo"])
def test_learner_same_bits_with_and_without_the_record(dev, monkeypatch, system):
    """Three updates from the same state with MAVA_X16_ACTOR=0 and with the default: every leaf of the returned learner state and
    metrics bit for bit; with the record every eight-wave launch stages from it (the actor's K x M per update, and under ff_ippo the
    critic's as many again), without it none."""
    off, n_off, _ = _learn_three_updates(dev, monkeypatch, system, "0")
    on, n_on, launches = _learn_three_updates(dev, monkeypatch, system, "1")
    want = launches * (2 if system == "ff_ippo" else 1)
    assert n_off == 0, "MAVA_X16_ACTOR=0: an eight-wave launch read a record"
    assert n_on == want, f"{n_on} of {want} eight-wave launches staged from the record"
    assert off.keys() == on.keys()
    for k in off:
        assert torch.equal(off[k], on[k]), f"{k} differs between MAVA_X16_ACTOR=0 and the default"
