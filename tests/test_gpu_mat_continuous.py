"""GPU: ff_mat with a ContinuousActionHead against the float64 model of tests/mat_continuous_model.py - the three kernels of
csrc/mat.hip (shifted actions, per-agent sampling, loss) through the C ABI, autoregressive acting and learn() on env=spread layer by
layer and with the fused step (csrc/mat_act.hip's continuous instance), and run_experiment with its checkpoint.

Tolerances (conftest.assert_close): 1e-5 actions, log-probs, values and losses, 1e-4 gradients except where float32 itself does not
reach it (test_loss_kernel), whole updates as tests/test_gpu_mat.py.  A later agent's mean depends on the earlier agents' actions, so
acting is compared agent by agent given the RECORDED earlier actions (the model's `forced`): float32 differences do not compound.
"""
import functools
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_mat as tgm
from oracle import tanh_normal as tn
from tests import mat_continuous_model as mc
from tests import seq_model as sm
from tests.conftest import assert_close
from tests.test_gpu_mat_fused_act import _Calls

pytestmark = pytest.mark.gpu

SENT = 12345.0
c32 = lambda n: -(-n // 32) * 32


def _lib():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return check, lib(), ptr, stream_ptr


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _t32(a, rows, dev):
    """(r, N) float32 numpy -> T32 (rows x N) on the device; the padding rows hold 7.0: they must not leak."""
    full = np.full((rows, a.shape[1]), 7.0, np.float32)
    full[: a.shape[0]] = a
    return _d(sm.to_t32(full), dev)


def _out(n, dev, guard=32 * 32):
    """n floats of sentinel and a guard tile of sentinel behind them."""
    return torch.full((int(n) + guard,), SENT, device=dev)


def _take(t, n, what):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert (a[n:] == np.float32(SENT)).all(), f"{what}: wrote past its {n} elements"
    return a[:n]


def _bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all(), f"{what}: not bit-identical"


# ---- 1. shifted actions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", mc.DIMS)
def test_shift_action_is_bit_exact(dev, d):
    check, L, ptr, sp = _lib()
    g = torch.Generator().manual_seed(d)
    for B, A in ((1, 1), (11, 3), (7, 5)):
        rows, Np, TE = c32(A * B), c32(d), B + 4
        action = torch.tanh(torch.randn((TE, A, d), generator=g)).float()
        idx = torch.randperm(TE, generator=g)[:B].to(torch.int32)
        d_action, d_idx = action.to(dev), idx.to(dev)
        for known in sorted({0, min(1, A - 1), A - 1}):
            for use_idx in (False, True):
                out = _out(rows * Np, dev)
                check(L.mava_transformer_shift_action_f32(ptr(d_action), ptr(d_idx) if use_idx else None, B, A, d, known, rows, Np, ptr(out),
                                                          sp()), "shift_action")
                src = action[idx.long()] if use_idx else action[:B]
                want = np.zeros((rows, Np), np.float32)  # padding rows and padding features come back zero
                want[: A * B, :d] = mc.shifted_action(src, known).view(A * B, d).float().numpy()
                got = sm.from_t32(_take(out, rows * Np, "shifted actions"), rows, Np)
                _bits(got, want, f"d={d} B={B} A={A} known={known} idx={use_idx}")


# ---- 2. sampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("d", mc.DIMS)
def test_sample_kernel(dev, d, row_offset):
    check, L, ptr, sp = _lib()
    B, A, step = 43, 3, 5
    rng = np.random.default_rng(100 + d)
    R, rows = B * A, c32(B * A)
    mean, log_std = np.float32(rng.standard_normal((R, d)) * 0.5), np.float32(rng.standard_normal(d) * 0.5)
    scale = tn.softplus(log_std.astype(np.float64)) + tn.MIN_SCALE
    noise = tn.normal_noise(mc.SEED, step, R, d, tn.STREAM_SAMPLE, row_offset).astype(np.float64)
    m_d, ls_d = _t32(mean, rows, dev), _d(log_std, dev)
    for greedy in (0, 1):
        eps = np.zeros_like(noise) if greedy else noise
        want = np.tanh(mean.astype(np.float64) + scale * eps)
        for agent in range(A):
            act, lp = _out(R * d, dev), _out(R, dev)
            check(L.mava_transformer_sample_continuous_f32(B, A, agent, d, tn.MIN_SCALE, ptr(m_d), ptr(ls_d), mc.SEED, step, row_offset, greedy,
                                                           ptr(act), ptr(lp), sp()), "sample_continuous")
            a_, lp_ = _take(act, R * d, "action").reshape(R, d), _take(lp, R, "log_prob")
            own = np.zeros(R, bool)
            own[agent::A] = True
            assert (a_[~own] == np.float32(SENT)).all() and (lp_[~own] == np.float32(SENT)).all(), f"agent {agent}: wrote other agents' entries"
            assert_close(a_[own], want[own], 1e-5, f"action of agent {agent} (greedy={greedy})")
            lp_want = tn.log_prob_terms(a_[own], mean[own], np.broadcast_to(scale, (own.sum(), d)))[0].sum(-1)
            assert_close(lp_[own], lp_want, 1e-5, f"log_prob of the kernel's own action, agent {agent} (greedy={greedy})")


# ---- 3. loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.LOSS_SHAPES, ids=lambda s: f"Bm{s[0]}xA{s[1]}")
@pytest.mark.parametrize("d", mc.DIMS)
def test_loss_kernel(dev, d, shape):
    """The gradient bound is mat_continuous_model.loss_grad_bound: the project's 1e-4 wherever the float32 NumPy evaluation of the loss
    head stays inside it on the case's inputs (at most 1.4e-05 on 19 of the 20 cases), and four times the case's measured float32 floor
    where it does not: 1.56e-04 at d = 8, (Bm, A) = (7, 5), so 6.2e-04 there (tests/test_mat_continuous_model.py measures both)."""
    check, L, ptr, sp = _lib()
    for row_offset in (0, 1000):
        c = mc.loss_case(d, *shape, row_offset)
        Bm, A, R, rows, w = c["Bm"], c["A"], c["R"], c["rows"], c["want"]
        bound, gscale = mc.loss_grad_bound(c), 256.0
        dv = {k: _d(c[k], dev) for k in ("idx", "log_std", "action", "old_lp", "adv", "old_value", "target", "stats")}
        m_d, v_d = _t32(c["mean"], rows, dev), _t32(c["values"][:, None], rows, dev)
        ref = None
        for nb in (1, 2):
            dm, dvl, part, dls = _out(rows * d, dev), _out(rows, dev), _out(3 * nb, dev), _out(nb * d, dev)
            check(L.mava_transformer_loss_continuous_f32(Bm, A, d, tn.MIN_SCALE, rows, ptr(dv["idx"]), ptr(m_d), ptr(dv["log_std"]), ptr(v_d),
                                                         ptr(dv["action"]), ptr(dv["old_lp"]), ptr(dv["adv"]), ptr(dv["old_value"]),
                                                         ptr(dv["target"]), ptr(dv["stats"]), c["stats"].shape[0], mc.CLIP, mc.ENT_COEF,
                                                         mc.VF_COEF, mc.SEED, mc.ENT_STEP, row_offset, gscale, ptr(dm), ptr(dvl), ptr(part),
                                                         ptr(dls), nb, sp()), "loss_continuous")
            dm_ = sm.from_t32(_take(dm, rows * d, "dmean"), rows, d)
            dv_, part_, dls_ = _take(dvl, rows, "dvalues"), _take(part, 3 * nb, "loss partials").reshape(nb, 3), _take(dls, nb * d, "dlog_std partials")
            what = f"d={d} Bm={Bm} A={A} row_offset={row_offset} blocks={nb}"
            assert_close(part_.astype(np.float64).sum(0), np.array([w["actor_loss"], w["entropy"], w["value_loss"]]), 1e-5,
                         f"actor loss | entropy | value loss ({what})", scale=1.0)
            assert (part_[1:] == 0.0).all() and (dls_.reshape(nb, d)[1:] == 0.0).all(), "a block without rows writes zero partials"
            assert_close(dls_.reshape(nb, d).astype(np.float64).sum(0), w["dlog_std"], bound, f"dlog_std ({what})")
            if ref is None:
                ref = (dm_, dv_)
            _bits(dm_, ref[0], f"dmean ({what})")
            _bits(dv_, ref[1], f"dvalues ({what})")
        dm_, dv_ = ref
        assert_close(dm_[:R] / gscale, w["dmean"], bound, f"dmean (d={d} {shape} row_offset={row_offset})")
        assert_close(dv_[:R] / gscale, w["dvalues"], bound, f"dvalues (d={d} {shape} row_offset={row_offset})")
        assert (dm_[R:] == 0.0).all() and (dv_[R:] == 0.0).all(), "padding rows are exact zero"


def test_argument_refusals_launch_nothing(dev):
    check, L, ptr, sp = _lib()
    out, x = torch.full((64 * 32,), 9.0, device=dev), torch.zeros(64 * 32, device=dev)
    assert L.mava_transformer_shift_action_f32(ptr(x), None, 2, 3, 17, 1, 32, 32, ptr(out), sp()) <= -1000
    assert L.mava_transformer_shift_action_f32(ptr(x), None, 2, 3, 2, 3, 32, 32, ptr(out), sp()) <= -1000
    assert L.mava_transformer_sample_continuous_f32(2, 3, 3, 2, 1e-3, ptr(x), ptr(x), 0, 0, 0, 0, ptr(out), ptr(out), sp()) <= -1000
    assert L.mava_transformer_sample_continuous_f32(2, 3, 0, 0, 1e-3, ptr(x), ptr(x), 0, 0, 0, 0, ptr(out), ptr(out), sp()) <= -1000
    torch.cuda.synchronize()
    assert float(out.min()) == 9.0 and float(out.max()) == 9.0


# ---- 4. acting on env=spread -----------------------------------------------------------------------------------------------------
SPREAD = ["network=continuous_transformer", "env=spread"]


def _scale(tree):
    return mc.scale_of(tree["decoder"]["log_std"])


def _check_step(tree, obs, action, log_prob, value, eps, H, what):
    """One acting step against the model given the recorded actions: the means of the forced (= teacher-forced, by causality) pass,
    the recorded actions = tanh(mean + scale * eps), the recorded log-probs = the model's of the recorded actions, the values."""
    lp_want, val, mean, scale = mc.forward(tree, obs, action, H)
    e = torch.zeros_like(mean) if eps is None else torch.as_tensor(eps, dtype=torch.float64)
    assert_close(action.numpy(), torch.tanh(mean + scale * e).numpy(), 1e-5, f"{what}: actions")
    assert_close(log_prob.numpy(), lp_want.numpy(), 1e-5, f"{what}: log-probs")
    if value is not None:
        assert_close(value.numpy(), val.numpy(), 1e-5, f"{what}: values")
    return mean, scale


def _check_rollout(dev, L, H):
    """Every step of a finished rollout against the model, and the teacher-forced kernel pass on the recorded actions."""
    from mava_amd.mat_learner import MATPass

    rep, E, A, d, T = L.rep, L.E, L.A, L.nA, L.T
    tree = tgm._f64_tree(L)
    tf = MATPass(L.net, E, dev, True, L.ctx)
    tf.idx[:E].copy_(torch.arange(E, dtype=torch.int32))
    for t in range(T):
        obs, act = rep.agents_view[t].double().cpu(), rep.action[t].double().cpu()
        assert act.shape == (E, A, d) and float(act.abs().max()) < 1.0
        _, scale = _check_step(tree, obs, act, rep.log_prob[t].double().cpu(), rep.value[t].double().cpu(),
                               mc.sample_noise(L.seed, t, E, A, d), H, f"step {t}")
        tf.gather_obs(rep.agents_view[t], E)
        tf.shift_onehot(rep.action[t], A - 1, False)
        tf.encode(L.p)
        tf.decode(L.p)
        means = tgm._from_t32(tf.logits.t, tf.rows, d)[: E * A].view(E, A, d)
        lp_tf = mc.log_prob(act, means, scale)
        assert_close(lp_tf.numpy(), rep.log_prob[t].double().cpu().numpy(), 1e-5, f"teacher-forced kernel pass at step {t}")


def _perturb(L, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    L.p.add_((0.05 * torch.randn(L.P, generator=g)).to(dev))  # (the head starts at 0.01: give the means some spread)


def test_acting_matches_model_and_teacher_forced_pass(dev):
    from mava_amd.types import Observation

    cfg, learn, L, _ = tgm._make(dev, SPREAD + ["arch.num_envs=4", "system.rollout_length=4", "system.matmul_mode=f32", "network.n_head=2"])
    assert L.continuous and L.net.continuous and L.nA == 2 and L.rep.action.dtype == torch.float32
    _perturb(L, dev)
    L._rollout(0)
    _check_rollout(dev, L, 2)
    rep = L.rep
    ob = Observation(rep.agents_view[0], rep.action_mask[0].bool(), rep.step_count[0])
    ga = L.actor_network.apply(L.learner_state().params.actor_params, ob).mode()
    assert ga.dtype == torch.float32 and ga.shape == (L.E, L.A, L.nA)
    ga = ga.double().cpu()
    mean = mc.forward(tgm._f64_tree(L), rep.agents_view[0].double().cpu(), ga, 2)[2]
    assert_close(ga.numpy(), torch.tanh(mean).numpy(), 1e-5, "mode() = tanh(mean) given the earlier agents")


# ---- 5. learn() ------------------------------------------------------------------------------------------------------------------
def _learn_against_model(dev, learn, L, state, cfg, H, f16, calls_check=None):
    s, rep, T, E, A, d = cfg.system, L.rep, L.T, L.E, L.A, L.nA
    mcfg = {"n_head": H, "clip_eps": float(s.clip_eps), "ent_coef": float(s.ent_coef), "vf_coef": float(s.vf_coef), "lr": float(s.actor_lr),
            "max_grad_norm": float(s.max_grad_norm), "seed": L.seed, "min_scale": L.min_scale}
    count, ent_step = 0, 0
    L.debug = {"grads": [], "perms": [], "state": []}
    t64 = lambda x: x.double().cpu()
    off = L.net.off[("decoder", "log_std")]
    for upd in range(3):
        for rec in L.debug.values():
            if isinstance(rec, list):
                rec.clear()
        with _Calls() as calls:
            out = learn(state)
        if calls_check is not None:
            calls_check(calls.by)
        state = out.learner_state
        TE = T * E
        adv, tgt = mc.gae(t64(rep.reward).view(T, E * A), t64(rep.value).view(T, E * A), rep.done.cpu().view(T, E * A),
                          t64(rep.last_val).view(E * A), float(s.gamma), float(s.gae_lambda))
        assert_close(rep.adv.cpu().numpy().reshape(T, -1), adv.numpy(), 1e-5, f"update {upd}: advantages")
        view = rep.agents_view[:T].clone()
        view[0] = L.debug["slot0"][0]  # (the update ends by moving the last observation into slot 0)
        batch = {"obs": t64(view).view(TE, A, -1), "action": t64(rep.action).view(TE, A, d), "log_prob": t64(rep.log_prob).view(TE, A),
                 "adv": t64(rep.adv).view(TE, A), "value": t64(rep.value).view(TE, A), "target": t64(rep.tgt).view(TE, A)}
        i = 0
        for k in range(L.K):
            perm = L.debug["perms"][k].long().cpu()
            assert sorted(perm.tolist()) == list(range(TE))
            for mb in range(L.M):
                idx = perm[mb * L.Bm : (mb + 1) * L.Bm]
                flat, m, v = (x.double().cpu().numpy() for x in L.debug["state"][i])
                flat, m, v, count, grad, met = mc.minibatch_step(L.net, flat, m, v, count, batch, idx, dict(mcfg, ent_step=ent_step))
                ent_step += 1
                what = f"update {upd} epoch {k} minibatch {mb}"
                got = L.debug["grads"][i][: L.P].double().cpu().numpy()
                tgm._compare_grad(got, grad, f"{what}: gradient", f16)
                assert float(np.abs(grad[off:]).min()) > 0.0
                assert_close(got[off:], grad[off:], 1e-3 if f16 else 1e-4, f"{what}: log_std gradient")
                assert_close(L.train_metrics[0, k, mb].double().cpu().numpy(), met, 1e-4 if f16 else 1e-5, f"{what}: metrics")
                i += 1
                after = L.debug["state"][i][0] if i < len(L.debug["state"]) else L.p
                tgm._compare_params(after.double().cpu().numpy(), flat, f"{what}: parameters", f16)
        assert int(L.count[0]) == count and L.ent_step == ent_step
    for k in ("total_loss", "actor_loss", "value_loss", "entropy"):
        assert out.train_metrics[k].shape == (1, 1, 1, L.K, L.M)


LEARN = SPREAD + ["arch.num_envs=4", "system.rollout_length=8", "system.num_minibatches=2", "system.ppo_epochs=2", "system.actor_lr=1e-3"]


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("n_block,D,H", [(1, 64, 1), (2, 64, 2)])
def test_learn_matches_model(dev, mode, n_block, D, H):
    cfg, learn, L, state = tgm._make(dev, LEARN + [f"system.matmul_mode={mode}", f"network.n_block={n_block}", f"network.n_embd={D}",
                                                   f"network.n_head={H}"])
    assert L.A == 3 and L.continuous
    _learn_against_model(dev, learn, L, state, cfg, H, mode == "f16x2")


# ---- 6. the fused step -----------------------------------------------------------------------------------------------------------
# (B, A, O, d, D, H, n_block)
SHAPES = [(1, 1, 3, 1, 32, 1, 1), (11, 3, 7, 2, 32, 1, 1), (43, 3, 7, 5, 64, 2, 2), (43, 5, 33, 16, 96, 4, 1), (3, 20, 9, 9, 128, 4, 2),
          (2, 32, 5, 8, 128, 1, 1)]
STEP, ROW_OFFSET = 7, 1000


@functools.lru_cache(maxsize=None)
def case(shape):
    from mava_amd.mat_learner import MATNet

    B, A, O, d, D, H, nb = shape
    net = MATNet(O, d, A, D, H, nb, continuous=True)
    g = torch.Generator().manual_seed(sum(shape))
    flat = net.init_flat(5) + 0.05 * torch.randn(net.num_params, generator=g)
    obs = torch.randn((B, A, O), generator=g)
    return {"net": net, "flat": flat, "obs": obs, "tree": net.tree(flat.double()), "eps": mc.sample_noise(mc.SEED, STEP, B, A, d, ROW_OFFSET)}


def run_fused(dev, shape, greedy=False, n_blocks=None, fill_ws=float("nan"), with_value=True):
    """One launch into sentinel-filled outputs one sample longer than B (the guard sample must survive) over a NaN-filled workspace."""
    check, L, ptr, sp = _lib()
    B, A, O, d, D, H, nb = shape
    c = case(shape)
    if n_blocks is None:
        n_blocks = max(1, min(256, -(-B // max(1, 32 // A))))
    need = L.mava_transformer_act_workspace_bytes(B, A, D, nb, n_blocks)
    ws = torch.empty(max(need, 16) // 4, device=dev)
    ws.fill_(fill_ws)
    action = torch.full((B + 1, A, d), 9.0, device=dev)
    log_prob, value = torch.full((B + 1, A), 9.0, device=dev), torch.full((B + 1, A), 9.0, device=dev)
    flat, obs = c["flat"].to(dev), c["obs"].to(dev).contiguous()
    check(L.mava_transformer_act_continuous_f32(ptr(flat), ptr(obs), B, A, O, d, D, H, nb, tn.MIN_SCALE, mc.SEED, STEP, ROW_OFFSET, int(greedy),
                                                ptr(action), ptr(log_prob), ptr(value) if with_value else None, ptr(ws), ws.numel() * 4,
                                                n_blocks, sp()), "mava_transformer_act_continuous_f32")
    torch.cuda.synchronize()
    assert bool((action[B] == 9.0).all()) and bool((log_prob[B] == 9.0).all()) and bool((value[B] == 9.0).all()), "the guard sample changed"
    if not with_value:
        assert bool((value == 9.0).all())
    assert bool(torch.isfinite(action[:B]).all()) and bool(torch.isfinite(log_prob[:B]).all())
    return action[:B].double().cpu(), log_prob[:B].double().cpu(), value[:B].double().cpu() if with_value else None


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_matches_float64_model(dev, shape, greedy):
    c = case(shape)
    act, lp, val = run_fused(dev, shape, greedy)
    _check_step(c["tree"], c["obs"].double(), act, lp, val, None if greedy else c["eps"], shape[5], f"{shape} greedy={greedy}")


def test_fused_is_bit_identical_for_any_grid_and_workspace(dev):
    for shape in (SHAPES[2], SHAPES[3]):
        ref = run_fused(dev, shape, n_blocks=1)
        for nb, fill in ((3, float("nan")), (256, float("nan")), (3, 0.0)):
            for a, b, name in zip(ref, run_fused(dev, shape, n_blocks=nb, fill_ws=fill), ("action", "log_prob", "value")):
                assert torch.equal(a, b), f"{name} differs between 1 and {nb} blocks (workspace filled with {fill})"
    act, lp, _ = run_fused(dev, SHAPES[3], n_blocks=1, with_value=False)  # value = NULL: nothing else changes
    assert torch.equal(act, ref[0]) and torch.equal(lp, ref[1])


def _act_pass(dev, c, acting, B, greedy=False):
    from mava_amd._lib import Ctx
    from mava_amd.mat_learner import MATActor

    net = c["net"]
    p = MATActor(net, Ctx("f32"), dev, acting).pass_for(B)
    action = torch.zeros((B, net.A, net.nA), device=dev)
    log_prob, value = torch.zeros((B, net.A), device=dev), torch.zeros((B, net.A), device=dev)
    p.act(c["flat"].to(dev), c["obs"].to(dev).contiguous(), None, action, log_prob, mc.SEED, STEP, ROW_OFFSET, greedy, value_out=value)
    torch.cuda.synchronize()
    return action.double().cpu(), log_prob.double().cpu(), value.double().cpu()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_fused_draws_what_the_layerwise_pass_draws(dev, shape):
    c = case(shape)
    with _Calls() as calls:
        lw = _act_pass(dev, c, "layerwise", shape[0])
    assert calls.by["mava_transformer_sample_continuous_f32"] == shape[1] and "mava_transformer_act_continuous_f32" not in calls.by
    with _Calls() as calls:
        fu = _act_pass(dev, c, "fused", shape[0])
    assert calls.by["mava_transformer_act_continuous_f32"] == 1 and "mava_transformer_sample_continuous_f32" not in calls.by, calls.by
    _check_step(c["tree"], c["obs"].double(), *lw, c["eps"], shape[5], f"{shape} layerwise")
    assert_close(fu[0].numpy(), lw[0].numpy(), 1e-5, "actions, fused against layerwise")
    assert_close(fu[1].numpy(), lw[1].numpy(), 1e-5, "log-probs, fused against layerwise")
    assert_close(fu[2].numpy(), lw[2].numpy(), 1e-5, "values, fused against layerwise")


def test_fused_depth_beyond_the_cap_falls_back_to_the_layers(dev):
    shape = (11, 3, 7, 2, 32, 1, 5)
    c = case(shape)
    with _Calls() as calls:
        got = _act_pass(dev, c, "fused", shape[0])
    assert calls.by["mava_transformer_act_continuous_f32"] == 1 and calls.by["mava_transformer_sample_continuous_f32"] == shape[1]
    _check_step(c["tree"], c["obs"].double(), *got, c["eps"], shape[5], f"{shape} fallback")


FUSED = LEARN + ["network.acting=fused", "network.n_block=2", "network.n_head=2"]


def test_fused_rollout_is_one_launch_per_env_step(dev):
    cfg, learn, L, _ = tgm._make(dev, FUSED + ["system.matmul_mode=f32"])
    _perturb(L, dev)
    with _Calls() as calls:
        L._rollout(0)
        torch.cuda.synchronize()
    assert calls.by == {"mava_transformer_act_continuous_f32": L.T, "mava_spread_step": L.T}, calls.by
    _check_rollout(dev, L, 2)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_fused_learn_matches_model(dev, mode):
    cfg, learn, L, state = tgm._make(dev, FUSED + [f"system.matmul_mode={mode}"])
    assert L.roll.acting == "fused"

    def calls_check(by):
        assert by["mava_transformer_act_continuous_f32"] == L.T and "mava_transformer_sample_continuous_f32" not in by

    _learn_against_model(dev, learn, L, state, cfg, 2, mode == "f16x2", calls_check)


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acting", ["layerwise", "fused"])
def test_run_experiment_and_checkpoint(dev, tmp_path, monkeypatch, acting):
    from mava_amd.config import compose
    from mava_amd.mat_learner import MATParams
    from mava_amd.systems.ppo import anakin, ff_mat
    from mava_amd.types import AdamState
    from mava_amd.utils.checkpointing import Checkpointer

    monkeypatch.chdir(tmp_path)
    over = SPREAD + ["arch.num_envs=4", "system.rollout_length=8", "arch.num_eval_episodes=4", "arch.num_absolute_metric_eval_episodes=4",
                     "arch.evaluation_greedy=true", f"network.acting={acting}"]
    recs = []
    with _Calls() as calls:
        ret = ff_mat.run_experiment(compose("default_ff_mat", over + ["system.num_updates=4", "arch.num_evaluation=2",
                                                                     "logger.checkpointing.save_model=true"]), log=recs.append)
    assert len([r for r in recs if "eval_episode_return" in r]) == 2 and np.isfinite(ret)
    for k in ("total_loss", "actor_loss", "value_loss", "entropy"):
        assert np.isfinite(recs[0][k])
    if acting == "fused":
        assert calls.by["mava_transformer_act_continuous_f32"] > 4 * 8 and "mava_transformer_sample_continuous_f32" not in calls.by
    else:
        assert calls.by["mava_transformer_sample_continuous_f32"] > 4 * 8 * 3 and "mava_transformer_act_continuous_f32" not in calls.by
    ck = Checkpointer(model_name="ff_mat", checkpoint_uid=os.listdir(os.path.join(tmp_path, "checkpoints", "ff_mat"))[0])
    raw = ck.restore_learner_state_raw()
    assert set(raw["params"]) == {"encoder", "decoder"} and "log_std" in raw["params"]["decoder"]
    if acting == "fused":
        return
    # two updates, a checkpoint of the state, and the next update from the checkpoint against the next update in memory
    cfg, learn, L, state = tgm._make(dev, over)
    for _ in range(2):
        state = learn(state).learner_state
    ck2 = Checkpointer(model_name="ff_mat_next", checkpoint_uid="t")
    ck2.save(timestep=2, unreplicated_learner_state=anakin._unreplicate_n_dims(state), episode_return=0.0)
    raw = ck2.restore_learner_state_raw()
    snap = (L.p.clone(), L.m.clone(), L.v.clone())
    ends = []
    for from_disk in (False, True):
        _, learn2, L2, st2 = tgm._make(dev, over, keys=(7, 99, 13))  # other initial parameters, the same environment stream
        if from_disk:
            st2 = st2._replace(params=MATParams(**raw["params"]), opt_states=AdamState(**raw["opt_states"]))
        else:
            st2 = st2._replace(params=L.net.tree(snap[0]), opt_states=AdamState(L.count[0].clone(), L.net.tree(snap[1]), L.net.tree(snap[2])))
        learn2(st2)
        ends.append((L2.p.clone(), L2.m.clone(), L2.v.clone(), int(L2.count[0])))
    assert ends[0][3] == ends[1][3] == int(L.count[0]) + L.K * L.M
    for a, b in zip(ends[0][:3], ends[1][:3]):
        assert torch.equal(a, b)
    assert not torch.equal(ends[0][0], snap[0])
