"""GPU: the kernels of mava_amd/csrc/mat.hip against float64 autograd, autoregressive acting and learn() against the
float64 model of tests/mat_model.py step by step, and run_experiment with its checkpoint.

Kernel outputs and gradients are held to 1e-6 of the tensor's max-abs (tests/test_gpu_qmix.py's bound for a single kernel):
the kernels sum in f64, so no bound is widened and there is no profiles/mat_kernel_error.json.  Whole updates: gradients
1e-4 of rms, parameters and metrics 1e-5 in f32 mode; rec_iql's allowance in f16x2 mode (tests/test_gpu_iql.py).
"""
import os

import numpy as np
import pytest
import torch

from oracle import philox
from tests import mat_model as mm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

c32 = lambda n: -(-n // 32) * 32


def _lib():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return check, lib(), ptr, stream_ptr


def _to_t32(x: torch.Tensor, rows: int, dev, ld=None) -> torch.Tensor:
    """(n, N) host tensor -> T32 (rows x ld) on the device; rows past n and features past N hold 7.0: they must not leak."""
    from mava_amd.rec_networks import rows_to_t32

    n, N = x.shape
    full = torch.full((rows, ld or N), 7.0, dtype=torch.float32)
    full[:n, :N] = x.float()
    return rows_to_t32(full.to(dev))


def _from_t32(t: torch.Tensor, rows: int, N: int) -> torch.Tensor:
    from mava_amd.rec_networks import t32_to_rows

    return t32_to_rows(t, N, rows).double().cpu()


def _maxabs_close(got, want, what, tol=1e-6):
    err = float((got - want).abs().max())
    assert err <= tol * max(float(want.abs().max()), 1e-30), f"{what}: max error {err:.3e} against max-abs {float(want.abs().max()):.3e}"


# ---- attention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H", [(32, 1), (64, 2), (96, 4), (128, 4), (128, 1)])  # head widths 32, 24 (no power of two) and 128
# A = 7: groups of S = 4 samples, 28 rows that do not divide the tile, a partial last group; A = 20: S = 1 under a tile's 32 rows,
# and the 400 scores of an item take two trips of the block
@pytest.mark.parametrize("A", [1, 2, 3, 5, 7, 16, 20, 32])
def test_attention_forward_and_backward(dev, A, D, H):
    check, L, ptr, sp = _lib()
    g = torch.Generator().manual_seed(A * 1000 + D + H)
    for B in (1, 11, 43):  # with A = 3: 3, 33 and 129 rows - under one tile, a sample across a tile edge, a padded last tile
        n, rows = B * A, c32(B * A)
        for causal in (False, True):
            for cross in (False, True):
                # unit-scale activations: the scores stay within +-8 (q k^T / sqrt(hd) of unit normals is ~ N(0, 1))
                q, k, v, dy = (torch.randn((n, D), generator=g).float().double() for _ in range(4))
                if not cross:
                    q = (k + 0.5 * q).float().double()  # self-attention: q and k come from the same rows
                qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
                y, P = mm.attention_core(qr.view(B, A, D), kr.view(B, A, D), vr.view(B, A, D), H, causal)
                (y.reshape(n, D) * dy).sum().backward()
                dq, dk, dv, dyd = (_to_t32(t, rows, dev) for t in (q, k, v, dy))
                outs = {}
                for nb in (1, 8, 64):
                    yo, po = torch.full((rows * D,), 9.0, device=dev), torch.full((rows * H * A,), 9.0, device=dev)
                    gq, gk, gv = (torch.full((rows * D,), 9.0, device=dev) for _ in range(3))
                    check(L.mava_mat_attn_fwd_f32(ptr(dq), ptr(dk), ptr(dv), rows, D, B, A, H, int(causal), ptr(yo), ptr(po), nb, sp()), "attn_fwd")
                    # the backward pass reads dy on real rows only: its padding (7.0) must not reach the outputs
                    check(L.mava_mat_attn_bwd_f32(ptr(dyd), ptr(dq), ptr(dk), ptr(dv), rows, D, B, A, H, int(causal), ptr(gq), ptr(gk), ptr(gv),
                                                  nb, sp()), "attn_bwd")
                    outs[nb] = [t.cpu() for t in (yo, po, gq, gk, gv)]
                for nb in (8, 64):
                    for a, b, name in zip(outs[1], outs[nb], ("y", "P", "dq", "dk", "dv")):
                        assert torch.equal(a, b), f"{name} differs between 1 and {nb} blocks (B={B} causal={causal})"
                yo, po, gq, gk, gv = (t.to(dev) for t in outs[1])
                what = f"A={A} B={B} D={D} H={H} causal={causal} cross={cross}"
                for got, want, N, name in ((yo, y.detach().reshape(n, D), D, "y"), (gq, qr.grad, D, "dq"), (gk, kr.grad, D, "dk"),
                                           (gv, vr.grad, D, "dv")):
                    full = _from_t32(got, rows, N)
                    _maxabs_close(full[:n], want, f"{name} ({what})")
                    assert float(full[n:].abs().max() if rows > n else 0.0) == 0.0, f"{name}: padding rows are not exact zero ({what})"
                pf = _from_t32(po, rows, H * A)
                _maxabs_close(pf[:n].view(B, A, H, A).permute(0, 2, 1, 3), P.detach(), f"P ({what})")
                assert float(pf[n:].abs().max() if rows > n else 0.0) == 0.0
                if causal and A > 1:
                    up = torch.triu(torch.ones(A, A, dtype=torch.bool), 1)
                    assert float(pf[:n].view(B, A, H, A).permute(0, 2, 1, 3)[..., up].abs().max()) == 0.0, "P above the diagonal"


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 32, 63, 64, 128, 403])
@pytest.mark.parametrize("n", [3, 33, 129])
def test_layer_norm_forward_and_backward(dev, n, N):
    check, L, ptr, sp = _lib()
    from mava_amd import ops

    g = torch.Generator().manual_seed(n * 1000 + N)
    rows = c32(n)
    for with_res in (False, True):
        x, res, dy = (torch.randn((n, N), generator=g).float().double() for _ in range(3))
        x[n // 2] = 1.25  # one row of constant input: variance 0
        if with_res:
            res[n // 2] = -0.5
        scale, bias = (1.0 + 0.3 * torch.randn(N, generator=g)).float().double(), torch.randn(N, generator=g).float().double()
        xin = ((x.float() + res.float()) if with_res else x.float()).double()  # the kernel adds in f32, as the residual stream is f32
        xr, sr, br = xin.clone().requires_grad_(True), scale.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = mm.layer_norm(xr, {"scale": sr, "bias": br})
        (y * dy).sum().backward()
        dx_, dres, ddy = _to_t32(x, rows, dev), _to_t32(res, rows, dev) if with_res else None, _to_t32(dy, rows, dev)
        ds, db = scale.float().to(dev), bias.float().to(dev)
        ref = None
        for nb in (1, 8, 64):
            yo, xh, gx = (torch.full((rows * N,), 9.0, device=dev) for _ in range(3))
            rs = torch.full((rows,), 9.0, device=dev)
            slab = torch.full((nb, 2 * N + 3), 9.0, device=dev)
            check(L.mava_mat_ln_fwd_f32(ptr(dx_), ptr(dres), ptr(ds), ptr(db), N, rows, n, ptr(yo), ptr(xh), ptr(rs), nb, sp()), "ln_fwd")
            check(L.mava_mat_ln_bwd_f32(ptr(ddy), ptr(xh), ptr(rs), ptr(ds), N, rows, n, 0.5, ptr(gx), ptr(slab), slab.shape[1], nb, sp()),
                  "ln_bwd")
            gsb = torch.zeros(2 * N, device=dev)
            ops.slab_reduce(slab, 2 * N, gsb)
            if nb > rows // 32:  # blocks without a tile write exact zeros
                assert float(slab[rows // 32 :, : 2 * N].abs().max()) == 0.0
            cur = [t.cpu() for t in (yo, xh, rs, gx)]
            if ref is None:
                ref, gsb1 = cur, gsb.double().cpu()
            else:
                for a, b, name in zip(ref, cur, ("y", "xhat", "rstd", "dx")):
                    assert torch.equal(a, b), f"{name} differs between 1 and {nb} blocks"
                _maxabs_close(gsb.double().cpu(), gsb1, f"dscale | dbias with {nb} slabs", 1e-6)
        what = f"n={n} N={N} res={with_res}"
        yf, gxf = _from_t32(ref[0].to(dev), rows, N), _from_t32(ref[3].to(dev), rows, N)
        _maxabs_close(yf[:n], y.detach(), f"y ({what})")
        # N = 1: xhat = 0 and dx = 0 exactly; the bound is on the tensor's max-abs, so compare absolutely then
        if float(xr.grad.abs().max()) > 0:
            _maxabs_close(gxf[:n], xr.grad, f"dx ({what})", 1e-6 if N > 1 else 1e-5)
        else:
            assert float(gxf[:n].abs().max()) == 0.0
        assert float(yf[n:].abs().max()) == 0.0 and float(gxf[n:].abs().max()) == 0.0, f"padding rows ({what})"
        assert torch.equal(yf[n // 2].float(), bias.float()) or N == 1 or float((yf[n // 2] - bias).abs().max()) <= 1e-6
        _maxabs_close(gsb1[:N], 0.5 * sr.grad, f"dscale ({what})") if float(sr.grad.abs().max()) > 0 else None
        _maxabs_close(gsb1[N:], 0.5 * br.grad, f"dbias ({what})")


# ---- GELU, shifted one-hot ------------------------------------------------------------------------------------------------
def test_gelu_forward_and_backward(dev):
    check, L, ptr, sp = _lib()
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.tensor([0.0, 30.0, -30.0, 1e-4, -1e-4, 8.0, -8.0]), 3.0 * torch.randn(4089, generator=g),
                   torch.linspace(-30.0, 30.0, 4096)]).float()
    dy = torch.randn(x.shape, generator=g).float()
    dy[0] = 1.0
    xr = x.double().requires_grad_(True)
    y = mm.gelu(xr)
    (y * dy.double()).sum().backward()
    xd, dyd = x.to(dev), dy.to(dev)
    yo, gx = torch.empty_like(xd), torch.empty_like(xd)
    check(L.mava_mat_gelu_f32(ptr(xd), x.numel(), ptr(yo), sp()), "gelu")
    check(L.mava_mat_gelu_bwd_f32(ptr(dyd), ptr(xd), x.numel(), ptr(gx), sp()), "gelu_bwd")
    assert bool(torch.isfinite(yo).all()) and bool(torch.isfinite(gx).all())
    assert float(gx[0]) == 0.5 and float(yo[0]) == 0.0 and float(yo[1]) == 30.0 and float(yo[2]) == 0.0
    _maxabs_close(yo.double().cpu(), y.detach(), "gelu")
    _maxabs_close(gx.double().cpu(), xr.grad, "gelu'")


@pytest.mark.parametrize("nA", [2, 5, 31, 32, 64])
def test_shifted_onehot_is_bit_exact(dev, nA):
    check, L, ptr, sp = _lib()
    g = torch.Generator().manual_seed(nA)
    for A, B in ((1, 5), (3, 11), (5, 13), (32, 3)):
        rows, Np, TE = c32(A * B), c32(nA + 1), B + 4
        action = torch.randint(0, nA, (TE, A), generator=g, dtype=torch.int32)
        action[0, 0], action[-1, -1] = nA - 1, 0
        idx = torch.randperm(TE, generator=g)[:B].to(torch.int32)
        d_action, d_idx = action.to(dev), idx.to(dev)
        for known in sorted({0, min(1, A - 1), A - 1}):
            for use_idx in (False, True):
                out = torch.full((rows * Np,), 9.0, device=dev)
                check(L.mava_mat_shift_onehot_f32(ptr(d_action), ptr(d_idx) if use_idx else None, B, A, nA, known, rows, Np,
                                                  ptr(out), sp()), "shift_onehot")
                src = action[idx.long()] if use_idx else action[:B]
                want = torch.zeros((rows, Np), dtype=torch.float64)
                want[: A * B, : nA + 1] = mm.shifted_onehot(src, nA, known).view(A * B, nA + 1)
                assert torch.equal(_from_t32(out, rows, Np), want), f"nA={nA} A={A} known={known} idx={use_idx}"


def test_argument_refusals_launch_nothing(dev):
    check, L, ptr, sp = _lib()
    out = torch.full((32 * 64,), 9.0, device=dev)
    x = torch.zeros(32 * 64, device=dev)
    assert L.mava_mat_attn_fwd_f32(ptr(x), ptr(x), ptr(x), 32, 64, 1, 33, 1, 0, ptr(out), None, 1, sp()) <= -1000
    assert L.mava_mat_attn_fwd_f32(ptr(x), ptr(x), ptr(x), 32, 64, 1, 4, 3, 0, ptr(out), None, 1, sp()) <= -1000
    assert L.mava_mat_ln_fwd_f32(ptr(x), None, ptr(x), ptr(x), 64, 48, 40, ptr(out), None, None, 1, sp()) <= -1000
    assert L.mava_mat_ln_fwd_f32(ptr(x), None, ptr(x), ptr(x), 64, 32, 32, ptr(out), ptr(x), None, 1, sp()) <= -1000
    assert L.mava_mat_shift_onehot_f32(None, None, 2, 4, 5, 2, 32, 32, ptr(out), sp()) <= -1000
    assert L.mava_mat_sample_f32(2, 4, 0, 65, ptr(x), None, 0, 0, 0, 0, ptr(out), ptr(out), sp()) <= -1000
    torch.cuda.synchronize()
    assert float(out.min()) == 9.0 and float(out.max()) == 9.0


# ---- acting ---------------------------------------------------------------------------------------------------------------
def _make(dev, overrides, keys=(7, 11, 13)):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.mat_learner import learner_setup

    cfg = compose("default_ff_mat", list(overrides))
    env, _ = envs.make(cfg, device=dev)
    learn, actor, state = learner_setup(env, keys, cfg)
    return cfg, learn, learn.learner, state


def _f64_tree(L, flat=None):
    return L.net.tree((L.p if flat is None else flat).double().cpu())


@pytest.mark.parametrize("env", [["env=rware", "env/scenario=tiny-4ag"], ["env=lbf", "env/scenario=2s-8x8-2p-2f-coop"]])
def test_acting_matches_model_and_teacher_forced_pass(dev, env):
    from mava_amd.mat_learner import MATPass

    cfg, learn, L, _ = _make(dev, env + ["arch.num_envs=4", "system.rollout_length=4", "system.matmul_mode=f32", "network.n_head=2"])
    g = torch.Generator().manual_seed(3)
    L.p.add_((0.05 * torch.randn(L.P, generator=g)).to(dev))  # (the heads start at 0.01: give the logits some spread)
    L._rollout(0)
    rep, E, A, nA, T = L.rep, L.E, L.A, L.nA, L.T
    tree = _f64_tree(L)
    tf = MATPass(L.net, E, dev, True, L.ctx)
    tf.idx[:E].copy_(torch.arange(E, dtype=torch.int32))
    compared = 0
    for t in range(T):
        obs, mask = rep.agents_view[t].double().cpu(), rep.action_mask[t].bool().cpu()
        u = torch.from_numpy(philox.policy_uniforms(L.seed, t, E * A, nA, 0).astype(np.float64)).view(E, A, nA)
        act, lp, val, gap = mm.act(tree, obs, mask, u, 2)
        got = rep.action[t].long().cpu()
        assert bool(mask.gather(-1, got.unsqueeze(-1)).all()), "an illegal action was sampled"
        # a later agent conditions on the earlier actions: compare a sample up to its first near-tie
        for e in range(E):
            for a in range(A):
                if float(gap[e, a]) < 1e-4:
                    break
                assert int(got[e, a]) == int(act[e, a]), f"step {t} env {e} agent {a}"
                assert abs(float(rep.log_prob[t, e, a]) - float(lp[e, a])) <= 1e-5
                compared += 1
        assert_close(rep.value[t].cpu().numpy(), val.numpy(), 1e-5, f"value at step {t}")
        # teacher-forced pass of the kernels on the recorded actions
        tf.gather_obs(rep.agents_view[t], E)
        tf.shift_onehot(rep.action[t], A - 1, False)
        tf.encode(L.p)
        tf.decode(L.p)
        logits = _from_t32(tf.logits.t, tf.rows, nA)[: E * A].view(E, A, nA)
        lp_tf = mm.masked_log_softmax(logits, mask)[0].gather(-1, got.unsqueeze(-1))[..., 0]
        assert float((lp_tf - rep.log_prob[t].double().cpu()).abs().max()) <= 2e-6, f"teacher-forced log-probs at step {t}"
    assert compared >= 0.9 * T * E * A
    # greedy acting through the evaluator's path picks the arg-max of every agent's masked logits given the earlier ones
    from mava_amd.types import Observation

    ob = Observation(rep.agents_view[0], rep.action_mask[0].bool(), rep.step_count[0])
    ga = L.actor_network.apply(L.learner_state().params.actor_params, ob).mode().long().cpu()
    want, _, _, gap = mm.act(tree, rep.agents_view[0].double().cpu(), rep.action_mask[0].bool().cpu(), None, 2, greedy=True)
    ok = gap.min(-1).values > 1e-4
    assert bool(ok.any()) and torch.equal(ga[ok], want[ok])


# ---- learn() --------------------------------------------------------------------------------------------------------------
def _compare_grad(g, w, what, f16):
    if f16:  # rec_iql's allowance (tests/test_gpu_iql.py)
        bad = np.abs(g - w) > 1e-3 * (np.abs(w) + np.sqrt(np.mean(w * w)))
        assert bad.sum() <= max(12, 5e-4 * bad.size), f"{what}: {int(bad.sum())} entries outside 1e-3"
        assert_close(g, w, 1e-2, f"{what} (hard bound)")
    else:
        assert_close(g, w, 1e-4, what)


def _compare_params(got, want, what, f16):
    if f16:
        bad = np.abs(got - want) > 1e-4 * (np.abs(want) + np.sqrt(np.mean(want * want)))
        assert bad.sum() <= max(12, 5e-4 * bad.size), f"{what}: {int(bad.sum())} entries outside 1e-4"
        assert_close(got, want, 1e-3, f"{what} (hard bound)")
    else:
        assert_close(got, want, 1e-5, what)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("n_block,D,H,scenario", [(1, 64, 1, "2s-8x8-2p-2f-coop"), (2, 64, 2, "2s-10x10-3p-3f"), (1, 64, 2, "2s-10x10-3p-3f"),
                                                  (2, 64, 1, "2s-8x8-2p-2f-coop")])
def test_learn_matches_model(dev, mode, n_block, D, H, scenario):
    cfg, learn, L, state = _make(dev, ["env=lbf", f"env/scenario={scenario}", "arch.num_envs=4", "system.rollout_length=8",
                                       "system.num_minibatches=2", "system.ppo_epochs=2", f"system.matmul_mode={mode}",
                                       f"network.n_block={n_block}", f"network.n_embd={D}", f"network.n_head={H}", "system.actor_lr=1e-3"])
    f16 = mode == "f16x2"
    s, rep, T, E, A = cfg.system, L.rep, L.T, L.E, L.A
    assert A == (2 if "2p" in scenario else 3)
    mcfg = {"n_head": H, "clip_eps": float(s.clip_eps), "ent_coef": float(s.ent_coef), "vf_coef": float(s.vf_coef),
            "lr": float(s.actor_lr), "max_grad_norm": float(s.max_grad_norm)}
    count = 0
    L.debug = {"grads": [], "perms": [], "state": []}
    t64 = lambda x: x.double().cpu()
    for upd in range(3):
        for rec in L.debug.values():
            if isinstance(rec, list):
                rec.clear()
        out = learn(state)
        state = out.learner_state
        TE = T * E
        adv, tgt = mm.gae(t64(rep.reward).view(T, E * A), t64(rep.value).view(T, E * A), rep.done.cpu().view(T, E * A),
                          t64(rep.last_val).view(E * A), float(s.gamma), float(s.gae_lambda))
        assert_close(rep.adv.cpu().numpy().reshape(T, -1), adv.numpy(), 1e-5, f"update {upd}: advantages")
        view, mask = rep.agents_view[:T].clone(), rep.action_mask[:T].clone()
        view[0], mask[0] = L.debug["slot0"]  # (the update ends by moving the last observation into slot 0)
        batch = {"obs": t64(view).view(TE, A, -1), "action": rep.action.long().cpu().view(TE, A),
                 "mask": mask.bool().cpu().view(TE, A, -1), "log_prob": t64(rep.log_prob).view(TE, A),
                 "adv": t64(rep.adv).view(TE, A), "value": t64(rep.value).view(TE, A), "target": t64(rep.tgt).view(TE, A)}
        i = 0
        for k in range(L.K):
            perm = L.debug["perms"][k].long().cpu()
            assert sorted(perm.tolist()) == list(range(TE))
            for mb in range(L.M):
                idx = perm[mb * L.Bm : (mb + 1) * L.Bm]
                # every step starts from the learner's own parameters and moments: Adam's g / (sqrt(v) + eps) turns a 1e-7
                # difference on an entry near eps into a visible step, and a gradient taken at other parameters is another one
                flat, m, v = (x.double().cpu().numpy() for x in L.debug["state"][i])
                flat, m, v, count, grad, met = mm.minibatch_step(L.net, flat, m, v, count, batch, idx, mcfg)
                what = f"update {upd} epoch {k} minibatch {mb}"
                _compare_grad(L.debug["grads"][i][: L.P].double().cpu().numpy(), grad, f"{what}: gradient", f16)
                assert_close(L.train_metrics[0, k, mb].double().cpu().numpy(), met, 1e-4 if f16 else 1e-5, f"{what}: metrics")
                i += 1
                after = L.debug["state"][i][0] if i < len(L.debug["state"]) else L.p
                _compare_params(after.double().cpu().numpy(), flat, f"{what}: parameters", f16)
        assert int(L.count[0]) == count
    for k in ("total_loss", "actor_loss", "value_loss", "entropy"):
        assert out.train_metrics[k].shape == (1, 1, 1, L.K, L.M)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_run_experiment_and_checkpoint(dev, tmp_path, monkeypatch):
    from mava_amd.mat_learner import MATParams
    from mava_amd.systems.ppo import anakin, ff_mat
    from mava_amd.types import AdamState
    from mava_amd.utils.checkpointing import Checkpointer

    monkeypatch.chdir(tmp_path)
    over = ["env=lbf", "arch.num_envs=4", "system.rollout_length=8", "arch.num_eval_episodes=4", "arch.num_absolute_metric_eval_episodes=4",
            "arch.evaluation_greedy=true"]
    from mava_amd.config import compose

    recs = []
    ret = ff_mat.run_experiment(compose("default_ff_mat", over + ["system.num_updates=4", "arch.num_evaluation=2",
                                                                 "logger.checkpointing.save_model=true"]), log=recs.append)
    assert len([r for r in recs if "eval_episode_return" in r]) == 2 and np.isfinite(ret)
    for k in ("total_loss", "actor_loss", "value_loss", "entropy"):
        assert np.isfinite(recs[0][k])
    ck = Checkpointer(model_name="ff_mat", checkpoint_uid=os.listdir(os.path.join(tmp_path, "checkpoints", "ff_mat"))[0])
    raw = ck.restore_learner_state_raw()
    assert set(raw["params"]) == {"encoder", "decoder"} and set(raw["opt_states"]) == {"count", "mu", "nu"}
    restored, _ = ck.restore_params(input_params=MATParams())
    assert isinstance(restored, MATParams) and restored.actor_params is restored

    # two updates, a checkpoint of the state, and the next update from the checkpoint against the next update in memory
    cfg, learn, L, state = _make(dev, over)
    for _ in range(2):
        state = learn(state).learner_state
    ck2 = Checkpointer(model_name="ff_mat_next", checkpoint_uid="t")
    ck2.save(timestep=2, unreplicated_learner_state=anakin._unreplicate_n_dims(state), episode_return=0.0)
    raw = ck2.restore_learner_state_raw()
    snap = (L.p.clone(), L.m.clone(), L.v.clone())
    ends = []
    for from_disk in (False, True):
        _, learn2, L2, st2 = _make(dev, over, keys=(7, 99, 13))  # other initial parameters, the same environment stream
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
