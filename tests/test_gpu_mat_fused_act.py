"""GPU: ff_mat's fused acting step (mava_transformer_act_f32, csrc/mat_act.hip) against the float64 model of
tests/mat_model.py, its determinism and bounds, the same draws as the layer-wise path, and the learner, the evaluator and
run_experiment under network.acting=fused.

Bounds are those of tests/test_gpu_mat.py::test_acting_matches_model_and_teacher_forced_pass: a sample is compared up to its
first row whose top-two gap is below 1e-4, actions equal, log-probs and values within 1e-5.  Every case prints its measured
maxima (pytest -s); DESIGN.md 3.25 quotes them.
"""
import functools

import numpy as np
import pytest
import torch

import tests.test_gpu_mat as tgm
from oracle import philox
from tests import mat_model as mm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

# (B, A, O, nA, D, H, n_block)
SHAPES = [(1, 1, 3, 1, 32, 1, 1),      # one agent, one action
          (11, 3, 7, 5, 32, 1, 1),     # A does not divide 32
          (43, 3, 7, 5, 64, 2, 2),     # 129 rows, a partial last group, two blocks, two heads
          (11, 4, 70, 5, 64, 1, 1),    # the default network
          (43, 5, 33, 33, 96, 4, 1),   # head width 24, 33 actions = 9 Philox blocks
          (7, 7, 12, 6, 64, 2, 1),
          (3, 20, 9, 64, 128, 4, 2),   # 64 actions, A over half a tile
          (2, 32, 5, 3, 128, 1, 1),    # 32 agents, head width 128
          (5, 16, 1024, 7, 128, 4, 1)]  # the widest observation
MANY_GROUPS = (300, 4, 70, 5, 64, 1, 1)  # 38 groups: at n_blocks = 1 one workgroup takes them all
SEED, STEP, ROW_OFFSET = 0x1234_5678_9ABC_DEF1, 7, 1000
GAP = 1e-4


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs of a shape and the float64 model's answers, computed once: sampled, greedy and sampled without a mask."""
    from mava_amd.mat_learner import MATNet

    B, A, O, nA, D, H, nb = shape
    net = MATNet(O, nA, A, D, H, nb)
    g = torch.Generator().manual_seed(hash(shape) & 0xFFFF)
    flat = net.init_flat(5) + 0.05 * torch.randn(net.num_params, generator=g)  # the heads start at 0.01: the logits need spread
    obs = torch.randn((B, A, O), generator=g)
    mask = torch.rand((B, A, nA), generator=g) < 0.7
    mask[..., 0] |= ~mask.any(-1)
    mask[0, A - 1] = False  # the uniform-row path, on the rows that come last in their samples
    mask[B - 1, A - 1] = False
    u = torch.from_numpy(philox.policy_uniforms(SEED, STEP, B * A, nA, ROW_OFFSET).astype(np.float64)).view(B, A, nA)
    tree = net.tree(flat.double())
    want = {"sampled": mm.act(tree, obs.double(), mask, u, H), "greedy": mm.act(tree, obs.double(), mask, None, H, greedy=True)}
    return {"net": net, "flat": flat, "obs": obs, "mask": mask, "u": u, "tree": tree, "want": want}


def run(dev, shape, greedy=False, n_blocks=None, step=STEP, with_mask=True, with_value=True, ws=None, fill_ws=float("nan")):
    """One launch.  The outputs are one sample longer than B and pre-filled: the guard sample must come back unchanged.  The
    workspace is filled with NaN first: the kernel reads nothing it has not written.  Returns (action, log_prob, value)."""
    from mava_amd._lib import check, lib, ptr, stream_ptr

    B, A, O, nA, D, H, nb = shape
    c, L = case(shape), lib()
    if n_blocks is None:
        n_blocks = max(1, min(256, -(-B // max(1, 32 // A))))
    need = L.mava_transformer_act_workspace_bytes(B, A, D, nb, n_blocks)
    if ws is None:
        ws = torch.empty(max(need, 16) // 4, device=dev)
        ws.fill_(fill_ws)
    assert ws.numel() * 4 >= need
    action = torch.full((B + 1, A), -7, dtype=torch.int32, device=dev)
    log_prob, value = torch.full((B + 1, A), 9.0, device=dev), torch.full((B + 1, A), 9.0, device=dev)
    flat, obs = c["flat"].to(dev), c["obs"].to(dev).contiguous()
    mask = c["mask"].to(torch.uint8).to(dev).contiguous() if with_mask else None
    check(L.mava_transformer_act_f32(ptr(flat), ptr(obs), ptr(mask), B, A, O, nA, D, H, nb, SEED, step, ROW_OFFSET, int(greedy), ptr(action),
                                     ptr(log_prob), ptr(value) if with_value else None, ptr(ws), ws.numel() * 4, n_blocks, stream_ptr()),
          "mava_transformer_act_f32")
    torch.cuda.synchronize()
    assert bool((action[B] == -7).all()) and bool((log_prob[B] == 9.0).all()) and bool((value[B] == 9.0).all()), "the guard sample changed"
    if not with_value:
        assert bool((value == 9.0).all()), "value written although NULL was passed"
    assert bool(torch.isfinite(log_prob[:B]).all()) and (not with_value or bool(torch.isfinite(value[:B]).all()))
    assert int(action[:B].min()) >= 0 and int(action[:B].max()) < nA
    return action[:B].long().cpu(), log_prob[:B].double().cpu(), value[:B].double().cpu()


def compare(got, want, what, min_frac=0.9):
    """The convention of test_acting_matches_model_and_teacher_forced_pass.  Returns (rows compared, max log-prob error,
    max value error)."""
    act, lp, val = got
    wact, wlp, wval, gap = want
    B, A = wact.shape
    compared, err = 0, 0.0
    for b in range(B):
        for i in range(A):
            if float(gap[b, i]) < GAP:
                break
            assert int(act[b, i]) == int(wact[b, i]), f"{what}: action of sample {b} agent {i}"
            err = max(err, abs(float(lp[b, i]) - float(wlp[b, i])))
            compared += 1
    verr = float((val - wval).abs().max()) if val is not None else 0.0
    print(f"{what}: {compared}/{B * A} rows compared, max log-prob error {err:.3e}, max value error {verr:.3e}")
    assert err <= 1e-5, f"{what}: log-prob error {err:.3e}"
    if val is not None:
        assert verr <= 1e-5, f"{what}: value error {verr:.3e}"
        assert_close(val.numpy(), wval.numpy(), 1e-5, f"{what}: value")
    assert compared >= min_frac * B * A, f"{what}: only {compared} of {B * A} rows compared"
    return compared, err, verr


def measure(dev, shape, greedy):
    """(rows compared, rows, max log-prob error, max value error) of one case: tools/mat_bench.py records these."""
    n, e, v = compare(run(dev, shape, greedy), case(shape)["want"]["greedy" if greedy else "sampled"], f"{shape} greedy={greedy}")
    return n, shape[0] * shape[1], e, v


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [MANY_GROUPS])
def test_matches_float64_model(dev, shape, greedy):
    act, lp, val = run(dev, shape, greedy)
    c = case(shape)
    picked = c["mask"].gather(-1, act.unsqueeze(-1))[..., 0]
    assert bool((picked | ~c["mask"].any(-1)).all()), "an illegal action was chosen on a row that has a legal one"
    compare((act, lp, val), c["want"]["greedy" if greedy else "sampled"], f"{shape} greedy={greedy}")


def test_without_a_mask_and_without_values(dev):
    shape = SHAPES[2]
    c = case(shape)
    want = mm.act(c["tree"], c["obs"].double(), None, c["u"], shape[5])
    compare(run(dev, shape, with_mask=False), want, f"{shape} mask=NULL")
    act, lp, _ = run(dev, shape, with_value=False)
    compare((act, lp, None), c["want"]["sampled"], f"{shape} value=NULL")


# ---- 2. determinism and bounds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], MANY_GROUPS])
def test_bit_identical_for_any_grid(dev, shape):
    ref = run(dev, shape, n_blocks=1)
    for nb in (3, 64):
        for a, b, name in zip(ref, run(dev, shape, n_blocks=nb), ("action", "log_prob", "value")):
            assert torch.equal(a, b), f"{name} differs between 1 and {nb} blocks"


def test_workspace_contents_do_not_matter(dev):
    """NaN (every run above), zeros, and what another step left behind: the same bits."""
    from mava_amd._lib import lib

    shape = SHAPES[2]
    B, A, O, nA, D, H, nb = shape
    ref = run(dev, shape, step=STEP + 1, n_blocks=5)
    for a, b in zip(ref, run(dev, shape, step=STEP + 1, n_blocks=5, fill_ws=0.0)):
        assert torch.equal(a, b)
    ws = torch.full((lib().mava_transformer_act_workspace_bytes(B, A, D, nb, 5) // 4,), float("nan"), device=dev)
    first = run(dev, shape, step=STEP, n_blocks=5, ws=ws)
    again = run(dev, shape, step=STEP + 1, n_blocks=5, ws=ws)
    assert not torch.equal(first[0], again[0]), "another step draws other actions"
    for a, b in zip(ref, again):
        assert torch.equal(a, b), "a launch over a used workspace differs from one over a fresh workspace"


# ---- 3. the same draws as the layer-wise path -----------------------------------------------------------------------------
def _act_pass(dev, net, ctx, acting, c, B, greedy=False):
    from mava_amd.mat_learner import MATActor

    p = MATActor(net, ctx, dev, acting).pass_for(B)
    action = torch.zeros((B, net.A), dtype=torch.int32, device=dev)
    log_prob, value = torch.zeros((B, net.A), device=dev), torch.zeros((B, net.A), device=dev)
    p.act(c["flat"].to(dev), c["obs"].to(dev).contiguous(), c["mask"].to(torch.uint8).to(dev).contiguous(), action, log_prob, SEED, STEP,
          ROW_OFFSET, greedy, value_out=value)
    torch.cuda.synchronize()
    return action.long().cpu(), log_prob.double().cpu(), value.double().cpu()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_same_draws_as_the_layerwise_pass(dev, shape):
    from mava_amd._lib import Ctx

    c, ctx = case(shape), Ctx("f32")
    lw = _act_pass(dev, c["net"], ctx, "layerwise", c, shape[0])
    fu = _act_pass(dev, c["net"], ctx, "fused", c, shape[0])
    want = c["want"]["sampled"]
    compare(lw, want, f"{shape} layerwise")
    compare(fu, want, f"{shape} fused pass")
    gap, worst = want[3], 0.0
    for b in range(shape[0]):
        for i in range(shape[1]):
            if float(gap[b, i]) < GAP:
                break
            assert int(lw[0][b, i]) == int(fu[0][b, i])
            worst = max(worst, abs(float(lw[1][b, i]) - float(fu[1][b, i])))
    print(f"{shape}: fused against layerwise, max log-prob difference {worst:.3e}")
    assert worst <= 1e-5


# ---- 4. learner -----------------------------------------------------------------------------------------------------------
class _Calls:
    """Counts the calls into the library by symbol while active (tools/mat_bench.py::_CallCounter)."""

    def __enter__(self):
        from mava_amd import _lib

        self.lib, self.by = _lib.lib(), {}
        self.saved = {k: getattr(self.lib, k) for k in _lib._SIGNATURES}
        for k, fn in self.saved.items():
            def wrapped(*a, _fn=fn, _k=k):
                self.by[_k] = self.by.get(_k, 0) + 1
                return _fn(*a)
            setattr(self.lib, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(self.lib, k, fn)


LEARNER = ["env=lbf", "env/scenario=2s-10x10-3p-3f", "arch.num_envs=4", "system.rollout_length=8", "network.acting=fused",
           "network.n_block=2", "network.n_head=2"]


def test_rollout_is_one_launch_per_env_step(dev):
    from mava_amd.mat_learner import MATPass

    cfg, learn, L, _ = tgm._make(dev, LEARNER + ["system.matmul_mode=f32"])
    g = torch.Generator().manual_seed(3)
    L.p.add_((0.05 * torch.randn(L.P, generator=g)).to(dev))
    with _Calls() as calls:
        L._rollout(0)
        torch.cuda.synchronize()
    rep, E, A, nA, T = L.rep, L.E, L.A, L.nA, L.T
    assert calls.by == {"mava_transformer_act_f32": T, "mava_lbf_step": T}, calls.by
    tree = tgm._f64_tree(L)
    tf = MATPass(L.net, E, dev, True, L.ctx)
    tf.idx[:E].copy_(torch.arange(E, dtype=torch.int32))
    worst, compared = 0.0, 0
    for t in range(T):
        obs, mask = rep.agents_view[t].double().cpu(), rep.action_mask[t].bool().cpu()
        u = torch.from_numpy(philox.policy_uniforms(L.seed, t, E * A, nA, 0).astype(np.float64)).view(E, A, nA)
        got = (rep.action[t].long().cpu(), rep.log_prob[t].double().cpu(), rep.value[t].double().cpu())
        assert bool(mask.gather(-1, got[0].unsqueeze(-1)).all()), "an illegal action was sampled"
        compared += compare(got, mm.act(tree, obs, mask, u, 2), f"rollout step {t}", min_frac=0.0)[0]
        # the teacher-forced layer-wise pass on the recorded actions: another summation order than the fused step's
        tf.gather_obs(rep.agents_view[t], E)
        tf.shift_onehot(rep.action[t], A - 1, False)
        tf.encode(L.p)
        tf.decode(L.p)
        logits = tgm._from_t32(tf.logits.t, tf.rows, nA)[: E * A].view(E, A, nA)
        lp_tf = mm.masked_log_softmax(logits, mask)[0].gather(-1, got[0].unsqueeze(-1))[..., 0]
        worst = max(worst, float((lp_tf - got[1]).abs().max()))
    print(f"teacher-forced layer-wise log-probs against the fused rollout's: max difference {worst:.3e}")
    assert worst <= 1e-5
    assert compared >= 0.9 * T * E * A


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_learn_matches_model(dev, mode):
    """tests/test_gpu_mat.py::test_learn_matches_model's method and bounds, with the rollout on the fused step."""
    cfg, learn, L, state = tgm._make(dev, LEARNER + ["system.num_minibatches=2", "system.ppo_epochs=2", f"system.matmul_mode={mode}",
                                                    "system.actor_lr=1e-3"])
    f16, H = mode == "f16x2", 2
    s, rep, T, E, A = cfg.system, L.rep, L.T, L.E, L.A
    assert A == 3 and L.roll.acting == "fused"
    mcfg = {"n_head": H, "clip_eps": float(s.clip_eps), "ent_coef": float(s.ent_coef), "vf_coef": float(s.vf_coef),
            "lr": float(s.actor_lr), "max_grad_norm": float(s.max_grad_norm)}
    count = 0
    L.debug = {"grads": [], "perms": [], "state": []}
    t64 = lambda x: x.double().cpu()
    for upd in range(3):
        for rec in L.debug.values():
            if isinstance(rec, list):
                rec.clear()
        with _Calls() as calls:
            out = learn(state)
        assert calls.by["mava_transformer_act_f32"] == T and "mava_mat_sample_f32" not in calls.by
        state = out.learner_state
        TE = T * E
        adv, tgt = mm.gae(t64(rep.reward).view(T, E * A), t64(rep.value).view(T, E * A), rep.done.cpu().view(T, E * A),
                          t64(rep.last_val).view(E * A), float(s.gamma), float(s.gae_lambda))
        assert_close(rep.adv.cpu().numpy().reshape(T, -1), adv.numpy(), 1e-5, f"update {upd}: advantages")
        view, mask = rep.agents_view[:T].clone(), rep.action_mask[:T].clone()
        view[0], mask[0] = L.debug["slot0"]
        batch = {"obs": t64(view).view(TE, A, -1), "action": rep.action.long().cpu().view(TE, A),
                 "mask": mask.bool().cpu().view(TE, A, -1), "log_prob": t64(rep.log_prob).view(TE, A),
                 "adv": t64(rep.adv).view(TE, A), "value": t64(rep.value).view(TE, A), "target": t64(rep.tgt).view(TE, A)}
        i = 0
        for k in range(L.K):
            perm = L.debug["perms"][k].long().cpu()
            assert sorted(perm.tolist()) == list(range(TE))
            for mb in range(L.M):
                idx = perm[mb * L.Bm : (mb + 1) * L.Bm]
                flat, m, v = (x.double().cpu().numpy() for x in L.debug["state"][i])
                flat, m, v, count, grad, met = mm.minibatch_step(L.net, flat, m, v, count, batch, idx, mcfg)
                what = f"update {upd} epoch {k} minibatch {mb}"
                tgm._compare_grad(L.debug["grads"][i][: L.P].double().cpu().numpy(), grad, f"{what}: gradient", f16)
                assert_close(L.train_metrics[0, k, mb].double().cpu().numpy(), met, 1e-4 if f16 else 1e-5, f"{what}: metrics")
                i += 1
                after = L.debug["state"][i][0] if i < len(L.debug["state"]) else L.p
                tgm._compare_params(after.double().cpu().numpy(), flat, f"{what}: parameters", f16)
        assert int(L.count[0]) == count


# ---- 5. evaluator and refusal ---------------------------------------------------------------------------------------------
def test_evaluator_mode_is_the_models_greedy_choice(dev):
    from mava_amd.types import Observation

    cfg, learn, L, _ = tgm._make(dev, LEARNER + ["system.matmul_mode=f32"])
    g = torch.Generator().manual_seed(4)
    L.p.add_((0.05 * torch.randn(L.P, generator=g)).to(dev))
    rep = L.rep
    ob = Observation(rep.agents_view[0], rep.action_mask[0].bool(), rep.step_count[0])
    params = L.learner_state().params.actor_params
    with _Calls() as calls:
        ga = L.actor_network.apply(params, ob).mode().long().cpu()
    assert calls.by == {"mava_transformer_act_f32": 1}, calls.by
    want, _, _, gap = mm.act(tgm._f64_tree(L), rep.agents_view[0].double().cpu(), rep.action_mask[0].bool().cpu(), None, 2, greedy=True)
    ok = gap.min(-1).values > GAP
    assert bool(ok.any()) and torch.equal(ga[ok], want[ok])


def test_unknown_acting_is_refused_before_any_allocation(dev):
    from mava_amd._lib import MavaHipError

    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MavaHipError, match="network.acting"):
        tgm._make(dev, ["env=lbf", "arch.num_envs=4", "system.rollout_length=8", "network.acting=bogus"])
    assert torch.cuda.memory_allocated() <= before + (1 << 20)  # (the environment's own state at most)


def test_depth_beyond_the_cap_falls_back_to_the_layers(dev):
    from mava_amd._lib import Ctx

    shape = (11, 3, 7, 5, 32, 1, 5)
    c = case(shape)
    with _Calls() as calls:
        got = _act_pass(dev, c["net"], Ctx("f32"), "fused", c, shape[0])
    assert calls.by["mava_transformer_act_f32"] == 1 and calls.by["mava_mat_sample_f32"] == shape[1]
    compare(got, c["want"]["sampled"], f"{shape} fallback")


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
def test_run_experiment(dev, tmp_path, monkeypatch):
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mat

    monkeypatch.chdir(tmp_path)
    recs = []
    cfg = compose("default_ff_mat", ["env=lbf", "env/scenario=2s-8x8-2p-2f-coop", "arch.num_envs=4", "system.rollout_length=8",
                                     "arch.num_eval_episodes=4", "arch.num_absolute_metric_eval_episodes=4", "arch.evaluation_greedy=true",
                                     "system.num_updates=4", "arch.num_evaluation=2", "network.acting=fused"])
    with _Calls() as calls:
        ret = ff_mat.run_experiment(cfg, log=recs.append)
    assert np.isfinite(ret) and len([r for r in recs if "eval_episode_return" in r]) == 2
    for k in ("total_loss", "actor_loss", "value_loss", "entropy"):
        assert np.isfinite(recs[0][k])
    assert calls.by["mava_transformer_act_f32"] > 4 * 8 and "mava_mat_sample_f32" not in calls.by
