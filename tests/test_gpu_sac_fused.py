"""GPU: the fused soft actor-critic kernels (csrc/sac_fused.hip) through the C ABI against tests/sac_model.py (float64) at
the project's f16x2 gradient tolerance (1e-4 of rms), then a whole train step with MAVA_SAC_FUSED=1
and the fallback outside the envelope.  Shapes: (A 3, D 2, B 12) two tiles of 30 and 6 real rows; (A 2, D 1, B 16) a full
tile; (A 5, D 16, B 7) the widest action, MASAC's Kq = 100.  Input widths 15 and 16 sit on and past a 16-deep k-step.
The edges of the envelope, the noise and the refusals are in tests/test_gpu_sac_fused_edges.py."""
import math

import numpy as np
import pytest
import torch

from tests import sac_model as sm
from tests.conftest import assert_close
from tests.test_gpu_sac import _batch, _model_of, _np, _params, _setup

pytestmark = pytest.mark.gpu

GAMMA, MIN_SCALE, SEED, SENT = 0.97, 1e-3, 0x1234567890ABCDEF, 7.5
# (A, D, B, O, S): isac Kq = O + D = 15, 16, 36; masac Kq = S + A D = 16, 15, 100
CASES = [(3, 2, 12, 13, 10), (2, 1, 16, 15, 13), (5, 16, 7, 20, 20)]
GRID = [(c, j) for c in CASES for j in (False, True)]
IDS = [f"A{c[0]}D{c[1]}B{c[2]}-{'masac' if j else 'isac'}" for c, j in GRID]


def _flat(net: sm.Net, gen, head_scale=1.0):
    feat = net.layer_sizes[-1]
    dims = list(zip([net.din] + net.layer_sizes[:-1], net.layer_sizes)) + [(feat, n) for n in net.head_sizes]
    parts = []
    for i, (k, n) in enumerate(dims):
        gain = head_scale if i >= len(net.layer_sizes) else 1.4
        parts += [gain * torch.randn(k, n, generator=gen, dtype=torch.float64).reshape(-1) / math.sqrt(k),
                  0.1 * gain * torch.randn(n, generator=gen, dtype=torch.float64)]
    return torch.cat(parts).float().double()  # float32 values: the kernels and the model see the same numbers


def _case(dev, case, joint, head_scale=1.0, seed=None):
    A, D, B, O, S = case
    gen = torch.Generator().manual_seed(7 + A + D if seed is None else seed)
    Kq = S + A * D if joint else O + D
    model = sm.Sac(sm.Net(O, [128, 128], [D, D]), sm.Net(Kq, [128, 128], [1]), A, D, joint, GAMMA, MIN_SCALE, -float(D))
    p = {"actor": _flat(model.actor, gen, head_scale), "log_alpha": torch.tensor([0.3, -0.2, 0.1, 0.25, -0.15][:A], dtype=torch.float64)}
    for k in ("q1", "q2", "q1_t", "q2_t"):
        p[k] = _flat(model.q, gen)
    r = lambda *s: torch.randn(*s, generator=gen).double()
    batch = {"obs": r(B, A, O), "next_obs": r(B, A, O), "action": torch.tanh(r(B, A, D)).float().double(), "reward": r(B, A),
             "done": (torch.rand(B, 1, generator=gen) < 0.4).double().expand(B, A).contiguous(), "gs": r(B, S), "next_gs": r(B, S)}
    assert 0 < batch["done"].sum() < B * A
    f = lambda t: t.float().contiguous().to(dev)
    d = {k: f(v) for k, v in batch.items()}
    d["done"] = batch["done"].to(torch.uint8).contiguous().to(dev)
    d.update(actor=f(p["actor"]), q=f(torch.cat([p["q1"], p["q2"]])), q_t=f(torch.cat([p["q1_t"], p["q2_t"]])), la=f(p["log_alpha"]))
    n_tiles = -(-B // (32 // A))
    return model, p, batch, d, n_tiles


def _abi():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr()


@pytest.mark.parametrize("case,joint", GRID, ids=IDS)
def test_q_update_against_the_model(dev, case, joint):
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _case(dev, case, joint)
    L, check, ptr, s = _abi()
    Pq, BA = model.q.num_params, B * A
    stride = 2 * Pq + 3  # a slab wider than the gradient: the stride is honoured
    slab = torch.full((n_tiles, stride), SENT, device=dev)
    part, tgt, eps = torch.full((n_tiles, 4), SENT, device=dev), torch.full((BA,), SENT, device=dev), torch.full((BA, D), SENT, device=dev)
    check(L.mava_sac_q_update_f32(int(joint), B, A, O, D, S, ptr(d["obs"]), ptr(d["next_obs"]), ptr(d["action"]), ptr(d["reward"]),
                                  ptr(d["done"]), ptr(d["gs"]), ptr(d["next_gs"]), ptr(d["actor"]), ptr(d["q"]), ptr(d["q_t"]), ptr(d["la"]),
                                  GAMMA, MIN_SCALE, SEED, 5, ptr(slab), stride, ptr(part), ptr(tgt), ptr(eps), s), "mava_sac_q_update_f32")
    torch.cuda.synchronize()
    g1, g2, info = model.q_grads(p, batch, eps.cpu().double().view(B, A, D))
    got = slab[:, : 2 * Pq].sum(0)
    assert torch.equal(slab[:, 2 * Pq:], torch.full((n_tiles, 3), SENT, device=dev))
    assert_close(_np(tgt), _np(info["target"].reshape(-1)), 1e-4, "target")
    assert_close(_np(got[:Pq]), _np(g1), 1e-4, "q1 gradient")
    assert_close(_np(got[Pq:]), _np(g2), 1e-4, "q2 gradient")
    assert_close(_np(part.sum(0)), np.array([info["q1_loss"], info["q2_loss"], info["mean_q1"], info["mean_q2"]]), 1e-4, "metric sums")


@pytest.mark.parametrize("case,joint", GRID, ids=IDS)
def test_actor_update_against_the_model(dev, case, joint):
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _case(dev, case, joint, head_scale=3.0)
    L, check, ptr, s = _abi()
    Pa, BA = model.actor.num_params, B * A
    slab, part = torch.full((n_tiles, Pa), SENT, device=dev), torch.full((n_tiles, 2), SENT, device=dev)
    eps, logp = torch.full((BA, D), SENT, device=dev), torch.full((BA,), SENT, device=dev)
    call = lambda mode, step, lp: check(L.mava_sac_actor_update_f32(
        mode, int(joint), B, A, O, D, S, ptr(d["obs"]), ptr(d["action"]), ptr(d["gs"]), ptr(d["actor"]), ptr(d["q"]), ptr(d["la"]), MIN_SCALE,
        SEED, step, ptr(slab), Pa, ptr(part), lp, ptr(eps), s), "mava_sac_actor_update_f32")
    call(0, 6, None)
    torch.cuda.synchronize()
    e64 = eps.cpu().double().view(B, A, D)
    a = model.pi(p["actor"], batch["obs"], e64)[0].abs()
    assert (a >= sm.THRESH).any() and (a < sm.THRESH).any()  # both branches of the clipped log-prob
    g, loss = model.actor_grad(p, batch, e64)
    assert_close(_np(slab.sum(0)), _np(g), 1e-4, "actor gradient")
    assert_close(_np(part.sum(0)[:1]), np.array([loss]), 1e-4, "actor loss")
    call(1, 7, ptr(logp))
    torch.cuda.synchronize()
    e64 = eps.cpu().double().view(B, A, D)
    assert_close(_np(logp), _np(model.pi(p["actor"], batch["obs"], e64)[1].reshape(-1)), 1e-4, "log_prob")


@pytest.mark.parametrize("system", ["ff_isac", "ff_masac"])
def test_fused_train_step_gradients_match_the_model(dev, system, monkeypatch):
    """test_train_step_gradients_match_the_model's comparisons on the fused path, and no product or concat launch inside it."""
    from mava_amd import _lib

    monkeypatch.setenv("MAVA_SAC_FUSED", "1")
    _cfg, learn, L, state = _setup(dev, system, ["system.policy_update_delay=1"])
    assert L.fused
    learn.explore()
    L.log_alpha.copy_(torch.tensor([0.3, -0.2, 0.1], device=dev))
    L.buf.done[::3] = 1
    before = _params(L)
    names, step = [], L._train_step

    def counted(n, k, t):
        _lib.TIMERS = {}
        try:
            step(n, k, t)
            names.extend(_lib.TIMERS)
        finally:
            _lib.TIMERS = None

    monkeypatch.setattr(L, "_train_step", counted)
    learn(state)
    torch.cuda.synchronize()
    assert {"sac_q_update", "sac_actor_update"} <= set(names) and not [k for k in names if k.startswith("gen_") or k == "sac_concat"]
    after = _params(L)
    model, dbg = _model_of(L), L.debug
    B, A, D = L.B, L.A, L.D
    batch = _batch(L, dbg["index"][0])
    assert batch["done"].sum() > 0
    eps = lambda k: dbg[k][0][: B * A].cpu().double().view(B, A, D)
    g1, g2, info = model.q_grads(before, batch, eps("eps_q"))
    assert_close(_np(dbg["target"][0][: B * A]), _np(info["target"].reshape(-1)), 1e-4, "target")
    assert_close(_np(dbg["g_q"][0][: L.Pq]), _np(g1), 1e-4, "q1 gradient")
    assert_close(_np(dbg["g_q"][0][L.Pq:]), _np(g2), 1e-4, "q2 gradient")
    mid = dict(before, q1=after["q1"], q2=after["q2"])
    ga, loss = model.actor_grad(mid, batch, eps("eps_actor"))
    assert_close(_np(dbg["g_actor"][0]), _np(ga), 1e-4, "actor gradient")
    gl, aloss = model.alpha_grad(dict(mid, actor=after["actor"]), batch, eps("eps_alpha"))
    assert_close(_np(dbg["g_alpha"][0]), _np(gl), 1e-4, "log_alpha gradient")
    assert not torch.equal(dbg["eps_actor"][0], dbg["eps_alpha"][0]) and not torch.equal(dbg["eps_q"][0], dbg["eps_actor"][0])
    tm = L.train_metrics[0, 0].cpu().double().numpy()
    assert_close(tm, np.array([info["q1_loss"], info["q2_loss"], info["mean_q1"], info["mean_q2"], loss, aloss]), 1e-4, "metrics")
    for k in ("q1", "q2"):
        assert_close(_np(after[k + "_t"]), _np(sm.polyak(after[k], before[k + "_t"], L.tau)), 1e-6, f"{k} target")
    assert L.count.tolist() == [1, 1, 1]


@pytest.mark.parametrize("system", ["ff_isac", "ff_masac"])
def test_fused_policy_delay_two_repeats_the_update_with_the_same_noise(dev, system, monkeypatch):
    """test_gpu_sac's test of the same name, on the fused path."""
    monkeypatch.setenv("MAVA_SAC_FUSED", "1")
    _cfg, learn, L, state = _setup(dev, system, ["system.policy_update_delay=2", "system.autotune=false"])
    assert L.fused
    learn.explore()
    before = _params(L)
    learn(state)  # t = 64 entering the update: 64 % 2 == 0, the actor trains - twice
    torch.cuda.synchronize()
    after, dbg = _params(L), L.debug
    assert sm.policy_fires(64, 2) and len(dbg["g_actor"]) == 2 and L.count.tolist() == [2, 1, 0]
    assert torch.equal(dbg["eps_actor"][0], dbg["eps_actor"][1]) and not torch.equal(dbg["g_actor"][0], dbg["g_actor"][1])
    for k in ("q1", "q2"):
        assert_close(_np(after[k + "_t"]), _np(sm.polyak(after[k], before[k + "_t"], L.tau)), 1e-6, f"{k} target")
    # autotune off: log_alpha keeps log(init_alpha) and reports no alpha loss
    assert torch.equal(after["log_alpha"], before["log_alpha"]) and abs(float(after["log_alpha"][0]) - math.log(0.1)) < 1e-6
    assert float(L.train_metrics[0, 0, 5]) == 0.0 and dbg["g_alpha"] == []


def test_outside_the_envelope_the_layer_wise_path_runs(dev, monkeypatch):
    monkeypatch.setenv("MAVA_SAC_FUSED", "1")
    _cfg, learn, L, state = _setup(dev, "ff_isac", ["network.critic_network.pre_torso.layer_sizes=[64,64]"])
    assert not L.fused and not hasattr(L, "slab_q")
    learn.explore()
    learn(state)
    torch.cuda.synchronize()
    assert L.count.tolist()[1] == 1 and torch.isfinite(L.train_metrics).all()
