"""GPU: the soft actor-critic kernels (csrc/sac.hip) one by one against tests/sac_model.py, then a whole train step of
ff_isac and ff_masac from an identical state: the Q, actor and log_alpha gradients at the project's gradient tolerance
(1e-4 of rms), the polyak step, the policy-delay rule and the noise repeated across the delay."""
import math

import numpy as np
import pytest
import torch

from tests import sac_model as sm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHAPES = [(32, 32, 1), (96, 96, 3), (64, 40, 5)]  # (rows, n_real, A): B = 32 with A = 1 and A = 3; B * A = 40, padded
DIMS = [1, 2, 5, 16]
SENT = 7.5  # outputs start from this value: a padding row must be overwritten with 0


def _lib():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr()


def _t32(x: torch.Tensor) -> torch.Tensor:
    """(rows, N) -> the T32 layout, on the host side of the test (not with the library's converter)."""
    rows, N = x.shape
    return x.view(rows // 32, 32, N).permute(0, 2, 1).contiguous().view(-1)


def _rows(t: torch.Tensor, rows: int, N: int) -> torch.Tensor:
    return t.view(rows // 32, N, 32).permute(0, 2, 1).reshape(rows, N)


def _np(t):
    return t.detach().cpu().double().numpy()


# ---- 1. item replay ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 4], ids=["isac", "masac"])
def test_replay_ring_and_sample_across_a_wrap(dev, S):
    L, check, ptr, st = _lib()
    cap, E, A, O, D, B = 64, 24, 3, 5, 2, 32
    Rp, seed = 96, 0x1234567890
    g = torch.Generator().manual_seed(2)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=dev)
    buf = {"obs": z(cap, A, O), "action": z(cap, A, D), "reward": z(cap, A), "done": z(cap, A, dtype=torch.uint8),
           "next_obs": z(cap, A, O), "gs": z(cap, max(S, 1)), "next_gs": z(cap, max(S, 1))}
    host = {k: v.cpu().numpy().copy() for k, v in buf.items()}
    gsp = lambda t: ptr(t) if S else None
    head, n_added = 0, 0
    for add in range(3):  # the third add wraps: slots 48..63, 0..7
        new = {"obs": torch.randn(E, A, O, generator=g), "action": torch.rand(E, A, D, generator=g) * 2 - 1,
               "reward": torch.randn(E, A, generator=g), "done": (torch.rand(E, generator=g) < 0.3).to(torch.uint8),
               "next_obs": torch.randn(E, A, O, generator=g), "gs": torch.randn(E, max(S, 1), generator=g),
               "next_gs": torch.randn(E, max(S, 1), generator=g)}
        dv = {k: v.to(dev) for k, v in new.items()}
        check(L.mava_sac_replay_add_f32(E, A, O, D, S, cap, head, ptr(dv["obs"]), ptr(dv["action"]), ptr(dv["reward"]), ptr(dv["done"]),
                                        ptr(dv["next_obs"]), gsp(dv["gs"]), gsp(dv["next_gs"]), ptr(buf["obs"]), ptr(buf["action"]),
                                        ptr(buf["reward"]), ptr(buf["done"]), ptr(buf["next_obs"]), gsp(buf["gs"]), gsp(buf["next_gs"]), st),
              "add")
        slots = sm.ring_slots(head, E, cap)
        for k in host:
            if k == "done":
                host[k][slots] = new[k].numpy()[:, None]
            elif S or "gs" not in k:
                host[k][slots] = new[k].numpy()
        head, n_added = (head + E) % cap, n_added + E
        for k in host:
            assert np.array_equal(buf[k].cpu().numpy(), host[k]), (add, k)
        out = {"obs": z(Rp, O) + SENT, "action": z(Rp, D) + SENT, "reward": z(Rp) + SENT, "done": z(Rp, dtype=torch.uint8) + 9,
               "next_obs": z(Rp, O) + SENT, "gs": z(B, max(S, 1)), "next_gs": z(B, max(S, 1))}
        index = z(B, dtype=torch.int32)
        check(L.mava_sac_replay_sample_f32(A, O, D, S, cap, n_added, B, Rp, seed, add + 5, ptr(buf["obs"]), ptr(buf["action"]),
                                           ptr(buf["reward"]), ptr(buf["done"]), ptr(buf["next_obs"]), gsp(buf["gs"]), gsp(buf["next_gs"]),
                                           ptr(out["obs"]), ptr(out["action"]), ptr(out["reward"]), ptr(out["done"]), ptr(out["next_obs"]),
                                           gsp(out["gs"]), gsp(out["next_gs"]), ptr(index), st), "sample")
        want = sm.sampled_items(seed, add + 5, B, n_added, cap)
        assert np.array_equal(index.cpu().numpy(), want)
        if add == 2:
            assert len(set(want.tolist()) & set(range(8))) > 0  # items of the wrapped part are drawn
        for k in ("obs", "action", "reward", "done", "next_obs"):
            got = out[k].cpu().numpy()
            assert np.array_equal(got[: B * A].reshape((B, A) + host[k].shape[2:]), host[k][want]), (add, k)  # rows b * A + agent
        if S:
            assert np.array_equal(out["gs"].cpu().numpy(), host["gs"][want]) and np.array_equal(out["next_gs"].cpu().numpy(), host["next_gs"][want])
    lib_err = L.mava_sac_replay_add_f32(65, A, O, D, S, cap, 0, *([None] * 14), st)
    assert lib_err <= -1000


# ---- 2. reparameterised sample ------------------------------------------------------------------------------------------------
def _policy_inputs(rows, D, gen):
    """means with components in the inner branch and, in columns 0 mod 3 of every fourth row, far in each clipped branch"""
    mean = 1.2 * torch.randn(rows, D, generator=gen)
    r = torch.arange(rows)
    mean[r % 4 == 1, 0::3] = 6.0
    mean[r % 4 == 3, 0::3] = -6.0
    raw = -2.0 + 0.5 * torch.randn(rows, D, generator=gen)
    return mean, raw


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"rows{s[0]}real{s[1]}")
def test_sample_and_log_prob(dev, shape, D):
    L, check, ptr, st = _lib()
    rows, n_real, _A = shape
    gen = torch.Generator().manual_seed(rows + D)
    mean, raw = _policy_inputs(rows, D, gen)
    a, lp, eps = (torch.full(s, SENT, device=dev) for s in ((rows, D), (rows,), (rows, D)))
    mean_d, raw_d = _t32(mean).to(dev), _t32(raw).to(dev)  # (kept alive: the calls below take their addresses)
    args = (rows, n_real, D, 1e-3, ptr(mean_d), ptr(raw_d), 77, 5, 1000)
    check(L.mava_sac_sample_f32(*args, ptr(a), ptr(lp), ptr(eps), st), "sample")
    a_, lp_, eps_ = a.cpu(), lp.cpu(), eps.cpu()
    assert (a_[n_real:] == 0).all() and (lp_[n_real:] == 0).all() and (eps_[n_real:] == 0).all()
    m64, r64, e64 = mean[:n_real].double(), raw[:n_real].double(), eps_[:n_real].double()
    scale = sm.scale_of(r64, 1e-3)
    assert_close(_np(a_[:n_real]), _np(torch.tanh(m64 + scale * e64)), 1e-5, "action")
    want = sm.log_prob_terms(a_[:n_real].double(), m64, scale).sum(-1)  # of the kernel's own action
    assert_close(_np(lp_[:n_real]), _np(want), 1e-5, "log_prob")
    clipped = a_[:n_real].abs() >= sm.THRESH
    assert clipped.any() and (~clipped).any() and (a_[:n_real][clipped] > 0).any() and (a_[:n_real][clipped] < 0).any()
    # the noise: standard normals of (row_offset + row, step, component); another step draws others; NULL outputs are skipped
    if n_real * D >= 64:
        assert abs(float(eps_[:n_real].mean())) < 0.5 and 0.5 < float(eps_[:n_real].std()) < 1.5
    a2 = torch.empty_like(a)
    check(L.mava_sac_sample_f32(*args, ptr(a2), None, None, st), "sample")
    assert torch.equal(a2, a)
    check(L.mava_sac_sample_f32(*args[:7], 6, 1000, ptr(a2), None, None, st), "sample")
    assert not torch.equal(a2[:n_real], a[:n_real])


# ---- 3. Q target and loss --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"rows{s[0]}real{s[1]}")
def test_q_target_and_loss(dev, shape, nblk):
    L, check, ptr, st = _lib()
    rows, n_real, A = shape
    gen = torch.Generator().manual_seed(rows)
    q1, q2, q1t, q2t, lpn, rew = (torch.randn(rows, generator=gen) * 2 for _ in range(6))
    done = (torch.rand(rows, generator=gen) < 0.3).to(torch.uint8)
    la = torch.randn(A, generator=gen) * 0.5
    gamma, gscale = 0.97, 64.0
    dq1, dq2, tgt = (torch.full((rows,), SENT, device=dev) for _ in range(3))
    part = torch.full((nblk, 4), SENT, device=dev)
    keep = [t.to(dev) for t in (q1, q2, q1t, q2t, lpn, rew, done, la)]
    check(L.mava_sac_q_loss_f32(rows, n_real, A, *(ptr(t) for t in keep), gamma, gscale, ptr(dq1), ptr(dq2), ptr(tgt), ptr(part), nblk, st),
          "q_loss")
    n = n_real
    f = lambda t: t[:n].double()
    alpha = torch.exp(la.double())[torch.arange(n) % A]
    want_t = f(rew) + (1.0 - f(done)) * gamma * (torch.minimum(f(q1t), f(q2t)) - alpha * f(lpn))
    assert_close(_np(tgt[:n]), _np(want_t), 1e-5, "target")
    assert (want_t[done[:n] == 1] == f(rew)[done[:n] == 1]).all() and done[:n].any()
    for got, q, name in ((dq1, q1, "dq1"), (dq2, q2, "dq2")):
        assert_close(_np(got[:n]) / gscale, _np(2.0 * (f(q) - want_t) / n), 1e-4, name)
        assert (got[n:] == 0).all()
    want = [((f(q1) - want_t) ** 2).mean(), ((f(q2) - want_t) ** 2).mean(), f(q1).mean(), f(q2).mean()]
    assert_close(_np(part).sum(0), np.array([float(v) for v in want]), 1e-5, "loss partials", scale=1.0)


# ---- 4. concatenation, joint actions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True], ids=["isac", "masac"])
def test_q_input_and_joint_actions(dev, joint):
    L, check, ptr, st = _lib()
    B, A, D, O = 11, 3, 2, 5  # 33 real rows of 64
    rows, n_real = 64, B * A
    gen = torch.Generator().manual_seed(4)
    state = torch.randn((B, O) if joint else (n_real, O), generator=gen)
    act, new = torch.randn(rows, D, generator=gen), torch.randn(rows, D, generator=gen)
    W = A * D if joint else D
    K, ld = O + W, 32
    for use_new in (False, True):
        x = torch.full((rows * ld,), SENT, device=dev)
        sd, ad, nd = state.to(dev), act.to(dev), new.to(dev)
        check(L.mava_sac_concat_f32(rows, n_real, O, A if joint else 1, A, D, int(joint), ptr(sd), ptr(ad), ptr(nd) if use_new else None,
                                    ptr(x), ld, st), "concat")
        got = _rows(x.cpu(), rows, ld)
        assert (got[n_real:] == 0).all() and (got[:, K:] == 0).all()
        a3, n3 = act[:n_real].view(B, A, D).double(), new[:n_real].view(B, A, D).double()
        if joint:
            block = sm.get_updated_joint_actions(a3, n3) if use_new else sm.get_joint_action(a3)
            st_rows = state.double().unsqueeze(1).expand(B, A, O)
        else:
            block = n3 if use_new else a3
            st_rows = state.double().view(B, A, O)
        want = torch.cat([st_rows, block], -1).reshape(n_real, K)
        assert torch.equal(got[:n_real, :K].double(), want)
    assert L.mava_sac_concat_f32(rows, n_real, O, 1, A, D, int(joint), ptr(sd), ptr(ad), None, ptr(x), K - 1, st) <= -1000


# ---- 5. actor gradient ------------------------------------------------------------------------------------------------------------
def _actor_case(rows, n_real, A, D, joint, gen):
    O = 7
    K = O + (A * D if joint else D)
    mean = 1.0 * torch.randn(rows, D, generator=gen)
    raw = -2.0 + 0.5 * torch.randn(rows, D, generator=gen)
    eps = torch.randn(rows, D, generator=gen).clamp(-2.5, 2.5)
    r = torch.arange(rows)
    # both clipped branches, at tail masses that are neither 0 nor 1: mean +-4.2 with scale ~0.3 and the noise kept small
    for sel, v in ((r % 4 == 1, 4.2), (r % 4 == 3, -4.2)):
        mean[sel, 0::3] = v
        raw[sel, 0::3] = -1.1
        eps[sel, 0::3] = eps[sel, 0::3].clamp(-0.5, 0.5)
    scale = sm.scale_of(raw.double(), 1e-3)
    a = torch.tanh(mean.double() + scale * eps.double()).float()
    q1, q2 = torch.randn(rows, generator=gen), torch.randn(rows, generator=gen)
    dx1, dx2 = torch.randn(rows, K, generator=gen), torch.randn(rows, K, generator=gen)
    la = 0.5 * torch.randn(A, generator=gen)
    return O, K, mean, raw, eps, a, q1, q2, dx1, dx2, la


def _actor_want(n, A, D, O, joint, mean, raw, eps, a, q1, q2, dx1, dx2, la):
    """autograd through the sample, the Q networks replaced by their first-order expansion around the action"""
    m = mean[:n].double().requires_grad_(True)
    rw = raw[:n].double().requires_grad_(True)
    act, lp = sm.sample(m, rw, eps[:n].double(), 1e-3)
    agent = torch.arange(n) % A
    cols = (O + (agent * D if joint else torch.zeros_like(agent))).unsqueeze(1) + torch.arange(D).unsqueeze(0)
    lin = lambda q, dx: q[:n].double() + (torch.gather(dx[:n].double(), 1, cols) * (act - act.detach())).sum(-1)
    alpha = torch.exp(la.double())[agent]
    loss = (alpha * lp - torch.minimum(lin(q1, dx1), lin(q2, dx2))).mean()
    gm, gr = torch.autograd.grad(loss, [m, rw])
    return gm, gr, loss.item(), lp.mean().item(), (a[:n].abs() >= sm.THRESH)


# every shape at every action width, and MASAC's case: the own slot of the joint action, read back from dX at O + agent * D
ACTOR_CASES = [(s, D, False) for s in SHAPES for D in DIMS] + [((32, 30, 3), 2, True)]


@pytest.mark.parametrize("shape,D,joint", ACTOR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_actor_gradient(dev, shape, D, joint):
    L, check, ptr, st = _lib()
    rows, n_real, A = shape
    gen = torch.Generator().manual_seed(rows * 17 + D)
    O, K, mean, raw, eps, a, q1, q2, dx1, dx2, la = _actor_case(rows, n_real, A, D, joint, gen)
    qscale, gscale = 4.0, 128.0
    dm, dr = torch.full((rows * D,), SENT, device=dev), torch.full((rows * D,), SENT, device=dev)
    ref = None
    for nblk in (1, 8):
        part = torch.full((nblk, 2), SENT, device=dev)
        keep = [t.to(dev) for t in (_t32(mean), _t32(raw), eps, a, la, q1, q2, _t32(dx1 * qscale), _t32(dx2 * qscale))]
        check(L.mava_sac_actor_grad_f32(rows, n_real, A, D, 1e-3, *(ptr(t) for t in keep), K, O, int(joint), qscale, gscale, ptr(dm),
                                        ptr(dr), ptr(part), nblk, st), "actor_grad")
        gm, gr, loss, mean_lp, clipped = _actor_want(n_real, A, D, O, joint, mean, raw, eps, a, q1, q2, dx1, dx2, la)
        assert_close(_np(part).sum(0), np.array([loss, mean_lp]), 1e-5, f"loss partials, {nblk} blocks", scale=1.0)
        got = (_rows(dm.cpu(), rows, D), _rows(dr.cpu(), rows, D))
        if ref is None:
            ref = got
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert clipped.any() and (~clipped).any()
    assert_close(_np(ref[0][:n_real]) / gscale, _np(gm), 1e-4, "d mean")
    assert_close(_np(ref[1][:n_real]) / gscale, _np(gr), 1e-4, "d raw log_std")
    assert (ref[0][n_real:] == 0).all() and (ref[1][n_real:] == 0).all()
    if D > 1:  # the clipped components' gradient is the tail mass's, not zero
        assert float(gm[clipped].abs().max()) > 1e-6


# ---- 6. alpha --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"rows{s[0]}real{s[1]}")
def test_alpha_loss_and_gradient(dev, shape):
    L, check, ptr, st = _lib()
    rows, n_real, A = shape
    gen = torch.Generator().manual_seed(rows + 1)
    lp, la = torch.randn(rows, generator=gen) * 3, torch.randn(A, generator=gen) * 0.5
    te = -5.0 * 2
    grad, parts = torch.full((A,), SENT, device=dev), torch.full((A,), SENT, device=dev)
    lpd, lad = lp.to(dev), la.to(dev)
    check(L.mava_sac_alpha_loss_f32(n_real, A, ptr(lpd), ptr(lad), te, ptr(grad), ptr(parts), st), "alpha")
    la64 = la.double().requires_grad_(True)
    loss = (-torch.exp(la64).view(1, A) * (lp[:n_real].double().view(-1, A) + te)).mean()
    (g,) = torch.autograd.grad(loss, [la64])
    assert_close(_np(grad), _np(g), 1e-5, "d log_alpha")
    assert_close(np.array([_np(parts).sum()]), np.array([loss.item()]), 1e-5, "alpha loss", scale=1.0)


# ---- 7. a whole train step ---------------------------------------------------------------------------------------------------------------
def _setup(dev, system, overrides=()):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.sac_learner import learner_setup

    central = system == "ff_masac"
    cfg = compose(f"default_{system}_spread", ["arch.num_envs=8", "system.buffer_size=256", "system.explore_steps=64", "system.batch_size=16",
                                        "system.epochs=1", "system.rollout_length=2", *overrides])
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, actor, state = learner_setup(env, (3, 4, 5, 6, 7, 8), cfg, central, device=dev)
    L = learn.learner
    L.debug = {k: [] for k in ("actions", "index", "eps_q", "eps_actor", "eps_alpha", "g_q", "g_actor", "g_alpha", "target")}
    return cfg, learn, L, state


def _model_of(L):
    ly = lambda net: [l.N for l in net.layers]
    an, qn = L.actor_network.net, L.q_network.net
    return sm.Sac(sm.Net(L.O, ly(an), [L.D, L.D]), sm.Net(L.Kq, ly(qn), [1]), L.A, L.D, L.centralised, L.gamma, L.min_scale,
                  L.target_entropy)


def _params(L):
    Pq = L.Pq
    c = lambda t: t.detach().cpu().double().clone()
    return {"actor": c(L.pa), "q1": c(L.pq[:Pq]), "q2": c(L.pq[Pq:]), "q1_t": c(L.pqt[:Pq]), "q2_t": c(L.pqt[Pq:]), "log_alpha": c(L.log_alpha)}


def _batch(L, index):
    i = index.cpu().long()
    c = lambda t: t.detach().cpu()[i].double()
    b = L.buf
    out = {"obs": c(b.obs[0]), "next_obs": c(b.next_obs[0]), "action": c(b.action), "reward": c(b.reward), "done": c(b.done)}
    if L.centralised:
        out["gs"], out["next_gs"] = c(b.obs[1]), c(b.next_obs[1])
    return out


@pytest.mark.parametrize("system", ["ff_isac", "ff_masac"])
def test_train_step_gradients_match_the_model(dev, system):
    """policy_update_delay = 1: one Q, one actor and one alpha update from a known state.  The actor gradient is taken at the
    learner's own updated Q parameters and the alpha gradient at its own updated actor, so every comparison starts from an
    identical state and Adam's amplification of near-eps entries stays out of it (conftest.check_and_sync_f16x2_state)."""
    _cfg, learn, L, state = _setup(dev, system, ["system.policy_update_delay=1"])
    learn.explore()
    assert L.n_added == 64 and L.t == 64
    # a log_alpha away from 0 and a `done` in the buffer, so that neither drops out of the target
    L.log_alpha.copy_(torch.tensor([0.3, -0.2, 0.1], device=dev))
    L.buf.done[::3] = 1
    before = _params(L)
    learn(state)
    torch.cuda.synchronize()
    after = _params(L)
    model, dbg = _model_of(L), L.debug
    B, A, D = L.B, L.A, L.D
    batch = _batch(L, dbg["index"][0])
    assert np.array_equal(dbg["index"][0].cpu().numpy(), sm.sampled_items(L.seed, 0, B, L.n_added, L.cap))
    assert batch["done"].sum() > 0
    eps = lambda k: dbg[k][0][: B * A].cpu().double().view(B, A, D)
    g1, g2, info = model.q_grads(before, batch, eps("eps_q"))
    assert_close(_np(dbg["target"][0][: B * A]), _np(info["target"].reshape(-1)), 1e-4, "target")
    assert_close(_np(dbg["g_q"][0][: L.Pq]), _np(g1), 1e-4, "q1 gradient")
    assert_close(_np(dbg["g_q"][0][L.Pq:]), _np(g2), 1e-4, "q2 gradient")
    mid = dict(before, q1=after["q1"], q2=after["q2"])  # the actor step sees the updated Q networks
    ga, loss = model.actor_grad(mid, batch, eps("eps_actor"))
    assert_close(_np(dbg["g_actor"][0]), _np(ga), 1e-4, "actor gradient")
    gl, aloss = model.alpha_grad(dict(mid, actor=after["actor"]), batch, eps("eps_alpha"))
    assert_close(_np(dbg["g_alpha"][0]), _np(gl), 1e-4, "log_alpha gradient")
    assert not torch.equal(dbg["eps_actor"][0], dbg["eps_alpha"][0]) and not torch.equal(dbg["eps_q"][0], dbg["eps_actor"][0])
    tm = L.train_metrics[0, 0].cpu().double().numpy()
    assert_close(tm, np.array([info["q1_loss"], info["q2_loss"], info["mean_q1"], info["mean_q2"], loss, aloss]), 1e-4, "metrics")
    # the polyak step after the Q update (tau), on the learner's own new online parameters
    for k in ("q1", "q2"):
        assert_close(_np(after[k + "_t"]), _np(sm.polyak(after[k], before[k + "_t"], L.tau)), 1e-6, f"{k} target")
    assert not torch.equal(after["log_alpha"], before["log_alpha"]) and L.count.tolist() == [1, 1, 1]


@pytest.mark.parametrize("system", ["ff_isac", "ff_masac"])
def test_policy_delay_two_repeats_the_update_with_the_same_noise(dev, system):
    _cfg, learn, L, state = _setup(dev, system, ["system.policy_update_delay=2", "system.autotune=false"])
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


def test_policy_delay_reads_the_env_step_counter(dev):
    """num_envs = 5, rollout_length = 1, delay = 2: t = 0, 5, 10 entering the three update steps - the actor trains in
    the first and the third, whatever the epoch."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.sac_learner import learner_setup

    cfg = compose("default_ff_isac_spread", ["arch.num_envs=5", "system.buffer_size=64", "system.explore_steps=0", "system.batch_size=8",
                                      "system.epochs=3", "system.rollout_length=1", "system.policy_update_delay=2"])
    cfg.system.num_updates_per_eval = 3
    env, _ = envs.make(cfg, device=dev)
    learn, _actor, state = learner_setup(env, (3, 4, 5, 6, 7, 8), cfg, False, device=dev)
    out = learn(state)
    torch.cuda.synchronize()
    L = learn.learner
    assert L.t == 15 and L.count.tolist() == [2 * 3 * 2, 9, 2 * 3 * 2]  # (updates that fire) * epochs * delay
    al = out.train_metrics["actor_loss"].cpu()
    assert (al[1] == 0).all() and (al[0] != 0).all() and (al[2] != 0).all()
    assert all(bool(torch.isfinite(v).all()) for v in out.train_metrics.values())


def test_refusals(dev):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.sac_learner import learner_setup
    from mava_amd.systems.sac import ff_isac, ff_masac

    env, _ = envs.make(compose("default_ff_isac_spread"), device=dev)
    keys = (1, 2, 3, 4, 5, 6)
    with pytest.raises(NotImplementedError, match="update_batch_size"):
        learner_setup(env, keys, compose("default_ff_isac_spread", ["system.update_batch_size=2"]), False, device=dev)
    with pytest.raises(ValueError, match="ContinuousActionHead"):
        learner_setup(env, keys, compose("default_ff_isac_spread", ["network=mlp"]), False, device=dev)
    with pytest.raises(NotImplementedError, match="CNN critic"):
        ff_masac._check_config(compose("default_ff_masac_spread", ["network=cnn", "network.action_head._target_=mava.networks.ContinuousActionHead"]))
    lbf, _ = envs.make(compose("default_ff_ippo", ["env=lbf", "arch.num_envs=16"]), device=dev)
    with pytest.raises(ValueError, match="continuous actions"):
        learner_setup(lbf, keys, compose("default_ff_isac_spread"), False, device=dev)
    with pytest.raises(ValueError, match="continuous actions"):
        ff_isac._check_config(compose("default_ff_isac_spread", ["env=lbf"]))
    with pytest.raises(ValueError, match="Global state"):
        learner_setup(env, keys, compose("default_ff_masac_spread"), True, device=dev)
