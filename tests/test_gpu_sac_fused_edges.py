"""GPU: the fused soft actor-critic kernels (csrc/sac_fused.hip) at the edges of their envelope, their noise, their reads
and writes, their refusals, and the fused learner next to the layer-wise one.

1. Both kernels against tests/sac_model.py (float64) at shapes (A, D, B, O, S) that reach: A = MAX_A with two-row items and
   Kq = 127 (16, 16, 5, 111, 1); O = Kq = 127 with the fourth wave of dX = dZ1 W1^T active (7, 16, 9, 127, 15); MASAC's own
   slot across a wave boundary (7, 5, 9, 9, 3); A = 1 with 32 items per tile, D = 9, O = 1 (1, 9, 70, 1, 1); 10 padding rows
   per tile and Kq = 64 exactly (11, 3, 5, 33, 31); 26 tiles (3, 2, 256, 13, 10).
   Bound: every quantity is held to max(1e-4, 4 x floor) of its rms, where `floor` is the float32 evaluation of the model
   against its float64 evaluation on the same inputs and the same noise - computed from the model alone - and the factor 4
   is the one tests/test_gpu_rec_out_continuous.py grants its wide cases (split-f16 operands on top of f32 accumulation).
   Every floor must itself stay at or below 2.5e-4, so no bound exceeds 1e-3.  The cases use head_scale = 1.0: with the 3.0
   of test_gpu_sac_fused's actor test (which reaches both log-prob branches, and keeps asserting that) the model's own
   float32 floor, measured on the CPU, reaches 2.8e-3 at (7, 5, 9, masac) and 1.0e-3 for the target at (3, 2, 256, masac),
   because the clipped log-prob branch is ill-conditioned.  `pytest -s` prints floor, bound and error per case and quantity.
   Worst measured error / bound per quantity (MI355X): target 0.14 (3, 2, 256, masac), q1 gradient 0.29 and q2 gradient 0.16
   (7, 16, 9, masac, where the floor lifts the q1 bound to 1.18e-4), metric sums 0.013, actor gradient 0.029 (7, 5, 9, masac),
   actor loss 0.069, mean log-prob 0.025 and log-prob 0.099 (1, 9, 70).  The largest floor is the actor gradient's at
   (1, 9, 70): 1.15e-4 isac, 1.39e-4 masac (bounds 4.6e-4 and 5.6e-4; measured errors 3.9e-6 and 5.3e-6 of rms).
2. The noise is mava_sac_sample_f32's bit for bit, and Box-Muller over oracle/philox.py within 1e-5 (|eps| <= 5.8 for 24-bit
   uniforms, a float32 ulp there is 4.8e-7: about 20 ulp for the device's logf, cosf and sqrtf; measured: at most 1.2e-6).
3. Guard tails behind every output stay untouched, inputs followed by NaN give the same bits, a second launch gives the
   same bits.
4. done = 1 or gamma = 0 make the target the reward, bit for bit.
5. Outside the envelope the entry points return 1, on bad arguments a code <= -1000; neither launches anything.
6. ff_isac / ff_masac built twice from the same seeds, fused and layer-wise: the same indices and noise, the same gradients
   within 2e-4 of rms (each path is held to 1e-4 of the model; measured: at most 2.9e-6, the actor gradient).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sac_model as sm
from tests.conftest import assert_close
from tests.test_gpu_sac import _np, _setup
from tests.test_gpu_sac_fused import GAMMA, MIN_SCALE, SEED, SENT, _abi, _case

pytestmark = pytest.mark.gpu

GUARD, FLOOR_CAP = 64, 2.5e-4
BENCH, ONE_AGENT, PADDED = (3, 2, 256, 13, 10), (1, 9, 70, 1, 1), (11, 3, 5, 33, 31)
# ((A, D, B, O, S), joint)
EDGES = [((16, 16, 5, 111, 1), False), ((7, 16, 9, 127, 15), True), ((7, 5, 9, 9, 3), True), (ONE_AGENT, False), (ONE_AGENT, True),
         (PADDED, False), (PADDED, True), (BENCH, False), (BENCH, True)]
NOISE = [(BENCH, False), (ONE_AGENT, True)]
STRAY = [(PADDED, True), (ONE_AGENT, False)]


def _id(v):
    return "A%dD%dB%dO%dS%d" % v[0] + ("-masac" if v[1] else "-isac")


def _ids(grid):
    return [_id(v) for v in grid]


def _edge_case(dev, case, joint, seed=None):
    """test_gpu_sac_fused._case at head_scale 1.0, with a log_alpha drawn per agent (all entries distinct)."""
    A, D, B, O, S = case
    assert A <= 16 and D <= 16 and O <= 127 and (S + A * D if joint else O + D) <= 127  # inside served()
    model, p, batch, d, n_tiles = _case(dev, case, joint, head_scale=1.0, seed=seed)
    la = (0.4 * torch.randn(A, generator=torch.Generator().manual_seed(100 + A))).float()
    assert len(set(la.tolist())) == A
    p["log_alpha"], d["la"] = la.double(), la.to(dev)
    return model, p, batch, d, n_tiles


def _guards(slab, n_tiles, P, *vectors):
    """The slab region the kernel owns was NaN and is finite; everything behind an output's end still holds the sentinel."""
    assert torch.isfinite(slab[:n_tiles, :P]).all(), "slab entries left unwritten"
    assert (slab[:n_tiles, P:] == SENT).all() and (slab[n_tiles:] == SENT).all(), "slab written past the parameters or the tiles"
    for name, v, n in vectors:
        assert (v[n:] == SENT).all(), f"{name} written past its end"


def _q_launch(dev, model, case, joint, d, step=5, gamma=GAMMA):
    """mava_sac_q_update_f32 into outputs with guard tails: 64 elements, a slab stride 3 past the parameters, one slab row."""
    A, D, B, O, S = case
    L, check, ptr, s = _abi()
    P, BA, n_tiles = 2 * model.q.num_params, B * A, -(-B // (32 // A))
    slab = torch.full((n_tiles + 1, P + 3), SENT, device=dev)
    slab[:n_tiles, :P] = float("nan")
    part, tgt, eps = (torch.full((n + GUARD,), SENT, device=dev) for n in (4 * n_tiles, BA, BA * D))
    check(L.mava_sac_q_update_f32(int(joint), B, A, O, D, S, ptr(d["obs"]), ptr(d["next_obs"]), ptr(d["action"]), ptr(d["reward"]),
                                  ptr(d["done"]), ptr(d["gs"]), ptr(d["next_gs"]), ptr(d["actor"]), ptr(d["q"]), ptr(d["q_t"]), ptr(d["la"]),
                                  gamma, MIN_SCALE, SEED, step, ptr(slab), P + 3, ptr(part), ptr(tgt), ptr(eps), s), "mava_sac_q_update_f32")
    torch.cuda.synchronize()
    _guards(slab, n_tiles, P, ("partials", part, 4 * n_tiles), ("target", tgt, BA), ("eps", eps, BA * D))
    return SimpleNamespace(slab=slab[:n_tiles, :P], part=part[: 4 * n_tiles].view(n_tiles, 4), tgt=tgt[:BA], eps=eps[: BA * D].view(BA, D))


def _actor_launch(dev, model, case, joint, d, mode, step):
    """mava_sac_actor_update_f32 likewise.  Mode 0 leaves log_prob alone, mode 1 the slab and the partials."""
    A, D, B, O, S = case
    L, check, ptr, s = _abi()
    P, BA, n_tiles = model.actor.num_params, B * A, -(-B // (32 // A))
    slab = torch.full((n_tiles + 1, P + 3), SENT, device=dev)
    if mode == 0:
        slab[:n_tiles, :P] = float("nan")
    part, logp, eps = (torch.full((n + GUARD,), SENT, device=dev) for n in (2 * n_tiles, BA, BA * D))
    check(L.mava_sac_actor_update_f32(mode, int(joint), B, A, O, D, S, ptr(d["obs"]), ptr(d["action"]), ptr(d["gs"]), ptr(d["actor"]),
                                      ptr(d["q"]), ptr(d["la"]), MIN_SCALE, SEED, step, ptr(slab), P + 3, ptr(part), ptr(logp), ptr(eps), s),
          "mava_sac_actor_update_f32")
    torch.cuda.synchronize()
    if mode == 0:
        _guards(slab, n_tiles, P, ("partials", part, 2 * n_tiles), ("log_prob", logp, 0), ("eps", eps, BA * D))
    else:
        assert (slab == SENT).all(), "mode 1 wrote the slab"
        _guards(slab, 0, P, ("partials", part, 0), ("log_prob", logp, BA), ("eps", eps, BA * D))
    return SimpleNamespace(slab=slab[:n_tiles, :P], part=part[: 2 * n_tiles].view(n_tiles, 2), logp=logp[:BA], eps=eps[: BA * D].view(BA, D))


# ---- the model's quantities, in the precision of what it is given ---------------------------------------------------------
def _f32(tree):
    return {k: v.float() for k, v in tree.items()}


def _q_quantities(model, p, batch, eps):
    g1, g2, info = model.q_grads(p, batch, eps)
    return {"target": _np(info["target"].reshape(-1)), "q1 gradient": _np(g1), "q2 gradient": _np(g2),
            "metric sums": np.array([info["q1_loss"], info["q2_loss"], info["mean_q1"], info["mean_q2"]], np.float64)}


def _actor_quantities(model, p, batch, eps_grad, eps_logp):
    g, loss = model.actor_grad(p, batch, eps_grad)
    pi = lambda eps: model.pi(p["actor"], batch["obs"], eps)[1]
    return {"actor gradient": _np(g), "actor loss": np.array([loss], np.float64), "mean log_prob": np.array([float(pi(eps_grad).mean())]),
            "log_prob": _np(pi(eps_logp).reshape(-1))}


def _rel(a, b):
    """The smallest rtol at which conftest.assert_close(a, b, rtol) passes: max |a - b| / (|b| + rms(b))."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + np.sqrt(np.mean(b * b)))))


def _hold(tag, got, want, low, keep=None):
    """Each quantity of `got` within max(1e-4, 4 x floor) of `want` (float64); floor = the float32 model `low` against `want`."""
    rows = []
    for name in want:
        sel = slice(None) if keep is None or name not in keep else keep[name]
        floor = _rel(low[name][sel], want[name][sel])
        bound, err = max(1e-4, 4.0 * floor), _rel(got[name][sel], want[name][sel])
        rows.append((name, floor, bound, err))
        print(f"\n{tag:26s} {name:14s} floor {floor:.2e} bound {bound:.2e} error {err:.2e} ratio {err / bound:.3f}", end="")
    for name, floor, bound, err in rows:
        assert floor <= FLOOR_CAP, f"{tag} {name}: the float32 floor {floor:.2e} is above {FLOOR_CAP}: the case is ill-conditioned"
    for name, floor, bound, err in rows:
        assert err <= bound, f"{tag} {name}: error {err:.3e} of rms above the bound {bound:.3e} (floor {floor:.2e})"


# ---- 1. against the model at the edge shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,joint", EDGES, ids=_ids(EDGES))
def test_q_update_at_the_edges(dev, case, joint):
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _edge_case(dev, case, joint)
    out = _q_launch(dev, model, case, joint, d, step=5)
    Pq = model.q.num_params
    eps = out.eps.cpu().view(B, A, D)
    got = {"target": _np(out.tgt), "q1 gradient": _np(out.slab.sum(0)[:Pq]), "q2 gradient": _np(out.slab.sum(0)[Pq:]),
           "metric sums": _np(out.part.sum(0))}
    _hold(_id((case, joint)), got, _q_quantities(model, p, batch, eps.double()), _q_quantities(model, _f32(p), _f32(batch), eps))


@pytest.mark.parametrize("case,joint", EDGES, ids=_ids(EDGES))
def test_actor_update_at_the_edges(dev, case, joint):
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _edge_case(dev, case, joint)
    grad = _actor_launch(dev, model, case, joint, d, 0, 6)
    logp = _actor_launch(dev, model, case, joint, d, 1, 7)
    e0, e1 = grad.eps.cpu().view(B, A, D), logp.eps.cpu().view(B, A, D)
    got = {"actor gradient": _np(grad.slab.sum(0)), "actor loss": _np(grad.part.sum(0)[:1]), "mean log_prob": _np(grad.part.sum(0)[1:]),
           "log_prob": _np(logp.logp)}
    _hold(_id((case, joint)), got, _actor_quantities(model, p, batch, e0.double(), e1.double()),
          _actor_quantities(model, _f32(p), _f32(batch), e0, e1))


# ---- 2. the noise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,joint", NOISE, ids=_ids(NOISE))
def test_noise_is_the_layer_wise_samplers(dev, case, joint):
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _edge_case(dev, case, joint)
    L, check, ptr, s = _abi()
    BA = B * A
    rows = -(-BA // 32) * 32
    assert BA >= 64
    zeros, drawn = torch.zeros(rows * D, device=dev), []
    for step in (5, 6, 7):
        act, eps = torch.empty(rows, D, device=dev), torch.full((rows, D), SENT, device=dev)
        check(L.mava_sac_sample_f32(rows, BA, D, MIN_SCALE, ptr(zeros), ptr(zeros), SEED, step, 0, ptr(act), None, ptr(eps), s), "sample")
        torch.cuda.synchronize()
        want = eps[:BA]
        fused = {"q update": _q_launch(dev, model, case, joint, d, step=step).eps,
                 "actor update, mode 0": _actor_launch(dev, model, case, joint, d, 0, step).eps,
                 "actor update, mode 1": _actor_launch(dev, model, case, joint, d, 1, step).eps}
        for name, got in fused.items():
            assert torch.equal(got, want), f"{name}, step {step}: not the noise of mava_sac_sample_f32"
        host = sm.sac_noise(SEED, step, BA, D)
        err = float(np.abs(_np(want) - host).max())
        print(f"\n{_id((case, joint))} step {step}: max |eps - host Box-Muller| {err:.2e}", end="")
        assert err <= 1e-5, (step, err)
        drawn.append(want.clone())
    assert not any(torch.equal(drawn[i], drawn[j]) for i, j in ((0, 1), (0, 2), (1, 2)))  # another step, other noise
    assert not torch.equal(drawn[0][:32], drawn[0][32:64])  # the second tile's rows are not the first's


# ---- 3. stray reads and writes, and the same bits twice -----------------------------------------------------------------------
def _behind_nan(d):
    """The batch at the front of larger buffers whose remainder is NaN (255 for done)."""
    out = dict(d)
    for k in ("obs", "next_obs", "action", "reward", "gs", "next_gs"):
        out[k] = torch.cat([d[k].reshape(-1), torch.full((4096,), float("nan"), device=d[k].device)])
    out["done"] = torch.cat([d["done"].reshape(-1), torch.full((4096,), 255, dtype=torch.uint8, device=d["done"].device)])
    return out


@pytest.mark.parametrize("case,joint", STRAY, ids=_ids(STRAY))
def test_nothing_outside_the_batch_is_read_or_written(dev, case, joint):
    model, p, batch, d, n_tiles = _edge_case(dev, case, joint)

    def launches(data):  # (the guard tails are checked inside each launch)
        return (_q_launch(dev, model, case, joint, data, step=5), _actor_launch(dev, model, case, joint, data, 0, 6),
                _actor_launch(dev, model, case, joint, data, 1, 7))

    first, again, behind = launches(d), launches(d), launches(_behind_nan(d))
    for what, other in (("a second launch", again), ("inputs followed by NaN", behind)):
        for kernel, a, b in zip(("q update", "actor update mode 0", "actor update mode 1"), first, other):
            for name in vars(a):
                assert torch.equal(getattr(a, name), getattr(b, name)), f"{kernel}: {name} differs with {what}"


# ---- 4. exact properties of the target ----------------------------------------------------------------------------------------
def test_target_is_the_reward_where_nothing_is_bootstrapped(dev):
    case, joint = BENCH, False
    A, D, B, O, S = case
    model, p, batch, d, n_tiles = _edge_case(dev, case, joint)
    reward = d["reward"].reshape(-1)
    ones, zeros = torch.ones_like(d["done"]), torch.zeros_like(d["done"])
    assert torch.equal(_q_launch(dev, model, case, joint, dict(d, done=ones)).tgt, reward)
    assert torch.equal(_q_launch(dev, model, case, joint, dict(d, done=zeros), gamma=0.0).tgt, reward)
    free = _q_launch(dev, model, case, joint, dict(d, done=zeros)).tgt
    assert not (free == reward).any()  # (the bootstrap term is there when asked for)
    # mixed: done rows are the reward exactly, the others the model's target at part 1's bound
    done = d["done"].reshape(-1).bool()
    assert done.any() and not done.all()
    out = _q_launch(dev, model, case, joint, d)
    assert torch.equal(out.tgt[done], reward[done])
    eps = out.eps.cpu().view(B, A, D)
    want, low = (_q_quantities(model, q, b, e) for q, b, e in ((p, batch, eps.double()), (_f32(p), _f32(batch), eps)))
    live = (~done).cpu().numpy()
    _hold("bootstrapped rows", {"target": _np(out.tgt)}, {"target": want["target"]}, low, keep={"target": live})


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
BASE = dict(mode=0, joint=0, B=4, A=3, O=13, D=2, S=10, min_scale=MIN_SCALE, stride=0, null=())
OUTSIDE = [dict(A=17), dict(D=17), dict(O=128), dict(O=120, D=8), dict(joint=1, S=100, A=7, D=4)]
BAD = [dict(B=0), dict(joint=1, S=0), dict(joint=1, null=("gs",)), dict(stride=-1), dict(min_scale=-1e-3), dict(null=("obs",))]
BAD_ACTOR = [dict(mode=2), dict(mode=1, null=("logp",))]


@pytest.mark.parametrize("entry", ["q_update", "actor_update"])
def test_refusals_launch_nothing(dev, entry):
    """Every buffer is far larger than any of the shapes below needs; the outputs start from the sentinel and keep it."""
    L, _check, ptr, s = _abi()
    n = 1 << 18
    b = {k: torch.zeros(n, device=dev) for k in ("obs", "next_obs", "action", "reward", "gs", "next_gs", "actor", "q", "q_t", "la")}
    b["done"] = torch.zeros(n, dtype=torch.uint8, device=dev)
    outs = {k: torch.full((n,), SENT, device=dev) for k in ("slab", "part", "tgt", "eps", "logp")}
    b.update(outs)
    for over, outside in [(o, True) for o in OUTSIDE] + [(o, False) for o in BAD + (BAD_ACTOR if entry == "actor_update" else [])]:
        a = SimpleNamespace(**dict(BASE, **over))
        Kq = a.S + a.A * a.D if a.joint else a.O + a.D
        g = lambda k: None if k in a.null else ptr(b[k])
        if entry == "q_update":
            stride = 2 * sm.Net(Kq, [128, 128], [1]).num_params + a.stride
            rc = L.mava_sac_q_update_f32(a.joint, a.B, a.A, a.O, a.D, a.S, g("obs"), g("next_obs"), g("action"), g("reward"), g("done"), g("gs"),
                                         g("next_gs"), g("actor"), g("q"), g("q_t"), g("la"), GAMMA, a.min_scale, SEED, 5, g("slab"), stride,
                                         g("part"), g("tgt"), g("eps"), s)
        else:
            stride = sm.Net(a.O, [128, 128], [a.D, a.D]).num_params + a.stride
            rc = L.mava_sac_actor_update_f32(a.mode, a.joint, a.B, a.A, a.O, a.D, a.S, g("obs"), g("action"), g("gs"), g("actor"), g("q"), g("la"),
                                             a.min_scale, SEED, 5, g("slab"), stride, g("part"), g("logp"), g("eps"), s)
        torch.cuda.synchronize()
        assert (rc == 1) if outside else (rc <= -1000), (entry, over, rc)
        for k, t in outs.items():
            assert (t == SENT).all(), (entry, over, k)


# ---- 6. the fused learner next to the layer-wise one ----------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["ff_isac", "ff_masac"])
def test_fused_and_layer_wise_learners_agree(dev, system, monkeypatch):
    """Built twice from the same seeds: the same sampled items and the same three noise draws bit for bit, and the first train
    step's target and gradients within 2e-4 of rms - each path is held to 1e-4 of the model."""
    runs = {}
    for fused in (False, True):
        monkeypatch.setenv("MAVA_SAC_FUSED", "1" if fused else "0")
        _cfg, learn, L, state = _setup(dev, system, ["system.policy_update_delay=1"])
        assert L.fused is fused
        learn.explore()
        L.log_alpha.copy_(torch.tensor([0.3, -0.2, 0.1], device=dev))  # (as test_gpu_sac: alpha and done stay in the target)
        L.buf.done[::3] = 1
        learn(state)
        torch.cuda.synchronize()
        runs[fused] = L.debug
    BA = L.B * L.A
    lw, fu = runs[False], runs[True]
    assert all(len(lw[k]) == len(fu[k]) >= 1 for k in lw)
    assert torch.equal(lw["index"][0], fu["index"][0])
    for k in ("eps_q", "eps_actor", "eps_alpha"):
        assert torch.equal(lw[k][0][:BA], fu[k][0][:BA]), k
    pairs = [(k, _np(fu[k][0][:BA] if k == "target" else fu[k][0]), _np(lw[k][0][:BA] if k == "target" else lw[k][0]))
             for k in ("target", "g_q", "g_actor", "g_alpha")]
    for k, a, b in pairs:
        print(f"\n{system} {k:8s} fused against layer-wise: {_rel(a, b):.2e} of rms", end="")
    for k, a, b in pairs:
        assert_close(a, b, 2e-4, k)
