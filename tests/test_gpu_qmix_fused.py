"""GPU: the fused mixer kernel (csrc/qmix_fused.hip) through the C ABI against float64 autograd of tests/qmix_model.py's
hypernetworks + mix_raw + the TD loss, at the project's f16x2 gradient tolerance (1e-4 of the tensor's rms, BASELINE.md
section 2) and 1e-4 on the metrics; then learn() with MAVA_QMIX_FUSED=1 against QMIXModel step by step."""
import math

import numpy as np
import pytest
import torch

from tests import qmix_model as xm
from tests import test_gpu_qmix as tq
from tests.conftest import assert_close
from tests.iql_model import F32_MIN
from tests.test_gpu_iql import _eq, _from_t32, _np, _t, _to_t32

pytestmark = pytest.mark.gpu

GAMMA, SENT = 0.99, 9.0
c32 = tq.c32
# (L, B, A, O, actions, Em, Hh)
CASES = [
    (1, 1, 1, 5, 2, 1, 1),        # one real row in a tile; every width at its minimum
    (2, 33, 2, 7, 3, 32, 64),     # two tiles per step; Rp != Bp * A; Ds = 14
    (2, 5, 3, 21, 5, 32, 64),     # the default widths; Ds = 63
    (1, 32, 16, 9, 4, 32, 128),   # A * Em = 512, Hh at its edge; Ds = 144 crosses the state chunks
    (1, 3, 2, 70, 32, 64, 40),    # Em at its edge; Hh no multiple of 32; Ds = 140; 32 actions
]


def _case(L, B, A, O, nA, Em, Hh, garbage=0):
    """Random inputs: next-Q values a permutation of a 0.5-spaced ladder plus +-0.1 (no ties: the top two differ by >= 0.3),
    continuous states and parameters.  `garbage` reseeds what lies in the agent rows past B * A alone."""
    rng = np.random.default_rng(11)
    Rp, Ds, n_real = c32(B * A), A * O, B * A
    c = {k: rng.standard_normal((L, Rp, nA)).astype(np.float32) for k in ("q", "qt")}
    c["qn"] = (rng.permuted(np.tile(0.5 * np.arange(nA), (L, Rp, 1)), axis=-1) + rng.uniform(-0.1, 0.1, (L, Rp, nA))).astype(np.float32)
    c["mask"] = rng.random((L, Rp, nA)) < 0.6
    c["mask"][..., 0] = True
    c["act"] = rng.integers(0, nA, (L, Rp)).astype(np.int32)
    c["rew"] = rng.standard_normal((L, Rp)).astype(np.float32)
    c["term"] = (rng.random((L, Rp)) < 0.3).astype(np.uint8)
    c["obs"], c["nobs"] = (rng.standard_normal((L, Rp, O)).astype(np.float32) for _ in range(2))
    flat = []
    for _ in range(2):  # online, target: kernels ~ 1 / sqrt(fan-in), output kernels smaller (OUT_SCALE's role), biases 0.1
        parts = [rng.standard_normal(s) * ((0.3 if n.endswith("k1") or n == "b1_k" else 1.4) / math.sqrt(s[0]) if len(s) == 2 else 0.1)
                 for n, s in xm.mixer_shapes(Ds, A, Em, Hh)]
        flat.append(np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32))
    c["p"], c["pt"] = flat
    if garbage:
        g = np.random.default_rng(garbage)
        for k in ("q", "qt", "qn", "rew", "obs", "nobs"):
            c[k][:, n_real:] = g.standard_normal(c[k][:, n_real:].shape)
        c["act"][:, n_real:] = g.integers(0, nA, (L, Rp - n_real))
        c["term"][:, n_real:] ^= 1
        c["mask"][:, n_real:, 1:] ^= True
    c.update(L=L, B=B, A=A, O=O, nA=nA, Em=Em, Hh=Hh, Rp=Rp, Bp=c32(B), Ds=Ds, gs=float(2 ** math.ceil(math.log2(L * max(Rp, c32(B))))))
    return c


def _want(c):
    """float64: (dq in units of gs (L, Rp, nA), the mixer's gradient, [q_loss, mean_q, mean_target])."""
    L, B, A, nA, Ds, Em, Hh = (c[k] for k in ("L", "B", "A", "nA", "Ds", "Em", "Hh"))
    n = B * A
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    q, p = t(c["q"]).requires_grad_(True), t(c["p"]).requires_grad_(True)
    z = torch.where(torch.from_numpy(c["mask"][:, :n]), t(c["qn"])[:, :n], torch.full((L, n, nA), float(F32_MIN), dtype=torch.float64))
    top = z.topk(2, -1).values if nA > 1 else None
    assert top is None or (top[..., 0] - top[..., 1] >= 1e-3).all()
    nq = t(c["qt"])[:, :n].gather(-1, z.argmax(-1, keepdim=True))[..., 0].reshape(L, B, A)
    qa = q[:, :n].gather(-1, torch.from_numpy(c["act"][:, :n]).long().unsqueeze(-1))[..., 0].reshape(L, B, A)
    q_tot = xm.mix_raw(qa, *xm.hyper(xm.unpack(p, Ds, A, Em, Hh), t(c["obs"])[:, :n].reshape(L, B, Ds)))
    with torch.no_grad():
        q_tot_t = xm.mix_raw(nq, *xm.hyper(xm.unpack(t(c["pt"]), Ds, A, Em, Hh), t(c["nobs"])[:, :n].reshape(L, B, Ds)))
        y = t(c["rew"])[:, :n].reshape(L, B, A).mean(-1) + (1.0 - t(c["term"])[:, :n].reshape(L, B, A)[..., 0]) * GAMMA * q_tot_t
    loss = ((q_tot - y) ** 2).mean()
    loss.backward()
    return q.grad.numpy() * c["gs"], p.grad.numpy(), np.array([float(loss.detach()), float(q_tot.detach().mean()), float(y.mean())])


def _run(dev, c, n_slab, ctx=None, **over):
    """One launch on sentinel-filled outputs: (return code, dq, slab)."""
    from mava_amd._lib import Ctx, lib, ptr, stream_ptr

    a = dict(c, **over)
    L, Rp, nA = c["L"], c["Rp"], c["nA"]
    f3 = lambda x: _t(_to_t32(x.reshape(L * Rp, nA)), dev)
    ins = [_t(c["obs"], dev), _t(c["nobs"], dev), _t(c["act"], dev), _t(c["rew"], dev), _t(c["term"], dev), _t(c["mask"].astype(np.uint8), dev),
           f3(c["q"]), f3(c["qn"]), f3(c["qt"]), _t(c["p"], dev), _t(c["pt"], dev)]
    Pm = c["p"].size
    dq, slab = torch.full((L * Rp * nA,), SENT, device=dev), torch.full((n_slab, Pm + 5), SENT, device=dev)
    ctx = Ctx("f16x2") if ctx is None else ctx
    rc = lib().mava_qmix_mixer_update_f32(ctx.handle, L, a["B"], a["A"], a["O"], a["Rp"], a["nA"], a["Em"], a["Hh"], *[ptr(x) for x in ins],
                                          GAMMA, c["gs"], ptr(dq), ptr(slab), Pm + 5, n_slab, stream_ptr())
    torch.cuda.synchronize()
    return rc, _np(dq), _np(slab)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_kernel_matches_f64_autograd(dev, case):
    c = _case(*case)
    L, B, A, nA, Rp, Ds, Em, Hh = (c[k] for k in ("L", "B", "A", "nA", "Rp", "Ds", "Em", "Hh"))
    n_slab = 3  # tiles stride over the blocks; with fewer tiles a slab stays idle
    rc, dq, slab = _run(dev, c, n_slab)
    assert rc == 0
    Pm = c["p"].size
    assert (slab[:, Pm + 3:] == SENT).all()  # the stride is honoured
    idle = np.arange(n_slab) >= L * c["Bp"] // 32
    assert (slab[idle, : Pm + 3] == 0.0).all()
    want_dq, want_g, want_m = _want(c)
    got_dq = _from_t32(dq, L * Rp, nA).reshape(L, Rp, nA)
    taken = np.zeros((L, Rp, nA), bool)
    np.put_along_axis(taken, c["act"][..., None].astype(np.int64), True, -1)
    taken[:, B * A:] = False
    assert (got_dq[~taken] == 0.0).all()  # exact zeros off the taken action and on padding rows
    print(f"dq ratio {tq._ratio(got_dq, want_dq):.3g}")
    assert_close(got_dq, want_dq, 1e-4, "dq")
    got, off = slab[:, :Pm].astype(np.float64).sum(0), 0
    for name, shape in xm.mixer_shapes(Ds, A, Em, Hh):
        n = int(np.prod(shape))
        print(f"{name} ratio {tq._ratio(got[off:off + n], want_g[off:off + n]):.3g}")
        assert_close(got[off:off + n], want_g[off:off + n], 1e-4, name)
        off += n
    print(f"metrics ratio {tq._ratio(slab[:, Pm:Pm + 3].sum(0), want_m):.3g}")
    assert_close(slab[:, Pm:Pm + 3].astype(np.float64).sum(0), want_m, 1e-4, "metrics")
    # deterministic: a second launch is bit-identical
    _, dq2, slab2 = _run(dev, c, n_slab)
    _eq(dq2, dq, "dq of a second launch")
    _eq(slab2, slab, "slabs of a second launch")


def test_padding_rows_contribute_exact_zeros(dev):
    case = CASES[1]  # B = 33: 31 padding mixer rows in the second tile, 30 padding agent rows
    (_, dq, slab), (_, dq_g, slab_g) = _run(dev, _case(*case), 4), _run(dev, _case(*case, garbage=5), 4)
    _eq(slab_g, slab, "slabs with other values in the padding rows")
    _eq(dq_g, dq, "dq with other values in the padding rows")


@pytest.mark.parametrize("over,msg", [
    ({"A": 17}, b"agents"), ({"nA": 33}, b"actions"), ({"Em": 65}, b"Em=65"), ({"Hh": 129}, b"Hh=129"),
    ({"A": 16, "Em": 33, "Rp": 64}, b"A*Em=528"), ({"Rp": 48}, b"multiple of 32"), ({"ctx": "f32"}, b"f16x2"),
])
def test_refusals_launch_nothing(dev, over, msg):
    from mava_amd._lib import Ctx, lib

    over = dict(over)
    ctx = Ctx(over.pop("ctx", "f16x2"))
    rc, dq, slab = _run(dev, _case(*CASES[2]), 2, ctx=ctx, **over)
    assert rc <= -1000 and msg in lib().mava_last_error()
    assert (dq == SENT).all() and (slab == SENT).all()


def test_learn_fused_matches_model(dev, monkeypatch):
    """tests/test_gpu_qmix.py::test_learn_matches_model itself (f16x2: its allowance) on the fused path."""
    monkeypatch.setenv("MAVA_QMIX_FUSED", "1")
    seen, case = [], tq._learner_case
    monkeypatch.setattr(tq, "_learner_case", lambda *a, **k: seen.append(case(*a, **k)) or seen[-1])
    tq.test_learn_matches_model(dev, "qmix", "f16x2")
    L = seen[0][1]
    assert L.fused is True and L.slab.shape[1] == L.Pm + 3
    assert not any(hasattr(L, k) for k in ("hp", "hp_target", "mstate", "mstate_next", "d_w1", "d_b1", "d_w2", "d_b2"))
