"""The PPO minibatch tail (mava_ppo_finish_f32: slab sum launch + Adam launch) against a NumPy restatement of what it is
defined to compute: the f32 column sums and the f64 norm partials in their stated order, bit for bit, for slabs of any row
stride and alignment; clip + Adam against the oracle; the weights of the wide critic's first layer - which
the Adam launch updates in blocks of their own and splits on the spot - bit for bit what the flat lanes give and, through
the next critic launch, bit for bit the split of the stand-alone pack kernel."""
import functools

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

DIN_A, N_ACT = 70, 5
KW = dict(max_norm=0.5, decay=True, steps_per_update=2, num_updates=10, vf_coef=0.5, ent_coef=0.01)
LR_A, LR_C = 1e-3, 2e-3
# the kernels take b1 = 0.9 and b2 = 0.999 as f32: the oracle gets those very numbers (1 - 0.999f is 1.3e-5 off 1e-3)
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))


def _pcount(din, n_out):  # Dense(din,128)-Dense(128,128)-Dense(128,n_out), weights and biases
    return (din + 1) * 128 + 129 * 128 + 129 * n_out


@functools.lru_cache(maxsize=None)
def _slabs(din_c, n_slab, scale, Pa=None, Pc=None):
    """Random slabs [gradient | loss sums] of both networks (read-only: shared between tests).  Pa / Pc: the networks'
    sizes, by default those of the MLPs on DIN_A and din_c inputs (the fused finish takes any)."""
    Pa = _pcount(DIN_A, N_ACT) if Pa is None else Pa
    Pc = _pcount(din_c, 1) if Pc is None else Pc
    rng = np.random.default_rng(1000 * din_c + n_slab)
    a = (rng.standard_normal((n_slab, Pa + 2)) * scale / n_slab).astype(np.float32)
    c = (rng.standard_normal((n_slab, Pc + 1)) * scale / n_slab).astype(np.float32)
    a.setflags(write=False)
    c.setflags(write=False)
    return a, c


def _column_sums(slab):
    """f32 sums in the kernels' order: quarters of ceil(n_slab / 4) slabs, ascending, then ((p0 + p1) + p2) + p3."""
    n = slab.shape[0]
    per = (n + 3) // 4
    part = np.zeros((4, slab.shape[1]), np.float32)
    for q in range(4):
        for b in range(q * per, min(n, (q + 1) * per)):
            part[q] = part[q] + slab[b]
    return ((part[0] + part[1]) + part[2]) + part[3]


@functools.lru_cache(maxsize=None)
def _reduced(din_c, n_slab, scale, grad_scale, Pa=None, Pc=None):
    """g = [actor grad | critic grad | actor_loss, entropy, value_loss] and the (n_partial, 2) f64 norm partials: per network
    the squares of f32(sum * grad_scale) over 64 consecutive virtual columns of [actor Pa + 2 | critic Pc + 1], ascending."""
    a, c = _slabs(din_c, n_slab, scale, Pa, Pc)
    Pa, Pc = a.shape[1] - 2, c.shape[1] - 1
    sa, sc = _column_sums(a), _column_sums(c)
    g = np.concatenate([sa[:Pa], sc[:Pc], sa[Pa:], sc[Pc:]]).astype(np.float32)
    virt = np.concatenate([sa, sc])
    seg = np.concatenate([np.zeros(Pa), -np.ones(2), np.ones(Pc), -np.ones(1)])
    gi = (virt * np.float32(grad_scale)).astype(np.float32).astype(np.float64)
    sq = gi * gi
    n_partial = (virt.size + 63) // 64
    partials = np.zeros((n_partial, 2))
    for s in range(2):
        x = np.where(seg == s, sq, 0.0)
        x = np.concatenate([x, np.zeros(64 * n_partial - x.size)]).reshape(n_partial, 64)
        t = np.zeros(n_partial)
        for k in range(64):
            t = t + x[:, k]
        partials[:, s] = t
    g.setflags(write=False)
    return g, partials


def _norm_from_partials(col):
    """The Adam launch's total: thread t adds partials t, t + 256, ... ascending; a 64-lane shuffle-down tree; 4 waves."""
    n = col.size
    acc = np.zeros(256)
    for b in range(0, n, 256):
        chunk = col[b : b + 256]
        acc[: chunk.size] = acc[: chunk.size] + chunk
    w = acc.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, : 64 - o] = w[:, : 64 - o] + w[:, o:64].copy()  # lanes past 64 - o add their own garbage, never read by lane 0
    t = 0.0
    for i in range(4):
        t = t + w[i, 0]
    return float(np.sqrt(t))


def _layout(a, c, layout, dev):
    """Device slabs as (n_slab, stride) views: stride padded to a multiple of 4 floats on a 16-byte aligned base, the
    unpadded odd stride Pa + 2, or a padded stride behind a base pointer one float off 16-byte alignment.  (A slab sum on
    16-byte loads would take the first and fall back on the other two; the sum as it stands makes no difference.)"""
    out = []
    for x, odd_cols in ((a, a.shape[1]), (c, c.shape[1] + (c.shape[1] % 2 == 0))):
        n, cols = x.shape
        stride = odd_cols if layout == "odd" else (cols + 3) & ~3
        off = 1 if layout == "offset" else 0
        buf = torch.zeros(n * stride + 4, device=dev)
        view = buf[off : off + n * stride].view(n, stride)
        view[:, :cols] = torch.from_numpy(x.copy()).to(dev)
        assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (layout != "offset")
        out.append(view)
    assert (out[0].shape[1] % 2 == 1) == (layout == "odd")
    return out


def _oracle_step(p, m, v, count, g, Pa, grad_scale):
    """Oracle clip + Adam per network on the kernels' scaled f32 gradient; the schedule at the pre-increment count."""
    P = p.size
    outs = []
    for lo, hi, lr, k in ((0, Pa, LR_A, 0), (Pa, P, LR_C, 1)):
        gi = (g[lo:hi] * np.float32(grad_scale)).astype(np.float32)
        frac = 1.0 - (int(count[k]) // KW["steps_per_update"]) / KW["num_updates"]
        outs.append(po.clip_adam(p[lo:hi], gi, m[lo:hi], v[lo:hi], int(count[k]), lr * frac, KW["max_norm"], b1=B1, b2=B2))
    return (np.concatenate([o[i] for o in outs]) for i in range(3))


@pytest.mark.parametrize("layout", ["padded", "odd", "offset"])
@pytest.mark.parametrize("n_slab", [1, 3, 8, 37, 256])
def test_slab_sum_is_the_stated_sum(dev, n_slab, layout):
    """g[:P + 3] and the norm partials of the slab sum launch, bit for bit the NumPy sums in the stated order: fewer slabs
    than quarters (1, 3), exactly one eight-load group per quarter (8... 37 adds a remainder loop), 256 as in the learner."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    din_c, scale, grad_scale = 70, 3.0, 0.5
    a, c = _slabs(din_c, n_slab, scale)
    Pa, Pc = a.shape[1] - 2, c.shape[1] - 1
    P = Pa + Pc
    assert Pa == ops.mlp_param_count(DIN_A, N_ACT) and Pc == ops.mlp_param_count(din_c, 1)
    g_want, partials_want = _reduced(din_c, n_slab, scale, grad_scale)
    slab_a, slab_c = _layout(a, c, layout, dev)
    g = torch.full((P + 4,), 7.0, device=dev)
    p = torch.zeros(P, device=dev)
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = ops.ppo_finish_workspace(Pa, Pc, dev)
    ops.ppo_finish(Ctx("f16x2"), slab_a, slab_c, Pa, Pc, g, p, m, v, count, LR_A, LR_C, grad_scale=grad_scale,
                   metrics_out=torch.zeros(4, device=dev), critic_din=din_c, workspace=ws, **KW)
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert np.array_equal(got[: P + 3].view(np.uint32), g_want.view(np.uint32)), "column sums"
    assert got[P + 3] == 7.0, "the pad behind the loss sums is not written"
    n_partial = partials_want.shape[0]
    got_partials = ws.cpu().numpy()[: 2 * n_partial].reshape(n_partial, 2)
    assert np.array_equal(got_partials.view(np.uint64), partials_want.view(np.uint64)), "norm partials"
    assert count.tolist() == [1, 1]


@pytest.mark.parametrize("big", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("mode", ["f16x2", "f32"])
@pytest.mark.parametrize("din_c", [70, 96, 191, 192, 264, 287])
def test_adam_launch_and_w1_resplit(dev, din_c, mode, big):
    """Three consecutive finish launches on one workspace (ticket reuse, counts [k, k]).  After each: p / m / v against the
    oracle; p / m / v bit-equal to ops.clip_adam from the same state and g - the W1 range comes from the pack blocks there
    and from the flat lanes here -; and the re-split W1 through the next critic launch against a handle that packs itself.
    din_c: 70 no pack; 96 seven steps, the smallest wide layer; 191 / 192 the last width of the 12-step and the first of the
    18-step instantiation; 264 the headline shape; 287 the widest."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    n_slab, grad_scale = 8, 0.5
    scale = 3.0 if big else 1e-3  # clip active / inactive
    a, c = _slabs(din_c, n_slab, scale)
    Pa, Pc = a.shape[1] - 2, c.shape[1] - 1
    P = Pa + Pc
    g_want, partials = _reduced(din_c, n_slab, scale, grad_scale)
    norms = [_norm_from_partials(partials[:, s]) for s in range(2)]
    assert all((np.float32(n) >= np.float32(KW["max_norm"])) == big for n in norms), norms
    slab_a, slab_c = _layout(a, c, "padded", dev)
    rng = np.random.default_rng(din_c)
    p_np = (rng.standard_normal(P) * 0.1).astype(np.float32)
    m_np, v_np = np.zeros(P, np.float32), np.zeros(P, np.float32)
    cnt_np = np.zeros(2, np.int64)
    p2, m2, v2 = (torch.from_numpy(x).to(dev) for x in (p_np, m_np, v_np))
    c2 = torch.zeros(2, dtype=torch.int32, device=dev)
    g2 = torch.zeros(P + 4, device=dev)
    ws = ops.ppo_finish_workspace(Pa, Pc, dev)
    ctx = Ctx(mode)
    wide = mode == "f16x2" and 96 <= din_c <= 287
    TE, A, Rb = 64, 4, 64
    gs = torch.from_numpy(rng.standard_normal((TE, din_c)).astype(np.float32)).to(dev)
    ov = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
    tg = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
    for step in range(3):
        p1, m1, v1, c1 = p2.clone(), m2.clone(), v2.clone(), c2.clone()
        met1, met2 = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
        ops.ppo_finish(ctx, slab_a, slab_c, Pa, Pc, g2, p2, m2, v2, c2, LR_A, LR_C, grad_scale=grad_scale, metrics_out=met2,
                       critic_din=din_c, workspace=ws, **KW)
        ops.clip_adam(p1, g2, m1, v1, c1, [0, Pa, P], [LR_A, LR_C], grad_scale=grad_scale, loss_sums=g2[P:], metrics_out=met1, **KW)
        torch.cuda.synchronize()
        assert np.array_equal(g2.cpu().numpy()[: P + 3].view(np.uint32), g_want.view(np.uint32)), "column sums"
        assert c2.tolist() == c1.tolist() == [step + 1, step + 1]
        assert torch.equal(met1, met2)
        p_np, m_np, v_np = _oracle_step(p_np, m_np, v_np, cnt_np, g_want[:P], Pa, grad_scale)
        cnt_np += 1
        for name, got, flat, want in (("p", p2, p1, p_np), ("m", m2, m1, m_np), ("v", v2, v1, v_np)):
            assert_close(got.cpu().numpy(), want, 2e-6, f"{name} after step {step}")
            assert torch.equal(got.view(torch.int32), flat.view(torch.int32)), f"{name} after step {step}: pack blocks vs flat lanes"
        # (the oracle continues from the kernel's own f32 state: each step is checked on its own)
        p_np, m_np, v_np = (t.cpu().numpy() for t in (p2, m2, v2))
        assert ctx.get(ctx.W1_SPLIT_FRESH) == (1 if wide else 0)
        if wide:
            outs = []
            for c_ in (ctx, Ctx(mode)):
                slab = torch.zeros((3, Pc + 2), device=dev)
                ops.ppo_critic_grad(p2[Pa:], gs, A, ov, tg, None, 0, Rb, A, 0.2, 0.5, slab, ctx=c_)
                torch.cuda.synchronize()
                outs.append(slab.clone())
            assert ctx.get(ctx.W1_SPLIT_FRESH) == 0, "the fresh flag is one-shot"
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "critic gradient on the re-split W1"


@pytest.mark.parametrize("din_c", [150, 264])
def test_adam_launch_on_a_reduced_gradient_carries_the_pack(dev, din_c):
    """n_slab = 0 (several ranks: g is already summed): the Adam launch takes the norms from g and still carries the count
    increment and the W1 re-split."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    grad_scale = 0.5
    g_want, _ = _reduced(din_c, 8, 3.0, grad_scale)
    Pa, Pc = _pcount(DIN_A, N_ACT), _pcount(din_c, 1)
    P = Pa + Pc
    rng = np.random.default_rng(din_c + 1)
    p_np = (rng.standard_normal(P) * 0.1).astype(np.float32)
    g = torch.zeros(P + 4, device=dev)
    g[: P + 3] = torch.from_numpy(g_want.copy()).to(dev)
    p2 = torch.from_numpy(p_np).to(dev)
    m2, v2 = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    c2 = torch.zeros(2, dtype=torch.int32, device=dev)
    p1, m1, v1, c1 = p2.clone(), m2.clone(), v2.clone(), c2.clone()
    ctx = Ctx("f16x2")
    ops.ppo_finish(ctx, None, None, Pa, Pc, g, p2, m2, v2, c2, LR_A, LR_C, grad_scale=grad_scale,
                   metrics_out=torch.zeros(4, device=dev), critic_din=din_c, workspace=ops.ppo_finish_workspace(Pa, Pc, dev), **KW)
    ops.clip_adam(p1, g, m1, v1, c1, [0, Pa, P], [LR_A, LR_C], grad_scale=grad_scale, **KW)
    torch.cuda.synchronize()
    assert c2.tolist() == c1.tolist() == [1, 1]
    z = np.zeros(P, np.float32)
    want = _oracle_step(p_np, z, z, np.zeros(2, np.int64), g_want[:P], Pa, grad_scale)
    for name, got, flat, w in zip("pmv", (p2, m2, v2), (p1, m1, v1), want):
        assert_close(got.cpu().numpy(), w, 2e-6, name)
        assert torch.equal(got.view(torch.int32), flat.view(torch.int32)), f"{name}: pack blocks vs flat lanes"
    assert ctx.get(ctx.W1_SPLIT_FRESH) == 1
    TE, A = 64, 4
    gs = torch.from_numpy(rng.standard_normal((TE, din_c)).astype(np.float32)).to(dev)
    ov = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
    tg = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
    outs = []
    for c_ in (ctx, Ctx("f16x2")):
        slab = torch.zeros((3, Pc + 2), device=dev)
        ops.ppo_critic_grad(p2[Pa:], gs, A, ov, tg, None, 0, TE, A, 0.2, 0.5, slab, ctx=c_)
        torch.cuda.synchronize()
        outs.append(slab.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "critic gradient on the re-split W1"
