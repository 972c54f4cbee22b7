"""GPU: the direct convolution kernels (csrc/conv_direct.hip) through the C ABI, GenericNet's conv="direct" switch and the
learner's MAVA_CONV_DIRECT opt-in.  Reference: torch.nn.functional.conv2d in float64 on the CPU with flax's 'SAME' padding
applied by hand, and its autograd.  Bounds: values 1e-5 of the tensor's max-abs, gradients 1e-4 of the tensor's rms, in both
arithmetic modes.
The power-of-two grad_scale check draws dz on a 2^-8 grid: such values split into f16 terms without rounding at either
scale, so the scaled run must be bit-identical (a general dz leaves low terms in f16's subnormal range at scale 1)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import generic_layers_model as gm

pytestmark = pytest.mark.gpu

# (Hin, Win, Cin, k, stride, Cout, src_flat)
CASES = [
    (5, 5, 5, 3, 1, 32, 1),     # Connector's first layer: 25 pixels per image, every tile straddles images
    (5, 5, 32, 3, 1, 32, 0),    # ... its second layer
    (2, 7, 1, 3, 1, 32, 1),     # rcnn: Cin 1, K = 9 padded, the image narrower than the kernel's reach
    (10, 10, 4, 3, 1, 32, 1),   # Cleaner: tiles inside one image and across its end
    (4, 6, 2, 2, 1, 32, 1),     # even kernels: asymmetric 'SAME' padding
    (4, 6, 32, 4, 2, 64, 0),    # ... stride 2, Cout 64
    (7, 7, 32, 3, 3, 32, 0),    # stride 3
    (3, 3, 32, 1, 1, 32, 0),    # 1 x 1
]


def _pad(H, W, k, st):
    Hout, Wout, (th, tw), (lh, lw) = gm.same_geo(H, W, k, st)
    return Hout, Wout, (lw, tw - lw, lh, th - lh)


@functools.lru_cache(maxsize=None)
def _case(case, S):
    """Inputs (float32) and the float64 reference of one case, computed once."""
    H, W, C, k, st, Co, _ = case
    rng = np.random.default_rng(61)
    Hout, Wout, pad = _pad(H, W, k, st)
    x = rng.standard_normal((S, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((k * k * C, Co)) / np.sqrt(k * k * C)).astype(np.float32)
    b = (rng.standard_normal(Co) * 0.5).astype(np.float32)
    dz = rng.standard_normal((S * Hout * Wout, Co)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_()
    wt = torch.from_numpy(w).double().requires_grad_()
    bt = torch.from_numpy(b).double().requires_grad_()
    z = F.conv2d(F.pad(xt, pad), wt.view(k, k, C, Co).permute(3, 2, 0, 1), bt, stride=st).permute(0, 2, 3, 1).reshape(-1, Co)
    (z * torch.from_numpy(dz).double()).sum().backward()
    ref = dict(z=z.detach().numpy(), dx=xt.grad.permute(0, 2, 3, 1).reshape(S * H * W, C).numpy(), dw=wt.grad.numpy(), db=bt.grad.numpy())
    return x, w, b, dz, ref


def _within(got, want, frac, scale, what):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"{what}: max error {err:.3e}, allowed {frac * scale:.3e}")
    assert err <= frac * scale, what


def _value(got, want, what):
    _within(got, want, 1e-5, float(np.abs(want).max()), what)


def _grad(got, want, what):
    _within(got, want, 1e-4, float(np.sqrt(np.mean(want * want))), what)


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(params=["f32", "f16x2"])
def ctx(request):
    from mava_amd._lib import Ctx

    c = Ctx(request.param)
    yield c
    c.close()


@pytest.mark.parametrize("samples", [32, 96])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_direct_kernels(dev, case, samples, ctx):
    from mava_amd import ops
    from mava_amd._lib import check, lib, ptr, stream_ptr

    L, s, S = lib(), stream_ptr(), samples
    H, W, C, k, st, Co, flat = case
    x, w, b, dz, ref = _case(case, S)
    Hout, Wout, _ = _pad(H, W, k, st)
    rows, K = S * Hout * Wout, k * k * C
    src, wd, bd = _d(gm.to_t32(gm.image_matrix(x, flat)), dev), _d(w, dev), _d(b, dev)
    geo = (S, H, W, C, k, st, Co)

    # ---- forward: z, and y for both activations
    for act, fn in ((1, lambda v: np.maximum(v, 0.0)), (2, np.tanh)):
        z, y = torch.full((rows * Co,), np.nan, device=dev), torch.full((rows * Co,), np.nan, device=dev)
        check(L.mava_conv_fwd_f32(ctx.handle, ptr(src), flat, *geo, ptr(wd), ptr(bd), act, ptr(z), ptr(y), s), "conv_fwd")
        _value(gm.from_t32(z.cpu().numpy(), rows, Co), ref["z"], "z")
        _value(gm.from_t32(y.cpu().numpy(), rows, Co), fn(ref["z"]), f"y (act {act})")

    # ---- input gradient (the tiled layout only), and its exact scaling with a power of two
    grid = np.round(dz * 256.0) / 256.0
    if not flat:
        def dsrc_of(g):
            out = torch.full((S * H * W * C,), np.nan, device=dev)
            check(L.mava_conv_bwd_data_f32(ctx.handle, ptr(_d(gm.to_t32(g.astype(np.float32)), dev)), *geo, ptr(wd), ptr(out), s), "conv_bwd_data")
            return gm.from_t32(out.cpu().numpy(), S * H * W, C)

        _grad(dsrc_of(dz), ref["dx"], "dsrc")
        assert np.array_equal(dsrc_of(grid * 1024.0), dsrc_of(grid) * np.float32(1024.0)), "dsrc is not linear in a power-of-two scale"

    # ---- weight and bias gradient: one slab per block, also with more blocks than tiles
    def slabs_of(g, grad_scale, n_slab):
        slab = torch.full((n_slab, K * Co + Co + 3), np.nan, device=dev)
        check(L.mava_conv_bwd_weight_f32(ctx.handle, ptr(src), flat, *geo, ptr(_d(gm.to_t32(g.astype(np.float32)), dev)), grad_scale, ptr(slab),
                                         slab.shape[1], n_slab, s), "conv_bwd_weight")
        return slab

    ntiles = rows // 32
    for n_slab in (1, 3, ntiles + 2):
        slab = slabs_of(dz, 1.0, n_slab)
        dw, db = torch.empty(K * Co, device=dev), torch.empty(Co, device=dev)
        ops.slab_reduce(slab, K * Co, dw)
        ops.slab_reduce_cols(slab, K * Co, Co, db)
        _grad(dw.cpu().numpy().reshape(K, Co), ref["dw"], f"dW ({n_slab} slabs)")
        _grad(db.cpu().numpy(), ref["db"], f"db ({n_slab} slabs)")
        host = slab.cpu().numpy()
        assert np.isnan(host[:, K * Co + Co :]).all(), "wrote past [dW | db]"
        assert (host[ntiles:, : K * Co + Co] == 0.0).all(), "a block without tiles writes exact zeros"
        assert np.array_equal(host[:, : K * Co + Co], slabs_of(dz, 1.0, n_slab).cpu().numpy()[:, : K * Co + Co]), "not reproducible"
    one, scaled = slabs_of(grid, 1.0, 3).cpu().numpy(), slabs_of(grid * 1024.0, 1024.0, 3).cpu().numpy()
    assert np.array_equal(one[:, : K * Co + Co], scaled[:, : K * Co + Co]), "slabs do not scale exactly with grad_scale"


@pytest.mark.parametrize("bad", [dict(k=5), dict(stride=4), dict(Cout=48), dict(C=65), dict(samples=48)], ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_conv_direct_refuses_outside_its_envelope(dev, bad):
    """Return code 1, nothing launched: NaN-filled outputs stay as they are."""
    from mava_amd._lib import lib, ptr, stream_ptr

    L, s = lib(), stream_ptr()
    g = dict(samples=32, H=5, W=5, C=32, k=3, stride=1, Cout=32)
    g.update(bad)
    geo = (g["samples"], g["H"], g["W"], g["C"], g["k"], g["stride"], g["Cout"])
    n = 64 * 25 * 65
    src, w = torch.zeros(n, device=dev), torch.zeros(25 * 65 * 64, device=dev)
    outs = [torch.full((n,), np.nan, device=dev) for _ in range(3)]
    assert L.mava_conv_fwd_f32(None, ptr(src), 0, *geo, ptr(w), None, 1, ptr(outs[0]), ptr(outs[1]), s) == 1
    assert L.mava_conv_bwd_data_f32(None, ptr(src), *geo, ptr(w), ptr(outs[2]), s) == 1
    assert L.mava_conv_bwd_weight_f32(None, ptr(src), 0, *geo, ptr(src), 1.0, ptr(outs[0]), n, 1, s) == 1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)


@pytest.mark.parametrize("act,ln", [("relu", False), ("tanh", True)], ids=["default", "ln-tanh"])
def test_generic_net_direct_against_im2col(dev, ctx, act, ln):
    """The default CNNTorso on (5, 5, 5) at 64 rows: forward and backward of the same net under both settings."""
    from mava_amd.generic_networks import CNNTorso, GenericNet
    from mava_amd.rec_networks import t32_to_rows

    rows, nA = 64, 5
    net = GenericNet(CNNTorso([32, 32], [3, 3], [1, 1], act, ln), 125, [("Dense_0", nA, 0.01)], obs_shape=(5, 5, 5))
    net.ctx = ctx
    flat = net.init_flat(3, dev)
    gen = torch.Generator().manual_seed(4)
    obs = torch.randn((1, rows, 1, 125), generator=gen).to(dev)
    d_out = torch.randn(rows * nA, generator=gen).to(dev)
    got = {}
    for conv in ("im2col", "direct"):
        net.conv = conv
        ws = net.workspace(rows, dev, True)
        assert all((c is None) == (conv == "direct") for c in ws.col + ws.dcol)
        out = net.forward(flat, ws, obs, 1, None, rows, rows, 1)[0]
        grad = torch.zeros(net.num_params, device=dev)
        net.backward(flat, ws, [d_out], grad, accumulate=False, grad_scale=64.0)
        got[conv] = (t32_to_rows(out, nA, rows).cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64))
    _value(got["direct"][0], got["im2col"][0], "head output")
    for ly in net.layers + net.heads:
        segs = [("kernel", ly.w, ly.K * ly.N), ("bias", ly.b, ly.N)] + ([("layer-norm bias", ly.lnb, ly.N)] if ly.ln else [])
        for name, off, n in segs:
            _grad(got["direct"][1][off : off + n], got["im2col"][1][off : off + n], f"{ly.name} {name} gradient")


def test_learner_update_with_direct_conv(dev, monkeypatch):
    """ff_mappo network=cnn on con-5x5x3a (32 envs, rollout 8), one learn() call in exact f32: MAVA_CONV_DIRECT=1 set before
    the learner is built against the same call without it.  The sampled actions are compared without any allowance for
    near-ties (stricter than tests/test_gpu_mat.py's phrasing: the logits of the two paths differ by parts in 10^7)."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo

    monkeypatch.setenv("MAVA_MATMUL", "f32")

    def run(direct):
        monkeypatch.setenv("MAVA_CONV_DIRECT", "1" if direct else "0")
        cfg = compose("default_ff_mappo", ["env=connector", "env/scenario=con-5x5x3a", "network=cnn", "arch.num_envs=32",
                                           "system.rollout_length=8", "system.update_batch_size=1"])
        cfg.system.num_updates_per_eval = 1
        env, _ = envs.make(cfg, add_global_state=True, device=dev)
        learn, _net, state = ff_mappo.learner_setup(env, (42, 43, 44), cfg, device=dev)
        L = learn.learner
        assert L.actor_network.net.conv == L.critic_network.net.conv == ("direct" if direct else "im2col")
        learn(state)
        torch.cuda.synchronize()
        return L.reps[0].action.cpu().numpy().copy(), L.p.cpu().numpy().astype(np.float64)

    (act0, p0), (act1, p1) = run(False), run(True)
    assert np.array_equal(act0, act1), "the rollout sampled other actions"
    err = float(np.abs(p1 - p0).max())
    print(f"parameters after the update: max difference {err:.3e}, allowed 1e-5")
    assert err <= 1e-5
