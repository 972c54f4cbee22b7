"""GPU: ff_mat's fused training pass (mava_transformer_train_fwd_f32 / _bwd_f32, csrc/mat_train.hip) against the float64 model
of tests/mat_model.py and its autograd, its determinism, and the learner under network.training=fused.

Bounds: logits and values 1e-5 (the bound mat_act.hip is held to; a plain float32 evaluation of the model lies at most 3.8e-6
from float64 on these inputs); the summed gradient per leaf 1e-4 of the leaf's own rms (the project's gradient bound; float32
autograd lies at most 2.0e-5 from float64 on the worst leaf).  The attention key biases have a true gradient of zero (the
softmax does not see a shift of all keys' scores): they are held to 1e-4 of the whole gradient vector's rms.
Every case prints its measured maxima (pytest -s).
"""
import functools
import math

import numpy as np
import pytest
import torch

import tests.test_gpu_mat as tgm
from tests import mat_model as mm
from tests.conftest import assert_close
from tests.test_gpu_mat_fused_act import _Calls

pytestmark = pytest.mark.gpu

# (Bm, A, O, nA, D, H, n_block)
SHAPES = [(1, 1, 3, 1, 32, 1, 1),        # one agent, one action, one key
          (11, 3, 7, 5, 32, 1, 1),       # A does not divide 32; a partial last group
          (43, 3, 7, 5, 64, 2, 2),       # 129 rows, two heads, two blocks
          (5, 4, 70, 5, 64, 1, 1),       # the default network
          (9, 5, 33, 33, 96, 4, 1),      # three column tiles, head width 24
          (3, 20, 9, 64, 128, 4, 2),     # A over half a tile, 64 actions
          (2, 32, 5, 3, 128, 1, 1),      # a sample is a whole tile
          (3, 16, 1024, 7, 128, 4, 1)]   # the widest observation
MANY_GROUPS = (300, 4, 70, 5, 64, 1, 1)  # 38 groups through one workgroup's loop and slab row
CASES = [(s, None) for s in SHAPES] + [(MANY_GROUPS, 1), (MANY_GROUPS, 3)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs of a shape and the float64 model's logits, values and gradient of sum(dl * logits) + sum(dv * value), once."""
    from mava_amd.mat_learner import MATNet

    Bm, A, O, nA, D, H, nb = shape
    net, TE = MATNet(O, nA, A, D, H, nb), Bm + 37
    g = torch.Generator().manual_seed(hash(shape) & 0xFFFF)
    flat = net.init_flat(5) + 0.05 * torch.randn(net.num_params, generator=g)
    obs, action = torch.randn((TE, A, O), generator=g), torch.randint(0, nA, (TE, A), generator=g, dtype=torch.int32)
    idx = torch.randperm(TE, generator=g)[:Bm].to(torch.int32)
    dl, dv = torch.randn((Bm * A, nA), generator=g), torch.randn(Bm * A, generator=g)
    f = flat.double().requires_grad_(True)
    _, _, value, logits = mm.forward(net.tree(f), obs[idx.long()].double(), action[idx.long()].long(), None, H)
    ((dl.double() * logits.reshape(Bm * A, nA)).sum() + (dv.double() * value.reshape(-1)).sum()).backward()
    return {"net": net, "flat": flat, "obs": obs, "action": action, "idx": idx, "dl": dl, "dv": dv,
            "logits": logits.detach().reshape(Bm * A, nA), "value": value.detach().reshape(-1), "grad": f.grad}


def run(dev, shape, n_blocks=None, grad_scale=1.0, backward=True):
    """The two launches.  The outputs carry a guard tile, the workspace is NaN-filled and the slab garbage-filled first: the
    kernel reads nothing it has not written.  Returns (logits, value, summed gradient or None) on the host."""
    from mava_amd import ops
    from mava_amd._lib import check, lib, ptr, stream_ptr
    from mava_amd.rec_networks import rows_to_t32, t32_to_rows

    Bm, A, O, nA, D, H, nb = shape
    c, L, n, rows = case(shape), lib(), Bm * A, tgm.c32(Bm * A)
    if n_blocks is None:
        n_blocks = max(1, min(256, -(-Bm // max(1, 32 // A))))
    flat, obs, action, idx = (c[k].to(dev).contiguous() for k in ("flat", "obs", "action", "idx"))
    logits, value = torch.full(((rows + 32) * nA,), 9.0, device=dev), torch.full((rows + 32,), 9.0, device=dev)
    common = (ptr(flat), ptr(obs), Bm + 37, ptr(idx), ptr(action), Bm, A, O, nA, D, H, nb)
    check(L.mava_transformer_train_fwd_f32(*common, ptr(logits), ptr(value), n_blocks, stream_ptr()), "train_fwd")
    torch.cuda.synchronize()
    assert bool((logits[rows * nA:] == 9.0).all()) and bool((value[rows:] == 9.0).all()), "the guard tile changed"
    lg, vl = t32_to_rows(logits, nA, rows).cpu(), value[:rows].cpu()
    assert float(lg[n:].abs().max() if rows > n else 0.0) == 0.0 and float(vl[n:].abs().max() if rows > n else 0.0) == 0.0, "padding rows"
    grad = None
    if backward:
        pad = lambda t, N: torch.cat([t.view(n, N) * grad_scale, torch.zeros((rows - n, N))]).to(dev)
        dl, dv = rows_to_t32(pad(c["dl"], nA)), pad(c["dv"], 1).view(-1).contiguous()
        P = c["net"].num_params
        ws = torch.full((L.mava_transformer_train_workspace_bytes(Bm, A, O, D, nb, n_blocks) // 4,), float("nan"), device=dev)
        slab = torch.full((n_blocks, P + 3), -3e30, device=dev)
        check(L.mava_transformer_train_bwd_f32(*common, ptr(dl), ptr(dv), grad_scale, ptr(slab), slab.shape[1], ptr(ws), ws.numel() * 4,
                                               n_blocks, stream_ptr()), "train_bwd")
        assert bool((slab[:, P:] == -3e30).all()), "the slab was written past the parameters"
        gsum = torch.zeros(P, device=dev)
        ops.slab_reduce(slab, P, gsum)
        grad = gsum.cpu()
    return lg[:n], vl[:n], grad


@pytest.mark.parametrize("shape,n_blocks", CASES)
def test_forward_matches_float64_model(dev, shape, n_blocks):
    c = case(shape)
    lg, vl, _ = run(dev, shape, n_blocks, backward=False)
    print(f"{shape} n_blocks={n_blocks}: max logit error {float((lg - c['logits']).abs().max()):.3e}, "
          f"max value error {float((vl - c['value']).abs().max()):.3e}")
    assert_close(lg.numpy(), c["logits"].numpy(), 1e-5, f"{shape}: logits")
    assert_close(vl.numpy(), c["value"].numpy(), 1e-5, f"{shape}: value")


@pytest.mark.parametrize("grad_scale", [1.0, 1024.0])
@pytest.mark.parametrize("shape,n_blocks", CASES)
def test_backward_matches_float64_autograd(dev, shape, n_blocks, grad_scale):
    c = case(shape)
    net, want = c["net"], c["grad"].numpy()
    got = run(dev, shape, n_blocks, grad_scale)[2].double().numpy()
    rms_all, worst = float(np.sqrt(np.mean(want * want))), ("", 0.0)
    for path, shp, _ in net.spec:
        sl = slice(net.off[path], net.off[path] + math.prod(shp))
        g, w = got[sl], want[sl]
        rel = float(np.abs(g - w).max()) / max(float(np.sqrt(np.mean(w * w))), 1e-300)
        if path[-2:] == ("key", "bias"):
            assert float(np.abs(w).max()) <= 1e-12 * rms_all, "the model's key-bias gradient is zero"
            assert float(np.abs(g).max()) <= 1e-4 * rms_all, f"{shape} {'/'.join(path)}: {float(np.abs(g).max()):.3e} of rms {rms_all:.3e}"
            continue
        worst = max(worst, ("/".join(path), rel), key=lambda t: t[1])
        assert_close(g, w, 1e-4, f"{shape} scale {grad_scale}: {'/'.join(path)}")
    print(f"{shape} n_blocks={n_blocks} grad_scale={grad_scale}: worst leaf {worst[0]} at {worst[1]:.3e} of its rms")


@pytest.mark.parametrize("shape", [SHAPES[2], MANY_GROUPS])
def test_deterministic_and_grid_independent(dev, shape):
    ref = run(dev, shape, 1)
    again = run(dev, shape, 1)
    assert all(torch.equal(a, b) for a, b in zip(ref, again)), "two runs at n_blocks = 1 differ"
    for nb in (3, 64):
        lg, vl, grad = run(dev, shape, nb)
        assert torch.equal(lg, ref[0]) and torch.equal(vl, ref[1]), f"logits or values differ between 1 and {nb} blocks"
        assert float((grad - ref[2]).abs().max()) <= 1e-6 * float(ref[2].abs().max()), f"summed gradient at {nb} blocks"
        assert torch.equal(grad, run(dev, shape, nb)[2]), f"two runs at n_blocks = {nb} differ"


def test_shapes_without_an_instance_and_bad_arguments_launch_nothing(dev):
    from mava_amd._lib import lib, ptr, stream_ptr

    L, x = lib(), torch.full((4096,), 9.0, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    fwd = lambda Bm=2, A=3, O=7, nA=5, D=32, H=1, nb=1, blocks=1: L.mava_transformer_train_fwd_f32(
        ptr(x), ptr(x), 8, ptr(i), ptr(i), Bm, A, O, nA, D, H, nb, ptr(x), ptr(x), blocks, stream_ptr())
    assert fwd(nb=5) == 1 and fwd(D=160, H=5) == 1 and L.mava_transformer_train_workspace_bytes(2, 3, 7, 32, 5, 1) == 0
    for bad in (dict(A=33), dict(nA=65), dict(O=1025), dict(H=3), dict(blocks=0), dict(Bm=0)):
        assert fwd(**bad) <= -1000, bad
    assert L.mava_transformer_train_bwd_f32(ptr(x), ptr(x), 8, ptr(i), ptr(i), 2, 3, 7, 5, 32, 1, 1, ptr(x), ptr(x), 1.0, ptr(x), 4096,
                                            ptr(x), 16, 1, stream_ptr()) <= -1000  # the workspace is too small
    torch.cuda.synchronize()
    assert float(x.min()) == 9.0 and float(x.max()) == 9.0


# ---- learner --------------------------------------------------------------------------------------------------------------
LEARNER = ["env=lbf", "env/scenario=2s-10x10-3p-3f", "arch.num_envs=4", "system.rollout_length=8", "network.acting=fused",
           "network.training=fused", "network.n_head=2", "system.num_minibatches=2", "system.ppo_epochs=2", "system.matmul_mode=f32",
           "system.actor_lr=1e-3"]


@pytest.mark.parametrize("n_block,fused", [(2, True), (5, False)])  # five blocks: no instance, every minibatch runs on the tape
def test_learn_matches_model(dev, n_block, fused):
    """tests/test_gpu_mat.py::test_learn_matches_model's convention and f32 bounds, two updates."""
    cfg, learn, L, state = tgm._make(dev, LEARNER + [f"network.n_block={n_block}"])
    s, rep, T, E, A, TE = cfg.system, L.rep, L.T, L.E, L.A, L.T * L.E
    mcfg = {"n_head": 2, "clip_eps": float(s.clip_eps), "ent_coef": float(s.ent_coef), "vf_coef": float(s.vf_coef),
            "lr": float(s.actor_lr), "max_grad_norm": float(s.max_grad_norm)}
    assert L.training == "fused" and L._train is None  # the tape is built by the first minibatch that needs it
    count, t64 = 0, lambda x: x.double().cpu()
    L.debug = {"grads": [], "perms": [], "state": []}
    for upd in range(2):
        for rec in L.debug.values():
            if isinstance(rec, list):
                rec.clear()
        with _Calls() as calls:
            state = learn(state).learner_state
        assert calls.by.get("mava_transformer_train_bwd_f32", 0) == (L.K * L.M if fused else 0), calls.by
        assert ("mava_mat_attn_bwd_f32" in calls.by) != fused and (L._train is None) == fused
        view, mask = rep.agents_view[:T].clone(), rep.action_mask[:T].clone()
        view[0], mask[0] = L.debug["slot0"]
        batch = {"obs": t64(view).view(TE, A, -1), "action": rep.action.long().cpu().view(TE, A),
                 "mask": mask.bool().cpu().view(TE, A, -1), "log_prob": t64(rep.log_prob).view(TE, A),
                 "adv": t64(rep.adv).view(TE, A), "value": t64(rep.value).view(TE, A), "target": t64(rep.tgt).view(TE, A)}
        for i in range(L.K * L.M):
            idx = L.debug["perms"][i // L.M].long().cpu()[(i % L.M) * L.Bm : (i % L.M + 1) * L.Bm]
            flat, m, v = (x.double().cpu().numpy() for x in L.debug["state"][i])
            flat, m, v, count, grad, met = mm.minibatch_step(L.net, flat, m, v, count, batch, idx, mcfg)
            what = f"update {upd} minibatch {i}"
            assert_close(L.debug["grads"][i][: L.P].double().cpu().numpy(), grad, 1e-4, f"{what}: gradient")
            assert_close(L.train_metrics[0, i // L.M, i % L.M].double().cpu().numpy(), met, 1e-5, f"{what}: metrics")
            after = L.debug["state"][i + 1][0] if i + 1 < len(L.debug["state"]) else L.p
            assert_close(after.double().cpu().numpy(), flat, 1e-5, f"{what}: parameters")
        assert int(L.count[0]) == count
    if fused:  # one minibatch is a handful of library calls (the tape takes about 175)
        L.debug = None
        with _Calls() as calls:
            L._minibatch(0, 0, 0, torch.randperm(TE, device=dev).to(torch.int32))
            torch.cuda.synchronize()
        print(f"library calls of one fused minibatch: {calls.by}")
        assert sum(calls.by.values()) <= 10 and L._train is None, calls.by


@pytest.mark.parametrize("over,match", [(["network.training=bogus"], "network.training"),
                                        (["env=spread", "network=continuous_transformer", "network.training=fused"], "continuous")])
def test_refusals_come_before_any_allocation(dev, over, match):
    from mava_amd._lib import MavaHipError

    base = [] if over[0].startswith("env=") else ["env=lbf"]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MavaHipError, match=match):
        tgm._make(dev, base + ["arch.num_envs=4", "system.rollout_length=8"] + over)
    assert torch.cuda.memory_allocated() <= before + (1 << 20)  # (the environment's own state at most)
