"""CPU: properties of the float64 ff_mat model (tests/mat_model.py), the config root and the refusals.  No GPU."""
import numpy as np
import pytest
import torch

from tests import mat_model as mm
from mava_amd import _lib
from mava_amd.config import compose
from mava_amd.mat_learner import MATNet, check_supported

B, A, O, NA, D = 3, 4, 7, 5, 32


def _setup(n_head=2, n_block=2, seed=0):
    net = MATNet(O, NA, A, D, n_head, n_block)
    flat = net.init_flat(seed).double()
    g = torch.Generator().manual_seed(seed + 1)
    # the output layers start at 0.01: widen them so that the logits and values are O(1) and every path carries signal
    flat = flat + 0.05 * torch.randn(flat.shape, generator=g, dtype=torch.float64)
    obs = torch.randn((B, A, O), generator=g, dtype=torch.float64)
    action = torch.randint(0, NA, (B, A), generator=g)
    mask = torch.rand((B, A, NA), generator=g) > 0.3
    mask[..., 0] = True
    return net, flat, obs, action, mask, g


def test_layout_covers_the_flat_vector_once():
    net = MATNet(O, NA, A, D, 2, 2)
    spans = sorted((net.off[p], net.off[p] + int(np.prod(s))) for p, s, _ in net.spec)
    assert spans[0][0] == 0 and spans[-1][1] == net.num_params
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    flat = net.init_flat(3)
    tree = net.tree(flat)
    assert set(tree) == {"encoder", "decoder"} and "bias" not in tree["decoder"]["act_dense"]
    assert torch.equal(net.flat_from_tree(net.tree(flat, (1, 1)), torch.zeros_like(flat)), flat)
    assert float(tree["encoder"]["ln"]["scale"].min()) == 1.0 and float(tree["encoder"]["obs_dense"]["bias"].abs().max()) == 0.0
    k = tree["decoder"]["head_out"]["kernel"].double()  # orthogonal(0.01): D x NA with orthonormal columns times 0.01
    assert torch.allclose(k.T @ k, 1e-4 * torch.eye(NA, dtype=torch.float64), atol=1e-10)
    k = tree["encoder"]["block_1"]["mlp_0"]["kernel"].double()
    assert torch.allclose(k.T @ k, 2.0 * torch.eye(D, dtype=torch.float64), atol=1e-6)


def test_causality():
    net, flat, obs, action, mask, _ = _setup()
    p = net.tree(flat)
    _, _, value, logits = mm.forward(p, obs, action, mask, 2)
    for j in range(A):
        a2 = action.clone()
        a2[:, j] = (a2[:, j] + 1) % NA
        _, _, v2, l2 = mm.forward(p, obs, a2, mask, 2)
        assert torch.equal(l2[:, : j + 1], logits[:, : j + 1]), f"agent {j}'s action reached the logits of agents <= {j}"
        assert torch.equal(v2, value)
        if j + 1 < A:
            assert (l2[:, j + 1 :] != logits[:, j + 1 :]).any()
    for j in range(A):  # the encoder is not causal: any agent's observation reaches every agent's value
        o2 = obs.clone()
        o2[:, j, 0] += 0.5  # (one feature: the observation norm removes a shift of the whole row)
        _, _, v2, _ = mm.forward(p, o2, action, mask, 2)
        assert bool((v2 != value).all())


@pytest.mark.parametrize("greedy", [False, True])
def test_teacher_forced_equals_autoregressive(greedy):
    net, flat, obs, _, mask, g = _setup()
    p = net.tree(flat)
    u = torch.rand((B, A, NA), generator=g, dtype=torch.float64).clamp(1e-6, 1 - 1e-6)
    action, lp_act, value, _ = mm.act(p, obs, mask, u, 2, greedy)
    assert bool(mask.gather(-1, action.unsqueeze(-1)).all()), "an illegal action was chosen"
    lp, _, v2, _ = mm.forward(p, obs, action, mask, 2)
    assert float((lp - lp_act).abs().max()) < 1e-12 and float((v2 - value).abs().max()) < 1e-12


def test_gradient_against_central_differences():
    net, flat, obs, action, mask, g = _setup(n_head=2, n_block=1)
    old_lp = -1.5 + 0.2 * torch.randn((B, A), generator=g, dtype=torch.float64)
    adv, old_v, tgt = (torch.randn((B, A), generator=g, dtype=torch.float64) for _ in range(3))

    def f(x):
        return mm.loss(net.tree(x), obs, action, mask, old_lp, adv, 0.1 * old_v, tgt, 2, 0.2, 0.01, 0.5)[0]

    x = flat.clone().requires_grad_(True)
    f(x).backward()
    grad = x.grad
    idx = torch.randperm(net.num_params, generator=g)[:60].tolist()
    idx += [net.off[p] for p, _, _ in net.spec]  # one entry of every leaf
    h = 1e-6
    for i in idx:
        e = torch.zeros_like(flat)
        e[i] = h
        num = float(f(flat + e) - f(flat - e)) / (2 * h)
        assert abs(num - float(grad[i])) <= 1e-6 * max(1.0, float(grad.abs().max())), (i, num, float(grad[i]))
    assert float(grad.abs().max()) > 1e-3


def test_config_root():
    cfg = compose("default_ff_mat")
    assert cfg.logger.system_name == "ff_mat" and cfg.env.env_name == "RobotWarehouse"
    assert (int(cfg.network.n_block), int(cfg.network.n_head), int(cfg.network.n_embd)) == (1, 1, 64)
    assert int(cfg.system.update_batch_size) == 1 and float(cfg.system.actor_lr) == 2.5e-4 and "critic_lr" in cfg.system
    assert int(cfg.system.ppo_epochs) == 4 and int(cfg.system.num_minibatches) == 2 and int(cfg.system.rollout_length) == 128
    assert int(compose("default_ff_mat", ["network.n_head=2"]).network.n_head) == 2
    from mava_amd.systems.ppo import ff_mat

    assert callable(ff_mat.run_experiment) and callable(ff_mat.learner_setup)


GOOD = dict(num_agents=4, n_actions=5, n_embd=64, n_head=1, continuous=False, world=1, update_batch_size=1)


@pytest.mark.parametrize("bad", [dict(continuous=True), dict(num_agents=33), dict(n_embd=48), dict(n_embd=160), dict(n_embd=64, n_head=3),
                                 dict(n_actions=65), dict(world=2), dict(update_batch_size=2)])
def test_refusals(bad):
    check_supported(**GOOD)
    with pytest.raises(_lib.MavaHipError):
        check_supported(**dict(GOOD, **bad))


def test_symbols_are_declared():
    names = [n for n in _lib.declared_symbols() if n.startswith("mava_mat_")]
    assert len(names) == 9
    lib = _lib.lib()
    assert lib.mava_abi_version() == 4 and all(hasattr(lib, n) for n in names)


def test_kernel_argument_refusals_need_no_gpu():
    """MAVA_ARG_CHECK comes before any launch: bad shapes and null pointers return an error code and a message."""
    lib = _lib.lib()
    assert lib.mava_mat_attn_fwd_f32(None, None, None, 32, 64, 1, 33, 1, 0, None, None, 1, None) <= -1000 and b"A <= 32" in lib.mava_last_error()
    assert lib.mava_mat_attn_fwd_f32(None, None, None, 32, 64, 1, 4, 3, 0, None, None, 1, None) <= -1000
    assert lib.mava_mat_attn_fwd_f32(None, None, None, 32, 64, 1, 4, 1, 0, None, None, 1, None) <= -1000 and b"null pointer" in lib.mava_last_error()
    assert lib.mava_mat_attn_fwd_f32(None, None, None, 32, 64, 9, 4, 1, 0, None, None, 1, None) <= -1000  # 36 rows in 32
    assert lib.mava_mat_attn_bwd_f32(None, None, None, None, 33, 64, 1, 4, 1, 0, None, None, None, 1, None) <= -1000
    assert lib.mava_mat_ln_fwd_f32(None, None, None, None, 0, 32, 32, None, None, None, 1, None) <= -1000
    assert lib.mava_mat_ln_fwd_f32(None, None, None, None, 5, 32, 33, None, None, None, 1, None) <= -1000
    assert lib.mava_mat_ln_bwd_f32(None, None, None, None, 5, 32, 3, 1.0, None, None, 9, 1, None) <= -1000 and b"2 N" in lib.mava_last_error()
    assert lib.mava_mat_gelu_f32(None, 8, None, None) <= -1000 and lib.mava_mat_gelu_bwd_f32(None, None, -1, None, None) <= -1000
    assert lib.mava_mat_shift_onehot_f32(None, None, 1, 4, 5, 4, 32, 32, None, None) <= -1000  # known > A - 1
    assert lib.mava_mat_shift_onehot_f32(None, None, 1, 4, 40, 1, 32, 32, None, None) <= -1000  # n_pad too small
    assert lib.mava_mat_sample_f32(1, 4, 4, 5, None, None, 0, 0, 0, 0, None, None, None) <= -1000
    assert lib.mava_mat_sample_f32(1, 4, 0, 65, None, None, 0, 0, 0, 0, None, None, None) <= -1000
    assert lib.mava_mat_loss_f32(8, 4, 5, 32, *([None] * 10), 1, 0.2, 0.01, 0.5, 1.0, None, None, None, 1, None) <= -1000
    assert lib.mava_mat_loss_f32(9, 4, 5, 32, *([None] * 10), 1, 0.2, 0.01, 0.5, 1.0, None, None, None, 1, None) <= -1000
