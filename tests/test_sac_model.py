"""CPU: tests/sac_model.py on its own - the analytic gradients of the reparameterised tanh-normal log-density against
autograd in all three branches, the joint-action helpers, the policy-delay rule and the item buffer's indices."""
import numpy as np
import pytest
import torch

from tests import sac_model as sm

F64 = torch.float64


def _autograd_logp_grads(mean, raw, eps, min_scale):
    mean, scale = mean.clone().requires_grad_(True), sm.scale_of(raw, min_scale).clone().requires_grad_(True)
    a = torch.tanh(mean + scale * eps)
    lp = sm.log_prob_terms(a, mean, scale)
    gm, gs = torch.autograd.grad(lp.sum(), [mean, scale])
    return a.detach(), scale.detach(), gm, gs


@pytest.mark.parametrize("branch,centre", [("inner", 0.0), ("left", -7.0), ("right", 7.0)])
def test_analytic_logp_gradients_match_autograd(branch, centre):
    g = torch.Generator().manual_seed(3)
    n, D = 200, 5
    mean = centre + 0.5 * torch.randn((n, D), generator=g, dtype=F64)
    # (the clipped cases keep the scale small: every sample stays beyond atanh(0.999) = 3.8)
    raw = (-1.0 if branch == "inner" else -2.0) + (0.7 if branch == "inner" else 0.3) * torch.randn((n, D), generator=g, dtype=F64)
    eps = torch.randn((n, D), generator=g, dtype=F64)
    a, scale, gm, gs = _autograd_logp_grads(mean, raw, eps, 1e-3)
    if branch == "inner":
        assert (a.abs() < sm.THRESH).all()
    else:
        assert ((a <= -sm.THRESH) if branch == "left" else (a >= sm.THRESH)).all()
    am, as_ = sm.analytic_logp_grads(a, eps, mean, scale)
    torch.testing.assert_close(am, gm, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(as_, gs, rtol=1e-9, atol=1e-11)
    if branch == "inner":  # the issue's closed forms
        torch.testing.assert_close(gm, 2.0 * a, rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(gs, -1.0 / scale + 2.0 * a * eps, rtol=1e-9, atol=1e-11)


def test_mixed_branches_in_one_batch():
    mean = torch.tensor([[0.1, -7.0, 7.0, 0.3]], dtype=F64)
    raw = torch.tensor([[-0.5, -2.0, -2.0, 0.2]], dtype=F64)
    eps = torch.tensor([[0.4, -0.3, 0.2, -1.1]], dtype=F64)
    a, scale, gm, gs = _autograd_logp_grads(mean, raw, eps, 1e-3)
    assert (a.abs() >= sm.THRESH).tolist() == [[False, True, True, False]]
    am, as_ = sm.analytic_logp_grads(a, eps, mean, scale)
    torch.testing.assert_close(am, gm, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(as_, gs, rtol=1e-9, atol=1e-11)


def test_log_prob_restates_the_numpy_oracle():
    from oracle import tanh_normal as tn

    g = torch.Generator().manual_seed(1)
    mean = 3.0 * torch.randn((64, 3), generator=g, dtype=F64)
    scale = 0.2 + torch.rand((64, 3), generator=g, dtype=F64)
    a = torch.tanh(mean + scale * torch.randn((64, 3), generator=g, dtype=F64)).float().double()  # float32 actions
    want, _, _ = tn.log_prob_terms(a.numpy(), mean.numpy(), scale.numpy())
    np.testing.assert_allclose(sm.log_prob_terms(a, mean, scale).numpy(), want, rtol=1e-9, atol=1e-9)


def test_joint_actions_follow_the_docstring_example():
    rb = torch.tensor([[[0.0], [1.0], [2.0]]], dtype=F64)
    new = torch.tensor([[[3.0], [4.0], [5.0]]], dtype=F64)
    assert sm.get_joint_action(rb).tolist() == [[[0, 1, 2], [0, 1, 2], [0, 1, 2]]]
    assert sm.get_updated_joint_actions(rb, new).tolist() == [[[3, 1, 2], [0, 4, 2], [0, 1, 5]]]
    # action_dim 2: slots are (agent, component) pairs
    rb = torch.arange(12, dtype=F64).view(2, 3, 2)
    new = -torch.arange(12, dtype=F64).view(2, 3, 2) - 100
    j = sm.get_updated_joint_actions(rb, new)
    assert j.shape == (2, 3, 6) and j[1, 2].tolist() == [6, 7, 8, 9, -110, -111] and j[0, 0].tolist() == [-100, -101, 2, 3, 4, 5]
    assert sm.get_joint_action(rb)[1, 0].tolist() == [6, 7, 8, 9, 10, 11]


def test_policy_delay_reads_the_env_step_counter():
    # the reference's defaults: explore_steps 5000, rollout_length 2, delay 4
    t0 = sm.env_steps_after(5000, 16, 2, 0)
    assert t0 == 4992 and sm.policy_fires(t0, 4)  # 312 explore steps of 16 envs
    # t advances by num_envs * rollout_length per update step, never inside the epochs: with 16 * 2 = 32 a multiple of 4
    # the actor is trained in EVERY epoch of every update step ...
    assert all(sm.policy_fires(sm.env_steps_after(5000, 16, 2, u), 4) for u in range(10))
    # ... and with num_envs 3, rollout_length 1 only where 4998 + 3u is a multiple of 4
    fires = [sm.policy_fires(sm.env_steps_after(5000, 3, 1, u), 4) for u in range(8)]
    assert sm.env_steps_after(5000, 3, 1, 0) == 4998 and fires == [False, False, True, False, False, False, True, False]
    assert sm.policy_fires(7, 1)


def test_ring_and_sampled_items_across_a_wrap():
    cap, E = 64, 24
    head, stored = 0, {}
    for add in range(4):
        slots = sm.ring_slots(head, E, cap)
        for e, s in enumerate(slots):
            stored[int(s)] = add * E + e  # the serial number of the item in the slot
        head = (head + E) % cap
        n_added = (add + 1) * E
        filled = min(n_added, cap)
        idx = sm.sampled_items(seed=9, counter=add, B=4096, n_added=n_added, capacity=cap)
        serial = np.array([stored[int(i)] for i in idx])
        # every live item and nothing else: the newest `filled` serial numbers, each drawn about equally often
        assert serial.min() == n_added - filled and serial.max() == n_added - 1 and len(np.unique(serial)) == filled
        assert np.bincount(serial - serial.min()).min() > 4096 / filled / 3
    assert sm.ring_slots(48, 24, 64).tolist() == list(range(48, 64)) + list(range(8))  # the third add wraps
    # k counts from the oldest item: word * filled / 2^32, floor
    a = sm.sampled_items(5, 2, 8, n_added=100, capacity=64)
    b = sm.sampled_items(5, 2, 8, n_added=100 + 64, capacity=64)
    assert np.array_equal(a, b) and not np.array_equal(a, sm.sampled_items(5, 3, 8, 100, 64))


def test_update_pieces_on_a_tiny_system():
    """Shapes and signs of the model's three gradients (isac and masac), and the target with done set."""
    torch.manual_seed(0)
    B, A, O, D, S = 6, 3, 5, 2, 4
    for joint in (False, True):
        actor = sm.Net(O, [8, 8], [D, D])
        q = sm.Net((S + A * D) if joint else (O + D), [8, 8], [1])
        sac = sm.Sac(actor, q, A, D, joint, 0.99, 1e-3, -5.0 * D)
        p = {"actor": 0.3 * torch.randn(actor.num_params, dtype=F64), "log_alpha": torch.tensor([0.0, -0.5, 0.3], dtype=F64)}
        for k in ("q1", "q2", "q1_t", "q2_t"):
            p[k] = 0.3 * torch.randn(q.num_params, dtype=F64)
        batch = {"obs": torch.randn(B, A, O, dtype=F64), "next_obs": torch.randn(B, A, O, dtype=F64),
                 "action": torch.rand(B, A, D, dtype=F64) * 2 - 1, "reward": torch.randn(B, A, dtype=F64),
                 "done": (torch.rand(B, A) < 0.3).double(), "gs": torch.randn(B, S, dtype=F64), "next_gs": torch.randn(B, S, dtype=F64)}
        eps = torch.randn(B, A, D, dtype=F64)
        target = sac.target(p, batch, eps)
        assert torch.equal(target[batch["done"] == 1], batch["reward"][batch["done"] == 1])
        g1, g2, info = sac.q_grads(p, batch, eps)
        assert g1.shape == p["q1"].shape and g2.abs().sum() > 0 and info["q1_loss"] > 0
        ga, _ = sac.actor_grad(p, batch, eps)
        gl, loss = sac.alpha_grad(p, batch, eps)
        assert ga.shape == p["actor"].shape and ga.abs().sum() > 0 and gl.shape == (A,)
        # d/d log_alpha of -exp(log_alpha) x is itself: the gradients sum to the loss
        assert abs(gl.sum().item() - loss) < 1e-12
