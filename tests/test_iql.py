"""CPU: rec_iql configuration, refusals, argument errors of the new entry points (no GPU needed) and invariants of the
model in tests/iql_model.py."""

import numpy as np
import pytest

from mava_amd import _lib
from mava_amd.config import compose
from tests import iql_model as qm


def test_compose_carries_reference_defaults():
    c = compose("default_rec_iql")
    s = c.system
    want = {"total_timesteps": None, "num_updates": 156250, "seed": 1, "add_agent_id": True, "min_buffer_size": 32,
            "update_batch_size": 1, "rollout_length": 2, "epochs": 2, "buffer_size": 5000, "sample_batch_size": 32,
            "sample_sequence_length": 20, "q_lr": 3e-4, "max_grad_norm": 10, "hard_update": False, "update_period": 200,
            "tau": 0.01, "gamma": 0.99, "eps_min": 0.05, "eps_decay": 1e5}
    assert dict(s) == want
    assert c.arch.num_envs == 16 and c.logger.system_name == "rec_iql" and c.env.env_name == "LevelBasedForaging"
    assert c.network.hidden_state_dim == 128
    for part in ("pre_torso", "post_torso"):
        assert c.network.q_network[part]["layer_sizes"] == [128] and c.network.q_network[part]["activation"] == "relu"
    assert compose("default_rec_ippo", ["system=rec_iql"]).system.q_lr == 3e-4
    assert compose("default_rec_ippo", ["system=rec_ippo"]).system.get("q_lr") is None


@pytest.mark.parametrize("override,exc,msg", [
    (["env=rware"], ValueError, "pre-reset observation"),
    (["env=smax"], ValueError, "pre-reset observation"),
    (["system.update_batch_size=2"], NotImplementedError, "update_batch_size"),
    (["network.hidden_state_dim=64"], ValueError, "hidden_state_dim"),
    (["network.q_network.pre_torso.layer_sizes=[64]"], NotImplementedError, "torsos"),
    (["network.q_network.post_torso.activation=tanh"], NotImplementedError, "torsos"),
])
def test_run_experiment_refuses_at_setup(override, exc, msg):
    from mava_amd.systems.q_learning import rec_iql

    with pytest.raises(exc, match=msg):
        rec_iql.run_experiment(compose("default_rec_iql", override))


def test_learner_refuses_env_without_terminal_observation():
    from mava_amd.envs.synthetic_rware import SyntheticRware
    from mava_amd.iql_learner import IQLLearner

    assert not getattr(SyntheticRware, "emits_real_next_obs", False)

    class Env:  # the synthetic stand-in's surface, no pre-reset observation
        num_envs, num_agents, action_dim, obs_dim = 16, 3, 6, 21

    with pytest.raises(ValueError, match="pre-reset observation"):
        IQLLearner(Env(), compose("default_rec_iql"), device="cpu")


def test_new_entry_points_report_argument_errors():
    L = _lib.lib()
    err = lambda: L.mava_last_error()
    n = [None] * 24
    # mava_lbf_step: the shape checks, then the three real-next pointers - all of them or none
    assert L.mava_lbf_step(4, 0, 1, 5, 1, 2, 0, 0, 10, 1, 0, None, 0, 0, *n, None) <= -1000
    assert b"mava_lbf_step: bad shape" in err()
    step = lambda action, *real: L.mava_lbf_step(4, 2, 1, 5, 1, 2, 0, 0, 10, 1, 0, None, 0, 0, *[16] * 20, action, *real, None)
    assert step(None, None, None, None) <= -1000 and b"action array" in err()  # none of the three: the later checks are reached
    for part in ((16, None, None), (None, 16, None), (None, None, 16), (16, 16, None), (16, None, 16), (None, 16, 16)):
        assert step(16, *part) <= -1000 and b"real_view" in err()
    assert step(16, 16, 16, 16) <= -1000 and b"alias" in err()
    assert L.mava_rec_q_step_f32(None, 21, 6, None, None, None, None, None, 33, 0.1, 1, 0, 0, None, None, None) <= -1000
    assert b"multiple of 32" in err()
    assert L.mava_rec_q_step_f32(None, 21, 17, None, None, None, None, None, 32, 0.1, 1, 0, 0, None, None, None) <= -1000
    assert b"n_actions" in err()
    assert L.mava_rec_q_step_f32(None, 21, 6, None, None, None, None, None, 32, 0.1, 1, 0, 0, None, None, None) <= -1000
    assert b"null pointer" in err()
    assert L.mava_replay_add_f32(16, 3, 21, 6, 8, 8, *[None] * 16, None) <= -1000 and b"slot 8" in err()
    assert L.mava_replay_add_f32(16, 3, 21, 6, 8, 0, *[None] * 16, None) <= -1000 and b"null input" in err()
    assert L.mava_replay_sample_f32(16, 3, 21, 6, 8, 8, 8, 5, 20, 1, 0, *[None] * 17, None) <= -1000
    assert b"multiple of 32" in err()
    assert L.mava_replay_sample_f32(16, 3, 21, 6, 8, 4, 8, 5, 32, 1, 0, *[None] * 17, None) <= -1000
    assert b"hold no window" in err()
    assert L.mava_q_td_loss_f32(4, 32, 6, 33, *[None] * 7, 0.99, 1.0, None, None, 4, None) <= -1000 and b"n_real" in err()
    assert L.mava_q_td_loss_f32(4, 32, 6, 24, *[None] * 7, 0.99, 1.0, None, None, 4, None) <= -1000 and b"null pointer" in err()
    assert L.mava_target_update_f32(8, None, None, 1.5, 0, None) <= -1000 and b"tau" in err()
    assert L.mava_target_update_f32(8, None, None, 0.01, 0, None) <= -1000 and b"null or aliased" in err()
    assert L.mava_target_update_f32(0, None, None, 0.01, 0, None) == 0


def test_model_windows_never_cross_the_head():
    rng = np.random.default_rng(3)
    for _ in range(200):
        cap = int(rng.integers(5, 40))
        S = int(rng.integers(1, cap + 1))
        n_added = int(rng.integers(S, 3 * cap))
        E, B = int(rng.integers(1, 9)), 64
        env, start = qm.windows(int(rng.integers(1 << 40)), int(rng.integers(1000)), B, E, cap, n_added, S)
        assert ((env >= 0) & (env < E)).all()
        filled = min(n_added, cap)
        oldest = n_added - filled
        # the window's time steps, in add order: all stored, none at or past the head
        tau0 = oldest + ((start - oldest) % cap)
        assert (tau0 >= oldest).all() and (tau0 + S <= n_added).all()


def test_model_sample_pads_rows():
    E, A, O, nA, cap = 3, 3, 5, 6, 6
    rb = qm.Replay(E, A, O, nA, cap)
    rng = np.random.default_rng(0)
    for _ in range(9):  # wraps the buffer
        rb.add(rng.standard_normal((E, A, O)), rng.integers(0, 2, (E, A, nA)), rng.integers(0, nA, (E, A)),
               rng.standard_normal((E, A)), rng.integers(0, 2, E), rng.integers(0, 2, (E, A)), rng.standard_normal((E, A, O)),
               rng.integers(0, 2, (E, A, nA)))
    B, S, Rp = 5, 4, 32
    smp, pairs = rb.sample(7, 2, B, S, Rp)
    assert smp["obs"].shape == (S, Rp, O) and pairs.shape == (B, 2)
    pad = slice(B * A, Rp)
    assert (smp["tot"][:, pad] == 1).all()
    for k in ("obs", "mask", "action", "reward", "terminal", "next_obs", "next_mask"):
        assert not smp[k][:, pad].any(), k
    e, s0 = pairs[0]
    assert np.array_equal(smp["obs"][:, 1], rb.f["obs"][e, (s0 + np.arange(S)) % cap, 1])


def test_model_eps_greedy_extremes():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((64, 6))
    mask = rng.integers(0, 2, (64, 6)).astype(bool)
    mask[:, 0] = True
    a0, greedy = qm.eps_greedy(q, mask, 0.0, 5, 3)
    assert np.array_equal(a0, greedy) and np.array_equal(greedy, np.where(mask, q, qm.F32_MIN).argmax(-1))
    a1, _ = qm.eps_greedy(q, mask, 1.0, 5, 3)
    assert mask[np.arange(64), a1].all()
