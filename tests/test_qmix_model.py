"""CPU: rec_qmix / rec_vdn configuration and refusals, the argument errors of the two new entry points, and invariants of
the float64 model in tests/qmix_model.py (monotonicity, its gradient against finite differences, vdn = the plain sum)."""
import numpy as np
import pytest
import torch

from mava_amd import _lib
from mava_amd.config import compose
from oracle import rec_oracle as ro
from tests import qmix_model as xm


def _random_mixer(rng, Ds, A, Em, Hh, scale=1.0):
    n = xm.mixer_param_count(Ds, A, Em, Hh)
    return torch.from_numpy(rng.standard_normal(n) * scale)


def test_mixer_is_monotonic_in_every_agent_q():
    """dQ_tot / dqa_j >= 0 everywhere, with hypernet outputs of both signs (the abs is what makes it so)."""
    rng = np.random.default_rng(0)
    Ds, A, Em, Hh, R = 10, 3, 8, 16, 200
    p = xm.unpack(_random_mixer(rng, Ds, A, Em, Hh, 0.7), Ds, A, Em, Hh)
    state = torch.from_numpy(rng.standard_normal((R, Ds)))
    qa = torch.from_numpy(rng.standard_normal((R, A)) * 3.0).requires_grad_(True)
    w1, b1, w2, b2 = xm.hyper(p, state)
    assert (w1 < 0).any() and (w1 > 0).any() and (w2 < 0).any() and (w2 > 0).any()
    tot, pre = xm.mix_raw(qa, w1, b1, w2, b2, with_pre=True)
    assert (pre < 0).any() and (pre > 0).any()
    tot.sum().backward()
    assert (qa.grad >= 0).all()
    assert (qa.grad > 0).any()


def _tiny_case(mixer):
    rng = np.random.default_rng(3)
    A, Em, Hh, L, B, O, nA = 2, 4, 8, 2, 3, 5, 4
    S, Rp, n_real = L + 1, 32, B * A
    Pq = ro.rec_param_count(O, nA)
    Pm = xm.mixer_param_count(A * O, A, Em, Hh) if mixer == "qmix" else 0
    online = np.concatenate([ro.init_rec(rng, O, nA, 1.0), rng.standard_normal(Pm) * 0.3])
    target = online + rng.standard_normal(online.size) * 0.05
    smp = {"obs": rng.standard_normal((S, Rp, O)), "next_obs": rng.standard_normal((S, Rp, O)),
           "tot": (rng.random((S, Rp)) < 0.2).astype(np.uint8), "terminal": (rng.random((S, Rp)) < 0.3).astype(np.uint8),
           "next_mask": np.ones((S, Rp, nA), np.uint8), "reward": rng.standard_normal((S, Rp)),
           "action": rng.integers(0, nA, (S, Rp)).astype(np.int32)}
    smp["next_mask"][:, :, 1] = rng.random((S, Rp)) < 0.5
    for k in smp:
        smp[k][:, n_real:] = 0
    return online, target, O, nA, smp, L, B, A, Em, Hh, Pq


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
def test_model_gradient_matches_finite_differences(mixer):
    online, target, O, nA, smp, L, B, A, Em, Hh, Pq = _tiny_case(mixer)
    f = lambda p: xm.qmix_loss_grad(p, target, O, nA, smp, L, B, A, 0.9, mixer, Em, Hh)
    loss, mq, mt, grad, _ = f(online)
    assert np.isfinite(loss) and grad.shape == online.shape and np.abs(grad).max() > 0
    rng = np.random.default_rng(4)
    # the largest entries of the Q network's and of the mixer's gradient, and random ones of both
    idx = list(np.argsort(-np.abs(grad[:Pq]))[:6]) + list(rng.integers(0, Pq, 6))
    if mixer == "qmix":
        assert np.abs(grad[Pq:]).max() > 0
        idx += list(Pq + np.argsort(-np.abs(grad[Pq:]))[:8]) + list(rng.integers(Pq, online.size, 8))
    scale = np.sqrt(np.mean(grad[idx] ** 2))
    for i in idx:
        h = 1e-5
        up, dn = online.copy(), online.copy()
        up[i] += h
        dn[i] -= h
        fd = (f(up)[0] - f(dn)[0]) / (2 * h)
        assert abs(fd - grad[i]) <= 1e-6 * (abs(grad[i]) + scale), (i, fd, grad[i])


def test_vdn_is_the_plain_sum():
    rng = np.random.default_rng(1)
    qa = torch.from_numpy(rng.standard_normal((4, 5, 3)))
    assert torch.equal(xm.mix(None, qa, torch.zeros(4, 5, 7)), qa.sum(-1))
    # and the vdn loss is rec_iql's arithmetic on the summed Q against the mean reward
    online, target, O, nA, smp, L, B, A, Em, Hh, Pq = _tiny_case("vdn")
    assert online.size == Pq
    loss, mq, mt, grad, _ = xm.qmix_loss_grad(online, target, O, nA, smp, L, B, A, 0.9, "vdn")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = B * A
    h0 = torch.zeros((n, 128), dtype=torch.float64)
    q, _ = ro.t_rec_forward(t(online), O, nA, t(smp["obs"][:L, :n]), t(smp["tot"][:L, :n]).bool(), h0)
    qa = q.gather(-1, t(smp["action"][:L, :n]).long().unsqueeze(-1))[..., 0].reshape(L, B, A).sum(-1)
    assert float(qa.mean()) == pytest.approx(mq, rel=1e-12)


def test_compose_resolves_both_roots():
    base = dict(compose("default_rec_iql").system)
    for root, mixer in (("default_rec_qmix", "qmix"), ("default_rec_vdn", "vdn")):
        c = compose(root)
        s = dict(c.system)
        assert s.pop("mixer") == mixer and s.pop("mixer_embed_dim") == 32 and s.pop("hypernet_hidden_dim") == 64
        assert s == base  # rec_iql's keys and defaults
        assert c.logger.system_name == f"rec_{mixer}" and c.env.env_name == "LevelBasedForaging"
        assert c.network.hidden_state_dim == 128
    assert compose("default_rec_iql", ["system=rec_qmix"]).system.mixer == "qmix"
    assert compose("default_rec_qmix", ["env=smax_native"]).env.env_name == "Smax"


@pytest.mark.parametrize("system", ["rec_qmix", "rec_vdn"])
@pytest.mark.parametrize("override,exc,msg", [
    (["env=rware"], ValueError, "pre-reset observation"),
    (["env=smax"], ValueError, "pre-reset observation"),
    (["system.update_batch_size=2"], NotImplementedError, "update_batch_size"),
    (["network.hidden_state_dim=64"], ValueError, "hidden_state_dim"),
    (["network.q_network.pre_torso.layer_sizes=[64]"], NotImplementedError, "torsos"),
    (["network.q_network.post_torso.activation=tanh"], NotImplementedError, "torsos"),
])
def test_run_experiment_refuses_what_rec_iql_refuses(system, override, exc, msg):
    import importlib

    mod = importlib.import_module(f"mava_amd.systems.q_learning.{system}")
    with pytest.raises(exc, match=msg):
        mod.run_experiment(compose(f"default_{system}", override))
    with pytest.raises(exc, match=msg):
        mod._check_config(compose(f"default_{system}", override))


def test_check_config_refuses_bad_mixer_keys():
    from mava_amd.systems.q_learning import rec_qmix, rec_vdn

    with pytest.raises(ValueError, match="mixer_embed_dim"):
        rec_qmix._check_config(compose("default_rec_qmix", ["system.mixer_embed_dim=65"]))
    with pytest.raises(ValueError, match="system.mixer"):
        rec_qmix._check_config(compose("default_rec_qmix", ["system.mixer=vdn"]))
    with pytest.raises(ValueError, match="system.mixer"):
        rec_vdn._check_config(compose("default_rec_vdn", ["system.mixer=qmix"]))
    rec_qmix._check_config(compose("default_rec_qmix"))
    rec_vdn._check_config(compose("default_rec_vdn", ["env=connector"]))


def test_learner_refuses_env_without_terminal_observation():
    from mava_amd.qmix_learner import QMIXLearner

    class Env:  # the synthetic stand-in's surface, no pre-reset observation
        num_envs, num_agents, action_dim, obs_dim = 16, 3, 6, 21

    with pytest.raises(ValueError, match="pre-reset observation"):
        QMIXLearner(Env(), compose("default_rec_qmix"), device="cpu")


def test_entry_points_report_argument_errors():
    """Every refusal comes back as an error code before anything is launched (all pointers are NULL or fake)."""
    L = _lib.lib()
    err = lambda: L.mava_last_error()
    P = 4096  # a non-null address that is never dereferenced: every call below is refused on the host
    td = lambda mode=1, Lq=4, B=8, A=3, Rp=32, nA=6, Em=32, ins=(P,) * 7, hyp=(P,) * 8, dq=P + 64, grads=(P + 128,) * 4, part=P, nblk=4: \
        L.mava_qmix_td_f32(mode, Lq, B, A, Rp, nA, Em, *ins, *hyp, 0.99, 1.0, dq, *grads, part, nblk, None)
    assert td(A=17) <= -1000 and b"agents" in err()
    assert td(Em=65) <= -1000 and b"Em=65" in err()
    assert td(nA=33) <= -1000 and b"n_actions" in err()
    assert td(B=11, A=3, Rp=32) <= -1000 and b"holding B*A=33" in err()
    assert td(Rp=40) <= -1000 and b"multiple of 32" in err()
    assert td(nblk=0) <= -1000 and b"nblk" in err()
    assert td(mode=2) <= -1000 and b"mode" in err()
    assert td(ins=(None,) * 7) <= -1000 and b"null pointer" in err()
    for i in range(8):
        hyp = [P] * 8
        hyp[i] = None
        assert td(hyp=tuple(hyp)) <= -1000 and b"null hypernet pointer" in err()
    assert td(grads=(None,) * 4) <= -1000 and b"null hypernet pointer" in err()
    assert td(dq=P) <= -1000 and b"alias" in err()
    assert td(grads=(P,) * 4) <= -1000 and b"alias" in err()
    st = lambda Lq=4, B=8, A=3, O=5, Rp=32, kp=32, ptrs=(P, P + 64, P + 128, P + 192): \
        L.mava_qmix_state_t32_f32(Lq, B, A, O, Rp, kp, *ptrs, None)
    assert st(B=11) <= -1000 and b"holding B*A=33" in err()
    assert st(kp=14) <= -1000 and b"k_pad" in err()
    assert st(ptrs=(None,) * 4) <= -1000 and b"null pointer" in err()
    assert st(ptrs=(P, P + 64, P + 128, P + 128)) <= -1000 and b"alias" in err()
