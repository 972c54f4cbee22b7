"""CPU: the float64 model of ff_mat's continuous head (tests/mat_continuous_model.py), the continuous layout of MATNet against the
C ABI, the argument checks of the five new entry points, the config group and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from mava_amd import _lib
from mava_amd.config import compose
from mava_amd.mat_learner import MATNet, check_supported, check_supported_continuous
from oracle import tanh_normal as tn
from tests import mat_continuous_model as mc

B, A, O, DIM, D = 3, 4, 7, 3, 32
# (B, A, O, d, D, H, n_block): the shapes tests/test_gpu_mat_continuous.py runs the fused step at
SHAPES = [(1, 1, 3, 1, 32, 1, 1), (11, 3, 7, 2, 32, 1, 1), (43, 3, 7, 5, 64, 2, 2), (43, 5, 33, 16, 96, 4, 1), (3, 20, 9, 9, 128, 4, 2),
          (2, 32, 5, 8, 128, 1, 1)]
NEW = ("mava_transformer_shift_action_f32", "mava_transformer_sample_continuous_f32", "mava_transformer_loss_continuous_f32",
       "mava_transformer_param_count_continuous", "mava_transformer_act_continuous_f32")


def _setup(n_head=2, n_block=2, seed=0):
    net = MATNet(O, DIM, A, D, n_head, n_block, continuous=True)
    g = torch.Generator().manual_seed(seed + 1)
    flat = net.init_flat(seed).double() + 0.05 * torch.randn(net.num_params, generator=g, dtype=torch.float64)
    obs = torch.randn((B, A, O), generator=g, dtype=torch.float64)
    return net, flat, obs, g


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_distribution_is_the_oracles():
    """The torch restatement (differentiable) against oracle/tanh_normal.py, clipped branches and far tails included."""
    rng = np.random.default_rng(0)
    mean = rng.standard_normal((400, DIM)) * 2.0
    mean[:20] += 12.0  # z beyond the branch points of log_ndtr on the clipped rows
    mean[20:40] -= 12.0
    log_std = rng.standard_normal(DIM) * 0.5
    action = np.tanh(rng.standard_normal((400, DIM)))
    action.reshape(-1)[::7] = 0.9995 * np.sign(action.reshape(-1)[::7])
    scale = tn.softplus(log_std) + tn.MIN_SCALE
    want, dm, dsc = tn.log_prob_terms(action, mean, scale)
    mt, lt = torch.tensor(mean, requires_grad=True), torch.tensor(log_std, requires_grad=True)
    got = mc.log_prob(torch.tensor(action), mt, mc.scale_of(lt))
    assert float((got.detach() - torch.tensor(want.sum(-1))).abs().max()) < 1e-10
    got.sum().backward()
    # the oracle's clipped-branch derivative is pdf / cdf; autograd differentiates log_ndtr's branches themselves (erfc of the
    # far side, the truncated series): the two agree to the series' truncation, about 1e-7 of the largest entry
    assert np.abs(mt.grad.numpy() - dm).max() <= 1e-6 * np.abs(dm).max()
    dls = (dsc * tn.sigmoid(log_std)).sum(0)
    assert np.abs(lt.grad.numpy() - dls).max() <= 1e-6 * np.abs(dls).max()
    eps = rng.standard_normal((400, DIM))
    ent = mc.entropy(torch.tensor(mean), torch.tensor(scale), torch.tensor(eps))
    want_ent = (0.5 + tn.HALF_LOG_2PI + np.log(scale) + tn.tanh_fldj(mean + scale * eps)).sum(-1)
    assert float((ent - torch.tensor(want_ent)).abs().max()) <= 1e-10 * float(np.abs(want_ent).max())


def test_shifted_action():
    a = torch.arange(2 * 4 * 3, dtype=torch.float64).view(2, 4, 3) + 1.0
    s = mc.shifted_action(a)
    assert float(s[:, 0].abs().max()) == 0.0 and torch.equal(s[:, 1:], a[:, :-1])
    s = mc.shifted_action(a, known=1)
    assert torch.equal(s[:, 1], a[:, 0]) and float(s[:, 2:].abs().max()) == 0.0 and float(s[:, 0].abs().max()) == 0.0
    assert float(mc.shifted_action(a, known=0).abs().max()) == 0.0


def test_causality():
    net, flat, obs, g = _setup()
    p = net.tree(flat)
    action = torch.tanh(torch.randn((B, A, DIM), generator=g, dtype=torch.float64))
    _, value, mean, _ = mc.forward(p, obs, action, 2)
    for j in range(A):
        a2 = action.clone()
        a2[:, j, 0] += 0.1
        _, v2, m2, _ = mc.forward(p, obs, a2, 2)
        assert torch.equal(m2[:, : j + 1], mean[:, : j + 1]), f"agent {j}'s action reached the means of agents <= {j}"
        assert torch.equal(v2, value)
        if j + 1 < A:
            assert (m2[:, j + 1 :] != mean[:, j + 1 :]).any()


@pytest.mark.parametrize("greedy", [False, True])
def test_teacher_forced_equals_autoregressive(greedy):
    """The teacher-forced pass on the model's own sampled actions gives the means that acting produced."""
    net, flat, obs, g = _setup()
    p = net.tree(flat)
    eps = None if greedy else mc.sample_noise(mc.SEED, 3, B, A, DIM)
    action, lp_act, value, mean_act = mc.act(p, obs, eps, 2)
    lp, v2, mean, scale = mc.forward(p, obs, action, 2)
    assert float((mean - mean_act).abs().max()) < 1e-12 and float((lp - lp_act).abs().max()) < 1e-12
    assert float((v2 - value).abs().max()) < 1e-12
    if greedy:
        assert torch.equal(action, torch.tanh(mean_act))
    # forced: conditioning on the same actions is the same computation; on other actions only agent 0 keeps its mean
    a2, _, _, m2 = mc.act(p, obs, eps, 2, forced=action)
    assert torch.equal(a2, action) and torch.equal(m2, mean_act)
    _, _, _, m3 = mc.act(p, obs, eps, 2, forced=-action)
    assert torch.equal(m3[:, 0], mean_act[:, 0]) and (m3[:, 1:] != mean_act[:, 1:]).any()


def test_gradient_against_central_differences():
    net, flat, obs, g = _setup(n_head=2, n_block=1)
    action = torch.tanh(torch.randn((B, A, DIM), generator=g, dtype=torch.float64))
    action[0, 1, 0], action[2, 3, 1] = 0.9995, -0.9995
    old_lp = mc.forward(net.tree(flat), obs, action, 2)[0] + 0.2 * torch.randn((B, A), generator=g, dtype=torch.float64)
    adv, old_v, tgt = (torch.randn((B, A), generator=g, dtype=torch.float64) for _ in range(3))
    eps = mc.entropy_noise(mc.SEED, 5, np.arange(B), A, DIM)

    def f(x):
        return mc.loss(net.tree(x), obs, action, old_lp, adv, 0.1 * old_v, tgt, 2, 0.2, 0.01, 0.5, eps)[0]

    x = flat.clone().requires_grad_(True)
    f(x).backward()
    grad = x.grad
    idx = torch.randperm(net.num_params, generator=g)[:40].tolist() + [net.off[p] for p, _, _ in net.spec]
    idx += list(range(net.num_params - DIM, net.num_params))  # every log_std entry
    h = 1e-6
    for i in idx:
        e = torch.zeros_like(flat)
        e[i] = h
        num = float(f(flat + e) - f(flat - e)) / (2 * h)
        assert abs(num - float(grad[i])) <= 1e-6 * max(1.0, float(grad.abs().max())), (i, num, float(grad[i]))
    assert float(grad[-DIM:].abs().min()) > 1e-4


@pytest.mark.parametrize("d", mc.DIMS)
def test_loss_head_is_the_models_loss(d):
    """The NumPy loss head (the loss kernel's reference) against torch autograd through loss_terms on the same rows."""
    c = mc.loss_case(d, *mc.LOSS_SHAPES[0])
    mean, log_std, values, action, old_lp, adv, old_value, target, eps = (torch.tensor(np.asarray(a, np.float64)) for a in c["rows_in"])
    mean.requires_grad_(True), log_std.requires_grad_(True), values.requires_grad_(True)
    scale = mc.scale_of(log_std)
    total, actor, vloss, ent = mc.loss_terms(mc.log_prob(action, mean, scale), mc.entropy(mean, scale, eps), values, old_lp, adv, old_value,
                                             target, mc.CLIP, mc.ENT_COEF, mc.VF_COEF)
    total.backward()
    w = c["want"]
    for got, want in ((actor, w["actor_loss"]), (ent, w["entropy"]), (vloss, w["value_loss"])):
        assert abs(float(got.detach()) - float(want)) < 1e-12
    # (1e-6: the clipped branch's pdf / cdf against autograd through log_ndtr's series, as in test_distribution_is_the_oracles)
    for got, want in ((mean.grad, w["dmean"]), (values.grad, w["dvalues"]), (log_std.grad, w["dlog_std"])):
        assert np.abs(got.numpy() - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    # both clipped action branches and both sides of the ratio clip are in the case
    a = c["rows_in"][3]
    f64 = lambda x: np.asarray(x, np.float64)
    ratio = np.exp(tn.log_prob_terms(a, f64(c["mean"]), tn.softplus(f64(c["log_std"])) + tn.MIN_SCALE)[0].sum(-1) - c["rows_in"][4])
    assert (ratio < 1 - mc.CLIP).any() and (ratio > 1 + mc.CLIP).any()
    assert d == 1 or (np.abs(a) >= tn.THRESH).any()  # (d = 1: 48 action entries, the planted ones need not be in the minibatch)


def test_float32_floor_of_the_loss():
    """The float32 NumPy evaluation of the loss head's gradients against float64 at the GPU loss test's inputs
    (tests/test_gpu_mat_continuous.py::test_loss_kernel), relative in assert_close's form.  Measured: at most 1.4e-05 on 19 of the
    20 cases, inside the project's 1e-4, which the GPU test keeps there; 1.56e-04 at d = 8, (Bm, A) = (7, 5) (dlog_std; dmean
    5.6e-05), where the GPU bound is four times the case's measured floor, 6.2e-04 (mat_continuous_model.loss_grad_bound)."""
    floors = {}
    for d in mc.DIMS:
        for shape in mc.LOSS_SHAPES:
            for row_offset in (0, 1000):
                c = mc.loss_case(d, *shape, row_offset)
                floors[(d, shape, row_offset)] = f = mc.loss_f32_floor(c)
                assert mc.loss_grad_bound(c) == (1e-4 if f <= 1e-4 else 4.0 * f)
    print("float32 floor of the continuous loss head:", {k: f"{v:.2e}" for k, v in floors.items()})
    outside = {k: v for k, v in floors.items() if v > 1e-4}
    assert set(k[:2] for k in outside) == {(8, (7, 5))} and max(outside.values()) <= 1.6e-4, outside
    assert 0.0 < max(v for k, v in floors.items() if k not in outside) <= 1.5e-5


# ---- layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_continuous_layout(shape):
    _, A_, O_, d, D_, H, nb = shape
    net = MATNet(O_, d, A_, D_, H, nb, continuous=True)
    lib = _lib.lib()
    assert net.num_params == lib.mava_transformer_param_count_continuous(O_, d, D_, nb)
    assert net.num_params == MATNet(O_, d, A_, D_, H, nb).num_params + d == lib.mava_transformer_param_count(O_, d, D_, nb) + d
    assert net.spec[-1][0] == ("decoder", "log_std") and net.off[("decoder", "log_std")] == net.num_params - d
    spans = sorted((net.off[p], net.off[p] + int(np.prod(s))) for p, s, _ in net.spec)
    assert spans[0][0] == 0 and spans[-1][1] == net.num_params and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    flat = net.init_flat(3)
    tree = net.tree(flat)
    dec = tree["decoder"]
    assert dec["act_dense"]["kernel"].shape == (d, D_) and dec["act_dense"]["bias"].shape == (D_,) and dec["head_out"]["kernel"].shape == (D_, d)
    assert float(dec["act_dense"]["bias"].abs().max()) == 0.0 and float(dec["log_std"].abs().max()) == 0.0 and dec["log_std"].shape == (d,)
    assert torch.equal(flat[-d:], dec["log_std"])
    k = dec["head_out"]["kernel"].double()
    assert torch.allclose(k.T @ k, 1e-4 * torch.eye(d, dtype=torch.float64), atol=1e-10)
    k = dec["act_dense"]["kernel"].double()  # orthogonal(sqrt 2): d <= D orthonormal rows times sqrt 2
    assert torch.allclose(k @ k.T, 2.0 * torch.eye(d, dtype=torch.float64), atol=1e-6)
    assert torch.equal(net.flat_from_tree(net.tree(flat, (1, 1)), torch.zeros_like(flat)), flat)


def test_discrete_layout_is_unchanged():
    net = MATNet(O, 5, A, D, 2, 2)
    assert not net.continuous and ("decoder", "log_std") not in net.off and "bias" not in net.tree(net.init_flat(0))["decoder"]["act_dense"]
    assert net.num_params == _lib.lib().mava_transformer_param_count(O, 5, D, 2)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib._SIGNATURES
    assert lib.mava_abi_version() == 4
    assert lib.mava_transformer_param_count_continuous(0, 2, 64, 1) == -1


def _fake():
    return C.cast((C.c_uint8 * 64)(), C.c_void_p)  # never dereferenced: the checks come first


def test_shift_action_refusals():
    lib, f = _lib.lib(), _fake()
    call = lambda action=f, out=f, B=2, A=3, d=2, known=2, rows=32, n_pad=32: lib.mava_transformer_shift_action_f32(
        action, None, B, A, d, known, rows, n_pad, out, None)
    for bad, word in ((dict(d=0), b"action_dim=0"), (dict(d=17), b"action_dim=17"), (dict(A=33, rows=96), b"A=33"), (dict(rows=48), b"rows=48"),
                      (dict(known=3), b"known=3"), (dict(n_pad=16), b"n_pad=16"), (dict(B=11), b"rows=32"), (dict(out=None), b"null pointer"),
                      (dict(action=None), b"null pointer")):
        assert call(**bad) <= -1000 and word in lib.mava_last_error(), (bad, lib.mava_last_error())


def test_sample_continuous_refusals():
    lib, f = _lib.lib(), _fake()
    call = lambda mean=f, log_std=f, action=f, lp=f, B=2, A=3, agent=0, d=2, ms=1e-3: lib.mava_transformer_sample_continuous_f32(
        B, A, agent, d, ms, mean, log_std, 1, 2, 3, 0, action, lp, None)
    for bad, word in ((dict(d=0), b"action_dim=0"), (dict(d=17), b"action_dim=17"), (dict(A=33), b"A=33"), (dict(agent=3), b"agent=3"),
                      (dict(B=0), b"B=0"), (dict(ms=-1.0), b"min_scale"), (dict(mean=None), b"null pointer"), (dict(log_std=None), b"null pointer"),
                      (dict(action=None), b"null pointer"), (dict(lp=None), b"null pointer")):
        assert call(**bad) <= -1000 and word in lib.mava_last_error(), (bad, lib.mava_last_error())


def test_loss_continuous_refusals():
    lib, f = _lib.lib(), _fake()

    def call(Bm=5, A=3, d=2, rows=32, nb=1, null=None):
        p = [None if null == i else f for i in range(14)]
        return lib.mava_transformer_loss_continuous_f32(Bm, A, d, 1e-3, rows, *p[:10], 3, 0.2, 0.01, 0.5, 1, 2, 3, 1.0, *p[10:], nb, None)

    for bad, word in ((dict(d=0), b"action_dim=0"), (dict(d=17), b"action_dim=17"), (dict(A=33, rows=192), b"A=33"), (dict(rows=48), b"rows=48"),
                      (dict(Bm=11), b"Bm=11"), (dict(nb=0), b"n_blocks=0")):
        assert call(**bad) <= -1000 and word in lib.mava_last_error(), (bad, lib.mava_last_error())
    for i in range(14):
        assert call(null=i) <= -1000 and b"null pointer" in lib.mava_last_error(), i


def test_act_continuous_refusals():
    lib, f = _lib.lib(), _fake()
    good = dict(B=2, A=4, O=7, d=2, D=64, H=2, nb=1, n_blocks=1)

    def call(null=(), ws=f, ws_bytes=None, **over):
        a = dict(good, **over)
        need = lib.mava_transformer_act_workspace_bytes(a["B"], a["A"], a["D"], a["nb"], max(a["n_blocks"], 1))
        p = {k: (None if k in null else f) for k in ("params", "agents_view", "action", "log_prob")}
        return lib.mava_transformer_act_continuous_f32(p["params"], p["agents_view"], a["B"], a["A"], a["O"], a["d"], a["D"], a["H"], a["nb"],
                                                       1e-3, 1, 2, 3, 0, p["action"], p["log_prob"], None, ws,
                                                       need if ws_bytes is None else ws_bytes, a["n_blocks"], None)

    for bad, word in ((dict(d=0), b"action_dim=0"), (dict(d=17), b"action_dim=17"), (dict(A=33), b"A=33"), (dict(A=0), b"A=0"),
                      (dict(D=48), b"D=48"), (dict(D=64, H=3), b"n_head=3"), (dict(O=1025), b"O=1025"), (dict(B=0), b"B=0"),
                      (dict(n_blocks=0), b"n_blocks=0"), (dict(nb=0), b"n_block=0")):
        assert call(**bad) <= -1000 and word in lib.mava_last_error(), (bad, lib.mava_last_error())
    for null in ("params", "agents_view", "action", "log_prob"):
        assert call(null=(null,)) <= -1000 and b"null pointer" in lib.mava_last_error()
    assert call(ws=None) <= -1000 and b"workspace" in lib.mava_last_error()
    assert call(ws_bytes=16) <= -1000 and b"workspace" in lib.mava_last_error()
    assert call(nb=64) == 1  # depth beyond the cap: nothing launched, the caller runs layer by layer


# ---- config and refusals ---------------------------------------------------------------------------------------------------------
def test_config_group():
    cfg = compose("default_ff_mat", ["network=continuous_transformer", "env=spread"])
    assert "ContinuousActionHead" in cfg.network.action_head._target_ and cfg.env.env_name == "Spread"
    assert (int(cfg.network.n_block), int(cfg.network.n_head), int(cfg.network.n_embd), cfg.network.acting) == (1, 1, 64, "layerwise")
    assert compose("default_ff_mat", ["network=continuous_transformer", "env=spread", "network.acting=fused"]).network.acting == "fused"
    assert "DiscreteActionHead" in compose("default_ff_mat").network.action_head._target_


GOOD = dict(num_agents=3, action_dim=2, n_embd=64, n_head=1, independent_std=True, world=1, update_batch_size=1)


@pytest.mark.parametrize("bad", [dict(num_agents=33), dict(num_agents=0), dict(n_embd=48), dict(n_embd=160), dict(n_embd=64, n_head=3),
                                 dict(action_dim=0), dict(action_dim=17), dict(independent_std=False), dict(world=2),
                                 dict(update_batch_size=2)])
def test_continuous_refusals(bad):
    check_supported_continuous(**GOOD)
    with pytest.raises(_lib.MavaHipError):
        check_supported_continuous(**dict(GOOD, **bad))


def test_the_discrete_check_still_refuses_a_continuous_head():
    with pytest.raises(_lib.MavaHipError):
        check_supported(num_agents=4, n_actions=5, n_embd=64, n_head=1, continuous=True, world=1, update_batch_size=1)
