"""Every reachable instance of the feed-forward gradient and acting kernel templates against the float64 oracle, one small
case per instance (tests/instances.py holds the tables and the restatement of the dispatch; DESIGN.md §"Support envelope of
the feed-forward kernels").  Each case asserts through mava_debug_train_last_instance() / mava_debug_policy_last_instance()
WHICH instantiation it compared.  Tolerances are the project's own, not chosen per case: 1e-4 for gradients, 1e-5 for loss sums,
logits, values and log-probs - with one exception, the continuous gradient at (2 dimensions, 130 inputs), held to four times
the error of a float32 NumPy run of the oracle itself (instances.CONTINUOUS_F32_MEASURED, test_continuous_gradient_instance)."""
import numpy as np
import pytest
import torch

from tests import instances as I
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu


def _dev(a, dev, offset=0):
    """`a` on the device; offset > 0: as a view that starts `offset` elements into its allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset == 0:
        return t.to(dev)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=dev)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset * t.element_size()
    return view


def _train_instance():
    from mava_amd._lib import lib

    return lib().mava_debug_train_last_instance()


def _policy_instance():
    from mava_amd._lib import lib

    return lib().mava_debug_policy_last_instance()


def _train_ctx(mode, variant):
    from mava_amd._lib import Ctx

    if mode == "f32":
        return None
    ctx = Ctx("f16x2")
    ctx.set(ctx.TRAIN_VARIANT, variant)
    return ctx


def _check_slab(slab, d, P, what, tail=2, grad_tol=1e-4):
    got = slab.cpu().numpy().astype(np.float64).sum(0)  # two slabs: the order of the sum does not matter
    assert np.isfinite(got).all()
    assert_close(got[:P], d["grad"], grad_tol, f"{what} grad")  # north_star: PPO gradients within 1e-4
    assert_close(got[P : P + tail], d["sums"][:tail], 1e-5, f"{what} loss sums", scale=1.0)


def _check_counters(ctx, want):
    if ctx is not None:
        assert ctx.h2_launches == want.h2_launches, "launches on the f16x2 kernels"
        assert ctx.get(ctx.W8_LAUNCHES) == want.w8_launches, "eight-wave / four-wave kernel selection"
        ctx.close()


def _launch_actor(dev, c, d, ctx):
    from mava_amd import ops

    P = d["flat"].size
    slab = torch.full((I.N_SLAB, P + 2), I.SENTINEL, device=dev)
    adv, idx = _dev(d["adv"], dev), _dev(d["idx"], dev)
    stats = ops.adv_stats(adv, idx, 0, I.RB, I.A)
    ops.ppo_actor_grad(_dev(d["flat"], dev), _dev(d["av"], dev, c.offset), _dev(d["mask"], dev), _dev(d["action"], dev),
                       _dev(d["old_lp"], dev), adv, stats, idx, 0, I.RB, I.A, c.n_actions, 0.2, 0.01, slab, ctx=ctx)
    torch.cuda.synchronize()
    return slab, P


@pytest.mark.parametrize("c", I.ACTOR_CASES, ids=I.case_id)
def test_actor_gradient_instance(dev, c):
    d = I.actor_data(c)
    want = I.predict_actor(c.mode, c.variant, c.din, c.n_actions, c.offset)
    assert want.instance is not None
    ctx = _train_ctx(c.mode, c.variant)
    slab, P = _launch_actor(dev, c, d, ctx)
    assert _train_instance() == want.instance, "another template instance ran than this case was written for"
    _check_counters(ctx, want)
    _check_slab(slab, d, P, "actor")


@pytest.mark.parametrize("n_actions,din", I.ACTOR_F32_REFUSED)
def test_actor_gradient_f32_envelope(dev, n_actions, din):
    """The first input width past the exact-f32 kernel's LDS envelope is refused by an argument error before any launch (14
    actions on 128 inputs and 20 on 32 run on the four-wave f16x2 kernel: ACTOR_CASES; 192 inputs are past the f16x2
    envelope too), and the last width inside it runs (ACTOR_CASES too)."""
    from mava_amd._lib import MavaHipError

    c = I.ActorCase("f32", 0, n_actions, din)
    assert I.predict_actor("f32", 0, din, n_actions).refusal == "LDS"
    assert I.predict_actor("f32", 0, din - 1, n_actions).instance is not None
    before = _train_instance()
    with pytest.raises(MavaHipError, match="LDS"):
        _launch_actor(dev, c, I.actor_data(c), None)
    torch.cuda.synchronize()
    assert _train_instance() == before, "a refused shape launched nothing"


@pytest.mark.parametrize("variant,n_actions,din", I.ACTOR_F16X2_REFUSED)
def test_actor_gradient_f16x2_envelope(dev, variant, n_actions, din):
    """The f16x2 actor ends at 191 inputs whatever the number of actions: the 18-step WIDE instance needs 167 136 bytes of LDS
    with the actor's dy planes (the critic's fits), and launch_h2 refuses it before any launch.  From 192 inputs on a discrete
    actor therefore runs in neither arithmetic (support envelope)."""
    from mava_amd._lib import MavaHipError

    c = I.ActorCase("f16x2", variant, n_actions, din)
    assert I.predict_actor("f16x2", variant, din, n_actions) == I.Prediction(None, "LDS", 0, 0)
    ctx = _train_ctx("f16x2", variant)
    before = _train_instance()
    with pytest.raises(MavaHipError, match="LDS"):
        _launch_actor(dev, c, I.actor_data(c), ctx)
    torch.cuda.synchronize()
    assert _train_instance() == before, "a refused shape launched nothing"
    assert ctx.h2_launches == 0 and ctx.get(ctx.W8_LAUNCHES) == 0
    ctx.close()


@pytest.mark.parametrize("c", I.CRITIC_CASES, ids=I.case_id)
def test_critic_gradient_instance(dev, c):
    from mava_amd import ops
    from mava_amd._lib import Ctx

    d = I.critic_data(c)
    want = I.predict_critic(c.mode, c.variant, c.din, c.agg, I.A, d["share"], c.offset)
    ctx = Ctx(c.mode, critic_aggregation=bool(c.agg))
    ctx.set(ctx.TRAIN_VARIANT, c.variant)
    P = d["flat"].size
    slab = torch.full((I.N_SLAB, P + 2), I.SENTINEL, device=dev)
    ops.ppo_critic_grad(_dev(d["flat"], dev), _dev(d["gs"], dev, c.offset), d["share"], _dev(d["old_v"], dev), _dev(d["tgt"], dev),
                        _dev(d["idx"], dev), 0, I.RB, I.A, 0.2, 0.5, slab, ctx=ctx)
    torch.cuda.synchronize()
    assert _train_instance() == want.instance, "another template instance ran than this case was written for"
    _check_counters(ctx, want)
    _check_slab(slab, d, P, "critic")


def _launch_continuous(dev, c, d):
    from mava_amd import ops

    P = d["flat"].size
    slab = torch.full((I.N_SLAB, P + 2), I.SENTINEL, device=dev)
    adv, idx = _dev(d["adv"], dev), _dev(d["idx"], dev)
    stats = ops.adv_stats(adv, idx, 0, I.RB, I.A)
    ops.ppo_actor_grad_continuous(_dev(d["flat"], dev), _dev(d["av"], dev), _dev(d["action"], dev), _dev(d["old_lp"], dev), adv,
                                  stats, idx, 0, I.RB, I.A, c.dim, 0.2, 0.01, I.CONT_SEED, I.CONT_ENT_STEP, I.CONT_ROW_OFFSET,
                                  slab)
    torch.cuda.synchronize()
    return slab, P


@pytest.mark.parametrize("c", I.CONTINUOUS_CASES, ids=I.case_id)
def test_continuous_gradient_instance(dev, c):
    d = I.continuous_data(c)
    slab, P = _launch_continuous(dev, c, d)
    assert _train_instance() == I.predict_continuous(c.din, c.dim).instance
    # 1e-4, but 4.376e-4 for (2 dimensions, 130 inputs): four times the 1.094e-4 by which a float32 NumPy run of the oracle
    # misses the float64 one there (instances.CONTINUOUS_F32_MEASURED); the kernel's own error there is 1.36e-4
    _check_slab(slab, d, P, "continuous actor", grad_tol=I.continuous_grad_tolerance(c))  # (P: the MLP and the log_std entries)


@pytest.mark.parametrize("dim,din", I.CONTINUOUS_REFUSED)
def test_continuous_gradient_envelope(dev, dim, din):
    """More than 8 action dimensions run the NO = 16 body, whose LDS ends at four 32-input tiles: 128 inputs are the first
    refused width (9 dimensions at kt = 5 cannot run); 8 dimensions and fewer end at 191 inputs like the discrete actor."""
    from mava_amd._lib import MavaHipError

    assert I.predict_continuous(din, dim).refusal == "LDS"
    c = I.ContinuousCase(dim, din)
    before = _train_instance()
    with pytest.raises(MavaHipError, match="LDS"):
        _launch_continuous(dev, c, I.continuous_data(c))
    torch.cuda.synchronize()
    assert _train_instance() == before, "a refused shape launched nothing"


# ------------------------------------------------------------------------------------------ acting kernels
@pytest.mark.parametrize("c", I.STEP_CASES, ids=I.case_id)
def test_policy_step_instance(dev, c):
    """Logits, values, log-probs at 1e-5; sampled and greedy actions EQUAL to the float64 oracle's on every row (the case's
    inputs and sampling seed are the first whose float64 top-two score gaps are >= 1e-3 everywhere: instances.step_data)."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    d = I.step_data(c)
    assert d is not None, "no input draw / sampling seed with a top-two gap >= 1e-3 on every row"
    rows, nA, share = c.rows, c.n_actions, d["share"]
    critic_rows = c.critic_in_rows * share
    ctx = Ctx()
    ctx.set(ctx.POLICY_VARIANT, c.variant)
    fa, fc, av, gs, mask = (_dev(d[k], dev) for k in ("fa", "fc", "av", "gs", "mask"))
    kw = dict(n_actions=nA, seed=d["seed"], step=I.STEP_NUMBER, row_offset=I.ROW_OFFSET, ctx=ctx)
    actor_id, last_id = I.predict_policy_step(c.variant, c.actor_din, nA, c.critic_din, rows, critic_rows)

    action, logp, value, logits = ops.policy_step(fa, fc, av, mask, gs, critic_share=share, want_logits=True, **kw)
    torch.cuda.synchronize()
    assert _policy_instance() == last_id, "another template instance ran than this case was written for"
    r = np.arange(rows)
    a = action.cpu().numpy()
    assert_close(logits.cpu().numpy(), d["logits"], 1e-5, "logits")
    assert np.array_equal(a, d["sampled"]), f"{int((a != d['sampled']).sum())} sampled actions differ from the oracle's"
    assert_close(logp.cpu().numpy(), d["lsm"][r, d["sampled"]], 1e-5, "log_prob")
    assert_close(value.cpu().numpy(), np.repeat(d["value"], share), 1e-5, "value")
    one = d["one_legal_row"]
    assert d["mask"][one].sum() == 1 and d["mask"][one, a[one]] and abs(float(logp[one])) <= 1e-6, "row with one legal action"
    none = d["none_legal_row"]  # no legal action: uniform over the nA real actions (padding slots never enter the softmax sum)
    assert not d["mask"][none].any() and a[none] == 0 and abs(float(logp[none]) + np.log(nA)) <= 1e-5, "row without a legal action"

    if actor_id != last_id:  # block-cooperative kernels, one launch per network: the actor's launch alone
        action_a, logp_a, _, _ = ops.policy_step(fa, fc, av, mask, gs, critic_share=share, critic_rows=0, **kw)
        torch.cuda.synchronize()
        assert _policy_instance() == actor_id
        assert torch.equal(action_a, action) and torch.equal(logp_a, logp)
    if share > 1:  # one critic pass per env, the value written to all `share` agent slots
        action_b, logp_b, value_b, _ = ops.policy_step(fa, fc, av, mask, gs, critic_share=1, critic_rows=c.critic_in_rows,
                                                       value_broadcast=share, **kw)
        torch.cuda.synchronize()
        assert _policy_instance() == I.predict_policy_step(c.variant, c.actor_din, nA, c.critic_din, rows, c.critic_in_rows)[1]
        assert_close(value_b.cpu().numpy(), np.repeat(d["value"], share), 1e-5, "broadcast value")
        assert torch.equal(action_b, action) and torch.equal(logp_b, logp)

    _, logp_f, _, _ = ops.policy_step(fa, fc, av, mask, gs, critic_share=share, forced_action=_dev(d["forced"], dev), **kw)
    assert_close(logp_f.cpu().numpy(), d["lsm"][r, d["forced"]], 1e-5, "forced log_prob")
    action_g, logp_g, _, _ = ops.policy_step(fa, fc, av, mask, gs, critic_share=share, greedy=True, **kw)
    assert np.array_equal(action_g.cpu().numpy(), d["greedy"]), "greedy actions differ from argmax of the masked logits"
    assert_close(logp_g.cpu().numpy(), d["lsm"][r, d["greedy"]], 1e-5, "greedy log_prob")
    ctx.close()


@pytest.mark.parametrize("c", I.FORWARD_CASES, ids=I.case_id)
def test_mlp_forward_instance(dev, c):
    from mava_amd import ops
    from mava_amd._lib import Ctx

    d = I.forward_data(c)
    ctx = Ctx()
    ctx.set(ctx.POLICY_VARIANT, c.variant)
    y = ops.mlp_forward(_dev(d["flat"], dev), c.din, c.n_out, _dev(d["x"], dev), ctx=ctx)
    torch.cuda.synchronize()
    assert _policy_instance() == I.predict_forward(c.variant, c.din, c.n_out)
    assert_close(y.cpu().numpy(), d["want"], 1e-5, "mlp forward")
    ctx.close()
