"""The deferred-dW1 form of the eight-wave f16x2 gradient kernel's tile loop (ppo_train_w8.hip, w8_body DF): on the f16 record
the role-split instances run a tile's layer-1 weight gradient inside the next tile's loss phase, from a ring of three x slots and
with an h2 image of its own.  The form changes no bit: every check is torch.equal of whole slabs between three launches on the same
data - staging from the f32 rows, the record with MAVA_CTX_TRAIN_VARIANT bit 2 (the record path with dW1 at the tile's end) and the
record with the default - and the handle's two device counters say which form each launch ran.

Mutants of the kernel this file was run against once (scratch copies; failed cases of 15): a ring of two slots 9, no flush behind
the loop 13, h2 left in L.dz1 10, the deferred product reading slot n mod 3 10.  The first-tile guard removed: 0 - the guard
saves work only, the dz1 image is still zero when the unguarded product would read it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

A = 4
TE = 400
NO_DEFER = 4  # MAVA_CTX_TRAIN_VARIANT bit 2


def _w8_id(actor, no_pad, s1, xv):
    """ppo_train_w8_kernel<NO, S1, XV, ., ACTOR> as mava_debug_train_last_instance() reports it (ppo_train_task.h)."""
    return 3000000 + (100000 if actor else 0) + no_pad * 1000 + s1 * 10 + xv


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rp(din):
    return 8 * ((din + 8) // 8)


def _exact_rows(rng, rows, din):
    """Rows of the synthetic env's kind, exact in f16: a one-hot agent id, two integers 0..9, 0 / 1 flags."""
    x = (rng.random((rows, din)) < 0.2).astype(np.float32)
    x[:, :A] = np.eye(A, dtype=np.float32)[np.arange(rows) % A]
    x[:, A : A + 2] = rng.integers(0, 10, (rows, 2)).astype(np.float32)
    return x


def _record(x, dev, fill=None):
    """The record of x as the rollout writes it: din halves, 1.0, zeros up to RP (or `fill` everywhere)."""
    rows, din = x.shape
    rec = torch.zeros((rows, _rp(din)), dtype=torch.float16, device=dev)
    if fill is not None:
        rec.fill_(fill)
        return rec
    rec[:, :din] = _t(x, dev).half()
    rec[:, din] = 1.0
    assert torch.equal(rec[:, :din].float(), _t(x, dev))
    return rec


def _actor_data(rng, din, nA, exact=True):
    rows = TE * A
    av = _exact_rows(rng, rows, din) if exact else rng.standard_normal((rows, din)).astype(np.float32)
    flat = po.mlp_flatten(po.init_mlp(rng, din, nA, 0.01)).astype(np.float32)
    mask = np.ones((rows, nA), np.uint8)
    mask[:, 1] = rng.random(rows) > 0.2
    y = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, nA), av.astype(np.float64))
    logp = po.log_softmax(po.masked_logits(y, mask))
    u = rng.random(rows)[:, None]  # one legal action per row, drawn uniformly
    legal = mask.astype(np.float64)
    action = (np.cumsum(legal, 1) / legal.sum(1, keepdims=True) > u).argmax(1).astype(np.int32)
    assert mask[np.arange(rows), action].all()
    old_lp = (logp[np.arange(rows), action] + rng.standard_normal(rows) * 0.1).astype(np.float32)
    adv = rng.standard_normal(rows).astype(np.float32)
    return SimpleNamespace(din=din, nA=nA, av=av, flat=flat, mask=mask, action=action, old_lp=old_lp, adv=adv)


def _counted(ctx, variant, launch):
    """Runs `launch` on `ctx` under MAVA_CTX_TRAIN_VARIANT = variant; returns (kernel instance, (launches that staged from the
    record, launches in the deferred-dW1 form))."""
    from mava_amd._lib import Ctx, lib

    ctx.set(Ctx.TRAIN_VARIANT, variant)
    ctx.set(Ctx.X16_W8_LAUNCHES, 0)
    ctx.set(Ctx.W8_DEFER_LAUNCHES, 0)
    launch()
    torch.cuda.synchronize()
    return lib().mava_debug_train_last_instance(), (ctx.get(Ctx.X16_W8_LAUNCHES), ctx.get(Ctx.W8_DEFER_LAUNCHES))


def _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab, variant=0, rec=None, word=None):
    from mava_amd import ops

    slab = torch.zeros((n_slab, d.flat.size + 2), device=dev)
    valid = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
    adv, idx_d = _t(d.adv, dev), None if idx is None else _t(idx, dev)
    stats = ops.adv_stats(adv, idx_d, idx_base, Rb, A)
    inst, counts = _counted(ctx, variant, lambda: ops.ppo_actor_grad(
        _t(d.flat, dev), _t(d.av, dev), _t(d.mask, dev), _t(d.action, dev), _t(d.old_lp, dev), adv, stats, idx_d, idx_base, Rb, A,
        d.nA, 0.2, 0.01, slab, ctx=ctx, input16=rec, input16_valid=valid))
    return slab, inst, counts


def _launch_rows(idx, idx_base, Rb):
    p_rows = idx.astype(np.int64) if idx is not None else idx_base + np.arange(Rb, dtype=np.int64)
    return np.repeat(p_rows, A) * A + np.tile(np.arange(A), Rb)  # agent rows in launch order


def _three_actor_launches(dev, d, idx, idx_base, Rb, n_slab, rec, word):
    """(slab, instance, counters) of the f32 staging launch, the record under TRAIN_VARIANT = 4 and the record with the default."""
    from mava_amd._lib import Ctx

    ctx = Ctx("f16x2")
    out = [_launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab),
           _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab, NO_DEFER, rec, word),
           _launch_actor(dev, ctx, d, idx, idx_base, Rb, n_slab, 0, rec, word)]
    ctx.close()
    return out


# (din, actions, instance, Rb, n_slab, index vector?, idx_base).  65 x 4 = 260 rows = 9 tiles, the last one with 4 rows; a block's
# tiles are every n_slab-th one: 9 on one block (the ring of three slots wraps three times), 5 and 4, 3 2 2 2, one each (the
# first-tile guard and the flush behind the loop meet in the same tile), 16 blocks of which seven have none (no flush).  One block
# with a single full tile (8 x 4 rows) and with two (the ring not yet wrapped).  Consecutive rows from a base instead of an index
# vector.  Input widths with one, two, three (twice) and four 32-input steps of layer 1: 1 .. 8 x tiles per deferred product; width
# 126 is <8, 4, 2, 0>, without resident W2 steps.
DEFER_CASES = [
    (70, 5, _w8_id(True, 8, 3, 2), 65, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 2, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 4, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 9, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 16, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 8, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 16, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 2, False, 37),
    (30, 5, _w8_id(True, 8, 1, 2), 65, 2, True, 0),
    (62, 5, _w8_id(True, 8, 2, 2), 65, 2, True, 0),
    (94, 5, _w8_id(True, 8, 3, 2), 65, 2, True, 0),
    (126, 5, _w8_id(True, 8, 4, 2), 65, 2, True, 0),
]


def _assert_off_the_kinks(flat, din, x):
    """Precondition of the comparison with the float64 model, a property of the DATA: no hidden pre-activation of the launch's rows
    within 1e-6 of zero.  The model's gradient jumps where a ReLU input changes sign, and the split-f16 products carry ~2^-22 of
    sum |w x| (~1e-6 here, |z| ~ 0.8 on average): a row that close to the kink may legitimately fall on the other side, which moves
    a whole column of dW1 by that row's share.  (Seed 7011 of the 11-action case had z1 = 8.8e-8 in one of its 33 280 values - and
    two dW1 entries of that feature 3.8 tolerances off under f16x2, none under exact f32; a case that trips this picks another seed.)"""
    H = 128
    f = flat.astype(np.float64)
    W1, b1 = f[: din * H].reshape(din, H), f[din * H : (din + 1) * H]
    o = (din + 1) * H
    W2, b2 = f[o : o + H * H].reshape(H, H), f[o + H * H : o + H * H + H]
    z1 = x.astype(np.float64) @ W1 + b1
    z2 = np.maximum(z1, 0.0) @ W2 + b2
    assert min(np.abs(z1).min(), np.abs(z2).min()) > 1e-6, "test data: a hidden pre-activation sits on a ReLU kink"


def _check_actor_oracle(d, slab, idx, idx_base, Rb):
    rows = _launch_rows(idx, idx_base, Rb)
    _assert_off_the_kinks(d.flat, d.din, d.av[rows])
    P = d.flat.size
    total = slab.double().sum(0).cpu().numpy()
    _, la, ent, want = po.actor_loss_and_grad(d.flat.astype(np.float64), d.din, d.nA, d.av[rows].astype(np.float64), d.mask[rows],
                                              d.action[rows], d.old_lp[rows].astype(np.float64), d.adv[rows].astype(np.float64),
                                              0.2, 0.01)
    assert_close(total[:P], want, 1e-4, "actor grad")
    assert_close(total[P : P + 2], np.array([la, ent]), 1e-5, "actor loss sums", scale=1.0)


@pytest.mark.parametrize("din,nA,instance,Rb,n_slab,use_idx,idx_base", DEFER_CASES)
def test_actor_deferred_form_equals_both_other_schedules(dev, din, nA, instance, Rb, n_slab, use_idx, idx_base):
    """f32 staging, the record with dW1 at the tile's end and the record in the deferred-dW1 form: whole slabs bit for bit, the
    counters (0, 0), (1, 0), (1, 1), the sum within the actor gradient tests' tolerance of the float64 model."""
    rng = np.random.default_rng(din * 1000 + Rb * 20 + n_slab + idx_base)
    d = _actor_data(rng, din, nA)
    idx = rng.permutation(TE)[:Rb].astype(np.int32) if use_idx else None
    (f32, i0, c0), (late, i1, c1), (got, i2, c2) = _three_actor_launches(dev, d, idx, idx_base, Rb, n_slab, _record(d.av, dev), 1)
    assert i0 == i1 == i2 == instance, "the eight-wave instantiation took all three launches"
    assert (c0, c1, c2) == ((0, 0), (1, 0), (1, 1)), "(record, deferred) launches of: no record, TRAIN_VARIANT = 4, default"
    assert torch.equal(late, f32), "record with dW1 at the tile's end differs from f32 staging"
    assert torch.equal(got, late), "deferred-dW1 form differs from the record with dW1 at the tile's end"
    assert torch.equal(got, f32), "deferred-dW1 form differs from f32 staging"
    _check_actor_oracle(d, got, idx, idx_base, Rb)


def test_sixteen_loss_lanes_never_defer(dev):
    """11 actions: sixteen loss lanes, every thread stages (ROLE 0) - that body has no deferred form; the default launch on the
    record counts none and equals the other two."""
    din, nA, Rb, n_slab = 70, 11, 65, 2
    rng = np.random.default_rng(7012)  # (7011: see _assert_off_the_kinks)
    d = _actor_data(rng, din, nA)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    (f32, i0, c0), (late, i1, c1), (got, i2, c2) = _three_actor_launches(dev, d, idx, 0, Rb, n_slab, _record(d.av, dev), 1)
    assert i0 == i1 == i2 == _w8_id(True, 16, 3, 2)
    assert (c0, c1, c2) == ((0, 0), (1, 0), (1, 0))
    assert torch.equal(late, f32) and torch.equal(got, f32)
    _check_actor_oracle(d, got, idx, 0, Rb)


def test_narrow_critic_deferred_form_equals_both_other_schedules(dev):
    """The value network on agents_view (ACTOR = false, one output, x_share = 1) runs the same three schedules."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    din, Rb, n_slab = 70, 65, 2
    rng = np.random.default_rng(7071)
    rows = TE * A
    x = _exact_rows(rng, rows, din)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), x.astype(np.float64))[:, 0]
    old_v = (v_now + rng.standard_normal(rows) * 0.2).astype(np.float32)
    tgt = (v_now + rng.standard_normal(rows)).astype(np.float32)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    rec = _record(x, dev)
    ctx = Ctx("f16x2")

    def launch(variant, rec=None, word=None):
        slab = torch.zeros((n_slab, flat.size + 2), device=dev)
        valid = None if word is None else torch.tensor([word], dtype=torch.int32, device=dev)
        inst, counts = _counted(ctx, variant, lambda: ops.ppo_critic_grad(
            _t(flat, dev), _t(x, dev), 1, _t(old_v, dev), _t(tgt, dev), _t(idx, dev), 0, Rb, A, 0.2, 0.5, slab, ctx=ctx,
            input16=rec, input16_valid=valid))
        return slab, inst, counts

    (f32, i0, c0), (late, i1, c1), (got, i2, c2) = launch(0), launch(NO_DEFER, rec, 1), launch(0, rec, 1)
    ctx.close()
    assert i0 == i1 == i2 == _w8_id(False, 8, 3, 2), "the eight-wave critic instantiation took all three launches"
    assert (c0, c1, c2) == ((0, 0), (1, 0), (1, 1))
    assert torch.equal(late, f32), "record with dW1 at the tile's end differs from f32 staging"
    assert torch.equal(got, late) and torch.equal(got, f32), "deferred-dW1 form differs"
    r = _launch_rows(idx, 0, Rb)
    _assert_off_the_kinks(flat, din, x[r])
    Pn = flat.size
    total = got.double().sum(0).cpu().numpy()
    _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, x[r].astype(np.float64), old_v[r].astype(np.float64),
                                          tgt[r].astype(np.float64), 0.2, 0.5)
    assert_close(total[:Pn], want, 1e-4, "critic grad")
    assert_close(total[Pn : Pn + 1], np.array([vl]), 1e-5, "value loss", scale=1.0)


def test_record_that_must_not_be_read(dev):
    """A record full of NaN beside f32 rows that are not exact in f16, the word 0: every launch takes the f32 form - counters
    (0, 0) - whose tile loop never touches the deferred form's h2 plane behind the small vectors (part of every launch's LDS),
    and gives finite, equal slabs."""
    din, nA, Rb, n_slab = 70, 5, 65, 2
    rng = np.random.default_rng(7000)
    d = _actor_data(rng, din, nA, exact=False)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    rec = _record(d.av, dev, fill=float("nan"))
    (f32, i0, c0), (late, i1, c1), (got, i2, c2) = _three_actor_launches(dev, d, idx, 0, Rb, n_slab, rec, 0)
    assert i0 == i1 == i2 == _w8_id(True, 8, 3, 2)
    assert (c0, c1, c2) == ((0, 0), (0, 0), (0, 0)), "a launch staged from a record whose word is 0"
    assert torch.isfinite(f32).all() and torch.isfinite(got).all() and torch.isfinite(late).all(), "NaN in a slab"
    assert torch.equal(late, f32) and torch.equal(got, f32), "the record was read"
    _check_actor_oracle(d, got, idx, 0, Rb)
