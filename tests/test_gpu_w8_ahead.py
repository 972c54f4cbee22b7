"""The gathers-ahead form of the eight-wave kernel's deferred-dW1 tile loop (ppo_train_w8.hip, w8_body AH): on the f16 record the
actor's staging waves issue the x gathers of tile n + 2 in P3 of tile n, into the registers that the commit of tile n + 1 has just
emptied, and load the index of tile n + 3 there.  The form moves loads and cursor updates only, so every check is torch.equal
of whole slabs between three launches on the same data - staging from the f32 rows, the record with MAVA_CTX_TRAIN_VARIANT bit 3 (the deferred form with the gathers in front of barrier A) and the record with
the default - and the handle's three device counters say which form each launch ran.  Record rows that no row of the launch
refers to hold 6e4: a gather from a wrong row shows in the slab.

The cursors run two tiles ahead for the gathers and three for the index, so the shapes are about the ends of a block's tile
sequence: 9 tiles over 1, 2, 3, 4, 9 and 16 blocks (9, 5/4, 3/3/3, 3/2/2/2, one each, none), one block with 1, 2, 3 and 4 tiles
(the prologue's extra stage and each have-next condition where it first turns false), consecutive rows from a base.

Mutants of the kernel this file was run against once (scratch copies, one library each; failed cases of 17): the gathers of tile
n + 2 addressed with the index of tile n + 1: 11; the prologue's second stage dropped: 12; "gathers for n + 2 exist" one tile too
strict: 11; "an index for n + 3 exists" one tile too strict: 8 (the blocks with four tiles or more: 9 tiles on one and on two
blocks, the four widths, the base, 32 index rows); "a commit for n + 1 exists" one tile too strict: 12.  The five cases no
staging mutant can fail: blocks of at most one tile (8 index rows; 9 and 16 blocks), sixteen loss lanes and the value network (no
form); two tiles on one block have no tile n + 2 either."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close
from tests.test_gpu_w8_defer import (A, TE, _actor_data, _assert_off_the_kinks, _check_actor_oracle, _exact_rows, _launch_rows,
                                     _record, _t, _w8_id)

pytestmark = pytest.mark.gpu

NO_AHEAD = 8  # MAVA_CTX_TRAIN_VARIANT bit 3
FILL = 6e4    # finite in f16: a wrong row moves the slab by orders of magnitude instead of making it NaN on every path


def _counted(ctx, variant, launch):
    """Runs `launch` on `ctx` under MAVA_CTX_TRAIN_VARIANT = variant; returns (kernel instance, (launches that staged from the
    record, of which in the deferred-dW1 form, of which with the gathers ahead))."""
    from mava_amd._lib import Ctx, lib

    ctx.set(Ctx.TRAIN_VARIANT, variant)
    for key in (Ctx.X16_W8_LAUNCHES, Ctx.W8_DEFER_LAUNCHES, Ctx.W8_AHEAD_LAUNCHES):
        ctx.set(key, 0)
    launch()
    torch.cuda.synchronize()
    return lib().mava_debug_train_last_instance(), tuple(
        ctx.get(key) for key in (Ctx.X16_W8_LAUNCHES, Ctx.W8_DEFER_LAUNCHES, Ctx.W8_AHEAD_LAUNCHES))


def _guarded_record(x, dev, rows):
    """The record of x with every row outside `rows` (the agent rows of the launch) filled with FILL."""
    rec = _record(x, dev)
    other = torch.ones(x.shape[0], dtype=torch.bool, device=dev)
    other[_t(rows, dev)] = False
    rec[other] = FILL
    return rec


def _three_actor_launches(dev, d, idx, idx_base, Rb, n_slab):
    """(slab, instance, counters) of the f32 staging launch, the record under TRAIN_VARIANT = 8 and the record with the default."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    rec = _guarded_record(d.av, dev, _launch_rows(idx, idx_base, Rb))
    adv, idx_d = _t(d.adv, dev), None if idx is None else _t(idx, dev)
    stats = ops.adv_stats(adv, idx_d, idx_base, Rb, A)
    ctx = Ctx("f16x2")

    def launch(variant, rec=None):
        slab = torch.zeros((n_slab, d.flat.size + 2), device=dev)
        valid = None if rec is None else torch.tensor([1], dtype=torch.int32, device=dev)
        inst, counts = _counted(ctx, variant, lambda: ops.ppo_actor_grad(
            _t(d.flat, dev), _t(d.av, dev), _t(d.mask, dev), _t(d.action, dev), _t(d.old_lp, dev), adv, stats, idx_d, idx_base, Rb,
            A, d.nA, 0.2, 0.01, slab, ctx=ctx, input16=rec, input16_valid=valid))
        return slab, inst, counts

    out = [launch(0), launch(NO_AHEAD, rec), launch(0, rec)]
    ctx.close()
    return out


def _seed(din, Rb, n_slab, idx_base):
    return din * 1000 + Rb * 20 + n_slab + idx_base


# (din, actions, instance, Rb, n_slab, index vector?, idx_base).  65 x 4 = 260 rows = 9 tiles, the last one with 4 rows; 8, 16, 24
# and 32 index rows are 1, 2, 3 and 4 full tiles.  n_slab = 3: the tile stride is no multiple of the ring's three slots.  Widths
# with one, two, three (twice) and four 32-input steps of layer 1; 126 is <8, 4, 2, 0>, which takes the form too.
AHEAD_CASES = [
    (70, 5, _w8_id(True, 8, 3, 2), 65, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 2, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 4, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 9, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 16, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 8, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 16, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 24, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 32, 1, True, 0),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 2, False, 37),
    (70, 5, _w8_id(True, 8, 3, 2), 65, 3, True, 0),
    (30, 5, _w8_id(True, 8, 1, 2), 65, 2, True, 0),
    (62, 5, _w8_id(True, 8, 2, 2), 65, 2, True, 0),
    (94, 5, _w8_id(True, 8, 3, 2), 65, 2, True, 0),
    (126, 5, _w8_id(True, 8, 4, 2), 65, 2, True, 0),
]


@pytest.mark.parametrize("din,nA,instance,Rb,n_slab,use_idx,idx_base", AHEAD_CASES)
def test_actor_gathers_ahead_equals_both_other_schedules(dev, din, nA, instance, Rb, n_slab, use_idx, idx_base):
    """f32 staging, the deferred form with the gathers in front of barrier A and with the gathers ahead: whole slabs bit for bit,
    the counters (0, 0, 0), (1, 1, 0), (1, 1, 1), the sum within the actor gradient tests' tolerance of the float64 model."""
    rng = np.random.default_rng(_seed(din, Rb, n_slab, idx_base))
    d = _actor_data(rng, din, nA)
    idx = rng.permutation(TE)[:Rb].astype(np.int32) if use_idx else None
    (f32, i0, c0), (near, i1, c1), (got, i2, c2) = _three_actor_launches(dev, d, idx, idx_base, Rb, n_slab)
    assert i0 == i1 == i2 == instance, "the eight-wave instantiation took all three launches"
    assert (c0, c1, c2) == ((0, 0, 0), (1, 1, 0), (1, 1, 1)), "(record, deferred, ahead) launches of: no record, TRAIN_VARIANT = 8, default"
    assert torch.isfinite(got).all(), "a filled record row reached the slab"
    assert torch.equal(near, f32), "deferred form with the gathers in front of barrier A differs from f32 staging"
    assert torch.equal(got, near), "gathers-ahead form differs from the deferred form with the gathers in front of barrier A"
    assert torch.equal(got, f32), "gathers-ahead form differs from f32 staging"
    _check_actor_oracle(d, got, idx, idx_base, Rb)


def test_sixteen_loss_lanes_never_run_ahead(dev):
    """11 actions: sixteen loss lanes, every thread stages (ROLE 0) - that body has neither form; the default launch on the record
    counts none of the two and equals the other launches."""
    din, nA, Rb, n_slab = 70, 11, 65, 2
    rng = np.random.default_rng(7012)  # (the seed of the same case in test_gpu_w8_defer.py: off the ReLU kinks)
    d = _actor_data(rng, din, nA)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    (f32, i0, c0), (near, i1, c1), (got, i2, c2) = _three_actor_launches(dev, d, idx, 0, Rb, n_slab)
    assert i0 == i1 == i2 == _w8_id(True, 16, 3, 2)
    assert (c0, c1, c2) == ((0, 0, 0), (1, 0, 0), (1, 0, 0))
    assert torch.equal(near, f32) and torch.equal(got, f32)


def test_narrow_critic_keeps_its_gathers_and_equals_both_other_schedules(dev):
    """The value network on agents_view (ACTOR = false, one output, x_share = 1) with the record, as ff_ippo runs it: its instances
    keep the gathers in front of barrier A (the form made ff_ippo slower), so the default launch counts (1, 1, 0) - and the three
    launches still agree bit for bit beside the filled record rows."""
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
    r = _launch_rows(idx, 0, Rb)
    rec = _guarded_record(x, dev, r)
    ctx = Ctx("f16x2")

    def launch(variant, rec=None):
        slab = torch.zeros((n_slab, flat.size + 2), device=dev)
        valid = None if rec is None else torch.tensor([1], dtype=torch.int32, device=dev)
        inst, counts = _counted(ctx, variant, lambda: ops.ppo_critic_grad(
            _t(flat, dev), _t(x, dev), 1, _t(old_v, dev), _t(tgt, dev), _t(idx, dev), 0, Rb, A, 0.2, 0.5, slab, ctx=ctx,
            input16=rec, input16_valid=valid))
        return slab, inst, counts

    (f32, i0, c0), (near, i1, c1), (got, i2, c2) = launch(0), launch(NO_AHEAD, rec), launch(0, rec)
    ctx.close()
    assert i0 == i1 == i2 == _w8_id(False, 8, 3, 2), "the eight-wave critic instantiation took all three launches"
    assert (c0, c1, c2) == ((0, 0, 0), (1, 1, 0), (1, 1, 0))
    assert torch.equal(near, f32), "deferred form under TRAIN_VARIANT = 8 differs from f32 staging"
    assert torch.equal(got, near) and torch.equal(got, f32), "the default launch on the record differs"
    _assert_off_the_kinks(flat, din, x[r])
    Pn = flat.size
    total = got.double().sum(0).cpu().numpy()
    _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, x[r].astype(np.float64), old_v[r].astype(np.float64),
                                          tgt[r].astype(np.float64), 0.2, 0.5)
    assert_close(total[:Pn], want, 1e-4, "critic grad")
    assert_close(total[Pn : Pn + 1], np.array([vl]), 1e-5, "value loss", scale=1.0)
