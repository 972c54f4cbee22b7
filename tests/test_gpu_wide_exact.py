"""The wide f16x2 critic kernel's two tile loops (ppo_train_h2.hip): tiles whose input rows are exact in f16 run in an
exact-input loop (hi plane only, two MFMAs per product, the next x tile staged beside the current one); the first tile
with a low term sends the block into the general loop for good.  mava_ppo_critic_grad_f32 is called directly at small
shapes where the host knows, per tile, which loop it must take."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

# (input width, agents): 264 = 4 x 66 aggregated is the headline instance (18 steps, 16-byte pieces); 150 = 2 x 75 aggregated
# runs the 12-step instantiation and 263 (one agent, no aggregation) the 18-step one, both on 4-byte pieces.  (Wide launches
# stage 16-byte or 4-byte pieces only: a width that is even but no multiple of 4 - 150 - takes the 4-byte form.)
WIDTHS = [(264, 4, 2401184), (150, 2, 2401121), (263, 1, 2401181)]
# (blocks, tiles, rows in the last tile)
GRIDS = [(1, 1, 32), (1, 2, 27), (1, 3, 32), (1, 5, 1), (3, 3, 27), (3, 6, 32), (3, 9, 5), (3, 15, 27), (3, 5, 32), (3, 1, 20),
         (1, 1, 7)]
PATTERNS = ["exact", "inexact", "first", "last", "middle"]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _block_tiles(n_slab, ntiles):
    """Static striding of the persistent blocks: block k runs tiles k, k + n_slab, ..."""
    return [list(range(k, ntiles, n_slab)) for k in range(n_slab)]


def _inexact_tiles(pattern, n_slab, ntiles):
    bad = set()
    for tiles in _block_tiles(n_slab, ntiles):
        if not tiles:
            continue
        if pattern == "inexact":
            bad.update(tiles)
        elif pattern == "first":
            bad.add(tiles[0])
        elif pattern == "last":
            bad.add(tiles[-1])
        elif pattern == "middle" and len(tiles) >= 3:
            bad.add(tiles[len(tiles) // 2])
    return bad


def _predicted_exact_tiles(bad, n_slab, ntiles):
    """One-way rule: a block stays in the exact loop up to its first tile with a low term."""
    n = 0
    for tiles in _block_tiles(n_slab, ntiles):
        for t in tiles:
            if t in bad:
                break
            n += 1
    return n


@pytest.mark.parametrize("n_slab,ntiles,last_rows", GRIDS)
@pytest.mark.parametrize("din,A,instance", WIDTHS)
def test_exact_loop_same_bits_and_counted(dev, din, A, instance, n_slab, ntiles, last_rows):
    """Every pattern of exact / inexact tiles: slabs bit-identical to the launch forced through the three-product loop
    (MAVA_CTX_TRAIN_VARIANT bit 1), gradient and value loss at the kernels' 1e-4 / 1e-5 of the float64 oracle, and the
    handle's MAVA_CTX_EXACT_TILES equal to the host's prediction (0 when forced)."""
    from mava_amd import ops
    from mava_amd._lib import Ctx, lib

    rng = np.random.default_rng(din * 1000 + n_slab * 100 + ntiles)
    Rb = 32 * (ntiles - 1) + last_rows
    TE = Rb + 13  # (indices the minibatch does not draw)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    Pn = flat.size
    ctxs = {v: Ctx("f16x2") for v in (0, 2)}
    ctxs[2].set(Ctx.TRAIN_VARIANT, 2)
    for pattern in PATTERNS:
        # f16-exact rows: bits and two small integers
        gs = (rng.random((TE, din)) < 0.2).astype(np.float32)
        gs[:, :2] = rng.integers(0, 10, (TE, 2)).astype(np.float32)
        idx = rng.permutation(TE)[:Rb].astype(np.int32)
        bad = _inexact_tiles(pattern, n_slab, ntiles)
        for t in bad:
            pos = np.arange(32 * t, min(32 * t + 32, Rb))
            if pattern == "inexact":
                gs[idx[pos]] += rng.standard_normal((pos.size, din)).astype(np.float32) * 1e-3
            else:  # ONE element of the tile carries a low term
                gs[idx[rng.choice(pos)], rng.integers(0, din)] += np.float32(1.0 / 3.0)
        rows = np.repeat(idx.astype(np.int64), A) * A + np.tile(np.arange(A), Rb)  # agent rows in launch order
        v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), gs.astype(np.float64))[:, 0]
        old_v = (np.repeat(v_now, A) + rng.standard_normal(TE * A) * 0.2).astype(np.float32)
        tgt = (np.repeat(v_now, A) + rng.standard_normal(TE * A)).astype(np.float32)
        slabs, counts = {}, {}
        for variant, ctx in ctxs.items():
            ctx.set(Ctx.EXACT_TILES, 0)
            slab = torch.zeros((n_slab, Pn + 2), device=dev)
            ops.ppo_critic_grad(_t(flat, dev), _t(gs, dev), A, _t(old_v, dev), _t(tgt, dev), _t(idx, dev), 0, Rb, A, 0.2, 0.5,
                                slab, ctx=ctx)
            torch.cuda.synchronize()
            assert lib().mava_debug_train_last_instance() == instance, "the wide f16x2 critic instantiation took the launch"
            slabs[variant], counts[variant] = slab, ctx.get(Ctx.EXACT_TILES)
        want_n = _predicted_exact_tiles(bad, n_slab, ntiles)
        print(f"{din}/{n_slab}x{ntiles}/{pattern}: exact-loop tiles {counts[0]} (predicted {want_n}), forced {counts[2]}")
        assert torch.equal(slabs[0], slabs[2]), f"{pattern}: exact-loop slabs != three-product slabs"
        assert counts[2] == 0, f"{pattern}: the forced launch ran {counts[2]} tiles in the exact loop"
        assert counts[0] == want_n, f"{pattern}: {counts[0]} exact-loop tiles, predicted {want_n}"
        got = slabs[0].double().sum(0).cpu().numpy()
        _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, gs[rows // A].astype(np.float64),
                                              old_v[rows].astype(np.float64), tgt[rows].astype(np.float64), 0.2, 0.5)
        assert_close(got[:Pn], want, 1e-4, f"{pattern}: critic grad")
        assert_close(got[Pn : Pn + 1], np.array([vl]), 1e-5, f"{pattern}: value loss", scale=1.0)
    for ctx in ctxs.values():
        ctx.close()
