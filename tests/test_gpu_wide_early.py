"""The wide f16x2 critic's early layer 1 (ppo_train_h2.hip, P1_EARLY): in the exact-input tile loop the loader group runs layer 1
of tile i + 1 under the chain group's backward phases of tile i and hands the h1 image and the ReLU bits over behind barrier E.
The launch forced through the general loop (MAVA_CTX_TRAIN_VARIANT bit 1) runs the layer at the top of every tile, split between
the groups: it is the reference, bit for bit, for the slab rows and the loss sums, at every place the hand-over can go wrong - a
block's first, second, middle and last tile, blocks of one tile, partial last tiles, a tile with low terms anywhere in a block -
and the handle's MAVA_CTX_EXACT_TILES must equal the host's count of the tiles that may run in the exact loop."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

A = 4
# (input width, kernel instance): 264 = 4 x 66 is the headline instance (18 steps); 152 = 4 x 38 runs the 12-step one
WIDTHS = [(264, 2401184), (152, 2401124)]
# (blocks, tiles, rows in the last tile): 1, 2, 3 and 5 tiles per block, and one grid where the blocks differ (5, 4, 4)
GRIDS = [(1, 1, 32), (1, 1, 1), (1, 2, 31), (1, 3, 32), (1, 5, 1), (2, 2, 31), (2, 4, 32), (2, 6, 1), (2, 10, 31), (3, 3, 1),
         (3, 6, 32), (3, 9, 31), (3, 15, 32), (3, 13, 31)]
PATTERNS = ["exact", "first", "second", "middle", "last", "block"]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _block_tiles(n_slab, ntiles):
    """Static striding of the persistent blocks: block k runs tiles k, k + n_slab, ..."""
    return [list(range(k, ntiles, n_slab)) for k in range(n_slab)]


def _inexact_tiles(pattern, n_slab, ntiles):
    """Tiles that carry a low term, or None when the grid has no such tile (a block too short for the pattern)."""
    blocks = _block_tiles(n_slab, ntiles)
    bad = set()
    if pattern == "block":  # every tile of the LAST block; the other blocks stay exact throughout
        bad.update(blocks[-1])
        return bad
    for tiles in blocks:
        if pattern == "first":
            bad.add(tiles[0])
        elif pattern == "second" and len(tiles) >= 2:  # the flag is set by the very first commit behind barrier B
            bad.add(tiles[1])
        elif pattern == "middle" and len(tiles) >= 3:
            bad.add(tiles[len(tiles) // 2])
        elif pattern == "last":
            bad.add(tiles[-1])
    return bad if (bad or pattern == "exact") else None


def _predicted_exact_tiles(bad, n_slab, ntiles):
    """One-way rule: a block stays in the exact loop up to its first tile with a low term."""
    n = 0
    for tiles in _block_tiles(n_slab, ntiles):
        for t in tiles:
            if t in bad:
                break
            n += 1
    return n


def _inputs(rng, din, Rb, bad):
    """f16-exact rows (bits and two small integers); ONE element of every tile in `bad` carries a low term."""
    TE = Rb + 13  # (indices the minibatch does not draw)
    gs = (rng.random((TE, din)) < 0.2).astype(np.float32)
    gs[:, :2] = rng.integers(0, 10, (TE, 2)).astype(np.float32)
    idx = rng.permutation(TE)[:Rb].astype(np.int32)
    for t in bad:
        pos = np.arange(32 * t, min(32 * t + 32, Rb))
        gs[idx[rng.choice(pos)], rng.integers(0, din)] += np.float32(1.0 / 3.0)
    old_v = rng.standard_normal(TE * A).astype(np.float32)
    tgt = (old_v + rng.standard_normal(TE * A)).astype(np.float32)
    return gs, idx, old_v, tgt


class _Pair:
    """The launch under test and the launch forced through the general loop, on handles of their own."""

    def __init__(self):
        from mava_amd._lib import Ctx

        self.ctxs = {v: Ctx("f16x2") for v in (0, 2)}
        self.ctxs[2].set(Ctx.TRAIN_VARIANT, 2)

    def run(self, dev, flat, gs, idx, old_v, tgt, Rb, n_slab, instance):
        from mava_amd import ops
        from mava_amd._lib import Ctx, lib

        slabs, counts = {}, {}
        for variant, ctx in self.ctxs.items():
            ctx.set(Ctx.EXACT_TILES, 0)
            slab = torch.zeros((n_slab, flat.size + 2), device=dev)
            ops.ppo_critic_grad(_t(flat, dev), _t(gs, dev), A, _t(old_v, dev), _t(tgt, dev), _t(idx, dev), 0, Rb, A, 0.2, 0.5, slab,
                                ctx=ctx)
            torch.cuda.synchronize()
            assert lib().mava_debug_train_last_instance() == instance, "the wide f16x2 critic instantiation took the launch"
            slabs[variant], counts[variant] = slab, ctx.get(Ctx.EXACT_TILES)
        return slabs, counts

    def close(self):
        for ctx in self.ctxs.values():
            ctx.close()


def _assert_same_bits(slabs, counts, want_n, Pn, what):
    assert torch.equal(slabs[0][:, :Pn], slabs[2][:, :Pn]), f"{what}: slab rows differ from the general loop's"
    assert torch.equal(slabs[0][:, Pn:], slabs[2][:, Pn:]), f"{what}: loss sums differ from the general loop's"
    assert counts[2] == 0, f"{what}: the forced launch ran {counts[2]} tiles in the exact loop"
    assert counts[0] == want_n, f"{what}: {counts[0]} exact-loop tiles, predicted {want_n}"


@pytest.mark.parametrize("n_slab,ntiles,last_rows", GRIDS)
@pytest.mark.parametrize("din,instance", WIDTHS)
def test_early_layer1_same_bits_and_counted(dev, din, instance, n_slab, ntiles, last_rows):
    """Every place of a tile with low terms in a block (and none): slab rows and loss sums bit-identical to the general loop,
    exact-loop tile count equal to the host's prediction."""
    Rb = 32 * (ntiles - 1) + last_rows
    rng = np.random.default_rng(din * 1000 + n_slab * 100 + ntiles)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    pair = _Pair()
    ran = 0
    for pattern in PATTERNS:
        bad = _inexact_tiles(pattern, n_slab, ntiles)
        if bad is None:
            continue
        gs, idx, old_v, tgt = _inputs(rng, din, Rb, bad)
        slabs, counts = pair.run(dev, flat, gs, idx, old_v, tgt, Rb, n_slab, instance)
        want_n = _predicted_exact_tiles(bad, n_slab, ntiles)
        print(f"{din}/{n_slab}x{ntiles}/{last_rows}/{pattern}: exact-loop tiles {counts[0]} (predicted {want_n}), forced {counts[2]}")
        _assert_same_bits(slabs, counts, want_n, flat.size, pattern)
        ran += 1
    pair.close()
    assert ran >= 4  # exact, first, last and block exist on every grid


@pytest.mark.parametrize("din,instance", WIDTHS)
def test_relu_bits_of_activations_that_round_to_zero(dev, din, instance):
    """Hidden features whose layer-1 value is positive but below 2^-25: both f16 terms of the h1 image are zero, the ReLU bit is
    set, and the layer-1 gradient of those features is what the general loop computes - the bits travel beside the image."""
    n_slab, ntiles, last_rows = 2, 6, 31
    Rb = 32 * (ntiles - 1) + last_rows
    rng = np.random.default_rng(din + 7)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    W1 = flat[: din * 128].reshape(din, 128)  # (views into flat: row din of the layer-1 block is b1)
    b1 = flat[din * 128 : (din + 1) * 128]
    const = np.arange(3, 128, 8)  # z1 = 2^-27 in every row: the column of W1 is zero, the bias tiny
    small = np.arange(5, 128, 8)  # z1 = 2^-27 + a sum of weights of magnitude ~2^-26
    W1[:, const] = 0.0
    W1[:, small] *= np.float32(2.0 ** -23)
    b1[const] = np.float32(2.0 ** -27)
    b1[small] = np.float32(2.0 ** -27)
    gs, idx, old_v, tgt = _inputs(rng, din, Rb, set())
    z1 = gs[idx].astype(np.float64) @ W1.astype(np.float64) + b1.astype(np.float64)
    tiny = (z1 > 0.0) & (z1 < 2.0 ** -25)
    assert tiny[:, const].all() and tiny[:, small].any(), "no positive layer-1 value below 2^-25: the case tests nothing"
    print(f"{din}: {int(tiny.sum())} of {tiny.size} layer-1 values in (0, 2^-25)")
    pair = _Pair()
    slabs, counts = pair.run(dev, flat, gs, idx, old_v, tgt, Rb, n_slab, instance)
    pair.close()
    _assert_same_bits(slabs, counts, ntiles, flat.size, "tiny activations")
    # the gradient of those features' biases is not zero: their ReLU bits were set (an image read back would say zero)
    db1 = slabs[0].double().sum(0).cpu().numpy()[din * 128 : (din + 1) * 128]
    assert np.all(db1[const] != 0.0), "the bias gradient of a feature with tiny positive activations is zero"


def test_early_layer1_against_float64(dev):
    """One launch that stays in the exact loop against the float64 model, at the tolerances of tests/test_gpu_wide_exact.py."""
    din, instance = WIDTHS[0]
    n_slab, ntiles, last_rows = 3, 13, 27
    Rb = 32 * (ntiles - 1) + last_rows
    rng = np.random.default_rng(20)
    flat = po.mlp_flatten(po.init_mlp(rng, din, 1, 1.0)).astype(np.float32)
    gs, idx, _, _ = _inputs(rng, din, Rb, set())
    TE = gs.shape[0]
    v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), gs.astype(np.float64))[:, 0]
    old_v = (np.repeat(v_now, A) + rng.standard_normal(TE * A) * 0.2).astype(np.float32)
    tgt = (np.repeat(v_now, A) + rng.standard_normal(TE * A)).astype(np.float32)
    pair = _Pair()
    slabs, counts = pair.run(dev, flat, gs, idx, old_v, tgt, Rb, n_slab, instance)
    pair.close()
    Pn = flat.size
    _assert_same_bits(slabs, counts, ntiles, Pn, "exact")
    rows = np.repeat(idx.astype(np.int64), A) * A + np.tile(np.arange(A), Rb)  # agent rows in launch order
    got = slabs[0].double().sum(0).cpu().numpy()
    _, vl, want = po.critic_loss_and_grad(flat.astype(np.float64), din, gs[rows // A].astype(np.float64),
                                          old_v[rows].astype(np.float64), tgt[rows].astype(np.float64), 0.2, 0.5)
    assert_close(got[:Pn], want, 1e-4, "critic grad")
    assert_close(got[Pn : Pn + 1], np.array([vl]), 1e-5, "value loss", scale=1.0)
