"""adv_stats_kernel (csrc/ppo_train.hip): rows of 2, 4 or 8 agents are fetched with one 8-byte or one / two 16-byte
loads when the base is aligned to them; the partial sums keep the bits of the scalar loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TE = 5000  # (t, e) rows of the trajectory the minibatches are drawn from


def _adv(dev, A, misalign=0):
    """TE x A advantages with mean 1 (their sum does not cancel: the relative bound below means something); misalign = 1:
    the same values in a view one float off the allocation's 16-byte alignment."""
    g = torch.Generator(device="cpu").manual_seed(100 + A)
    v = torch.randn(TE * A, generator=g) + 1.0
    buf = torch.empty(TE * A + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[misalign : misalign + TE * A].copy_(v)
    return buf[misalign : misalign + TE * A], v.numpy().astype(np.float64).reshape(TE, A)


def _idx(dev, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randperm(TE, generator=g)[:n].to(torch.int32).to(dev)


def _check(partials, rows64):
    s = partials.cpu().numpy().sum(0)
    want = np.array([rows64.sum(), (rows64 * rows64).sum()])
    assert np.all(np.abs(s - want) <= 1e-12 * np.abs(want)), (s, want)


# Rb = 1: one thread; 1000: fewer indices than one pass of the grid's threads holds (4 x 128 x 256), the last three of a
# thread's four slots empty; 4100: not a multiple of 256.  A = 1, 3: scalar loop; 2, 4, 8: the vector paths.
@pytest.mark.parametrize("Rb", [1, 1000, 4100])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 8])
def test_partials_against_float64(dev, A, Rb):
    from mava_amd import ops

    adv, ref = _adv(dev, A)
    idx = _idx(dev, Rb, Rb + A)
    _check(ops.adv_stats(adv, idx, 0, Rb, A), ref[idx.cpu().numpy()])
    base = TE - Rb - 3 if Rb > 1 else TE - 1  # (the last row of the trajectory is read by Rb = 1)
    _check(ops.adv_stats(adv, None, base, Rb, A), ref[base : base + Rb])


@pytest.mark.parametrize("Rb", [1, 1000, 4100])
@pytest.mark.parametrize("A", [2, 4, 8])
def test_vector_path_keeps_the_bits_of_the_scalar_loop(dev, A, Rb):
    """The same values through a 16-byte aligned base (vector loads) and through a view one float off it (scalar loop)."""
    from mava_amd import ops

    adv, _ = _adv(dev, A)
    off, _ = _adv(dev, A, misalign=1)
    assert adv.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and torch.equal(adv, off)
    idx = _idx(dev, Rb, 7 * Rb + A)
    assert torch.equal(ops.adv_stats(adv, idx, 0, Rb, A), ops.adv_stats(off, idx, 0, Rb, A))
    assert torch.equal(ops.adv_stats(adv, None, 5, Rb, A), ops.adv_stats(off, None, 5, Rb, A))


@pytest.mark.parametrize("A", [3, 4])
def test_batched_entry(dev, A):
    from mava_amd import ops

    Rb, nb = 1000, 3
    adv, ref = _adv(dev, A)
    idx = _idx(dev, nb * Rb, 77)
    out = ops.adv_stats_batched(adv, idx, Rb, A, nb)
    for j in range(nb):
        sl = idx[j * Rb : (j + 1) * Rb]
        _check(out[j], ref[sl.cpu().numpy()])
        assert torch.equal(out[j], ops.adv_stats(adv, sl.contiguous(), 0, Rb, A))
    if A == 4:
        off, _ = _adv(dev, A, misalign=1)
        assert torch.equal(out, ops.adv_stats_batched(off, idx, Rb, A, nb))
