"""mava_permutation_batched_i32: the K epoch permutations of an update in one launch, each bit-identical to the
single-permutation launch with counter + k."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, C0 = 0x1234_5678_9ABC_DEF0, 41


# n = 1, 2: the smallest domains (b = 2: cycle walking from 4); 31, 1000: below a power of two; 4097: just above one
# (the longest walks) and 17 blocks
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 31, 1000, 4097])
def test_batched_rows_equal_single_launches(dev, n, K):
    from mava_amd import ops

    out = torch.full((K, n), -1, dtype=torch.int32, device=dev)
    ops.permutation_batched(n, SEED, C0, out)
    for k in range(K):
        assert torch.equal(out[k], ops.permutation(n, SEED, C0 + k)), f"row {k}"
    if K > 1 and n > 31:
        assert not torch.equal(out[0], out[1])


def test_batched_rows_equal_the_oracle(dev):
    from mava_amd import ops
    from oracle import permutation as operm

    n, K = 4097, 4
    out = torch.empty((K, n), dtype=torch.int32, device=dev)
    ops.permutation_batched(n, SEED, C0, out)
    got = out.cpu().numpy()
    for k in range(K):
        assert np.array_equal(got[k], operm.permutation(n, SEED, C0 + k)), f"row {k}"


def test_batched_argument_errors(dev):
    from mava_amd._lib import lib

    assert lib().mava_permutation_batched_i32(8, 1, 0, 0, None, 8, None) <= -1000
    assert lib().mava_permutation_batched_i32(8, 1, 0, 17, None, 8, None) <= -1000
    assert lib().mava_permutation_batched_i32(8, 1, 0, 2, None, 7, None) <= -1000
    assert lib().mava_permutation_batched_i32(8, 1, 0, 2, None, 8, None) <= -1000 and b"null pointer" in lib().mava_last_error()
