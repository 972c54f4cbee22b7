"""mava_gae_f32 at its time, column and flag edges against oracle.ppo_oracle.gae in float64, for both systems' masking
(feed-forward: done[t]; recurrent: done[t + 1], last_done behind the last row).  The default instantiation cuts time into
slabs of 8 chunks of 16 steps and the columns into strips of 64 (of 32 from N = 2048); T % 16 == 0 takes the branch-free
kernel, anything else the ragged one.  Outputs go into the first T rows of pre-filled (T + 1, N) buffers: a store beyond T
shows.  The case tables are those of tests/test_tail_edges_model.py."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests import test_tail_edges_model as tm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

MASKING = pytest.mark.parametrize("rec", [False, True], ids=["ff", "rec"])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, inputs, rec, gamma=0.99, lam=0.95):
    from mava_amd import ops

    r, v, d, lv, ld = inputs
    T, N = r.shape
    bufs = [torch.full((T + 1, N), tm.SENTINEL, device=dev) for _ in range(2)]
    adv, tgt = (b[:T] for b in bufs)
    ops.gae(_t(r, dev), _t(v, dev), _t(d, dev), _t(lv, dev), gamma, lam, last_done=_t(ld, dev) if rec else None, out=(adv, tgt))
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[T] == tm.SENTINEL).all(), "a store behind row T - 1"
    return adv.cpu().numpy(), tgt.cpu().numpy()


def _want(inputs, rec, gamma=0.99, lam=0.95):
    r, v, d, lv, ld = inputs
    return po.gae(r, v, d, lv, gamma, lam, last_done=ld if rec else None)


def _check(got, want, what):
    assert_close(got[0], want[0], tm.GAE_TOL, f"adv {what}")
    assert_close(got[1], want[1], tm.GAE_TOL, f"tgt {what}")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------- B.1
@MASKING
@pytest.mark.parametrize("N", tm.GAE_WIDTHS)
@pytest.mark.parametrize("T", tm.GAE_TIMES)
def test_time_edges(dev, T, N, rec):
    """T below, on and above a chunk (16) and a slab (128), up to three slabs, on the fast path (T % 16 == 0: 16, 112, 128,
    144, 256, 272) and on the ragged one; in the recurrent form last_done and the shifted mask cross the slab carry."""
    inputs = tm.time_edge_inputs(T, N)
    _check(_run(dev, inputs, rec), _want(inputs, rec), f"T={T} N={N}")


# --------------------------------------------------------------------------------------------------------------- B.2
@MASKING
@pytest.mark.parametrize("N", tm.GAE_COLS)
@pytest.mark.parametrize("T", tm.GAE_COL_TIMES)
def test_column_edges(dev, T, N, rec):
    """N on both sides of the strip permutation (number of strips a multiple of 8 or not) for both strip widths.  Against
    float64, and 16 columns - the first, the last, both sides of the strip boundaries next to either end - bit-equal to
    the same column computed alone in an N = 1 launch: the instantiations on either side of N = 2048 share chunk length and
    count, and a column's arithmetic does not depend on the strip it sits in."""
    inputs = tm.column_edge_inputs(T, N)
    got = _run(dev, inputs, rec)
    _check(got, _want(inputs, rec), f"T={T} N={N}")
    for j in tm.probe_columns(N):
        a1, t1 = _run(dev, tm.gae_column(inputs, j), rec)
        assert np.array_equal(_bits(got[0][:, j]), _bits(a1[:, 0])), f"adv column {j} of {N} against the column alone"
        assert np.array_equal(_bits(got[1][:, j]), _bits(t1[:, 0])), f"tgt column {j} of {N} against the column alone"


# --------------------------------------------------------------------------------------------------------------- B.3
@pytest.mark.parametrize("masking", tm.GAE_DONE_MASKINGS)
@pytest.mark.parametrize("pattern", tm.GAE_DONE_PATTERNS)
def test_done_placement(dev, pattern, masking):
    """Flags exactly on the last row of a chunk / slab and on the first row of the next (15, 16, 127, 128, 255, 256) and
    on the last row (299); everywhere; nowhere.  Where the mask of row t is set the scan restarts: adv[t] == r[t] - v[t]
    exactly (feed-forward: done[t]; recurrent: done[t + 1], last_done for the last row)."""
    rec = masking != "ff"
    inputs = tm.done_placement_inputs(pattern, masking)
    r, v, d, lv, ld = inputs
    got = _run(dev, inputs, rec)
    _check(got, _want(inputs, rec), f"{pattern}, {masking}")
    mask = np.concatenate([d[1:], ld[None]], 0) if rec else d
    assert mask.any() or pattern == "none"
    assert np.array_equal(got[0][mask], (r - v)[mask]), "adv == r - v where the scan restarts"
    if pattern == "all" and not rec:
        assert np.array_equal(got[0], r - v)
        assert_close(got[1], r.astype(np.float64), 1e-6, "targets all-done")


# --------------------------------------------------------------------------------------------------------------- B.4
@MASKING
@pytest.mark.parametrize("T", tm.GAE_COEF_TIMES)
@pytest.mark.parametrize("gamma,lam", tm.GAE_COEFS)
def test_coefficients(dev, gamma, lam, T, rec):
    """gamma = lambda = 1, and either or both at 0.  With gamma * lambda = 0 nothing flows between rows: adv[t] is
    delta[t], and a change of row k's reward (k the first row of the last chunk: 16, or of the last slab: 256) leaves the
    bits of every earlier row alone."""
    inputs = tm.coefficient_inputs(T)
    got = _run(dev, inputs, rec, gamma, lam)
    _check(got, _want(inputs, rec, gamma, lam), f"gamma={gamma} lambda={lam}")
    if gamma * lam == 0.0:
        r, v, d, lv, ld = inputs
        mask = np.concatenate([d[1:], ld[None]], 0) if rec else d
        nxt = np.concatenate([v[1:], lv[None]], 0).astype(np.float64)
        delta = r.astype(np.float64) + gamma * nxt * (1.0 - mask) - v.astype(np.float64)
        assert_close(got[0], delta, tm.GAE_TOL, "adv == delta")
        k = 16 if T == 17 else 256
        r2 = r.copy()
        r2[k] += 1.0
        got2 = _run(dev, (r2, v, d, lv, ld), rec, gamma, lam)
        for a, b in zip(got, got2):
            assert np.array_equal(_bits(a[:k]), _bits(b[:k])), "rows before the changed one moved"
            assert np.array_equal(_bits(a[k + 1 :]), _bits(b[k + 1 :]))
            assert not np.array_equal(a[k], b[k])
