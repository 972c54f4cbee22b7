"""GPU: mava_mat_sample_f32 and mava_mat_loss_f32 (csrc/mat.hip), each on its own through the C ABI, against the float64 cases of
tests/mat_kernel_model.py on the same float32 inputs.  Shapes (its case tables): a second sampler block with idle threads, 900 loss
rows of 928 in four waves over one, two and five blocks (the fifth without rows), up to 64 actions, one agent, samples that
straddle tiles, an idx that is no identity, rows with one legal action and rows with none.
Tolerances (conftest.assert_close): 1e-5 log-probs and losses (losses with scale = 1), 1e-4 gradients (after dividing by
grad_scale), bit-exact where two launches must agree.  Every output buffer holds a sentinel before the call and is followed by a
sentinel-filled guard that must survive; T32 inputs carry 7.0 on their padding rows."""
import numpy as np
import pytest
import torch

from tests import mat_kernel_model as mk
from tests import seq_model as sm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

SENT = 12345.0


def _lib():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return check, lib(), ptr, stream_ptr


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u8(a, dev):
    return _d(np.asarray(a).astype(np.uint8), dev)


def _t32(a, rows, dev):
    """(r, N) float32 numpy -> T32 (rows x N) on the device; the padding rows hold 7.0: they must not leak."""
    full = np.full((rows, a.shape[1]), 7.0, np.float32)
    full[: a.shape[0]] = a
    return _d(sm.to_t32(full), dev)


def _out(n, dev, dtype=torch.float32, guard=64):
    return torch.full((int(n) + guard,), SENT, device=dev).to(dtype)


def _take(t, n, what):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert (a[n:] == np.asarray(SENT).astype(a.dtype)).all(), f"{what}: wrote past its {n} elements"
    return a[:n]


def _bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def _sample(dev, c, greedy, mask=True):
    """One launch per agent into sentinel-filled outputs; every launch must leave the other agents' rows and the rows past
    B * A as they were, bit for bit.  Returns the agents' rows put together."""
    check, L, ptr, sp = _lib()
    B, A, n, rows = c["B"], c["A"], c["n"], c["rows"]
    pad = mk.c32(rows)
    y_d, mask_d = _t32(c["logits"], pad, dev), (_u8(c["mask"], dev) if mask else None)
    act, lp = np.empty(rows, np.int32), np.empty(rows, np.float32)
    sent_i, sent_f = np.int32(SENT), np.float32(SENT).view(np.uint32)
    for agent in range(A):
        a_d, lp_d = _out(pad, dev, torch.int32), _out(pad, dev)
        check(L.mava_mat_sample_f32(B, A, agent, n, ptr(y_d), ptr(mask_d), sm.SEED, c["step"], c["row_offset"], greedy, ptr(a_d), ptr(lp_d), sp()),
              "mat sample")
        a_, lp_ = _take(a_d, pad, "action"), _take(lp_d, pad, "log_prob")
        own = np.zeros(pad, bool)
        own[agent:rows:A] = True
        assert (a_[~own] == sent_i).all(), f"agent {agent}: action written outside rows b * A + {agent}"
        assert (lp_[~own].view(np.uint32) == sent_f).all(), f"agent {agent}: log_prob written outside rows b * A + {agent}"
        act[agent::A], lp[agent::A] = a_[own], lp_[own]
    return act, lp


@pytest.mark.parametrize("row_offset", mk.ROW_OFFSETS)
@pytest.mark.parametrize("shape", mk.MAT_SAMPLE_SHAPES, ids=lambda s: f"B{s[0]}xA{s[1]}")
@pytest.mark.parametrize("n", mk.MAT_N)
def test_mat_sample(dev, n, shape, row_offset):
    """Sampled actions equal the float64 Gumbel arg-max on philox.policy_uniforms at row id row_offset + b * A + agent wherever the
    two best float64 scores lie further apart than a gap.  The gap is measured: the float32 NumPy evaluation of the scores differs
    from float64 by at most 8.6e-07 on these inputs (mat_kernel_model.mat_sample_case, f32_diff; largest at n = 64), the gap is four
    times the case's own figure.  No row of any case is that close (tests/test_mat_kernel_model.py holds the share under 1 %).
    The mask is (B, A, n) row-major with different flags for the agents of a sample: read at b, or where a T32 matrix would keep
    it, it gives other actions (shown on the CPU in tests/test_mat_kernel_model.py)."""
    c = mk.mat_sample_case(n, *shape, row_offset)
    rows = c["rows"]
    r = np.arange(rows)
    flat = c["mask"].reshape(rows, n)
    none = np.zeros(rows, bool)
    none[c["all_masked"]] = True
    # greedy: the exact arg-max of the masked logits, lowest index on ties
    a, lp = _sample(dev, c, 1)
    assert np.array_equal(a, c["greedy"])
    assert_close(lp, c["logp"][r, a], 1e-5, "log_prob (greedy)")
    # sampled
    a, lp = _sample(dev, c, 0)
    decided = (c["gap"] > 4.0 * c["f32_diff"]) | none
    assert (~decided).mean() <= 0.01
    assert np.array_equal(a[decided], c["sampled"][decided])
    assert ((a >= 0) & (a < n)).all() and flat[r, a][~none].all(), "a masked action is never returned"
    assert_close(lp, c["logp"][r, a], 1e-5, "log_prob of the kernel's own action")
    if none.any():  # a row without a legal action: action 0, log_prob = -log(n_actions)
        assert (a[none] == 0).all()
        assert_close(lp[none], np.full(int(none.sum()), -np.log(n)), 1e-5, "log_prob of a row without a legal action")
    # without a mask
    a, lp = _sample(dev, c, 1, mask=False)
    assert np.array_equal(a, sm.greedy_discrete(c["logits"], None))
    assert_close(lp, sm.log_probs(c["logits"], None)[r, a], 1e-5, "log_prob (no mask)")


@pytest.mark.parametrize("n", [1, 2, 5, 17])
def test_mat_sample_equals_seq_sample(dev, n):
    """include/mava_hip.h: the sampler draws "exactly as mava_seq_sample_f32 does for row b * A + agent".  Both kernels evaluate the
    same float32 expression on the same Philox words, so the actions agree on every row, near-ties included."""
    check, L, ptr, sp = _lib()
    for row_offset in mk.ROW_OFFSETS:
        c = mk.mat_sample_case(n, 300, 3, row_offset)
        rows, pad = c["rows"], mk.c32(c["rows"])
        y_d = _t32(c["logits"], pad, dev)
        mask = np.ones((pad, n), np.uint8)
        mask[:rows] = c["mask"].reshape(rows, n)
        mask_d = _d(mask, dev)
        for greedy in (0, 1):
            a_d, lp_d = _out(pad, dev, torch.int32), _out(pad, dev)
            check(L.mava_seq_sample_f32(pad, n, ptr(y_d), ptr(mask_d), sm.SEED, c["step"], row_offset, greedy, ptr(a_d), ptr(lp_d), sp()),
                  "seq sample")
            a_seq, lp_seq = _take(a_d, pad, "action")[:rows], _take(lp_d, pad, "log_prob")[:rows]
            a_mat, lp_mat = _sample(dev, c, greedy)
            assert np.array_equal(a_mat, a_seq), f"greedy={greedy} row_offset={row_offset}: rows {np.flatnonzero(a_mat != a_seq)[:8].tolist()}"
            assert float(np.abs(lp_mat.astype(np.float64) - lp_seq.astype(np.float64)).max()) <= 1e-6


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(dev, c):
    d = {k: _d(c[k], dev) for k in ("idx", "action", "old_lp", "adv", "old_value", "target", "stats")}
    d["logits"] = _t32(c["logits"], c["rows"], dev)
    d["values"] = _t32(c["values"][:, None], c["rows"], dev)
    d["mask"] = None if c["mask"] is None else _u8(c["mask"], dev)
    return d


def _loss(dev, c, d, gscale, nb, stats=None):
    """-> dlogits (rows, n), dvalues (rows,), partials (nb, 3), padding rows included."""
    check, L, ptr, sp = _lib()
    n, rows = c["n"], c["rows"]
    st = d["stats"] if stats is None else stats
    dy, dv, part = _out(rows * n, dev), _out(rows, dev), _out(3 * nb, dev)
    check(L.mava_mat_loss_f32(c["Bm"], c["A"], n, rows, ptr(d["idx"]), ptr(d["logits"]), ptr(d["values"]), ptr(d["mask"]), ptr(d["action"]),
                              ptr(d["old_lp"]), ptr(d["adv"]), ptr(d["old_value"]), ptr(d["target"]), ptr(st), st.shape[0], sm.CLIP,
                              sm.ENT_COEF, sm.VF_COEF, gscale, ptr(dy), ptr(dv), ptr(part), nb, sp()), "mat loss")
    return (sm.from_t32(_take(dy, rows * n, "dlogits"), rows, n), _take(dv, rows, "dvalues"),
            _take(part, 3 * nb, "loss partials").reshape(nb, 3))


def _check_loss(dev, c, stats=None, gscales=mk.GRAD_SCALES):
    R, rows = c["R"], c["rows"]
    d = _loss_inputs(dev, c)
    want = np.array([c["actor_loss"], c["entropy"], c["value_loss"]])
    for gscale in gscales:
        ref = None
        for nb in mk.N_BLOCKS:
            dy, dv, part = _loss(dev, c, d, gscale, nb, stats)
            assert_close(part.astype(np.float64).sum(0), want, 1e-5, f"actor loss | entropy | value loss, {nb} blocks", scale=1.0)
            idle = np.arange(nb) * 256 >= rows
            assert (part[idle] == 0.0).all(), "a block without rows writes zero partials"
            if c["actor_loss"] == 0.0:
                assert (part[:, 0] == 0.0).all(), "actor_loss is exactly 0"
            if ref is None:
                ref = (dy, dv)
            _bits(dy, ref[0], f"dlogits, {nb} blocks")
            _bits(dv, ref[1], f"dvalues, {nb} blocks")
        dy, dv = ref
        assert_close(dy[:R] / gscale, c["dlogits"], 1e-4, f"dlogits (grad_scale {gscale})")
        assert_close(dv[:R] / gscale, c["dvalues"], 1e-4, f"dvalues (grad_scale {gscale})")
        assert (dy[R:] == 0.0).all() and (dv[R:] == 0.0).all(), "padding rows are exact zero"
        if c["mask_rows"] is not None:
            assert (dy[:R][~c["mask_rows"]] == 0.0).all(), "an illegal action receives exactly 0"
        for r in c["all_masked"]:
            assert (dy[r] == 0.0).all(), "a row without a legal action: no gradient into its logits"
    return dy, dv, part


@pytest.mark.parametrize("shape", mk.MAT_LOSS_SHAPES, ids=lambda s: f"Bm{s[0]}xA{s[1]}")
@pytest.mark.parametrize("n", mk.MAT_N)
def test_mat_loss(dev, n, shape):
    """Logits at 33 to 64 actions have no earlier test here.  The float32 NumPy evaluation of the gradient formulas lies at most
    8.8e-07 (relative, assert_close's form) from float64 on these inputs (mat_kernel_model.loss_f32_error, re-measured by
    tests/test_mat_kernel_model.py; largest at n = 64, 900 rows): four times that is inside the project's 1e-4, which is kept."""
    c = mk.mat_loss_case(n, *shape)
    assert len(c["one_legal"]) == 2 and len(c["all_masked"]) == (2 if n >= 5 else 0)
    _check_loss(dev, c)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
def test_mat_loss_constant_advantages(dev, masked):
    """Variance 0: the normalised advantages are exactly 0, the surrogate vanishes, only the entropy term reaches dlogits, and
    dvalues is that of the same values under varying advantages."""
    c = mk.mat_loss_case(9, 300, 3, True, masked)
    assert c["actor_loss"] == 0.0
    dy, dv, _ = _check_loss(dev, c)
    _, ent, dz = sm.actor_loss(c["logits"], c["mask_rows"], c["action_rows"], c["old_lp_rows"], np.zeros(c["R"]))
    assert_close(dy[: c["R"]] / mk.GRAD_SCALES[-1], dz, 1e-4, "dlogits = the entropy term alone")
    other = mk.mat_loss_case(9, 300, 3, False, masked)
    assert np.array_equal(other["values"], c["values"])
    _, dv_other, _ = _loss(dev, other, _loss_inputs(dev, other), mk.GRAD_SCALES[-1], 1)
    _bits(dv, dv_other, "dvalues under constant and under varying advantages")


def test_mat_loss_reads_the_rows_adv_stats_summed(dev):
    """The statistics come from the library's own ops.adv_stats on (advantages, idx, Bm, A): both kernels must mean idx[b] * A + j.
    The samples the minibatch leaves out carry advantages of 1e3, so sums over other rows move the mean by more than 10."""
    from mava_amd import ops

    c = mk.mat_loss_case(5, 300, 3, left_out_adv=1e3)
    stats = ops.adv_stats(_d(c["adv"], dev).view(-1), _d(c["idx"], dev), 0, c["Bm"], c["A"])
    got = stats.double().cpu().numpy().sum(0)
    assert_close(got, c["stats"].sum(0), 1e-6, "sum | sum of squares of the minibatch advantages")
    _check_loss(dev, c, stats=stats)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_launch_nothing(dev):
    check, L, ptr, sp = _lib()
    c = mk.mat_loss_case(5, 5, 3)
    d = _loss_inputs(dev, c)
    dy, dv, part = _out(64 * 65, dev), _out(64, dev), _out(3, dev)
    y64 = torch.zeros(64 * 65, device=dev)

    def loss(Bm=5, A=3, n=5, rows=32, idx=d["idx"], nb=1):
        return L.mava_mat_loss_f32(Bm, A, n, rows, ptr(idx), ptr(y64), ptr(d["values"]), ptr(d["mask"]), ptr(d["action"]), ptr(d["old_lp"]),
                                   ptr(d["adv"]), ptr(d["old_value"]), ptr(d["target"]), ptr(d["stats"]), 3, sm.CLIP, sm.ENT_COEF,
                                   sm.VF_COEF, 1.0, ptr(dy), ptr(dv), ptr(part), nb, sp())

    assert loss(n=65) <= -1000
    assert loss(Bm=11) <= -1000  # 33 agent rows in 32
    assert loss(rows=48) <= -1000
    assert loss(nb=0) <= -1000
    assert loss(idx=None) <= -1000
    act = _out(32, dev, torch.int32)
    assert L.mava_mat_sample_f32(5, 3, 3, 5, ptr(y64), ptr(d["mask"]), sm.SEED, 0, 0, 0, ptr(act), ptr(dv), sp()) <= -1000
    torch.cuda.synchronize()
    for t in (dy, dv, part):
        assert float(t.min()) == SENT and float(t.max()) == SENT
    assert int(act.min()) == int(SENT) and int(act.max()) == int(SENT)
