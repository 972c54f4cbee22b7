"""mava_clip_adam, mava_ppo_finish_f32 and the slab sums at the layouts the learners send them, beyond PPO's own sizes:
every Adam comparison is ONE step from an identical f32 state against oracle.ppo_oracle.clip_adam in float64 (b1, b2 as the
f32 values), every output buffer sits between sentinels, g must come back untouched and exactly n_seg counts move.  The case
tables, the references and the bounds are those of tests/test_tail_edges_model.py, which checks them on the CPU."""
import numpy as np
import pytest
import torch

from tests import test_tail_edges_model as tm
from tests.conftest import assert_close
from tests.test_gpu_tail import KW, LR_A, LR_C, _column_sums, _layout, _norm_from_partials, _oracle_step, _reduced, _slabs

pytestmark = pytest.mark.gpu

GUARD = 4  # sentinel floats on either side of a live range (a multiple of 4: the guard does not move the alignment)


def _guarded(x, off, dev):
    """x on the device, `off` floats behind a 16-byte aligned address, sentinels in front and behind: (buffer, view)."""
    x = np.ascontiguousarray(x, np.float32)
    buf = torch.full((GUARD + off + x.size + GUARD,), tm.SENTINEL, device=dev)
    view = buf[GUARD + off : GUARD + off + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return buf, view


def _sentinels_intact(buf, view, name):
    b = buf.cpu().numpy()
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    assert (b[:lo] == tm.SENTINEL).all(), f"{name}: written in front of the live range"
    assert (b[lo + view.numel() :] == tm.SENTINEL).all(), f"{name}: written behind the live range"


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _launch(dev, st, seg_off, lrs, counts, off=0, **kw):
    """One ops.clip_adam launch on copies of the state st = (p, g, m, v), each view `off` floats off 16-byte alignment.
    Returns the new (p, m, v); the sentinels, g and the counts are checked here."""
    from mava_amd import ops

    (pb, p), (gb, g), (mb, m), (vb, v) = (_guarded(x, off, dev) for x in st)
    g_before = gb.clone()
    n_seg = len(lrs)
    spare = [77, 78]  # counts behind the last segment's: not the launch's to touch
    count = torch.tensor(list(counts) + spare, dtype=torch.int32, device=dev)
    ops.clip_adam(p, g, m, v, count, list(seg_off), list(lrs), grad_scale=kw.pop("grad_scale", 1.0), max_norm=tm.MAX_NORM, **kw)
    torch.cuda.synchronize()
    for name, b, x in (("p", pb, p), ("m", mb, m), ("v", vb, v)):
        _sentinels_intact(b, x, name)
    assert torch.equal(gb.view(torch.int32), g_before.view(torch.int32)), "g was written"
    assert count.tolist() == [c + 1 for c in counts] + spare, f"counts of {n_seg} segments"
    return tuple(x.cpu().numpy() for x in (p, m, v))


def _launch_case(dev, case, st, off=0, **kw):
    return _launch(dev, st, case.seg_off, case.lrs, case.counts, off, **case.kwargs, **kw)


def _check_segments(got, want, case, what=""):
    """p / m / v against the float64 oracle, segment by segment (each network against its own rms)."""
    for k in range(len(case.lrs)):
        sl = slice(case.seg_off[k], case.seg_off[k + 1])
        for name, a, b in zip("pmv", got, want):
            tol = tm.P0_ZERO_TOL if (case.p0_zero and name == "p") else tm.ADAM_TOL
            assert_close(a[sl], b[sl], tol, f"{name} of segment {k} {what}")


# --------------------------------------------------------------------------------------------------------------- A.1
@tm.by_name(tm.SIZE_CASES)
def test_sizes_and_base_pointers(dev, case):
    """One segment of 1 .. 8197 parameters behind base pointers 0 .. 3 floats off 16-byte alignment (an unaligned g takes
    the scalar norm loop for the whole segment; sac_learner.py passes such slices), clip on and off.  With the clip on the
    moments start at zero: m = (1 - b1) g / n * c then shows the pre-clip norm n to f32 accuracy, read back here from the
    largest entry (three roundings - n, the quotient, the product - of 2^-24 each; the bound is 2^-22)."""
    st = case.state()
    want = case.reference(st)
    g64 = st[1].astype(np.float64)
    norm = float(np.sqrt((g64 * g64).sum()))
    i = int(np.argmax(np.abs(g64)))
    for off in tm.ADAM_OFFSETS:
        got = _launch_case(dev, case, st, off)
        _check_segments(got, want, case, f"at offset {off}")
        if case.clips(0):
            seen = (1 - tm.B1) * tm.MAX_NORM * g64[i] / float(got[1][i])
            assert abs(seen - norm) <= 2.0 ** -22 * norm, f"norm at offset {off}: m shows {seen!r}, float64 {norm!r}"


# --------------------------------------------------------------------------------------------------------------- A.2
@tm.by_name(tm.SEGMENT_CASES)
def test_segments(dev, case):
    """Up to eight segments, one of them empty, boundaries off multiples of 4 (the head / float4 / tail split of the norm
    loop), each with its own learning rate and count, the clip on in some and off in others.  Each segment against the
    oracle, and bit-equal to a launch of that segment alone at the same address modulo 16 bytes; alone at another alignment
    it must still be bit-equal where the clip is off (no norm enters the step).  (The norm is summed in double: between two
    orders it differs far below its f32 rounding, so the first of these holds whichever loop a launch takes.)"""
    st = case.state()
    got = _launch_case(dev, case, st)
    _check_segments(got, case.reference(st), case)
    for k in range(len(case.lrs)):
        lo, hi = case.seg_off[k], case.seg_off[k + 1]
        if hi == lo:
            continue
        sub = tuple(x[lo:hi] for x in st)
        for shift in (0, 1):
            alone = _launch(dev, sub, (0, hi - lo), (case.lrs[k],), (case.counts[k],), (lo + shift) % 4, **case.kwargs)
            if shift == 0 or not case.clips(k):
                for name, a, b in zip("pmv", got, alone):
                    assert np.array_equal(_bits(a[lo:hi]), _bits(b)), f"{name} of segment {k} against the segment alone, alignment shift {shift}"


# --------------------------------------------------------------------------------------------------------------- A.3
@tm.by_name(tm.CAPPED_CASES)
def test_capped_grid(dev, case):
    """More than 262 144 parameters: the grid stays at 256 blocks and the flat loop takes a second batch, with a segment
    boundary inside it.  With the clip off the parameters of the second batch are bit-equal to a launch on them alone."""
    st = case.state()
    got = _launch_case(dev, case, st)
    _check_segments(got, case.reference(st), case)
    if not case.clips(0) and case.total > tm.CAP:
        sub = tuple(x[tm.CAP :] for x in st)
        alone = _launch(dev, sub, (0, case.seg_off[1] - tm.CAP, case.total - tm.CAP), case.lrs, case.counts, **case.kwargs)
        for name, a, b in zip("pmv", got, alone):
            assert np.array_equal(_bits(a[tm.CAP :]), _bits(b)), f"{name} of the second batch against a launch of its own"


# --------------------------------------------------------------------------------------------------------------- A.4
@tm.by_name(tm.COUNT_CASES + tm.P0_ZERO_CASES)
def test_counts_and_schedule(dev, case):
    """Step counts up to 100 000 (1 - b^t), the decayed learning rate on both sides of the floor division and at the last
    update, eight segments with eight different counts (each coefficient lane on a value of its own); and the same from
    p0 = 0, where p IS the update: held to tm.P0_ZERO_TOL instead of disappearing in ulp(p)."""
    st = case.state()
    _check_segments(_launch_case(dev, case, st), case.reference(st), case)


# --------------------------------------------------------------------------------------------------------------- A.5
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
def test_clip_threshold(dev, side, off):
    """A gradient whose norm is max_norm (1 +- 2^-20), exactly, in float64 and in f32 (8 f32 ulps from max_norm: no rounding
    of the sum or of the root can change the side): the first step from zero moments is the clipped one above and the plain
    one below, which lie 2^-20 apart - m within 2^-22 of the right one."""
    g = tm.threshold_gradient(side)
    z = np.zeros(g.size, np.float32)
    _, m, _ = _launch(dev, (z, g, z, z), (0, g.size), (1e-3,), (0,), off)
    g64 = g.astype(np.float64)
    norm = tm.MAX_NORM * (1.0 + side * tm.THRESHOLD_EPS)
    assert float(np.sqrt((g64 * g64).sum())) == norm and abs(norm - tm.MAX_NORM) >= 4 * float(np.spacing(np.float32(tm.MAX_NORM)))
    plain, clipped = (1 - tm.B1) * g64, (1 - tm.B1) * (g64 / norm) * tm.MAX_NORM
    want, other = (clipped, plain) if side > 0 else (plain, clipped)
    err = np.abs(m - want).max() / want[0]
    assert err <= 2.0 ** -22, f"m is not the {'clipped' if side > 0 else 'plain'} step: off by {err:.3e}"
    assert np.abs(m - other).min() / other[0] >= 2.0 ** -21


# --------------------------------------------------------------------------------------------------------------- A.6
@pytest.mark.parametrize("metrics", [False, True], ids=["nometrics", "metrics"])
@pytest.mark.parametrize("n_seg", [1, 8])
def test_metrics(dev, n_seg, metrics):
    """Without metrics_out and loss_sums, and with both - loss_sums a view at an odd offset - for one segment and eight."""
    case = tm.METRICS_CASES[n_seg]
    assert len(case.lrs) == n_seg
    st = case.state()
    U_D = round(1 / tm.METRICS_GRAD_SCALE)
    loss = np.random.default_rng(n_seg).random(3).astype(np.float32)
    kw = {}
    if metrics:
        lb, lv = _guarded(loss, 1, dev)
        ob, ov = _guarded(np.zeros(4, np.float32), 1, dev)
        kw = dict(loss_sums=lv, metrics_out=ov, vf_coef=0.5, ent_coef=0.01)
    got = _launch_case(dev, case, st, grad_scale=tm.METRICS_GRAD_SCALE, **kw)
    p, g, m, v = st
    want = tm.adam_ref(p, g, m, v, case.counts, case.seg_off, case.lrs, grad_scale=tm.METRICS_GRAD_SCALE, **case.kwargs)
    _check_segments(got, want, case)
    if metrics:
        _sentinels_intact(lb, lv, "loss_sums")
        _sentinels_intact(ob, ov, "metrics_out")
        assert np.array_equal(lv.cpu().numpy(), loss)
        a, e, vl = (loss / U_D).tolist()
        assert_close(ov.cpu().numpy(), np.array([a - 0.01 * e + 0.5 * vl, vl, a, e]), 1e-6, "metrics")


# --------------------------------------------------------------------------------------------------------------- A.7
@pytest.mark.parametrize("big", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("name,mode,Pa,Pc,din_c", tm.FINISH_CASES, ids=[c[0] for c in tm.FINISH_CASES])
def test_fused_finish_beyond_ppo_sizes(dev, name, mode, Pa, Pc, din_c, big):
    """mava_ppo_finish_f32 where its grid is capped and its norm partials outnumber the 2048 a block preloads (the cases:
    tests/test_tail_edges_model.py FINISH_CASES).  Three consecutive launches on one workspace; after each, g and the norm
    partials bit-equal to the NumPy restatement, counts [k, k], p / m / v against the oracle and - clip off, or both
    launches' restated norms rounding to the same f32 - bit-equal to ops.clip_adam from the same state; where the launch
    packs, the re-split W1 through the next critic launch, as in test_adam_launch_and_w1_resplit."""
    from mava_amd import ops
    from mava_amd._lib import Ctx

    n_slab, grad_scale = tm.FINISH_SLABS, tm.FINISH_GRAD_SCALE
    scale = tm.FINISH_SCALES[big]  # clip active / inactive
    a, c = _slabs(din_c, n_slab, scale, Pa, Pc)
    assert (a.shape[1] - 2, c.shape[1] - 1) == (Pa, Pc)
    P = Pa + Pc
    g_want, partials = _reduced(din_c, n_slab, scale, grad_scale, Pa, Pc)
    n_partial = partials.shape[0]
    assert n_partial == (P + 3 + 63) // 64
    if name.startswith("partials"):
        assert n_partial == int(name[len("partials") :])
    else:
        assert P > tm.CAP and n_partial > 2048
    fused = [_norm_from_partials(partials[:, s]) for s in range(2)]
    gs = (g_want[:P] * np.float32(grad_scale)).astype(np.float32)
    flat = [tm.norm_flat(gs, 0, Pa), tm.norm_flat(gs, Pa, P)]
    assert all((np.float32(n) >= np.float32(KW["max_norm"])) == big for n in fused + flat), (fused, flat)
    same_norms = all(np.float32(x) == np.float32(y) for x, y in zip(fused, flat))
    branch = "clip off" if not big else f"clip on, restated norms {fused} (fused) / {flat} (flat): {'equal' if same_norms else 'different'} in f32"
    slab_a, slab_c = _layout(a, c, "padded", dev)
    rng = np.random.default_rng(Pa + Pc + 1)
    p_np = tm.finish_p0(Pa, Pc)
    m_np, v_np = np.zeros(P, np.float32), np.zeros(P, np.float32)
    cnt_np = np.zeros(2, np.int64)
    (pb, p2), (mb, m2), (vb, v2) = (_guarded(x, 0, dev) for x in (p_np, m_np, v_np))
    c2 = torch.zeros(2, dtype=torch.int32, device=dev)
    g2 = torch.full((P + 4,), tm.SENTINEL, device=dev)
    assert g2.data_ptr() % 16 == 0
    ws = ops.ppo_finish_workspace(Pa, Pc, dev)
    ctx = Ctx(mode)
    wide = mode == "f16x2" and 96 <= din_c <= 287
    assert wide == name.startswith("pack")
    TE, A, Rb = 64, 4, 64
    if wide:
        x = torch.from_numpy(rng.standard_normal((TE, din_c)).astype(np.float32)).to(dev)
        ov = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
        tg = torch.from_numpy(rng.standard_normal(TE * A).astype(np.float32)).to(dev)
    for step in range(3):
        p1, m1, v1, c1 = p2.clone(), m2.clone(), v2.clone(), c2.clone()
        met1, met2 = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
        ops.ppo_finish(ctx, slab_a, slab_c, Pa, Pc, g2, p2, m2, v2, c2, LR_A, LR_C, grad_scale=grad_scale, metrics_out=met2,
                       critic_din=din_c, workspace=ws, **KW)
        ops.clip_adam(p1, g2, m1, v1, c1, [0, Pa, P], [LR_A, LR_C], grad_scale=grad_scale, loss_sums=g2[P:], metrics_out=met1, **KW)
        torch.cuda.synchronize()
        got_g = g2.cpu().numpy()
        assert np.array_equal(_bits(got_g[: P + 3]), _bits(g_want)), f"column sums, step {step}"
        assert got_g[P + 3] == tm.SENTINEL, "the pad behind the loss sums is not written"
        got_partials = ws.cpu().numpy()[: 2 * n_partial].reshape(n_partial, 2)
        assert np.array_equal(got_partials.view(np.uint64), partials.view(np.uint64)), f"norm partials, step {step}"
        assert c2.tolist() == c1.tolist() == [step + 1, step + 1]
        assert torch.equal(met1, met2)
        for name_, b, x_ in (("p", pb, p2), ("m", mb, m2), ("v", vb, v2)):
            _sentinels_intact(b, x_, name_)
        p_np, m_np, v_np = _oracle_step(p_np, m_np, v_np, cnt_np, g_want[:P], Pa, grad_scale)
        cnt_np += 1
        for nm, got, flat_, want in (("p", p2, p1, p_np), ("m", m2, m1, m_np), ("v", v2, v1, v_np)):
            got_np = got.cpu().numpy()
            assert_close(got_np[:Pa], want[:Pa], tm.ADAM_TOL, f"actor {nm} after step {step}")
            assert_close(got_np[Pa:], want[Pa:], tm.ADAM_TOL, f"critic {nm} after step {step}")
            if not big or same_norms:
                assert torch.equal(got.view(torch.int32), flat_.view(torch.int32)), f"{nm} after step {step}: fused finish vs clip_adam ({branch})"
        # (the oracle continues from the kernel's own f32 state: each step is checked on its own)
        p_np, m_np, v_np = (t.cpu().numpy() for t in (p2, m2, v2))
        assert ctx.get(ctx.W1_SPLIT_FRESH) == (1 if wide else 0)
        if wide:
            outs = []
            for c_ in (ctx, Ctx(mode)):
                slab = torch.zeros((3, Pc + 2), device=dev)
                ops.ppo_critic_grad(p2[Pa:], x, A, ov, tg, None, 0, Rb, A, 0.2, 0.5, slab, ctx=c_)
                torch.cuda.synchronize()
                outs.append(slab.clone())
            assert ctx.get(ctx.W1_SPLIT_FRESH) == 0, "the fresh flag is one-shot"
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "critic gradient on the re-split W1"


# --------------------------------------------------------------------------------------------------------------- A.8
def _slab_case(n_slab, stride, seed, dev):
    slab = np.random.default_rng(seed).standard_normal((n_slab, stride)).astype(np.float32)
    d = torch.from_numpy(slab).to(dev)
    assert tuple(d.shape) == (n_slab, stride)
    return slab, d


def _destination(n, seed, dev):
    """n live floats and 4 more the launch may not touch, all with earlier content, between sentinels."""
    prev = np.random.default_rng(seed).standard_normal(n + 4).astype(np.float32)
    buf, view = _guarded(prev, 0, dev)
    return prev, buf, view


def _check_destination(prev, buf, view, n, sums, accumulate, what):
    _sentinels_intact(buf, view, what)
    got = view.cpu().numpy()
    want = (prev[:n] + sums) if accumulate else sums
    assert np.array_equal(_bits(got[:n]), _bits(want)), f"{what}: not the stated sum"
    assert np.array_equal(_bits(got[n:]), _bits(prev[n:])), f"{what}: written beyond n"


@pytest.mark.parametrize("n", tm.SLAB_WIDTHS)
@pytest.mark.parametrize("n_slab", tm.SLAB_COUNTS)
def test_slab_sums(dev, n_slab, n):
    """slab_reduce and slab_reduce_cols for fewer slabs than waves (0 .. 3), one per wave and one more, an eight-load group
    and one more, 37; n on either side of a block's 64 columns; row stride n, n + 3, and a column window (an unaligned base
    pointer) from column 1 and from column 65.  Bit-equal to the sums in the kernels' stated order, plus the f32 add of the
    earlier content when accumulating; no slab at all gives zeros (or leaves the destination as it was); nothing beyond n."""
    from mava_amd import ops

    for layout, stride, col0 in (("tight", n, 0), ("stride+3", n + 3, 0), ("window1", n + 70, 1), ("window65", n + 70, 65)):
        slab, d = _slab_case(n_slab, stride, 1000 * n_slab + n, dev)
        sums = _column_sums(slab[:, col0 : col0 + n])
        if n_slab == 0:
            assert not sums.any()
        for accumulate in (False, True):
            prev, buf, out = _destination(n, n + accumulate, dev)
            if layout.startswith("window"):
                ops.slab_reduce_cols(d, col0, n, out, accumulate=accumulate)
            else:
                ops.slab_reduce(d, n, out, accumulate=accumulate)
            torch.cuda.synchronize()
            _check_destination(prev, buf, out, n, sums, accumulate, f"{layout}, accumulate={accumulate}")


@pytest.mark.parametrize("n_main,n_tail", tm.SLAB2_SPLITS)
@pytest.mark.parametrize("n_slab", [0, 1, 3, 5, 9, 37])
def test_slab_sums_two_destinations(dev, n_slab, n_main, n_tail):
    """slab_reduce2 into separate tensors - rec_networks.py's (K * N, nb) use among the splits, and either part empty."""
    from mava_amd import ops

    for stride in (n_main + n_tail, n_main + n_tail + 3):
        slab, d = _slab_case(n_slab, stride, 77 * n_slab + n_main, dev)
        sums = _column_sums(slab[:, : n_main + n_tail])
        for accumulate in (False, True):
            pm, bm, om = _destination(n_main, 1, dev)
            pt, bt, ot = _destination(n_tail, 2, dev)
            ops.slab_reduce2(d, n_main, om, n_tail, ot, accumulate=accumulate)
            torch.cuda.synchronize()
            _check_destination(pm, bm, om, n_main, sums[:n_main], accumulate, f"main, stride {stride}, accumulate={accumulate}")
            _check_destination(pt, bt, ot, n_tail, sums[n_main:], accumulate, f"tail, stride {stride}, accumulate={accumulate}")
