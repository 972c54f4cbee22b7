"""GPU: the recurrent PPO path's scan, loss, sampling, conversion and fused output kernels (csrc/rec_gru.hip, rec_gru_h2.hip,
rec_out_h2.hip), each on its own through the C ABI, against the float64 references of tests/seq_model.py on the same float32
inputs.  Shapes (seq_model's case tables): more than one sequence tile (Rm = 96), gathered minibatches, per-agent reset flags,
every head width on both sides of 8 | 9 and 16 | 17, rows with one legal action and rows with none.
Tolerances (conftest.assert_close): 1e-5 forward values and losses (losses with scale = 1), 1e-4 gradients (after dividing by
grad_scale), bit-exact where two launches must agree.  Every output buffer holds a sentinel before the call and is followed by
one sentinel-filled guard tile that must survive."""
import numpy as np
import pytest
import torch

from oracle import tanh_normal as tn
from tests import seq_model as sm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

SENT = 12345.0
H = sm.H


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u8(a, dev):
    return _d(np.asarray(a).astype(np.uint8), dev)


def _out(n, width, dev, dtype=torch.float32):
    """n output elements holding the sentinel and one guard tile (32 x width) behind them."""
    return torch.full((int(n) + 32 * int(width),), SENT, device=dev).to(dtype)


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


def _L():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr()


@pytest.fixture(params=[0, 1], ids=["f32", "f16x2"])
def ctx(request):
    from mava_amd._lib import Ctx

    c = Ctx("f16x2" if request.param == 1 else "f32")
    yield c
    c.close()


# ---- 1. GRU scans ----------------------------------------------------------------------------------------------------------------
def _scan_fwd(dev, ctx, c, h0_t32, training=True):
    L, check, ptr, s = _L()
    T, Rm, E, A = c["T"], c["Rm"], c["E"], c["A"]
    n = T * Rm
    idx_d = None if c["idx"] is None else _d(c["idx"], dev)
    done_d, wh_d, bhn_d = _d(c["done"], dev), _d(c["Wh"], dev), _d(c["bhn"], dev)
    h0_d = _d(sm.to_t32(c["h0_rows"]) if h0_t32 else c["h0"], dev)
    gi_d = _d(sm.to_t32(c["gi"].reshape(n, 3 * H)), dev)
    hs, hprev, saved = _out(n * H, H, dev), _out(n * H, H, dev), _out(n * 4 * H, 4 * H, dev)
    check(L.mava_gru_scan_fwd_f32(ctx.handle, T, Rm, E, A, ptr(idx_d), ptr(done_d), ptr(h0_d), h0_t32, ptr(wh_d), ptr(bhn_d), ptr(gi_d),
                                  ptr(hs), ptr(hprev) if training else None, ptr(saved) if training else None, s), "scan fwd")
    hs_, hp_, sv_ = _take(hs, n * H, "hs"), _take(hprev, n * H, "hprev"), _take(saved, n * 4 * H, "saved")
    if not training:
        assert (hp_ == np.float32(SENT)).all() and (sv_ == np.float32(SENT)).all()
    return hs_, hp_, sv_


def _scan_bwd(dev, ctx, c, dh_out, n_only):
    """On the float32 roundings of the reference's saved values."""
    L, check, ptr, s = _L()
    T, Rm, E, A = c["T"], c["Rm"], c["E"], c["A"]
    n = T * Rm
    idx_d = None if c["idx"] is None else _d(c["idx"], dev)
    done_d, wh_d = _d(c["done"], dev), _d(c["Wh"], dev)
    sv_d = _d(sm.to_t32(sm.f32(c["saved"]).reshape(n, 4 * H)), dev)
    hp_d = _d(sm.to_t32(sm.f32(c["hprev"]).reshape(n, H)), dev)
    dh_d = _d(sm.to_t32(sm.f32(dh_out).reshape(n, H)), dev)
    gw = H if n_only else 3 * H
    dgi, dgh = _out(n * 3 * H, 3 * H, dev), _out(n * gw, gw, dev)
    check(L.mava_gru_scan_bwd_f32(ctx.handle, T, Rm, E, A, ptr(idx_d), ptr(done_d), ptr(wh_d), ptr(sv_d), ptr(hp_d), ptr(dh_d), ptr(dgi),
                                  ptr(dgh), n_only, s), "scan bwd")
    return (sm.from_t32(_take(dgi, n * 3 * H, "dgi"), n, 3 * H).reshape(T, Rm, 3 * H),
            sm.from_t32(_take(dgh, n * gw, "dgh"), n, gw).reshape(T, Rm, gw))


@pytest.mark.parametrize("done_kind", sm.SCAN_DONE)
@pytest.mark.parametrize("h0_t32", [0, 1])
@pytest.mark.parametrize("shape", sm.SCAN_SHAPES, ids=["Rm32", "Rm96-idx"])
@pytest.mark.parametrize("T", sm.SCAN_T)
def test_gru_scans(dev, ctx, T, shape, h0_t32, done_kind):
    E, A, Em, gathered = shape
    c = sm.scan_case(T, E, A, Em, gathered, done_kind)
    n = T * c["Rm"]
    hs, hprev, saved = _scan_fwd(dev, ctx, c, h0_t32)
    rows = lambda a, w: sm.from_t32(a, n, w).reshape(T, c["Rm"], w)
    assert_close(rows(hs, H), c["hs"], 1e-5, "hs")
    assert_close(rows(hprev, H), c["hprev"], 1e-5, "hprev")
    assert (rows(hprev, H)[c["done_rows"]] == 0.0).all(), "a reset sequence enters its step with exact zeros"
    sv = rows(saved, 4 * H)
    for i, name in enumerate(("r", "z", "n", "W_hn h + b_hn")):
        assert_close(sv[..., i * H : (i + 1) * H], c["saved"][..., i * H : (i + 1) * H], 1e-5, f"saved {name}")
    hs2, _, _ = _scan_fwd(dev, ctx, c, h0_t32, training=False)
    _bits(hs2, hs, "hs of the acting call (hprev and saved null)")

    dgi, dghn = _scan_bwd(dev, ctx, c, c["dh_out"], 1)
    dgi0, dgh = _scan_bwd(dev, ctx, c, c["dh_out"], 0)
    _bits(dgi0, dgi, "dgi of both dgh forms")
    _bits(dgh[..., : 2 * H], dgi[..., : 2 * H], "dgh's r and z thirds = dgi's")
    _bits(dgh[..., 2 * H :], dghn, "dgh's n third = the dgh_n_only output")
    for i, name in enumerate("rzn"):  # each third apart: a small one must not hide behind a large one
        assert_close(dgi[..., i * H : (i + 1) * H], c["dgi"][..., i * H : (i + 1) * H], 1e-4, f"dgi {name}")
        assert_close(dgh[..., i * H : (i + 1) * H], c["dgh"][..., i * H : (i + 1) * H], 1e-4, f"dgh {name}")


def test_reset_cuts_the_gradient_chain(dev, ctx):
    """Every sequence is reset entering step 3 of 5: dgi of steps 0..2 must not see dh_out of steps 3 and 4."""
    c = dict(sm.scan_case(5, 40, 3, 32, True, "none"))
    c["done"] = c["done"].copy()
    c["done"][3] = 1
    c["done_rows"] = sm.done_rows(c["done"], c["idx"], c["A"], c["Rm"])
    c["hs"], c["hprev"], c["saved"] = sm.gru_scan(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"])
    dh2 = c["dh_out"].copy()
    dh2[3:] = dh2[3:] * 3.0 + 1.0
    a, _ = _scan_bwd(dev, ctx, c, c["dh_out"], 1)
    b, _ = _scan_bwd(dev, ctx, c, dh2, 1)
    _bits(b[:3], a[:3], "dgi before the reset")
    assert (b[3:] != a[3:]).any()
    want, _ = sm.gru_scan_grads(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"], dh2)
    assert_close(b, want, 1e-4, "dgi")


# ---- 2. discrete actor loss ----------------------------------------------------------------------------------------------------------
def _actor_loss(dev, c, gscale, n_blocks):
    L, check, ptr, s = _L()
    T, Rm, E, A, n, R = c["T"], c["Rm"], c["E"], c["A"], c["n"], c["R"]
    stats = sm.adv_stats(c["adv_rows"])
    idx_d, y_d, act_d, olp_d, adv_d, st_d = (_d(a, dev) for a in (c["idx"], sm.to_t32(c["logits"]), c["action"], c["old_lp"], c["adv"], stats))
    mask_d = None if c["mask"] is None else _u8(c["mask"], dev)
    dy, part = _out(R * n, n, dev), _out(2 * n_blocks, 1, dev)
    check(L.mava_seq_actor_loss_f32(T, Rm, E, A, n, ptr(idx_d), ptr(y_d), ptr(mask_d), ptr(act_d), ptr(olp_d), ptr(adv_d), ptr(st_d),
                                    stats.shape[0], sm.CLIP, sm.ENT_COEF, gscale, ptr(dy), ptr(part), n_blocks, s), "actor loss")
    return sm.from_t32(_take(dy, R * n, "dlogits"), R, n), _take(part, 2 * n_blocks, "loss partials").reshape(n_blocks, 2)


def _check_actor(dev, c, gscale):
    ref = None
    for nb in sm.N_BLOCKS:
        dy, part = _actor_loss(dev, c, gscale, nb)
        assert (part[1:] == 0.0).all(), "192 rows fit the first block: every other block writes zero partials"
        assert_close(part.sum(0), np.array([c["loss"], c["entropy"]]), 1e-5, f"loss / entropy, {nb} blocks", scale=1.0)
        if ref is None:
            ref = dy
        _bits(dy, ref, f"dlogits, {nb} blocks")
    assert_close(ref / gscale, c["dlogits"], 1e-4, "dlogits")
    if c["mask_rows"] is not None:
        assert (ref[~c["mask_rows"]] == 0.0).all(), "an illegal action receives exactly 0"
    for r in c["all_masked"]:
        assert (ref[r] == 0.0).all(), "a row without a legal action: no gradient into its logits"
    return ref


@pytest.mark.parametrize("gscale", sm.GRAD_SCALES)
@pytest.mark.parametrize("n", sm.ACTOR_N)
def test_seq_actor_loss(dev, n, gscale):
    c = sm.actor_case(n)
    assert len(c["one_legal"]) == 2 and len(c["all_masked"]) == (2 if n in sm.ALL_MASKED_N else 0)
    _check_actor(dev, c, gscale)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
def test_seq_actor_loss_constant_advantages(dev, masked):
    """Variance 0: the normalised advantages are exactly 0, the surrogate vanishes, the entropy term remains."""
    c = sm.actor_case(9, constant_adv=True, masked=masked)
    assert c["loss"] == 0.0
    _check_actor(dev, c, 256.0)


# ---- 3. critic loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", sm.GRAD_SCALES)
@pytest.mark.parametrize("na", sm.CRITIC_AGENTS)
def test_seq_critic_loss(dev, na, gscale):
    L, check, ptr, s = _L()
    c = sm.critic_case(na)
    T, Rm, E, A, R = c["T"], c["Rm"], c["E"], c["A"], c["R"]
    idx_d, v_d, ov_d, tg_d = (_d(a, dev) for a in (c["idx"], sm.to_t32(c["v"][:, None]), c["old_v"], c["tgt"]))
    ref = None
    for nb in sm.N_BLOCKS:
        dv, part = _out(R, 1, dev), _out(2 * nb, 1, dev)
        check(L.mava_seq_critic_loss_f32(T, Rm, E, A, na, ptr(idx_d), ptr(v_d), ptr(ov_d), ptr(tg_d), sm.CLIP, sm.VF_COEF, gscale, ptr(dv),
                                         ptr(part), nb, s), "critic loss")
        dv_, part_ = _take(dv, R, "dvalues"), _take(part, 2 * nb, "loss partials").reshape(nb, 2)
        assert (part_[1:] == 0.0).all() and (part_[:, 1] == 0.0).all()
        assert_close(part_[:, 0].sum(), c["loss"], 1e-5, f"value loss, {nb} blocks", scale=1.0)
        if ref is None:
            ref = dv_
        _bits(dv_, ref, f"dvalues, {nb} blocks")
    assert_close(ref / gscale, c["dv"], 1e-4, "dvalues")


# ---- 4. continuous loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset", sm.ROW_OFFSETS)
@pytest.mark.parametrize("per_row", [False, True], ids=["log_std", "log_std_rows"])
@pytest.mark.parametrize("dim", sm.CONT_DIMS)
def test_seq_continuous_loss(dev, dim, per_row, row_offset):
    """The float32 NumPy evaluation of the reference lies at most 4.2e-05 (relative, assert_close's form) from float64 on these
    inputs (seq_model.cont_f32_error, re-measured by tests/test_seq_model.py): inside the project's 1e-4, which is kept."""
    L, check, ptr, s = _L()
    c = sm.cont_case(dim, per_row, row_offset)
    T, Rm, E, A, R = c["T"], c["Rm"], c["E"], c["A"], c["R"]
    gscale, nb = 256.0, 2
    stats = sm.adv_stats(c["adv_rows"])
    idx_d, m_d, act_d, olp_d, adv_d, st_d = (_d(a, dev) for a in (c["idx"], sm.to_t32(c["mean"]), c["action"], c["old_lp"], c["adv"], stats))
    raw_d = _d(sm.to_t32(c["raw"]) if per_row else c["raw"], dev)
    dmean, drows, part, dsp = _out(R * dim, dim, dev), _out(R * dim, dim, dev), _out(2 * nb, 1, dev), _out(nb * dim, 1, dev)
    check(L.mava_seq_actor_loss_continuous_f32(T, Rm, E, A, dim, tn.MIN_SCALE, ptr(idx_d), ptr(m_d), None if per_row else ptr(raw_d),
                                               ptr(raw_d) if per_row else None, ptr(act_d), ptr(olp_d), ptr(adv_d), ptr(st_d), stats.shape[0],
                                               sm.CLIP, sm.ENT_COEF, sm.SEED, c["ent_step"], row_offset, gscale, ptr(dmean),
                                               ptr(drows) if per_row else None, ptr(part), ptr(dsp), nb, s), "continuous loss")
    part_ = _take(part, 2 * nb, "loss partials").reshape(nb, 2)
    assert_close(part_.sum(0), np.array([c["loss"], c["entropy"]]), 1e-5, "loss / entropy", scale=1.0)
    assert_close(sm.from_t32(_take(dmean, R * dim, "dmean"), R, dim) / gscale, c["dmean"], 1e-4, "dmean")
    dsp_, drows_ = _take(dsp, nb * dim, "dscale partials"), _take(drows, R * dim, "dlog_std_rows")
    if per_row:
        assert (dsp_ == np.float32(SENT)).all(), "no log_std vector: its partials stay untouched"
        assert_close(sm.from_t32(drows_, R, dim) / gscale, c["draw"], 1e-4, "dlog_std_rows")
    else:
        assert (drows_ == np.float32(SENT)).all()
        assert (dsp_.reshape(nb, dim)[1:] == 0.0).all()
        assert_close(dsp_.reshape(nb, dim).astype(np.float64).sum(0), c["draw"], 1e-4, "dlog_std (summed over blocks)")


# ---- 5. discrete sampling ----------------------------------------------------------------------------------------------------------------
def _sample(dev, c, greedy, mask=True):
    L, check, ptr, s = _L()
    rows, n = c["rows"], c["n"]
    y_d, mask_d = _d(sm.to_t32(c["logits"]), dev), (_u8(c["mask"], dev) if mask else None)
    act, lp = _out(rows, 1, dev, torch.int32), _out(rows, 1, dev)
    check(L.mava_seq_sample_f32(rows, n, ptr(y_d), ptr(mask_d), sm.SEED, c["step"], c["row_offset"], greedy, ptr(act), ptr(lp), s), "sample")
    return _take(act, rows, "action"), _take(lp, rows, "log_prob")


@pytest.mark.parametrize("row_offset", sm.ROW_OFFSETS)
@pytest.mark.parametrize("rows", sm.SAMPLE_ROWS)
@pytest.mark.parametrize("n", sm.SAMPLE_N)
def test_seq_sample(dev, n, rows, row_offset):
    """Sampled actions equal the float64 Gumbel arg-max on philox.policy_uniforms wherever the two best float64 scores lie further
    apart than a gap.  The gap is measured: the float32 NumPy evaluation of the scores z - log(-log(u)) differs from float64 by at
    most 6.35e-07 on these inputs (seq_model.sample_case, f32_diff; largest at n = 32, rows = 288), the gap is four times the
    case's own figure (at most 2.54e-06).  No row of any case is that close (tests/test_seq_model.py holds the share under 1 %).
    Rows without a legal action tie exactly at finfo.min: the first index wins, in the reference as in the kernel."""
    c = sm.sample_case(n, rows, row_offset)
    r = np.arange(rows)
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
    assert ((a >= 0) & (a < n)).all() and c["mask"][r, a][~none].all(), "a masked action is never returned"
    assert_close(lp, c["logp"][r, a], 1e-5, "log_prob of the kernel's own action")
    if none.any():  # a row without a legal action: log_prob = -log(n_actions), whatever the action
        assert np.allclose(c["logp"][none], -np.log(n), rtol=0, atol=1e-12) and (a[none] == 0).all()
    # without a mask
    a, lp = _sample(dev, c, 1, mask=False)
    assert np.array_equal(a, sm.greedy_discrete(c["logits"], None))
    assert_close(lp, sm.log_probs(c["logits"], None)[r, a], 1e-5, "log_prob (no mask)")


# ---- 6. continuous sampling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [False, True], ids=["log_std", "log_std_rows"])
@pytest.mark.parametrize("dim", sm.CONT_DIMS)
def test_seq_sample_continuous(dev, dim, per_row):
    L, check, ptr, s = _L()
    rows, step, off = 288, 5, 1000
    rng = np.random.default_rng(7000 + dim)
    mean = sm.f32(rng.standard_normal((rows, dim)) * 0.5)
    raw = sm.f32(rng.standard_normal((rows, dim) if per_row else dim) * 0.5)
    scale = np.broadcast_to(tn.scale_of(sm.f64(raw)), mean.shape)
    m_d, raw_d = _d(sm.to_t32(mean), dev), _d(sm.to_t32(raw) if per_row else raw, dev)
    for greedy in (1, 0):
        act, lp = _out(rows * dim, dim, dev), _out(rows, 1, dev)
        check(L.mava_seq_sample_continuous_f32(rows, dim, tn.MIN_SCALE, ptr(m_d), None if per_row else ptr(raw_d), ptr(raw_d) if per_row else None,
                                               sm.SEED, step, off, greedy, ptr(act), ptr(lp), s), "sample continuous")
        a, lp_ = _take(act, rows * dim, "action").reshape(rows, dim), _take(lp, rows, "log_prob")
        eps = 0.0 if greedy else tn.normal_noise(sm.SEED, step, rows, dim, tn.STREAM_SAMPLE, off)
        assert_close(a, np.tanh(sm.f64(mean) + scale * eps), 1e-5, "tanh(mean)" if greedy else "action")
        want = tn.log_prob_terms(sm.f64(a), sm.f64(mean), scale)[0].sum(-1)  # of the kernel's own action
        assert_close(lp_, want, 1e-5, "log_prob")


# ---- 7. T32 conversion -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 32, 96])
@pytest.mark.parametrize("N", [1, 13, 128])
def test_t32_convert_round_trip(dev, N, rows):
    L, check, ptr, s = _L()
    a = sm.f32(np.random.default_rng(N + rows).standard_normal((rows, N)))
    src, t32, back = _d(a.reshape(-1) if rows else np.zeros(1, np.float32), dev), _out(rows * N, N, dev), _out(rows * N, N, dev)
    check(L.mava_t32_convert_f32(ptr(src), N, rows, 1, ptr(t32), s), "rows -> T32")
    got = _take(t32, rows * N, "T32")
    check(L.mava_t32_convert_f32(ptr(t32), N, rows, 0, ptr(back), s), "T32 -> rows")
    got_back = _take(back, rows * N, "rows")
    if rows:
        _bits(got, sm.to_t32(a), "rows -> T32")
        _bits(got_back, a.reshape(-1), "round trip")


# ---- 8. fused output path --------------------------------------------------------------------------------------------------------------------
def _rec_out(dev, c, is_actor, n_out, na, n_slab, masked=True):
    """Returns (rc, dh rows, slabs (n_slab, needed)); the 8 floats between the slabs and the guard tiles are checked here."""
    L, check, ptr, s = _L()
    T, Rm, E, A, R = c["T"], c["Rm"], c["E"], c["A"], c["R"]
    need = H * H + H + H * n_out + n_out + 2
    stride = need + 8
    gscale = 256.0
    idx_d, hs_d = _d(c["idx"], dev), _d(sm.to_t32(c["hs"]), dev)
    par_d = _d(c["flat"], dev)
    if is_actor:
        stats = sm.adv_stats(c["adv_rows"])
        mask_d, act_d, f0_d, f1_d, st_d = (_u8(c["mask"], dev) if masked else None), _d(c["action"], dev), _d(c["old_lp"], dev), _d(c["adv"], dev), _d(stats, dev)
        n_stats, coef = stats.shape[0], sm.ENT_COEF
    else:
        mask_d = act_d = st_d = None
        f0_d, f1_d, n_stats, coef = _d(c["old_v"], dev), _d(c["tgt"], dev), 0, sm.VF_COEF
    dh, slab = _out(R * H, H, dev), _out(n_slab * stride, 1, dev)
    rc = L.mava_rec_out_f32(T, Rm, E, A, n_out, na, ptr(idx_d), ptr(hs_d), ptr(par_d), ptr(mask_d), ptr(act_d), ptr(f0_d), ptr(f1_d), ptr(st_d),
                            n_stats, sm.CLIP, coef, gscale, int(is_actor), ptr(dh), ptr(slab), stride, n_slab, s)
    dh_ = _take(dh, R * H, "dh")
    slab_ = _take(slab, n_slab * stride, "slab").reshape(n_slab, stride)
    assert (slab_[:, need:] == np.float32(SENT)).all(), "the tail of every slab row must stay untouched"
    return rc, dh_, slab_[:, :need], gscale


def _check_out(dev, c, is_actor, n_out, na):
    c = dict(c, flat=sm.out_flat(c["params"]))
    g, R = c["grads"], c["R"]
    for n_slab in sm.OUT_SLABS:
        rc, dh, slab, gscale = _rec_out(dev, c, is_actor, n_out, na, n_slab)
        assert rc == 0 and sm.rec_out_instance(is_actor, n_out, n_slab, R // 32) is not None
        tot = slab.astype(np.float64).sum(0)
        dh = sm.from_t32(dh, R, H)
        assert_close(dh / gscale, g["dh"], 1e-4, f"dh ({n_slab} slabs)")
        o = 0
        for name, shape in (("dWpost", (H, H)), ("dbpost", (H,)), ("dWhead", (H, n_out)), ("dbhead", (n_out,))):
            k = int(np.prod(shape))
            assert_close(tot[o : o + k].reshape(shape), g[name], 1e-4, f"{name} ({n_slab} slabs)")
            o += k
        assert_close(tot[o : o + 2], np.array(c["losses"], np.float64), 1e-5, f"loss sums ({n_slab} slabs)", scale=1.0)
    return dh


@pytest.mark.parametrize("n_out", sm.OUT_N)
def test_rec_out_actor(dev, n_out):
    c = sm.out_case(True, n_out)
    assert len(c["all_masked"]) == (2 if n_out in sm.ALL_MASKED_N else 0)
    _check_out(dev, c, True, n_out, 1)


@pytest.mark.parametrize("n_out", sm.OUT_N)
def test_rec_out_actor_without_mask(dev, n_out):
    c = dict(sm.out_case(True, n_out))
    c["mask"], c["mask_rows"] = None, None

    def loss_fn(y):
        la, ent, dy = sm.actor_loss(y, None, c["action_rows"], c["old_lp_rows"], c["adv_rows"])
        return (la, ent), dy

    c["losses"], c["grads"] = sm.out_path(c["hs"], c["params"], loss_fn)
    c["flat"] = sm.out_flat(c["params"])
    rc, dh, slab, gscale = _rec_out(dev, c, True, n_out, 1, 4, masked=False)
    assert rc == 0
    assert_close(sm.from_t32(dh, c["R"], H) / gscale, c["grads"]["dh"], 1e-4, "dh")
    tot = slab.astype(np.float64).sum(0)
    assert_close(tot[: H * H].reshape(H, H), c["grads"]["dWpost"], 1e-4, "dWpost")
    assert_close(tot[H * H + H : H * H + H + H * n_out].reshape(H, n_out), c["grads"]["dWhead"], 1e-4, "dWhead")
    assert_close(tot[-2:], np.array(c["losses"], np.float64), 1e-5, "loss sums", scale=1.0)


@pytest.mark.parametrize("na", sm.CRITIC_AGENTS)
def test_rec_out_critic(dev, na):
    _check_out(dev, sm.out_case(False, 1, na), False, 1, na)


@pytest.mark.parametrize("is_actor,n_out,n_slab", sm.OUT_REFUSED, ids=["actor-17", "critic-2", "7-slabs"])
def test_rec_out_refusals(dev, is_actor, n_out, n_slab):
    """Returns 1 (the caller runs the layer-wise kernels) and touches neither dh nor the slabs."""
    assert sm.rec_out_instance(is_actor, n_out, n_slab, 6) is None
    c = dict(sm.actor_case(n_out) if is_actor else sm.critic_case(1))
    rng = np.random.default_rng(n_out)
    c["hs"], c["flat"] = sm.f32(rng.standard_normal((c["R"], H))), sm.out_flat(sm.out_params(rng, n_out))
    rc, dh, slab, _ = _rec_out(dev, c, is_actor, n_out, 1, n_slab)
    assert rc == 1
    assert (dh == np.float32(SENT)).all() and (slab == np.float32(SENT)).all()
