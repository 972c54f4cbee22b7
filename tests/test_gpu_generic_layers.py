"""GPU: every kernel of csrc/generic_layers.hip on its own, through the C ABI, against the plain references of
tests/generic_layers_model.py (float64 on the same float32 inputs).  Shapes: odd sizes, more than one block (288 rows =
one full block of 256 and a ragged one), asymmetric 'SAME' padding, even kernels, k = 1, k > H, stride > k, C = 1, H != W.
Tolerances (conftest.assert_close): 1e-5 forward values, 1e-4 gradients, 1e-6 fixed-order sums, bit-exact copies.
Every output buffer is pre-filled with a sentinel and followed by guard elements that must survive."""
import numpy as np
import pytest
import torch

from tests import generic_layers_model as gm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

SENT, GUARD = 12345.0, 64
GEO_IDS = [f"{H}x{W}x{C}-k{k}-s{s}" for H, W, C, k, s, _ in gm.GEOMETRIES]


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out(n, dev):
    """n output elements holding the sentinel, and GUARD more that no kernel may touch."""
    return torch.full((int(n) + GUARD,), SENT, device=dev)


def _take(t, n, what):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert (a[n:] == np.float32(SENT)).all(), f"{what}: wrote past its {n} elements"
    return a[:n]


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


def _L():
    from mava_amd._lib import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr()


# ---- 1. im2col / col2im -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [32, 64])
@pytest.mark.parametrize("src_flat", [0, 1])
@pytest.mark.parametrize("geo", gm.GEOMETRIES, ids=GEO_IDS)
def test_im2col_col2im(dev, geo, src_flat, samples):
    L, check, ptr, s = _L()
    H, W, C, k, st, _ = geo
    S = samples
    rng = np.random.default_rng(21)
    Hout, Wout, _, _ = gm.same_geo(H, W, k, st)
    rows_out, KK = S * Hout * Wout, k * k * C
    x = rng.standard_normal((S, H, W, C)).astype(np.float32)
    m = gm.image_matrix(x, src_flat)
    src, dst = _d(gm.to_t32(m), dev), _out(rows_out * KK, dev)
    check(L.mava_t32_im2col_f32(ptr(src), src_flat, S, H, W, C, k, st, ptr(dst), s), "im2col")
    got = gm.from_t32(_take(dst, rows_out * KK, "im2col"), rows_out, KK)
    _bits(got, gm.im2col(x, k, st), "im2col")

    dcol = rng.standard_normal((rows_out, KK)).astype(np.float32)
    want = gm.image_matrix(gm.col2im(dcol, S, H, W, C, k, st), src_flat)
    unread = gm.image_matrix(gm.read_count(S, H, W, C, k, st), src_flat) == 0
    assert unread.any() == ((H, W, C, k, st) == (5, 5, 2, 2, 3))
    assert (want[unread] == 0.0).all()
    dc, dsrc = _d(gm.to_t32(dcol), dev), _out(m.size, dev)
    check(L.mava_t32_col2im_f32(ptr(dc), src_flat, S, H, W, C, k, st, ptr(dsrc), s), "col2im")
    got = gm.from_t32(_take(dsrc, m.size, "col2im"), *m.shape)
    assert_close(got, want, 1e-6, "col2im")
    assert (got[unread] == 0.0).all(), "col2im: a pixel no patch reads must receive 0"


# ---- 2. flatten ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [32, 96])
@pytest.mark.parametrize("P,C", [(1, 1), (6, 3), (25, 32)])
def test_flatten_both_directions(dev, P, C, samples):
    L, check, ptr, s = _L()
    a = np.random.default_rng(22).standard_normal((samples * P, C)).astype(np.float32)
    n = a.size
    src, flat, back = _d(gm.to_t32(a), dev), _out(n, dev), _out(n, dev)
    check(L.mava_t32_flatten_f32(ptr(src), samples, P, C, 1, ptr(flat), s), "flatten")
    _bits(gm.from_t32(_take(flat, n, "flatten"), samples, P * C), gm.flatten(a, P), "flatten")
    check(L.mava_t32_flatten_f32(ptr(flat), samples, P, C, 0, ptr(back), s), "unflatten")
    _bits(_take(back, n, "unflatten"), gm.to_t32(a), "round trip")
    # the inverse on its own, from an independent matrix
    b = np.random.default_rng(23).standard_normal((samples, P * C)).astype(np.float32)
    srcb, un = _d(gm.to_t32(b), dev), _out(n, dev)
    check(L.mava_t32_flatten_f32(ptr(srcb), samples, P, C, 0, ptr(un), s), "unflatten")
    _bits(gm.from_t32(_take(un, n, "unflatten"), samples * P, C), gm.unflatten(b, P), "unflatten")


# ---- 3. norm_act / norm_act_bwd -------------------------------------------------------------------------------------------
def _na_inputs(rows, N):
    """Rows of offset U[-2, 2] and spread U[0.5, 2]; a few constant rows whose N-fold sum is exact in float32."""
    rng = np.random.default_rng(31)
    x = (rng.uniform(-2, 2, (rows, 1)) + rng.uniform(0.5, 2, (rows, 1)) * rng.standard_normal((rows, N))).astype(np.float32)
    const = np.zeros(rows, bool)
    for r, v in ((3, 3.0), (17, -0.5), (rows - 1, 3.0)):
        x[r], const[r] = v, True
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    dy = rng.standard_normal((rows, N)).astype(np.float32)
    return x, const, bias, dy


def _close_split(got, want, const, tol, what):
    """Constant rows have 1 / sigma = 1000: compared apart, so that their magnitude does not widen the others' tolerance."""
    assert_close(got[~const], want[~const], tol, what)
    assert_close(got[const], want[const], tol, what + " (constant rows)")


def _norm_act(dev, x, bias, act, use_ln):
    L, check, ptr, s = _L()
    rows, N = x.shape
    xd, bd = _d(gm.to_t32(x), dev), _d(bias, dev)
    y, xhat, rstd = _out(rows * N, dev), _out(rows * N, dev), _out(rows, dev)
    check(L.mava_t32_norm_act_f32(ptr(xd), N, rows, int(use_ln), ptr(bd) if use_ln else None, act, ptr(y), ptr(xhat) if use_ln else None,
                                  ptr(rstd) if use_ln else None, s), "norm_act")
    y_, xh_, r_ = _take(y, rows * N, "y"), _take(xhat, rows * N, "xhat"), _take(rstd, rows, "rstd")
    if not use_ln:  # untouched
        assert (xh_ == np.float32(SENT)).all() and (r_ == np.float32(SENT)).all()
    return gm.from_t32(y_, rows, N), gm.from_t32(xh_, rows, N), r_


@pytest.mark.parametrize("use_ln", [0, 1], ids=["plain", "ln"])
@pytest.mark.parametrize("act", [0, 1, 2], ids=["id", "relu", "tanh"])
@pytest.mark.parametrize("rows,N", [(32, 1), (64, 13), (288, 96), (32, 512)])
def test_norm_act_forward_and_backward(dev, rows, N, act, use_ln):
    L, check, ptr, s = _L()
    x, const, bias, dy = _na_inputs(rows, N)
    y, xhat, rstd = _norm_act(dev, x, bias, act, use_ln)
    wy, wxhat, wrstd = gm.norm_act(x, bias, act, use_ln)
    _close_split(y, wy, const, 1e-5, "y")
    if use_ln:
        _close_split(xhat, wxhat, const, 1e-5, "xhat")
        _close_split(rstd, wrstd, const, 1e-5, "rstd")
        # a constant row: x - mean is exactly 0, so xhat is, and y = act(bias)
        assert (xhat[const] == 0.0).all()
        if act == 2:  # the device's own tanhf of the bias: the kernel without LayerNorm on rows that hold the bias
            act_bias = _norm_act(dev, np.tile(bias, (32, 1)), bias, 2, 0)[0][0]
        else:
            act_bias = gm.ACTS[act](bias)
        for r in np.flatnonzero(const):
            _bits(y[r], act_bias, f"y of constant row {r}")

    # backward, on the float32 roundings of the reference's forward values
    wdz, wdx = gm.norm_act_grads(x, bias, act, use_ln, dy)
    f32 = lambda a: np.asarray(a, np.float32)
    ins = [_d(gm.to_t32(dy), dev), _d(gm.to_t32(f32(wy)), dev)]
    if use_ln:
        ins += [_d(gm.to_t32(f32(wxhat)), dev), _d(f32(wrstd), dev)]
    dz, dx = _out(rows * N, dev), _out(rows * N, dev)
    check(L.mava_t32_norm_act_bwd_f32(ptr(ins[0]), ptr(ins[1]), N, rows, int(use_ln), ptr(ins[2]) if use_ln else None,
                                      ptr(ins[3]) if use_ln else None, act, ptr(dz), ptr(dx), s), "norm_act_bwd")
    dz_, dx_ = gm.from_t32(_take(dz, rows * N, "dz"), rows, N), gm.from_t32(_take(dx, rows * N, "dx"), rows, N)
    _close_split(dz_, wdz, const, 1e-4, "dz")
    _close_split(dx_, wdx, const, 1e-4, "dx")
    if not use_ln:
        _bits(dx_, dz_, "dx = dz without LayerNorm")
        # dx aliased to dz
        both = _out(rows * N, dev)
        check(L.mava_t32_norm_act_bwd_f32(ptr(ins[0]), ptr(ins[1]), N, rows, 0, None, None, act, ptr(both), ptr(both), s), "norm_act_bwd")
        _bits(gm.from_t32(_take(both, rows * N, "dz (aliased)"), rows, N), dz_, "dx aliased to dz")


def test_norm_act_ill_conditioned_rows(dev):
    """Offset 100, unit spread, N = 256: the rounding of the mean (about 1e-5 of it) shifts xhat by an absolute amount.
    Measured on the CPU (tests/generic_layers_model.py ill_conditioned_measure, re-measured by
    tests/test_generic_layers_model.py): a float32 NumPy restatement of the same two-pass formula lies 5.48e-05 from the
    float64 reference (xhat; 1.24e-07 for rstd).  Allowed: ILL_RTOL = 4 x 5.482e-05 = 2.19e-04, to cover another summation
    order and rsqrtf."""
    x = gm.ill_conditioned_rows()
    bias = (np.random.default_rng(32).standard_normal(x.shape[1]) * 0.5).astype(np.float32)
    y, xhat, rstd = _norm_act(dev, x, bias, 0, 1)
    wy, wxhat, wrstd = gm.norm_act(x, bias, 0, True)
    for got, want, name in ((y, wy, "y"), (xhat, wxhat, "xhat"), (rstd, wrstd, "rstd")):
        print(f"ill-conditioned {name}: rel_err {gm.rel_err(got, want):.3e} (allowed {gm.ILL_RTOL:.3e})")
        assert_close(got, want, gm.ILL_RTOL, name)  # measured 5.48e-05 on the CPU, x 4


# ---- 4. colsum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slab", [1, 3, 12])
@pytest.mark.parametrize("N", [1, 96, 300])
def test_colsum_slabs(dev, N, n_slab):
    L, check, ptr, s = _L()
    rows, scale, stride = 320, 1.0 / 64.0, N + 5
    ntiles = rows // 32
    y = np.random.default_rng(41).standard_normal((rows, N)).astype(np.float32)
    yd, slab = _d(gm.to_t32(y), dev), _out(n_slab * stride, dev)
    check(L.mava_t32_colsum_f32(ptr(yd), N, rows, scale, ptr(slab), stride, n_slab, s), "colsum")
    got = _take(slab, n_slab * stride, "colsum").reshape(n_slab, stride)
    assert (got[:, N:] == np.float32(SENT)).all(), "the columns between the slabs' rows must survive"
    y64 = y.astype(np.float64).reshape(ntiles, 32, N)
    want = np.zeros((n_slab, N))
    for b in range(n_slab):  # block b sums tiles b, b + n_slab, ...
        want[b] = scale * y64[b::n_slab].sum((0, 1))
    assert (got[ntiles:, :N] == 0.0).all(), "a block without tiles writes exact zeros"
    assert_close(got[:ntiles, :N], want[:ntiles], 1e-6, "slabs")
    assert_close(got[:, :N].astype(np.float64).sum(0), scale * y.astype(np.float64).sum(0), 1e-6, "column sums")


# ---- 5. the GRU cell's kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [False, True], ids=["identity", "idx"])
@pytest.mark.parametrize("rows", [96, 288])
@pytest.mark.parametrize("Hd", [1, 96, 160])
def test_gru_step_kernels(dev, Hd, rows, gathered):
    L, check, ptr, s = _L()
    A = 3
    rng = np.random.default_rng(51)
    E = 120 if gathered else rows // A
    idx = rng.permutation(E)[: rows // A].astype(np.int32) if gathered else None
    done, done_next = ((rng.random(E * A) < 0.3).astype(np.uint8) for _ in range(2))
    d_row, dn_row = gm.step_done(done, idx, A, rows), gm.step_done(done_next, idx, A, rows)
    for f in (d_row, dn_row):
        assert f.any() and not f.all()
    if gathered:
        assert not np.array_equal(d_row, done[:rows] != 0)  # the gather matters
    f32 = lambda a: np.asarray(a, np.float32)
    gi, gh = (f32(rng.standard_normal((rows, 3 * Hd))) for _ in range(2))
    bhn, h = f32(rng.standard_normal(Hd) * 0.5), f32(rng.standard_normal((rows, Hd)) * 0.5)
    idx_d, done_d, dnext_d = (None if idx is None else _d(idx, dev)), _d(done, dev), _d(done_next, dev)
    T = lambda a: _d(gm.to_t32(a), dev)
    n1, n3, n4 = rows * Hd, rows * 3 * Hd, rows * 4 * Hd

    # gru_mask
    h_d, hprev_d = T(h), _out(n1, dev)
    check(L.mava_t32_gru_mask_f32(ptr(h_d), ptr(done_d), ptr(idx_d), E, A, Hd, rows, ptr(hprev_d), s), "gru_mask")
    hprev = np.where(d_row[:, None], np.float32(0.0), h)
    _bits(gm.from_t32(_take(hprev_d, n1, "hprev"), rows, Hd), hprev, "gru_mask")

    # gru_gates with every output
    whs, wsaved, wnext = gm.gru_step(gi, gh, bhn, hprev, dn_row)
    gi_d, gh_d, bhn_d, hp_d = T(gi), T(gh), _d(bhn, dev), T(hprev)
    hs, saved, nxt = _out(n1, dev), _out(n4, dev), _out(n1, dev)
    check(L.mava_t32_gru_gates_f32(ptr(gi_d), ptr(gh_d), ptr(bhn_d), ptr(hp_d), Hd, rows, ptr(hs), ptr(saved), ptr(nxt), ptr(dnext_d),
                                   ptr(idx_d), E, A, s), "gru_gates")
    hs_ = gm.from_t32(_take(hs, n1, "hs"), rows, Hd)
    saved_ = gm.from_t32(_take(saved, n4, "saved"), rows, 4 * Hd)
    nxt_ = gm.from_t32(_take(nxt, n1, "hprev_next"), rows, Hd)
    assert_close(hs_, whs, 1e-5, "hs")
    for i, name in enumerate(("r", "z", "n", "gh_n + b_hn")):
        assert_close(saved_[:, i * Hd : (i + 1) * Hd], wsaved[:, i * Hd : (i + 1) * Hd], 1e-5, f"saved {name}")
    assert_close(nxt_, wnext, 1e-5, "hprev_next")
    _bits(nxt_, np.where(dn_row[:, None], np.float32(0.0), hs_), "hprev_next = the masked hs")
    # ... and without saved / hprev_next (the last step of an acting sequence)
    hs2 = _out(n1, dev)
    check(L.mava_t32_gru_gates_f32(ptr(gi_d), ptr(gh_d), ptr(bhn_d), ptr(hp_d), Hd, rows, ptr(hs2), None, None, None, ptr(idx_d), E, A, s),
          "gru_gates")
    _bits(gm.from_t32(_take(hs2, n1, "hs"), rows, Hd), hs_, "hs without the optional outputs")

    # gru_gates_bwd, on the float32 rounding of the reference's saved values
    dh_out, acc_next, dhp_next = (f32(rng.standard_normal((rows, Hd))) for _ in range(3))
    sv_d, dh_d, acc_d, dhpn_d = T(f32(wsaved)), T(dh_out), T(acc_next), T(dhp_next)
    carried = acc_next.astype(np.float64) + dhp_next
    for carry in (False, True):
        want = gm.gru_step_grads(gi, gh, bhn, hprev, dh_out, carried if carry else None, dn_row if carry else None)
        dgi, dgh, dhp = _out(n3, dev), _out(n3, dev), _out(n1, dev)
        check(L.mava_t32_gru_gates_bwd_f32(ptr(sv_d), ptr(hp_d), ptr(dh_d), ptr(acc_d) if carry else None, ptr(dhpn_d) if carry else None,
                                           ptr(dnext_d) if carry else None, ptr(idx_d), E, A, Hd, rows, ptr(dgi), ptr(dgh), ptr(dhp), s),
              "gru_gates_bwd")
        tag = "carried" if carry else "last step"
        for buf, n, w, name in ((dgi, 3 * Hd, want[0], "dgi"), (dgh, 3 * Hd, want[1], "dgh"), (dhp, Hd, want[2], "dhp")):
            got = gm.from_t32(_take(buf, rows * n, name), rows, n)
            assert_close(got, w, 1e-4, f"{name} ({tag})")
            for i in range(n // Hd):  # each third apart: a small one must not hide behind a large one
                assert_close(got[:, i * Hd : (i + 1) * Hd], w[:, i * Hd : (i + 1) * Hd], 1e-4, f"{name} part {i} ({tag})")
