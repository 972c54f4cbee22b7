"""CPU: the references of tests/generic_layers_model.py against independent implementations (torch's conv2d through
oracle/generic_oracle.py, torch.nn.functional.layer_norm, oracle/rec_oracle.py's GRU step), and the soundness of the
inputs tests/test_gpu_generic_layers.py is built on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import generic_oracle as go
from oracle import rec_oracle as ro
from tests import generic_layers_model as gm

GEO_IDS = [f"{H}x{W}x{C}-k{k}-s{s}" for H, W, C, k, s, _ in gm.GEOMETRIES]


def test_t32_round_trip_and_layout():
    a = np.arange(64 * 5, dtype=np.float32).reshape(64, 5)
    flat = gm.to_t32(a)
    for row, f in ((0, 0), (31, 4), (32, 0), (45, 3), (63, 4)):
        assert flat[((row // 32) * 5 + f) * 32 + row % 32] == a[row, f]
    assert np.array_equal(gm.from_t32(flat, 64, 5), a)


def test_same_geo_values():
    assert gm.same_geo(4, 4, 3, 2) == (2, 2, (1, 1), (0, 0))
    assert gm.same_geo(5, 4, 2, 1) == (5, 4, (1, 1), (0, 0))
    assert gm.same_geo(6, 5, 4, 2) == (3, 3, (2, 3), (1, 1))
    assert gm.same_geo(3, 3, 5, 1) == (3, 3, (4, 4), (2, 2))
    assert gm.same_geo(5, 7, 1, 1) == (5, 7, (0, 0), (0, 0))
    assert gm.same_geo(5, 5, 2, 3) == (2, 2, (0, 0), (0, 0))
    assert gm.same_geo(7, 3, 3, 3) == (3, 1, (2, 0), (1, 0))
    assert gm.same_geo(1, 1, 3, 1) == (1, 1, (2, 2), (1, 1))
    for H, W, C, k, s, asym in gm.GEOMETRIES:
        _, _, tot, _ = gm.same_geo(H, W, k, s)
        assert asym == bool(tot[0] % 2 or tot[1] % 2), (H, W, k, s)


@pytest.mark.parametrize("geo", gm.GEOMETRIES, ids=GEO_IDS)
def test_im2col_product_is_the_convolution(geo):
    """relu(im2col(x) @ W + b) against torch's conv2d with flax's 'SAME' padding (generic_oracle.forward)."""
    H, W, C, k, s, _ = geo
    rng = np.random.default_rng(11)
    S, co = 4, 5
    x = rng.standard_normal((S, H, W, C))
    spec = go.spec_cnn((H, W, C), [co], [k], [s], [], "relu", False)
    flat = rng.standard_normal(go.param_count(spec))
    w, b = flat[: k * k * C * co].reshape(k * k * C, co), flat[k * k * C * co :]
    Hout, Wout, _, _ = gm.same_geo(H, W, k, s)
    mine = np.maximum(gm.im2col(x, k, s) @ w + b, 0.0).reshape(S, Hout * Wout * co)
    with torch.no_grad():
        want = go.forward(torch.tensor(flat), spec, torch.tensor(x.reshape(S, -1)), features=True).numpy()
    assert mine.shape == want.shape
    assert np.abs(mine - want).max() < 1e-12


@pytest.mark.parametrize("geo", gm.GEOMETRIES, ids=GEO_IDS)
def test_col2im_is_the_adjoint_of_im2col(geo):
    H, W, C, k, s, _ = geo
    rng = np.random.default_rng(12)
    S = 4
    x = rng.standard_normal((S, H, W, C))
    col = gm.im2col(x, k, s)
    c = rng.standard_normal(col.shape)
    assert abs((col * c).sum() - (x * gm.col2im(c, S, H, W, C, k, s)).sum()) < 1e-10


def test_gap_geometry_has_unread_pixels():
    n = gm.read_count(4, 5, 5, 2, 2, 3)
    assert int((n == 0).sum()) == 72
    c = np.random.default_rng(0).standard_normal((4 * 4, 2 * 2 * 2))
    assert (gm.col2im(c, 4, 5, 5, 2, 2, 3)[n == 0] == 0.0).all()


@pytest.mark.parametrize("geo", [g for g in gm.GEOMETRIES if g[5]], ids=[i for i, g in zip(GEO_IDS, gm.GEOMETRIES) if g[5]])
def test_wrong_padding_split_is_visible(geo):
    """The extra pixel at the LOW end (the classic error) gives another im2col: the asymmetric cases can catch it."""
    H, W, C, k, s, _ = geo
    x = np.random.default_rng(13).standard_normal((4, H, W, C))
    _, _, tot, lo = gm.same_geo(H, W, k, s)
    wrong = (tot[0] - lo[0], tot[1] - lo[1])
    assert wrong != lo
    assert not np.array_equal(gm.im2col(x, k, s), gm.im2col(x, k, s, low=wrong))


def test_flatten_is_a_reshape_of_the_image():
    x = np.random.default_rng(14).standard_normal((32, 2, 3, 4))
    a = gm.image_matrix(x, 0)
    assert np.array_equal(gm.flatten(a, 6), gm.image_matrix(x, 1))
    assert np.array_equal(gm.unflatten(gm.flatten(a, 6), 6), a)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_layer_norm_reference(act):
    rng = np.random.default_rng(15)
    x, bias = rng.standard_normal((40, 13)) * 1.5 + 0.7, rng.standard_normal(13)
    y, xhat, rstd = gm.norm_act(x, bias, act, True)
    ln = F.layer_norm(torch.tensor(x), (13,), None, torch.tensor(bias), 1e-6)
    assert np.abs(y - gm.T_ACTS[act](ln).numpy()).max() < 1e-12
    assert np.abs(xhat + bias - ln.numpy()).max() < 1e-12
    assert np.abs(rstd - 1.0 / np.sqrt(x.var(-1) + 1e-6)).max() < 1e-12
    # the autograd helper: dz is the gradient in front of the activation, dx the gradient at the input
    dy = rng.standard_normal(x.shape)
    dz, dx = gm.norm_act_grads(x, bias, act, True, dy)
    xt = torch.tensor(x, requires_grad=True)
    (gm.T_ACTS[act](F.layer_norm(xt, (13,), None, torch.tensor(bias), 1e-6)) * torch.tensor(dy)).sum().backward()
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-12
    deriv = {0: np.ones_like(y), 1: (y > 0).astype(np.float64), 2: 1.0 - y * y}[act]
    assert np.abs(dz - dy * deriv).max() < 1e-12
    # without LayerNorm the gradient at the input is dz
    dz0, dx0 = gm.norm_act_grads(x, bias, act, False, dy)
    assert np.array_equal(dz0, dx0)


def test_gru_reference_matches_rec_oracle():
    rng = np.random.default_rng(16)
    R, D = 24, ro.H
    p = {"Wi": rng.standard_normal((D, 3 * D)) / np.sqrt(D), "bi": rng.standard_normal(3 * D) * 0.1,
         "Wh": rng.standard_normal((D, 3 * D)) / np.sqrt(D), "bhn": rng.standard_normal(D) * 0.1}
    x, h = rng.standard_normal((R, D)), rng.standard_normal((R, D)) * 0.5
    done_next = rng.random(R) < 0.3
    hs, saved, nxt = gm.gru_step(x @ p["Wi"] + p["bi"], h @ p["Wh"], p["bhn"], h, done_next)
    want = ro.gru_step(p, x, h)
    assert np.abs(hs - want).max() < 1e-12
    assert (nxt[done_next] == 0.0).all() and np.array_equal(nxt[~done_next], hs[~done_next])
    r, z, n, hl = (saved[:, i * D : (i + 1) * D] for i in range(4))
    assert np.abs((1.0 - z) * n + z * h - want).max() < 1e-12
    assert np.abs(n - np.tanh((x @ p["Wi"] + p["bi"])[:, 2 * D :] + r * hl)).max() < 1e-12


def test_gru_grads_are_the_cell_derivative():
    """dgi, dgh, dhp of the autograd helper against the closed form of the kernel's comment, and the carried gradient's cut."""
    rng = np.random.default_rng(17)
    R, D = 12, 5
    gi, gh = rng.standard_normal((R, 3 * D)), rng.standard_normal((R, 3 * D))
    bhn, hp = rng.standard_normal(D), rng.standard_normal((R, D))
    dh_out, carried = rng.standard_normal((R, D)), rng.standard_normal((R, D))
    done_next = rng.random(R) < 0.4
    assert done_next.any() and not done_next.all()
    _, saved, _ = gm.gru_step(gi, gh, bhn, hp)
    r, z, n, hl = (saved[:, i * D : (i + 1) * D] for i in range(4))
    for car in (None, carried):
        dgi, dgh, dhp = gm.gru_step_grads(gi, gh, bhn, hp, dh_out, car, done_next if car is not None else None)
        dh = dh_out if car is None else dh_out + np.where(done_next[:, None], 0.0, carried)
        dn_pre = dh * (1.0 - z) * (1.0 - n * n)
        want_gi = np.concatenate([dn_pre * hl * r * (1.0 - r), dh * (hp - n) * z * (1.0 - z), dn_pre], 1)
        want_gh = np.concatenate([want_gi[:, : 2 * D], dn_pre * r], 1)
        assert np.abs(dgi - want_gi).max() < 1e-12 and np.abs(dgh - want_gh).max() < 1e-12
        assert np.abs(dhp - dh * z).max() < 1e-12


def test_step_done_gathers_through_idx():
    rng = np.random.default_rng(18)
    E, A = 120, 3
    done = (rng.random(E * A) < 0.3).astype(np.uint8)
    idx = rng.permutation(E)[:32].astype(np.int32)
    got = gm.step_done(done, idx, A, 96)
    for row in (0, 1, 2, 3, 50, 95):
        assert got[row] == bool(done[idx[row // A] * A + row % A])
    assert np.array_equal(gm.step_done(done, None, A, 96), done[:96] != 0)


def test_ill_conditioned_tolerance_is_four_times_the_measured_error():
    """tests/test_gpu_generic_layers.py allows 4x what float32 arithmetic itself loses on the offset-100 rows."""
    xh, r = gm.ill_conditioned_measure()
    assert max(xh, r) == pytest.approx(gm.ILL_MEASURED, rel=1e-3)
    assert gm.ILL_RTOL == 4.0 * gm.ILL_MEASURED
    assert 1e-5 < gm.ILL_MEASURED < 1e-3  # above the well-conditioned 1e-5 (hence its own bound), still a float32-rounding figure
