"""TEST INFRASTRUCTURE: plain restatements of the layer kernels of csrc/generic_layers.hip (NumPy / torch float64, no GPU
and no project kernel), for tests/test_generic_layers_model.py (which checks them against torch's conv2d / layer_norm and
oracle/rec_oracle.py) and tests/test_gpu_generic_layers.py (which checks the kernels against them).

T32 (rec_dense.hip): element (row, f) of a (rows x N) matrix at ((row / 32) * N + f) * 32 + row % 32.
flax 'SAME' (nn.Conv): out = ceil(in / stride), pad_total = max((out - 1) * stride + k - in, 0), pad_low = pad_total // 2
(the odd pixel goes to the HIGH end).  flax LayerNorm: last axis, epsilon 1e-6, no scale, learned bias.
"""
from __future__ import annotations

import numpy as np
import torch

LN_EPS = 1e-6

# (H, W, C, k, stride, asymmetric): the convolution geometries both test files walk
GEOMETRIES = [
    (4, 4, 2, 3, 2, True),    # total 1, low 0
    (5, 4, 3, 2, 1, True),    # even kernel: total 1 on both axes
    (6, 5, 1, 4, 2, True),    # C = 1; totals 2 (H) and 3 (W): asymmetric in W only
    (3, 3, 2, 5, 1, False),   # k > H
    (5, 7, 2, 1, 1, False),   # k = 1, no padding
    (5, 5, 2, 2, 3, False),   # stride > k: pixels no patch reads
    (7, 3, 4, 3, 3, False),   # Wout = 1
    (1, 1, 8, 3, 1, False),   # a single pixel
    (5, 5, 3, 3, 1, False),   # the shape the network tests use
]


# ---- T32 ------------------------------------------------------------------------------------------------------------
def to_t32(a):
    rows, N = a.shape
    assert rows % 32 == 0
    return np.ascontiguousarray(a.reshape(rows // 32, 32, N).transpose(0, 2, 1)).reshape(-1)


def from_t32(flat, rows, N):
    return np.ascontiguousarray(np.asarray(flat).reshape(rows // 32, N, 32).transpose(0, 2, 1)).reshape(rows, N)


# ---- convolution geometry ---------------------------------------------------------------------------------------------
def same_geo(H, W, k, stride):
    """(Hout, Wout, (total_h, total_w), (low_h, low_w)) of flax's 'SAME' padding."""
    Hout, Wout = -(-H // stride), -(-W // stride)
    th, tw = max((Hout - 1) * stride + k - H, 0), max((Wout - 1) * stride + k - W, 0)
    return Hout, Wout, (th, tw), (th // 2, tw // 2)


def im2col(x, k, stride, low=None):
    """x (S, H, W, C) -> (S * Hout * Wout, k * k * C), feature (ky * k + kx) * C + c; zeros outside the image.  Gather form.
    `low` overrides the low padding (for the test that the wrong split is visible)."""
    S, H, W, C = x.shape
    Hout, Wout, _, lo = same_geo(H, W, k, stride)
    lh, lw = lo if low is None else low
    out = np.zeros((S, Hout, Wout, k, k, C), x.dtype)
    for oy in range(Hout):
        for ox in range(Wout):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * stride + ky - lh, ox * stride + kx - lw
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, oy, ox, ky, kx] = x[:, iy, ix]
    return out.reshape(S * Hout * Wout, k * k * C)


def col2im(col, S, H, W, C, k, stride):
    """Adjoint of im2col in float64, SCATTER form: every patch entry is added into the pixel it was read from."""
    Hout, Wout, _, (lh, lw) = same_geo(H, W, k, stride)
    c6 = np.asarray(col, np.float64).reshape(S, Hout, Wout, k, k, C)
    img = np.zeros((S, H, W, C), np.float64)
    for oy in range(Hout):
        for ox in range(Wout):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * stride + ky - lh, ox * stride + kx - lw
                    if 0 <= iy < H and 0 <= ix < W:
                        img[:, iy, ix] += c6[:, oy, ox, ky, kx]
    return img


def read_count(S, H, W, C, k, stride):
    """How many patch entries read each pixel (0 = a pixel no patch reads)."""
    Hout, Wout, _, _ = same_geo(H, W, k, stride)
    return col2im(np.ones((S * Hout * Wout, k * k * C)), S, H, W, C, k, stride)


def image_matrix(x, src_flat):
    """The two layouts an image batch (S, H, W, C) has as a matrix: (S x H*W*C) when src_flat else (S*H*W x C)."""
    S, H, W, C = x.shape
    return x.reshape(S, H * W * C) if src_flat else x.reshape(S * H * W, C)


def flatten(a, P):
    """(samples * P x C) -> (samples x P * C), feature p * C + c."""
    rows, C = a.shape
    return a.reshape(rows // P, P * C)


def unflatten(a, P):
    S, PC = a.shape
    return a.reshape(S * P, PC // P)


# ---- LayerNorm + activation ---------------------------------------------------------------------------------------------
ACTS = {0: lambda v: v, 1: lambda v: np.maximum(v, 0.0), 2: np.tanh}
T_ACTS = {0: lambda v: v, 1: torch.relu, 2: torch.tanh}


def norm_act(x, bias, act, use_ln):
    """float64: (y, xhat, rstd); xhat / rstd are None without LayerNorm."""
    x = np.asarray(x, np.float64)
    if not use_ln:
        return ACTS[act](x), None, None
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(v + LN_EPS)
    xhat = (x - m) * rstd
    return ACTS[act](xhat + np.asarray(bias, np.float64)), xhat, rstd[:, 0]


def t_norm_act(x: torch.Tensor, bias, act, use_ln):
    if use_ln:
        m = x.mean(-1, keepdim=True)
        v = ((x - m) ** 2).mean(-1, keepdim=True)
        x = (x - m) / torch.sqrt(v + LN_EPS) + bias
    return T_ACTS[act](x)


def norm_act_grads(x, bias, act, use_ln, dy):
    """torch float64 autograd of sum(dy * y): (dz = gradient at the activation's input, dx)."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    # a zero "probe" added in front of the activation receives dz
    probe = torch.zeros_like(xt, requires_grad=True)
    h = xt
    if use_ln:
        m = h.mean(-1, keepdim=True)
        v = ((h - m) ** 2).mean(-1, keepdim=True)
        h = (h - m) / torch.sqrt(v + LN_EPS) + torch.tensor(np.asarray(bias, np.float64))
    y = T_ACTS[act](h + probe)
    (y * torch.tensor(np.asarray(dy, np.float64))).sum().backward()
    return probe.grad.numpy(), xt.grad.numpy()


def norm_f32_two_pass(x):
    """The kernel's formula restated in float32 NumPy, features summed in order: mean, then the centred sum of squares.
    Returns (xhat, rstd) in float32."""
    x = np.asarray(x, np.float32)
    N = x.shape[1]
    s = np.zeros(x.shape[0], np.float32)
    for f in range(N):
        s = s + x[:, f]
    mean = s / np.float32(N)
    v = np.zeros(x.shape[0], np.float32)
    for f in range(N):
        d = x[:, f] - mean
        v = d * d + v
    rstd = (np.float32(1.0) / np.sqrt(v / np.float32(N) + np.float32(LN_EPS))).astype(np.float32)
    return ((x - mean[:, None]) * rstd[:, None]).astype(np.float32), rstd


def rel_err(got, want):
    """The smallest rtol at which conftest.assert_close(got, want, rtol) passes."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.sqrt(np.mean(want * want)))
    return float((np.abs(got - want) / (np.abs(want) + scale)).max())


def ill_conditioned_rows(rows=32, N=256):
    """Rows of offset 100 and unit spread: the mean's rounding error (about 1e-5 of it) is an absolute shift of xhat."""
    rng = np.random.default_rng(2024)
    return (100.0 + rng.standard_normal((rows, N))).astype(np.float32)


def ill_conditioned_measure():
    """How far the float32 two-pass formula lies from float64 on ill_conditioned_rows(): (xhat, rstd) as rel_err."""
    x = ill_conditioned_rows()
    _, xhat, rstd = norm_act(x, np.zeros(x.shape[1]), 0, True)
    xh32, r32 = norm_f32_two_pass(x)
    return rel_err(xh32, xhat), rel_err(r32, rstd)


# max(ill_conditioned_measure()) as measured on the CPU: 5.48e-05 for xhat (1.24e-07 for rstd).  The GPU test allows 4x that
# for another summation order and rsqrtf; tests/test_generic_layers_model.py re-measures it.
ILL_MEASURED = 5.482e-05
ILL_RTOL = 4.0 * ILL_MEASURED


# ---- one GRU-cell step -------------------------------------------------------------------------------------------------
def step_done(done, idx, A, rows):
    """The flag of each T32 row: done (E * A) read at idx[row / A] * A + row % A (idx None: the identity)."""
    row = np.arange(rows)
    e, a = row // A, row % A
    env = e if idx is None else np.asarray(idx, np.int64)[e]
    return np.asarray(done).reshape(-1)[env * A + a] != 0


def gru_cell(gi: torch.Tensor, gh: torch.Tensor, bhn: torch.Tensor, hprev: torch.Tensor):
    """flax GRUCell on the products gi = x W_i + b_i, gh = h W_h (rows x 3 Hd, thirds r | z | n):
    r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r (gh_n + b_hn)), h' = (1 - z) n + z h.
    Returns (h', saved = [r | z | n | gh_n + b_hn])."""
    D = hprev.shape[1]
    r = torch.sigmoid(gi[:, :D] + gh[:, :D])
    z = torch.sigmoid(gi[:, D : 2 * D] + gh[:, D : 2 * D])
    hl = gh[:, 2 * D :] + bhn
    n = torch.tanh(gi[:, 2 * D :] + r * hl)
    return (1.0 - z) * n + z * hprev, torch.cat([r, z, n, hl], 1)


def gru_step(gi, gh, bhn, hprev, done_next=None):
    """NumPy in, float64 NumPy out: (hs, saved, hprev_next); hprev_next = 0 where the next step's flag is set."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    with torch.no_grad():
        hs, saved = gru_cell(t(gi), t(gh), t(bhn), t(hprev))
    hs, saved = hs.numpy(), saved.numpy()
    nxt = None if done_next is None else np.where(np.asarray(done_next, bool)[:, None], 0.0, hs)
    return hs, saved, nxt


def gru_step_grads(gi, gh, bhn, hprev, dh_out, carried=None, done_next=None):
    """torch float64 autograd of one cell step with gi, gh and hprev as independent leaves.  The gradient at h' is dh_out
    plus `carried` (what step t + 1 hands back) where done_next is not set.  Returns (dgi, dgh, dhp): dhp is the DIRECT
    path dh * z only, because gh is a leaf here (the path through h W_h is a matrix product outside the cell)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    lgi, lgh, lhp = (t(a).requires_grad_(True) for a in (gi, gh, hprev))
    hs, _ = gru_cell(lgi, lgh, t(bhn), lhp)
    dh = t(dh_out)
    if carried is not None:
        dh = dh + torch.where(torch.tensor(np.asarray(done_next, bool))[:, None], torch.zeros_like(dh), t(carried))
    (hs * dh).sum().backward()
    return lgi.grad.numpy(), lgh.grad.numpy(), lhp.grad.numpy()
