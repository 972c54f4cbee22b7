"""float64 restatement of ff_mat with a ContinuousActionHead (mava_amd/mat_learner.py with MATNet(..., continuous=True),
csrc/mat.hip's mava_transformer_*_f32 kernels, csrc/mat_act.hip's continuous instance) in plain torch.

The encoder, attention, the loss on the network's outputs (loss_terms) and GAE are tests/mat_model.py's; the distribution is
oracle/tanh_normal.py's Independent(TanhTransformed(Normal(mean, softplus(log_std) + min_scale))), restated here in torch so
that autograd reaches the means and log_std (tests/test_mat_continuous_model.py holds the two against each other).  The decoder
differs from the discrete one in its input (the previous agents' action vectors, no start token, act_dense with a bias), its
head (d means) and the log_std leaf.  Parameters are the nested tree of MATNet.tree; nothing here calls the library.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import tanh_normal as tn
from tests import mat_model as mm

gae, loss_terms = mm.gae, mm.loss_terms  # shared with the discrete model
MIN_SCALE = tn.MIN_SCALE


def shifted_action(action, known=None):
    """action (B, A, d) -> (B, A, d): row 0 zero, row i = action[:, i - 1] for 1 <= i <= known, zero rows after that."""
    B, A, d = action.shape
    known = A - 1 if known is None else known
    s = torch.zeros((B, A, d), dtype=torch.float64)
    if known > 0:
        s[:, 1 : known + 1] = action[:, :known].to(torch.float64)
    return s


def decoder(p, rep, s, n_head: int):
    """tests/mat_model.decoder on the shifted action vectors (act_dense carries its bias in the tree): the means (B, A, d)."""
    return mm.decoder(p, rep, s, n_head)


def scale_of(log_std, min_scale: float = MIN_SCALE):
    return torch.nn.functional.softplus(log_std) + min_scale


def _log_ndtr(z):
    """oracle.tanh_normal.log_ndtr in torch (erfc on the central range, the asymptotic series below -10)."""
    hi, lo = z > 5.0, z <= -10.0
    zc = torch.where(hi | lo, torch.zeros_like(z), z)
    mid = torch.log(0.5 * torch.erfc(-zc / math.sqrt(2.0)))
    zh = torch.where(hi, z, torch.full_like(z, 6.0))
    top = -0.5 * torch.erfc(zh / math.sqrt(2.0))
    zl = torch.where(lo, z, torch.full_like(z, -11.0))
    r2 = 1.0 / (zl * zl)
    low = -0.5 * zl * zl - torch.log(-zl) - tn.HALF_LOG_2PI + torch.log(1.0 + r2 * (-1.0 + r2 * (3.0 - 15.0 * r2)))
    return torch.where(hi, top, torch.where(lo, low, mid))


def _fldj(x):
    return 2.0 * (tn.LOG2 - x - torch.nn.functional.softplus(-2.0 * x))


def log_prob(action, mean, scale):
    """TanhTransformedDistribution.log_prob summed over the last axis (oracle.tanh_normal.log_prob_terms, differentiable)."""
    yc = torch.clamp(action.to(mean.dtype), -tn.THRESH, tn.THRESH)
    left, right = yc <= -tn.THRESH, yc >= tn.THRESH
    edge = left | right
    z = torch.where(left, (-tn.ATANH_THRESH - mean) / scale, (mean - tn.ATANH_THRESH) / scale)
    x = torch.atanh(torch.where(edge, torch.zeros_like(yc), yc))
    d = (x - mean) / scale
    inner = -0.5 * d * d - torch.log(scale) - tn.HALF_LOG_2PI - _fldj(x)
    return torch.where(edge, _log_ndtr(z) - tn.LOG_EPS, inner).sum(-1)


def entropy(mean, scale, ent_eps):
    """Normal entropy + the tanh bijector's forward log-det-Jacobian at the sample mean + scale * ent_eps, summed over d."""
    xs = mean + scale * ent_eps
    return (0.5 + tn.HALF_LOG_2PI + torch.log(scale) + _fldj(xs)).sum(-1)


def forward(params, obs, action, n_head: int, min_scale: float = MIN_SCALE):
    """Teacher-forced pass: (log_prob of `action` (B, A), value (B, A), means (B, A, d), scale (d,))."""
    rep, value = mm.encoder(params["encoder"], obs, n_head)
    mean = decoder(params["decoder"], rep, shifted_action(action), n_head)
    scale = scale_of(params["decoder"]["log_std"], min_scale)
    return log_prob(action, mean, scale), value, mean, scale


def act(params, obs, eps, n_head: int, forced=None, min_scale: float = MIN_SCALE):
    """Autoregressive acting: agent i draws tanh(mean_i + scale * eps[:, i]) (eps None or zeros: greedy, the mode).  forced
    (B, A, d): agent i conditions on forced[:, :i] rather than on the model's own earlier actions, so that a float32 difference
    in an early agent does not compound into the later ones.  Returns (action (B, A, d), log_prob (B, A), value (B, A), mean)."""
    B, A, _ = obs.shape
    d = int(params["decoder"]["log_std"].shape[-1])
    rep, value = mm.encoder(params["encoder"], obs, n_head)
    scale = scale_of(params["decoder"]["log_std"], min_scale)
    action = torch.zeros((B, A, d), dtype=torch.float64)
    mean = torch.zeros((B, A, d), dtype=torch.float64)
    lp = torch.zeros((B, A), dtype=torch.float64)
    for i in range(A):
        given = action if forced is None else torch.as_tensor(forced, dtype=torch.float64)
        mean[:, i] = decoder(params["decoder"], rep, shifted_action(given, known=i), n_head)[:, i]
        e = 0.0 if eps is None else torch.as_tensor(eps[:, i], dtype=torch.float64)
        action[:, i] = torch.tanh(mean[:, i] + scale * e)
        lp[:, i] = log_prob(action[:, i], mean[:, i], scale)
    return action, lp, value, mean


def loss(params, obs, action, old_log_prob, adv, old_value, target, n_head: int, clip_eps: float, ent_coef: float, vf_coef: float,
         ent_eps, min_scale: float = MIN_SCALE):
    """(total, actor_loss, value_loss, entropy) over the agent rows of a minibatch; ent_eps (B, A, d) is the entropy sample's noise."""
    lp, value, mean, scale = forward(params, obs, action, n_head, min_scale)
    ent = entropy(mean, scale, torch.as_tensor(ent_eps, dtype=torch.float64))
    return loss_terms(lp, ent, value, old_log_prob, adv, old_value, target, clip_eps, ent_coef, vf_coef)


def entropy_noise(seed: int, ent_step: int, idx, A: int, d: int, row_offset: int = 0):
    """(len(idx), A, d) noise of the loss kernel: agent row idx[b] * A + j, counter (row_offset + row, ent_step, dim / 2, "TNEN")."""
    rows = (np.asarray(idx, np.int64)[:, None] * A + np.arange(A)[None]).reshape(-1)
    return tn.normal_noise(seed, ent_step, len(rows), d, tn.STREAM_ENTROPY, row_offset, gid=rows).astype(np.float64).reshape(len(idx), A, d)


def sample_noise(seed: int, step: int, B: int, A: int, d: int, row_offset: int = 0):
    """(B, A, d) acting noise: row b * A + agent, counter (row_offset + row, step, dim / 2, "TNSA")."""
    return tn.normal_noise(seed, step, B * A, d, tn.STREAM_SAMPLE, row_offset).astype(np.float64).reshape(B, A, d)


def minibatch_step(net, flat, m, v, count, batch, idx, cfg):
    """One minibatch of the update on the float64 flat vector: returns (flat, m, v, count, grad, metrics).  cfg carries "seed",
    "ent_step" and "min_scale" next to tests/mat_model.minibatch_step's keys."""
    from oracle.ppo_oracle import clip_adam

    f = torch.tensor(np.asarray(flat, np.float64), requires_grad=True)
    sel = lambda a: a[idx]
    A, d = batch["action"].shape[1:]
    eps = entropy_noise(cfg["seed"], cfg["ent_step"], np.asarray(idx), A, d)
    total, actor, vloss, ent = loss(net.tree(f), sel(batch["obs"]), sel(batch["action"]), sel(batch["log_prob"]), sel(batch["adv"]),
                                    sel(batch["value"]), sel(batch["target"]), cfg["n_head"], cfg["clip_eps"], cfg["ent_coef"],
                                    cfg["vf_coef"], eps, cfg.get("min_scale", MIN_SCALE))
    total.backward()
    grad = f.grad.numpy().copy()
    flat, m, v, count = clip_adam(np.asarray(flat, np.float64), grad, m, v, count, cfg["lr"], cfg["max_grad_norm"])
    return flat, m, v, count, grad, np.array([float(t.detach()) for t in (total, vloss, actor, ent)])


# ---- the loss head alone, in NumPy: the reference of the loss kernel's test and the float32 floor -----------------------------
def loss_head(mean, log_std, values, action, old_lp, adv, old_value, target, eps, clip_eps, ent_coef, vf_coef, min_scale=MIN_SCALE,
              dtype=np.float64):
    """The loss on given means (R, d) and values (R,) of agent rows, every operation in `dtype`: returns a dict with actor_loss,
    entropy, value_loss and the gradients dmean (R, d), dvalues (R,) (includes vf_coef), dlog_std (d,) of
    actor_loss - ent_coef * entropy + vf_coef * value_loss."""
    c = lambda a: np.asarray(a, dtype)
    mean, log_std, values, action, old_lp, adv, old_value, target, eps = (c(a) for a in (mean, log_std, values, action, old_lp, adv,
                                                                                          old_value, target, eps))
    R = mean.shape[0]
    scale = np.broadcast_to((tn.softplus(log_std) + dtype(min_scale)).astype(dtype), mean.shape)
    lpd, dm_lp, ds_lp = tn.log_prob_terms(action, mean, scale, dtype)
    g = (adv - adv.mean()) / (np.sqrt(np.maximum((adv * adv).mean() - adv.mean() ** 2, 0)) + dtype(1e-8))
    ratio = np.exp(lpd.sum(-1) - old_lp)
    lo, hi = dtype(1.0 - clip_eps), dtype(1.0 + clip_eps)
    l1, l2 = ratio * g, np.clip(ratio, lo, hi) * g
    inside = (ratio >= lo) & (ratio <= hi)
    g1 = np.where(l1 < l2, 1.0, np.where(l1 == l2, 0.5, 0.0)).astype(dtype)
    dlp = (-(g1 * g + (1.0 - g1) * g * inside) / R * ratio)[:, None]
    xs = mean + scale * eps
    ent = (0.5 + tn.HALF_LOG_2PI + np.log(scale) + tn.tanh_fldj(xs)).sum(-1)
    th, ec = np.tanh(xs), dtype(ent_coef) / R
    dmean = dlp * dm_lp + ec * 2.0 * th
    dls = ((dlp * ds_lp - ec * (1.0 / scale - 2.0 * th * eps)) * tn.sigmoid(log_std)).sum(0)
    diff = values - old_value
    vclip = old_value + np.clip(diff, -dtype(clip_eps), dtype(clip_eps))
    e1, e2 = values - target, vclip - target
    v1, v2 = e1 * e1, e2 * e2
    vin = (diff >= -dtype(clip_eps)) & (diff <= dtype(clip_eps))
    h1 = np.where(v1 > v2, 1.0, np.where(v1 == v2, 0.5, 0.0)).astype(dtype)
    dvalues = dtype(vf_coef) * (h1 * e1 + (1.0 - h1) * vin * e2) / R
    return {"actor_loss": -np.minimum(l1, l2).sum() / R, "entropy": ent.sum() / R, "value_loss": 0.5 * np.maximum(v1, v2).sum() / R,
            "dmean": dmean, "dvalues": dvalues, "dlog_std": dls}


SEED, ENT_STEP, CLIP, ENT_COEF, VF_COEF = 0x9E3779B97F4A7C15, 7, 0.2, 0.01, 0.5
LOSS_SHAPES = ((11, 3), (7, 5))  # (Bm, A): 33 rows (a sample across a tile edge, a padded last tile) and 35
DIMS = (1, 2, 8, 9, 16)  # both sides of the loss kernel's 8 | 16 split


def loss_case(d: int, Bm: int, A: int, row_offset: int = 0):
    """Inputs of the loss kernel's test at float32 values (trajectory arrays over TE = Bm + 5 samples, a gathered idx) and the
    float64 answers.  Every 37th action sits at +-0.9995 (both clipped branches), old_log_prob is jittered by 0.25 (both clip sides)."""
    rng = np.random.default_rng(7000 + 100 * d + 10 * Bm + A)
    f32 = lambda a: np.asarray(a, np.float32)
    TE, R = Bm + 5, Bm * A
    rows = -(-R // 32) * 32
    idx = rng.permutation(TE)[:Bm].astype(np.int32)
    g = lambda x: x[idx].reshape((R,) + x.shape[2:])
    mean, log_std = f32(rng.standard_normal((R, d)) * 0.5), f32(rng.standard_normal(d) * 0.5)
    action = f32(np.tanh(rng.standard_normal((TE, A, d))))
    action.reshape(-1)[::37] = np.float32(0.9995) * np.sign(action.reshape(-1)[::37] + np.float32(1e-3))
    scale = tn.softplus(log_std.astype(np.float64)) + MIN_SCALE
    lp_now = tn.log_prob_terms(g(action), mean.astype(np.float64), np.broadcast_to(scale, mean.shape))[0].sum(-1)
    old_lp = f32(rng.standard_normal((TE, A)))
    old_lp[idx] = f32(lp_now + rng.standard_normal(R) * 0.25).reshape(Bm, A)
    adv = f32(rng.standard_normal((TE, A)) * 2 + 0.3)
    values = f32(rng.standard_normal(R))
    old_value, target = f32(rng.standard_normal((TE, A))), f32(rng.standard_normal((TE, A)))
    old_value[idx] = f32(values + rng.standard_normal(R) * 0.2).reshape(Bm, A)
    target[idx] = f32(values + rng.standard_normal(R)).reshape(Bm, A)
    ext = (idx.astype(np.int64)[:, None] * A + np.arange(A)[None]).reshape(-1)
    eps = tn.normal_noise(SEED, ENT_STEP, R, d, tn.STREAM_ENTROPY, row_offset, gid=ext)
    a = g(adv).astype(np.float64).reshape(-1)
    stats = np.array([[s.sum(), (s * s).sum()] for s in np.array_split(a, 3)])
    c = dict(d=d, Bm=Bm, A=A, R=R, rows=rows, idx=idx, mean=mean, log_std=log_std, action=action, old_lp=old_lp, adv=adv, values=values,
             old_value=old_value, target=target, eps=eps, stats=stats, row_offset=row_offset,
             rows_in=(mean, log_std, values, g(action), g(old_lp), g(adv), g(old_value), g(target), eps))
    c["want"] = loss_head(*c["rows_in"], CLIP, ENT_COEF, VF_COEF)
    return c


def rel_err(a, b):
    """conftest.assert_close's form: the largest |a - b| / (|b| + rms(b))."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + np.sqrt(np.mean(b * b)))).max())


def loss_f32_floor(c):
    """How far the float32 NumPy evaluation of the loss head's gradients lies from float64 on a case's inputs."""
    got = loss_head(*c["rows_in"], CLIP, ENT_COEF, VF_COEF, dtype=np.float32)
    return max(rel_err(got[k], c["want"][k]) for k in ("dmean", "dvalues", "dlog_std"))


GRAD_TOL = 1e-4  # the project's gradient bound (tests/test_gpu_seq_kernels.py)


def loss_grad_bound(c):
    """The gradient bound of a case: the project's 1e-4 where float32 itself stays inside it on the case's inputs, four times
    the case's measured float32 floor where it does not."""
    floor = loss_f32_floor(c)
    return GRAD_TOL if floor <= GRAD_TOL else 4.0 * floor
