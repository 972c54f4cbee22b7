"""TEST INFRASTRUCTURE ONLY.  Plain float64 references of the recurrent PPO path's kernels, one operation each
(csrc/rec_gru.hip, rec_gru_h2.hip, rec_out_h2.hip), the case tables of tests/test_gpu_seq_kernels.py and a restatement of the
host dispatch that decides which template instance a case runs.  Built from oracle/rec_oracle.py (gru_step, _sigmoid),
oracle/ppo_oracle.py (masked_logits, log_softmax, gumbel_argmax), oracle/philox.py and oracle/tanh_normal.py; the gradients
of the scan and of the output path's layers come from torch float64 autograd.  tests/test_seq_model.py checks on the CPU that
the pieces, composed, are the whole-network oracle, and that each deliberately wrong variant below differs exactly where its
case is meant to catch it."""
from functools import lru_cache

import numpy as np
import torch

from oracle import philox
from oracle import ppo_oracle as po
from oracle import rec_oracle as ro
from oracle import tanh_normal as tn

H = 128
CLIP, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
f32 = lambda a: np.asarray(a, np.float32)
f64 = lambda a: np.asarray(a, np.float64)


# ---- T32: tiles of 32 rows, feature-major inside a tile ------------------------------------------------------------------
def to_t32(a):
    """(rows, N) row-major numpy -> T32 flat numpy."""
    rows, N = a.shape
    return a.reshape(rows // 32, 32, N).transpose(0, 2, 1).reshape(-1).copy()


def from_t32(flat, rows, N):
    return np.asarray(flat).reshape(rows // 32, N, 32).transpose(0, 2, 1).reshape(rows, N)


def ext_index(idx, E, A, Rm):
    """minibatch row m -> flat (env, agent) index of the external (E, A) arrays: env = idx[m / A], agent = m % A."""
    m = np.arange(Rm)
    e_local = m // A
    env = e_local if idx is None else np.asarray(idx)[e_local]
    return env * A + m % A


def gather_rows(x, idx, A, Rm):
    """external (T, E, A, ...) -> (T, Rm, ...) time-major minibatch rows."""
    T, E = x.shape[:2]
    return x.reshape(T, E * A, *x.shape[3:])[:, ext_index(idx, E, A, Rm)]


def done_rows(done, idx, A, Rm, env_flag_only=False):
    """(T, E, A) reset flags -> (T, Rm) bool.  env_flag_only: the WRONG rule that reads agent 0's flag for the whole env."""
    d = np.asarray(done) != 0
    if env_flag_only:
        d = np.repeat(d[:, :, :1], A, 2)
    return gather_rows(d, idx, A, Rm)


# ---- GRU scan --------------------------------------------------------------------------------------------------------------
_EYE = {"Wi": np.eye(3 * H), "bi": np.zeros(3 * H)}


def gru_scan(gi, Wh, bhn, h0, done, tile_stride=None):
    """gi (T, Rm, 384) = W_i x + b_i of every step, h0 (Rm, 128), done (T, Rm) bool (flag entering the step).
    Returns hs (T, Rm, 128), hprev (the masked state entering each step) and saved = [r | z | n | W_hn h + b_hn] (T, Rm, 512).
    tile_stride: the T32 tile of step t, sequence tile mt is read at t * tile_stride + mt; anything but Rm / 32 is WRONG."""
    gi, Wh, bhn, h = f64(gi), f64(Wh), f64(bhn), f64(h0)
    T, Rm, _ = gi.shape
    if tile_stride is not None:
        tiles = gi.reshape(T * Rm // 32, 32, 3 * H)
        gi = np.stack([np.concatenate([tiles[t * tile_stride + mt] for mt in range(Rm // 32)]) for t in range(T)])
    p = dict(_EYE, Wh=Wh, bhn=bhn)
    hs, hprev, saved = [], [], []
    for t in range(T):
        h = np.where(done[t][:, None], 0.0, h)
        gh = h @ Wh
        r = ro._sigmoid(gi[t][:, :H] + gh[:, :H])
        z = ro._sigmoid(gi[t][:, H : 2 * H] + gh[:, H : 2 * H])
        hl = gh[:, 2 * H :] + bhn
        n = np.tanh(gi[t][:, 2 * H :] + r * hl)
        hprev.append(h)
        saved.append(np.concatenate([r, z, n, hl], 1))
        h = ro.gru_step(p, gi[t], h)
        hs.append(h)
    return np.stack(hs), np.stack(hprev), np.stack(saved)


def gru_scan_grads(gi, Wh, bhn, h0, done, dh_out):
    """torch float64 autograd of sum(hs * dh_out): (dgi, dgh), both (T, Rm, 384); gh = h W_h before b_hn is added."""
    tt = lambda a: torch.tensor(f64(a))
    gi_t, Wh_t, bhn_t, h = tt(gi).requires_grad_(True), tt(Wh), tt(bhn), tt(h0)
    dn = torch.tensor(np.asarray(done, bool))
    total, ghs = 0.0, []
    for t in range(gi_t.shape[0]):
        h = torch.where(dn[t][:, None], torch.zeros_like(h), h)
        dg = torch.zeros(h.shape[0], 3 * H, dtype=torch.float64, requires_grad=True)  # its gradient is d / d gh
        gh = h @ Wh_t + dg
        ghs.append(dg)
        r = torch.sigmoid(gi_t[t][:, :H] + gh[:, :H])
        z = torch.sigmoid(gi_t[t][:, H : 2 * H] + gh[:, H : 2 * H])
        n = torch.tanh(gi_t[t][:, 2 * H :] + r * (gh[:, 2 * H :] + bhn_t))
        h = (1.0 - z) * n + z * h
        total = total + (h * tt(dh_out[t])).sum()
    total.backward()
    return gi_t.grad.numpy(), np.stack([g.grad.numpy() for g in ghs])


# ---- losses ------------------------------------------------------------------------------------------------------------------
def _ppo_terms(lp, old_lp, adv):
    """Clipped surrogate of rec_mappo.py:226-236: (loss, d loss / d lp, ratio, normalised advantages)."""
    R = lp.shape[0]
    g = po.normalise_advantages(f64(adv))
    ratio = np.exp(lp - old_lp)
    l1, l2 = ratio * g, np.clip(ratio, 1.0 - CLIP, 1.0 + CLIP) * g
    inside = (ratio >= 1.0 - CLIP) & (ratio <= 1.0 + CLIP)
    g1 = np.where(l1 < l2, 1.0, np.where(l1 == l2, 0.5, 0.0))
    dlp = -(g1 * g + (1.0 - g1) * g * inside) / R * ratio
    return -np.minimum(l1, l2).sum() / R, dlp, ratio, g


def actor_loss(logits, mask, action, old_lp, adv, ent_coef=ENT_COEF, slots=None):
    """Clipped PPO actor loss on masked logits (R, no): (loss_actor, entropy, d (loss_actor - ent_coef entropy) / d logits).
    A row without a legal action is uniform over its no actions (networks.py:116-120 + softmax).
    slots: the WRONG rule that pads the row to `slots` outputs and lets the padding into the softmax sum."""
    logits = f64(logits)
    R, no = logits.shape
    z = po.masked_logits(logits, mask)
    if slots is not None:
        z = np.concatenate([z, np.full((R, slots - no), po.F32_MIN)], 1)
    logp = po.log_softmax(z)
    p = np.exp(logp)
    ent_rows = po.categorical_entropy(logp)
    loss, dlp, _, _ = _ppo_terms(logp[np.arange(R), action], f64(old_lp), adv)
    onehot = np.zeros_like(z)
    onehot[np.arange(R), action] = 1.0
    dz = dlp[:, None] * (onehot - p) + (ent_coef / R) * p * (np.where(p > 0, logp, 0.0) + ent_rows[:, None])
    dz = dz[:, :no]
    if mask is not None:
        dz = np.where(np.asarray(mask).astype(bool), dz, 0.0)
    return loss, ent_rows.sum() / R, dz


def log_probs(logits, mask):
    return po.log_softmax(po.masked_logits(f64(logits), mask))


def critic_loss(v, old_v, tgt, vf_coef=VF_COEF, slots_summed=None):
    """Clipped value loss of rows that stand for na agent slots each: v (R,), old_v / tgt (R, na).  Returns (value_loss, dv) with
    dv = d (vf_coef value_loss) / d v summed over the row's slots.  slots_summed = 1: the WRONG rule that sees one slot."""
    v, ov, tg = f64(v)[:, None], f64(old_v), f64(tgt)
    R, na = ov.shape
    diff = v - ov
    vclip = ov + np.clip(diff, -CLIP, CLIP)
    l1, l2 = (v - tg) ** 2, (vclip - tg) ** 2
    inside = (diff >= -CLIP) & (diff <= CLIP)
    g1 = np.where(l1 > l2, 1.0, np.where(l1 == l2, 0.5, 0.0))
    dv = vf_coef * (g1 * (v - tg) + (1.0 - g1) * (vclip - tg) * inside) / (R * na)
    per = 0.5 * np.maximum(l1, l2) / (R * na)
    k = na if slots_summed is None else slots_summed
    return per[:, :k].sum(), dv[:, :k].sum(1)


def continuous_loss(mean, raw, action, old_lp, adv, eps, ent_coef=ENT_COEF, dtype=np.float64):
    """Clipped PPO loss of the tanh-normal head (networks.py:127-169): mean / action / eps (R, d); raw = the log_std vector (d,)
    or per-row raw scales (R, d).  Returns (loss_actor, entropy, dmean, draw) with draw shaped like raw.  dtype: every operation
    in it (how far float32 itself lies from float64)."""
    mean, raw, action, eps = (np.asarray(a, dtype) for a in (mean, raw, action, eps))
    R = mean.shape[0]
    scale = np.broadcast_to(tn.scale_of(raw).astype(dtype), mean.shape)
    lpd, dm_lp, ds_lp = tn.log_prob_terms(action, mean, scale, dtype)
    g = np.asarray(adv, dtype)
    g = (g - g.mean()) / (g.std() + dtype(1e-8))
    ratio = np.exp(lpd.sum(-1) - np.asarray(old_lp, dtype))
    l1, l2 = ratio * g, np.clip(ratio, 1.0 - CLIP, 1.0 + CLIP) * g
    inside = (ratio >= 1.0 - CLIP) & (ratio <= 1.0 + CLIP)
    g1 = np.where(l1 < l2, 1.0, np.where(l1 == l2, 0.5, 0.0)).astype(dtype)
    dlp = (-(g1 * g + (1.0 - g1) * g * inside) / R * ratio)[:, None]
    xs = mean + scale * eps
    ent = (0.5 + tn.HALF_LOG_2PI + np.log(scale) + tn.tanh_fldj(xs)).sum(-1)
    th, ec = np.tanh(xs), ent_coef / R
    dmean = dlp * dm_lp + ec * 2.0 * th
    draw = (dlp * ds_lp - ec * (1.0 / scale - 2.0 * th * eps)) * tn.sigmoid(raw)
    if raw.ndim == 1:
        draw = draw.sum(0)
    return -np.minimum(l1, l2).sum() / R, ent.sum() / R, dmean, draw


def entropy_noise(seed, ent_step, row_offset, ext_rows, dim):
    """The entropy draw as the kernel keys it: Philox counter (row_offset + external row, ent_step, d / 2, "TNEN")."""
    return tn.normal_noise(seed, ent_step, len(ext_rows), dim, tn.STREAM_ENTROPY, row_offset, gid=ext_rows)


# ---- output path: hs -> relu(Wpost) -> head -> loss ----------------------------------------------------------------------------
def out_params(rng, no, head_scale=1.0):
    return dict(Wpost=f32(po.orthogonal(rng, (H, H), np.sqrt(2.0))), bpost=f32(rng.standard_normal(H) * 0.1),
                Whead=f32(po.orthogonal(rng, (H, no), head_scale)), bhead=f32(rng.standard_normal(no) * 0.1))


def out_flat(p):
    return np.concatenate([p[k].reshape(-1) for k in ("Wpost", "bpost", "Whead", "bhead")])


CLIP_CLEAR = 2e-5  # ratios and value differences are O(1): twenty float32 roundings
RELU_CLEAR = 5e-5  # the split-f16 products carry about 1e-6 of a pre-activation's magnitude


def out_pre(hs, p):
    return f64(hs) @ f64(p["Wpost"]) + f64(p["bpost"])


def out_forward(hs, p):
    return np.maximum(out_pre(hs, p), 0.0) @ f64(p["Whead"]) + f64(p["bhead"])


def out_path(hs, p, loss_fn):
    """loss_fn(y (R, no)) -> (losses tuple, dy).  Returns (losses, grads) with grads = dh, dWpost, dbpost, dWhead, dbhead."""
    t = {k: torch.tensor(f64(v), requires_grad=True) for k, v in dict(p, hs=hs).items()}
    y = torch.relu(t["hs"] @ t["Wpost"] + t["bpost"]) @ t["Whead"] + t["bhead"]
    losses, dy = loss_fn(y.detach().numpy())
    y.backward(torch.tensor(dy.reshape(y.shape)))
    return losses, {"dh" if k == "hs" else "d" + k: v.grad.numpy() for k, v in t.items()}


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def gumbel_scores(logits, mask, u, dtype=np.float64):
    z = po.masked_logits(np.asarray(logits, dtype), mask)
    return z - np.log(-np.log(np.asarray(u, dtype)))


def sample_discrete(logits, mask, seed, step, row_offset):
    """(action of the float64 Gumbel arg-max, top-two gap of the float64 scores, float32-vs-float64 score difference)."""
    rows, n = logits.shape
    u = philox.policy_uniforms(seed, step, rows, n, row_offset)
    z = po.masked_logits(f64(logits), mask)
    a = po.gumbel_argmax(z, u)
    s64, s32 = gumbel_scores(logits, mask, u), gumbel_scores(logits, mask, u, np.float32)
    legal = np.ones_like(s64, bool) if mask is None else np.asarray(mask).astype(bool)
    srt = np.sort(s64, -1)
    gap = srt[:, -1] - srt[:, -2] if n > 1 else np.full(rows, np.inf)
    return a, gap, float(np.abs(s32.astype(np.float64) - s64)[legal].max())


def greedy_discrete(logits, mask):
    return np.argmax(po.masked_logits(f64(logits), mask), -1).astype(np.int32)  # first index of a tie


# ---- dispatch, restated from the hosts (rec_gru.hip, rec_gru_h2.hip, rec_out_h2.hip) ---------------------------------------------
def seq_loss_instance(n_actions):
    return ("seq_loss", 8 if n_actions <= 8 else 16 if n_actions <= 16 else 32, True)


def seq_sample_instance(n_actions):
    return ("seq_sample", 8 if n_actions <= 8 else 16 if n_actions <= 16 else 32)


def cont_instances(dim):
    w = 8 if dim <= 8 else 16
    return [("seq_loss_cont", w), ("seq_sample_cont", w)]


def rec_out_instance(is_actor, n_out, n_slab, tiles):
    """None: refused (returns 1, the caller runs the layer-wise kernels)."""
    if n_out > 16 or (not is_actor and n_out != 1) or n_slab > tiles:
        return None
    return ("rec_out", 8, False) if not is_actor else ("rec_out", 8 if n_out <= 8 else 16, True)


def scan_bwd_instance(mode, dgh_n_only):
    return ("gru_scan_bwd_h2", bool(dgh_n_only)) if mode == 1 else ("gru_scan_bwd",)


# ---- case tables -----------------------------------------------------------------------------------------------------------------
SCAN_T = (1, 5)
SCAN_SHAPES = ((8, 4, 8, False), (40, 3, 32, True))  # (E, A, Em, gathered): Rm = 32 | 96
SCAN_DONE = ("none", "all_t0", "one_seq", "random")
ALL_MASKED_N = (5, 9, 17)
ACTOR_N = (1, 2, 5, 8, 9, 16, 17, 32)
SAMPLE_N = ACTOR_N
SAMPLE_ROWS = (32, 288)
ROW_OFFSETS = (0, 1000)
CONT_DIMS = (1, 8, 9, 16)
CRITIC_AGENTS = (1, 3)
N_BLOCKS = (1, 2, 5)
GRAD_SCALES = (1.0, 256.0)
OUT_N = (1, 2, 5, 8, 9, 16)
OUT_SLABS = (1, 4, 6)
OUT_REFUSED = ((True, 17, 1), (False, 2, 1), (True, 5, 7))  # (is_actor, n_out, n_slab) at 6 tiles
LOSS_T, LOSS_E, LOSS_A, LOSS_EM = 3, 24, 4, 16  # Rm = 64, 192 rows, 6 tiles
SEED = 0x9E3779B97F4A7C15  # both 32-bit halves in use


@lru_cache(maxsize=None)
def scan_case(T, E, A, Em, gathered, done_kind):
    rng = np.random.default_rng(1000 * T + E)
    Rm = Em * A
    idx = rng.permutation(E)[:Em].astype(np.int32) if gathered else None
    done = np.zeros((T, E, A), np.uint8)
    if done_kind == "all_t0":
        done[0] = 1
    elif done_kind == "one_seq":
        done[:, 1 if idx is None else idx[1], 1] = 1
    elif done_kind == "random":
        done = (rng.random((T, E, A)) < 0.3).astype(np.uint8)
    c = dict(T=T, E=E, A=A, Rm=Rm, idx=idx, done=done, gi=f32(rng.standard_normal((T, Rm, 3 * H))),
             Wh=f32(np.concatenate([po.orthogonal(rng, (H, H), 1.0) for _ in range(3)], 1)), bhn=f32(rng.standard_normal(H) * 0.1),
             h0=f32(rng.standard_normal((E, A, H)) * 0.5), dh_out=f32(rng.standard_normal((T, Rm, H))))
    c["h0_rows"] = gather_rows(c["h0"][None], idx, A, Rm)[0]
    c["done_rows"] = done_rows(done, idx, A, Rm)
    c["hs"], c["hprev"], c["saved"] = gru_scan(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"])
    # the backward consumes the float32 roundings of the forward's values, as the kernel does
    c["dgi"], c["dgh"] = gru_scan_grads(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"], c["dh_out"])
    return c


def _mask(rng, shape_rows, n, all_masked):
    """25 % illegal, rows 3 and 70 with one legal action, rows 11 and 20 without any (flat external rows)."""
    m = rng.random(shape_rows + (n,)) > 0.25
    flat = m.reshape(-1, n)
    flat[np.arange(flat.shape[0]), rng.integers(0, n, flat.shape[0])] = True
    one, none = [r for r in (3, 70) if r < flat.shape[0]], [r for r in (11, 20) if r < flat.shape[0]] if all_masked else []
    for r in one:
        flat[r] = False
        flat[r, rng.integers(0, n)] = True
    for r in none:
        flat[r] = False
    return m, one, none


@lru_cache(maxsize=None)
def actor_case(n, constant_adv=False, masked=True):
    """External arrays of one minibatch of the discrete actor loss; the rows of the minibatch come first in idx so that the special
    mask rows (external rows 3, 11, 20, 70 of step 0: envs 0, 2, 5, 17) are inside it."""
    rng = np.random.default_rng(2000 + n)
    T, E, A, Em = LOSS_T, LOSS_E, LOSS_A, LOSS_EM
    Rm, R = Em * A, T * Em * A
    idx = np.concatenate([[0, 2, 5, 17], rng.permutation(np.setdiff1d(np.arange(E), [0, 2, 5, 17]))[: Em - 4]]).astype(np.int32)
    rng.shuffle(idx)
    mask, one, none = _mask(rng, (T, E, A), n, n in ALL_MASKED_N)
    if not masked:
        mask, one, none = None, [], []
    logits = f32(rng.standard_normal((R, n)) * 1.5)
    action = rng.integers(0, n, (T, E, A)).astype(np.int32)
    if mask is not None:
        flat, af = mask.reshape(-1, n), action.reshape(-1)
        for r in range(flat.shape[0]):
            if flat[r].any() and not flat[r, af[r]]:
                af[r] = np.flatnonzero(flat[r])[rng.integers(0, flat[r].sum())]
    g = lambda x: gather_rows(x, idx, A, Rm).reshape((R,) + x.shape[3:])
    mrows = None if mask is None else g(mask)
    lp_now = log_probs(logits, mrows)[np.arange(R), g(action)]
    old_lp = np.zeros((T, E, A), np.float32)
    old_lp.reshape(T, E * A)[:, ext_index(idx, E, A, Rm)] = (lp_now + rng.standard_normal(R) * 0.25).reshape(T, Rm)
    adv = np.full((T, E, A), 0.5, np.float32) if constant_adv else f32(rng.standard_normal((T, E, A)) * 2 + 0.3)
    c = dict(T=T, E=E, A=A, Rm=Rm, R=R, n=n, idx=idx, mask=mask, logits=logits, action=action, old_lp=old_lp, adv=adv,
             mask_rows=mrows, action_rows=g(action), old_lp_rows=g(old_lp), adv_rows=g(adv))
    ext = (np.arange(T)[:, None] * E * A + ext_index(idx, E, A, Rm)[None]).reshape(-1)
    c["one_legal"] = [int(np.flatnonzero(ext == r)[0]) for r in one if (ext == r).any()]
    c["all_masked"] = [int(np.flatnonzero(ext == r)[0]) for r in none if (ext == r).any()]
    c["ext"] = ext
    c["loss"], c["entropy"], c["dlogits"] = actor_loss(logits, mrows, c["action_rows"], c["old_lp_rows"], c["adv_rows"])
    return c


def adv_stats(adv_rows, parts=3):
    """Partial (sum, sum of squares) pairs in float64, as mava_adv_stats_f64 leaves them."""
    a = f64(adv_rows).reshape(-1)
    return np.array([[s.sum(), (s * s).sum()] for s in np.array_split(a, parts)])


@lru_cache(maxsize=None)
def critic_case(na):
    rng = np.random.default_rng(3000 + na)
    T, E, A, Em = (LOSS_T, 80, 1, 64) if na > 1 else (LOSS_T, LOSS_E, LOSS_A, LOSS_EM)  # Rm = 64 either way; na > 1 needs A = 1
    Rm, R = Em * A, T * Em * A
    idx = rng.permutation(E)[:Em].astype(np.int32)
    v = f32(rng.standard_normal(R))
    g = lambda x: gather_rows(x, idx, A, Rm).reshape((R,) + x.shape[3:])
    old_v, tgt = np.zeros((T, E, A, na), np.float32), np.zeros((T, E, A, na), np.float32)
    rows = ext_index(idx, E, A, Rm)
    old_v.reshape(T, E * A, na)[:, rows] = (v[:, None] + rng.standard_normal((R, na)) * 0.2).reshape(T, Rm, na)
    tgt.reshape(T, E * A, na)[:, rows] = (v[:, None] + rng.standard_normal((R, na))).reshape(T, Rm, na)
    c = dict(T=T, E=E, A=A, Rm=Rm, R=R, na=na, idx=idx, v=v, old_v=old_v, tgt=tgt, old_v_rows=g(old_v), tgt_rows=g(tgt))
    c["loss"], c["dv"] = critic_loss(v, c["old_v_rows"], c["tgt_rows"])
    return c


@lru_cache(maxsize=None)
def cont_case(dim, per_row, row_offset):
    rng = np.random.default_rng(4000 + dim)
    T, E, A, Em = LOSS_T, LOSS_E, LOSS_A, LOSS_EM
    Rm, R = Em * A, T * Em * A
    idx = rng.permutation(E)[:Em].astype(np.int32)
    g = lambda x: gather_rows(x, idx, A, Rm).reshape((R,) + x.shape[3:])
    mean = f32(rng.standard_normal((R, dim)) * 0.5)
    raw = f32(rng.standard_normal((R, dim)) * 0.5) if per_row else f32(rng.standard_normal(dim) * 0.5)
    action = f32(np.tanh(rng.standard_normal((T, E, A, dim))))
    action.reshape(-1)[::37] = np.float32(0.9995) * np.sign(action.reshape(-1)[::37] + np.float32(1e-3))  # the clipped branches
    lp_now = tn.log_prob_terms(g(action), f64(mean), np.broadcast_to(tn.scale_of(f64(raw)), mean.shape))[0].sum(-1)
    old_lp = np.zeros((T, E, A), np.float32)
    old_lp.reshape(T, E * A)[:, ext_index(idx, E, A, Rm)] = (lp_now + rng.standard_normal(R) * 0.25).reshape(T, Rm)
    adv = f32(rng.standard_normal((T, E, A)) * 2 + 0.3)
    ext = (np.arange(T)[:, None] * E * A + ext_index(idx, E, A, Rm)[None]).reshape(-1)
    c = dict(T=T, E=E, A=A, Rm=Rm, R=R, dim=dim, idx=idx, mean=mean, raw=raw, action=action, old_lp=old_lp, adv=adv, ent_step=7,
             row_offset=row_offset, action_rows=g(action), old_lp_rows=g(old_lp), adv_rows=g(adv), ext=ext)
    c["eps"] = entropy_noise(SEED, 7, row_offset, ext, dim)
    c["loss"], c["entropy"], c["dmean"], c["draw"] = continuous_loss(mean, raw, c["action_rows"], c["old_lp_rows"], c["adv_rows"], c["eps"])
    return c


def cont_f32_error(c):
    """Largest relative distance (conftest.assert_close's form) of the float32 NumPy evaluation of continuous_loss from float64."""
    got = continuous_loss(c["mean"], c["raw"], c["action_rows"], c["old_lp_rows"], c["adv_rows"], c["eps"], dtype=np.float32)
    return max(rel_err(got[2], c["dmean"]), rel_err(got[3], c["draw"]))


def rel_err(a, b):
    a, b = f64(a), f64(b)
    return float((np.abs(a - b) / (np.abs(b) + np.sqrt(np.mean(b * b)))).max())


@lru_cache(maxsize=None)
def sample_case(n, rows, row_offset):
    rng = np.random.default_rng(5000 + n + rows)
    logits = f32(rng.standard_normal((rows, n)) * 1.5)
    mask, one, none = _mask(rng, (rows,), n, n in ALL_MASKED_N)
    # exact ties: a whole row of equal logits, and a tie of the two largest with the lower index first
    logits[5] = np.float32(0.25)
    if n > 2:
        logits[6] = np.float32(-1.0)
        logits[6, [n - 2, n - 1]] = np.float32(2.0)
        mask[6, [n - 2, n - 1]] = True
    step = 5
    a, gap, f32_diff = sample_discrete(logits, mask, SEED, step, row_offset)
    return dict(n=n, rows=rows, row_offset=row_offset, step=step, logits=logits, mask=mask, one_legal=one, all_masked=none, sampled=a,
                gap=gap, f32_diff=f32_diff, greedy=greedy_discrete(logits, mask), logp=log_probs(logits, mask))


@lru_cache(maxsize=None)
def out_case(is_actor, n_out, na=1):
    """Fused output path: hidden states of 6 tiles, the loss case's external arrays, the model's gradients."""
    c = dict(actor_case(n_out)) if is_actor else dict(critic_case(na))
    for draw in range(64):  # the first draw that stays RELU_CLEAR from relu's kink and CLIP_CLEAR from the clip boundaries
        rng = np.random.default_rng([6000 + n_out + 10 * na, draw])
        p = out_params(rng, n_out)
        hs = f32(rng.standard_normal((c["R"], H)) * 0.5)
        y = out_forward(hs, p)
        if is_actor:  # old log-probs near the log-probs of THESE logits
            lp_now = log_probs(y, c["mask_rows"])[np.arange(c["R"]), c["action_rows"]]
            old = np.zeros_like(c["old_lp"])
            old.reshape(c["T"], -1)[:, ext_index(c["idx"], c["E"], c["A"], c["Rm"])] = (lp_now + rng.standard_normal(c["R"]) * 0.25).reshape(c["T"], c["Rm"])
            c["old_lp"], c["old_lp_rows"] = old, gather_rows(old, c["idx"], c["A"], c["Rm"]).reshape(-1)
            x = np.exp(lp_now - f64(c["old_lp_rows"]))
            edge = min(np.abs(x - (1 - CLIP)).min(), np.abs(x - (1 + CLIP)).min())
        else:
            x = y[:, :1] - c["old_v_rows"]
            edge = min(np.abs(x - CLIP).min(), np.abs(x + CLIP).min())
        if np.abs(out_pre(hs, p)).min() >= RELU_CLEAR and edge >= CLIP_CLEAR:
            break
    else:
        raise AssertionError("no draw clear of the kinks")
    if is_actor:
        def loss_fn(y):
            la, ent, dy = actor_loss(y, c["mask_rows"], c["action_rows"], c["old_lp_rows"], c["adv_rows"])
            return (la, ent), dy
    else:
        def loss_fn(y):
            vl, dv = critic_loss(y[:, 0], c["old_v_rows"], c["tgt_rows"])
            return (vl, 0.0), dv[:, None]
    c["params"], c["hs"] = p, hs
    c["losses"], c["grads"] = out_path(hs, p, loss_fn)
    return c
