"""TEST INFRASTRUCTURE ONLY.  Float64 cases of the two kernels of csrc/mat.hip that work on agent rows, mava_mat_sample_f32 and
mava_mat_loss_f32, and the case tables of tests/test_gpu_mat_kernels.py.  The formulas are tests/seq_model.py's (actor_loss,
critic_loss, log_probs, sample_discrete, greedy_discrete, adv_stats, _mask): the MAT kernels state the same operations on another
row layout.  tests/test_mat_kernel_model.py ties them to the independent statement of the loss in tests/mat_model.py and holds
every case to its conditions.  Nothing here calls the library.

Rows.  Agent j of sample b is row b * A + j.  The sampler's mask is (B, A, n) row-major, its logits T32; its Philox row id is
row_offset + b * A + agent.  The loss reads logits and values at the minibatch row q = b * A + j and everything else at the
trajectory row idx[b] * A + j."""
from functools import lru_cache

import numpy as np

from oracle import ppo_oracle as po
from tests import seq_model as sm

f32, f64 = sm.f32, sm.f64
c32 = lambda n: -(-n // 32) * 32

# ---- case tables ---------------------------------------------------------------------------------------------------------------
# one action | under one Philox word | a partial last word | past the 32 of the seq kernels | one under MAX_ACT | MAX_ACT
MAT_N = (1, 2, 5, 17, 33, 63, 64)
# (B, A): 21 rows under one tile | a second block with idle threads in its tail, 900 rows, samples across tile edges | 325 rows |
# one agent
MAT_SAMPLE_SHAPES = ((7, 3), (300, 3), (65, 5), (40, 1))
# (Bm, A): 15 rows of 32 | 900 rows of 928: four waves, grid-stride walks, 28 padding rows, several blocks | two full tiles
MAT_LOSS_SHAPES = ((5, 3), (300, 3), (64, 1))
ROW_OFFSETS = sm.ROW_OFFSETS
N_BLOCKS = sm.N_BLOCKS  # at 928 rows the fifth block owns no row
GRAD_SCALES = (1.0, 1024.0)
LEFT_OUT = 37  # samples of the trajectory that the minibatch leaves out
STEP = 5


def all_masked_rows(n):
    """The cases carry rows without a legal action from five actions on."""
    return n >= 5


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def mat_sample_case(n, B, A, row_offset):
    rng = np.random.default_rng([5100, n, B, A])
    rows = B * A
    logits = f32(rng.standard_normal((rows, n)) * 1.5)
    mask, one, none = sm._mask(rng, (B, A), n, all_masked_rows(n))
    flat = mask.reshape(rows, n)  # a view: the edits below reach mask
    # exact ties (seq_model.sample_case): a whole row of equal logits, and a tie of the two largest with the lower index first
    logits[5] = np.float32(0.25)
    if n > 2:
        logits[6] = np.float32(-1.0)
        logits[6, [n - 2, n - 1]] = np.float32(2.0)
        flat[6, [n - 2, n - 1]] = True
    a, gap, f32_diff = sm.sample_discrete(logits, flat, sm.SEED, STEP, row_offset)  # Philox row id = row_offset + b * A + agent
    return dict(n=n, B=B, A=A, rows=rows, row_offset=row_offset, step=STEP, logits=logits, mask=mask, one_legal=one, all_masked=none,
                sampled=a, gap=gap, f32_diff=f32_diff, greedy=sm.greedy_discrete(logits, flat), logp=sm.log_probs(logits, flat))


def mask_read_at_sample(c):
    """The WRONG layout that takes row b * A + j's flags at mask + b * n, as a (B, n) mask would be read."""
    flat = c["mask"].reshape(c["rows"], c["n"])
    return flat[np.arange(c["rows"]) // c["A"]]


def mask_read_at_t32(c):
    """The WRONG layout that takes flag o of row r where a T32 matrix keeps it."""
    rows, n, pad = c["rows"], c["n"], c32(c["rows"])
    store = np.ones(pad * n, bool)
    store[: rows * n] = c["mask"].reshape(-1)
    r, o = np.arange(rows)[:, None], np.arange(n)[None]
    return store[((r >> 5) * n + o) * 32 + (r & 31)]


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def _spread(Bm, k):
    """k distinct minibatch samples from the first to the last."""
    return [0] * k if k < 2 else [round(i * (Bm - 1) / (k - 1)) for i in range(k)]


def _clear(x, edges):
    return min(float(np.abs(np.asarray(x) - e).min()) for e in edges)


@lru_cache(maxsize=None)
def mat_loss_case(n, Bm, A, constant_adv=False, masked=True, left_out_adv=None):
    """Trajectory arrays over TE = Bm + 37 samples and one minibatch of Bm of them.  left_out_adv: the advantage of every sample that
    the minibatch leaves out (a kernel that summed other rows than the loss reads would shift the mean)."""
    TE, R = Bm + LEFT_OUT, Bm * A
    for draw in range(64):  # the first draw that stays CLIP_CLEAR from the clip boundaries
        rng = np.random.default_rng([7100, n, Bm, A, draw])
        idx = rng.permutation(TE)[:Bm].astype(np.int32)
        ext = (idx[:, None].astype(np.int64) * A + np.arange(A)[None]).reshape(-1)  # trajectory row of minibatch row q
        raw, one, none = sm._mask(rng, (TE, A), n, all_masked_rows(n))
        # the samples that hold the special rows move to samples the minibatch selects, spread from its first to its last
        src = sorted({r // A for r in one + none})
        dst = [int(idx[p]) for p in _spread(Bm, len(src))]
        mask = np.empty_like(raw)
        mask[dst] = raw[src]
        mask[np.setdiff1d(np.arange(TE), dst)] = raw[np.setdiff1d(np.arange(TE), src)]
        row_of = lambda r: _spread(Bm, len(src))[src.index(r // A)] * A + r % A  # minibatch row of raw's flat row r
        one_q, none_q = [row_of(r) for r in one], [row_of(r) for r in none]
        mflat = mask.reshape(TE * A, n)
        action = rng.integers(0, n, (TE, A)).astype(np.int32)
        af = action.reshape(-1)
        for r in range(TE * A):
            if mflat[r].any() and not mflat[r, af[r]]:
                af[r] = np.flatnonzero(mflat[r])[rng.integers(0, mflat[r].sum())]
        if not masked:
            mask, mflat, one_q, none_q = None, None, [], []
        logits, values = f32(rng.standard_normal((R, n)) * 1.5), f32(rng.standard_normal(R))
        mrows = None if mflat is None else mflat[ext]
        lp_now = sm.log_probs(logits, mrows)[np.arange(R), af[ext]]
        # rows outside the minibatch hold plausible values of their own: a read of the wrong row is a wrong number, not a fault
        old_lp = f32(rng.standard_normal((TE, A)) * 0.3 - 1.5)
        old_value, target = f32(rng.standard_normal((TE, A))), f32(rng.standard_normal((TE, A)))
        old_lp.reshape(-1)[ext] = lp_now + rng.standard_normal(R) * 0.25
        old_value.reshape(-1)[ext] = values + rng.standard_normal(R) * 0.2
        target.reshape(-1)[ext] = values + rng.standard_normal(R)
        adv = np.full((TE, A), 0.5, np.float32) if constant_adv else f32(rng.standard_normal((TE, A)) * 2 + 0.3)
        if left_out_adv is not None:
            adv[np.setdiff1d(np.arange(TE), idx)] = np.float32(left_out_adv)
        ratio = np.exp(lp_now - f64(old_lp.reshape(-1)[ext]))
        edge = min(_clear(ratio, (1 - sm.CLIP, 1 + sm.CLIP)), _clear(f64(values) - f64(old_value.reshape(-1)[ext]), (-sm.CLIP, sm.CLIP)))
        if edge >= sm.CLIP_CLEAR:
            break
    else:
        raise AssertionError("no draw clear of the clip boundaries")
    c = dict(n=n, Bm=Bm, A=A, TE=TE, R=R, rows=c32(R), idx=idx, ext=ext, mask=mask, action=action, old_lp=old_lp, adv=adv,
             old_value=old_value, target=target, logits=logits, values=values, one_legal=one_q, all_masked=none_q, draw=draw, edge=edge,
             mask_rows=mrows, action_rows=af[ext], old_lp_rows=old_lp.reshape(-1)[ext], adv_rows=adv.reshape(-1)[ext],
             old_value_rows=old_value.reshape(-1)[ext], target_rows=target.reshape(-1)[ext])
    c["stats"] = sm.adv_stats(c["adv_rows"])
    c.update(loss_reference(c))
    return c


def loss_reference(c, ext=None, mask_ext=None):
    """Means over the Bm * A agent rows: actor_loss, entropy, value_loss, dlogits (R, n), dvalues (R,) with vf_coef inside.
    ext / mask_ext: the trajectory rows to read instead (the WRONG indexings of tests/test_mat_kernel_model.py)."""
    ext = c["ext"] if ext is None else ext
    mask_ext = ext if mask_ext is None else mask_ext
    g = lambda k: c[k].reshape(-1)[ext]
    mrows = None if c["mask"] is None else c["mask"].reshape(-1, c["n"])[mask_ext]
    la, ent, dz = sm.actor_loss(c["logits"], mrows, g("action"), g("old_lp"), c["adv_rows"])
    vl, dv = sm.critic_loss(c["values"], g("old_value")[:, None], g("target")[:, None])
    return dict(actor_loss=la, entropy=ent, value_loss=vl, dlogits=dz, dvalues=dv)


def loss_f32_error(c):
    """Largest relative distance (conftest.assert_close's form) of the float32 NumPy evaluation of the gradient formulas from
    float64: how far float32 arithmetic alone lies from the reference at this width."""
    d = np.float32
    logits, R, n = c["logits"], c["R"], c["n"]
    z = logits if c["mask_rows"] is None else np.where(c["mask_rows"], logits, d(po.F32_MIN))
    s = z - z.max(-1, keepdims=True)
    logp = s - np.log(np.exp(s).sum(-1, keepdims=True, dtype=d))
    p = np.exp(logp)
    ent = -np.where(p > 0, p * logp, d(0)).sum(-1, dtype=d)
    adv = c["adv_rows"].astype(d)
    g = (adv - adv.mean(dtype=d)) / (adv.std(dtype=d) + d(1e-8))
    ratio = np.exp(logp[np.arange(R), c["action_rows"]] - c["old_lp_rows"].astype(d))
    lo, hi = d(1 - sm.CLIP), d(1 + sm.CLIP)
    l1, l2 = ratio * g, np.clip(ratio, lo, hi) * g
    g1 = np.where(l1 < l2, d(1), np.where(l1 == l2, d(0.5), d(0)))
    dlp = -(g1 * g + (d(1) - g1) * g * ((ratio >= lo) & (ratio <= hi))) / d(R) * ratio
    oh = np.zeros_like(z)
    oh[np.arange(R), c["action_rows"]] = 1
    dz = dlp[:, None] * (oh - p) + d(sm.ENT_COEF) / d(R) * p * (np.where(p > 0, logp, d(0)) + ent[:, None])
    if c["mask_rows"] is not None:
        dz = np.where(c["mask_rows"], dz, d(0))
    assert dz.dtype == d
    v, ov, tg = c["values"], c["old_value_rows"], c["target_rows"]
    diff = v - ov
    vclip = ov + np.clip(diff, d(-sm.CLIP), d(sm.CLIP))
    v1, v2 = (v - tg) ** 2, (vclip - tg) ** 2
    h1 = np.where(v1 > v2, d(1), np.where(v1 == v2, d(0.5), d(0)))
    dv = d(sm.VF_COEF) * (h1 * (v - tg) + (d(1) - h1) * (vclip - tg) * ((diff >= d(-sm.CLIP)) & (diff <= d(sm.CLIP)))) / d(R)
    assert dv.dtype == d
    return max(_rel_err(dz, c["dlogits"]), _rel_err(dv, c["dvalues"]))


def _rel_err(a, b):
    """seq_model.rel_err; an entry of an all-zero reference (one action: dlogits = 0) counts by its absolute error."""
    a, b = f64(a), f64(b)
    den = np.abs(b) + np.sqrt(np.mean(b * b))
    return float((np.abs(a - b) / np.where(den > 0, den, 1.0)).max())
