"""Case tables of tests/test_gpu_instances.py and a Python restatement of the host dispatch of the feed-forward kernels
(csrc/ppo_train.hip, ppo_train_h2.hip, ppo_train_w8.hip, mlp_policy.hip, mlp_coop.hip): which template instance a shape must
reach, as the integer that mava_debug_train_last_instance() / mava_debug_policy_last_instance() report (DESIGN.md §"No
process-wide state").  Plain NumPy and the float64 oracle only: tests/test_instances_table.py checks the tables without a GPU."""
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

from oracle import philox, ppo_oracle as po, tanh_normal as tn

LDS_BYTES = 163840  # the 160 KiB of a CU
F32, H2, W8 = 1, 2, 3  # gradient kernel families
HYBRID, PER_WAVE, COOP, FORWARD = 1, 2, 3, 4  # acting kernels
MODE_RAW, MODE_SAMPLE, MODE_VALUE = 0, 1, 2  # mlp_coop_body.h


# ------------------------------------------------------------------------------------------ instance ids
def train_id(family, actor, cont, wide, no, k, xv):
    """ppo_train_task.h train_instance_id; k = KT1 (exact f32) or S1 (h2, w8)."""
    return family * 1000000 + (int(actor) + 2 * int(cont) + 4 * int(wide)) * 100000 + no * 1000 + k * 10 + xv


def policy_id(kernel, mode, no, kt1):
    """mlp_coop_body.h policy_instance_id."""
    return kernel * 100000 + mode * 10000 + no * 100 + kt1


# ------------------------------------------------------------------------------- dispatch restatement
def head_bucket(n):
    """The NO / NOA template argument of a head of n outputs (actor and continuous head; the forward kernels add NO = 1)."""
    return 8 if n <= 8 else (16 if n <= 16 else 32)


def aligned(offset_floats, nbytes):
    """Alignment of a float pointer `offset_floats` floats into an allocation (allocations are aligned to 256 bytes)."""
    return (4 * offset_floats) % nbytes == 0


def f32_lds_bytes(no, kt1):
    """make_layout<NO>(KT1) of ppo_train.hip with MLP_LDW = 129, LDT = 33: the bytes of LDS the exact-f32 kernel cannot do
    without (the private dz1^T tile is only taken when it fits)."""
    tile = 128 * 33
    mlp_end = 128 * 129 + 128 * no + 128 + 128 + ((no + 3) & ~3)
    yp = mlp_end + 3 * tile
    dy = yp + 4 * 32 * (no + 1)
    xs = (dy + 32 * 33 + 3) & ~3
    return 4 * (xs + 32 * (32 * kt1 + 4) + 16)


_PAD_KT = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 9, 8: 9, 9: 9}  # 32-input tiles -> the instantiated count


class Prediction(NamedTuple):
    instance: Optional[int]  # None: refused by an argument error before any launch
    refusal: Optional[str]   # a word of the error message
    h2_launches: int         # MAVA_CTX_H2_LAUNCHES after one launch on a fresh handle
    w8_launches: int


def _f32(actor, cont, no, din, offset):
    kt = din // 32 + 1  # dispatch_kt: 32 * kt > din leaves a column for the ones input
    if kt not in _PAD_KT:
        return Prediction(None, "not instantiated", 0, 0)
    kt1 = _PAD_KT[kt]
    if f32_lds_bytes(no, kt1) > LDS_BYTES:
        return Prediction(None, "LDS", 0, 0)
    xv = 4 if (kt1 >= 4 and din % 4 == 0 and din >= 96 and aligned(offset, 16)) else 1  # pick_xv + launch_xv
    return Prediction(train_id(F32, actor, cont, False, no, kt1, xv), None, 0, 0)


def _w8(actor, no, din, offset, aggregated):
    """mava_train_w8_launch: the instance id, or None when the four-wave kernels take the shape."""
    if din + 1 > 128 or (actor and no > 16) or (not actor and aggregated):
        return None
    s1 = (din + 32) // 32
    if din % 2 == 0 and aligned(offset, 8):
        xv = 2
    elif s1 == 4:  # 97 .. 127 inputs one float at a time: left to the four-wave kernel
        return None
    else:
        xv = 1
    return train_id(W8, actor, False, False, no if actor else 8, s1, xv)  # (the critic runs the NO = 8 body)


def h2_lds_bytes(s1, wide, actor):
    """make_h2_layout<NO, S1, WIDE>(actor) of ppo_train_h2.hip (it does not depend on NO): seven f16 hi/lo images of 32 x 272
    bytes (h1, dz2, dz1, four of W2), the x tile (one buffer WIDE, else two; hi and lo plane), the actor's dy planes, the
    aggregation rows and the small f32 arrays."""
    img = 2 * 32 * 272
    xs_plane = 32 * (2 * 32 * ((s1 + 1) // 2) + 16)
    dy = 7 * img + (1 if wide else 2) * 2 * xs_plane
    small = (dy + (2 * 32 * 80 if actor else 0) + 8 * 33 * 4 + 15) & ~15
    return small + (128 + 32 + 16 + 128) * 4


def _h2(actor, no, din, offset):
    """dispatch_s1 / dispatch_xv of ppo_train_h2.hip: the instance id, None for input widths above 287, or the refusal of
    launch_h2 when the layout exceeds the LDS (the ACTOR's 18-step WIDE instance: 167 136 bytes)."""
    s1 = (din + 16) // 16
    if s1 > 18:
        return None
    wide = s1 >= 7
    k = s1 if not wide else (12 if s1 <= 12 else 18)
    if h2_lds_bytes(k, wide, actor) > LDS_BYTES:
        return Prediction(None, "LDS", 0, 0)
    if wide:
        xv = 4 if (din % 4 == 0 and aligned(offset, 16)) else 1
    else:
        xv = 2 if (din % 2 == 0 and aligned(offset, 8)) else 1
    return train_id(H2, actor, False, wide, no, k, xv)


def predict_actor(mode, variant, din, n_actions, offset=0):
    """mava_ppo_actor_grad_f32.  mode: "f32" | "f16x2"; variant: MAVA_CTX_TRAIN_VARIANT bit 0 (1 = four-wave kernels only)."""
    no = head_bucket(n_actions)
    if mode == "f16x2":
        if variant & 1 == 0:
            i = _w8(True, no, din, offset, False)
            if i is not None:
                return Prediction(i, None, 1, 1)
        i = _h2(True, no, din, offset)
        if isinstance(i, Prediction):
            return i
        if i is not None:
            return Prediction(i, None, 1, 0)
    return _f32(True, False, no, din, offset)


def critic_aggregated(agg_setting, A, x_share):
    """mava_ppo_critic_grad_f32: the A agents of an index are folded into their shared input row."""
    return bool(agg_setting) and 1 < A <= 8 and x_share == A


def predict_critic(mode, variant, din, agg_setting, A, x_share, offset=0):
    aggregated = critic_aggregated(agg_setting, A, x_share)
    if mode == "f16x2":
        if variant & 1 == 0:
            i = _w8(False, 1, din, offset, aggregated)
            if i is not None:
                return Prediction(i, None, 1, 1)
        i = _h2(False, 1, din, offset)
        if isinstance(i, Prediction):
            return i
        if i is not None:
            return Prediction(i, None, 1, 0)
    return _f32(False, False, 1, din, offset)


def predict_continuous(din, dim, offset=0):
    """mava_ppo_actor_grad_continuous_f32: exact f32 only, NO = 8 up to 8 action dimensions, 16 above."""
    return _f32(True, True, 8 if dim <= 8 else 16, din, offset)


def coop_kt(din):
    kt = (din + 31) // 32
    return _PAD_KT.get(kt)


def predict_policy_step(variant, actor_din, n_actions, critic_din, rows, critic_rows):
    """policy_step_impl: (the instance that carries the actor rows, the instance of the LAST launch of the call)."""
    noa = head_bucket(n_actions)
    if variant == 2 and actor_din <= 288 and critic_din <= 288:
        a = policy_id(COOP, MODE_SAMPLE, noa, coop_kt(actor_din))
        return a, (policy_id(COOP, MODE_VALUE, 1, coop_kt(critic_din)) if critic_rows > 0 else a)
    tiles_c = (critic_rows + 31) // 32
    if variant == 0 and rows > 0 and critic_rows > 0 and tiles_c <= 128 and critic_din <= 287:
        i = policy_id(HYBRID, 0, noa, coop_kt(critic_din))
    else:
        i = policy_id(PER_WAVE, 0, noa, 0)
    return i, i


def predict_forward(variant, din, n_out):
    no = 1 if n_out == 1 else head_bucket(n_out)
    if variant == 2 and din <= 288:
        return policy_id(COOP, MODE_RAW, no, coop_kt(din))
    return policy_id(FORWARD, 0, no, 0)


# ------------------------------------------------------------------------------------------- case tables
TE, A, RB, N_SLAB = 40, 2, 37, 2  # 74 agent rows: three 32-row tiles, the last ragged; two blocks with unequal tile counts
SENTINEL = 3.0                    # slabs start at this value: an entry the kernel forgets, or adds into, misses the oracle

H2_WIDTHS = (8, 20, 37, 50, 70, 85, 96, 191, 192, 287)  # s1 = 1 2 3 4 5 6 | 7 12 (WIDE 12) | 13 18 (WIDE 18); odd and even
H2_ACTOR_WIDTHS = H2_WIDTHS[:8]  # the actor's WIDE 18 layout does not fit the LDS: its f16x2 envelope ends at 191 inputs
H2_OTHER_PARITY = (7, 21, 36, 51, 71, 86)                # s1 = 1 .. 6 again, at the other vector width


class ActorCase(NamedTuple):
    mode: str       # "f32": exact f32, no handle; "f16x2": Ctx("f16x2")
    variant: int    # MAVA_CTX_TRAIN_VARIANT (f16x2 only)
    n_actions: int
    din: int
    offset: int = 0  # floats between the allocation and the first input


class CriticCase(NamedTuple):
    mode: str
    variant: int
    din: int
    shared: bool    # the A agents of an index read one input row (x_share = A)
    agg: int        # MAVA_CTX_CRITIC_AGGREGATION
    offset: int = 0


class ContinuousCase(NamedTuple):
    dim: int
    din: int


def _actor_cases():
    c = []
    # four-wave h2: every action bucket x every step count, then the bucket edges at 70 inputs
    c += [ActorCase("f16x2", 1, nA, din) for nA in (3, 14, 20) for din in H2_ACTOR_WIDTHS]
    c += [ActorCase("f16x2", 1, nA, 70) for nA in (8, 9, 16, 17, 32)]
    c += [ActorCase("f16x2", 1, nA, din) for nA in (3, 14, 20) for din in H2_OTHER_PARITY]
    # eight-wave w8: s1 = 1, 2, 3 at both vector widths, s1 = 4 at an even width
    c += [ActorCase("f16x2", 0, nA, din) for nA in (3, 14) for din in (8, 7, 50, 37, 70, 85, 100)]
    # ... and the two shapes it hands to the four-wave kernels: an odd width in 97..127, more than 16 actions
    c += [ActorCase("f16x2", 0, 3, 101), ActorCase("f16x2", 0, 14, 101), ActorCase("f16x2", 0, 20, 70)]
    # exact f32: NO = 8 at kt = 1..6, NO = 16 at kt = 1..4, NO = 32 at kt = 1; both vector widths from kt = 4 on
    c += [ActorCase("f32", 0, 3, din) for din in (8, 37, 70, 100, 101, 132, 130, 160, 191)]
    c += [ActorCase("f32", 0, 14, din) for din in (8, 37, 70, 100, 127)]
    c += [ActorCase("f32", 0, 20, din) for din in (8, 31)]
    # the first width past the exact-f32 envelope of NO = 16 and of NO = 32 runs in f16x2 (default variant)
    c += [ActorCase("f16x2", 0, nA, din) for nA, din in ACTOR_F32_REFUSED if din < 192]
    # an even width one float into its allocation: h2 narrow, h2 WIDE, w8, exact f32 at kt >= 4
    c += [ActorCase("f16x2", 1, 3, 70, 1), ActorCase("f16x2", 1, 14, 96, 1), ActorCase("f16x2", 0, 3, 70, 1),
          ActorCase("f32", 0, 3, 100, 1)]
    return c


ACTOR_F32_REFUSED = ((3, 192), (14, 128), (20, 32))  # (n_actions, din): the first width past the LDS envelope of each NO
# ... and of the f16x2 kernels, whatever NO: both ends of the WIDE 18 instance's range, with and without the eight-wave kernel
ACTOR_F16X2_REFUSED = ((1, 3, 192), (1, 14, 192), (1, 20, 192), (1, 20, 287), (0, 3, 192))  # (variant, n_actions, din)
ACTOR_CASES = _actor_cases()


def _critic_cases():
    c = []
    three = ((True, 1), (True, 0), (False, 1))  # shared + aggregated, shared + one pass per agent row, own input rows
    c += [CriticCase("f16x2", 1, din, sh, agg) for din in H2_WIDTHS for sh, agg in three]
    # w8 serves the value network only without aggregation; the aggregated launch falls through to h2
    c += [CriticCase("f16x2", 0, din, sh, agg) for din in (8, 37, 70, 100) for sh, agg in three]
    # exact f32: kt = 1 2 3 4 5 6 7 8 9 (5 runs on the 6 instance, 7 and 8 on the 9 instance)
    c += [CriticCase("f32", 0, din, sh, agg) for din in (8, 37, 70, 100, 130, 160, 200, 230, 264) for sh, agg in three]
    c += [CriticCase("f16x2", 1, din, False, 1) for din in H2_OTHER_PARITY]
    c += [CriticCase("f16x2", 0, din, False, 1) for din in (7, 50, 85)]  # w8 s1 = 1, 2, 3 at the other vector width
    c += [CriticCase("f16x2", 1, 70, True, 1, 1), CriticCase("f16x2", 1, 96, True, 1, 1), CriticCase("f16x2", 0, 70, False, 1, 1),
          CriticCase("f32", 0, 100, True, 1, 1)]
    return c


CRITIC_CASES = _critic_cases()

# dim 9 runs the NO = 16 body, whose LDS ends at kt = 4: kt = 5 (widths from 128) is refused
CONTINUOUS_CASES = ([ContinuousCase(2, din) for din in (8, 37, 70, 100, 101, 130, 132)]
                    + [ContinuousCase(9, din) for din in (8, 37, 70, 100, 101)])
CONTINUOUS_REFUSED = ((9, 128), (9, 130), (2, 192))  # (dim, din)


def case_id(c):
    return "-".join(str(v) for v in c)


def _net(rng, din, no, bias_noise=0.1):
    p = po.init_mlp(rng, din, no, 1.0)
    p = p._replace(b1=rng.standard_normal(128) * bias_noise, b2=rng.standard_normal(128) * bias_noise,
                   b3=rng.standard_normal(no) * bias_noise)
    return po.mlp_flatten(p).astype(np.float32)


def _seed(c):
    return [int(v) if not isinstance(v, str) else len(v) for v in c]


def _minibatch(rng):
    idx = rng.permutation(TE)[:RB].astype(np.int32)
    rows_sel = (idx[:, None].astype(np.int64) * A + np.arange(A)).reshape(-1)
    return idx, rows_sel


@lru_cache(maxsize=None)
def actor_data(c: ActorCase):
    """Inputs of one discrete actor gradient case and the float64 oracle on the selected rows."""
    rng = np.random.default_rng([1] + _seed(c))
    rows, din, nA = TE * A, c.din, c.n_actions
    av = rng.standard_normal((rows, din)).astype(np.float32)
    mask = rng.random((rows, nA)) > 0.25
    action = rng.integers(0, nA, rows).astype(np.int32)
    mask[np.arange(rows), action] = True
    idx, rows_sel = _minibatch(rng)
    one = rows_sel[5]  # a selected row with a single legal action
    mask[one] = False
    mask[one, action[one]] = True
    mask[rows_sel[9]] = False  # a selected row without a legal action: uniform over its nA actions, no gradient into its logits
    adv = (rng.standard_normal(rows) * 2.0 + 0.3).astype(np.float32)
    flat = _net(rng, din, nA)
    # old log-probs close to the current ones: both sides of the clip range
    y = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, nA), av.astype(np.float64))
    lsm = po.log_softmax(po.masked_logits(y, mask))
    old_lp = (lsm[np.arange(rows), action] + rng.standard_normal(rows) * 0.25).astype(np.float32)
    args = (flat.astype(np.float64), din, nA, av[rows_sel].astype(np.float64), mask[rows_sel], action[rows_sel],
            old_lp[rows_sel].astype(np.float64), adv[rows_sel].astype(np.float64), 0.2, 0.01)
    _, la, ent, g = po.actor_loss_and_grad(*args)
    ratio = np.exp(lsm[rows_sel, action[rows_sel]] - old_lp[rows_sel])
    return dict(flat=flat, av=av, mask=mask, action=action, old_lp=old_lp, adv=adv, idx=idx, rows_sel=rows_sel,
                oracle_args=args, grad=g, sums=np.array([la, ent]), ratio=ratio)


@lru_cache(maxsize=None)
def critic_data(c: CriticCase):
    rng = np.random.default_rng([2] + _seed(c))
    rows, din = TE * A, c.din
    share = A if c.shared else 1
    gs = rng.standard_normal((rows // share, din)).astype(np.float32)
    idx, rows_sel = _minibatch(rng)
    flat = _net(rng, din, 1)
    v_now = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), din, 1), gs.astype(np.float64))[:, 0]
    v_rows = v_now[np.arange(rows) // share]
    old_v = (v_rows + rng.standard_normal(rows) * 0.2).astype(np.float32)  # both sides of the clip range
    tgt = (v_rows + rng.standard_normal(rows)).astype(np.float32)
    args = (flat.astype(np.float64), din, gs[rows_sel // share].astype(np.float64), old_v[rows_sel].astype(np.float64),
            tgt[rows_sel].astype(np.float64), 0.2, 0.5)
    _, vl, g = po.critic_loss_and_grad(*args)
    return dict(flat=flat, gs=gs, share=share, old_v=old_v, tgt=tgt, idx=idx, rows_sel=rows_sel, oracle_args=args, grad=g,
                sums=np.array([vl, 0.0]), diff=(v_rows - old_v.astype(np.float64))[rows_sel])


CONT_SEED, CONT_ENT_STEP, CONT_ROW_OFFSET = 99, 12345, 777


@lru_cache(maxsize=None)
def continuous_data(c: ContinuousCase):
    rng = np.random.default_rng([3] + _seed(c))
    rows, din, dim = TE * A, c.din, c.dim
    flat = np.concatenate([_net(rng, din, dim, bias_noise=0.0), (rng.normal(size=dim) * 0.4).astype(np.float32)])
    av = rng.standard_normal((rows, din)).astype(np.float32)
    fm, ls = tn.split_params(flat.astype(np.float64), din, dim)
    mean64 = po.mlp_forward(po.mlp_unflatten(fm, din, dim), av.astype(np.float64))
    action = np.tanh(mean64 + tn.scale_of(ls) * rng.standard_normal((rows, dim))).astype(np.float32)
    action[rng.random((rows, dim)) < 0.02] = 0.9995  # some actions in the clipped tails
    action[rng.random((rows, dim)) < 0.02] = -1.0
    old_lp = (tn.log_prob(action.astype(np.float64), mean64, ls) + rng.standard_normal(rows) * 0.25).astype(np.float32)
    adv = rng.standard_normal(rows).astype(np.float32)
    idx, rows_sel = _minibatch(rng)
    eps = tn.normal_noise(CONT_SEED, CONT_ENT_STEP, 0, dim, tn.STREAM_ENTROPY, row_offset=CONT_ROW_OFFSET, gid=rows_sel).astype(np.float64)
    args = (flat.astype(np.float64), din, dim, av[rows_sel].astype(np.float64), action[rows_sel].astype(np.float64),
            old_lp[rows_sel].astype(np.float64), adv[rows_sel].astype(np.float64), 0.2, 0.01, eps)
    _, la, ent, g = tn.actor_loss_and_grad(*args)
    return dict(flat=flat, av=av, action=action, old_lp=old_lp, adv=adv, idx=idx, rows_sel=rows_sel, oracle_args=args, grad=g,
                sums=np.array([la, ent]))


def continuous_f32_error(c: ContinuousCase):
    """How far a float32 NumPy run of tanh_normal.actor_loss_and_grad lies from the float64 one on the case's rows, in the
    form of conftest.assert_close: max |g32 - g64| / (|g64| + rms(g64))."""
    d = continuous_data(c)
    g32 = tn.actor_loss_and_grad(*d["oracle_args"], dtype=np.float32)[3]
    assert g32.dtype == np.float32
    g = d["grad"]
    return float((np.abs(g32 - g) / (np.abs(g) + np.sqrt(np.mean(g * g)))).max())


# The gradient tolerance is 1e-4 for every case but the ones listed here, where a float32 NumPy run of the oracle itself misses
# 1e-4 of the float64 one (continuous_f32_error, re-measured by tests/test_instances_table.py): the case's tolerance is four
# times that measured error.  (2 dimensions, 130 inputs): 1.094e-4, at one dW3 entry.  One of the rows whose action the case
# puts into the clipped tail (-1.0) has its mean 7.5 scales away (mean 2.2, scale 0.80): the tail's d log_prob / d mean is the
# ratio pdf / cdf = exp(-z^2 / 2 - log Phi(z) - c) of two terms near 28 and -31 that cancel, so float32 carries it to 4e-6
# relative, 4e-5 absolute on a value of -9.5 - whatever evaluates the formula in float32 (the kernel: 1.36e-4 at that entry).
CONTINUOUS_F32_MEASURED = {ContinuousCase(2, 130): 1.094e-4}


def continuous_grad_tolerance(c: ContinuousCase):
    return 4.0 * CONTINUOUS_F32_MEASURED[c] if c in CONTINUOUS_F32_MEASURED else 1e-4


# ------------------------------------------------------------------------------------------ acting kernels
E_ACT, A_ACT = 33, 3  # 99 actor rows, 33 critic input rows
ACT_N_ACTIONS = (1, 8, 9, 16, 17, 32)
HYBRID_WIDTHS = (24, 60, 96, 100, 150, 192, 200, 264)  # critic widths: (din + 31) // 32 = 1 2 3 4 5 6 7 9
GAP = 1e-3  # smallest top-two score gap of the float64 oracle at which a float32 argmax must agree (score error ~1e-5)


class StepCase(NamedTuple):
    variant: int      # MAVA_CTX_POLICY_VARIANT
    n_actions: int
    actor_din: int
    critic_din: int
    rows: int = E_ACT * A_ACT
    critic_in_rows: int = E_ACT  # rows of the critic input; share = rows // critic_in_rows when that divides, else 1
    head_scale: float = 1.0


class ForwardCase(NamedTuple):
    variant: int
    n_out: int
    din: int
    rows: int = 99


def _step_cases():
    c = []
    actor_dins = (23, 70, 12)  # one, two and four floats per load in the per-wave actor
    # default: hybrid launch, every NOA x every critic step count (5 on the 6 instance, 7 on the 9 instance), and the
    # per-wave kernel for a critic wider than 287
    for i, nA in enumerate(ACT_N_ACTIONS):
        c += [StepCase(0, nA, actor_dins[(i + j) % 3], w) for j, w in enumerate(HYBRID_WIDTHS + (300,))]
    c += [StepCase(0, 5, 70, 250)]  # (din + 31) // 32 = 8 on the 9 instance
    c += [StepCase(1, nA, actor_dins[i % 3], w) for i, nA in enumerate(ACT_N_ACTIONS) for w in (24, 300)]
    # block-cooperative kernels: the ACTOR's width picks KT1 too; more than 16 actions dispatch the NO = 32 body
    c += [StepCase(2, nA, w, HYBRID_WIDTHS[(i + j) % 8]) for i, nA in enumerate(ACT_N_ACTIONS) for j, w in enumerate(HYBRID_WIDTHS)]
    c += [StepCase(2, 5, 250, 250), StepCase(2, 5, 70, 300)]  # 300 > 288: back on the per-wave kernel
    # more than 128 actor blocks' worth of rows in the hybrid launch (its tile loop wraps), and 129 critic tiles (per-wave)
    c += [StepCase(0, 2, 8, 8, rows=16384 + 37, critic_in_rows=33, head_scale=10.0),
          StepCase(0, 5, 8, 8, rows=99, critic_in_rows=4097)]
    return c


def _forward_cases():
    c = [ForwardCase(0, n, 70) for n in ACT_N_ACTIONS]
    c += [ForwardCase(0, 5, 300), ForwardCase(0, 5, 8, rows=65536 + 33)]  # more than 512 blocks' worth of rows: the loop wraps
    c += [ForwardCase(2, n, w) for n in ACT_N_ACTIONS for w in (24, 60, 96, 100, 192, 264)]
    c += [ForwardCase(2, 5, w) for w in (150, 200, 250)] + [ForwardCase(2, 5, 300)]
    return c


STEP_CASES = _step_cases()
FORWARD_CASES = _forward_cases()
STEP_NUMBER, ROW_OFFSET = 5, 7
NONE_LEGAL_ROW = 6


def top_two_gap(scores):
    if scores.shape[1] == 1:
        return np.full(scores.shape[0], np.inf)
    s = np.sort(scores, axis=1)
    return s[:, -1] - s[:, -2]


@lru_cache(maxsize=None)
def step_data(c: StepCase):
    """Inputs of one acting-step case and everything the float64 oracle says about it.  The inputs are the first draw (of 16)
    whose masked logits have a top-two gap >= GAP on every row, the sampling seed the first of range(64) whose Gumbel scores
    do: the float32 kernel must then pick the oracle's actions on EVERY row.  `None` where no such draw / seed exists."""
    nA, rows = c.n_actions, c.rows
    share = rows // c.critic_in_rows if rows % c.critic_in_rows == 0 else 1
    for draw in range(16):
        rng = np.random.default_rng([4, draw] + _seed(c))
        p = po.init_mlp(rng, c.actor_din, nA, c.head_scale)
        fa = po.mlp_flatten(p._replace(b1=rng.standard_normal(128) * 0.1, b2=rng.standard_normal(128) * 0.1,
                                       b3=rng.standard_normal(nA) * 0.1)).astype(np.float32)
        fc = _net(rng, c.critic_din, 1)
        av = rng.standard_normal((rows, c.actor_din)).astype(np.float32)
        gs = rng.standard_normal((c.critic_in_rows, c.critic_din)).astype(np.float32)
        mask = rng.random((rows, nA)) > 0.2
        mask[:, 0] = True
        mask[3, :] = False  # a row with a single legal action, not the first one
        mask[3, nA // 2] = True
        mask[NONE_LEGAL_ROW, :] = False  # a row without a legal action: an exact tie at finfo.min, the first index wins
        dec = np.arange(rows) != NONE_LEGAL_ROW
        y = po.mlp_forward(po.mlp_unflatten(fa.astype(np.float64), c.actor_din, nA), av.astype(np.float64))
        z = po.masked_logits(y, mask)
        if top_two_gap(z)[dec].min() >= GAP:
            break
    else:
        return None
    lsm = po.log_softmax(z)
    seed = None
    for s in range(64):
        u = philox.policy_uniforms(s, STEP_NUMBER, rows, nA, row_offset=ROW_OFFSET)
        sc = z + -np.log(-np.log(u.astype(np.float64)))
        if top_two_gap(sc)[dec].min() >= GAP:
            seed = s
            break
    if seed is None:
        return None
    sampled = np.argmax(sc, axis=-1).astype(np.int32)
    v = po.mlp_forward(po.mlp_unflatten(fc.astype(np.float64), c.critic_din, 1), gs.astype(np.float64))[:, 0]
    forced = ((sampled + 1 + np.arange(rows)) % nA).astype(np.int32)  # other actions than the sampled ones, legal or not
    forced = np.where(mask[np.arange(rows), forced], forced, sampled).astype(np.int32)
    forced[NONE_LEGAL_ROW] = nA - 1  # every action of that row has log_prob = -log(nA)
    return dict(fa=fa, fc=fc, av=av, gs=gs, mask=mask, share=share, seed=seed, logits=y, lsm=lsm, sampled=sampled,
                greedy=np.argmax(z, axis=-1).astype(np.int32), value=v, forced=forced, one_legal_row=3, none_legal_row=NONE_LEGAL_ROW)


@lru_cache(maxsize=None)
def forward_data(c: ForwardCase):
    rng = np.random.default_rng([5] + _seed(c))
    flat = _net(rng, c.din, c.n_out)
    x = rng.standard_normal((c.rows, c.din)).astype(np.float32)
    want = po.mlp_forward(po.mlp_unflatten(flat.astype(np.float64), c.din, c.n_out), x.astype(np.float64))
    return dict(flat=flat, x=x, want=want)
