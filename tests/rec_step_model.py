"""TEST INFRASTRUCTURE ONLY.  Case table and float64 references of the fused recurrent ACTING step (csrc/rec_step.hip: the
exact-f32 rec_step_kernel<NOA>; csrc/rec_step_h2.hip: the f16x2 rec_step_h2_kernel<NOA, RT> on pre-packed weights), and a
restatement of the host dispatch - rec_step_impl, mava_rec_step_h2_launch, setup, launch_step - that says which instance a
shape must reach, as the integer mava_debug_rec_step_last_instance() reports (rec_step_task.h).  Plain NumPy and the float64
oracle (oracle/rec_oracle.py, philox.py, tanh_normal.py) only: tests/test_rec_step_model.py checks the table without a GPU,
tests/test_gpu_rec_step.py runs every case through the C ABI.

A case uses every row it launches (the ABI takes rows in multiples of 32): there is no padding row whose wrong result could
go unseen."""
import zlib
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from oracle import philox
from oracle import rec_oracle as ro
from oracle import tanh_normal as tn
from tests import seq_model as sm

H = 128
LDS_BYTES = 163840  # the 160 KiB of a CU
IIMG = 2 * 32 * 272  # rec_step_h2.hip: hi + lo planes of a [32 rows][128 f16 + 16] activation image
CUS = 256
F32, H2 = 1, 2  # kernel families of the instance id
SEED = sm.SEED  # both 32-bit halves in use
STEP = 5
RTOL = 1e-5  # BASELINE.md section 2 form (conftest.assert_close), every compared value
GAP_FACTOR = 4.0  # the margin of test_seq_sample
UNDECIDED_CAP = 0.01
f32, f64 = sm.f32, sm.f64


# ------------------------------------------------------------------------------------------------ dispatch, restated
def step_id(family, noa, k):
    """rec_step_task.h rec_step_instance_id.  k: RT of the f16x2 kernel; 1 / 0 of the f32 kernel = CUs shared out or not."""
    return family * 1000 + noa * 10 + k


def head_bucket(n):
    return 8 if n <= 8 else (16 if n <= 16 else 32)


def pick_rt(ta, tc):
    """mava_rec_step_h2_launch: the smallest RT of 1..3 whose groups cover the chip in one round, else 3."""
    rt = 1
    while rt < 3 and -(-ta // rt) + -(-tc // rt) > CUS:
        rt += 1
    return rt


def h2_net_bytes(din, no, rt):
    """launch_step's la / lc with setup()'s xrow / abytes: RT x (region A + region B) + partial logits + biases."""
    nb1 = (din + 15) // 16
    xrow = 32 * nb1 + 16
    abytes = max(2 * 32 * xrow, IIMG)
    return rt * (abytes + IIMG) + 4 * (rt * 4 * no * 32 + 6 * H + no)


def h2_lds_bytes(n, din_a, din_c, rt):
    """The critic runs the 8-wide head tile."""
    return max(h2_net_bytes(din_a, head_bucket(n), rt), h2_net_bytes(din_c, 8, rt))


def f32_lds_bytes(n, din_a, din_c):
    """carve() of rec_step.hip (LDT = 33): x tile, three [128][33] exchange tiles, the head weights, the partial logits."""
    def net(din, no):
        return 4 * (32 * (16 * ((din + 15) // 16) + 1) + 3 * H * 33 + H * no + 4 * no * 32)

    return max(net(din_a, head_bucket(n)), net(din_c, 1))


def f32_blocks(ta, tc):
    """rec_step_impl: one block per tile up to 256 tiles, else the 256 CUs in proportion to the two networks' tiles."""
    nba, nbc = ta, tc
    if ta + tc > CUS:
        nbc = min(-(-CUS * tc // (ta + tc)), tc) if tc > 0 else 0
        if tc > 0:
            nbc = max(nbc, 1)
        nba = min(CUS - nbc, ta) if ta > 0 else 0
        if ta > 0:
            nba = max(nba, 1)
    return nba, nbc


def f32_instance(n, ta, tc):
    return step_id(F32, head_bucket(n), 1 if ta + tc > CUS else 0)


def predict(packed, n, din_a, din_c, ta, tc):
    """The id the export must report after one launch.  The packed entry runs the f16x2 kernel unless the head is wider than
    16 outputs or launch_step refuses the LDS bytes; then, silently, the exact-f32 kernel."""
    assert f32_lds_bytes(n, din_a, din_c) <= LDS_BYTES
    if packed and ta > 0 and tc > 0 and n <= 16:
        rt = pick_rt(ta, tc)
        if h2_lds_bytes(n, din_a, din_c, rt) <= LDS_BYTES:
            return step_id(H2, head_bucket(n), rt)
    return f32_instance(n, ta, tc)


# ------------------------------------------------------------------------------------------------ case table
class Spec(NamedTuple):
    family: str
    ta: int            # actor row tiles
    tc: int            # critic row tiles
    din_a: int
    din_c: int
    n: int             # actions, or action dimensions of the continuous head
    cont: bool = False
    form: str = "rows"  # critic: "rows" one sequence per row, own inputs and flags; "shared" input row r / A (critic_share = A);
    #                     "env" once per env: rows_c = rows_a / A, flags of agent 0 (done_stride = A), value copied A times
    A: int = 1
    masked: bool = True
    dead_rows: tuple = ()  # rows without a legal action
    row_offset: int = 0
    resets: str = "random"  # none | all | random (30 %) | odd_tiles (every odd tile fully reset, even tiles not)
    greedy: tuple = (0,)   # the greedy flags the GPU test launches
    expect_h2: bool = True  # the packed entry reaches the f16x2 kernel (False: one of its two silent fallbacks)


def _table():
    t = {}
    # heads at RT = 1: 3 tiles per network.  Masked (one row of the first and one of the last tile without a legal action, row
    # offset 1000) and without a mask (offset 0); sampled and greedy
    for n in (1, 2, 8, 9, 16, 17, 32):
        t[f"head{n}_mask"] = Spec("heads", 3, 3, 20, 24, n, dead_rows=(7, 94), row_offset=1000, greedy=(0, 1), expect_h2=n <= 16)
        t[f"head{n}_nomask"] = Spec("heads", 3, 2, 20, 24, n, masked=False, greedy=(0, 1), expect_h2=n <= 16)
    for d in (1, 8, 9, 16):
        t[f"cont{d}"] = Spec("continuous", 3, 2, 20, 24, d, cont=True, row_offset=1000 if d in (8, 16) else 0, greedy=(0, 1))
    # input widths at RT = 1, 2 tiles: nb1 below / at / above the ring depth 6, the fast_x limit 12, the slow x path, widths that
    # are no multiple of 16; the critic sees the same list reversed
    widths = (1, 16, 96, 97, 192, 193, 250)
    for da, dc in zip(widths, widths[::-1]):
        t[f"width{da}_{dc}"] = Spec("widths", 2, 2, da, dc, 5, dead_rows=(33,))
    # critic forms beyond one tile
    t["critic_shared4"] = Spec("critic", 3, 3, 20, 24, 5, form="shared", A=4)
    t["critic_env4"] = Spec("critic", 8, 2, 20, 40, 5, form="env", A=4)
    t["critic_env8"] = Spec("critic", 16, 2, 20, 40, 5, form="env", A=8, masked=False)
    # RT = 2, ragged last group in both networks (193 and 65 tiles), NOA = 16, narrow inputs; the four reset patterns
    for r in ("none", "all", "random", "odd_tiles"):
        t[f"rt2_{r}"] = Spec("rt2", 193, 65, 14, 40, 13, dead_rows=(6175,), resets=r)
    t["rt2_noa8_env"] = Spec("rt2", 256, 64, 14, 40, 5, form="env", A=4, resets="odd_tiles")
    # RT = 3, ragged in both networks (400 = 3 * 133 + 1, 115 = 3 * 38 + 1) at the benchmarked config-4 widths
    t["rt3_config4"] = Spec("rt3", 400, 115, 155, 188, 13, dead_rows=(12799,), row_offset=1000)
    t["rt3_noa8_odd"] = Spec("rt3", 400, 115, 30, 20, 5, resets="odd_tiles")
    t["rt3_cont"] = Spec("rt3", 400, 115, 30, 20, 9, cont=True)
    # more groups than CUs: 234 + 27 = 261 groups of RT = 3
    t["rt3_groups_over_cus"] = Spec("rt3", 700, 80, 30, 20, 5, resets="odd_tiles")
    # RT = 3 at the LDS edge: the widest actor x image beside a 16-wide head that fits (nb1 = 13), the first that does not (14);
    # the same for the critic beside the 8-wide head (nb1 = 15 | 16)
    t["edge_actor_fits"] = Spec("edge", 400, 115, 208, 20, 16, resets="odd_tiles")
    t["edge_actor_refused"] = Spec("edge", 400, 115, 209, 20, 16, resets="odd_tiles", expect_h2=False)
    t["edge_critic_fits"] = Spec("edge", 400, 115, 30, 240, 5, resets="odd_tiles")
    t["edge_critic_refused"] = Spec("edge", 400, 115, 30, 241, 5, resets="odd_tiles", expect_h2=False)
    return t


CASES = _table()
FAMILIES = ("heads", "continuous", "widths", "critic", "rt2", "rt3", "edge")
H2_INSTANCES = tuple(step_id(H2, noa, rt) for noa in (8, 16) for rt in (1, 2, 3))


def rows_of(s):
    return 32 * s.ta, 32 * s.tc


def predicted(name, packed):
    s = CASES[name]
    return predict(packed, s.n, s.din_a, s.din_c, s.ta, s.tc)


# ------------------------------------------------------------------------------------------------ references
def _params(rng, din, no, extra=0):
    """Reference-like weights, non-zero biases everywhere; `extra` trailing floats (the continuous head's log_std)."""
    flat = f32(ro.init_rec(rng, din, no, 1.0))
    p = ro.rec_unflatten(flat, din, no)
    for k in ("bpre", "bi", "bhn", "bpost", "bhead"):
        p[k][...] = rng.standard_normal(p[k].shape) * 0.1
    return np.concatenate([flat, f32(rng.standard_normal(extra) * 0.5)])


def _resets(rng, kind, rows):
    if kind == "none":
        return np.zeros(rows, bool)
    if kind == "all":
        return np.ones(rows, bool)
    if kind == "random":
        return rng.random(rows) < 0.3
    assert kind == "odd_tiles"
    return (np.arange(rows) // 32) % 2 == 1


def forward(flat, din, no, x, done, h):
    """One step of one network in float64: (outputs (rows, no), new hidden state (rows, 128))."""
    y, _, hn = ro.rec_forward(f64(flat[: ro.rec_param_count(din, no)]), din, no, f64(x)[None], np.asarray(done, bool)[None], f64(h))
    return y[0], hn


def logit_error_allowed(y):
    """What the 1e-5 form allows a logit of this case to be wrong by, at its largest."""
    return RTOL * (np.abs(y).max() + np.sqrt(np.mean(y * y)))


@lru_cache(maxsize=2)
def case(name):
    """Inputs (float32 / uint8, as the ABI takes them) and the float64 results of one case."""
    s = CASES[name]
    rng = np.random.default_rng([7100, zlib.crc32(name.encode())])
    Ra, Rc = rows_of(s)
    A = s.A
    c = dict(spec=s, name=name, rows_a=Ra, rows_c=Rc, share=1, done_stride=1, vbroadcast=1)
    c["pa"] = _params(rng, s.din_a, s.n, s.n if s.cont else 0)
    c["pc"] = _params(rng, s.din_c, 1)
    c["x"] = f32(rng.standard_normal((Ra, s.din_a)))
    c["ha"] = f32(rng.standard_normal((Ra, H)) * 0.5)
    c["hc"] = f32(rng.standard_normal((Rc, H)) * 0.5)
    c["done_a"] = _resets(rng, s.resets, Ra).astype(np.uint8)
    if s.form == "env":
        assert Ra == Rc * A
        c["done_stride"], c["vbroadcast"] = A, A
        c["done_c"] = c["done_a"]           # the actor's flags in place: the critic reads agent 0's of each env
        done_c_rows = c["done_a"][::A]
    else:
        c["done_c"] = _resets(rng, s.resets, Rc).astype(np.uint8)
        done_c_rows = c["done_c"]
    if s.form == "shared":
        assert Rc % A == 0
        c["share"] = A
        c["xc"] = f32(rng.standard_normal((Rc // A, s.din_c)))
        xc_rows = np.repeat(c["xc"], A, 0)
    else:
        c["xc"] = f32(rng.standard_normal((Rc, s.din_c)))
        xc_rows = c["xc"]
    c["done_c_rows"] = np.asarray(done_c_rows) != 0
    y, c["ha_new"] = forward(c["pa"], s.din_a, s.n, c["x"], c["done_a"] != 0, c["ha"])
    v, c["hc_new"] = forward(c["pc"], s.din_c, 1, xc_rows, c["done_c_rows"], c["hc"])
    c["value"], c["y"] = v[:, 0], y
    if s.cont:
        raw = f64(c["pa"][-s.n :])
        c["scale"] = np.broadcast_to(tn.scale_of(raw), y.shape)
        c["eps"] = tn.normal_noise(SEED, STEP, Ra, s.n, tn.STREAM_SAMPLE, s.row_offset)
        c["action"] = {0: np.tanh(y + c["scale"] * c["eps"]), 1: np.tanh(y)}
        c["mask"] = None
        return c
    mask = None
    if s.masked:
        mask = rng.random((Ra, s.n)) > 0.3
        mask[np.arange(Ra), rng.integers(0, s.n, Ra)] = True
        for r in s.dead_rows:
            mask[r] = False
    c["mask"] = mask
    dead = np.zeros(Ra, bool)
    dead[list(s.dead_rows)] = True
    c["dead"] = dead
    c["logp"] = sm.log_probs(y, mask)
    c["scores"] = sm.gumbel_scores(y, mask, philox.policy_uniforms(SEED, STEP, Ra, s.n, s.row_offset))
    c["sampled"], gap, _ = sm.sample_discrete(y, mask, SEED, STEP, s.row_offset)
    c["greedy"] = sm.greedy_discrete(y, mask)
    c["clear"] = GAP_FACTOR * logit_error_allowed(y)
    c["decided"] = (gap > c["clear"]) | dead
    z = np.sort(np.where(mask, y, -1e300) if mask is not None else y, -1)
    c["greedy_gap"] = np.where(dead, np.inf, z[:, -1] - z[:, -2]) if s.n > 1 else np.full(Ra, np.inf)
    return c


def action_ulp_reach(c, greedy):
    """Continuous head: how far one float32 rounding of the reference action moves its own log-density, in units of what the
    1e-5 form allows on that row - the kernel returns its action in float32, and log_prob(atanh(a)) is steep near the clip."""
    a = c["action"][greedy]
    lp = tn.log_prob_terms(a, c["y"], c["scale"])[0].sum(-1)
    a32 = f64(f32(a))
    lp32 = tn.log_prob_terms(a32, c["y"], c["scale"])[0].sum(-1)
    tol = RTOL * (np.abs(lp) + np.sqrt(np.mean(lp * lp)))
    return float((np.abs(lp32 - lp) / tol).max())
