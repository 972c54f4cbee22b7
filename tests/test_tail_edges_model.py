"""Case tables, NumPy references and tolerances of the tail-kernel edge tests (tests/test_gpu_adam_edges.py,
tests/test_gpu_gae_edges.py), and the checks that keep those GPU tests from hiding a failure behind their own tables: for
every case a float32 run of the oracle stays within a quarter of the bound the GPU test applies against the float64 run;
the multi-segment Adam wrapper is the per-segment oracle; the clip-threshold gradients sit where they claim; the single
column handed to an N = 1 GAE launch is the column it claims to be.  Runs without a GPU."""
from typing import NamedTuple

import numpy as np
import pytest

from oracle import ppo_oracle as po

# the kernels take b1 = 0.9 and b2 = 0.999 as f32: the oracle gets those very numbers (tests/test_gpu_tail.py)
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))
MAX_NORM = 0.5
SENTINEL = 7.0
ADAM_TOL = 2e-6  # one Adam step from an identical state, p / m / v against float64 (as tests/test_gpu_tail.py)
GAE_TOL = 1e-5   # advantages and targets against float64 (as tests/test_gpu_kernels.py)
# The update itself (p after one step from p0 = 0, where no ulp(p) hides it) has no earlier bound: four times the float32
# oracle's worst distance from the float64 one over P0_ZERO_CASES below, in assert_close's form, segment by segment.
# Measured 2.61e-6 (the float32 run forms 1 - b2^t in f32, a cancellation at small t; test_p0_zero_bound_is_four_times_...
# prints the figure and holds the constants to it), hence 1.044e-5 - against 1e-3 in test_clip_adam_matches_oracle,
# where p0 ~ 0.1.
P0_ZERO_MEASURED = 2.61e-6
P0_ZERO_TOL = 4 * P0_ZERO_MEASURED
CLIP_NORM, NOCLIP_NORM = 3.0, 0.05  # gradient norms that put a segment on either side of MAX_NORM


def distance(a, b):
    """The smallest rtol with which conftest.assert_close(a, b, rtol) passes: max |a - b| / (|b| + rms(b))."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    scale = float(np.sqrt(np.mean(b * b)))
    den = np.abs(b) + scale
    err = np.abs(a - b)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))))


# ------------------------------------------------------------------------------------------------------------------ Adam
def schedule(lr, count, decay, steps_per_update, num_updates, dtype=np.float64):
    """The learning rate at the pre-increment count (po.learning_rate), every operation in `dtype`."""
    lr = dtype(lr)
    if not decay:
        return lr
    return lr * (dtype(1) - dtype(int(count) // steps_per_update) / dtype(num_updates))


def adam_ref(p, g, m, v, counts, seg_off, lrs, *, grad_scale=1.0, max_norm=MAX_NORM, decay=False, steps_per_update=1,
             num_updates=1, dtype=np.float64):
    """One mava_clip_adam launch restated: po.clip_adam per segment on the kernels' scaled f32 gradient, each segment with
    its own count, learning rate and norm.  Returns (p, m, v) in `dtype`."""
    out = [np.array(x, dtype) for x in (p, m, v)]
    for k in range(len(lrs)):
        lo, hi = seg_off[k], seg_off[k + 1]
        if hi == lo:
            continue
        gi = (np.asarray(g[lo:hi], np.float32) * np.float32(grad_scale)).astype(np.float32)
        lr = schedule(lrs[k], counts[k], decay, steps_per_update, num_updates, dtype)
        pn, mn, vn, _ = po.clip_adam(p[lo:hi], gi, m[lo:hi], v[lo:hi], int(counts[k]), lr, max_norm, b1=B1, b2=B2, dtype=dtype)
        for o, x in zip(out, (pn, mn, vn)):
            o[lo:hi] = x
    return tuple(out)


class AdamCase(NamedTuple):
    name: str
    seg_off: tuple
    lrs: tuple
    counts: tuple
    norms: tuple       # float64 norm of each segment's (scaled) gradient: CLIP_NORM clips, NOCLIP_NORM does not
    kw: tuple = ()     # items of the launch's keyword arguments (decay, steps_per_update, num_updates)
    zero_moments: bool = False
    p0_zero: bool = False
    seed: int = 0

    @property
    def total(self):
        return self.seg_off[-1]

    @property
    def kwargs(self):
        return dict(self.kw)

    def state(self):
        """f32 p, g, m, v: p ~ 0.1, m ~ 1e-3 and v in [1, 2) e-6 (or zero), every segment's gradient scaled to its norm.
        (sqrt(v) >= |m| as in a real Adam state: a v of 1e-11 under an m of 1e-3 makes a step of 1e-2, on which the f32
        oracle's own 1 - b2^t - a cancellation the kernels avoid by forming it in double - shows at 1e-6 of p.)"""
        rng = np.random.default_rng(1 + self.seed)
        n = self.total
        p = rng.standard_normal(n) * (0.0 if self.p0_zero else 0.1)
        g = rng.standard_normal(n)
        for k, want in enumerate(self.norms):
            lo, hi = self.seg_off[k], self.seg_off[k + 1]
            if hi > lo:
                g[lo:hi] *= want / np.sqrt((g[lo:hi] ** 2).sum())
        m = rng.standard_normal(n) * (0.0 if self.zero_moments else 1e-3)
        v = (1.0 + rng.random(n)) * (0.0 if self.zero_moments else 1e-6)
        return tuple(x.astype(np.float32) for x in (p, g, m, v))

    def clips(self, k):
        return self.norms[k] >= MAX_NORM

    def reference(self, st, dtype=np.float64):
        p, g, m, v = st
        return adam_ref(p, g, m, v, self.counts, self.seg_off, self.lrs, dtype=dtype, **self.kwargs)


def _norm(clip):
    return CLIP_NORM if clip else NOCLIP_NORM


# A.1: one segment; 1 .. 5 below a float4, around one block's 256 lanes and 1024 parameters, 8197 = eight blocks + 5
ADAM_TOTALS = (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 8197)
ADAM_OFFSETS = (0, 1, 2, 3)  # floats between a 16-byte aligned allocation and the view the launch gets
SIZE_CASES = tuple(
    # with the clip on: zero moments, so that m = (1 - b1) g / n * c shows the norm on its own
    AdamCase(f"{total}-{'clip' if clip else 'noclip'}", (0, total), (1e-3,), (3,), (_norm(clip),), zero_moments=clip, seed=total)
    for total in ADAM_TOTALS for clip in (True, False))

# A.2: segment layouts (an empty middle segment; boundaries off multiples of 4; eight segments around multiples of 256)
SEG_LAYOUTS = ((0, 1), (0, 1, 2), (0, 5, 5, 12), (0, 3, 1030, 1031, 5000), (0, 255, 513, 514, 1027, 2049, 2050, 4099, 4100))
_SEG_COUNTS = (0, 4, 1, 7, 2, 9, 5, 3)
SEGMENT_CASES = tuple(
    AdamCase(f"{'-'.join(map(str, off))}-{'clipfirst' if first else 'noclipfirst'}", off,
             tuple(1e-3 * (k + 1) for k in range(len(off) - 1)), _SEG_COUNTS[: len(off) - 1],
             tuple(_norm((k % 2 == 0) == first) for k in range(len(off) - 1)), seed=100 + 2 * i + first)
    for i, off in enumerate(SEG_LAYOUTS) for first in (True, False))

# A.3: the grid is capped at 256 blocks x 256 lanes x 4 parameters: beyond 262 144 parameters the flat loop takes a second
# batch; two segments whose boundary lies inside it (at 262 144 there is no second batch: the boundary sits mid-way)
CAP = 256 * 256 * 4
CAPPED_TOTALS = (CAP, CAP + 1, CAP + 1025, 2 * CAP + 3)
CAPPED_CASES = tuple(
    AdamCase(f"{total}-{'clip' if clip else 'noclip'}", (0, CAP + (total - CAP) // 2 if total > CAP else CAP // 2 + 1, total),
             (1e-3, 2e-3), (2, 5), (_norm(clip),) * 2, seed=total % 1000 + clip)
    for total in CAPPED_TOTALS for clip in (True, False))

# A.4: step counts (the 1 - b^t terms) and the decay schedule across the floor division and at the last update
COUNTS = (0, 1, 9, 999, 100_000)
DECAY_KW = (("decay", True), ("steps_per_update", 8), ("num_updates", 10))
DECAY_COUNTS = (7, 8, 15, 16, 72, 79)
_EIGHT = tuple(range(0, 1001, 125))


def _count_cases(p0_zero):
    tag = "-p0zero" if p0_zero else ""
    cases = [AdamCase(f"count{c}{tag}", (0, 1000), (1e-3,), (c,), (_norm(i % 2 == 0),), p0_zero=p0_zero, seed=200 + i)
             for i, c in enumerate(COUNTS)]
    cases += [AdamCase(f"decay{c}{tag}", (0, 1000), (1e-3,), (c,), (_norm(i % 2 == 1),), DECAY_KW, p0_zero=p0_zero, seed=300 + i)
              for i, c in enumerate(DECAY_COUNTS)]
    lrs = tuple(1e-3 * (k + 1) for k in range(8))
    norms = tuple(_norm(k % 3 != 0) for k in range(8))
    cases.append(AdamCase(f"eight-counts{tag}", _EIGHT, lrs, (0, 1, 9, 999, 100_000, 7, 16, 79), norms, p0_zero=p0_zero, seed=400))
    cases.append(AdamCase(f"eight-decay{tag}", _EIGHT, lrs, (0, 7, 8, 15, 16, 72, 79, 1), norms, DECAY_KW, p0_zero=p0_zero, seed=401))
    return tuple(cases)


COUNT_CASES = _count_cases(False)
P0_ZERO_CASES = _count_cases(True)

ALL_ADAM_CASES = SIZE_CASES + SEGMENT_CASES + CAPPED_CASES + COUNT_CASES + P0_ZERO_CASES


def by_name(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


# A.5: k equal powers of two whose norm is max_norm exactly, scaled by (1 +- 2^-20): x = 2^-6 (1 +- 2^-20) is an f32, the
# sum of 1024 equal squares is exact in float64, and so is its root, max_norm (1 +- 2^-20): 8 f32 ulps of max_norm away.
THRESHOLD_K, THRESHOLD_X, THRESHOLD_EPS = 1024, 2.0 ** -6, 2.0 ** -20


def threshold_gradient(side):
    """side = +1: norm = MAX_NORM (1 + 2^-20), the clip is on; side = -1: norm = MAX_NORM (1 - 2^-20), it is off."""
    x = THRESHOLD_X * (1.0 + side * THRESHOLD_EPS)
    assert float(np.float32(x)) == x
    return np.full(THRESHOLD_K, x, np.float32)


# A.7: the fused finish beyond PPO's sizes: (name, Ctx mode, Pa, Pc, critic_din).  More than 262 144 parameters cap the
# flat grid (256 blocks, a second batch that crosses the W1 range where the launch packs); Pa + Pc + 3 above 131 072 gives
# more than 2048 norm partials (8 per lane are preloaded, the rest go through the tail loop).  The last three put the number
# of partials, ceil((Pa + Pc + 3) / 64), on 2048, 2049 and 2050: no tail loop, one partial in it, two.
def _pcount(din, n_out):
    return (din + 1) * 128 + 129 * 128 + 129 * n_out


FINISH_CASES = (
    ("pack18", "f16x2", 300_001, _pcount(264, 1), 264),
    ("pack12", "f16x2", 300_001, _pcount(150, 1), 150),
    ("nopack", "f32", 300_001, _pcount(150, 1), 0),
    ("partials2048", "f32", 131_006, 61, 0),
    ("partials2049", "f32", 131_070, 63, 0),
    ("partials2050", "f32", 131_070, 70, 0),
)
FINISH_SLABS = 3
FINISH_GRAD_SCALE = 0.5
FINISH_SCALES = {True: 3.0, False: 1e-3}  # of the slab entries: clip active / inactive


def finish_p0(Pa, Pc):
    return (np.random.default_rng(Pa + Pc).standard_normal(Pa + Pc) * 0.1).astype(np.float32)

# A.8
SLAB_COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 37)
SLAB_WIDTHS = (1, 63, 64, 65, 900)
SLAB2_SPLITS = ((0, 3), (5, 0), (64, 1), (63, 2), (1000, 128))


def block_sum_f64(acc):
    """clip_adam_kernel's block_sum of 256 per-lane doubles: a 64-lane shuffle-down tree per wave, then the 4 waves."""
    w = np.asarray(acc, np.float64).reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, : 64 - o] = w[:, : 64 - o] + w[:, o:64].copy()  # (lanes past 64 - o add garbage no one reads)
    t = 0.0
    for i in range(4):
        t = t + w[i, 0]
    return float(t)


def norm_flat(gs, lo, hi, base_aligned=True):
    """The norm mava_clip_adam forms of segment [lo, hi) of the scaled f32 gradient gs, in its order: lane t of 256 adds the
    squares (in double) of the head lo + t, lo + t + 256, ... below the first 16-byte aligned index `al` (the whole segment when
    the base pointer is unaligned), then of the float4s al + 4 i, i = t, t + 256, ..., one accumulator per component, then
    of the tail; ((a0 + a1) + (a2 + a3)); block_sum."""
    sq = np.asarray(gs, np.float32).astype(np.float64) ** 2
    al = min(hi, (lo + 3) & ~3) if base_aligned else hi
    a = np.zeros((4, 256))
    for i in range(lo, al, 256):
        c = sq[i : min(i + 256, al)]
        a[0, : c.size] = a[0, : c.size] + c
    n4 = (hi - al) >> 2
    q = sq[al : al + 4 * n4].reshape(n4, 4)
    for i in range(0, n4, 256):
        c = q[i : i + 256]
        a[:, : c.shape[0]] = a[:, : c.shape[0]] + c.T
    c = sq[al + 4 * n4 : hi]
    a[0, : c.size] = a[0, : c.size] + c
    return float(np.sqrt(block_sum_f64((a[0] + a[1]) + (a[2] + a[3]))))


# ------------------------------------------------------------------------------------------------------------------- GAE
def gae_inputs(T, N, seed, p_done=0.05):
    """reward, value, done, last_val, last_done drawn as in test_gae_matches_oracle (last_done: about 10 % ones)."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = rng.standard_normal((T, N)).astype(np.float32)
    d = rng.random((T, N)) < p_done
    lv = rng.standard_normal(N).astype(np.float32)
    ld = rng.random(N) < 0.1
    return r, v, d, lv, ld


def gae_column(inputs, j):
    """Column j alone, as the (T, 1) inputs of an N = 1 launch."""
    r, v, d, lv, ld = inputs
    return tuple(np.ascontiguousarray(x) for x in (r[:, j : j + 1], v[:, j : j + 1], d[:, j : j + 1], lv[j : j + 1], ld[j : j + 1]))


# B.1: 16 steps a chunk, 128 a slab: below, on and above either, ragged (T % 16 != 0) and not, up to three slabs
GAE_TIMES = (1, 2, 15, 16, 17, 112, 127, 128, 129, 144, 256, 272, 300)
GAE_WIDTHS = (1, 31, 64, 65)
# B.2: strips of 64 columns below N = 2048 (512: 8 strips, permuted; 520: 9, not), of 32 from there (2048: 64 strips; 2080:
# 65; 2304: 72; 4128: 129)
GAE_COL_TIMES = (16, 37)
GAE_COLS = (32, 63, 512, 520, 1024, 2048, 2050, 2080, 2304, 4096 + 32)
GAE_PROBES = 16


def strip_width(N):
    return 32 if N >= 2048 else 64


def probe_columns(N):
    """At most GAE_PROBES columns: the first, the last, both sides of every strip boundary next to either end, the rest
    spread over the middle."""
    w = strip_width(N)
    last_edge = ((N - 1) // w) * w
    want = [0, N - 1, w - 1, w, 2 * w - 1, 2 * w, last_edge - 1, last_edge, last_edge - w - 1, last_edge - w]
    cols = []
    for c in want:
        if 0 <= c < N and c not in cols:
            cols.append(c)
    rng = np.random.default_rng(N)
    for c in rng.permutation(N):
        if len(cols) >= min(GAE_PROBES, N):
            break
        if int(c) not in cols:
            cols.append(int(c))
    return sorted(cols)


# B.3
GAE_DONE_ROWS = (15, 16, 127, 128, 255, 256, 299)
# B.4
GAE_COEFS = ((1.0, 1.0), (0.99, 0.0), (0.0, 0.95), (0.0, 0.0))
GAE_COEF_TIMES = (17, 300)


GAE_DONE_PATTERNS = ("rows", "all", "none")
GAE_DONE_MASKINGS = ("ff", "rec", "rec-last-done-ones")


def time_edge_inputs(T, N):
    return gae_inputs(T, N, 1000 * T + N)


def column_edge_inputs(T, N):
    return gae_inputs(T, N, 1000 * T + N, p_done=0.05 if N < 1000 else 1 / 500)


def done_placement_inputs(pattern, masking):
    """T = 300, N = 64: flags exactly on GAE_DONE_ROWS, everywhere or nowhere; optionally last_done all ones."""
    T, N = 300, 64
    r, v, _, lv, ld = gae_inputs(T, N, 7)
    d = np.zeros((T, N), bool)
    if pattern == "rows":
        d[list(GAE_DONE_ROWS)] = True
    elif pattern == "all":
        d[:] = True
    else:
        assert pattern == "none"
    if masking == "rec-last-done-ones":
        ld = np.ones(N, bool)
    return r, v, d, lv, ld


def coefficient_inputs(T):
    return gae_inputs(T, 65, 1000 * T + 65)


# ------------------------------------------------------------------------------------------------------------- the checks
def segment_distances(case, got, want):
    """name -> the worst distance over the segments, each against its own rms as the GPU tests compare them."""
    out = {}
    for name, a, b in zip("pmv", got, want):
        out[name] = max(distance(a[case.seg_off[k] : case.seg_off[k + 1]], b[case.seg_off[k] : case.seg_off[k + 1]])
                        for k in range(len(case.lrs)))
    return out


METRICS_GRAD_SCALE = 0.25
METRICS_CASES = {1: COUNT_CASES[2], 8: COUNT_CASES[-2]}  # A.6: n_seg -> case, launched with grad_scale = 1 / 4


@by_name(ALL_ADAM_CASES)
def test_f32_adam_oracle_within_a_quarter_of_the_bound(case):
    st = case.state()
    want = case.reference(st)
    got = case.reference(st, np.float32)
    assert all(a.dtype == np.float32 for a in got)
    for name, dist in segment_distances(case, got, want).items():
        tol = P0_ZERO_TOL if (case.p0_zero and name == "p") else ADAM_TOL
        assert dist <= tol / 4, (name, dist)
    # the gradient norms are where the case says: every segment clips or not as announced, in f32 as in f64
    for k in range(len(case.lrs)):
        gk = st[1][case.seg_off[k] : case.seg_off[k + 1]]
        if gk.size:
            for dt in (np.float32, np.float64):
                assert bool(np.sqrt((gk.astype(dt) ** 2).sum()) >= MAX_NORM) == case.clips(k)


@pytest.mark.parametrize("n_seg", sorted(METRICS_CASES))
def test_f32_adam_oracle_within_a_quarter_of_the_bound_metrics_cases(n_seg):
    case = METRICS_CASES[n_seg]
    assert len(case.lrs) == n_seg and not case.kwargs
    p, g, m, v = case.state()
    runs = [adam_ref(p, g, m, v, case.counts, case.seg_off, case.lrs, grad_scale=METRICS_GRAD_SCALE, dtype=dt) for dt in (np.float32, np.float64)]
    for name, dist in segment_distances(case, *runs).items():
        assert dist <= ADAM_TOL / 4, (name, dist)


@pytest.mark.parametrize("big", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("name,mode,Pa,Pc,din_c", FINISH_CASES, ids=[c[0] for c in FINISH_CASES])
def test_f32_adam_oracle_within_a_quarter_of_the_bound_finish_cases(name, mode, Pa, Pc, din_c, big):
    """The first of the three steps of test_fused_finish_beyond_ppo_sizes (the later ones start from the kernel's state)."""
    from tests import test_gpu_tail as tail

    g, _ = tail._reduced(din_c, FINISH_SLABS, FINISH_SCALES[big], FINISH_GRAD_SCALE, Pa, Pc)
    P = Pa + Pc
    p = finish_p0(Pa, Pc)
    z = np.zeros(P, np.float32)
    case = AdamCase(name, (0, Pa, P), (tail.LR_A, tail.LR_C), (0, 0), ())
    kw = {k: tail.KW[k] for k in ("max_norm", "decay", "steps_per_update", "num_updates")}
    runs = [adam_ref(p, g[:P], z, z, case.counts, case.seg_off, case.lrs, grad_scale=FINISH_GRAD_SCALE, dtype=dt, **kw) for dt in (np.float32, np.float64)]
    want = tuple(tail._oracle_step(p, z, z, np.zeros(2, np.int64), g[:P], Pa, FINISH_GRAD_SCALE))
    assert all(np.array_equal(a, b) for a, b in zip(runs[1], want)), "adam_ref restates test_gpu_tail._oracle_step"
    for nm, dist in segment_distances(case, *runs).items():
        assert dist <= ADAM_TOL / 4, (nm, dist)


def test_p0_zero_bound_is_four_times_the_f32_oracles_distance():
    worst = 0.0
    for case in P0_ZERO_CASES:
        st = case.state()
        assert not st[0].any()
        worst = max(worst, segment_distances(case, case.reference(st, np.float32), case.reference(st))["p"])
    print(f"f32 oracle, update from p0 = 0: worst distance {worst:.3e}")
    assert worst <= P0_ZERO_MEASURED <= 1.05 * worst, "the recorded figure is the measured one"
    assert P0_ZERO_TOL == 4 * P0_ZERO_MEASURED


@by_name(SEGMENT_CASES + COUNT_CASES[-2:])
def test_adam_wrapper_is_the_per_segment_oracle(case):
    p, g, m, v = case.state()
    got = case.reference((p, g, m, v))
    kw = case.kwargs
    for k in range(len(case.lrs)):
        sl = slice(case.seg_off[k], case.seg_off[k + 1])
        lr = po.learning_rate(case.lrs[k], case.counts[k], kw.get("decay", False), kw.get("steps_per_update", 1), 1, kw.get("num_updates", 1))
        want = po.clip_adam(p[sl], g[sl], m[sl], v[sl], case.counts[k], lr, MAX_NORM, b1=B1, b2=B2)[:3] if sl.stop > sl.start else (p[sl], m[sl], v[sl])
        for a, b in zip(got, want):
            assert np.array_equal(a[sl], np.asarray(b, np.float64))
    if len(case.lrs) > 1 and all(case.seg_off[k + 1] > case.seg_off[k] for k in range(len(case.lrs))):  # and it is no one-network step
        whole = po.clip_adam(p, g, m, v, case.counts[0], case.lrs[0], MAX_NORM, b1=B1, b2=B2)
        assert not np.array_equal(whole[1], got[1])


@pytest.mark.parametrize("side", [1, -1])
def test_threshold_gradient_is_eight_ulps_from_max_norm(side):
    g = threshold_gradient(side)
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    assert norm == MAX_NORM * (1.0 + side * THRESHOLD_EPS)  # exact: no rounding anywhere in the construction
    ulp = float(np.spacing(np.float32(MAX_NORM)))
    assert abs(norm - MAX_NORM) >= 4 * ulp and abs(norm - MAX_NORM) == 8 * ulp
    assert float(np.float32(norm)) == norm and (np.float32(norm) >= np.float32(MAX_NORM)) == (side > 0)
    # any order of summation in double lands on the same f32: the partial sums are exact (22-bit squares, 1024 of them)
    assert norm_flat(g, 0, g.size) == norm and norm_flat(g, 0, g.size, base_aligned=False) == norm
    # and the two first steps differ by 8 ulps as well: (1 - b1) g against (1 - b1) (g / n) c
    plain, clipped = (1 - B1) * g.astype(np.float64), (1 - B1) * (g.astype(np.float64) / norm) * MAX_NORM
    assert np.all(np.abs(plain - clipped) > 6 * np.spacing(np.float32(clipped[0])))


@pytest.mark.parametrize("N", GAE_COLS)
def test_gae_column_extraction(N):
    T = 37
    inputs = gae_inputs(T, N, N)
    cols = probe_columns(N)
    w = strip_width(N)
    assert len(cols) == min(GAE_PROBES, N) == len(set(cols)) and cols[0] == 0 and cols[-1] == N - 1
    if N > w:  # one column on each side of the first and of the last strip boundary
        assert {w - 1, w} <= set(cols) and {((N - 1) // w) * w - 1, ((N - 1) // w) * w} <= set(cols)
    for rec in (False, True):
        adv, tgt = po.gae(*inputs[:4], 0.99, 0.95, last_done=inputs[4] if rec else None)
        for j in cols:
            one = gae_column(inputs, j)
            assert all(x.shape[1:] == (1,) or x.shape == (1,) for x in one) and np.array_equal(one[0][:, 0], inputs[0][:, j])
            a1, t1 = po.gae(*one[:4], 0.99, 0.95, last_done=one[4] if rec else None)
            assert np.array_equal(a1[:, 0], adv[:, j]) and np.array_equal(t1[:, 0], tgt[:, j])


def _gae_runs():
    """(inputs, rec, gamma, lambda) of every comparison of tests/test_gpu_gae_edges.py against float64."""
    for rec in (False, True):
        for T in GAE_TIMES:
            for N in GAE_WIDTHS:
                yield time_edge_inputs(T, N), rec, 0.99, 0.95
        for T in GAE_COL_TIMES:
            for N in GAE_COLS:
                yield column_edge_inputs(T, N), rec, 0.99, 0.95
        for T in GAE_COEF_TIMES:
            for gamma, lam in GAE_COEFS:
                yield coefficient_inputs(T), rec, gamma, lam
    for pattern in GAE_DONE_PATTERNS:
        for masking in GAE_DONE_MASKINGS:
            yield done_placement_inputs(pattern, masking), masking != "ff", 0.99, 0.95


def test_f32_gae_oracle_within_a_quarter_of_the_bound():
    worst, n = 0.0, 0
    for (r, v, d, lv, ld), rec, gamma, lam in _gae_runs():
        kw = dict(last_done=ld if rec else None)
        a64, t64 = po.gae(r, v, d, lv, gamma, lam, **kw)
        a32, t32 = po.gae(r, v, d, lv, gamma, lam, dtype=np.float32, **kw)
        assert a32.dtype == np.float32
        worst = max(worst, distance(a32, a64), distance(t32, t64))
        n += 1
    assert n == 2 * (len(GAE_TIMES) * len(GAE_WIDTHS) + len(GAE_COL_TIMES) * len(GAE_COLS) + len(GAE_COEF_TIMES) * len(GAE_COEFS)) + 9
    assert worst <= GAE_TOL / 4, worst
