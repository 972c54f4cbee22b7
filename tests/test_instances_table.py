"""CPU: the case tables of tests/instances.py reach, through its restatement of the dispatch, EVERY template instance that
the host dispatchers name and the LDS envelope allows - the lists below are written out from the dispatchers
(csrc/ppo_train*.hip, mlp_policy.hip, mlp_coop.hip), not derived from the tables - and every case has a usable oracle."""
import numpy as np
import pytest

from oracle import ppo_oracle as po
from tests import instances as I
from tests.instances import COOP, F32, FORWARD, H2, HYBRID, MODE_RAW, MODE_SAMPLE, MODE_VALUE, PER_WAVE, W8, policy_id, train_id

# --- exact f32, ppo_train_kernel<NO, KT1, ACTOR, XV, CONT>: XV = 4 exists from KT1 = 4 on -------------------------------------
_KT_XV = [(1, 1), (2, 1), (3, 1), (4, 1), (4, 4), (6, 1), (6, 4), (9, 1), (9, 4)]
F32_CRITIC = {train_id(F32, False, False, False, 1, kt, xv) for kt, xv in _KT_XV}
# envelope (LDS of make_layout<NO>): NO = 8 fits up to KT1 = 6, NO = 16 up to 4, NO = 32 only 1
F32_HEAD_ENVELOPE = {8: [(1, 1), (2, 1), (3, 1), (4, 1), (4, 4), (6, 1), (6, 4)], 16: [(1, 1), (2, 1), (3, 1), (4, 1), (4, 4)], 32: [(1, 1)]}
F32_ACTOR = {train_id(F32, True, False, False, no, kt, xv) for no, ks in F32_HEAD_ENVELOPE.items() for kt, xv in ks}
F32_CONTINUOUS = {train_id(F32, True, True, False, no, kt, xv) for no in (8, 16) for kt, xv in F32_HEAD_ENVELOPE[no]}
# instantiated by dispatch_kt but never launched: their LDS carve exceeds the 160 KiB of a CU, the launch is refused
F32_NEVER = ({(32, kt) for kt in (2, 3, 4, 6, 9)} | {(16, 6), (16, 9), (8, 9)})  # (NO, KT1), discrete and continuous head alike

# --- four-wave h2, ppo_train_h2_kernel<NO, S1, ACTOR, WIDE, XV>: XV 1 | 2 narrow, 1 | 4 WIDE; the layout does not depend on NO
_H2 = [(s1, False, xv) for s1 in (1, 2, 3, 4, 5, 6) for xv in (1, 2)] + [(s1, True, xv) for s1 in (12, 18) for xv in (1, 4)]
# instantiated by dispatch_s1 but never launched: the ACTOR's WIDE 18 layout (dy planes on top of the nine-tile x buffer)
# needs 167 136 bytes of LDS, launch_h2 refuses it - the f16x2 actor ends at 191 inputs
H2_ACTOR_NEVER = {(18, True, 1), (18, True, 4)}
H2_ACTOR = {train_id(H2, True, False, wide, no, s1, xv) for no in (8, 16, 32) for s1, wide, xv in _H2 if (s1, wide, xv) not in H2_ACTOR_NEVER}
H2_CRITIC = {train_id(H2, False, False, wide, 1, s1, xv) for s1, wide, xv in _H2}

# --- eight-wave w8, ppo_train_w8_kernel<NO, S1, XV, ., ACTOR>: S1 = 4 only two floats at a time; the critic runs the NO = 8 body
_W8 = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 2)]
W8_ACTOR = {train_id(W8, True, False, False, no, s1, xv) for no in (8, 16) for s1, xv in _W8}
W8_CRITIC = {train_id(W8, False, False, False, 8, s1, xv) for s1, xv in _W8}

# --- acting kernels --------------------------------------------------------------------------------------------------------
_KT = (1, 2, 3, 4, 6, 9)
POLICY_STEP = ({policy_id(HYBRID, 0, noa, kt) for noa in (8, 16, 32) for kt in _KT}
               | {policy_id(PER_WAVE, 0, noa, 0) for noa in (8, 16, 32)}
               | {policy_id(COOP, MODE_SAMPLE, no, kt) for no in (8, 16, 32) for kt in _KT}
               | {policy_id(COOP, MODE_VALUE, 1, kt) for kt in _KT})
FORWARD_ALL = ({policy_id(FORWARD, 0, no, 0) for no in (1, 8, 16, 32)}
               | {policy_id(COOP, MODE_RAW, no, kt) for no in (1, 8, 16, 32) for kt in _KT})


def test_gradient_tables_reach_every_instance():
    actor = {I.predict_actor(c.mode, c.variant, c.din, c.n_actions, c.offset).instance for c in I.ACTOR_CASES}
    assert actor == F32_ACTOR | H2_ACTOR | W8_ACTOR
    critic = {I.predict_critic(c.mode, c.variant, c.din, c.agg, I.A, I.A if c.shared else 1, c.offset).instance for c in I.CRITIC_CASES}
    assert critic == F32_CRITIC | H2_CRITIC | W8_CRITIC
    cont = {I.predict_continuous(c.din, c.dim).instance for c in I.CONTINUOUS_CASES}
    assert cont == F32_CONTINUOUS


def test_acting_tables_reach_every_instance():
    step = set()
    for c in I.STEP_CASES:
        share = c.rows // c.critic_in_rows if c.rows % c.critic_in_rows == 0 else 1
        step |= set(I.predict_policy_step(c.variant, c.actor_din, c.n_actions, c.critic_din, c.rows, c.critic_in_rows * share))
    assert step == POLICY_STEP
    assert {I.predict_forward(c.variant, c.din, c.n_out) for c in I.FORWARD_CASES} == FORWARD_ALL
    # the launches that only a row count reaches: the hybrid's actor tile loop wraps beyond 128 blocks x 4 waves x 32 rows, more
    # than 128 critic tiles and critic inputs wider than 287 take the per-wave kernel, the raw forward wraps beyond 512 blocks
    assert any(c.variant == 0 and c.rows > 16384 and c.critic_in_rows <= 4096 for c in I.STEP_CASES)
    assert any(c.variant == 0 and c.critic_in_rows > 4096 for c in I.STEP_CASES)
    assert any(c.variant == 0 and c.critic_din > 287 for c in I.STEP_CASES)
    assert any(c.variant == 0 and c.rows > 65536 for c in I.FORWARD_CASES)


def test_envelope_of_the_exact_f32_kernel():
    """The LDS carve decides which exact-f32 head instances can launch; the first refused width of each NO is in the refusal
    tables, and the instances beyond the envelope are exactly the ones listed as never launched."""
    for no in (8, 16, 32):
        for kt in _KT:
            fits = I.f32_lds_bytes(no, kt) <= I.LDS_BYTES
            assert fits == ((no, kt) not in F32_NEVER), (no, kt)
    assert all(I.f32_lds_bytes(1, kt) <= I.LDS_BYTES for kt in _KT)  # the critic fits at every width up to 287
    assert I.ACTOR_F32_REFUSED == ((3, 192), (14, 128), (20, 32))
    for nA, din in I.ACTOR_F32_REFUSED:
        assert I.predict_actor("f32", 0, din, nA).refusal == "LDS" and I.predict_actor("f32", 0, din - 1, nA).instance is not None
        for variant in (0, 1):  # the f16x2 arithmetic runs the same shape on the four-wave kernels - up to 191 inputs
            p = I.predict_actor("f16x2", variant, din, nA)
            if din >= 192:
                assert p == I.Prediction(None, "LDS", 0, 0)
            else:
                assert p.instance // 1000000 == H2 and (p.h2_launches, p.w8_launches) == (1, 0)
    for s1, wide in [(s, False) for s in range(1, 7)] + [(12, True), (18, True)]:
        assert I.h2_lds_bytes(s1, wide, False) <= I.LDS_BYTES
        assert (I.h2_lds_bytes(s1, wide, True) <= I.LDS_BYTES) == (s1 != 18), s1
    assert I.h2_lds_bytes(18, True, True) == 167136
    for variant, nA, din in I.ACTOR_F16X2_REFUSED:
        assert I.predict_actor("f16x2", variant, din, nA) == I.Prediction(None, "LDS", 0, 0)
        assert din >= 192 and I.predict_actor("f16x2", variant, 191, nA).instance is not None
    for dim, din in I.CONTINUOUS_REFUSED:
        assert I.predict_continuous(din, dim).refusal == "LDS"
    assert I.predict_continuous(127, 9).instance is not None and I.predict_continuous(191, 2).instance is not None
    assert I.predict_actor("f32", 0, 288, 3).refusal == "not instantiated"


def test_w8_hands_over_what_it_does_not_instantiate():
    for c in I.ACTOR_CASES + I.CRITIC_CASES:
        if c.mode == "f16x2" and c.variant == 1:
            p = (I.predict_actor(c.mode, 1, c.din, c.n_actions, c.offset) if isinstance(c, I.ActorCase)
                 else I.predict_critic(c.mode, 1, c.din, c.agg, I.A, I.A if c.shared else 1, c.offset))
            assert p.w8_launches == 0 and p.instance // 1000000 == H2
    # default variant: an odd width in 97..127, more than 16 actions, an aggregated critic row, widths from 128
    assert I.predict_actor("f16x2", 0, 101, 3) == I.Prediction(train_id(H2, True, False, True, 8, 12, 1), None, 1, 0)
    assert I.predict_actor("f16x2", 0, 70, 20) == I.Prediction(train_id(H2, True, False, False, 32, 5, 2), None, 1, 0)
    assert I.predict_critic("f16x2", 0, 70, 1, 2, 2) == I.Prediction(train_id(H2, False, False, False, 1, 5, 2), None, 1, 0)
    assert I.predict_critic("f16x2", 0, 70, 0, 2, 2) == I.Prediction(train_id(W8, False, False, False, 8, 3, 2), None, 1, 1)
    assert I.predict_critic("f16x2", 0, 128, 0, 2, 2).instance == train_id(H2, False, False, True, 1, 12, 4)
    # (both families end at 287 inputs: what the f16x2 kernels hand on to the exact-f32 dispatcher is refused there)
    assert I.predict_critic("f16x2", 0, 288, 0, 2, 2) == I.Prediction(None, "not instantiated", 0, 0)


def _blocks_nonzero(g, din, no):
    return all(np.abs(b).max() > 0 for b in po.mlp_unflatten(g, din, no))


@pytest.mark.parametrize("kind", ["actor", "critic", "continuous"])
def test_every_gradient_case_has_a_finite_nonzero_oracle(kind):
    if kind == "actor":
        for c in I.ACTOR_CASES:
            d = I.actor_data(c)
            assert np.isfinite(d["grad"]).all() and np.isfinite(d["sums"]).all() and _blocks_nonzero(d["grad"], c.din, c.n_actions), c
            sel = d["mask"][d["rows_sel"]]
            assert (sel.sum(1) == 1).any(), "a selected row with a single legal action"
            assert (sel.sum(1) == 0).sum() == 1, "a selected row without a legal action"
            assert (d["ratio"] > 1.2).any() and (d["ratio"] < 0.8).any() and ((d["ratio"] > 0.8) & (d["ratio"] < 1.2)).any(), c
            assert len(set(d["idx"].tolist())) == I.RB and not np.array_equal(d["idx"], np.sort(d["idx"]))
    elif kind == "critic":
        for c in I.CRITIC_CASES:
            d = I.critic_data(c)
            assert np.isfinite(d["grad"]).all() and d["sums"][0] > 0 and _blocks_nonzero(d["grad"], c.din, 1), c
            assert (d["diff"] > 0.2).any() and (d["diff"] < -0.2).any() and (np.abs(d["diff"]) < 0.2).any(), c
    else:
        for c in I.CONTINUOUS_CASES:
            d = I.continuous_data(c)
            n = po.mlp_param_count(c.din, c.dim)
            assert np.isfinite(d["grad"]).all() and _blocks_nonzero(d["grad"][:n], c.din, c.dim) and np.abs(d["grad"][n:]).min() > 0, c


def test_every_acting_case_has_a_decided_oracle():
    """The seed search of instances.step_data ends for every case: a draw of inputs whose masked logits, and a sampling seed in
    range(64) whose Gumbel scores, have a float64 top-two gap >= 1e-3 on every row."""
    for c in I.STEP_CASES:
        d = I.step_data(c)
        assert d is not None, c
        some = np.arange(c.rows) != d["none_legal_row"]
        assert 0 <= d["seed"] < 64 and d["mask"][np.arange(c.rows), d["sampled"]][some].all() and d["mask"][np.arange(c.rows), d["forced"]][some].all()
        assert d["mask"][d["one_legal_row"]].sum() == 1
        none = d["none_legal_row"]  # uniform over the real actions; the exact tie at finfo.min goes to index 0
        assert not d["mask"][none].any() and d["sampled"][none] == 0 and d["greedy"][none] == 0
        assert np.allclose(d["lsm"][none], -np.log(c.n_actions), rtol=0, atol=1e-12)
        assert np.isfinite(d["logits"]).all() and np.isfinite(d["value"]).all()
        if c.n_actions > 1 and c.rows < 1000:
            assert len(set(d["sampled"].tolist())) > 1, c


def test_widened_tolerances_are_four_times_the_measured_float32_error():
    """A case's gradient tolerance is 1e-4 unless a float32 NumPy run of the oracle itself misses 1e-4 of the float64 run on the
    case's rows; then it is four times that run's error, recorded in instances.CONTINUOUS_F32_MEASURED and re-measured here
    (to 25 %: the error is that of a handful of float32 roundings, the recorded figure must not drift from what it stands for)."""
    for c in I.CONTINUOUS_CASES:
        err = I.continuous_f32_error(c)
        if c in I.CONTINUOUS_F32_MEASURED:
            rec = I.CONTINUOUS_F32_MEASURED[c]
            assert rec > 1e-4 and 0.75 * rec < err < 1.25 * rec, (c, err)
            assert I.continuous_grad_tolerance(c) == 4.0 * rec
        else:
            assert err < 1e-4, (c, err)
            assert I.continuous_grad_tolerance(c) == 1e-4
    assert set(I.CONTINUOUS_F32_MEASURED) <= set(I.CONTINUOUS_CASES)
