"""CPU: tests/seq_model.py is the whole-network oracle taken apart (scan + output path + loss, composed, reproduce
oracle/rec_oracle.py's losses and gradients), its case tables reach every template instance the dispatchers of csrc/rec_gru.hip,
rec_gru_h2.hip and rec_out_h2.hip name, each deliberately wrong variant differs exactly where its case is meant to catch it, and the
loss inputs take every branch of the clipped objectives."""
import numpy as np
import pytest

from oracle import rec_oracle as ro
from oracle import tanh_normal as tn
from tests import seq_model as sm

H = sm.H


# ---- composition -------------------------------------------------------------------------------------------------------------------
def _network(kind, rng):
    din, no, T, R = 7, {"actor": 5, "critic": 1, "continuous": 3}[kind], 4, 32
    flat = ro.init_rec(rng, din, no, 1.0)
    flat += rng.standard_normal(flat.size) * 0.02  # non-zero biases
    obs = rng.standard_normal((T, R, din))
    done = rng.random((T, R)) < 0.3
    h0 = rng.standard_normal((R, H)) * 0.5
    return din, no, T, R, flat, obs, done, h0


def _compose(flat, din, no, obs, done, h0, loss_fn):
    """Gradient of the network's flat parameters, built from seq_model's pieces alone."""
    p = ro.rec_unflatten(flat, din, no)
    T, R, _ = obs.shape
    x = obs.reshape(T * R, din)
    pre = x @ p["Wpre"] + p["bpre"]
    xp = np.maximum(pre, 0.0)
    gi = (xp @ p["Wi"] + p["bi"]).reshape(T, R, 3 * H)
    hs, hprev, saved = sm.gru_scan(gi, p["Wh"], p["bhn"], h0, done)
    losses, g = sm.out_path(hs.reshape(T * R, H), {k: p[k] for k in ("Wpost", "bpost", "Whead", "bhead")}, loss_fn)
    dgi, dgh = sm.gru_scan_grads(gi, p["Wh"], p["bhn"], h0, done, g["dh"].reshape(T, R, H))
    dgi, dgh = dgi.reshape(T * R, 3 * H), dgh.reshape(T * R, 3 * H)
    dpre = (dgi @ p["Wi"].T) * (pre > 0)
    parts = [x.T @ dpre, dpre.sum(0), xp.T @ dgi, dgi.sum(0), hprev.reshape(T * R, H).T @ dgh, dgh[:, 2 * H :].sum(0),
             g["dWpost"], g["dbpost"], g["dWhead"], g["dbhead"]]
    return losses, np.concatenate([a.reshape(-1) for a in parts]), saved


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


def test_composition_actor():
    rng = np.random.default_rng(1)
    din, no, T, R, flat, obs, done, h0 = _network("actor", rng)
    mask = rng.random((T, R, no)) > 0.25
    action = rng.integers(0, no, (T, R))
    np.put_along_axis(mask, action[..., None], True, -1)
    mask[1, 3] = False  # a row without a legal action
    old_lp, adv = rng.standard_normal((T, R)) * 0.3 - 1.5, rng.standard_normal((T, R)) * 2 + 0.3
    flt = lambda a: a.reshape((T * R,) + a.shape[2:])

    def loss_fn(y):
        la, ent, dy = sm.actor_loss(y, flt(mask), flt(action), flt(old_lp), flt(adv))
        return (la, ent), dy

    (la, ent), grad, _ = _compose(flat, din, no, obs, done, h0, loss_fn)
    tot, la_o, ent_o, g_o = ro.rec_actor_loss_grad(flat, din, no, obs, done, h0, mask, action, old_lp, adv, sm.CLIP, sm.ENT_COEF)
    _close(la, la_o, "actor loss")
    _close(ent, ent_o, "entropy")
    _close(grad, g_o, "actor gradient")


def test_composition_critic():
    rng = np.random.default_rng(2)
    din, no, T, R, flat, obs, done, h0 = _network("critic", rng)
    old_v, tgt = rng.standard_normal((T, R)) * 0.3, rng.standard_normal((T, R))

    def loss_fn(y):
        vl, dv = sm.critic_loss(y[:, 0], old_v.reshape(-1, 1), tgt.reshape(-1, 1))
        return (vl,), dv[:, None]

    (vl,), grad, _ = _compose(flat, din, no, obs, done, h0, loss_fn)
    tot, vl_o, g_o = ro.rec_critic_loss_grad(flat, din, obs, done, h0, old_v, tgt, sm.CLIP, sm.VF_COEF)
    _close(vl, vl_o, "value loss")
    _close(grad, g_o, "critic gradient")


def test_composition_continuous():
    rng = np.random.default_rng(3)
    din, dim, T, R, flat, obs, done, h0 = _network("continuous", rng)
    raw = rng.standard_normal(dim) * 0.5
    action = np.tanh(rng.standard_normal((T, R, dim)))
    action[0, 0, 0], action[1, 2, 1] = 0.9995, -0.9995  # both clipped branches
    old_lp, adv = rng.standard_normal((T, R)) * 0.3 - 2.0, rng.standard_normal((T, R)) * 2 + 0.3
    eps = rng.standard_normal((T, R, dim))
    box = {}

    def loss_fn(y):
        la, ent, dmean, draw = sm.continuous_loss(y, raw, action.reshape(-1, dim), old_lp.reshape(-1), adv.reshape(-1), eps.reshape(-1, dim))
        box["draw"] = draw
        return (la, ent), dmean

    (la, ent), grad, _ = _compose(flat, din, dim, obs, done, h0, loss_fn)
    tot, la_o, ent_o, g_o = ro.rec_actor_loss_grad_continuous(np.concatenate([flat, raw]), din, dim, obs, done, h0, action, old_lp, adv,
                                                              sm.CLIP, sm.ENT_COEF, eps)
    _close(la, la_o, "actor loss")
    _close(ent, ent_o, "entropy")
    _close(np.concatenate([grad, box["draw"]]), g_o, "continuous actor gradient")
    # per-row raw scales: the rows' gradients add up to the vector's
    rows = np.tile(raw, (T * R, 1))
    y = rng.standard_normal((T * R, dim)) * 0.5
    args = (action.reshape(-1, dim), old_lp.reshape(-1), adv.reshape(-1), eps.reshape(-1, dim))
    a, b = sm.continuous_loss(y, raw, *args), sm.continuous_loss(y, rows, *args)
    _close(b[3].sum(0), a[3], "dlog_std_rows summed")
    _close(b[2], a[2], "dmean")


# ---- dispatch table ----------------------------------------------------------------------------------------------------------------------
# written out from the hosts: mava_seq_actor_loss_f32 / mava_seq_sample_f32 pick 8 | 16 | 32 by n_actions <= 8, <= 16; the critic is
# <1, false>; the continuous pair picks 8 | 16 by action_dim <= 8; mava_rec_out_f32 runs <8, true> | <16, true> by n_out <= 8 and the
# critic on <8, false>; mava_gru_scan_bwd_h2_launch picks <true | false> by dgh_n_only
SEQ_LOSS = {("seq_loss", 8, True), ("seq_loss", 16, True), ("seq_loss", 32, True), ("seq_loss", 1, False)}
SEQ_SAMPLE = {("seq_sample", 8), ("seq_sample", 16), ("seq_sample", 32)}
SEQ_CONT = {("seq_loss_cont", 8), ("seq_loss_cont", 16), ("seq_sample_cont", 8), ("seq_sample_cont", 16)}
REC_OUT = {("rec_out", 8, True), ("rec_out", 16, True), ("rec_out", 8, False)}
SCAN_BWD_H2 = {("gru_scan_bwd_h2", True), ("gru_scan_bwd_h2", False)}


def test_case_tables_reach_every_instance():
    loss = {sm.seq_loss_instance(n) for n in sm.ACTOR_N} | {("seq_loss", 1, False) for _ in sm.CRITIC_AGENTS}
    assert loss == SEQ_LOSS
    assert {sm.seq_sample_instance(n) for n in sm.SAMPLE_N} == SEQ_SAMPLE
    assert {i for d in sm.CONT_DIMS for i in sm.cont_instances(d)} == SEQ_CONT
    tiles = sm.LOSS_T * sm.LOSS_EM * sm.LOSS_A // 32
    out = {sm.rec_out_instance(True, n, s, tiles) for n in sm.OUT_N for s in sm.OUT_SLABS}
    out |= {sm.rec_out_instance(False, 1, s, tiles) for s in sm.OUT_SLABS}
    assert out == REC_OUT and tiles == 6
    assert all(sm.rec_out_instance(*r, tiles) is None for r in sm.OUT_REFUSED)
    assert {sm.scan_bwd_instance(1, k) for k in (0, 1)} == SCAN_BWD_H2
    # both sides of every boundary, and the rows without a legal action where the issue wants them
    for lo, hi in ((8, 9), (16, 17)):
        assert lo in sm.ACTOR_N and hi in sm.ACTOR_N and lo in sm.SAMPLE_N and hi in sm.SAMPLE_N
    assert {8, 9} <= set(sm.CONT_DIMS) and {8, 9} <= set(sm.OUT_N) and 16 in sm.OUT_N
    assert set(sm.ALL_MASKED_N) <= set(sm.ACTOR_N) and set(sm.ALL_MASKED_N) - {17} <= set(sm.OUT_N)
    assert {em * a for _, a, em, _ in sm.SCAN_SHAPES} == {32, 96}
    assert sm.SEED >> 32 and sm.SEED & 0xFFFFFFFF


# ---- deliberately wrong variants -----------------------------------------------------------------------------------------------------------
def test_wrong_tile_stride_shows_only_beyond_one_tile():
    for E, A, Em, gathered in sm.SCAN_SHAPES:
        c = sm.scan_case(5, E, A, Em, gathered, "none")
        hs, _, _ = sm.gru_scan(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"], tile_stride=1)
        same = np.array_equal(hs, c["hs"])
        assert same == (c["Rm"] == 32), c["Rm"]
        hs, _, _ = sm.gru_scan(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], c["done_rows"], tile_stride=c["Rm"] // 32)
        assert np.array_equal(hs, c["hs"])


def test_env_flag_broadcast_shows_only_on_per_agent_flags():
    for kind in sm.SCAN_DONE:
        c = sm.scan_case(5, 40, 3, 32, True, kind)
        wrong = sm.done_rows(c["done"], c["idx"], c["A"], c["Rm"], env_flag_only=True)
        assert np.array_equal(wrong, c["done_rows"]) == (kind in ("none", "all_t0")), kind
        if kind in ("one_seq", "random"):
            hs, _, _ = sm.gru_scan(c["gi"], c["Wh"], c["bhn"], c["h0_rows"], wrong)
            assert np.abs(hs - c["hs"]).max() > 1e-3
    assert sm.scan_case(5, 40, 3, 32, True, "one_seq")["done_rows"].sum() == 5  # one sequence, every step, inside the minibatch


def test_softmax_over_padding_shows_only_on_rows_without_a_legal_action():
    for n in sm.ACTOR_N:
        c = sm.actor_case(n)
        NO = sm.seq_loss_instance(n)[1]
        la, ent, dz = sm.actor_loss(c["logits"], c["mask_rows"], c["action_rows"], c["old_lp_rows"], c["adv_rows"], slots=NO)
        differs = abs(ent - c["entropy"]) > 1e-6
        assert differs == (n in sm.ALL_MASKED_N), n
        lp = sm.log_probs(c["logits"], c["mask_rows"])
        for r in c["all_masked"]:
            assert np.allclose(lp[r], -np.log(n), rtol=0, atol=1e-12) and (c["dlogits"][r] == 0).all()
        for r in c["one_legal"]:
            assert c["mask_rows"][r].sum() == 1 and lp[r, c["action_rows"][r]] == 0.0


def test_critic_summing_one_slot_shows_only_with_three_agents():
    for na in sm.CRITIC_AGENTS:
        c = sm.critic_case(na)
        vl, dv = sm.critic_loss(c["v"], c["old_v_rows"], c["tgt_rows"], slots_summed=1)
        assert (np.array_equal(dv, c["dv"]) and vl == c["loss"]) == (na == 1)
        assert c["A"] == (1 if na > 1 else sm.LOSS_A) and c["Rm"] == 64


# ---- branches of the clipped objectives ---------------------------------------------------------------------------------------------------
def test_actor_inputs_take_every_clip_branch():
    cases = [sm.actor_case(n) for n in sm.ACTOR_N] + [sm.out_case(True, n) for n in sm.OUT_N] + [sm.cont_case(d, p, 0) for d in sm.CONT_DIMS for p in (False, True)]
    for c in cases:
        if "dim" in c:
            scale = np.broadcast_to(tn.scale_of(sm.f64(c["raw"])), c["mean"].shape)
            lp = tn.log_prob_terms(c["action_rows"], sm.f64(c["mean"]), scale)[0].sum(-1)
        else:
            y = sm.out_forward(c["hs"], c["params"]) if "hs" in c else c["logits"]
            lp = sm.log_probs(y, c["mask_rows"])[np.arange(c["R"]), c["action_rows"]]
        _, _, ratio, g = sm._ppo_terms(lp, sm.f64(c["old_lp_rows"]), c["adv_rows"])
        for rsel in (ratio < 1 - sm.CLIP, (ratio >= 1 - sm.CLIP) & (ratio <= 1 + sm.CLIP), ratio > 1 + sm.CLIP):
            for gsel in (g > 0, g < 0):
                assert (rsel & gsel).any(), c.get("n", c.get("dim"))
    c = sm.actor_case(9, constant_adv=True)
    assert c["loss"] == 0.0 and (sm._ppo_terms(np.zeros(c["R"]), np.zeros(c["R"]), c["adv_rows"])[3] == 0).all()


def test_critic_inputs_take_every_clip_branch():
    """Inside the range the clipped value IS the value and the two terms tie (each gets half the gradient); outside, either term can be
    the larger one."""
    for c in [sm.critic_case(na) for na in sm.CRITIC_AGENTS] + [sm.out_case(False, 1, na) for na in sm.CRITIC_AGENTS]:
        v = sm.out_forward(c["hs"], c["params"])[:, 0] if "hs" in c else sm.f64(c["v"])
        diff = v[:, None] - c["old_v_rows"]
        vclip = c["old_v_rows"] + np.clip(diff, -sm.CLIP, sm.CLIP)
        l1, l2 = (v[:, None] - c["tgt_rows"]) ** 2, (vclip - c["tgt_rows"]) ** 2
        inside = np.abs(diff) <= sm.CLIP
        assert (inside & (l1 == l2)).any() and (~inside & (l1 > l2)).any() and (~inside & (l1 < l2)).any()


def test_inputs_stay_clear_of_the_kinks():
    """A float32 kernel may land on the other side of relu's kink or of a clip boundary when the float64 value lies within its
    rounding of it; the inputs keep 5e-5 from the first and 2e-5 from the second (ratios and value differences are O(1))."""
    def clear(x, edges):
        return min(float(np.abs(np.asarray(x) - e).min()) for e in edges)

    for c in [sm.out_case(True, n) for n in sm.OUT_N] + [sm.out_case(False, 1, na) for na in sm.CRITIC_AGENTS]:
        assert np.abs(sm.out_pre(c["hs"], c["params"])).min() >= sm.RELU_CLEAR
        y = sm.out_forward(c["hs"], c["params"])
        if "na" in c:
            assert clear(y[:, :1] - c["old_v_rows"], (-sm.CLIP, sm.CLIP)) >= sm.CLIP_CLEAR
        else:
            lp = sm.log_probs(y, c["mask_rows"])[np.arange(c["R"]), c["action_rows"]]
            assert clear(sm._ppo_terms(lp, sm.f64(c["old_lp_rows"]), c["adv_rows"])[2], (1 - sm.CLIP, 1 + sm.CLIP)) >= sm.CLIP_CLEAR
    for c in [sm.actor_case(n) for n in sm.ACTOR_N]:
        lp = sm.log_probs(c["logits"], c["mask_rows"])[np.arange(c["R"]), c["action_rows"]]
        assert clear(sm._ppo_terms(lp, sm.f64(c["old_lp_rows"]), c["adv_rows"])[2], (1 - sm.CLIP, 1 + sm.CLIP)) >= sm.CLIP_CLEAR
    for c in [sm.critic_case(na) for na in sm.CRITIC_AGENTS]:
        assert clear(sm.f64(c["v"])[:, None] - c["old_v_rows"], (-sm.CLIP, sm.CLIP)) >= sm.CLIP_CLEAR
    for c in [sm.cont_case(d, p, 0) for d in sm.CONT_DIMS for p in (False, True)]:
        scale = np.broadcast_to(tn.scale_of(sm.f64(c["raw"])), c["mean"].shape)
        lp = tn.log_prob_terms(c["action_rows"], sm.f64(c["mean"]), scale)[0].sum(-1)
        assert clear(sm._ppo_terms(lp, sm.f64(c["old_lp_rows"]), c["adv_rows"])[2], (1 - sm.CLIP, 1 + sm.CLIP)) >= sm.CLIP_CLEAR


# ---- measured figures --------------------------------------------------------------------------------------------------------------------
def test_sampling_cases_are_decided_and_the_gap_is_the_measured_one():
    worst = 0.0
    for n in sm.SAMPLE_N:
        for rows in sm.SAMPLE_ROWS:
            for off in sm.ROW_OFFSETS:
                c = sm.sample_case(n, rows, off)
                worst = max(worst, c["f32_diff"])
                none = np.zeros(rows, bool)
                none[c["all_masked"]] = True
                assert ((c["gap"] <= 4.0 * c["f32_diff"]) & ~none).mean() <= 0.01, (n, rows, off)
                assert len(c["all_masked"]) == (2 if n in sm.ALL_MASKED_N else 0)
                assert (c["sampled"][none] == 0).all() and (c["greedy"][none] == 0).all()
                assert c["mask"][np.arange(rows), c["sampled"]][~none].all()
                if n > 2:
                    assert c["greedy"][6] == n - 2  # the exact tie: the lower index
                if n > 1 and rows > 32:
                    assert len(set(c["sampled"].tolist())) > 1
    assert 0.75 * 6.35e-07 < worst < 1.25 * 6.35e-07, worst  # the figure in test_gpu_seq_kernels.test_seq_sample's docstring


def test_continuous_cases_stay_inside_the_project_tolerance_in_float32():
    worst = max(sm.cont_f32_error(sm.cont_case(d, p, off)) for d in sm.CONT_DIMS for p in (False, True) for off in sm.ROW_OFFSETS)
    assert worst < 1e-4 and 0.75 * 4.2e-05 < worst < 1.25 * 4.2e-05, worst  # the figure in test_seq_continuous_loss's docstring
    a, b = sm.cont_case(8, False, 0), sm.cont_case(8, False, 1000)
    assert not np.array_equal(a["eps"], b["eps"])  # row_offset moves the entropy draw


def test_t32_round_trip():
    a = np.arange(64 * 13, dtype=np.float32).reshape(64, 13)
    t = sm.to_t32(a)
    assert t[32] == a[0, 1] and t[1] == a[1, 0] and np.array_equal(sm.from_t32(t, 64, 13), a)
