"""CPU: tests/mat_kernel_model.py's loss reference is the float64 autograd of the loss as tests/mat_model.py states it, every
sampling case is decided, every loss case holds its special rows inside the minibatch, gathers through an idx that is not the
identity and stays clear of the clip boundaries, and the wrong indexings a kernel could have differ from the reference on these
cases.  No GPU."""
import numpy as np
import pytest
import torch

from tests import mat_kernel_model as mk
from tests import mat_model as mm
from tests import seq_model as sm


def _rel(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, size = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= 1e-12 * size, f"{what}: error {err:.3e} against max-abs {size:.3e}"


# ---- the loss reference against mat_model.loss's expression --------------------------------------------------------------------------
@pytest.mark.parametrize("constant_adv,masked", [(False, True), (False, False), (True, True), (True, False)],
                         ids=["mask", "no-mask", "constant-adv-mask", "constant-adv-no-mask"])
@pytest.mark.parametrize("n", [5, 64])
def test_loss_reference_is_autograd_of_the_model_loss(n, constant_adv, masked):
    c = mk.mat_loss_case(n, 300, 3, constant_adv, masked)
    Bm, A = c["Bm"], c["A"]
    t = lambda k, shape: torch.tensor(sm.f64(c[k])).view(shape)
    logits, values = t("logits", (Bm, A, n)).requires_grad_(True), t("values", (Bm, A)).requires_grad_(True)
    mask = None if not masked else torch.tensor(c["mask_rows"]).view(Bm, A, n)
    lp, ent = mm.log_prob_entropy(logits, torch.tensor(c["action_rows"]).view(Bm, A), mask)
    total, actor, vloss, entropy = mm.loss_terms(lp, ent, values, t("old_lp_rows", (Bm, A)), t("adv_rows", (Bm, A)),
                                                 t("old_value_rows", (Bm, A)), t("target_rows", (Bm, A)), sm.CLIP, sm.ENT_COEF, sm.VF_COEF)
    total.backward()
    actor, vloss, entropy = actor.detach(), vloss.detach(), entropy.detach()
    if constant_adv:
        assert float(actor) == 0.0 and c["actor_loss"] == 0.0
    else:
        _rel(c["actor_loss"], float(actor), "actor loss")
    _rel(c["entropy"], float(entropy), "entropy")
    _rel(c["value_loss"], float(vloss), "value loss")
    _rel(c["dlogits"], logits.grad.view(Bm * A, n).numpy(), "dlogits")
    _rel(c["dvalues"], values.grad.view(-1).numpy(), "dvalues")
    if masked:
        assert (logits.grad.view(Bm * A, n).numpy()[~c["mask_rows"]] == 0.0).all()
        assert len(c["all_masked"]) == 2 and (c["dlogits"][c["all_masked"]] == 0.0).all()


# ---- sampling cases --------------------------------------------------------------------------------------------------------------------
def test_sampling_cases_are_decided_and_the_gap_is_the_measured_one():
    """The float32 NumPy evaluation of the scores z - log(-log(u)) lies at most 8.6e-07 from float64 over every case (largest at
    n = 64); the GPU test's gap is four times the case's own figure."""
    worst = 0.0
    for n in mk.MAT_N:
        for B, A in mk.MAT_SAMPLE_SHAPES:
            for off in mk.ROW_OFFSETS:
                c = mk.mat_sample_case(n, B, A, off)
                rows, r = c["rows"], np.arange(c["rows"])
                worst = max(worst, c["f32_diff"])
                none = np.zeros(rows, bool)
                none[c["all_masked"]] = True
                assert ((c["gap"] <= 4.0 * c["f32_diff"]) & ~none).mean() <= 0.01, (n, B, A, off)
                assert len(c["all_masked"]) == (sum(x < rows for x in (11, 20)) if n >= 5 else 0) and len(c["all_masked"]) in (0, 2)
                assert len(c["one_legal"]) == sum(x < rows for x in (3, 70))
                flat = c["mask"].reshape(rows, n)
                assert not flat[c["all_masked"]].any() and (n == 1 or (flat[c["one_legal"]].sum(-1) == 1).all())
                assert (c["sampled"][none] == 0).all() and (c["greedy"][none] == 0).all()
                assert np.allclose(c["logp"][none], -np.log(n), rtol=0, atol=1e-12)
                assert flat[r, c["sampled"]][~none].all() and flat[r, c["greedy"]][~none].all()
                if n > 2:
                    assert c["greedy"][6] == n - 2  # the exact tie: the lower index
                if n > 1:
                    assert len(set(c["sampled"].tolist())) > 1
                if n >= 5 and A > 1:  # two agents of one sample differ in their masks, and a mask read elsewhere shows
                    assert (c["mask"][:, 0] != c["mask"][:, 1]).any()
                    for wrong in (mk.mask_read_at_sample(c), mk.mask_read_at_t32(c)):
                        assert (sm.greedy_discrete(c["logits"], wrong) != c["greedy"]).any()
                        assert (sm.sample_discrete(c["logits"], wrong, sm.SEED, c["step"], off)[0] != c["sampled"]).any()
            # the row offset moves the draw
            a, b = (mk.mat_sample_case(n, B, A, off)["sampled"] for off in mk.ROW_OFFSETS)
            assert n == 1 or not np.array_equal(a, b)
    assert 0.75 * 8.6e-07 < worst < 1.25 * 8.6e-07, worst


def test_sample_tables_reach_the_listed_code():
    assert mk.MAT_N[-1] == 64 and 63 in mk.MAT_N and any(32 < n for n in mk.MAT_N)
    assert any(n % 4 and n > 4 for n in mk.MAT_N) and any(n < 4 for n in mk.MAT_N)  # a partial last Philox word after a full one
    assert any(B > 256 and B % 256 for B, _ in mk.MAT_SAMPLE_SHAPES) and any(A == 1 for _, A in mk.MAT_SAMPLE_SHAPES)
    assert any(B * A < 32 for B, A in mk.MAT_SAMPLE_SHAPES) and any(32 % A for _, A in mk.MAT_SAMPLE_SHAPES)
    assert 0 in mk.ROW_OFFSETS and any(mk.ROW_OFFSETS)


# ---- loss cases ------------------------------------------------------------------------------------------------------------------------
def _loss_cases():
    for n in mk.MAT_N:
        for Bm, A in mk.MAT_LOSS_SHAPES:
            yield mk.mat_loss_case(n, Bm, A)
    yield mk.mat_loss_case(9, 300, 3, True, True)
    yield mk.mat_loss_case(9, 300, 3, True, False)
    yield mk.mat_loss_case(5, 300, 3, left_out_adv=1e3)


def test_loss_cases_meet_their_conditions():
    for c in _loss_cases():
        n, Bm, A, R = c["n"], c["Bm"], c["A"], c["R"]
        what = (n, Bm, A)
        assert c["rows"] % 32 == 0 and 0 <= c["rows"] - R < 32
        # idx: Bm distinct samples of Bm + 37, not the identity, out of order
        assert len(set(c["idx"].tolist())) == Bm and c["TE"] == Bm + 37 and c["idx"].max() < c["TE"]
        assert not np.array_equal(c["idx"], np.arange(Bm)) and (c["idx"] != np.arange(Bm)).mean() > 0.5 and (np.diff(c["idx"]) < 0).any()
        assert np.array_equal(c["ext"], np.repeat(c["idx"], A) * A + np.tile(np.arange(A), Bm))
        # the special rows are inside the minibatch, spread over it
        if c["mask"] is not None:
            assert len(c["one_legal"]) == 2 and len(c["all_masked"]) == (2 if n >= 5 else 0), what
            assert not c["mask_rows"][c["all_masked"]].any()
            assert n == 1 or (c["mask_rows"][c["one_legal"]].sum(-1) == 1).all()
            legal = c["mask_rows"].any(-1)
            assert c["mask_rows"][np.arange(R), c["action_rows"]][legal].all(), "the recorded action of a row is legal"
            if Bm == 300:  # one of them past the first wave of the second block
                assert max(c["one_legal"] + c["all_masked"]) >= 512 + 64
        # clear of the clip boundaries
        lp = sm.log_probs(c["logits"], c["mask_rows"])[np.arange(R), c["action_rows"]]
        ratio = np.exp(lp - sm.f64(c["old_lp_rows"]))
        assert mk._clear(ratio, (1 - sm.CLIP, 1 + sm.CLIP)) >= sm.CLIP_CLEAR, what
        assert mk._clear(sm.f64(c["values"]) - sm.f64(c["old_value_rows"]), (-sm.CLIP, sm.CLIP)) >= sm.CLIP_CLEAR, what
        assert c["draw"] < 64 and c["edge"] >= sm.CLIP_CLEAR
        # the statistics are those of the gathered rows
        s = c["stats"].sum(0)
        assert abs(s[0] - sm.f64(c["adv_rows"]).sum()) <= 1e-9 * max(1.0, abs(s[0])) and c["stats"].shape == (3, 2)


def test_loss_inputs_take_every_clip_branch():
    for n in mk.MAT_N:
        c = mk.mat_loss_case(n, 300, 3)
        lp = sm.log_probs(c["logits"], c["mask_rows"])[np.arange(c["R"]), c["action_rows"]]
        _, _, ratio, g = sm._ppo_terms(lp, sm.f64(c["old_lp_rows"]), c["adv_rows"])
        for rsel in (ratio < 1 - sm.CLIP, (ratio >= 1 - sm.CLIP) & (ratio <= 1 + sm.CLIP), ratio > 1 + sm.CLIP):
            for gsel in (g > 0, g < 0):
                assert n == 1 or (rsel & gsel).any(), n
        v, ov, tg = (sm.f64(c[k]) for k in ("values", "old_value_rows", "target_rows"))
        diff = v - ov
        l1, l2 = (v - tg) ** 2, (ov + np.clip(diff, -sm.CLIP, sm.CLIP) - tg) ** 2
        inside = np.abs(diff) <= sm.CLIP
        assert (inside & (l1 == l2)).any() and (~inside & (l1 > l2)).any() and (~inside & (l1 < l2)).any()


def test_wrong_row_indexings_differ_from_the_reference():
    """Reading the trajectory at b instead of idx[b], or the mask at the minibatch row, changes every output of the 900-row case; the
    statistics of other rows than the minibatch's move the mean when the left-out samples carry 1e3."""
    c = mk.mat_loss_case(5, 300, 3)
    q = np.arange(c["R"])
    for wrong in (mk.loss_reference(c, ext=q), mk.loss_reference(c, mask_ext=q)):
        assert abs(wrong["actor_loss"] - c["actor_loss"]) > 1e-3 and abs(wrong["entropy"] - c["entropy"]) > 1e-3
        assert sm.rel_err(wrong["dlogits"], c["dlogits"]) > 1e-2
    assert abs(mk.loss_reference(c, ext=q)["value_loss"] - c["value_loss"]) > 1e-3
    # an error confined to the rows past the first tile, or past the first wave, still shows
    for first in (32, 64, 256):
        ext = np.where(q < first, c["ext"], q)
        assert sm.rel_err(mk.loss_reference(c, ext=ext)["dlogits"], c["dlogits"]) > 1e-2
    c = mk.mat_loss_case(5, 300, 3, left_out_adv=1e3)
    assert (c["adv"] == 1e3).sum() == 37 * 3 and np.abs(c["adv_rows"]).max() < 20
    first_rows = sm.adv_stats(c["adv"].reshape(-1)[: c["R"]]).sum(0)  # the sums of a kernel that walked b instead of idx[b]
    assert abs(first_rows[0] - c["stats"].sum(0)[0]) / c["R"] > 10.0


def test_constant_advantages_leave_only_the_entropy_term():
    for masked in (True, False):
        c, d = mk.mat_loss_case(9, 300, 3, True, masked), mk.mat_loss_case(9, 300, 3, False, masked)
        assert c["actor_loss"] == 0.0 and d["actor_loss"] != 0.0
        _, ent, dz = sm.actor_loss(c["logits"], c["mask_rows"], c["action_rows"], c["old_lp_rows"], np.zeros(c["R"]))
        assert np.array_equal(dz, c["dlogits"]) and ent == c["entropy"]
        # the value side does not see the advantages
        assert np.array_equal(c["values"], d["values"]) and np.array_equal(c["dvalues"], d["dvalues"]) and c["value_loss"] == d["value_loss"]


def test_loss_cases_stay_inside_the_project_tolerance_in_float32():
    """The figure in test_gpu_mat_kernels.test_mat_loss's docstring."""
    worst = max(mk.loss_f32_error(mk.mat_loss_case(n, Bm, A)) for n in mk.MAT_N for Bm, A in mk.MAT_LOSS_SHAPES)
    assert 4.0 * worst < 1e-4 and 0.75 * 8.8e-07 < worst < 1.25 * 8.8e-07, worst


def test_loss_tables_reach_the_listed_code():
    rows = [mk.c32(Bm * A) for Bm, A in mk.MAT_LOSS_SHAPES]
    assert 928 in rows and 32 in rows and 64 in rows and (300, 3) in mk.MAT_LOSS_SHAPES
    assert any(nb * 256 < 928 for nb in mk.N_BLOCKS if nb > 1), "a grid-stride walk with more than one block"
    assert any((nb - 1) * 256 >= 928 for nb in mk.N_BLOCKS), "a block without rows at 928 rows"
    assert 1 in mk.N_BLOCKS and 1.0 in mk.GRAD_SCALES and max(mk.GRAD_SCALES) == 1024.0
