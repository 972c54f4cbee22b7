"""CPU checks of tests/rec_step_model.py: the case table of tests/test_gpu_rec_step.py reaches every instance it claims, its
edge cases sit where the LDS arithmetic says, its reset patterns are present, and the float64 reference alone leaves few enough
rows of every case undecided for the sampled actions to be compared exactly."""
import numpy as np
import pytest

from tests import rec_step_model as m

NAMES = sorted(m.CASES)


def _nb1(din):
    return (din + 15) // 16


def test_every_instance_is_reached():
    packed = {n: m.predicted(n, True) for n in NAMES}
    exact = {n: m.predicted(n, False) for n in NAMES}
    h2 = {n: i for n, i in packed.items() if i // 1000 == m.H2}
    assert set(h2.values()) == set(m.H2_INSTANCES) == {2081, 2082, 2083, 2161, 2162, 2163}
    for n in NAMES:  # the table's own claim, case by case
        assert (n in h2) == m.CASES[n].expect_h2, n
        assert exact[n] // 1000 == m.F32
    # both silent fallbacks of the packed entry: more than 16 outputs, and the LDS refusal of launch_step
    wide = [n for n in NAMES if not m.CASES[n].expect_h2 and m.CASES[n].n > 16]
    lds = [n for n in NAMES if not m.CASES[n].expect_h2 and m.CASES[n].n <= 16]
    assert {m.CASES[n].n for n in wide} == {17, 32} and all(packed[n] == exact[n] == 1320 for n in wide)
    assert sorted(lds) == ["edge_actor_refused", "edge_critic_refused"]
    assert packed["edge_actor_refused"] == 1161 and packed["edge_critic_refused"] == 1081
    # the exact-f32 kernel: every head width without the CU split, 8 and 16 with it
    assert set(exact.values()) == {1080, 1160, 1320, 1081, 1161}
    # the discrete entry, the continuous entry and the continuous head of the packed kernel at 8 and 16 outputs
    assert {m.head_bucket(m.CASES[n].n) for n in NAMES if m.CASES[n].cont} == {8, 16}
    assert packed["rt3_config4"] == 2163  # the benchmarked shape's instance: 13 actions, RT = 3


def test_dispatch_restatement():
    assert [m.pick_rt(*t) for t in ((8, 8), (200, 56), (200, 57), (384, 128), (384, 129), (512, 64), (3000, 3000))] == [1, 1, 2, 2, 3, 3, 3]
    assert m.pick_rt(512, 64) == 3 and m.predict(True, 13, 155, 188, 512, 64) == 2163  # BASELINE config 4: 2048 envs x 8 agents
    assert [m.head_bucket(n) for n in (1, 8, 9, 16, 17, 32)] == [8, 8, 16, 16, 32, 32]
    assert m.f32_blocks(8, 8) == (8, 8) and m.f32_blocks(200, 56) == (200, 56)
    assert m.f32_blocks(193, 65) == (191, 65) and m.f32_blocks(400, 115) == (198, 58) and m.f32_blocks(700, 80) == (229, 27)
    assert m.f32_blocks(5000, 1) == (255, 1) and m.f32_blocks(1, 5000) == (1, 256)  # (a lone actor tile beside a critic that rounds up to every CU: 257 blocks)
    for ta, tc in ((193, 65), (400, 115), (700, 80), (512, 64)):
        assert sum(m.f32_blocks(ta, tc)) <= m.CUS
    # x images narrower than an activation image share its bytes: region A is max(x image, IIMG)
    assert m.h2_net_bytes(1, 8, 1) == m.h2_net_bytes(128, 8, 1) < m.h2_net_bytes(129, 8, 1)


def test_lds_edges():
    C = m.CASES
    for fits, refused, side, no in (("edge_actor_fits", "edge_actor_refused", "din_a", 16), ("edge_critic_fits", "edge_critic_refused", "din_c", 8)):
        a, b = C[fits], C[refused]
        assert m.pick_rt(a.ta, a.tc) == m.pick_rt(b.ta, b.tc) == 3
        da, db = getattr(a, side), getattr(b, side)
        assert db == da + 1 and da % 16 == 0, "the last width of one 16-input batch and the first of the next"
        assert m.h2_net_bytes(da, no, 3) <= m.LDS_BYTES < m.h2_net_bytes(db, no, 3)
        assert m.h2_lds_bytes(a.n, a.din_a, a.din_c, 3) == m.h2_net_bytes(da, no, 3), "the other network is not what decides"
        assert m.h2_lds_bytes(b.n, b.din_a, b.din_c, 2) <= m.LDS_BYTES, "RT = 2 would have fitted: the refusal is RT = 3's"
    assert (_nb1(C["edge_actor_fits"].din_a), _nb1(C["edge_actor_refused"].din_a)) == (13, 14) and m.head_bucket(C["edge_actor_fits"].n) == 16
    assert (_nb1(C["edge_critic_fits"].din_c), _nb1(C["edge_critic_refused"].din_c)) == (15, 16) and m.head_bucket(C["edge_critic_fits"].n) == 8
    assert m.h2_net_bytes(208, 16, 3) == 162880 and m.h2_net_bytes(240, 8, 3) == 162848


def test_shapes_reach_their_paths():
    C = m.CASES
    DP, FAST_X = 6, 12  # rec_step_h2.hip: ring depth of the pre_torso fragments, nb1 limit of the register-staged x tile
    widths = sorted(s.din_a for s in C.values() if s.family == "widths")
    assert widths == sorted(s.din_c for s in C.values() if s.family == "widths") == [1, 16, 96, 97, 192, 193, 250]
    assert [_nb1(d) for d in widths] == [1, 1, DP, DP + 1, FAST_X, FAST_X + 1, 16]
    for n, s in C.items():
        rt = m.pick_rt(s.ta, s.tc)
        if s.family in ("heads", "continuous", "widths", "critic"):
            assert rt == 1 and s.ta >= 2 and s.tc >= 2, n
        if s.family == "rt2":
            assert rt == 2, n
        if s.family in ("rt3", "edge"):
            assert rt == 3, n
        if s.form == "env":
            assert s.ta == s.tc * s.A and s.tc >= 2
    for n in ("rt2_none", "rt2_all", "rt2_random", "rt2_odd_tiles"):  # ragged last group in both networks
        assert C[n].ta % 2 == 1 and C[n].tc % 2 == 1 and m.head_bucket(C[n].n) == 16
    s = C["rt3_config4"]
    assert s.ta % 3 == 1 and s.tc % 3 == 1 and (s.din_a, s.din_c, s.n) == (155, 188, 13) and _nb1(s.din_a) <= FAST_X
    s = C["rt3_groups_over_cus"]
    assert -(-s.ta // 3) + -(-s.tc // 3) > m.CUS
    # the exact kernel's persistent tile loops, in both networks
    assert any(b[0] < C[n].ta and b[1] < C[n].tc for n in NAMES for b in [m.f32_blocks(C[n].ta, C[n].tc)])
    assert {s.resets for s in C.values() if m.pick_rt(s.ta, s.tc) >= 2} == {"none", "all", "random", "odd_tiles"}
    assert {s.A for s in C.values() if s.form == "env"} == {4, 8} and any(s.form == "shared" for s in C.values())
    assert {s.row_offset for s in C.values()} == {0, 1000} and m.SEED >> 32 and m.SEED & 0xFFFFFFFF
    heads = {(s.n, s.masked) for s in C.values() if s.family == "heads"}
    assert heads == {(n, k) for n in (1, 2, 8, 9, 16, 17, 32) for k in (False, True)}
    assert all(s.greedy == (0, 1) for s in C.values() if s.family in ("heads", "continuous"))
    assert sorted(s.n for s in C.values() if s.family == "continuous") == [1, 8, 9, 16]


@pytest.mark.parametrize("name", NAMES)
def test_case_reference(name):
    """On the float64 reference alone: resets are where the case says, every row is real, rows without a legal action are
    there, and at most 1 % of the rows are undecided (the two best Gumbel scores closer than 4 x the logit error that the 1e-5
    form allows).  Cases that run greedy keep every row's two best logits further apart than that, so the arg-max is one."""
    c = m.case(name)
    s = c["spec"]
    Ra, Rc = c["rows_a"], c["rows_c"]
    for flags, rows in ((c["done_a"] != 0, Ra), (c["done_c_rows"], Rc)):
        assert flags.shape == (rows,)
        tiles = flags.reshape(-1, 32)
        if s.resets == "none":
            assert not flags.any()
        elif s.resets == "all":
            assert flags.all()
        elif s.resets == "random":
            assert 0.15 < flags.mean() < 0.45 and (tiles.any(1) & ~tiles.all(1)).all(), "every tile mixes reset and kept rows"
        elif s.form == "env" and rows == Rc:
            assert 0.4 < flags.mean() < 0.6  # agent 0's flags of the actor's alternating tiles
        else:
            assert np.array_equal(tiles.all(1), np.arange(rows // 32) % 2 == 1) and not tiles[::2].any()
    assert np.isfinite(c["ha_new"]).all() and np.isfinite(c["hc_new"]).all() and c["ha_new"].shape == (Ra, m.H)
    if s.resets != "none":  # a reset changes the result: the state entering the step matters
        kept, _ = m.forward(c["pa"], s.din_a, s.n, c["x"], np.zeros(Ra, bool), c["ha"])
        assert np.abs(kept - c["y"])[c["done_a"] != 0].max() > 1e-3
    if s.cont:
        for g in s.greedy:  # one float32 rounding of the action stays well inside the bound on its log-density
            assert m.action_ulp_reach(c, g) < 0.25
        return
    dead = c["dead"]
    assert dead.sum() == len(s.dead_rows)
    if s.masked:
        assert not c["mask"][dead].any() and c["mask"][~dead].any(1).all() and not c["mask"].all()
        assert np.allclose(c["logp"][dead], -np.log(s.n), rtol=0, atol=1e-12) and (c["sampled"][dead] == 0).all()
    else:
        assert c["mask"] is None and not dead.any()
    assert c["decided"][dead].all()
    assert np.array_equal(np.argmax(c["scores"], -1), c["sampled"]), "the sampled action is the arg-max of the Gumbel scores"
    assert (~c["decided"]).mean() <= m.UNDECIDED_CAP
    if 1 in s.greedy:
        assert c["greedy_gap"].min() > c["clear"]
