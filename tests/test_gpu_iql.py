"""GPU: rec_iql's kernels and learner against the float64 model of tests/iql_model.py (tolerances as in
tests/test_gpu_rec.py), run_experiment and learning on LBF."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import rec_oracle as ro
from tests import iql_model as qm
from tests import lbf_model as lm
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = ("agent_pos", "agent_level", "food_pos", "food_level", "food_alive", "total_food_level", "step_count",
                "run_return", "run_length", "ep_return", "ep_length")


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(dev)


def _to_t32(a):
    rows, N = a.shape
    return a.reshape(rows // 32, 32, N).transpose(0, 2, 1).reshape(-1).copy()


def _from_t32(flat, rows, N):
    return np.asarray(flat).reshape(rows // 32, N, 32).transpose(0, 2, 1).reshape(rows, N)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _eq(got, want, what):
    got, want = _np(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.astype(got.dtype).view(np.uint32) if got.dtype == np.float32 else got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} mismatches, first at {np.argwhere(bad)[0].tolist()}"


def _env(p, E, dev, seed, env_offset=0):
    from mava_amd.envs import LevelBasedForaging

    return LevelBasedForaging(E, p.G, p.fov, p.A, p.F, p.max_level, p.force_coop, p.time_limit, p.individual,
                              add_global_state=True, seed=seed, env_offset=env_offset, device=dev)


# ---- 1. LBF with its pre-reset observation --------------------------------------------------------------------------
def test_lbf_real_next_matches_model(dev):
    p = lm.Params(G=5, fov=2, A=3, F=1, max_level=2, force_coop=False, time_limit=6)
    E, seed, off = 500, 0x1234ABCD, 77
    env, twin = _env(p, E, dev, seed, off), _env(p, E, dev, seed, off)
    st, obs = env.alloc_state(), env.alloc_obs()
    st2, obs2 = twin.alloc_state(), twin.alloc_obs()
    env.step_into(st, 0, obs, is_reset=True)
    twin.step_into(st2, 0, obs2, is_reset=True)
    mst, _ = lm.reset(p, E, seed, off, 0)
    rng = np.random.default_rng(5)
    rv, rm = torch.empty((E, p.A, p.obs_dim), device=dev), torch.empty((E, p.A, 6), dtype=torch.uint8, device=dev)
    term = torch.empty(E, dtype=torch.uint8, device=dev)
    bufs = lambda: (torch.empty((E, p.A), device=dev), torch.empty((E, p.A), dtype=torch.uint8, device=dev),
                    torch.empty(E, device=dev), torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
    n_term = n_trunc = 0
    for t in range(1, 25):
        act = rng.integers(0, 6, (E, p.A)).astype(np.int32)
        act[rng.random((E, p.A)) < 0.5] = lm.LOAD
        a = _t(act, dev)
        b1, b2 = bufs(), bufs()
        env.step_into(st, t, obs, *b1, action=a, real_obs={"agents_view": rv, "action_mask": rm}, terminated=term)
        twin.step_into(st2, t, obs2, *b2, action=a)
        (mobs, rew, done, ir, il, it), real = qm.lbf_step_real(p, mst, act, seed, off, t)
        for k in ("agents_view", "global_state", "action_mask", "step_count"):
            _eq(obs[k], mobs[k], f"t={t} {k}")
            _eq(obs2[k], mobs[k], f"t={t} plain {k}")
        for got, want, name in zip(b1, (rew, done, ir, il, it), ("reward", "done", "info_return", "info_length", "info_terminal")):
            _eq(got, want, f"t={t} {name}")
        for x, y in zip(b1, b2):
            _eq(x, _np(y), f"t={t} plain vs real_next")
        _eq(rv, real["agents_view"], f"t={t} real_view")
        _eq(rm, real["action_mask"], f"t={t} real_mask")
        _eq(term, real["terminated"], f"t={t} terminated")
        for k in STATE_FIELDS:
            _eq(getattr(st, k), mst[k], f"t={t} state {k}")
        cont = it == 0
        _eq(rv[_t(cont, dev, torch.bool)], mobs["agents_view"][cont], "real_view equals the observation where the step did not end")
        n_term += int(real["terminated"].sum())
        n_trunc += int(((it == 1) & (real["terminated"] == 0)).sum())
    assert n_term > 20 and n_trunc > 20, (n_term, n_trunc)


# ---- 2. the acting step -----------------------------------------------------------------------------------------------
def _q_step(dev, flat, x, mask, done, h, eps, seed=99, step=3, q_out=True, row_offset=0):
    from mava_amd._lib import check, lib, ptr, stream_ptr

    R, O = x.shape
    nA = mask.shape[1]
    xs, ms, ds = _t(x, dev), _t(mask, dev, torch.uint8), _t(done, dev, torch.uint8)
    hi, ho = _t(_to_t32(h.astype(np.float32)), dev), torch.empty(R * 128, device=dev)
    act, q = torch.empty(R, dtype=torch.int32, device=dev), torch.empty((R, nA), device=dev)
    fl = _t(flat, dev)
    check(lib().mava_rec_q_step_f32(ptr(fl), O, nA, ptr(xs), ptr(ms), ptr(ds), ptr(hi), ptr(ho), R, eps, seed, step, row_offset,
                                    ptr(act), ptr(q) if q_out else None, stream_ptr()), "mava_rec_q_step_f32")
    return _np(act), _np(q), _from_t32(_np(ho), R, 128)


def _q_case(R=64, real=48, O=21, nA=6, seed=0, no_valid=()):
    """no_valid: real rows whose mask is all zero (no valid action: the kernel answers action 0)."""
    rng = np.random.default_rng(seed)
    flat = ro.init_rec(rng, O, nA, 0.01).astype(np.float32)
    # a larger head so that the Q-values spread (the greedy choice is then not decided by rounding)
    flat[-(128 * nA + nA):] *= 100.0
    x = np.zeros((R, O), np.float32)
    x[:real] = rng.standard_normal((real, O)).astype(np.float32)
    mask = np.zeros((R, nA), bool)
    mask[:real] = rng.random((real, nA)) < 0.6
    mask[:real, 0] = True
    mask[list(no_valid)] = False
    done = np.zeros(R, bool)
    done[:real] = rng.random(real) < 0.3
    h = np.zeros((R, 128), np.float32)
    h[:real] = rng.standard_normal((real, 128)).astype(np.float32) * 0.5
    return flat, x, mask, done, h


# (rows, real rows, din, actions, row_offset, q_out given)
Q_STEP_CASES = [
    (64, 48, 21, 6, 0, True),
    (64, 48, 16, 11, 0, True),       # one 16-input batch; the 16-wide instantiation
    (96, 96, 40, 16, 12345, True),   # an odd number of input batches, 16 actions, a row offset in the Philox counter
    (64, 64, 155, 1, 0, True),       # a single action
    (8288, 8288, 37, 6, 7, False),   # 259 tiles on 256 blocks: three blocks walk a second tile; q_out = None as the learner calls it
]


@pytest.mark.parametrize("R,real,O,nA,row_offset,q_out", Q_STEP_CASES)
def test_q_step_matches_oracle(dev, R, real, O, nA, row_offset, q_out):
    no_valid = (5, 17, real - 1)
    flat, x, mask, done, h = _q_case(R, real, O, nA, no_valid=no_valid)
    assert not mask[list(no_valid)].any() and mask[:real].any(-1).sum() == real - 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    y, hn = ro.t_rec_forward(t(flat), x.shape[1], nA, t(x[None]), torch.from_numpy(done[None]), t(h))
    valid = mask.any(-1)
    for eps in (0.0, 0.3, 1.0):
        act, q, h_out = _q_step(dev, flat, x, mask, done, h, eps, row_offset=row_offset, q_out=q_out)
        if not q_out:  # the Q-values of a second call that writes them; the two calls must agree bit for bit
            act2, q, h2 = _q_step(dev, flat, x, mask, done, h, eps, row_offset=row_offset, q_out=True)
            _eq(act, act2, f"actions with and without q_out at eps={eps}")
            _eq(h_out, h2, f"hidden state with and without q_out at eps={eps}")
        assert_close(q[:real], y[0].numpy()[:real], 1e-5, "q_out")
        assert_close(h_out[:real], hn.numpy()[:real], 1e-5, "hidden state")
        want, greedy = qm.eps_greedy(q, mask, np.float32(eps), 99, 3, row_offset)  # the greedy part from the kernel's own q
        _eq(act, want.astype(np.int32), f"actions at eps={eps}")
        if eps == 0.0:
            _eq(act, np.where(mask, q, qm.F32_MIN).argmax(-1).astype(np.int32), "greedy actions")
        assert (act[real:] == 0).all()  # padding rows: all-zero masks
        assert (act[~valid] == 0).all()  # and real rows without a valid action
        assert mask[valid, act[valid]].all()
        if eps == 1.0 and nA > 1:
            assert (act != greedy)[valid].any()  # exploration happened


def test_q_step_frequencies(dev):
    """Chi-square of the action frequencies of 8192 identical rows at eps = 0.5 against MaskedEpsGreedyDistribution."""
    flat, x, mask, done, h = _q_case(R=64, real=64, seed=4)
    R = 8192
    xs, ms, ds, hs = (np.repeat(a[:1], R, 0) for a in (x, mask, done, h))
    act, q, _ = _q_step(dev, flat, xs, ms, ds, hs, 0.5, seed=1234, step=0)
    m0 = ms[0]
    probs = 0.5 * m0 / m0.sum()
    probs[np.where(m0, q[0], qm.F32_MIN).argmax()] += 0.5
    counts = np.bincount(act, minlength=6)
    assert counts[~m0].sum() == 0
    valid = m0.nonzero()[0]
    exp = probs[valid] * R
    chi2 = float((((counts[valid] - exp) ** 2) / exp).sum())
    crit = {1: 10.83, 2: 13.82, 3: 16.27, 4: 18.47, 5: 20.52}[len(valid) - 1]  # p = 0.001
    assert chi2 < crit, (chi2, counts, exp)


# ---- 3. replay -------------------------------------------------------------------------------------------------------
def _replay_run(dev, S):
    """Adds 2 * cap + 2 steps and samples after each one that leaves a window; returns the (n_added, pairs) of every sample."""
    from mava_amd._lib import check, lib, ptr, stream_ptr

    E, A, O, nA, cap, B = 7, 3, 5, 6, 9, 11
    drawn = []
    Rp = -(-(B * A) // 32) * 32
    rng = np.random.default_rng(2)
    rb = qm.Replay(E, A, O, nA, cap)
    u8 = torch.uint8
    buf = [torch.zeros((E, cap, A, O), device=dev), torch.zeros((E, cap, A, nA), dtype=u8, device=dev),
           torch.zeros((E, cap, A), dtype=torch.int32, device=dev), torch.zeros((E, cap, A), device=dev),
           torch.zeros((E, cap, A), dtype=u8, device=dev), torch.zeros((E, cap, A), dtype=u8, device=dev),
           torch.zeros((E, cap, A, O), device=dev), torch.zeros((E, cap, A, nA), dtype=u8, device=dev)]
    for n in range(1, 2 * cap + 3):
        f = [rng.standard_normal((E, A, O)).astype(np.float32), rng.integers(0, 2, (E, A, nA)).astype(np.uint8),
             rng.integers(0, nA, (E, A)).astype(np.int32), rng.standard_normal((E, A)).astype(np.float32),
             rng.integers(0, 2, E).astype(np.uint8), rng.integers(0, 2, (E, A)).astype(np.uint8),
             rng.standard_normal((E, A, O)).astype(np.float32), rng.integers(0, 2, (E, A, nA)).astype(np.uint8)]
        dv = [_t(a, dev) for a in f]
        check(lib().mava_replay_add_f32(E, A, O, nA, cap, rb.n_added % cap, *[ptr(a) for a in dv], *[ptr(b) for b in buf],
                                        stream_ptr()), "mava_replay_add_f32")
        rb.add(*f)
        for k, b in zip(("obs", "mask", "action", "reward", "terminal", "tot", "next_obs", "next_mask"), buf):
            _eq(b, rb.f[k], f"add {n}: {k}")
        if n < S:
            continue
        out = [torch.full((S, Rp, O), 7.0, device=dev), torch.full((S, Rp, nA), 7, dtype=u8, device=dev),
               torch.full((S, Rp), 7, dtype=torch.int32, device=dev), torch.full((S, Rp), 7.0, device=dev),
               torch.full((S, Rp), 7, dtype=u8, device=dev), torch.full((S, Rp), 7, dtype=u8, device=dev),
               torch.full((S, Rp, O), 7.0, device=dev), torch.full((S, Rp, nA), 7, dtype=u8, device=dev)]
        pairs = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        check(lib().mava_replay_sample_f32(E, A, O, nA, cap, rb.n_added, B, S, Rp, 0xABCDEF12345, n, *[ptr(b) for b in buf],
                                           *[ptr(o) for o in out], ptr(pairs), stream_ptr()), "mava_replay_sample_f32")
        smp, want_pairs = rb.sample(0xABCDEF12345, n, B, S, Rp)
        _eq(pairs, want_pairs, f"sample {n}: pairs")
        for k, o in zip(("obs", "mask", "action", "reward", "terminal", "tot", "next_obs", "next_mask"), out):
            _eq(o, smp[k], f"sample {n}: {k}")
        drawn.append((rb.n_added, _np(pairs)))
    return cap, drawn


def test_replay_add_and_sample_match_model(dev):
    cap, drawn = _replay_run(dev, 4)
    assert len(drawn) == 2 * cap + 2 - 3
    starts = np.concatenate([p[:, 1] for _, p in drawn])
    assert len(set(starts.tolist())) > 1  # several windows to choose from


def test_replay_sample_window_of_the_whole_buffer(dev):
    """S == capacity: exactly one valid window, and it starts at the oldest slot (the write head)."""
    cap, drawn = _replay_run(dev, 9)
    assert [n for n, _ in drawn] == list(range(cap, 2 * cap + 3))
    for n, pairs in drawn:
        assert (pairs[:, 1] == n % cap).all(), (n, pairs[:, 1])


# ---- 4. TD loss --------------------------------------------------------------------------------------------------------
def _td_case(L, Rp, n_real, nA):
    """Inputs with the three fixtures every case must hold: exact ties of the masked maximum (the first index wins), a
    masked maximum (never chosen), and terminal rows (no bootstrap).  A single action admits no tie between two entries
    and its only entry is the maximum: there the masked-maximum rows have NO valid action (the argmax is still index 0)."""
    rows = L * Rp
    rng = np.random.default_rng(8)
    q, qn, qt = (rng.standard_normal((rows, nA)).astype(np.float32) for _ in range(3))
    t1, t2 = (2, 4) if nA >= 5 else (max(nA - 2, 0), nA - 1)
    qn[: rows // 4, t1] = qn[: rows // 4, t2] = 5.0    # exact ties: the first index wins
    mask = rng.random((L, Rp, nA)) < 0.5
    mask[:, :, 0] = True
    big = 1 if nA > 1 else 0
    qn[rows // 4 : rows // 2, big] = 50.0              # a masked maximum: never chosen where that action is invalid
    if nA == 1:
        mask.reshape(rows, nA)[rows // 4 : rows // 2 : 2] = False
    act = rng.integers(0, nA, (L, Rp)).astype(np.int32)
    rew = rng.standard_normal((L, Rp)).astype(np.float32)
    term = (rng.random((L, Rp)) < 0.3).astype(np.uint8)  # terminal rows do not bootstrap, truncated ones (0) do
    # the fixtures are there, among the real rows
    real = np.arange(Rp) < n_real
    z = np.where(mask, qn.reshape(L, Rp, nA), qm.F32_MIN)
    if nA > 1:
        tied = (z == z.max(-1, keepdims=True)).sum(-1) >= 2
        assert tied[:, real].any() and (z.argmax(-1) == t1)[tied & real].any()
    hidden = qn.reshape(L, Rp, nA).argmax(-1) != z.argmax(-1) if nA > 1 else ~mask[..., 0]
    assert hidden[:, real].any()
    assert term[:, real].any() and not term[:, real].all()
    return q, qn, qt, mask, act, rew, term


def _td_run(dev, case, L, Rp, n_real, nA, nblk, gamma=0.99, gs=256.0):
    from mava_amd._lib import check, lib, ptr, stream_ptr

    q, qn, qt, mask, act, rew, term = case
    rows = L * Rp
    dq, part = torch.full((rows * nA,), 9.0, device=dev), torch.full((nblk, 3), 9.0, device=dev)
    ins = [_t(_to_t32(a), dev) for a in (q, qn, qt)] + [_t(a, dev) for a in (act, rew, term, mask.astype(np.uint8))]  # kept alive
    check(lib().mava_q_td_loss_f32(L, Rp, nA, n_real, *[ptr(a) for a in ins], gamma, gs, ptr(dq), ptr(part), nblk, stream_ptr()),
          "mava_q_td_loss_f32")
    return _np(dq), _np(part)


def _td_check(case, L, Rp, n_real, nA, dq, part, gamma=0.99, gs=256.0):
    q, qn, qt, mask, act, rew, term = case
    rows = L * Rp
    q3, qn3, qt3 = (a.reshape(L, Rp, nA).astype(np.float64) for a in (q, qn, qt))
    a_star = np.where(mask, qn3, qm.F32_MIN).argmax(-1)
    target = rew + (1.0 - term) * gamma * np.take_along_axis(qt3, a_star[..., None], -1)[..., 0]
    qa = np.take_along_axis(q3, act[..., None].astype(np.int64), -1)[..., 0]
    real = np.arange(Rp) < n_real
    N = L * n_real
    want_dq = np.zeros((L, Rp, nA))
    np.put_along_axis(want_dq, act[..., None].astype(np.int64), (2.0 * (qa - target) / N * gs)[..., None], -1)
    want_dq[:, ~real] = 0.0
    got = _from_t32(dq, rows, nA).reshape(L, Rp, nA)
    assert_close(got, want_dq, 1e-6, "dQ")
    metrics = part.sum(0)
    d = (qa - target)[:, real]
    assert_close(metrics, np.array([(d ** 2).mean(), qa[:, real].mean(), target[:, real].mean()]), 1e-5, "metrics")


# (L, Rp, real rows, actions, blocks)
TD_CASES = [
    (5, 32, 27, 6, 3),
    (20, 96, 96, 6, 8),    # the learner's launch at the reference defaults: 1920 rows, no padding rows
    (20, 96, 96, 6, 1),    # one block strides eight times
    (20, 96, 96, 6, 16),   # idle blocks
    (3, 64, 33, 32, 2),    # padding rows that start inside the second tile; the widest head
    (2, 32, 32, 1, 1),     # a single action
]


@pytest.mark.parametrize("L,Rp,n_real,nA,nblk", TD_CASES)
def test_td_loss_matches_f64(dev, L, Rp, n_real, nA, nblk):
    case = _td_case(L, Rp, n_real, nA)
    dq, part = _td_run(dev, case, L, Rp, n_real, nA, nblk)
    _td_check(case, L, Rp, n_real, nA, dq, part)
    idle = np.arange(nblk) * 256 >= L * Rp
    assert (part[idle] == 0.0).all()  # a block without rows contributes exact zeros


def test_td_loss_gradient_is_independent_of_the_block_count(dev):
    """The three launches of the learner's shape: dQ bit-identical whatever the grid, the metrics at 1e-5 each."""
    L, Rp, n_real, nA = 20, 96, 96, 6
    case = _td_case(L, Rp, n_real, nA)
    runs = {nblk: _td_run(dev, case, L, Rp, n_real, nA, nblk) for nblk in (8, 1, 16)}
    for nblk, (dq, part) in runs.items():
        _td_check(case, L, Rp, n_real, nA, dq, part)
        _eq(dq, runs[8][0], f"dQ with {nblk} blocks against 8")


# ---- 5. target update --------------------------------------------------------------------------------------------------
def test_target_update(dev):
    from mava_amd._lib import check, lib, ptr, stream_ptr

    rng = np.random.default_rng(1)
    n = 300001
    on, tg = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    o, t = _t(on, dev), _t(tg, dev)
    check(lib().mava_target_update_f32(n, ptr(o), ptr(t), 0.01, 0, stream_ptr()), "mava_target_update_f32")
    assert_close(_np(t), 0.01 * on.astype(np.float64) + 0.99 * tg, 1e-6, "soft update")
    check(lib().mava_target_update_f32(n, ptr(o), ptr(t), 0.0, 1, stream_ptr()), "mava_target_update_f32")
    _eq(t, on, "hard update")


# ---- 6. one learn() call against the model ------------------------------------------------------------------------------
def _learner_case(dev, mode, extra=()):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.iql_learner import learner_setup

    cfg = compose("default_rec_iql", ["env/scenario=2s-10x10-3p-3f", "arch.num_envs=16", "system.sample_batch_size=9",
                                      "system.sample_sequence_length=4", "system.min_buffer_size=4", "system.buffer_size=8",
                                      f"system.matmul_mode={mode}", "system.num_updates_per_eval=6", "system.q_lr=1e-3",
                                      "system.eps_decay=400", *extra])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    host = {k: _np(getattr(L.state, k)).copy() for k in STATE_FIELDS}
    obs = {"agents_view": _np(L.view[0][: L.EA]).reshape(16, 3, -1), "action_mask": _np(L.mask[0][: L.EA]).reshape(16, 3, 6)}
    model = qm.IQLModel(lm.params_of(env), cfg, _np(L.p), host, obs, env.seed, env.env_offset, L.seed)
    return learn, L, state, model


def _compare_params(got, want, what, f16x2):
    got = np.asarray(got, np.float64)
    if f16x2:  # conftest.check_and_sync_f16x2_state's allowance, restated for the Q network
        bad = np.abs(got - want) > 1e-4 * (np.abs(want) + np.sqrt(np.mean(want * want)))
        assert bad.sum() <= max(12, 5e-4 * bad.size), f"{what}: {int(bad.sum())} entries outside 1e-4"
        assert_close(got, want, 1e-3, f"{what} (hard bound)")
    else:
        assert_close(got, want, 1e-5, what)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_learn_matches_model(dev, mode):
    learn, L, state, model = _learner_case(dev, mode, ["system.hard_update=true", "system.update_period=3"] if mode == "f16x2" else [])
    out = learn(state)
    torch.cuda.synchronize()
    n_train = sum(L.trained)
    assert L.trained[:2] == [False, False] and all(L.trained[2:]) and n_train == 4  # gate: 5 steps per env row
    assert set(out.train_metrics) == {"q_loss", "mean_q", "mean_target"} and out.train_metrics["q_loss"].shape == (4, 2)
    k = 0
    f16 = mode == "f16x2"
    for n in range(L.n_upd):
        for t in range(L.T):
            model.act(_np(L.debug["actions"][n * L.T + t]))
        if n < 2:
            continue
        for e in range(L.K):
            r = model.train()
            _eq(L.debug["pairs"][k], r["pairs"], f"train step {k}: sampled pairs")
            gm = _np(L.train_metrics[n, e]).astype(np.float64)
            assert_close(gm, np.array([r["q_loss"], r["mean_q"], r["mean_target"]]), 1e-4 if f16 else 1e-5, f"step {k} metrics")
            if f16:  # split-f16 forward and backward products: a handful of small entries move further
                g, w = _np(L.debug["grads"][k]).astype(np.float64), r["grad"]
                bad = np.abs(g - w) > 1e-3 * (np.abs(w) + np.sqrt(np.mean(w * w)))
                assert bad.sum() <= max(12, 5e-4 * bad.size), f"step {k} gradient: {int(bad.sum())} entries outside 1e-3"
                assert_close(g, w, 1e-2, f"step {k} gradient (hard bound)")
            else:
                assert_close(_np(L.debug["grads"][k]), r["grad"], 1e-4, f"step {k} gradient")
            k += 1
    for key, b in zip(("obs", "mask", "action", "reward", "terminal", "tot", "next_obs", "next_mask"),
                      (L.buf.obs[0], L.buf.obs[1], L.buf.action, L.buf.reward, L.buf.terminal, L.buf.term_or_trunc,
                       L.buf.next_obs[0], L.buf.next_obs[1])):
        _eq(b, model.replay.f[key], f"buffer {key}")
    _compare_params(_np(L.p), model.online, "online params", f16)
    _compare_params(_np(L.pt), model.target, "target params", f16)


# ---- 7. run_experiment ----------------------------------------------------------------------------------------------------
def test_run_experiment_logs_every_event(dev, tmp_path, monkeypatch):
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    monkeypatch.chdir(tmp_path)
    cfg = compose("default_rec_iql", ["env/scenario=2s-10x10-3p-3f", "arch.num_envs=16", "system.total_timesteps=512",
                                      "arch.num_evaluation=2", "system.sample_sequence_length=4", "system.min_buffer_size=4",
                                      "system.buffer_size=64", "arch.num_eval_episodes=16",
                                      "arch.num_absolute_metric_eval_episodes=16", "logger.checkpointing.save_model=true"])
    recs = []
    ret = rec_iql.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    for ev in ("MISC", "TRAIN", "EVAL", "ABSOLUTE"):
        assert ev in events, events
    misc = [r for r in recs if r["event"] == "MISC"]
    assert [r["timestep"] for r in misc] == [256, 512] and 0.05 <= misc[-1]["epsilon"] <= 1.0
    assert ret == pytest.approx([r for r in recs if r["event"] == "EVAL"][-1]["episode_return"])
    assert np.isfinite([r["q_loss"] for r in recs if r["event"] == "TRAIN"]).all()
    # the checkpoint holds online and target parameters and restores them
    from mava_amd.utils.checkpointing import Checkpointer

    ck = Checkpointer(model_name="rec_iql", checkpoint_uid=os.listdir(os.path.join(tmp_path, "checkpoints", "rec_iql"))[0])
    raw = ck.restore_learner_state_raw()
    assert set(raw["params"]) == {"online", "target"}


# ---- 8. learning --------------------------------------------------------------------------------------------------------
def test_rec_iql_learns_lbf(dev):
    from mava_amd.config import compose
    from mava_amd.systems.q_learning import rec_iql

    with open(os.path.join(ROOT, "profiles", "iql_learning_curve.json")) as f:
        curve = json.load(f)
    cfg = compose("default_rec_iql", curve["overrides"])
    recs = []
    rec_iql.run_experiment(cfg, log=recs.append)
    ev = [r["episode_return"] for r in recs if r["event"] == "EVAL"]
    measured = curve["measured_gain"]
    assert measured > 0.1
    got = sum(ev[-3:]) / 3.0 - ev[0]  # tools/iql_bench.py gain()
    assert got > 0.4 * measured, (ev, measured)  # the bar sits under half the measured gain
