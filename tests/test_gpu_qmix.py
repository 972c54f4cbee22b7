"""GPU: the two value-decomposition kernels (mava_amd/csrc/qmix.hip) against NumPy / float64 autograd, the learner
against the float64 model of tests/qmix_model.py step by step, and run_experiment with its checkpoint.

mava_amd/iql_learner.py is not edited by the value-decomposition systems (QMIXLearner subclasses IQLLearner and overrides
methods), so there is no "rec_iql is untouched" comparison against an older class here: tests/test_gpu_iql.py pins it.
"""
import os

import numpy as np
import pytest
import torch

from tests import lbf_model as lm
from tests import qmix_model as xm
from tests.conftest import assert_close
from tests.iql_model import F32_MIN
from tests.test_gpu_iql import STATE_FIELDS, _compare_params, _eq, _from_t32, _np, _t, _to_t32

pytestmark = pytest.mark.gpu

c32 = lambda n: -(-n // 32) * 32


# ---- 1. the mixer's state matrices ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,A,O", [
    (3, 9, 3, 21),    # one tile per step, padding rows
    (2, 33, 2, 7),    # padding starts inside the second tile; Ds = 14 is no multiple of 32
    (2, 32, 16, 5),   # no padding rows
])
def test_state_gather_is_bit_exact(dev, L, B, A, O):
    from mava_amd._lib import check, lib, ptr, stream_ptr

    rng = np.random.default_rng(L * 100 + B)
    S, Rp, Bp, Ds = L + 1, c32(B * A), c32(B), A * O
    kp = c32(Ds)
    obs, nxt = (rng.standard_normal((S, Rp, O)).astype(np.float32) for _ in range(2))  # padding rows hold values: they must not leak
    d_obs, d_nxt = _t(obs, dev), _t(nxt, dev)
    out = [torch.full((L * Bp * kp,), 9.0, device=dev) for _ in range(2)]
    check(lib().mava_qmix_state_t32_f32(L, B, A, O, Rp, kp, ptr(d_obs), ptr(d_nxt), ptr(out[0]), ptr(out[1]), stream_ptr()),
          "mava_qmix_state_t32_f32")
    for src, got, what in ((obs, out[0], "state"), (nxt, out[1], "next_state")):
        want = np.zeros((L, Bp, kp), np.float32)
        want[:, :B, :Ds] = src[:L, : B * A].reshape(L, B, Ds)
        _eq(_from_t32(_np(got), L * Bp, kp), want.reshape(L * Bp, kp), what)


# ---- 2. the TD loss through the mixer -------------------------------------------------------------------------------
def _td_case(L, B, A, nA, Em):
    """Random inputs, built like tests/test_gpu_iql.py::_td_case, with the fixtures every case must hold among its REAL
    rows: exact ties of the masked maximum (the first index wins), a masked maximum (never chosen; with a single action:
    rows without a valid action), terminal and non-terminal samples, raw w1 / w2 of both signs, pre-elu values of both
    signs, and per-agent rewards that differ within a sample."""
    rng = np.random.default_rng(8)
    Rp, Bp, n_real = c32(B * A), c32(B), B * A
    q, qn, qt = (rng.standard_normal((L, Rp, nA)).astype(np.float32) for _ in range(3))
    mask = rng.random((L, Rp, nA)) < 0.5
    mask[:, :, 0] = True
    m = np.arange(Rp)
    tie_rows, hid_rows = m[m % 4 == 0], m[m % 4 == 1] if n_real > 1 else m[:1]
    t1, t2 = (2, 4) if nA >= 5 else (max(nA - 2, 0), nA - 1)
    if nA > 1:
        qn[:, tie_rows, t1] = qn[:, tie_rows, t2] = 5.0  # exact ties: the first index wins
        mask[:, tie_rows, t1] = mask[:, tie_rows, t2] = True
        qn[:, hid_rows, 1] = 50.0                        # a masked maximum
        mask[:, hid_rows, 1] = False
    else:
        mask[:, hid_rows, 0] = False                     # no valid action: the argmax is still index 0
    act = rng.integers(0, nA, (L, Rp)).astype(np.int32)
    rew = rng.standard_normal((L, Rp)).astype(np.float32)
    term = (rng.random((L, Rp)) < 0.3).astype(np.uint8)
    mrows = L * Bp
    hyp = [rng.standard_normal((mrows, n)).astype(np.float32) for n in (A * Em, Em, Em, 1)]
    hyp_t = [rng.standard_normal((mrows, n)).astype(np.float32) for n in (A * Em, Em, Em, 1)]
    # ---- the fixtures are there, among the real rows
    real = m < n_real
    z = np.where(mask, qn, F32_MIN)
    if nA > 1:
        tied = (z == z.max(-1, keepdims=True)).sum(-1) >= 2
        assert tied[:, real].any() and (z.argmax(-1) == t1)[tied & real].any()
        assert (qn.argmax(-1) != z.argmax(-1))[:, real].any()
    else:
        assert (~mask[..., 0])[:, real].any()
    t0 = term[:, : n_real : A]  # agent 0's flag is the sample's
    assert t0.any() and not t0.all()
    if A > 1:
        r3 = rew[:, :n_real].reshape(L, B, A)
        assert (r3.max(-1) > r3.min(-1)).all()
    breal = (np.arange(Bp) < B)[None].repeat(L, 0).reshape(-1)
    for w in (hyp[0], hyp[2], hyp_t[0], hyp_t[2]):
        assert (w[breal] > 0).any() and (w[breal] < 0).any()
    return {"L": L, "B": B, "A": A, "nA": nA, "Em": Em, "Rp": Rp, "Bp": Bp, "q": q, "qn": qn, "qt": qt, "mask": mask, "act": act,
            "rew": rew, "term": term, "hyp": hyp, "hyp_t": hyp_t}


def _td_want(c, qmix, gamma=0.99, gs=256.0):
    """float64 autograd of the mixer + loss alone: (dq (L, Rp, nA), [d_w1, d_b1, d_w2, d_b2] (L*Bp, n), metrics)."""
    L, B, A, nA, Rp, Bp = c["L"], c["B"], c["A"], c["nA"], c["Rp"], c["Bp"]
    n_real = B * A
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    q = t(c["q"]).requires_grad_(True)
    sel = lambda x: x[:, :n_real]
    mask = torch.from_numpy(c["mask"][:, :n_real])
    z = torch.where(mask, sel(t(c["qn"])), torch.full((L, n_real, nA), float(F32_MIN), dtype=torch.float64))
    # torch's argmax may return any index on exact ties: take the FIRST maximum, which is the contract
    a_star =(z == z.max(-1, keepdim=True).values).double().argmax(-1)
    nq = sel(t(c["qt"])).gather(-1, a_star.unsqueeze(-1))[..., 0].reshape(L, B, A)
    qa = sel(q).gather(-1, torch.from_numpy(c["act"][:, :n_real]).long().unsqueeze(-1))[..., 0].reshape(L, B, A)
    real_m = lambda x: x.reshape(L, Bp, -1)[:, :B]
    hyp = [t(h).requires_grad_(True) for h in c["hyp"]]
    if qmix:
        q_tot, pre = xm.mix_raw(qa, *[real_m(h) for h in hyp], with_pre=True)
        assert (pre > 0).any() and (pre < 0).any()  # both branches of the elu
        q_tot_t = xm.mix_raw(nq, *[real_m(t(h)) for h in c["hyp_t"]])
    else:
        q_tot, q_tot_t = qa.sum(-1), nq.sum(-1)
    r = sel(t(c["rew"])).reshape(L, B, A).mean(-1)
    term = sel(t(c["term"])).reshape(L, B, A)[..., 0]
    y = (r + (1.0 - term) * gamma * q_tot_t).detach()
    loss = ((q_tot - y) ** 2).mean()
    (loss * gs).backward()
    grads = [h.grad.numpy() if (qmix and h.grad is not None) else np.zeros(tuple(h.shape)) for h in hyp]
    return q.grad.numpy(), grads, np.array([float(loss.detach()), float(q_tot.detach().mean()), float(y.mean())])


def _td_run(dev, c, qmix, nblk, gamma=0.99, gs=256.0):
    from mava_amd._lib import check, lib, ptr, stream_ptr

    L, B, A, nA, Em, Rp, Bp = (c[k] for k in ("L", "B", "A", "nA", "Em", "Rp", "Bp"))
    rows, mrows = L * Rp, L * Bp
    f3 = lambda a: _t(_to_t32(a.reshape(rows, nA)), dev)
    ins = [f3(c["q"]), f3(c["qn"]), f3(c["qt"]), _t(c["act"], dev), _t(c["rew"], dev), _t(c["term"], dev),
           _t(c["mask"].astype(np.uint8), dev)]
    hyp = [_t(_to_t32(h), dev) for h in c["hyp"] + c["hyp_t"]]
    dq, part = torch.full((rows * nA,), 9.0, device=dev), torch.full((nblk, 3), 9.0, device=dev)
    grads = [torch.full((mrows * n,), 9.0, device=dev) for n in (A * Em, Em, Em, 1)]
    hp = [ptr(h) for h in hyp] if qmix else [None] * 8
    gp = [ptr(g) for g in grads] if qmix else [None] * 4
    check(lib().mava_qmix_td_f32(int(qmix), L, B, A, Rp, nA, Em, *[ptr(a) for a in ins], *hp, gamma, gs, ptr(dq), *gp, ptr(part),
                                 nblk, stream_ptr()), "mava_qmix_td_f32")
    torch.cuda.synchronize()
    return _np(dq), [_np(g) for g in grads], _np(part)


def _ratio(got, want):
    """Worst |got - want| / (|want| + rms(want)): assert_close's form, as a number to print."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (np.abs(want) + np.sqrt(np.mean(want * want)) + 1e-300)).max())


def _td_check(c, qmix, dq, grads, part, nblk):
    L, B, A, nA, Em, Rp, Bp = (c[k] for k in ("L", "B", "A", "nA", "Em", "Rp", "Bp"))
    want_dq, want_g, want_m = _td_want(c, qmix)
    got_dq = _from_t32(dq, L * Rp, nA).reshape(L, Rp, nA)
    # the zero pattern is exact: padding agent rows and every action but the taken one
    taken = np.zeros((L, Rp, nA), bool)
    np.put_along_axis(taken, c["act"][..., None].astype(np.int64), True, -1)
    taken[:, B * A :] = False
    assert (got_dq[~taken] == 0.0).all()
    print(f"dq ratio {_ratio(got_dq, want_dq):.3g}")
    assert_close(got_dq, want_dq, 1e-6, "dq")
    if qmix:
        for g, w, n, name in zip(grads, want_g, (A * Em, Em, Em, 1), ("d_w1", "d_b1", "d_w2", "d_b2")):
            got = _from_t32(g, L * Bp, n).reshape(L, Bp, n)
            assert (got[:, B:] == 0.0).all(), f"{name}: padding mixer rows"
            print(f"{name} ratio {_ratio(got, w.reshape(L, Bp, n)):.3g}")
            assert_close(got, w.reshape(L, Bp, n), 1e-6, name)
    else:
        for g in grads:
            assert (g == 9.0).all()  # vdn: no hypernet gradient is touched
    print(f"metrics ratio {_ratio(part.sum(0), want_m):.3g}")
    assert_close(part.sum(0), want_m, 1e-5, "metrics")
    idle = np.arange(nblk) * 64 >= L * Bp
    assert (part[idle] == 0.0).all()  # a block without rows contributes exact zeros


# (L, B, A, actions, embed, blocks)
TD_CASES = [
    (5, 9, 3, 6, 32, 3),     # baseline
    (20, 32, 3, 6, 32, 8),   # the default launch
    (20, 32, 3, 6, 32, 1),   # one block strides
    (20, 32, 3, 6, 32, 16),  # idle blocks
    (3, 33, 2, 32, 8, 2),    # widest head, padding inside tile 2, B*A = 66 so Rp = 96 != Bp*A
    (2, 32, 16, 5, 32, 2),   # A*Em = 512: four 128-column blocks
    (2, 5, 1, 1, 64, 1),     # single agent, single action, widest embed
]


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
@pytest.mark.parametrize("L,B,A,nA,Em,nblk", TD_CASES)
def test_td_matches_f64_autograd(dev, L, B, A, nA, Em, nblk, mixer):
    c = _td_case(L, B, A, nA, Em)
    dq, grads, part = _td_run(dev, c, mixer == "qmix", nblk)
    _td_check(c, mixer == "qmix", dq, grads, part, nblk)


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
def test_td_gradients_are_independent_of_the_block_count(dev, mixer):
    c = _td_case(20, 32, 3, 6, 32)
    runs = {nblk: _td_run(dev, c, mixer == "qmix", nblk) for nblk in (8, 1, 16)}
    for nblk, (dq, grads, part) in runs.items():
        _eq(dq, runs[8][0], f"dq with {nblk} blocks against 8")
        for g, g8, name in zip(grads, runs[8][1], ("d_w1", "d_b1", "d_w2", "d_b2")):
            _eq(g, g8, f"{name} with {nblk} blocks against 8")


# ---- 3. argument refusals ---------------------------------------------------------------------------------------------
def test_td_refuses_bad_arguments_without_launching(dev):
    from mava_amd._lib import lib, ptr, stream_ptr

    L, B, A, nA, Em = 2, 8, 3, 6, 32
    Rp, Bp = c32(B * A), c32(B)
    z = lambda n: torch.zeros(n, device=dev)
    ins = [z(L * Rp * nA), z(L * Rp * nA), z(L * Rp * nA), torch.zeros(L * Rp, dtype=torch.int32, device=dev), z(L * Rp),
           torch.zeros(L * Rp, dtype=torch.uint8, device=dev), torch.ones(L * Rp * nA, dtype=torch.uint8, device=dev)]
    hyp = [z(L * Bp * n) for n in (A * Em, Em, Em, 1)] * 2
    outs = [torch.full((L * Rp * nA,), 9.0, device=dev)] + [torch.full((L * Bp * n,), 9.0, device=dev) for n in (A * Em, Em, Em, 1)]
    part = torch.full((4, 3), 9.0, device=dev)

    def call(mode=1, A_=A, Em_=Em, Rp_=Rp, B_=B, hyp_=None, dq=None):
        hp = [ptr(h) for h in hyp] if hyp_ is None else hyp_
        return lib().mava_qmix_td_f32(mode, L, B_, A_, Rp_, nA, Em_, *[ptr(a) for a in ins], *hp, 0.99, 1.0,
                                      ptr(outs[0]) if dq is None else dq, *[ptr(o) for o in outs[1:]], ptr(part), 4, stream_ptr())

    err = lambda: lib().mava_last_error()
    assert call(A_=17) <= -1000 and b"agents" in err()
    assert call(Em_=65) <= -1000 and b"Em=65" in err()
    assert call(B_=11) <= -1000 and b"holding B*A=33" in err()  # Rp = 32 does not hold 33 agent rows
    null_w2 = [ptr(h) for h in hyp]
    null_w2[2] = None
    assert call(hyp_=null_w2) <= -1000 and b"null hypernet pointer" in err()
    assert call(dq=ptr(ins[0])) <= -1000 and b"alias" in err()
    torch.cuda.synchronize()
    for o in outs + [part]:
        assert (o == 9.0).all()  # nothing was launched
    assert call(mode=0, hyp_=[None] * 8) == 0  # vdn takes NULL hypernet pointers
    torch.cuda.synchronize()
    assert (outs[0] == 0.0).all() and all((o == 9.0).all() for o in outs[1:])


# ---- 4. one learn() call against the model --------------------------------------------------------------------------
def _learner_case(dev, mixer, mode, extra=()):
    """tests/test_gpu_iql.py::_learner_case's configuration with the value-decomposition learner and a small mixer."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.qmix_learner import learner_setup

    cfg = compose(f"default_rec_{mixer}", ["env/scenario=2s-10x10-3p-3f", "arch.num_envs=16", "system.sample_batch_size=9",
                                           "system.sample_sequence_length=4", "system.min_buffer_size=4", "system.buffer_size=8",
                                           f"system.matmul_mode={mode}", "system.num_updates_per_eval=6", "system.q_lr=1e-3",
                                           "system.eps_decay=400", "system.mixer_embed_dim=8", "system.hypernet_hidden_dim=16", *extra])
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = learner_setup(env, (7, 11), cfg)
    L = learn.learner
    L.debug = {"grads": [], "pairs": [], "actions": []}
    host = {k: _np(getattr(L.state, k)).copy() for k in STATE_FIELDS}
    obs = {"agents_view": _np(L.view[0][: L.EA]).reshape(16, 3, -1), "action_mask": _np(L.mask[0][: L.EA]).reshape(16, 3, 6)}
    model = xm.QMIXModel(lm.params_of(env), cfg, _np(L.p), host, obs, env.seed, env.env_offset, L.seed)
    return learn, L, state, model


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
def test_learn_matches_model(dev, mixer, mode):
    learn, L, state, model = _learner_case(dev, mixer, mode, ["system.hard_update=true", "system.update_period=3"] if mode == "f16x2" else [])
    assert (L.Pm > 0) == (mixer == "qmix") and L.p.numel() == L.Pq + L.Pm
    out = learn(state)
    torch.cuda.synchronize()
    assert L.trained[:2] == [False, False] and all(L.trained[2:]) and sum(L.trained) == 4  # gate: 5 steps per env row
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
            want_m = np.array([r["q_loss"], r["mean_q"], r["mean_target"]])
            g, w = _np(L.debug["grads"][k]).astype(np.float64), r["grad"]
            if mixer == "qmix":
                assert np.abs(w[L.Pq :]).max() > 0  # the mixer is trained
            print(f"step {k}: metrics ratio {_ratio(gm, want_m):.3g} gradient ratio {_ratio(g, w):.3g}")
            assert_close(gm, want_m, 1e-4 if f16 else 1e-5, f"step {k} metrics")
            if f16:  # split-f16 forward and backward products: a handful of small entries move further
                bad = np.abs(g - w) > 1e-3 * (np.abs(w) + np.sqrt(np.mean(w * w)))
                print(f"step {k}: {int(bad.sum())} of {bad.size} gradient entries outside 1e-3 ({int(bad[L.Pq:].sum())} in the mixer)")
                assert bad.sum() <= max(12, 5e-4 * bad.size), f"step {k} gradient: {int(bad.sum())} entries outside 1e-3"
                assert_close(g, w, 1e-2, f"step {k} gradient (hard bound)")
            else:
                assert_close(g, w, 1e-4, f"step {k} gradient")
            k += 1
    for key, b in zip(("obs", "mask", "action", "reward", "terminal", "tot", "next_obs", "next_mask"),
                      (L.buf.obs[0], L.buf.obs[1], L.buf.action, L.buf.reward, L.buf.terminal, L.buf.term_or_trunc,
                       L.buf.next_obs[0], L.buf.next_obs[1])):
        _eq(b, model.replay.f[key], f"buffer {key}")
    _compare_params(_np(L.p), model.online, "online params", f16)
    _compare_params(_np(L.pt), model.target, "target params", f16)


# ---- 5. run_experiment ---------------------------------------------------------------------------------------------------
def _leaves(tree, path=()):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from _leaves(v, path + (k,))
    else:
        yield path, tree


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
def test_run_experiment_logs_every_event_and_restores(dev, tmp_path, monkeypatch, mixer):
    import importlib

    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.utils.checkpointing import Checkpointer

    system = importlib.import_module(f"mava_amd.systems.q_learning.rec_{mixer}")
    monkeypatch.chdir(tmp_path)
    cfg = compose(f"default_rec_{mixer}", ["env/scenario=2s-10x10-3p-3f", "arch.num_envs=16", "system.total_timesteps=512",
                                           "arch.num_evaluation=2", "system.sample_sequence_length=4", "system.min_buffer_size=4",
                                           "system.buffer_size=64", "arch.num_eval_episodes=16",
                                           "arch.num_absolute_metric_eval_episodes=16", "logger.checkpointing.save_model=true"])
    recs = []
    ret = system.run_experiment(cfg, log=recs.append)
    events = [r["event"] for r in recs]
    for ev in ("MISC", "TRAIN", "EVAL", "ABSOLUTE"):
        assert ev in events, events
    misc = [r for r in recs if r["event"] == "MISC"]
    assert [r["timestep"] for r in misc] == [256, 512] and 0.05 <= misc[-1]["epsilon"] <= 1.0
    assert ret == pytest.approx([r for r in recs if r["event"] == "EVAL"][-1]["episode_return"])
    train = [r for r in recs if r["event"] == "TRAIN"]
    assert np.isfinite([[r["q_loss"], r["mean_q"], r["mean_target"]] for r in train]).all()
    # the checkpoint holds online and target, each with the Q network and the mixer
    name = f"rec_{mixer}"
    ck = Checkpointer(model_name=name, checkpoint_uid=os.listdir(os.path.join(tmp_path, "checkpoints", name))[0])
    raw = ck.restore_learner_state_raw()
    assert set(raw["params"]) == {"online", "target"}
    for side in ("online", "target"):
        assert set(raw["params"][side]) == {"q_network", "mixer"}
        assert set(raw["params"][side]["mixer"]) == ({"hyper_w1", "hyper_b1", "hyper_w2", "hyper_b2"} if mixer == "qmix" else set())
    # a fresh learner (other keys) adopts the restored parameters: learn() starts from them (it calls adopt first)
    env, _ = envs.make(cfg, device=dev)
    learn, _, state = system.learner_setup(env, (3, 5), cfg)
    L = learn.learner
    before = L.p.clone()
    restored, _ = ck.restore_params(input_params=state.params)
    L.adopt(state._replace(params=restored))
    assert not torch.equal(L.p, before)
    got = L.learner_state().params
    n = 0
    for side in ("online", "target"):
        want = dict(_leaves(raw["params"][side]))
        have = dict(_leaves(getattr(got, side)))
        assert set(want) == set(have)
        for path, leaf in want.items():
            assert torch.equal(have[path][0, 0].cpu(), leaf), (side, path)
            n += leaf.numel()
    assert n == 2 * L.p.numel()  # every parameter is in the checkpoint, once
    online_q = dict(_leaves(raw["params"]["online"]["q_network"]))
    target_q = dict(_leaves(raw["params"]["target"]["q_network"]))
    assert any(not torch.equal(online_q[p], target_q[p]) for p in online_q)  # tau = 0.01: the target lags
