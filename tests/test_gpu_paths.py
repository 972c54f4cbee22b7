"""The learners' run-time execution paths pinned against each other and against the oracle learners.

Each switch below selects another schedule or launch structure for the same arithmetic (or for arithmetic that differs
only in a fixed summation order), so the paths are compared bit for bit where they must agree and at the kernel tests'
figure where they need not:
  MAVA_ROLLOUT_STREAMS  ff, U > 1: replicas 1.. roll out on side streams (learner.py _rollout_fused)
  MAVA_FUSED_TAIL       ff, one rank: slab sums + clip + Adam + count + W1 re-split in two launches (mava_ppo_finish_f32)
  MAVA_REC_OVERLAP      recurrent: the critic's forward / loss / backward on a side stream (rec_learner.py _minibatch)
  MAVA_CRITIC_AGGREGATION, MAVA_TRAIN_VARIANT, MAVA_REC_CRITIC_AGG, MAVA_REC_FUSED_OUT: kernel selections, against the oracle

The side streams are NOT probed here (streams.overlapping_stream is replaced by a plain new stream), so the overlapped path
runs whatever the machine's load, and every test asserts that the path it names really ran.  A missing stream ordering only
gives a wrong result when the other stream happens to be late, so the tests make it late on purpose: the work queued on a
side stream starts with a spin kernel in some minibatches / updates, and the launch stream spins before the Adam launch in
others (a side stream that does not wait for the new parameters then reads the old ones).
"""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close, check_and_sync_f16x2_state

pytestmark = pytest.mark.gpu

SPIN = 10_000_000  # clock cycles of one torch.cuda._sleep (~5 ms): longer than any one step of these small shapes


def _plain_side_streams(monkeypatch):
    from mava_amd import streams

    monkeypatch.setattr(streams, "overlapping_stream", lambda device, tries=8: torch.cuda.Stream(device=device))


class _Delays:
    """Spin kernels that widen the race windows of the side-stream paths.  `adam` counts the Adam launches of the learner
    (one per minibatch); side(c) / main(c) decide from it whether the side-stream work of the current minibatch / update
    starts late, and whether the launch stream holds back Adam launch c."""

    def __init__(self, monkeypatch, dev, side, main):
        from mava_amd import ops

        self.launch = torch.cuda.current_stream(dev)
        self.adam = 0
        self.side_sleeps = 0
        self.side, self.main = side, main
        for name in ("ppo_finish", "clip_adam"):
            monkeypatch.setattr(ops, name, self._before_adam(getattr(ops, name)))

    def _before_adam(self, fn):
        def wrapped(*args, **kwargs):
            if self.main(self.adam):
                torch.cuda._sleep(SPIN)
            self.adam += 1
            return fn(*args, **kwargs)

        return wrapped

    def on_side(self, fn):
        def wrapped(*args, **kwargs):
            if torch.cuda.current_stream() != self.launch and self.side(self.adam):
                torch.cuda._sleep(SPIN)
                self.side_sleeps += 1
            return fn(*args, **kwargs)

        return wrapped


# ---------------------------------------------------------------------------------------------------------- ff_mappo
E_FF, A_FF, O_FF, NA_FF, T_FF, K_FF, M_FF, U_FF, TL_FF = 32, 4, 66, 5, 32, 2, 2, 2, 10  # critic: 264 inputs (wide, re-split W1)


def _run_ff(dev, monkeypatch, env_vars, n_upd=2, U=U_FF):
    """Two updates of ff_mappo (U = 2 by default, fused rollout, f16x2) from fixed parameters with the learner's own epoch
    permutations, each checked against OracleLearner and then synced to its state (so every update starts from the same state in every
    configuration).  Returns the learner and per-update snapshots taken BEFORE the sync."""
    from mava_amd import envs, ops
    from mava_amd._lib import lib
    from mava_amd.systems.ppo import ff_mappo
    from oracle.ppo_loop import OracleLearner
    from tests.test_gpu_learner import _cfg, _check_traj

    monkeypatch.setenv("MAVA_FUSED_ROLLOUT", "1")
    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    for k_, v_ in env_vars.items():
        monkeypatch.setenv(k_, str(v_))
    _plain_side_streams(monkeypatch)
    # side rollouts of update 0 start late (the launch stream must wait for them); the launch stream holds back every Adam
    # launch.  (This test synchronises between updates for the oracle: the parameters the side rollouts of update 1 must
    # wait for are therefore also rewritten on the launch stream behind a spin just before it, below.)
    delays = _Delays(monkeypatch, dev, side=lambda c: c == 0, main=lambda c: True)
    monkeypatch.setattr(ops, "rollout_ff", delays.on_side(ops.rollout_ff))

    E, A, O, nA, T, K, M, TL = E_FF, A_FF, O_FF, NA_FF, T_FF, K_FF, M_FF, TL_FF
    cfg = _cfg("ff_mappo", A, E, T, K, M, U)
    cfg.env.kwargs.time_limit = TL
    cfg.system.num_updates_per_eval = n_upd
    env, _ = envs.make(cfg, add_global_state=True, device=dev)
    learn, _, _ = ff_mappo.learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    rng = np.random.default_rng(4066)
    fa = po.mlp_flatten(po.init_mlp(rng, A + O, nA, 1.0)).astype(np.float32)
    fc = po.mlp_flatten(po.init_mlp(rng, A * O, 1, 1.0)).astype(np.float32)
    L.p[: L.Pa].copy_(torch.from_numpy(fa))
    L.p[L.Pa :].copy_(torch.from_numpy(fc))
    ora = OracleLearner(E=E, A=A, O=O, nA=nA, T=T, K=K, M=M, U=U, D=1, centralised=True, seed=42, time_limit=TL)
    ora.set_params(fa, fc)
    snaps = []
    n_term = 0
    for n in range(n_upd):
        L.update(n)
        torch.cuda.synchronize()
        assert L.fused_rollout and lib().mava_debug_rollout_last_instance() == 805171, "the fused rollout <8,5,17,true> ran"
        snaps.append({
            "traj": [{f: getattr(r, f).clone() for f in ("action", "value", "log_prob", "adv", "tgt", "done")}
                     | {"info_return": r.info_return[n].clone(), "info_length": r.info_length[n].clone(),
                        "info_terminal": r.info_terminal[n].clone()} for r in L.reps],
            "p": L.p.clone(), "m": L.m.clone(), "v": L.v.clone(), "count": L.count.clone(),
            "train_metrics": L.train_metrics[n].clone(),
        })
        perms = [b.cpu().numpy() for b in L._perm_bufs]
        res = ora.update(perms, forced_actions=[[r.action.cpu().numpy() for r in L.reps]])
        _check_traj(L, ora, n, 5e-5)
        n_term += int(sum(r.info_terminal[n].sum().item() for r in L.reps))
        assert_close(L.train_metrics[n].cpu().numpy(), res["train_metrics"], 1e-4, "train metrics", scale=1.0)
        check_and_sync_f16x2_state(L, ora)
        if n + 1 < n_upd:  # parameters still being written on the launch stream when the next update is queued
            held = L.p.clone()
            L.p.zero_()
            torch.cuda._sleep(SPIN)
            L.p.copy_(held)
    assert n_term >= n_upd * U * E * (T // TL - 1), "the time limit must force resets inside the rollout"
    assert L.count.cpu().tolist() == [n_upd * K * M] * 2
    L._delays = delays
    return L, snaps


def test_ff_rollout_streams_and_fused_tail_agree(dev, monkeypatch):
    """{MAVA_FUSED_TAIL, MAVA_ROLLOUT_STREAMS} in {0, 1}^2 from the same state, every run also against the oracle.
    ROLLOUT_STREAMS 0 vs 1 is the same arithmetic on other streams: trajectories, p, m, v, count and train metrics bit for
    bit.  FUSED_TAIL 0 vs 1 with one replica sums the squared norm in another fixed order and nothing else: p, m, v within
    2e-6 (test_fused_tail_equals_separate_launches' figure), the counts equal.  With two replicas the gradient itself is
    summed in another grouping too (the fused tail: one column sum over both replicas' slabs; the separate launches: one
    per replica, the second accumulated onto the first), which moves the small entries of m and v by up to ~5e-6 of their
    rms: 2e-5 there."""
    runs = {}
    n_grad = 2 * U_FF * K_FF * M_FF  # actor launches (= critic launches) of two updates
    for ft in (0, 1):
        for rs in (0, 1):
            with monkeypatch.context() as mp:
                L, snaps = _run_ff(dev, mp, {"MAVA_FUSED_TAIL": ft, "MAVA_ROLLOUT_STREAMS": rs})
            assert L.fused_tail == bool(ft)
            if rs:
                assert len(L._roll_streams) == U_FF - 1, "replica 1 did not roll out on a side stream"
                assert L._delays.side_sleeps == U_FF - 1, "the side-stream rollout of update 0 was not delayed"
            else:
                assert not getattr(L, "_roll_streams", []), "MAVA_ROLLOUT_STREAMS=0 still used side streams"
            assert L.ctx.h2_launches == 2 * n_grad, "every gradient launch on the f16x2 kernels"
            assert L.ctx.get(L.ctx.W8_LAUNCHES) == n_grad, "the actor on the eight-wave kernel, the wide critic on the four-wave one"
            runs[ft, rs] = snaps
        for n, (a, b) in enumerate(zip(runs[ft, 0], runs[ft, 1])):
            for u, (ta, tb) in enumerate(zip(a["traj"], b["traj"])):
                for f in ta:
                    assert torch.equal(ta[f], tb[f]), f"update {n} replica {u}: {f} differs with the side-stream rollouts"
            for f in ("p", "m", "v", "count", "train_metrics"):
                assert torch.equal(a[f], b[f]), f"update {n}: {f} differs with the side-stream rollouts (fused tail {ft})"
    for ft in (0, 1):  # one replica
        with monkeypatch.context() as mp:
            L, runs[ft, "U1"] = _run_ff(dev, mp, {"MAVA_FUSED_TAIL": ft}, U=1)
        assert L.fused_tail == bool(ft)
    for key, rtol in (("U1", 2e-6), (1, 2e-5)):
        for n, (a, b) in enumerate(zip(runs[0, key], runs[1, key])):
            for f in ("p", "m", "v"):
                assert_close(b[f].cpu().numpy(), a[f].cpu().numpy(), rtol, f"update {n} ({key}): {f}, fused against six-launch tail")
            assert torch.equal(a["count"], b["count"])


@pytest.mark.parametrize("env_vars,w8_per_launch", [({"MAVA_CRITIC_AGGREGATION": 0}, 1), ({"MAVA_TRAIN_VARIANT": 1}, 0)],
                         ids=["critic-per-agent", "four-wave-kernels"])
def test_ff_kernel_selection_matches_oracle(dev, monkeypatch, env_vars, w8_per_launch):
    """The critic evaluated once per agent row instead of once per shared input row, and the four-wave gradient kernels
    instead of the eight-wave actor kernel: each against OracleLearner, the selection asserted on the handle."""
    L, _ = _run_ff(dev, monkeypatch, env_vars)
    ctx = L.ctx
    assert ctx.get(ctx.CRITIC_AGGREGATION) == env_vars.get("MAVA_CRITIC_AGGREGATION", 1)
    assert ctx.get(ctx.TRAIN_VARIANT) == env_vars.get("MAVA_TRAIN_VARIANT", 0)
    n_grad = 2 * U_FF * K_FF * M_FF  # actor launches (= critic launches) of two updates
    assert ctx.h2_launches == 2 * n_grad, "every gradient launch on the f16x2 kernels"
    assert ctx.get(ctx.W8_LAUNCHES) == w8_per_launch * n_grad, "eight-wave / four-wave kernel selection"


# --------------------------------------------------------------------------------------------------------- recurrent
def _run_rec(dev, monkeypatch, system, U, E, matmul, overlap, n_upd=2):
    """Two updates of a recurrent learner from fixed parameters and epoch permutations; snapshots of g, p, m, v and the
    train metrics after each."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import rec_ippo, rec_mappo
    from oracle import rec_oracle as ro

    monkeypatch.setenv("MAVA_REC_OVERLAP", str(overlap))
    _plain_side_streams(monkeypatch)
    A, O, nA, T, K, M = 4, 10, 5, 6, 2, 2
    cfg = compose(f"default_{system}", [f"arch.num_envs={E}", f"system.rollout_length={T}", f"system.ppo_epochs={K}",
                                        f"system.num_minibatches={M}", f"system.update_batch_size={U}"])
    cfg.env.scenario.task_config.num_agents = A
    cfg.env.synthetic = {"obs_dim": O, "num_actions": nA}
    cfg.env.kwargs.time_limit = 4
    cfg.system.num_updates_per_eval = n_upd
    cfg.system.actor_lr, cfg.system.critic_lr = 1e-3, 2e-3
    cfg.system.matmul_mode = matmul
    central = system == "rec_mappo"
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _, _ = (rec_mappo if central else rec_ippo).learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    assert L.overlap_critic == bool(overlap), "MAVA_REC_OVERLAP did not select the path"
    # minibatch c's side-stream critic starts late when c % 4 == 1 (Adam launch c must wait for it); Adam launch c is held
    # back when c % 4 == 2 (the critic of minibatch c + 1, not delayed, must wait for it)
    delays = _Delays(monkeypatch, dev, side=lambda c: c % 4 == 1, main=lambda c: c % 4 == 2)
    monkeypatch.setattr(L.critic_network, "forward_sequence", delays.on_side(L.critic_network.forward_sequence))
    rng = np.random.default_rng(2)
    fa = ro.init_rec(rng, A + O, nA, 1.0).astype(np.float32)
    fc = ro.init_rec(rng, A * O if central else A + O, 1, 1.0).astype(np.float32)
    L.p[: L.Pa].copy_(torch.from_numpy(fa))
    L.p[L.Pa :].copy_(torch.from_numpy(fc))
    snaps = []
    for n in range(n_upd):
        perms = [rng.permutation(E).astype(np.int32) for _ in range(K)]
        L.update(n, permutations=[torch.from_numpy(p).to(dev) for p in perms])
        torch.cuda.synchronize()
        snaps.append({f: getattr(L, f).clone() for f in ("g", "p", "m", "v")} | {"train_metrics": L.train_metrics[n].clone()})
    assert delays.adam == n_upd * K * M
    if overlap:
        assert delays.side_sleeps == 2 * U, "the side-stream critic of minibatches 1 and 5 was not delayed"
    return L, snaps


@pytest.mark.parametrize("matmul", ["f32", "f16x2"])
@pytest.mark.parametrize("system,U,E", [("rec_mappo", 1, 64), ("rec_ippo", 2, 16)])
def test_rec_overlap_is_bit_identical(dev, monkeypatch, system, U, E, matmul):
    """MAVA_REC_OVERLAP 0 vs 1: the critic's chain on a side stream with its own workspace and slabs is the same arithmetic -
    g, p, m, v and the train metrics bit for bit after each of two updates."""
    runs = []
    for overlap in (0, 1):
        with monkeypatch.context() as mp:
            L, snaps = _run_rec(dev, mp, system, U, E, matmul, overlap)
        assert L.critic_agg == (system == "rec_mappo")
        runs.append(snaps)
    for n, (a, b) in enumerate(zip(*runs)):
        for f in a:
            assert torch.equal(a[f], b[f]), f"update {n}: {f} differs with the critic on the side stream"


@pytest.mark.parametrize("matmul,env_vars", [("f32", {"MAVA_REC_CRITIC_AGG": 0}), ("f16x2", {"MAVA_REC_CRITIC_AGG": 0}),
                                             ("f16x2", {"MAVA_REC_FUSED_OUT": 0})],
                         ids=["f32-critic-per-agent", "f16x2-critic-per-agent", "f16x2-layerwise-out"])
def test_rec_paths_match_oracle(dev, monkeypatch, matmul, env_vars):
    """rec_mappo at E = 64 (where the critic runs once per env by default) with the critic once per agent row, and in f16x2
    with the layer-wise output path instead of the fused output + loss launch: against OracleRecLearner at the tolerances
    of test_rec_learner_update_matches_oracle, the path asserted on the learner."""
    from tests.test_gpu_rec import _rec_learner_vs_oracle

    for k_, v_ in env_vars.items():
        monkeypatch.setenv(k_, str(v_))
    L = _rec_learner_vs_oracle(dev, "rec_mappo", 1, 64, matmul)
    assert L.critic_agg == ("MAVA_REC_CRITIC_AGG" not in env_vars)
    assert L.fused_out == (matmul == "f16x2" and "MAVA_REC_FUSED_OUT" not in env_vars)
