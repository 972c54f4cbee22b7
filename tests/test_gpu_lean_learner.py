"""FFLearner with MAVA_ROLLOUT_LEAN=1 (the fused rollout leaves slots 1 .. T - 1 of the f32 agents_view / global_state unwritten
where every gradient launch reads the f16 record instead) against =0, two updates from the same state: parameters, both Adam
moments and the train metrics bit for bit, the observations a host read of the replica returns included - and the two ways a
stale f32 slot could be read: a slot-0 value with a low f16 term (the device words end 0) and a handle setting that sends the
gradient launches back to the f32 input.  Runs are compared with each other: no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

A, E, T, K, M = 4, 32, 8, 2, 2


def _run(dev, monkeypatch, system, U, lean, *, plant=False, variant_env=None, flip=False, updates=2):
    from mava_amd import envs
    from mava_amd._lib import Ctx
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_ippo, ff_mappo

    monkeypatch.setenv("MAVA_ROLLOUT_LEAN", lean)
    monkeypatch.setenv("MAVA_X16", "1")
    monkeypatch.setenv("MAVA_FUSED_ROLLOUT", "1")
    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    if variant_env is None:
        monkeypatch.delenv("MAVA_TRAIN_VARIANT", raising=False)
    else:
        monkeypatch.setenv("MAVA_TRAIN_VARIANT", variant_env)
    mod = ff_mappo if system == "ff_mappo" else ff_ippo
    cfg = compose(f"default_{system}", [f"arch.num_envs={E}", f"system.rollout_length={T}", f"system.ppo_epochs={K}",
                                        f"system.num_minibatches={M}", f"system.update_batch_size={U}"])
    cfg.env.scenario.task_config.num_agents = A
    cfg.system.num_updates_per_eval = 1
    cfg.env.kwargs.time_limit = 5
    env, _ = envs.make(cfg, add_global_state=system == "ff_mappo", device=dev)
    learn, _, _ = mod.learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    assert L.fused_rollout and L.view16 and L.lean == (lean == "1") and L.x16 == (system == "ff_mappo")
    if plant:  # a slot-0 value that is not exact in f16, in both arrays of the last replica
        L.reps[-1].av_raw[0, 17, 2, 9] = 0.1
        if L.centralised:
            L.reps[-1].gs_raw[0, 17, 0, 75] = 0.1
    if flip:  # the handle changes between the rollout and the first epoch of the FIRST update
        inner = L._rollout

        def rollout_then_flip(n):
            inner(n)
            if L.ctx.get(Ctx.TRAIN_VARIANT) == 0:
                L.ctx.set(Ctx.TRAIN_VARIANT, 1)

        L._rollout = rollout_then_flip
    skipped = []
    for n in range(updates):
        L.update(0)
        skipped.append([(r.stale_av, r.stale_gs) for r in L.reps])
    torch.cuda.synchronize()
    assert L.fused_rollout, "the fused rollout served the updates"
    out = {"p": L.p.clone(), "m": L.m.clone(), "v": L.v.clone(), "train_metrics": L.train_metrics.clone()}
    counts = {"x16": L.ctx.get(Ctx.X16_LAUNCHES), "x16_w8": L.ctx.get(Ctx.X16_W8_LAUNCHES)}
    words = [(int(r.view16_valid.item()), int(r.state16_valid.item()) if L.x16 else None) for r in L.reps]
    # a host read of the replica's observations (what the existing tests do): the recorded ones, skipped or not
    for u, r in enumerate(L.reps):
        out[f"agents_view{u}"] = r.agents_view[1:T].clone()
        out[f"global_state{u}"] = r.global_state[1:T].clone() if L.centralised else None
        assert not r.stale_av and not r.stale_gs, "a read through the property leaves nothing stale"
    return out, counts, skipped, words


def _same(off, on, what):
    for k in off:
        if off[k] is None:
            continue
        assert torch.equal(off[k], on[k]), f"{what}: {k} differs between MAVA_ROLLOUT_LEAN=0 and =1"


@pytest.mark.parametrize("system,U", [("ff_mappo", 1), ("ff_mappo", 2), ("ff_ippo", 1)])
def test_lean_updates_have_the_same_bits(dev, monkeypatch, system, U):
    off, _, sk_off, _ = _run(dev, monkeypatch, system, U, "0")
    on, counts, sk_on, words = _run(dev, monkeypatch, system, U, "1")
    assert not any(a or g for upd in sk_off for a, g in upd), "MAVA_ROLLOUT_LEAN=0 skipped something"
    central = system == "ff_mappo"
    assert all((a, g) == (True, central) for upd in sk_on for a, g in upd), f"=1 did not skip what it can: {sk_on}"
    assert all(w == (1, 1 if central else None) for w in words)
    # every gradient launch of the =1 run read a record: 2 updates x K x M minibatches x U replicas, the actor on the eight-wave
    # kernel, the critic on the wide kernel (ff_mappo) or the eight-wave one (ff_ippo)
    n = 2 * K * M * U
    assert (counts["x16_w8"], counts["x16"]) == ((n, n) if central else (2 * n, 0)), counts
    _same(off, on, f"{system} U={U}")


def test_low_term_in_slot0_reads_the_repaired_f32_trajectory(dev, monkeypatch):
    """0.1 in slot 0: the words of that replica end 0 in the first update, its gradient launches read the f32 arrays - which the
    conditional expand behind the rollout must have completed.  (The second update starts from the environment's own slot 0.)"""
    off, _, _, _ = _run(dev, monkeypatch, "ff_mappo", 2, "0", plant=True)
    on, counts, skipped, _ = _run(dev, monkeypatch, "ff_mappo", 2, "1", plant=True)
    assert all((a, g) == (True, True) for upd in skipped for a, g in upd)
    n = 2 * K * M * 2
    assert counts["x16_w8"] == n - K * M and counts["x16"] == n - K * M, f"the planted replica's first update read a record: {counts}"
    _same(off, on, "planted 0.1")


@pytest.mark.parametrize("how", ["env", "flip"])
def test_train_variant_sends_the_actor_back_to_f32(dev, monkeypatch, how):
    """MAVA_CTX_TRAIN_VARIANT = 1 (four-wave kernels only: the actor's launches read the f32 agents_view; the wide critic still
    reads its record) set from the start, and set on the handle between the rollout and the first epoch: the learner asks the
    library again before a gradient launch and rebuilds agents_view first."""
    kw = {"variant_env": "1"} if how == "env" else {"flip": True}
    off, _, _, _ = _run(dev, monkeypatch, "ff_mappo", 1, "0", **kw)
    on, counts, skipped, _ = _run(dev, monkeypatch, "ff_mappo", 1, "1", **kw)
    # flip: the first rollout skipped agents_view and the guard rebuilt it (nothing stale by the update's end); from then on, and
    # with the variable set from the start, the answer at rollout time is already "no"
    assert all((a, g) == (False, True) for upd in skipped for a, g in upd), skipped
    assert counts["x16_w8"] == 0 and counts["x16"] == 2 * K * M, counts
    _same(off, on, f"TRAIN_VARIANT ({how})")
