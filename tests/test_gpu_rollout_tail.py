"""The one-launch rollout's tail (csrc/rollout_h2.hip): GAE by the whole workgroup from LDS, last_reward / last_done and
the device step counter written by the launch itself (mava_rollout_ff_f32's optional tail outputs), and the slot T ->
slot 0 carry launch (mava_rollout_carry)."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

E, TL, O, NA = 24, 5, 66, 5  # two workgroups at 4 agents, the second half full; every env resets every 5 steps


def _learner(dev, system, T, fused, monkeypatch):
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_ippo, ff_mappo

    monkeypatch.setenv("MAVA_FUSED_ROLLOUT", "1" if fused else "0")
    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    cfg = compose(f"default_{system}", [f"arch.num_envs={E}", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                        "system.num_minibatches=2", "system.update_batch_size=1"])
    cfg.env.scenario.task_config.num_agents = 4  # tiny-4ag
    cfg.env.kwargs.time_limit = TL
    central = system == "ff_mappo"
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _, _ = (ff_mappo if central else ff_ippo).learner_setup(env, (42, 7, 8), cfg, device=dev)
    L = learn.learner
    rng = np.random.default_rng(11)
    L.p[: L.Pa].copy_(torch.from_numpy(po.mlp_flatten(po.init_mlp(rng, 4 + O, NA, 1.0)).astype(np.float32)))
    L.p[L.Pa :].copy_(torch.from_numpy(po.mlp_flatten(po.init_mlp(rng, 4 * O if central else 4 + O, 1, 1.0)).astype(np.float32)))
    return L


# T = 3, 13: shorter than / not a multiple of the eight entries a thread loads per pass; 8: exactly one; 128: the
# benchmarked length; ff_ippo at 300: longer than the LDS of <8,5,5,false> holds (160 steps): two chunks, 140 + 160.
@pytest.mark.parametrize("system,inst,T", [("ff_mappo", 805171, 3), ("ff_mappo", 805171, 8), ("ff_mappo", 805171, 13),
                                           ("ff_mappo", 805171, 128), ("ff_ippo", 805050, 13), ("ff_ippo", 805050, 300)])
def test_rollout_tail_outputs(dev, system, inst, T, monkeypatch):
    from mava_amd import ops
    from mava_amd._lib import lib

    L = _learner(dev, system, T, True, monkeypatch)
    L._rollout(0)
    torch.cuda.synchronize()
    assert L.fused_rollout and lib().mava_debug_rollout_last_instance() == inst
    r = L.reps[0]
    adv, tgt = ops.gae(r.reward, r.value, r.done, r.last_val, float(L.config.system.gamma), float(L.config.system.gae_lambda))
    assert_close(r.adv.cpu().numpy(), adv.cpu().numpy(), 1e-5, "advantages")
    assert_close(r.tgt.cpu().numpy(), tgt.cpu().numpy(), 1e-5, "targets")
    a64, t64 = po.gae(r.reward.cpu().numpy(), r.value.cpu().numpy(), r.done.cpu().numpy().astype(bool),
                      r.last_val.cpu().numpy(), float(L.config.system.gamma), float(L.config.system.gae_lambda))
    assert_close(r.adv.cpu().numpy(), a64, 1e-5, "advantages against float64")
    assert_close(r.tgt.cpu().numpy(), t64, 1e-5, "targets against float64")
    assert torch.equal(r.last_reward, r.reward[T - 1]) and torch.equal(r.last_done, r.done[T - 1])
    assert int(r.done.sum().item()) >= (T // TL) * E * 4, "the time limit must force resets inside the rollout"
    assert int(L.step_dev.item()) == T and L.t_global == T
    fused = {k: getattr(r, k).clone() for k in ("agents_view", "global_state", "action_mask", "step_count", "reward", "done")}
    fused |= {"ret": r.info_return[0].clone(), "len": r.info_length[0].clone(), "term": r.info_terminal[0].clone()}

    S = _learner(dev, system, T, False, monkeypatch)
    S._rollout(0)
    torch.cuda.synchronize()
    assert not S.fused_rollout and int(S.step_dev.item()) == T
    s = S.reps[0]
    step = {k: getattr(s, k) for k in ("agents_view", "global_state", "action_mask", "step_count", "reward", "done")}
    step |= {"ret": s.info_return[0], "len": s.info_length[0], "term": s.info_terminal[0]}
    for k, v in fused.items():
        if k == "global_state" and system != "ff_mappo":
            continue  # (the decentralised critic does not read it and the one-launch rollout does not write it)
        assert torch.equal(v, step[k]), k
    assert torch.equal(r.last_reward, s.last_reward) and torch.equal(r.last_done, s.last_done)

    # a second rollout counts on from the counter the first one left
    L._rollout(0)
    torch.cuda.synchronize()
    assert int(L.step_dev.item()) == 2 * T


@pytest.mark.parametrize("with_gs", [True, False])
@pytest.mark.parametrize("E_,A,W,offset", [(3, 3, 7, 0),    # 63 floats / 45 mask bytes per slot: 4-byte and single-byte pieces
                                           (5, 4, 70, 0),   # 16-byte pieces with a 4-byte rest in the mask (100 bytes)
                                           (37, 2, 10, 1),  # every base one element off its allocation
                                           (300, 4, 70, 0)])  # more than one block
def test_rollout_carry(dev, with_gs, E_, A, W, offset):
    from mava_amd import ops

    T, nA, G = 6, 5, 11
    g = torch.Generator(device="cpu").manual_seed(E_ * 7 + A)

    def arr(shape, dtype):
        n = int(np.prod(shape))
        flat = torch.empty(n + offset, dtype=dtype, device=dev)
        if dtype == torch.float32:
            flat.copy_(torch.rand(n + offset, generator=g))
        else:
            flat.copy_(torch.randint(0, 120, (n + offset,), generator=g).to(dtype))
        return flat[offset:].view(shape)

    av, gs = arr((T + 1, E_, A, W), torch.float32), arr((T + 1, E_, 1, G), torch.float32)
    mask, sc = arr((T + 1, E_, A, nA), torch.uint8), arr((T + 1, E_, A), torch.int32)
    before = [x.clone() for x in (av, gs, mask, sc)]
    ops.rollout_carry(av, gs if with_gs else None, mask, sc)
    torch.cuda.synchronize()
    for name, x, b in zip(("agents_view", "global_state", "action_mask", "step_count"), (av, gs, mask, sc), before):
        assert torch.equal(x[1:], b[1:]), f"{name}: slots 1..T changed"
        if name == "global_state" and not with_gs:
            assert torch.equal(x[0], b[0]), "global_state: not given, must stay"
        else:
            assert torch.equal(x[0], b[T]), f"{name}: slot 0 is not slot T"
