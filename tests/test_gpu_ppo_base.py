"""The contract the three on-policy learners share through PPOLearner (mava_amd/ppo_learner.py): the shapes and dtypes
learn() returns, adoption of the learner's own state (a no-op) and of a foreign one, and MAT's refusals."""
import types

import pytest
import torch

from mava_amd._lib import MavaHipError
from mava_amd.utils.tree import tree_to

pytestmark = pytest.mark.gpu

KINDS = ("ff_mappo", "rec_mappo", "ff_mat")
N_UPD = 2


def _make(kind, dev, keys):
    """(learn, learner, initial state) of one system at its smallest shape."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import ff_mappo, ff_mat, rec_mappo

    if kind == "ff_mappo":
        over, mod, central = ["arch.num_envs=8", "system.update_batch_size=2", "system.num_minibatches=2"], ff_mappo, True
    elif kind == "rec_mappo":  # the smallest shape with E * A and (E / M) * A multiples of 32
        over, mod, central = ["arch.num_envs=32", "system.update_batch_size=1", "system.num_minibatches=1"], rec_mappo, True
    else:
        over, mod, central = ["arch.num_envs=8", "system.num_minibatches=2", "network.n_embd=32"], ff_mat, False
    cfg = compose(f"default_{kind}", ["env/scenario=tiny-2ag", "system.rollout_length=4", "system.ppo_epochs=1"] + over)
    cfg.system.num_updates_per_eval = N_UPD
    if kind == "ff_mappo":
        cfg.env.synthetic = {"obs_dim": 10, "num_actions": 5}
    env, _ = envs.make(cfg, add_global_state=central, device=dev)
    learn, _actor, state = mod.learner_setup(env, keys, cfg, device=dev)
    return learn, learn.learner, state


def _first_segment(L, state):
    """(network, parameter tree, AdamState) of the segment the flat buffers start with."""
    if hasattr(state.params, "critic_params"):
        return L.actor_network, state.params.actor_params, state.opt_states.actor_opt_state
    return L.net, state.params, state.opt_states


def _flat(L):
    return [t.clone() for t in (L.p, L.m, L.v, L.count)]


@pytest.fixture(scope="module", params=KINDS)
def case(request, dev):
    """One learner per system after two learn() calls, the second on the state the first returned; what the tests read
    are the outputs and clones taken in between, which nothing changes afterwards."""
    kind = request.param
    learn, L, state = _make(kind, dev, (7, 11, 13))
    out1 = learn(state)
    torch.cuda.synchronize()
    c = types.SimpleNamespace(kind=kind, L=L, out1=out1, flat1=_flat(L))
    c.shapes1 = {g: {k: (tuple(v.shape), v.dtype) for k, v in getattr(out1, g).items()} for g in ("episode_metrics", "train_metrics")}
    net, params, opt = _first_segment(L, out1.learner_state)
    c.aliases = (net.first_leaf(params).data_ptr() == L.p.data_ptr(), net.first_leaf(opt.mu).data_ptr() == L.m.data_ptr(),
                 net.first_leaf(opt.nu).data_ptr() == L.v.data_ptr())
    c.foreign = out1.learner_state._replace(params=tree_to(out1.learner_state.params, "cpu"),
                                            opt_states=tree_to(out1.learner_state.opt_states, "cpu"))
    learn(out1.learner_state)
    torch.cuda.synchronize()
    c.flat2 = _flat(L)
    return c


def test_learn_output_shapes_and_dtypes(case):
    L = case.L
    U = 2 if case.kind == "ff_mappo" else 1
    assert (L.U, L.T, L.K, L.A) == (U, 4, 1, 2) and (L.E, L.M) == {"ff_mappo": (8, 2), "rec_mappo": (32, 1), "ff_mat": (8, 2)}[case.kind]
    ep, tm = case.shapes1["episode_metrics"], case.shapes1["train_metrics"]
    assert ep == {"episode_return": ((1, N_UPD, U, L.T, L.E), torch.float32), "episode_length": ((1, N_UPD, U, L.T, L.E), torch.int32),
                  "is_terminal_step": ((1, N_UPD, U, L.T, L.E), torch.bool)}
    assert tm == {k: ((1, N_UPD, U, L.K, L.M), torch.float32) for k in ("total_loss", "value_loss", "actor_loss", "entropy")}
    assert all(bool(torch.isfinite(v).all()) for v in case.out1.train_metrics.values())


def test_own_state_is_adopted_as_a_no_op(case, dev):
    """The returned state's parameter and moment leaves are views of p / m / v, so learn() on it copies nothing: it leaves
    the buffers where the same number of update() calls leaves a twin built with the same keys."""
    assert case.aliases == (True, True, True)
    _, twin, _ = _make(case.kind, dev, (7, 11, 13))
    for _ in range(2):
        for n in range(N_UPD):
            twin.update(n)
    torch.cuda.synchronize()
    assert not torch.equal(case.flat1[0], case.flat2[0])  # (the second call did train)
    for name, a, b in zip("p m v count".split(), case.flat2, _flat(twin)):
        assert torch.equal(a, b), name


def test_foreign_state_is_adopted(case, dev):
    """Host copies of the trees (a restored checkpoint) land bit for bit in the buffers of a learner built from other
    seeds that has trained already; FFLearner also drops the W1 split its context handle cached for the old parameters."""
    _, other, _ = _make(case.kind, dev, (8, 9, 10))
    other.update(0)
    assert not torch.equal(other.p, case.flat1[0]) and int(other.count[0]) != int(case.flat1[3][0])
    other.adopt(case.foreign)
    torch.cuda.synchronize()
    for name, a, b in zip("p m v count".split(), case.flat1, _flat(other)):
        assert torch.equal(a, b), name
    if case.kind == "ff_mappo":
        assert other.ctx.get(other.ctx.W1_SPLIT_FRESH) == 0


@pytest.mark.parametrize("bad,text", [("update_batch_size", "system.update_batch_size must be 1, got 2"),
                                      ("continuous", "a continuous action head is not implemented")])
def test_mat_refuses_before_anything_is_allocated(dev, bad, text):
    from mava_amd.config import compose
    from mava_amd.mat_learner import MATLearner

    cfg = compose("default_ff_mat", ["env/scenario=tiny-2ag", "arch.num_envs=8", "system.rollout_length=4", "network.n_embd=32"]
                  + (["system.update_batch_size=2"] if bad == "update_batch_size" else []))
    if bad == "continuous":
        cfg.network.action_head = {"_target_": "mava.networks.ContinuousActionHead"}
    # an environment that has nothing but what the refusals read: cloning it or allocating its state would fail otherwise
    env = types.SimpleNamespace(num_envs=8, num_agents=2, action_dim=5)
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(MavaHipError, match=text):
        MATLearner(env, cfg, dev)
    assert torch.cuda.memory_allocated(dev) == before
    assert "num_agents" not in cfg.system  # (the prologue had not started)
