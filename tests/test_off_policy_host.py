"""CPU: the host arithmetic of the replay-buffer systems' experiment loop (mava_amd/systems/off_policy.py::eval_schedule)
on the literals the GPU run_experiment tests pin, and the tree helpers (mava_amd/utils/tree.py) on a nested structure."""
from typing import NamedTuple

import torch

from mava_amd.systems.off_policy import eval_schedule
from mava_amd.utils.tree import tree_clone, tree_to, unreplicate_n_dims


def test_eval_schedule():
    # rec_iql, tests/test_gpu_iql.py::test_run_experiment_logs_every_event: MISC at [256, 512], 8 updates of 16 x 2 steps
    assert eval_schedule(512, 2, 16, 2) == (256, 8, [256, 512])
    # ff_isac / ff_masac, tests/test_gpu_sac_learning.py::test_run_experiment: t = explore_steps + k * steps_per_rollout
    steps, n_upd, ts = eval_schedule(256, 2, 16, 2, explore_steps=400)
    assert (steps, n_upd) == (128, 4) and ts == [400 + 128 * k for k in (1, 2)] == [528, 656]
    # an interval shorter than one update's act steps still runs one update
    assert eval_schedule(100, 4, 16, 2) == (25, 1, [25, 50, 75, 100])
    # integer division throughout: what int(a / b) gives for operands below 2^53
    assert eval_schedule(1000, 3, 7, 5) == (333, int(333 / 35), [333, 666, 999])


class _Pair(NamedTuple):
    a: object
    b: object


class _Tree(dict):  # a dict subclass, like MATParams
    pass


def _nested():
    return {"pair": _Pair(torch.arange(24.0).view(2, 3, 4), [torch.ones(1, 1, 5), torch.zeros(3)]),
            "sub": _Tree(w=torch.full((1, 1, 2), 7.0), scalar=torch.tensor(3.0)), "name": "leaf", "n": 4}


def test_tree_helpers():
    tree = _nested()
    # tree_to: every tensor leaf converted, containers kept (a dict subclass comes back as a plain dict), other leaves as is
    moved = tree_to(tree, torch.device("meta"))
    assert isinstance(moved["pair"], _Pair) and isinstance(moved["pair"].b, list) and type(moved["sub"]) is dict
    leaves = [moved["pair"].a, *moved["pair"].b, moved["sub"]["w"], moved["sub"]["scalar"]]
    assert all(t.device.type == "meta" for t in leaves) and moved["pair"].a.shape == (2, 3, 4)
    assert moved["name"] == "leaf" and moved["n"] == 4
    same = tree_to(tree, torch.device("cpu"))
    assert torch.equal(same["pair"].a, tree["pair"].a) and torch.equal(same["sub"]["w"], tree["sub"]["w"])

    # unreplicate_n_dims: x[0, 0] on leaves with at least n dims, leaves with fewer left alone
    un = unreplicate_n_dims(tree)
    assert isinstance(un["pair"], _Pair) and torch.equal(un["pair"].a, tree["pair"].a[0, 0]) and un["pair"].b[0].shape == (5,)
    assert un["pair"].b[1] is tree["pair"].b[1] and un["sub"]["scalar"] is tree["sub"]["scalar"]  # 1 and 0 dims < 2
    assert torch.equal(un["sub"]["w"], torch.full((2,), 7.0)) and un["name"] == "leaf" and un["n"] == 4
    un1 = unreplicate_n_dims(tree, 1)  # n is the number of leading dims dropped: here only the 0-dim leaf stays
    assert un1["pair"].a.shape == (3, 4) and un1["pair"].b[1].shape == () and un1["sub"]["scalar"] is tree["sub"]["scalar"]

    # tree_clone: equal values, no shared storage anywhere - through the NamedTuple and the list too
    clone = tree_clone(tree)
    pairs = [(clone["pair"].a, tree["pair"].a), (clone["pair"].b[0], tree["pair"].b[0]), (clone["pair"].b[1], tree["pair"].b[1]),
             (clone["sub"]["w"], tree["sub"]["w"]), (clone["sub"]["scalar"], tree["sub"]["scalar"])]
    for c, t in pairs:
        assert torch.equal(c, t) and c.data_ptr() != t.data_ptr()
    for c, t in pairs:
        t.add_(1.0)
        assert not torch.equal(c, t)
    assert isinstance(clone["pair"], _Pair) and clone["name"] == "leaf"
