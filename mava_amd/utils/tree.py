"""Helpers over the nested containers the learner states are made of: dicts (and dict subclasses), NamedTuples, lists
and tuples, with tensors and plain Python values as leaves."""
from __future__ import annotations

import copy
from typing import Any

import torch


def unreplicate_n_dims(tree: Any, n: int = 2) -> Any:
    """mava/utils/jax_utils.py:52-59: x[0, 0] on every array leaf with at least n leading dims."""
    if isinstance(tree, torch.Tensor):
        return tree[(0,) * n] if tree.dim() >= n else tree
    if hasattr(tree, "_asdict"):
        return type(tree)(**{k: unreplicate_n_dims(v, n) for k, v in tree._asdict().items()})
    if isinstance(tree, dict):
        return {k: unreplicate_n_dims(v, n) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(unreplicate_n_dims(v, n) for v in tree)
    return tree


def tree_to(tree: Any, device) -> Any:
    """Every tensor leaf moved to `device`; a dict subclass comes back as a plain dict."""
    if isinstance(tree, torch.Tensor):
        return tree.to(device)
    if hasattr(tree, "_asdict"):
        return type(tree)(**{k: tree_to(v, device) for k, v in tree._asdict().items()})
    if isinstance(tree, dict):
        return {k: tree_to(v, device) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(tree_to(v, device) for v in tree)
    return tree


def tree_clone(tree: Any) -> Any:
    """A copy that shares no tensor storage with `tree`."""
    if isinstance(tree, torch.Tensor):
        return tree.clone()
    if isinstance(tree, dict):
        return {k: tree_clone(v) for k, v in tree.items()}
    return copy.deepcopy(tree)
