"""Plumbing every learner repeats outside its update path: the arithmetic-mode context, the episode-metric views, the
`learn` closure of learner_setup, and the 32-row padding of the kernels' tiles."""
from __future__ import annotations

import os
from typing import Any, Callable, Dict, Tuple

import torch

from . import ops


def pad32(n: int) -> int:
    """`n` rounded up to the kernels' 32-row tiles."""
    return -(-n // 32) * 32


def matmul_ctx(system_cfg, **ctx_kwargs) -> Tuple[str, ops.Ctx]:
    """Arithmetic of the matrix products (not a Mava key): system.matmul_mode, else the environment variable below, else
    "f16x2" (every operand split into two f16 terms); "f32" runs the exact-f32 kernels everywhere.  Returns the mode and
    this learner's context handle (include/mava_hip.h mava_ctx_*): the library keeps no process-wide mode."""
    mode = str(system_cfg.get("matmul_mode", None) or os.environ.get("MAVA_MATMUL", "f16x2"))
    if mode not in ("f16x2", "f32"):
        raise ValueError(f"system.matmul_mode must be 'f16x2' or 'f32', got {mode!r}")
    return mode, ops.Ctx(mode, **ctx_kwargs)


def episode_metrics(info_return: torch.Tensor, info_length: torch.Tensor, info_terminal: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The (n_upd, T, E) episode-metric buffers of a single-replica learner as (1, n_upd, 1, T, E) views."""
    return {"episode_return": info_return.unsqueeze(1).unsqueeze(0),
            "episode_length": info_length.unsqueeze(1).unsqueeze(0),
            "is_terminal_step": info_terminal.unsqueeze(1).unsqueeze(0).bool()}


def bind_learn(learner) -> Callable[[Any], Any]:
    """The LearnerFn of learner_setup: `learn(state)` runs learner.learn; `learn.learner` is the handle tests and
    benchmarks reach the learner through."""
    def learn(learner_state):
        return learner.learn(learner_state)

    learn.learner = learner  # type: ignore[attr-defined]
    return learn
