"""rec_iql state types (mava/systems/q_learning/types.py): leaves are torch tensors; parameter trees are views of the
learner's flat buffers (mava_amd/iql_learner.py)."""
from __future__ import annotations

from typing import Any, NamedTuple


class Transition(NamedTuple):
    """One stored step (types.py:29-38): the flags are those of the step that produced `obs`; next_obs is the pre-reset
    observation of the step (AutoResetWrapper's extras["real_next_obs"])."""

    obs: Any
    action: Any
    reward: Any
    terminal: Any
    term_or_trunc: Any
    next_obs: Any


class QNetParams(NamedTuple):
    """Double Q-learning network parameters (types.py:44-48)."""

    online: Any
    target: Any


class LearnerState(NamedTuple):
    """types.py:51-68: interaction, train and shared variables of the act-train loop."""

    obs: Any
    terminal: Any
    term_or_trunc: Any
    hidden_state: Any
    env_state: Any
    time_steps: Any
    train_steps: Any
    opt_state: Any
    buffer_state: Any
    params: QNetParams
    key: Any
