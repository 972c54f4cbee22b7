"""ff_isac / ff_masac state types (mava/systems/sac/types.py): leaves are torch tensors; parameter trees are views of the
learner's flat buffers (mava_amd/sac_learner.py)."""
from __future__ import annotations

from typing import Any, NamedTuple


class QVals(NamedTuple):
    """types.py:32-34."""

    q1: Any
    q2: Any


class QValsAndTarget(NamedTuple):
    """types.py:37-39."""

    online: QVals
    targets: QVals


class SacParams(NamedTuple):
    """types.py:42-45; log_alpha is (1, A)."""

    actor: Any
    q: QValsAndTarget
    log_alpha: Any


class OptStates(NamedTuple):
    """types.py:48-51: one Adam state per chain."""

    actor: Any
    q: Any
    alpha: Any


class Transition(NamedTuple):
    """One stored item (types.py:54-59): an env's step for all agents.  obs / next_obs are (agents_view, global_state or
    None); next_obs is the pre-reset observation of the step (AutoResetWrapper's extras["real_next_obs"]); done is the
    termination flag (a time-limit end is a truncation)."""

    obs: Any
    action: Any
    reward: Any
    done: Any
    next_obs: Any


class LearnerState(NamedTuple):
    """types.py:65-72."""

    obs: Any
    env_state: Any
    buffer_state: Any
    params: SacParams
    opt_states: OptStates
    t: Any  # the env-step counter the policy-delay test reads
    key: Any
