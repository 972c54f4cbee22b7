"""Cleaner (the `env=cleaner` task) on the GPU: mava_cleaner_step (csrc/cleaner.hip).

An R x C maze, new on every reset, and A agents that start in its top-left corner and clean the dirty cells they step on;
the team earns (cells cleaned) - 0.5 per step and the episode ends when nothing is dirty (won), when an agent walks into
a wall or off the board, or at the time limit.  The complete rules are in DESIGN.md "Cleaner", include/mava_hip.h and,
as the contract, tests/cleaner_model.py; the observation encoding is the one the reference's CleanerWrapper shows -
parity with Jumanji's Cleaner itself is UNPINNED (its source is not part of this project).

The observation is an image: `agents_view` is the flat R C 4 row of `obs_shape = (R, C, 4)` (dirty, wall, agents in the
cell, the viewer's own cell) and carries no one-hot agent id (`implicit_agent_id`); `global_state` is the first three
channels, `state_shape = (R, C, 3)`.  network=mlp / rnn read the flat row, network=cnn / rcnn the image.

Cleaner is the environment that reports a win: `reset` / `step` put `won_episode` (E,) bool into the extras, which the
evaluator forwards and the logger turns into `win_rate` (env.log_win_rate).

The object has the batched MarlEnv surface of Connector: `step_into` writes straight into trajectory slots owned by the
learner, `reset` / `step` allocate.  It declares no fused rollout.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .._lib import ptr
from .base import COMMON_STATE, BatchedEnv, make_pair

MAX_SIDE, MAX_AGENTS = 32, 32  # compile-time maxima of csrc/cleaner.hip
NUM_ACTIONS = 4  # UP, RIGHT, DOWN, LEFT


CleanerState = NamedTuple("CleanerState", COMMON_STATE + [
    ("pos", torch.Tensor),  # (E, A, 2) i32 (row, col)
    ("grid", torch.Tensor),  # (E, R, C) u8: 0 dirty, 1 clean, 2 wall
])


class Cleaner(BatchedEnv):
    State = CleanerState
    action_dim = NUM_ACTIONS
    implicit_agent_id = True
    reports_win = True  # info_won / extras["won_episode"]
    step_symbol = "mava_cleaner_step"  # terminated: won or an invalid action

    def __init__(self, num_envs: int, num_rows: int, num_cols: int, num_agents: int, time_limit: int = 25,
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0, device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        R, C, A = int(num_rows), int(num_cols), int(num_agents)
        if not (3 <= R <= MAX_SIDE and 3 <= C <= MAX_SIDE):
            raise ValueError(f"Cleaner supports 3 <= num_rows, num_cols <= {MAX_SIDE}; got {R} x {C}")
        if not (1 <= A <= MAX_AGENTS):
            raise ValueError(f"Cleaner supports 1 <= num_agents <= {MAX_AGENTS}; got {A}")
        if int(time_limit) < 1:
            raise ValueError(f"time_limit must be >= 1, got {time_limit}")
        super().__init__(kw)
        self.num_rows, self.num_cols = R, C
        self.obs_shape, self.state_shape = (R, C, 4), (R, C, 3)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        return self.num_rows * self.num_cols * 4

    @property
    def state_dim(self) -> int:
        return self.num_rows * self.num_cols * 3

    def alloc_own_state(self) -> tuple:
        E, A, d = self.num_envs, self.num_agents, self.device
        return (torch.zeros((E, A, 2), dtype=torch.int32, device=d),
                torch.zeros((E, self.num_rows, self.num_cols), dtype=torch.uint8, device=d))

    def step_args(self, state: CleanerState):
        return (self.num_rows, self.num_cols, self.time_limit), (ptr(state.pos), ptr(state.grid))


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=cleaner` configuration, sized by config.arch.num_envs / num_eval_episodes.  The
    time limit is the scenario's (env.scenario.env_kwargs.time_limit); env.kwargs.time_limit overrides it."""
    scen = config.env.scenario
    tc = scen.task_config
    time_limit = (config.env.get("kwargs", None) or {}).get("time_limit", None)
    if time_limit is None:
        time_limit = (scen.get("env_kwargs", None) or {}).get("time_limit", 25)
    kw = dict(num_rows=int(tc.num_rows), num_cols=int(tc.num_cols), num_agents=int(tc.num_agents), time_limit=int(time_limit),
              add_global_state=add_global_state, device=device)
    return make_pair(Cleaner, config, kw, env_offset)
