"""Connector (the `env=connector` task) on the GPU: mava_connector_step (csrc/connector.hip).

A G x G board and A agents that each grow a path from their head to their own target without crossing anything; an
agent scores 1 for the team when it connects and every unconnected agent costs 0.03 per step.  The complete rules are in
DESIGN.md "Connector", include/mava_hip.h and, as the contract, tests/connector_model.py; they follow the published
Connector task and the encoding the reference's ConnectorWrapper shows - parity with Jumanji's MaConnector itself is
UNPINNED (its source is not part of this project).

The observation is an image: `agents_view` is the flat G G 5 row of `obs_shape = (G, G, 5)` and carries no one-hot agent
id (`implicit_agent_id`: the channels encode the agent index relative to the viewer); `global_state` is agent 0's first
three channels, `state_shape = (G, G, 3)`.  network=mlp / rnn read the flat row, network=cnn / rcnn the image.

The object has the batched MarlEnv surface of LevelBasedForaging: `step_into` writes straight into trajectory slots
owned by the learner, `reset` / `step` allocate.  It declares no fused rollout.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .._lib import ptr
from .base import COMMON_STATE, BatchedEnv, make_pair

MAX_GRID, MAX_AGENTS = 16, 32  # compile-time maxima of csrc/connector.hip
NUM_ACTIONS = 5  # NOOP, UP, RIGHT, DOWN, LEFT


ConnectorState = NamedTuple("ConnectorState", COMMON_STATE + [
    ("head", torch.Tensor),  # (E, A, 2) i32 (row, col)
    ("target", torch.Tensor),  # (E, A, 2) i32
    ("connected", torch.Tensor),  # (E, A) u8
    ("grid", torch.Tensor),  # (E, G, G) u8: 0 empty, 1 + 3k path, 2 + 3k head, 3 + 3k target of agent k
])


class Connector(BatchedEnv):
    State = ConnectorState
    action_dim = NUM_ACTIONS
    implicit_agent_id = True  # the channels encode the agent index relative to the viewer
    step_symbol = "mava_connector_step"  # terminated: no agent has a legal move

    def __init__(self, num_envs: int, grid_size: int, num_agents: int, time_limit: int = 50, add_global_state: bool = False,
                 seed: int = 42, env_offset: int = 0, device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        G, A = int(grid_size), int(num_agents)
        if not (3 <= G <= MAX_GRID):
            raise ValueError(f"Connector supports 3 <= grid_size <= {MAX_GRID}; got {G}")
        if not (1 <= A <= MAX_AGENTS):
            raise ValueError(f"Connector supports 1 <= num_agents <= {MAX_AGENTS}; got {A}")
        if 2 * A > G * G - 2:
            raise ValueError(f"Connector needs 2 * num_agents <= grid_size^2 - 2 (a head and a target per agent); got "
                             f"num_agents={A}, grid_size={G}")
        if int(time_limit) < 1:
            raise ValueError(f"time_limit must be >= 1, got {time_limit}")
        super().__init__(kw)
        self.grid_size = G
        self.obs_shape, self.state_shape = (G, G, 5), (G, G, 3)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        return self.grid_size * self.grid_size * 5

    @property
    def state_dim(self) -> int:
        return self.grid_size * self.grid_size * 3

    def alloc_own_state(self) -> tuple:
        E, A, G, d = self.num_envs, self.num_agents, self.grid_size, self.device
        i32, u8 = torch.int32, torch.uint8
        return (torch.zeros((E, A, 2), dtype=i32, device=d), torch.zeros((E, A, 2), dtype=i32, device=d),
                torch.zeros((E, A), dtype=u8, device=d), torch.zeros((E, G, G), dtype=u8, device=d))

    def step_args(self, state: ConnectorState):
        return ((self.grid_size, self.time_limit),
                (ptr(state.head), ptr(state.target), ptr(state.connected), ptr(state.grid)))


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=connector` configuration, sized by config.arch.num_envs / num_eval_episodes.  The
    time limit is the scenario's (env.scenario.env_kwargs.time_limit); env.kwargs.time_limit overrides it."""
    scen = config.env.scenario
    tc = scen.task_config
    time_limit = (config.env.get("kwargs", None) or {}).get("time_limit", None)
    if time_limit is None:
        time_limit = (scen.get("env_kwargs", None) or {}).get("time_limit", 50)
    kw = dict(grid_size=int(tc.grid_size), num_agents=int(tc.num_agents), time_limit=int(time_limit),
              add_global_state=add_global_state, device=device)
    return make_pair(Connector, config, kw, env_offset)
