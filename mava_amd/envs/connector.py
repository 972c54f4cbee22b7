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

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from .._lib import launch, lib, ptr, stream_ptr
from ..types import Observation, ObservationGlobalState, TimeStep
from .synthetic_rware import EVAL_KEY_TAG, ObsSpec

MAX_GRID, MAX_AGENTS = 16, 32  # compile-time maxima of csrc/connector.hip
NUM_ACTIONS = 5  # NOOP, UP, RIGHT, DOWN, LEFT


class ConnectorState(NamedTuple):
    # the five fields the learners read, with SynthState's names and meaning
    step_count: torch.Tensor  # (E, A) i32
    run_return: torch.Tensor  # (E,) f32
    run_length: torch.Tensor  # (E,) i32
    ep_return: torch.Tensor  # (E,) f32
    ep_length: torch.Tensor  # (E,) i32
    t: torch.Tensor  # () i64 host-side step counter of the allocating API
    head: torch.Tensor  # (E, A, 2) i32 (row, col)
    target: torch.Tensor  # (E, A, 2) i32
    connected: torch.Tensor  # (E, A) u8
    grid: torch.Tensor  # (E, G, G) u8: 0 empty, 1 + 3k path, 2 + 3k head, 3 + 3k target of agent k


class Connector:
    action_dim = NUM_ACTIONS
    gs_tiles = 1
    global_state_shared = True
    supports_fused_rollout = False
    emits_real_next_obs = True  # step_into(real_obs=, terminated=): what rec_iql stores as next_obs / terminal
    implicit_agent_id = True  # no one-hot id in agents_view; system.add_agent_id is ignored, as the reference's make_env does

    def __init__(self, num_envs: int, grid_size: int, num_agents: int, time_limit: int = 50, add_global_state: bool = False,
                 seed: int = 42, env_offset: int = 0, device: Optional[torch.device] = None):
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
        self.num_envs, self.num_agents, self.grid_size, self.time_limit = int(num_envs), A, G, int(time_limit)
        self.add_global_state = add_global_state
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.obs_shape: Tuple[int, int, int] = (G, G, 5)
        self.state_shape: Tuple[int, int, int] = (G, G, 3)

    def clone(self, env_offset: int, num_envs: Optional[int] = None) -> "Connector":
        """Same scenario on a disjoint range of global env ids (one per replica / rank)."""
        return Connector(num_envs or self.num_envs, self.grid_size, self.num_agents, self.time_limit, self.add_global_state,
                         self.seed, env_offset, self.device)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        return self.grid_size * self.grid_size * 5

    @property
    def state_dim(self) -> int:
        return self.grid_size * self.grid_size * 3

    def observation_spec(self) -> ObsSpec:
        A = self.num_agents
        return ObsSpec((A, self.obs_dim), (A, self.action_dim), (A, self.state_dim) if self.add_global_state else None, (A,))

    def alloc_state(self) -> ConnectorState:
        E, A, G, d = self.num_envs, self.num_agents, self.grid_size, self.device
        i32, u8 = torch.int32, torch.uint8
        return ConnectorState(torch.zeros((E, A), dtype=i32, device=d), torch.zeros(E, device=d),
                              torch.zeros(E, dtype=i32, device=d), torch.zeros(E, device=d), torch.zeros(E, dtype=i32, device=d),
                              torch.zeros((), dtype=torch.int64), torch.zeros((E, A, 2), dtype=i32, device=d),
                              torch.zeros((E, A, 2), dtype=i32, device=d), torch.zeros((E, A), dtype=u8, device=d),
                              torch.zeros((E, G, G), dtype=u8, device=d))

    def alloc_obs(self) -> Dict[str, torch.Tensor]:
        E, A, d = self.num_envs, self.num_agents, self.device
        return {
            "agents_view": torch.empty((E, A, self.obs_dim), device=d),
            "global_state": torch.empty((E, 1, self.state_dim), device=d),
            "action_mask": torch.empty((E, A, self.action_dim), dtype=torch.uint8, device=d),
            "step_count": torch.empty((E, A), dtype=torch.int32, device=d),
        }

    # ---- kernel call ----------------------------------------------------------------------
    def step_into(self, state: ConnectorState, t: int, obs: Dict[str, torch.Tensor], reward=None, done=None,
                  info_return=None, info_length=None, info_terminal=None, is_reset: bool = False,
                  env_offset: Optional[int] = None, t_base: Optional[torch.Tensor] = None,
                  action: Optional[torch.Tensor] = None, real_obs: Optional[Dict[str, torch.Tensor]] = None,
                  terminated: Optional[torch.Tensor] = None) -> None:
        """One vectorised step (or reset) with the (E, A) int32 `action`, writing the next observation into `obs` and the
        transition into the given (E, A) / (E,) slots.  `t` is the replica's global step index (Philox counter of the
        resets); `t_base` (a device int32 word) is added to it on the device, for rollouts replayed from a captured
        graph.  `real_obs` ({"agents_view", "action_mask"}) and `terminated` (E,) u8, given together, receive the
        pre-reset observation (AutoResetWrapper's extras["real_next_obs"]) and the termination flag (no agent has a legal
        move; a time-limit end alone is a truncation) - mava_connector_step_real_next; they are not written on a reset."""
        off = self.env_offset if env_offset is None else env_offset
        if not is_reset and (action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents):
            raise ValueError("Connector.step_into needs the (E, A) int32 discrete actions of the step")
        if (real_obs is None) != (terminated is None):
            raise ValueError("Connector.step_into: real_obs and terminated go together")
        real = () if real_obs is None else (ptr(real_obs["agents_view"]), ptr(real_obs["action_mask"]), ptr(terminated))
        launch("env_step", lib().mava_connector_step_real_next if real else lib().mava_connector_step, self.num_envs,
               self.num_agents, self.grid_size, self.time_limit, self.seed & 0xFFFFFFFFFFFFFFFF, t & 0xFFFFFFFF, ptr(t_base),
               off & 0xFFFFFFFF, int(is_reset), ptr(state.head), ptr(state.target), ptr(state.connected), ptr(state.grid),
               ptr(state.step_count), ptr(state.run_return), ptr(state.run_length), ptr(state.ep_return),
               ptr(state.ep_length), ptr(obs["agents_view"]), ptr(obs["global_state"]), ptr(obs["action_mask"]),
               ptr(obs["step_count"]), ptr(reward), ptr(done), ptr(info_return), ptr(info_length), ptr(info_terminal),
               None if is_reset else ptr(action), *real, stream_ptr())

    # ---- MarlEnv-style batched API (allocating; the learner uses step_into) -----------------
    def _observation(self, obs: Dict[str, torch.Tensor]):
        mask = obs["action_mask"].bool()
        if self.add_global_state:
            gs = obs["global_state"].expand(-1, self.num_agents, -1)
            return ObservationGlobalState(obs["agents_view"], mask, gs, obs["step_count"])
        return Observation(obs["agents_view"], mask, obs["step_count"])

    def reset(self, key: Any = None) -> Tuple[ConnectorState, TimeStep]:
        state, obs = self.alloc_state(), self.alloc_obs()
        self.step_into(state, 0, obs, is_reset=True)
        E, A, d = self.num_envs, self.num_agents, self.device
        extras = {"episode_metrics": {"episode_return": torch.zeros(E, device=d),
                                      "episode_length": torch.zeros(E, dtype=torch.int32, device=d),
                                      "is_terminal_step": torch.zeros(E, dtype=torch.bool, device=d)}}
        ts = TimeStep(torch.zeros(E, dtype=torch.int8, device=d), torch.zeros((E, A), device=d),
                      torch.ones((E, A), device=d), self._observation(obs), extras)
        return state, ts

    def step(self, state: ConnectorState, action: torch.Tensor) -> Tuple[ConnectorState, TimeStep]:
        E, A, d = self.num_envs, self.num_agents, self.device
        obs = self.alloc_obs()
        reward = torch.empty((E, A), device=d)
        done = torch.empty((E, A), dtype=torch.uint8, device=d)
        ir = torch.empty(E, device=d)
        il = torch.empty(E, dtype=torch.int32, device=d)
        it = torch.empty(E, dtype=torch.uint8, device=d)
        t = int(state.t) + 1
        self.step_into(state, t, obs, reward, done, ir, il, it, action=action.to(torch.int32).contiguous())
        state = state._replace(t=torch.tensor(t, dtype=torch.int64))
        last = it.bool()
        extras = {"episode_metrics": {"episode_return": ir, "episode_length": il, "is_terminal_step": last}}
        step_type = torch.where(last, 2, 1).to(torch.int8)
        ts = TimeStep(step_type, reward, 1.0 - done.float(), self._observation(obs), extras)
        return state, ts


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=connector` configuration, sized by config.arch.num_envs / num_eval_episodes.  The
    time limit is the scenario's (env.scenario.env_kwargs.time_limit); env.kwargs.time_limit overrides it."""
    head = config.network.get("action_head", None) or {}
    if "ContinuousActionHead" in str(head.get("_target_", "")):
        raise ValueError("Connector has discrete actions only: use a DiscreteActionHead")
    scen = config.env.scenario
    tc = scen.task_config
    time_limit = (config.env.get("kwargs", None) or {}).get("time_limit", None)
    if time_limit is None:
        time_limit = (scen.get("env_kwargs", None) or {}).get("time_limit", 50)
    kw = dict(grid_size=int(tc.grid_size), num_agents=int(tc.num_agents), time_limit=int(time_limit),
              add_global_state=add_global_state, device=device)
    seed = int(config.system.seed)
    train = Connector(num_envs=int(config.arch.num_envs), env_offset=env_offset, seed=seed, **kw)
    # the evaluation envs draw from their own Philox key, as the synthetic env's do
    evale = Connector(num_envs=int(config.arch.num_eval_episodes), env_offset=env_offset, seed=seed ^ EVAL_KEY_TAG, **kw)
    return train, evale
