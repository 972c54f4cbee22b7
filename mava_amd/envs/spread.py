"""Spread (the `env=spread` task) on the GPU: mava_spread_step (csrc/spread.hip).

This project's own continuous-action task, modelled on MPE `simple_spread` (cooperative navigation): A agents and A
landmarks in the square [-1, 1]^2.  An action is a displacement, (A, 2) f32 clamped to [-1, 1] and scaled by 0.1; the
team is paid minus the mean over landmarks of the distance to the closest agent and fined 0.5 / A per pair of agents
closer than 0.15.  The rules never end an episode, the time limit (default 25) truncates it.  The complete rules are in
DESIGN.md "Spread", include/mava_hip.h and, as the contract, tests/spread_model.py.

It stands in for MaBrax, the Brax physics task the reference pairs with its soft actor-critic systems, which cannot be
restated here; it restates no environment of the reference.  It is the one environment of this package whose rewards
depend on a continuous action: `continuous_actions` tells the learners to hand it the f32 action they stored.

`agents_view` is [one-hot id (only with system.add_agent_id),] own position, landmarks relative to self, the other
agents relative to self; `global_state` the agent then the landmark positions; `action_mask` all ones, (A, 2).

The object has the batched MarlEnv surface of LevelBasedForaging: `step_into` writes straight into trajectory slots
owned by the learner, `reset` / `step` allocate.  It declares no fused rollout.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .._lib import ptr
from ..types import TimeStep
from .base import COMMON_STATE, BatchedEnv, make_pair

MIN_AGENTS, MAX_AGENTS = 2, 8  # compile-time bounds of csrc/spread.hip
ACTION_DIM = 2  # (dx, dy)
SCENARIOS = {"spread-2a": 2, "spread-3a": 3, "spread-5a": 5}


SpreadState = NamedTuple("SpreadState", COMMON_STATE + [
    ("agent_pos", torch.Tensor),  # (E, A, 2) f32 (x, y)
    ("landmark_pos", torch.Tensor),  # (E, A, 2) f32
])


class Spread(BatchedEnv):
    State = SpreadState
    action_dim = ACTION_DIM
    continuous_actions = True  # the learners pass the stored f32 action, not an int32 index
    step_symbol = "mava_spread_step"  # terminated: never (the time limit truncates)
    real_extra_keys = ("global_state",)  # real_obs["global_state"] (E, 1, 4A), optional: ff_masac stores it as next state

    def __init__(self, num_envs: int, num_agents: int = 3, time_limit: int = 25, add_agent_id: bool = False,
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0,
                 device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        A = int(num_agents)
        if not (MIN_AGENTS <= A <= MAX_AGENTS):
            raise ValueError(f"Spread supports {MIN_AGENTS} <= num_agents <= {MAX_AGENTS}; got {A}")
        if int(time_limit) < 1:
            raise ValueError(f"time_limit must be >= 1, got {time_limit}")
        super().__init__(kw)
        self.add_agent_id = bool(add_agent_id)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        A = self.num_agents
        return (A if self.add_agent_id else 0) + 2 + 2 * A + 2 * (A - 1)

    @property
    def state_dim(self) -> int:
        return 4 * self.num_agents

    def alloc_own_state(self) -> tuple:
        E, A, d = self.num_envs, self.num_agents, self.device
        return (torch.zeros((E, A, 2), device=d), torch.zeros((E, A, 2), device=d))

    def step_args(self, state: SpreadState):
        return ((int(self.add_agent_id), self.time_limit), (ptr(state.agent_pos), ptr(state.landmark_pos)))

    def _action_ptr(self, action: Optional[torch.Tensor], is_reset: bool) -> Optional[int]:
        if is_reset:
            return None
        if (action is None or action.dtype != torch.float32 or not action.is_contiguous()
                or action.numel() != self.num_envs * self.num_agents * ACTION_DIM):
            raise ValueError("Spread.step_into needs the contiguous (E, A, 2) float32 continuous actions of the step")
        return ptr(action)

    def step(self, state, action: torch.Tensor):
        """BatchedEnv.step with the float action (the base class casts to int32)."""
        E, A, d = self.num_envs, self.num_agents, self.device
        obs = self.alloc_obs()
        reward = torch.empty((E, A), device=d)
        done = torch.empty((E, A), dtype=torch.uint8, device=d)
        ir = torch.empty(E, device=d)
        il = torch.empty(E, dtype=torch.int32, device=d)
        it = torch.empty(E, dtype=torch.uint8, device=d)
        t = int(state.t) + 1
        self.step_into(state, t, obs, reward, done, ir, il, it, action=action.to(torch.float32).contiguous())
        state = state._replace(t=torch.tensor(t, dtype=torch.int64))
        last = it.bool()
        extras = {"episode_metrics": {"episode_return": ir, "episode_length": il, "is_terminal_step": last}}
        step_type = torch.where(last, 2, 1).to(torch.int8)
        return state, TimeStep(step_type, reward, 1.0 - done.float(), self._observation(obs), extras)


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=spread` configuration, sized by config.arch.num_envs / num_eval_episodes.  The
    time limit is the scenario's (env.scenario.env_kwargs.time_limit); env.kwargs.time_limit overrides it.  The one-hot
    agent id follows system.add_agent_id."""
    head = config.network.get("action_head", None) or {}
    if "DiscreteActionHead" in str(head.get("_target_", "")):
        raise ValueError("Spread has continuous actions only: use a ContinuousActionHead (network=continuous_mlp)")
    scen = config.env.scenario
    time_limit = (config.env.get("kwargs", None) or {}).get("time_limit", None)
    if time_limit is None:
        time_limit = (scen.get("env_kwargs", None) or {}).get("time_limit", 25)
    add_id = bool(config.system.add_agent_id) and not bool(config.env.get("implicit_agent_id", False))
    kw = dict(num_agents=int(scen.task_config.num_agents), time_limit=int(time_limit), add_agent_id=add_id,
              add_global_state=add_global_state, device=device)
    return make_pair(Spread, config, kw, env_offset, discrete_only=False)
