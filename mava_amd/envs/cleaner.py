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

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from .._lib import launch, lib, ptr, stream_ptr
from ..types import Observation, ObservationGlobalState, TimeStep
from .synthetic_rware import EVAL_KEY_TAG, ObsSpec

MAX_SIDE, MAX_AGENTS = 32, 32  # compile-time maxima of csrc/cleaner.hip
NUM_ACTIONS = 4  # UP, RIGHT, DOWN, LEFT


class CleanerState(NamedTuple):
    # the five fields the learners read, with SynthState's names and meaning
    step_count: torch.Tensor  # (E, A) i32
    run_return: torch.Tensor  # (E,) f32
    run_length: torch.Tensor  # (E,) i32
    ep_return: torch.Tensor  # (E,) f32
    ep_length: torch.Tensor  # (E,) i32
    t: torch.Tensor  # () i64 host-side step counter of the allocating API
    pos: torch.Tensor  # (E, A, 2) i32 (row, col)
    grid: torch.Tensor  # (E, R, C) u8: 0 dirty, 1 clean, 2 wall


class Cleaner:
    action_dim = NUM_ACTIONS
    gs_tiles = 1
    global_state_shared = True
    supports_fused_rollout = False
    emits_real_next_obs = True  # step_into(real_obs=, terminated=): what rec_iql stores as next_obs / terminal
    implicit_agent_id = True  # no one-hot id in agents_view; system.add_agent_id is ignored, as the reference's make_env does

    def __init__(self, num_envs: int, num_rows: int, num_cols: int, num_agents: int, time_limit: int = 25,
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0, device: Optional[torch.device] = None):
        R, C, A = int(num_rows), int(num_cols), int(num_agents)
        if not (3 <= R <= MAX_SIDE and 3 <= C <= MAX_SIDE):
            raise ValueError(f"Cleaner supports 3 <= num_rows, num_cols <= {MAX_SIDE}; got {R} x {C}")
        if not (1 <= A <= MAX_AGENTS):
            raise ValueError(f"Cleaner supports 1 <= num_agents <= {MAX_AGENTS}; got {A}")
        if int(time_limit) < 1:
            raise ValueError(f"time_limit must be >= 1, got {time_limit}")
        self.num_envs, self.num_agents, self.time_limit = int(num_envs), A, int(time_limit)
        self.num_rows, self.num_cols = R, C
        self.add_global_state = add_global_state
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.obs_shape: Tuple[int, int, int] = (R, C, 4)
        self.state_shape: Tuple[int, int, int] = (R, C, 3)

    def clone(self, env_offset: int, num_envs: Optional[int] = None) -> "Cleaner":
        """Same scenario on a disjoint range of global env ids (one per replica / rank)."""
        return Cleaner(num_envs or self.num_envs, self.num_rows, self.num_cols, self.num_agents, self.time_limit,
                       self.add_global_state, self.seed, env_offset, self.device)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        return self.num_rows * self.num_cols * 4

    @property
    def state_dim(self) -> int:
        return self.num_rows * self.num_cols * 3

    def observation_spec(self) -> ObsSpec:
        A = self.num_agents
        return ObsSpec((A, self.obs_dim), (A, self.action_dim), (A, self.state_dim) if self.add_global_state else None, (A,))

    def alloc_state(self) -> CleanerState:
        E, A, d = self.num_envs, self.num_agents, self.device
        i32 = torch.int32
        return CleanerState(torch.zeros((E, A), dtype=i32, device=d), torch.zeros(E, device=d),
                            torch.zeros(E, dtype=i32, device=d), torch.zeros(E, device=d), torch.zeros(E, dtype=i32, device=d),
                            torch.zeros((), dtype=torch.int64), torch.zeros((E, A, 2), dtype=i32, device=d),
                            torch.zeros((E, self.num_rows, self.num_cols), dtype=torch.uint8, device=d))

    def alloc_obs(self) -> Dict[str, torch.Tensor]:
        E, A, d = self.num_envs, self.num_agents, self.device
        return {
            "agents_view": torch.empty((E, A, self.obs_dim), device=d),
            "global_state": torch.empty((E, 1, self.state_dim), device=d),
            "action_mask": torch.empty((E, A, self.action_dim), dtype=torch.uint8, device=d),
            "step_count": torch.empty((E, A), dtype=torch.int32, device=d),
        }

    # ---- kernel call ----------------------------------------------------------------------
    def step_into(self, state: CleanerState, t: int, obs: Dict[str, torch.Tensor], reward=None, done=None,
                  info_return=None, info_length=None, info_terminal=None, is_reset: bool = False,
                  env_offset: Optional[int] = None, t_base: Optional[torch.Tensor] = None,
                  action: Optional[torch.Tensor] = None, real_obs: Optional[Dict[str, torch.Tensor]] = None,
                  terminated: Optional[torch.Tensor] = None, info_won: Optional[torch.Tensor] = None) -> None:
        """One vectorised step (or reset) with the (E, A) int32 `action`, writing the next observation into `obs` and the
        transition into the given (E, A) / (E,) slots.  `t` is the replica's global step index (Philox counter of the
        resets); `t_base` (a device int32 word) is added to it on the device, for rollouts replayed from a captured
        graph.  `real_obs` ({"agents_view", "action_mask"}) and `terminated` (E,) u8, given together, receive the
        pre-reset observation (AutoResetWrapper's extras["real_next_obs"]) and the termination flag (won or an invalid
        action; a time-limit end alone is a truncation) - mava_cleaner_step_real_next; they are not written on a reset.
        `info_won` (E,) u8, optional, receives done & won (the learners do not pass it)."""
        off = self.env_offset if env_offset is None else env_offset
        if not is_reset and (action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents):
            raise ValueError("Cleaner.step_into needs the (E, A) int32 discrete actions of the step")
        if (real_obs is None) != (terminated is None):
            raise ValueError("Cleaner.step_into: real_obs and terminated go together")
        real = () if real_obs is None else (ptr(real_obs["agents_view"]), ptr(real_obs["action_mask"]), ptr(terminated))
        launch("env_step", lib().mava_cleaner_step_real_next if real else lib().mava_cleaner_step, self.num_envs,
               self.num_agents, self.num_rows, self.num_cols, self.time_limit, self.seed & 0xFFFFFFFFFFFFFFFF, t & 0xFFFFFFFF,
               ptr(t_base), off & 0xFFFFFFFF, int(is_reset), ptr(state.pos), ptr(state.grid), ptr(state.step_count),
               ptr(state.run_return), ptr(state.run_length), ptr(state.ep_return), ptr(state.ep_length),
               ptr(obs["agents_view"]), ptr(obs["global_state"]), ptr(obs["action_mask"]), ptr(obs["step_count"]),
               ptr(reward), ptr(done), ptr(info_return), ptr(info_length), ptr(info_terminal), ptr(info_won),
               None if is_reset else ptr(action), *real, stream_ptr())

    # ---- MarlEnv-style batched API (allocating; the learner uses step_into) -----------------
    def _observation(self, obs: Dict[str, torch.Tensor]):
        mask = obs["action_mask"].bool()
        if self.add_global_state:
            gs = obs["global_state"].expand(-1, self.num_agents, -1)
            return ObservationGlobalState(obs["agents_view"], mask, gs, obs["step_count"])
        return Observation(obs["agents_view"], mask, obs["step_count"])

    def reset(self, key: Any = None) -> Tuple[CleanerState, TimeStep]:
        state, obs = self.alloc_state(), self.alloc_obs()
        self.step_into(state, 0, obs, is_reset=True)
        E, A, d = self.num_envs, self.num_agents, self.device
        extras = {"episode_metrics": {"episode_return": torch.zeros(E, device=d),
                                      "episode_length": torch.zeros(E, dtype=torch.int32, device=d),
                                      "is_terminal_step": torch.zeros(E, dtype=torch.bool, device=d)},
                  "won_episode": torch.zeros(E, dtype=torch.bool, device=d)}
        ts = TimeStep(torch.zeros(E, dtype=torch.int8, device=d), torch.zeros((E, A), device=d),
                      torch.ones((E, A), device=d), self._observation(obs), extras)
        return state, ts

    def step(self, state: CleanerState, action: torch.Tensor) -> Tuple[CleanerState, TimeStep]:
        E, A, d = self.num_envs, self.num_agents, self.device
        obs = self.alloc_obs()
        reward = torch.empty((E, A), device=d)
        done = torch.empty((E, A), dtype=torch.uint8, device=d)
        ir = torch.empty(E, device=d)
        il = torch.empty(E, dtype=torch.int32, device=d)
        it = torch.empty(E, dtype=torch.uint8, device=d)
        won = torch.empty(E, dtype=torch.uint8, device=d)
        t = int(state.t) + 1
        self.step_into(state, t, obs, reward, done, ir, il, it, action=action.to(torch.int32).contiguous(), info_won=won)
        state = state._replace(t=torch.tensor(t, dtype=torch.int64))
        last = it.bool()
        extras = {"episode_metrics": {"episode_return": ir, "episode_length": il, "is_terminal_step": last},
                  "won_episode": won.bool()}
        step_type = torch.where(last, 2, 1).to(torch.int8)
        ts = TimeStep(step_type, reward, 1.0 - done.float(), self._observation(obs), extras)
        return state, ts


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=cleaner` configuration, sized by config.arch.num_envs / num_eval_episodes.  The
    time limit is the scenario's (env.scenario.env_kwargs.time_limit); env.kwargs.time_limit overrides it."""
    head = config.network.get("action_head", None) or {}
    if "ContinuousActionHead" in str(head.get("_target_", "")):
        raise ValueError("Cleaner has discrete actions only: use a DiscreteActionHead")
    scen = config.env.scenario
    tc = scen.task_config
    time_limit = (config.env.get("kwargs", None) or {}).get("time_limit", None)
    if time_limit is None:
        time_limit = (scen.get("env_kwargs", None) or {}).get("time_limit", 25)
    kw = dict(num_rows=int(tc.num_rows), num_cols=int(tc.num_cols), num_agents=int(tc.num_agents), time_limit=int(time_limit),
              add_global_state=add_global_state, device=device)
    seed = int(config.system.seed)
    train = Cleaner(num_envs=int(config.arch.num_envs), env_offset=env_offset, seed=seed, **kw)
    # the evaluation envs draw from their own Philox key, as the synthetic env's do
    evale = Cleaner(num_envs=int(config.arch.num_eval_episodes), env_offset=env_offset, seed=seed ^ EVAL_KEY_TAG, **kw)
    return train, evale
