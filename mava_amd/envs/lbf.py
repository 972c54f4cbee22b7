"""Level-Based Foraging (the `env=lbf` task of Mava's config set) on the GPU: mava_lbf_step (csrc/lbf.hip).

A G x G grid, A agents and F foods with levels.  Each step an agent moves (UP / DOWN / LEFT / RIGHT), waits (NOOP) or
LOADs; a food is eaten when the LOADing agents next to it together reach its level, and its reward is split between
them in proportion to their levels.  The complete rules are in DESIGN.md "Level-Based Foraging" and
include/mava_hip.h; they follow the published LBF task and Jumanji's documented behaviour - parity with Jumanji's
LevelBasedForaging itself is UNPINNED (its source is not part of this project).

The object has the batched MarlEnv surface of SyntheticRware (the one the learners and the evaluator use): `step_into`
writes straight into trajectory slots owned by the learner, `reset` / `step` allocate.  It declares no fused rollout,
so the feed-forward learner steps it per time step (captured into a HIP graph from the second rollout on).
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from .._lib import launch, lib, ptr, stream_ptr
from ..types import Observation, ObservationGlobalState, TimeStep
from .synthetic_rware import EVAL_KEY_TAG, ObsSpec

MAX_GRID, MAX_AGENTS, MAX_FOOD, MAX_LEVEL = 32, 16, 16, 1000  # compile-time maxima of csrc/lbf.hip
NUM_ACTIONS = 6  # NOOP, UP, DOWN, LEFT, RIGHT, LOAD


class LBFState(NamedTuple):
    # the five fields the learners read, with SynthState's names and meaning
    step_count: torch.Tensor  # (E, A) i32
    run_return: torch.Tensor  # (E,) f32
    run_length: torch.Tensor  # (E,) i32
    ep_return: torch.Tensor  # (E,) f32
    ep_length: torch.Tensor  # (E,) i32
    t: torch.Tensor  # () i64 host-side step counter of the allocating API
    agent_pos: torch.Tensor  # (E, A, 2) i32 (row, col)
    agent_level: torch.Tensor  # (E, A) i32
    food_pos: torch.Tensor  # (E, F, 2) i32
    food_level: torch.Tensor  # (E, F) i32
    food_alive: torch.Tensor  # (E, F) u8
    total_food_level: torch.Tensor  # (E,) f32


class LevelBasedForaging:
    action_dim = NUM_ACTIONS
    gs_tiles = 1
    global_state_shared = True
    supports_fused_rollout = False
    emits_real_next_obs = True  # step_into(real_obs=, terminated=): what rec_iql stores as next_obs / terminal

    def __init__(self, num_envs: int, grid_size: int, fov: int, num_agents: int, num_food: int, max_agent_level: int,
                 force_coop: bool, time_limit: int = 100, use_individual_rewards: bool = False,
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0,
                 device: Optional[torch.device] = None):
        G, A, F = int(grid_size), int(num_agents), int(num_food)
        if not (3 <= G <= MAX_GRID and 1 <= A <= MAX_AGENTS and 1 <= F <= MAX_FOOD):
            raise ValueError(f"LBF supports 3 <= grid_size <= {MAX_GRID}, 1 <= num_agents <= {MAX_AGENTS}, "
                             f"1 <= num_food <= {MAX_FOOD}; got {G}, {A}, {F}")
        if (G - 2) ** 2 < 9 * (F - 1) + 1 or G * G < F + A:
            raise ValueError(f"a {G}x{G} grid cannot place {F} non-adjacent interior foods and {A} agents")
        if not (1 <= int(max_agent_level) <= MAX_LEVEL) or int(fov) < 0 or int(time_limit) < 1:
            raise ValueError(f"bad LBF scenario: max_agent_level={max_agent_level}, fov={fov}, time_limit={time_limit}")
        self.num_envs, self.num_agents, self.num_food, self.grid_size = int(num_envs), A, F, G
        self.fov, self.max_agent_level, self.force_coop = int(fov), int(max_agent_level), bool(force_coop)
        self.time_limit, self.use_individual_rewards = int(time_limit), bool(use_individual_rewards)
        self.add_global_state = add_global_state
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.obs_shape: Optional[tuple] = None
        self.state_shape: Optional[tuple] = None

    def clone(self, env_offset: int, num_envs: Optional[int] = None) -> "LevelBasedForaging":
        """Same scenario on a disjoint range of global env ids (one per replica / rank)."""
        return LevelBasedForaging(num_envs or self.num_envs, self.grid_size, self.fov, self.num_agents, self.num_food,
                                  self.max_agent_level, self.force_coop, self.time_limit, self.use_individual_rewards,
                                  self.add_global_state, self.seed, env_offset, self.device)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def raw_obs_dim(self) -> int:
        return 3 * (self.num_food + self.num_agents)

    @property
    def obs_dim(self) -> int:
        return self.num_agents + self.raw_obs_dim

    @property
    def state_dim(self) -> int:
        return self.num_agents * self.raw_obs_dim

    def observation_spec(self) -> ObsSpec:
        A = self.num_agents
        return ObsSpec((A, self.obs_dim), (A, self.action_dim), (A, self.state_dim) if self.add_global_state else None, (A,))

    def alloc_state(self) -> LBFState:
        E, A, F, d = self.num_envs, self.num_agents, self.num_food, self.device
        i32 = torch.int32
        return LBFState(torch.zeros((E, A), dtype=i32, device=d), torch.zeros(E, device=d),
                        torch.zeros(E, dtype=i32, device=d), torch.zeros(E, device=d), torch.zeros(E, dtype=i32, device=d),
                        torch.zeros((), dtype=torch.int64), torch.zeros((E, A, 2), dtype=i32, device=d),
                        torch.zeros((E, A), dtype=i32, device=d), torch.zeros((E, F, 2), dtype=i32, device=d),
                        torch.zeros((E, F), dtype=i32, device=d), torch.zeros((E, F), dtype=torch.uint8, device=d),
                        torch.zeros(E, device=d))

    def alloc_obs(self) -> Dict[str, torch.Tensor]:
        E, A, d = self.num_envs, self.num_agents, self.device
        return {
            "agents_view": torch.empty((E, A, self.obs_dim), device=d),
            "global_state": torch.empty((E, 1, self.state_dim), device=d),
            "action_mask": torch.empty((E, A, self.action_dim), dtype=torch.uint8, device=d),
            "step_count": torch.empty((E, A), dtype=torch.int32, device=d),
        }

    # ---- kernel call ----------------------------------------------------------------------
    def step_into(self, state: LBFState, t: int, obs: Dict[str, torch.Tensor], reward=None, done=None, info_return=None,
                  info_length=None, info_terminal=None, is_reset: bool = False, env_offset: Optional[int] = None,
                  t_base: Optional[torch.Tensor] = None, action: Optional[torch.Tensor] = None,
                  real_obs: Optional[Dict[str, torch.Tensor]] = None, terminated: Optional[torch.Tensor] = None) -> None:
        """One vectorised step (or reset) with the (E, A) int32 `action`, writing the next observation into `obs` and the
        transition into the given (E, A) / (E,) slots.  `t` is the replica's global step index (Philox counter of the
        resets); `t_base` (a device int32 word) is added to it on the device, for rollouts replayed from a captured graph.
        `real_obs` ({"agents_view", "action_mask"}) and `terminated` (E,) u8, given together, receive the pre-reset
        observation (AutoResetWrapper's extras["real_next_obs"]) and the termination flag (every food eaten; a time-limit
        end is a truncation) - mava_lbf_step_real_next; they are not written on a reset."""
        off = self.env_offset if env_offset is None else env_offset
        if not is_reset and (action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents):
            raise ValueError("LevelBasedForaging.step_into needs the (E, A) int32 discrete actions of the step")
        if (real_obs is None) != (terminated is None):
            raise ValueError("LevelBasedForaging.step_into: real_obs and terminated go together")
        real = () if real_obs is None else (ptr(real_obs["agents_view"]), ptr(real_obs["action_mask"]), ptr(terminated))
        launch("env_step", lib().mava_lbf_step_real_next if real else lib().mava_lbf_step, self.num_envs, self.num_agents, self.num_food, self.grid_size, self.fov,
               self.max_agent_level, int(self.force_coop), int(self.use_individual_rewards), self.time_limit,
               self.seed & 0xFFFFFFFFFFFFFFFF, t & 0xFFFFFFFF, ptr(t_base), off & 0xFFFFFFFF, int(is_reset),
               ptr(state.agent_pos), ptr(state.agent_level), ptr(state.food_pos), ptr(state.food_level),
               ptr(state.food_alive), ptr(state.total_food_level), ptr(state.step_count), ptr(state.run_return),
               ptr(state.run_length), ptr(state.ep_return), ptr(state.ep_length), ptr(obs["agents_view"]),
               ptr(obs["global_state"]), ptr(obs["action_mask"]), ptr(obs["step_count"]), ptr(reward), ptr(done),
               ptr(info_return), ptr(info_length), ptr(info_terminal), None if is_reset else ptr(action), *real, stream_ptr())

    # ---- MarlEnv-style batched API (allocating; the learner uses step_into) -----------------
    def _observation(self, obs: Dict[str, torch.Tensor]):
        mask = obs["action_mask"].bool()
        if self.add_global_state:
            gs = obs["global_state"].expand(-1, self.num_agents, -1)
            return ObservationGlobalState(obs["agents_view"], mask, gs, obs["step_count"])
        return Observation(obs["agents_view"], mask, obs["step_count"])

    def reset(self, key: Any = None) -> Tuple[LBFState, TimeStep]:
        state, obs = self.alloc_state(), self.alloc_obs()
        self.step_into(state, 0, obs, is_reset=True)
        E, A, d = self.num_envs, self.num_agents, self.device
        extras = {"episode_metrics": {"episode_return": torch.zeros(E, device=d),
                                      "episode_length": torch.zeros(E, dtype=torch.int32, device=d),
                                      "is_terminal_step": torch.zeros(E, dtype=torch.bool, device=d)}}
        ts = TimeStep(torch.zeros(E, dtype=torch.int8, device=d), torch.zeros((E, A), device=d),
                      torch.ones((E, A), device=d), self._observation(obs), extras)
        return state, ts

    def step(self, state: LBFState, action: torch.Tensor) -> Tuple[LBFState, TimeStep]:
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
    """(train_env, eval_env) of an `env=lbf` configuration, sized by config.arch.num_envs / num_eval_episodes."""
    head = config.network.get("action_head", None) or {}
    if "ContinuousActionHead" in str(head.get("_target_", "")):
        raise ValueError("LevelBasedForaging has discrete actions only: use a DiscreteActionHead")
    if not bool(config.system.add_agent_id) or bool(config.env.implicit_agent_id):
        raise NotImplementedError("LevelBasedForaging always prepends the agent one-hot id (add_agent_id=True)")
    tc = config.env.scenario.task_config
    kw = dict(grid_size=int(tc.grid_size), fov=int(tc.fov), num_agents=int(tc.num_agents), num_food=int(tc.num_food),
              max_agent_level=int(tc.max_agent_level), force_coop=bool(tc.force_coop),
              time_limit=int(config.env.kwargs.get("time_limit", 100)),
              use_individual_rewards=bool(config.env.get("use_individual_rewards", False)),
              add_global_state=add_global_state, device=device)
    seed = int(config.system.seed)
    train = LevelBasedForaging(num_envs=int(config.arch.num_envs), env_offset=env_offset, seed=seed, **kw)
    # the evaluation envs draw from their own Philox key, as the synthetic env's do
    evale = LevelBasedForaging(num_envs=int(config.arch.num_eval_episodes), env_offset=env_offset, seed=seed ^ EVAL_KEY_TAG, **kw)
    return train, evale
