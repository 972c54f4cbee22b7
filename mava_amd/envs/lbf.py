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

from typing import NamedTuple, Optional

import torch

from .._lib import ptr
from .base import COMMON_STATE, BatchedEnv, make_pair

MAX_GRID, MAX_AGENTS, MAX_FOOD, MAX_LEVEL = 32, 16, 16, 1000  # compile-time maxima of csrc/lbf.hip
NUM_ACTIONS = 6  # NOOP, UP, DOWN, LEFT, RIGHT, LOAD


LBFState = NamedTuple("LBFState", COMMON_STATE + [
    ("agent_pos", torch.Tensor),  # (E, A, 2) i32 (row, col)
    ("agent_level", torch.Tensor),  # (E, A) i32
    ("food_pos", torch.Tensor),  # (E, F, 2) i32
    ("food_level", torch.Tensor),  # (E, F) i32
    ("food_alive", torch.Tensor),  # (E, F) u8
    ("total_food_level", torch.Tensor),  # (E,) f32
])


class LevelBasedForaging(BatchedEnv):
    State = LBFState
    action_dim = NUM_ACTIONS
    step_symbol = "mava_lbf_step"  # terminated: every food eaten

    def __init__(self, num_envs: int, grid_size: int, fov: int, num_agents: int, num_food: int, max_agent_level: int,
                 force_coop: bool, time_limit: int = 100, use_individual_rewards: bool = False,
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0,
                 device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        G, A, F = int(grid_size), int(num_agents), int(num_food)
        if not (3 <= G <= MAX_GRID and 1 <= A <= MAX_AGENTS and 1 <= F <= MAX_FOOD):
            raise ValueError(f"LBF supports 3 <= grid_size <= {MAX_GRID}, 1 <= num_agents <= {MAX_AGENTS}, "
                             f"1 <= num_food <= {MAX_FOOD}; got {G}, {A}, {F}")
        if (G - 2) ** 2 < 9 * (F - 1) + 1 or G * G < F + A:
            raise ValueError(f"a {G}x{G} grid cannot place {F} non-adjacent interior foods and {A} agents")
        if not (1 <= int(max_agent_level) <= MAX_LEVEL) or int(fov) < 0 or int(time_limit) < 1:
            raise ValueError(f"bad LBF scenario: max_agent_level={max_agent_level}, fov={fov}, time_limit={time_limit}")
        super().__init__(kw)
        self.num_food, self.grid_size = F, G
        self.fov, self.max_agent_level, self.force_coop = int(fov), int(max_agent_level), bool(force_coop)
        self.use_individual_rewards = bool(use_individual_rewards)

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

    def alloc_own_state(self) -> tuple:
        E, A, F, d = self.num_envs, self.num_agents, self.num_food, self.device
        i32 = torch.int32
        return (torch.zeros((E, A, 2), dtype=i32, device=d), torch.zeros((E, A), dtype=i32, device=d),
                torch.zeros((E, F, 2), dtype=i32, device=d), torch.zeros((E, F), dtype=i32, device=d),
                torch.zeros((E, F), dtype=torch.uint8, device=d), torch.zeros(E, device=d))

    def step_args(self, state: LBFState):
        return ((self.num_food, self.grid_size, self.fov, self.max_agent_level, int(self.force_coop),
                 int(self.use_individual_rewards), self.time_limit),
                (ptr(state.agent_pos), ptr(state.agent_level), ptr(state.food_pos), ptr(state.food_level),
                 ptr(state.food_alive), ptr(state.total_food_level)))


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=lbf` configuration, sized by config.arch.num_envs / num_eval_episodes."""
    if not bool(config.system.add_agent_id) or bool(config.env.implicit_agent_id):
        raise NotImplementedError("LevelBasedForaging always prepends the agent one-hot id (add_agent_id=True)")
    tc = config.env.scenario.task_config
    kw = dict(grid_size=int(tc.grid_size), fov=int(tc.fov), num_agents=int(tc.num_agents), num_food=int(tc.num_food),
              max_agent_level=int(tc.max_agent_level), force_coop=bool(tc.force_coop),
              time_limit=int(config.env.kwargs.get("time_limit", 100)),
              use_individual_rewards=bool(config.env.get("use_individual_rewards", False)),
              add_global_state=add_global_state, device=device)
    return make_pair(LevelBasedForaging, config, kw, env_offset)
