"""Robot Warehouse (the `env=rware_native` task) on the GPU: mava_rware_step (csrc/rware.hip).

An H x W warehouse of highways and shelf homes, A robots that turn, drive forward and load / unload shelves, and a queue
of requested shelves: a robot that stands on a goal cell with a requested shelf scores 1 for the team.  The complete
rules are in DESIGN.md "Robot Warehouse" and include/mava_hip.h; they follow the published RWARE task - parity with
Jumanji's RobotWarehouse itself is UNPINNED (its source is not part of this project).  `env=rware` remains the synthetic
stand-in of the benchmark (envs/synthetic_rware.py).

The object has the batched MarlEnv surface of LevelBasedForaging: `step_into` writes straight into trajectory slots
owned by the learner, `reset` / `step` allocate.  It declares no fused rollout, so the feed-forward learner steps it
per time step (captured into a HIP graph from the second rollout on).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Tuple

import torch

from .._lib import ptr
from .base import COMMON_STATE, BatchedEnv, make_pair

MAX_GRID, MAX_AGENTS, MAX_SHELVES, MAX_QUEUE, MAX_SENSOR = 32, 16, 256, 16, 2  # compile-time maxima of csrc/rware.hip
NUM_ACTIONS = 5  # NOOP, FORWARD, LEFT, RIGHT, TOGGLE_LOAD
COLLISION_MODES = ("terminate", "overlap")


class Layout(NamedTuple):
    height: int
    width: int
    highway_rows: List[int]  # bit x of word y: cell (x, y) is a highway
    shelf_home: List[int]  # cell (y * width + x) of shelf s, increasing
    goals: Tuple[Tuple[int, int], Tuple[int, int]]  # (x, y)


def warehouse_layout(column_height: int, shelf_rows: int, shelf_columns: int) -> Layout:
    """The warehouse of a scenario: highways every third column and between the shelf blocks, a bottom row with the two
    goals in its middle and a two-cell corridor leading up from them through the lowest block."""
    ch, H, W = int(column_height), (int(column_height) + 1) * int(shelf_rows) + 2, 3 * int(shelf_columns) + 1
    rows = []
    for y in range(H):
        m = 0
        for x in range(W):
            if x % 3 == 0 or y % (ch + 1) == 0 or y == H - 1 or (y > H - (ch + 3) and x in (W // 2 - 1, W // 2)):
                m |= 1 << x
        rows.append(m)
    homes = [y * W + x for y in range(H) for x in range(W) if not (rows[y] >> x) & 1]
    return Layout(H, W, rows, homes, ((W // 2 - 1, H - 1), (W // 2, H - 1)))


RwareState = NamedTuple("RwareState", COMMON_STATE + [
    ("agent_pos", torch.Tensor),  # (E, A, 2) i32 (x, y)
    ("agent_dir", torch.Tensor),  # (E, A) i32: 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT
    ("agent_carry", torch.Tensor),  # (E, A) i32 shelf id or -1
    ("shelf_pos", torch.Tensor),  # (E, S) i32 cell (y * W + x); a carried shelf has its carrier's cell
    ("request_queue", torch.Tensor),  # (E, R) i32 distinct shelf ids
])


class RobotWarehouse(BatchedEnv):
    State = RwareState
    action_dim = NUM_ACTIONS
    step_symbol = "mava_rware_step"  # terminated: a collision in mode "terminate"

    def __init__(self, num_envs: int, column_height: int, shelf_rows: int, shelf_columns: int, num_agents: int,
                 sensor_range: int, request_queue_size: int, time_limit: int = 500, collision_mode: str = "terminate",
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0,
                 device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        ch, sr, sc = int(column_height), int(shelf_rows), int(shelf_columns)
        if ch < 1 or sr < 1 or sc < 1:
            raise ValueError(f"bad warehouse: column_height={ch}, shelf_rows={sr}, shelf_columns={sc}")
        H, W = (ch + 1) * sr + 2, 3 * sc + 1
        if H > MAX_GRID or W > MAX_GRID:
            raise ValueError(f"RobotWarehouse supports grids up to {MAX_GRID} x {MAX_GRID}; this scenario is {H} x {W}")
        lay = warehouse_layout(ch, sr, sc)
        A, S, R = int(num_agents), len(lay.shelf_home), int(request_queue_size)
        if not (1 <= A <= MAX_AGENTS) or A > H * W:
            raise ValueError(f"RobotWarehouse supports 1 <= num_agents <= {MAX_AGENTS} (and <= H * W); got {A}")
        if S > MAX_SHELVES:
            raise ValueError(f"RobotWarehouse supports up to {MAX_SHELVES} shelves; this scenario has {S}")
        if not (1 <= R <= MAX_QUEUE) or R >= S:
            raise ValueError(f"request_queue_size must be in 1 .. min({MAX_QUEUE}, shelves - 1 = {S - 1}); got {R}")
        if not (1 <= int(sensor_range) <= MAX_SENSOR) or int(time_limit) < 1:
            raise ValueError(f"bad RWARE scenario: sensor_range={sensor_range} (1 .. {MAX_SENSOR}), time_limit={time_limit}")
        if collision_mode not in COLLISION_MODES:
            raise ValueError(f"collision_mode must be one of {COLLISION_MODES}, got {collision_mode!r}")
        super().__init__(kw)
        self.num_shelves, self.request_queue_size = S, R
        self.column_height, self.shelf_rows, self.shelf_columns = ch, sr, sc
        self.layout, self.height, self.width = lay, H, W
        self.sensor_range, self.collision_mode = int(sensor_range), collision_mode
        # the layout travels with every launch as kernel arguments: host arrays, built once
        self._highway_rows = (C.c_uint32 * H)(*lay.highway_rows)
        self._shelf_home = (C.c_int32 * S)(*lay.shelf_home)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def raw_obs_dim(self) -> int:
        return 8 + 7 * (2 * self.sensor_range + 1) ** 2

    @property
    def obs_dim(self) -> int:
        return self.num_agents + self.raw_obs_dim

    @property
    def state_dim(self) -> int:
        return self.num_agents * self.raw_obs_dim

    def alloc_own_state(self) -> tuple:
        E, A, S, R, d = self.num_envs, self.num_agents, self.num_shelves, self.request_queue_size, self.device
        i32 = torch.int32
        return (torch.zeros((E, A, 2), dtype=i32, device=d), torch.zeros((E, A), dtype=i32, device=d),
                torch.full((E, A), -1, dtype=i32, device=d), torch.zeros((E, S), dtype=i32, device=d),
                torch.zeros((E, R), dtype=i32, device=d))

    def step_args(self, state: RwareState):
        return ((self.num_shelves, self.request_queue_size, self.height, self.width, self.sensor_range, self.time_limit,
                 int(self.collision_mode == "terminate"), self._highway_rows, self._shelf_home),
                (ptr(state.agent_pos), ptr(state.agent_dir), ptr(state.agent_carry), ptr(state.shelf_pos),
                 ptr(state.request_queue)))


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=rware_native` configuration, sized by config.arch.num_envs / num_eval_episodes."""
    if not bool(config.system.add_agent_id) or bool(config.env.implicit_agent_id):
        raise ValueError("RobotWarehouse always prepends the agent one-hot id (add_agent_id=True)")
    tc = config.env.scenario.task_config
    kw = dict(column_height=int(tc.column_height), shelf_rows=int(tc.shelf_rows), shelf_columns=int(tc.shelf_columns),
              num_agents=int(tc.num_agents), sensor_range=int(tc.sensor_range),
              request_queue_size=int(tc.request_queue_size), time_limit=int(config.env.kwargs.get("time_limit", 500)),
              collision_mode=str(config.env.kwargs.get("collision_mode", "terminate")),
              add_global_state=add_global_state, device=device)
    return make_pair(RobotWarehouse, config, kw, env_offset)
