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
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import torch

from .._lib import launch, lib, ptr, stream_ptr
from ..types import Observation, ObservationGlobalState, TimeStep
from .synthetic_rware import EVAL_KEY_TAG, ObsSpec

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


class RwareState(NamedTuple):
    # the five fields the learners read, with SynthState's names and meaning
    step_count: torch.Tensor  # (E, A) i32
    run_return: torch.Tensor  # (E,) f32
    run_length: torch.Tensor  # (E,) i32
    ep_return: torch.Tensor  # (E,) f32
    ep_length: torch.Tensor  # (E,) i32
    t: torch.Tensor  # () i64 host-side step counter of the allocating API
    agent_pos: torch.Tensor  # (E, A, 2) i32 (x, y)
    agent_dir: torch.Tensor  # (E, A) i32: 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT
    agent_carry: torch.Tensor  # (E, A) i32 shelf id or -1
    shelf_pos: torch.Tensor  # (E, S) i32 cell (y * W + x); a carried shelf has its carrier's cell
    request_queue: torch.Tensor  # (E, R) i32 distinct shelf ids


class RobotWarehouse:
    action_dim = NUM_ACTIONS
    gs_tiles = 1
    global_state_shared = True
    supports_fused_rollout = False
    emits_real_next_obs = True  # step_into(real_obs=, terminated=): what rec_iql stores as next_obs / terminal

    def __init__(self, num_envs: int, column_height: int, shelf_rows: int, shelf_columns: int, num_agents: int,
                 sensor_range: int, request_queue_size: int, time_limit: int = 500, collision_mode: str = "terminate",
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0,
                 device: Optional[torch.device] = None):
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
        self.num_envs, self.num_agents, self.num_shelves, self.request_queue_size = int(num_envs), A, S, R
        self.column_height, self.shelf_rows, self.shelf_columns = ch, sr, sc
        self.layout, self.height, self.width = lay, H, W
        self.sensor_range, self.time_limit, self.collision_mode = int(sensor_range), int(time_limit), collision_mode
        self.add_global_state = add_global_state
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        # the layout travels with every launch as kernel arguments: host arrays, built once
        self._highway_rows = (C.c_uint32 * H)(*lay.highway_rows)
        self._shelf_home = (C.c_int32 * S)(*lay.shelf_home)
        self.obs_shape: Optional[tuple] = None
        self.state_shape: Optional[tuple] = None

    def clone(self, env_offset: int, num_envs: Optional[int] = None) -> "RobotWarehouse":
        """Same scenario on a disjoint range of global env ids (one per replica / rank)."""
        return RobotWarehouse(num_envs or self.num_envs, self.column_height, self.shelf_rows, self.shelf_columns,
                              self.num_agents, self.sensor_range, self.request_queue_size, self.time_limit,
                              self.collision_mode, self.add_global_state, self.seed, env_offset, self.device)

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

    def observation_spec(self) -> ObsSpec:
        A = self.num_agents
        return ObsSpec((A, self.obs_dim), (A, self.action_dim), (A, self.state_dim) if self.add_global_state else None, (A,))

    def alloc_state(self) -> RwareState:
        E, A, S, R, d = self.num_envs, self.num_agents, self.num_shelves, self.request_queue_size, self.device
        i32 = torch.int32
        return RwareState(torch.zeros((E, A), dtype=i32, device=d), torch.zeros(E, device=d),
                          torch.zeros(E, dtype=i32, device=d), torch.zeros(E, device=d), torch.zeros(E, dtype=i32, device=d),
                          torch.zeros((), dtype=torch.int64), torch.zeros((E, A, 2), dtype=i32, device=d),
                          torch.zeros((E, A), dtype=i32, device=d), torch.full((E, A), -1, dtype=i32, device=d),
                          torch.zeros((E, S), dtype=i32, device=d), torch.zeros((E, R), dtype=i32, device=d))

    def alloc_obs(self) -> Dict[str, torch.Tensor]:
        E, A, d = self.num_envs, self.num_agents, self.device
        return {
            "agents_view": torch.empty((E, A, self.obs_dim), device=d),
            "global_state": torch.empty((E, 1, self.state_dim), device=d),
            "action_mask": torch.empty((E, A, self.action_dim), dtype=torch.uint8, device=d),
            "step_count": torch.empty((E, A), dtype=torch.int32, device=d),
        }

    # ---- kernel call ----------------------------------------------------------------------
    def step_into(self, state: RwareState, t: int, obs: Dict[str, torch.Tensor], reward=None, done=None, info_return=None,
                  info_length=None, info_terminal=None, is_reset: bool = False, env_offset: Optional[int] = None,
                  t_base: Optional[torch.Tensor] = None, action: Optional[torch.Tensor] = None,
                  real_obs: Optional[Dict[str, torch.Tensor]] = None, terminated: Optional[torch.Tensor] = None) -> None:
        """One vectorised step (or reset) with the (E, A) int32 `action`, writing the next observation into `obs` and the
        transition into the given (E, A) / (E,) slots.  `t` is the replica's global step index (Philox counter of the
        resets and queue refills); `t_base` (a device int32 word) is added to it on the device, for rollouts replayed
        from a captured graph.  `real_obs` ({"agents_view", "action_mask"}) and `terminated` (E,) u8, given together,
        receive the pre-reset observation (AutoResetWrapper's extras["real_next_obs"]) and the termination flag (a
        collision in collision mode "terminate"; a time-limit end is a truncation) - mava_rware_step_real_next; they
        are not written on a reset."""
        off = self.env_offset if env_offset is None else env_offset
        if not is_reset and (action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents):
            raise ValueError("RobotWarehouse.step_into needs the (E, A) int32 discrete actions of the step")
        if (real_obs is None) != (terminated is None):
            raise ValueError("RobotWarehouse.step_into: real_obs and terminated go together")
        real = () if real_obs is None else (ptr(real_obs["agents_view"]), ptr(real_obs["action_mask"]), ptr(terminated))
        launch("env_step", lib().mava_rware_step_real_next if real else lib().mava_rware_step, self.num_envs,
               self.num_agents, self.num_shelves, self.request_queue_size, self.height, self.width, self.sensor_range,
               self.time_limit, int(self.collision_mode == "terminate"), self._highway_rows, self._shelf_home,
               self.seed & 0xFFFFFFFFFFFFFFFF, t & 0xFFFFFFFF, ptr(t_base), off & 0xFFFFFFFF, int(is_reset),
               ptr(state.agent_pos), ptr(state.agent_dir), ptr(state.agent_carry), ptr(state.shelf_pos),
               ptr(state.request_queue), ptr(state.step_count), ptr(state.run_return), ptr(state.run_length),
               ptr(state.ep_return), ptr(state.ep_length), ptr(obs["agents_view"]), ptr(obs["global_state"]),
               ptr(obs["action_mask"]), ptr(obs["step_count"]), ptr(reward), ptr(done), ptr(info_return),
               ptr(info_length), ptr(info_terminal), None if is_reset else ptr(action), *real, stream_ptr())

    # ---- MarlEnv-style batched API (allocating; the learner uses step_into) -----------------
    def _observation(self, obs: Dict[str, torch.Tensor]):
        mask = obs["action_mask"].bool()
        if self.add_global_state:
            gs = obs["global_state"].expand(-1, self.num_agents, -1)
            return ObservationGlobalState(obs["agents_view"], mask, gs, obs["step_count"])
        return Observation(obs["agents_view"], mask, obs["step_count"])

    def reset(self, key: Any = None) -> Tuple[RwareState, TimeStep]:
        state, obs = self.alloc_state(), self.alloc_obs()
        self.step_into(state, 0, obs, is_reset=True)
        E, A, d = self.num_envs, self.num_agents, self.device
        extras = {"episode_metrics": {"episode_return": torch.zeros(E, device=d),
                                      "episode_length": torch.zeros(E, dtype=torch.int32, device=d),
                                      "is_terminal_step": torch.zeros(E, dtype=torch.bool, device=d)}}
        ts = TimeStep(torch.zeros(E, dtype=torch.int8, device=d), torch.zeros((E, A), device=d),
                      torch.ones((E, A), device=d), self._observation(obs), extras)
        return state, ts

    def step(self, state: RwareState, action: torch.Tensor) -> Tuple[RwareState, TimeStep]:
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
    """(train_env, eval_env) of an `env=rware_native` configuration, sized by config.arch.num_envs / num_eval_episodes."""
    head = config.network.get("action_head", None) or {}
    if "ContinuousActionHead" in str(head.get("_target_", "")):
        raise ValueError("RobotWarehouse has discrete actions only: use a DiscreteActionHead")
    if not bool(config.system.add_agent_id) or bool(config.env.implicit_agent_id):
        raise ValueError("RobotWarehouse always prepends the agent one-hot id (add_agent_id=True)")
    tc = config.env.scenario.task_config
    kw = dict(column_height=int(tc.column_height), shelf_rows=int(tc.shelf_rows), shelf_columns=int(tc.shelf_columns),
              num_agents=int(tc.num_agents), sensor_range=int(tc.sensor_range),
              request_queue_size=int(tc.request_queue_size), time_limit=int(config.env.kwargs.get("time_limit", 500)),
              collision_mode=str(config.env.kwargs.get("collision_mode", "terminate")),
              add_global_state=add_global_state, device=device)
    seed = int(config.system.seed)
    train = RobotWarehouse(num_envs=int(config.arch.num_envs), env_offset=env_offset, seed=seed, **kw)
    # the evaluation envs draw from their own Philox key, as the synthetic env's do
    evale = RobotWarehouse(num_envs=int(config.arch.num_eval_episodes), env_offset=env_offset, seed=seed ^ EVAL_KEY_TAG, **kw)
    return train, evale
