"""What every batched environment of this package shares (DESIGN.md "Adding an environment").

An environment follows the MarlEnv protocol (mava/types.py:34-108) in a natively BATCHED form: `reset` / `step` act on all
`num_envs` environments of one (device, update-batch) replica at once and allocate; `step_into` - the call the learners
use - writes straight into trajectory slots owned by the learner.  The step kernels share one argument order
(include/mava_hip.h):

    E, A, *scenario, seed, t, t_base, env_offset, is_reset, *own state, step_count, run_return, run_length, ep_return,
    ep_length, agents_view, global_state, action_mask, obs_step_count, reward, done, info_return, info_length,
    info_terminal, [info_won,] action, [*step_tail_args,] [real_view, real_mask, terminated, [*real_extra_keys,]] stream

(the real_* group only where `emits_real_next_obs`, null pointers when the caller passes no `real_obs`), so
`BatchedEnv.step_into` assembles it once.  A subclass states `State`, `action_dim`, `step_symbol`, `obs_dim`, `state_dim`,
`alloc_own_state` and `step_args`, validates its scenario in `__init__` and reads it from the config in its
module's `make`.
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from .._lib import launch, lib, ptr, stream_ptr
from ..types import Observation, ObservationGlobalState, TimeStep

EVAL_KEY_TAG = 0x4556414C4556414C  # "EVALEVAL": xor-ed into the Philox key of the evaluation environments

# the first six fields of every state tuple: the five the learners read, and the allocating API's host-side counter
COMMON_STATE = [
    ("step_count", torch.Tensor),  # (E, A) i32
    ("run_return", torch.Tensor),  # (E,) f32   running_count_episode_return
    ("run_length", torch.Tensor),  # (E,) i32
    ("ep_return", torch.Tensor),  # (E,) f32   episode_return (last finished)
    ("ep_length", torch.Tensor),  # (E,) i32
    ("t", torch.Tensor),  # () i64 host-side step counter of this replica's stream
]


class ObsSpec(NamedTuple):
    agents_view: Tuple[int, ...]
    action_mask: Tuple[int, ...]
    global_state: Optional[Tuple[int, ...]]
    step_count: Tuple[int, ...]


class BatchedEnv:
    gs_tiles = 1  # rows of global_state per env: 1 (shared by the agents) or A (a tiled copy)
    global_state_shared = True  # all agents of an env receive the same global_state row (mava/wrappers/jumanji.py:53-59)
    supports_fused_rollout = False  # True: the feed-forward learner may route the env to the one-launch rollout
    emits_real_next_obs = True  # step_into(real_obs=, terminated=): what rec_iql stores as next_obs / terminal
    implicit_agent_id = False  # True: no one-hot id in agents_view (system.add_agent_id is ignored)
    reports_win = False  # True: the symbol takes info_won after info_terminal, reset / step add extras["won_episode"]
    step_tail_args: tuple = ()  # arguments of the symbol after `action`, before the real_* group
    real_extra_keys: tuple = ()  # keys of real_obs whose pointers follow `terminated` (None if absent)
    State: type  # the state tuple: COMMON_STATE, then the fields of alloc_own_state in its order
    action_dim: int
    step_symbol: str  # mava_X_step

    def __init__(self, ctor_kw: Dict[str, Any]):
        """`ctor_kw`: `dict(locals())` of the subclass constructor, taken as its first statement; `clone` builds from them."""
        kw = {k: v for k, v in ctor_kw.items() if k not in ("self", "__class__")}
        self.num_envs, self.num_agents, self.time_limit = int(kw["num_envs"]), int(kw["num_agents"]), int(kw["time_limit"])
        self.add_global_state = kw["add_global_state"]
        self.seed, self.env_offset = int(kw["seed"]), int(kw["env_offset"])
        dev = kw["device"]
        self.device = kw["device"] = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
        self._ctor_kw = kw
        # image view of the observation / state vectors for CNN torsos: (H, W, C) with H*W*C = obs_dim / state_dim
        self.obs_shape: Optional[tuple] = None
        self.state_shape: Optional[tuple] = None

    def clone(self, env_offset: int, num_envs: Optional[int] = None):
        """Same scenario on a disjoint range of global env ids (one per replica / rank)."""
        c = type(self)(**dict(self._ctor_kw, env_offset=env_offset, num_envs=num_envs or self.num_envs))
        c.obs_shape, c.state_shape = self.obs_shape, self.state_shape
        return c

    # ---- what a subclass states -------------------------------------------------------------
    obs_dim: int
    state_dim: int

    def alloc_own_state(self) -> tuple:
        """The environment's own state tensors, in the order of State's fields after COMMON_STATE."""
        return ()

    def step_args(self, state) -> Tuple[tuple, tuple]:
        """(the scenario arguments between A and seed, the own state pointers between is_reset and step_count)."""
        raise NotImplementedError

    # ---- specs ----------------------------------------------------------------------------
    def observation_spec(self) -> ObsSpec:
        A = self.num_agents
        return ObsSpec((A, self.obs_dim), (A, self.action_dim), (A, self.state_dim) if self.add_global_state else None, (A,))

    def alloc_state(self):
        E, A, d = self.num_envs, self.num_agents, self.device
        i32 = torch.int32
        return self.State(torch.zeros((E, A), dtype=i32, device=d), torch.zeros(E, device=d),
                          torch.zeros(E, dtype=i32, device=d), torch.zeros(E, device=d), torch.zeros(E, dtype=i32, device=d),
                          torch.zeros((), dtype=torch.int64), *self.alloc_own_state())

    def alloc_obs(self) -> Dict[str, torch.Tensor]:
        E, A, d = self.num_envs, self.num_agents, self.device
        return {
            "agents_view": torch.empty((E, A, self.obs_dim), device=d),
            "global_state": torch.empty((E, self.gs_tiles, self.state_dim), device=d),
            "action_mask": torch.empty((E, A, self.action_dim), dtype=torch.uint8, device=d),
            "step_count": torch.empty((E, A), dtype=torch.int32, device=d),
        }

    # ---- kernel call ----------------------------------------------------------------------
    def step_into(self, state, t: int, obs: Dict[str, torch.Tensor], reward=None, done=None, info_return=None,
                  info_length=None, info_terminal=None, is_reset: bool = False, env_offset: Optional[int] = None,
                  t_base: Optional[torch.Tensor] = None, action: Optional[torch.Tensor] = None,
                  real_obs: Optional[Dict[str, torch.Tensor]] = None, terminated: Optional[torch.Tensor] = None,
                  info_won: Optional[torch.Tensor] = None) -> None:
        """One vectorised step (or reset) with the (E, A) int32 `action`, writing the next observation into `obs` and the
        transition into the given (E, A) / (E,) slots.  `t` is the replica's global step index (Philox counter); `t_base`
        (a device int32 word) is added to it on the device, for rollouts replayed from a captured graph.  `real_obs`
        ({"agents_view", "action_mask"}) and `terminated` (E,) u8, given together, receive the pre-reset observation
        (AutoResetWrapper's extras["real_next_obs"]) and the termination flag (a time-limit end alone is a truncation);
        they are not written on a reset.  `info_won` (E,) u8, optional and only where `reports_win`, receives done & won
        (the learners do not pass it)."""
        act = self._action_ptr(action, is_reset)
        if (real_obs is None) != (terminated is None):
            raise ValueError(f"{type(self).__name__}.step_into: real_obs and terminated go together")
        if info_won is not None and not self.reports_win:
            raise ValueError(f"{type(self).__name__}.step_into: this environment reports no win")
        off = self.env_offset if env_offset is None else env_offset
        if not self.emits_real_next_obs:
            if real_obs is not None:
                raise ValueError(f"{type(self).__name__}.step_into: this environment emits no real next observation")
            real = ()
        elif real_obs is None:
            real = (None,) * (3 + len(self.real_extra_keys))
        else:
            real = (ptr(real_obs["agents_view"]), ptr(real_obs["action_mask"]), ptr(terminated),
                    *(ptr(real_obs.get(k, None)) for k in self.real_extra_keys))
        won = (ptr(info_won),) if self.reports_win else ()
        scenario, own = self.step_args(state)
        self._call(self.step_symbol, (
            self.num_envs, self.num_agents, *scenario, self.seed & 0xFFFFFFFFFFFFFFFF, t & 0xFFFFFFFF, ptr(t_base),
            off & 0xFFFFFFFF, int(is_reset), *own, ptr(state.step_count), ptr(state.run_return), ptr(state.run_length),
            ptr(state.ep_return), ptr(state.ep_length), ptr(obs["agents_view"]), ptr(obs["global_state"]),
            ptr(obs["action_mask"]), ptr(obs["step_count"]), ptr(reward), ptr(done), ptr(info_return), ptr(info_length),
            ptr(info_terminal), *won, act, *self.step_tail_args, *real, stream_ptr()))

    def _action_ptr(self, action: Optional[torch.Tensor], is_reset: bool) -> Optional[int]:
        """The `action` argument of the symbol, after checking it: a reset passes none."""
        if is_reset:
            return None
        if action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents:
            raise ValueError(f"{type(self).__name__}.step_into needs the (E, A) int32 discrete actions of the step")
        return ptr(action)

    def _call(self, symbol: str, args: tuple) -> None:
        launch("env_step", getattr(lib(), symbol), *args)

    # ---- MarlEnv-style batched API (allocating; the learner uses step_into) -----------------
    def _observation(self, obs: Dict[str, torch.Tensor]):
        mask = obs["action_mask"].bool()
        if self.add_global_state:
            gs = obs["global_state"]
            gs = gs.expand(-1, self.num_agents, -1) if self.gs_tiles == 1 else gs
            return ObservationGlobalState(obs["agents_view"], mask, gs, obs["step_count"])
        return Observation(obs["agents_view"], mask, obs["step_count"])

    def reset(self, key: Any = None):
        state, obs = self.alloc_state(), self.alloc_obs()
        self.step_into(state, 0, obs, is_reset=True)
        E, A, d = self.num_envs, self.num_agents, self.device
        extras = {"episode_metrics": {"episode_return": torch.zeros(E, device=d),
                                      "episode_length": torch.zeros(E, dtype=torch.int32, device=d),
                                      "is_terminal_step": torch.zeros(E, dtype=torch.bool, device=d)}}
        if self.reports_win:
            extras["won_episode"] = torch.zeros(E, dtype=torch.bool, device=d)
        ts = TimeStep(torch.zeros(E, dtype=torch.int8, device=d), torch.zeros((E, A), device=d),
                      torch.ones((E, A), device=d), self._observation(obs), extras)
        return state, ts

    def step(self, state, action: torch.Tensor):
        E, A, d = self.num_envs, self.num_agents, self.device
        obs = self.alloc_obs()
        reward = torch.empty((E, A), device=d)
        done = torch.empty((E, A), dtype=torch.uint8, device=d)
        ir = torch.empty(E, device=d)
        il = torch.empty(E, dtype=torch.int32, device=d)
        it = torch.empty(E, dtype=torch.uint8, device=d)
        won = torch.empty(E, dtype=torch.uint8, device=d) if self.reports_win else None
        t = int(state.t) + 1
        self.step_into(state, t, obs, reward, done, ir, il, it, info_won=won, action=action.to(torch.int32).contiguous())
        state = state._replace(t=torch.tensor(t, dtype=torch.int64))
        last = it.bool()
        extras = {"episode_metrics": {"episode_return": ir, "episode_length": il, "is_terminal_step": last}}
        if self.reports_win:
            extras["won_episode"] = won.bool()
        step_type = torch.where(last, 2, 1).to(torch.int8)
        ts = TimeStep(step_type, reward, 1.0 - done.float(), self._observation(obs), extras)
        return state, ts


def make_pair(cls, config, kw: Dict[str, Any], env_offset: int, discrete_only: bool = True):
    """The tail of every module's `make`: (train_env, eval_env) of class `cls` with the scenario keywords `kw`, sized by
    config.arch.num_envs / num_eval_episodes.  The evaluation envs draw from their own Philox KEY (not an env-id offset:
    the kernels form per-agent counters from (env_offset + e) * A + agent in 32 bits, where an offset of 2^30 wraps back
    onto the training envs for A >= 4)."""
    head = config.network.get("action_head", None) or {}
    if discrete_only and "ContinuousActionHead" in str(head.get("_target_", "")):
        raise ValueError(f"{cls.__name__} has discrete actions only: use a DiscreteActionHead")
    seed = int(config.system.seed)
    train = cls(num_envs=int(config.arch.num_envs), env_offset=env_offset, seed=seed, **kw)
    evale = cls(num_envs=int(config.arch.num_eval_episodes), env_offset=env_offset, seed=seed ^ EVAL_KEY_TAG, **kw)
    return train, evale
