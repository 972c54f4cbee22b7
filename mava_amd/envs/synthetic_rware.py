"""Synthetic RWARE-shaped vectorised environment.

Stands in for `environments.make(config, add_global_state=...)` (mava/utils/make_env.py:215-240):
Jumanji's RobotWarehouse is third-party JAX code that is not available, so observations, masks,
rewards and dones are generated with RWARE's shapes and statistics by mava_synth_rware_step while
the wrapper semantics the learner records (agent ids, global state, auto-reset, episode metrics)
are reproduced.  The object follows the MarlEnv protocol (mava/types.py:34-108) in a natively
BATCHED form: `reset`/`step` act on all `num_envs` environments of one (device, update-batch)
replica at once, and `step_into` writes straight into trajectory slots owned by the learner.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .._lib import check, lib, ptr
from .base import COMMON_STATE, EVAL_KEY_TAG, BatchedEnv, ObsSpec, make_pair  # noqa: F401 (EVAL_KEY_TAG, ObsSpec: public here)

SynthState = NamedTuple("SynthState", COMMON_STATE)


class SyntheticRware(BatchedEnv):
    State = SynthState
    # mava_rollout_ff_f32 (csrc/rollout_h2.hip) carries THIS generator's env phase: the feed-forward learner routes an
    # env to the one-launch rollout only when it declares so (any other MarlEnv steps through step_into per time step)
    supports_fused_rollout = True
    emits_real_next_obs = False
    step_symbol = "mava_synth_rware_step"

    def __init__(self, num_envs: int, num_agents: int, obs_dim: int = 66, num_actions: int = 5, time_limit: int = 500,
                 add_global_state: bool = False, add_agent_id: bool = True, seed: int = 42, env_offset: int = 0,
                 tile_global_state: bool = False, device: Optional[torch.device] = None, state_dim: int = 0,
                 reward_mode: str = "random"):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        if not add_agent_id:
            raise NotImplementedError("the synthetic generator always prepends the agent one-hot id (add_agent_id=True)")
        if reward_mode not in ("random", "match"):
            raise ValueError(f"reward_mode must be 'random' or 'match', got {reward_mode!r}")
        super().__init__(kw)
        self.raw_obs_dim, self.action_dim = int(obs_dim), int(num_actions)
        self.gs_tiles = self.num_agents if tile_global_state else 1
        self.synth_state_dim = int(state_dim)  # 0: global_state = concatenated raw views; > 0: own state vector
        self.global_state_shared = not tile_global_state
        # "random": Bernoulli(0.02) team reward, independent of the actions (the measurement workload of SURVEY 8d);
        # "match": team reward = fraction of agents whose action equals (first grid coordinate they observed) mod
        # n_actions - an action-dependent task, so that runs can show the PPO stack LEARNS (tests/test_gpu_learning.py)
        self.reward_mode = reward_mode
        self.step_tail_args = (int(reward_mode == "match"),)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def obs_dim(self) -> int:
        return self.num_agents + self.raw_obs_dim

    @property
    def state_dim(self) -> int:
        return self.synth_state_dim if self.synth_state_dim > 0 else self.num_agents * self.raw_obs_dim

    def _action_ptr(self, action, is_reset):  # the action is passed only in "match"
        if self.reward_mode != "match":
            return None
        if not is_reset and (action is None or action.dtype != torch.int32 or action.numel() != self.num_envs * self.num_agents):
            raise ValueError("reward_mode='match' needs the (E, A) int32 actions of the step")
        return ptr(action)

    def _call(self, symbol, args):  # a plain check(...): launch() would bracket the step with bench.py's HIP event timers
        check(getattr(lib(), symbol)(*args), symbol)

    def step_args(self, state: SynthState):
        return (self.raw_obs_dim, self.action_dim, self.gs_tiles, self.synth_state_dim, self.time_limit), ()


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """Counterpart of mava/utils/make_env.py:215-240 for the synthetic stand-in: returns
    (train_env, eval_env) sized by config.arch.num_envs / config.arch.num_eval_episodes."""
    tc = config.env.scenario.task_config
    syn = config.env.get("synthetic", {"obs_dim": 66, "num_actions": 5})
    kw = dict(num_agents=int(tc.num_agents), obs_dim=int(syn["obs_dim"]), num_actions=int(syn["num_actions"]),
              time_limit=int(config.env.kwargs.get("time_limit", 500)), add_global_state=add_global_state,
              add_agent_id=bool(config.system.add_agent_id) and not bool(config.env.implicit_agent_id),
              device=device, state_dim=int(syn.get("state_dim", 0) or 0), reward_mode=str(syn.get("reward_mode", "random")))
    train, evale = make_pair(SyntheticRware, config, kw, env_offset, discrete_only=False)
    for e in (train, evale):
        e.obs_shape = tuple(int(v) for v in syn["obs_shape"]) if syn.get("obs_shape", None) else None
        e.state_shape = tuple(int(v) for v in syn["state_shape"]) if syn.get("state_shape", None) else None
    return train, evale
