"""What the replay-buffer learners (IQLLearner and its QMIX / VDN subclass, SACLearner) share: the constructor's
prologue, the episode-metric buffers, the environment state and step counters, the env / buffer views of their
LearnerStates, and learn().  Buffers, samplers, train steps and LearnerState types stay with each learner.

A subclass sets `name` (its system's name in the refusal texts) and implements
  _refuse(env, config)     its own refusals, before anything is allocated or the device is touched;
  _buffer_sizes(system)    B and cap (and what hangs on them), with their refusals;
  _obs_slot(k), adopt(state), learner_state(), update(n)
  _guard_tensors()         (parameters, observation leaves) for the f16 range guard;
  _train_metrics()         the TRAIN dict of one learn() call.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from . import parallel
from .guards import check_f16_range
from .learner_common import episode_metrics, matmul_ctx, pad32
from .types import ExperimentOutput


class ReplayLearner:
    name = ""

    def __init__(self, env, config, device: Optional[torch.device] = None):
        self.config = config
        s, arch = config.system, config.arch
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.rank, self.world = parallel.rank_world()
        if self.world > 1:
            raise NotImplementedError(f"{self.name} runs on one device (multi-GPU is not implemented)")
        if int(s.update_batch_size) != 1:
            raise NotImplementedError(f"{self.name} supports update_batch_size == 1 only")
        self._refuse(env, config)
        self.E, self.T, self.K = int(arch.num_envs), int(s.rollout_length), int(s.epochs)
        if env.num_envs != self.E:
            raise ValueError(f"env.num_envs={env.num_envs} != arch.num_envs={self.E}")
        self._buffer_sizes(s)
        self.n_upd = int(s.get("num_updates_per_eval", 1))
        self.env = env
        self.A, self.O = env.num_agents, env.obs_dim
        config.system.num_agents = self.A
        self.EA = self.E * self.A
        self.Rpa, self.Rp = pad32(self.EA), pad32(self.B * self.A)  # acting / sampled rows, padded to the 32-row tiles
        self.matmul_mode, self.ctx = matmul_ctx(s)
        d, shape = self.device, (self.n_upd, self.T, self.E)
        self.info_return = torch.zeros(shape, device=d)
        self.info_length = torch.zeros(shape, dtype=torch.int32, device=d)
        self.info_terminal = torch.zeros(shape, dtype=torch.uint8, device=d)
        self.state = env.alloc_state()
        self.cur = 0         # which of the ping-pong observation slots holds the current observation
        self.act_steps = 0   # act steps taken: the Philox counter of the env and of the acting draws
        self.n_added = 0     # what the buffer's head and fill level are computed from
        self.t_train = 0     # train steps taken: the sampler's counter
        self._learn_calls = 0
        self.debug: Optional[Dict[str, List[Any]]] = None  # tests: clones of gradients / draws / indices when set

    def reset_envs(self) -> None:
        self.cur = 0
        self.env.step_into(self.state, 0, self._obs_slot(0), is_reset=True)

    def _info(self, n: int, t: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The (E,) episode-metric slots of act step t of update n."""
        return self.info_return[n, t], self.info_length[n, t], self.info_terminal[n, t]

    # ---------------------------------------------------------------------------- state views
    def env_state(self) -> Dict[str, torch.Tensor]:
        return {"step_count": self.state.step_count, "episode_return": self.state.ep_return,
                "episode_length": self.state.ep_length}

    def buffer_state(self) -> Dict[str, Any]:
        return {"experience": self.buf, "current_index": self.n_added % self.cap, "is_full": self.n_added >= self.cap}

    def learn(self, state) -> ExperimentOutput:
        self.adopt(state)
        if self.matmul_mode == "f16x2":
            params, obs = self._guard_tensors()
            check_f16_range(params, obs, self.train_metrics if self._learn_calls else None, type(self).__name__)
        self._learn_calls += 1
        for n in range(self.n_upd):
            self.update(n)
        ep_metrics = episode_metrics(self.info_return, self.info_length, self.info_terminal)
        train_metrics = self._train_metrics()
        return ExperimentOutput(self.learner_state(), ep_metrics, train_metrics)
