"""What the on-policy learners (FFLearner, RecLearner, MATLearner) share: the trajectory replica, the constructor's
prologue, the flat parameter / Adam storage over network segments (init_params, state trees, adopt), the slot-0
observation views of their LearnerStates, the clip+Adam launch with its hyper-parameter block, learn() and
learner_setup().  Networks, rollouts, gradient launches and learner_state() stay with each learner.

A subclass implements
  _refuse(env, config)           its own refusals, before anything is allocated or the device is touched;
  _rollout(n), _bootstrap_and_gae(), _minibatch(n, k, mb, perm), learner_state()
and calls _alloc_params([(network, lr), ...]) once its networks exist.  It may override
  perm_rows                      length of an epoch's permutation (default T * E);
  _params_tree(), _opt_tree(), _state_segments(state)   how the segments are packed (default: actor / critic);
  _adopted()                     runs after adopt() really copied a foreign tree;
  reset_envs()                   to reset what else it carries between rollouts;
  _carry_observation()           slot T -> slot 0 (default: four copies per replica);
  update(n, permutations)        (default: rollout, bootstrap + GAE, K permutations x M minibatches, carry).
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops, parallel
from .guards import check_f16_range
from .learner_common import bind_learn, matmul_ctx
from .networks import make_action_head
from .types import AdamState, ExperimentOutput, Observation, ObservationGlobalState, OptStates, Params
from .utils.tree import tree_to

NUM_CU = 256  # MI355X compute units: one persistent gradient block per CU


class _Replica:
    """Trajectory + env buffers of one update-batch replica (the vmapped axis of ff_mappo.py:319)."""

    def __init__(self, env, T: int, n_upd: int, device, continuous: bool = False):
        E, A = env.num_envs, env.num_agents
        self.env = env
        self.state = env.alloc_state()
        d = device
        self.agents_view = torch.empty((T + 1, E, A, env.obs_dim), device=d)
        self.global_state = torch.empty((T + 1, E, env.gs_tiles, env.state_dim), device=d)
        self.action_mask = torch.empty((T + 1, E, A, env.action_dim), dtype=torch.uint8, device=d)
        self.step_count = torch.empty((T + 1, E, A), dtype=torch.int32, device=d)
        # discrete: action index per agent; continuous head: action vector in (-1, 1) per agent
        self.action = (torch.empty((T, E, A, env.action_dim), device=d) if continuous
                       else torch.empty((T, E, A), dtype=torch.int32, device=d))
        self.value = torch.empty((T, E, A), device=d)
        self.reward = torch.empty((T, E, A), device=d)
        self.log_prob = torch.empty((T, E, A), device=d)
        self.done = torch.empty((T, E, A), dtype=torch.uint8, device=d)
        self.last_val = torch.empty((E, A), device=d)
        self.adv = torch.empty((T, E, A), device=d)
        self.tgt = torch.empty((T, E, A), device=d)
        # episode metrics of every update of one learn() call: (N_upd, T, E)
        self.info_return = torch.zeros((n_upd, T, E), device=d)
        self.info_length = torch.zeros((n_upd, T, E), dtype=torch.int32, device=d)
        self.info_terminal = torch.zeros((n_upd, T, E), dtype=torch.uint8, device=d)
        # the rollout writes the metrics of the CURRENT update here (fixed addresses: one captured HIP graph serves
        # every update index n); FFLearner._rollout copies them to slot n afterwards
        self.cur_return = torch.zeros((T, E), device=d)
        self.cur_length = torch.zeros((T, E), dtype=torch.int32, device=d)
        self.cur_terminal = torch.zeros((T, E), dtype=torch.uint8, device=d)
        self.last_reward = torch.zeros((E, A), device=d)
        self.last_done = torch.zeros((E, A), dtype=torch.uint8, device=d)

    def obs_slot(self, t: int) -> Dict[str, torch.Tensor]:
        return {"agents_view": self.agents_view[t], "global_state": self.global_state[t],
                "action_mask": self.action_mask[t], "step_count": self.step_count[t]}

    # the buffers themselves, for code that touches slots 0 and T only or hands the kernels a pointer (see LeanReplica)
    @property
    def av_raw(self) -> torch.Tensor:
        return self.agents_view

    @property
    def gs_raw(self) -> torch.Tensor:
        return self.global_state


class LeanReplica(_Replica):
    """The replica of a learner whose fused rollout may leave slots 1 .. T - 1 of the f32 agents_view / global_state
    unwritten, their f16 records holding the same values (FFLearner._rollout_fused).  `agents_view` and `global_state`
    are properties: a read while the array's inner slots are stale first rebuilds them from the record (one forced
    ops.rollout_expand launch on the current stream) and then returns the same tensor object as ever.  The update's own
    code takes av_raw / gs_raw: it reads slots 0 and T, which are always written, and passes pointers."""

    def __init__(self, *args, **kwargs):
        self.stale_av = self.stale_gs = False  # slots 1 .. T - 1 of the f32 array were skipped by the last rollout
        self.state16 = self.state16_valid = self.view16 = self.view16_valid = None
        super().__init__(*args, **kwargs)

    def materialise(self, av: bool = True, gs: bool = True) -> None:
        av, gs = av and self.stale_av, gs and self.stale_gs
        if av or gs:
            ops.rollout_expand(self.av_raw if av else None, self.view16 if av else None, self.view16_valid if av else None,
                               self.gs_raw if gs else None, self.state16 if gs else None, self.state16_valid if gs else None,
                               force=True)
            self.stale_av, self.stale_gs = self.stale_av and not av, self.stale_gs and not gs

    av_raw = gs_raw = None  # (plain attributes here: the buffers live under these names)

    @property
    def agents_view(self) -> torch.Tensor:
        self.materialise(gs=False)
        return self.av_raw

    @agents_view.setter
    def agents_view(self, t: torch.Tensor) -> None:
        self.av_raw = t

    @property
    def global_state(self) -> torch.Tensor:
        self.materialise(av=False)
        return self.gs_raw

    @global_state.setter
    def global_state(self, t: torch.Tensor) -> None:
        self.gs_raw = t


class PPOLearner:
    def __init__(self, env, config, centralised_critic: bool, device: Optional[torch.device] = None, *, replica=_Replica,
                 replica_kwargs: Optional[Dict[str, Any]] = None, ctx_kwargs: Optional[Dict[str, Any]] = None):
        self.config = config
        self.centralised = centralised_critic
        self.rank, self.world = parallel.rank_world()
        s, arch = config.system, config.arch
        self.E, self.U, self.T = int(arch.num_envs), int(s.update_batch_size), int(s.rollout_length)
        self.K, self.M = int(s.ppo_epochs), int(s.num_minibatches)
        self._refuse(env, config)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_upd = int(s.get("num_updates_per_eval", 1))
        if env.num_envs != self.E:
            raise ValueError(f"env.num_envs={env.num_envs} != arch.num_envs={self.E}")
        if centralised_critic and not getattr(env, "add_global_state", False):
            raise ValueError("Global state must be provided to the centralised critic.")  # networks.py:196-197, :315-316
        # Arithmetic of the matrix products (not a Mava key): "f16x2" (default) = every operand split into two f16 terms,
        # "f32" = the exact-f32 MFMA kernels everywhere (learner_common.matmul_ctx).  The library keeps no process-wide
        # settings: the mode and the kernels' own workspaces belong to this learner's context handle (mava_ctx_*).
        self.matmul_mode, self.ctx = matmul_ctx(s, **(ctx_kwargs or {}))
        # ff_mappo.py:348-350: the action head of the configuration, sized by the env's action dimension
        self.action_head = make_action_head(config.network.get("action_head", None), env.action_dim)
        self.continuous = type(self.action_head).__name__ == "ContinuousActionHead"
        self.min_scale = float(getattr(self.action_head, "min_scale", 1e-3))
        # a discrete env reads the action index; of the continuous ones only an env with `continuous_actions` reads the
        # f32 action vector (the synthetic stand-in ignores it)
        self._env_reads_action = not self.continuous or getattr(env, "continuous_actions", False)
        # one env object per replica; global env ids are disjoint over (rank, replica)
        self.reps: List[Any] = []
        for u in range(self.U):
            rep_env = env.clone(env_offset=getattr(env, "env_offset", 0) + (self.rank * self.U + u) * self.E)
            self.reps.append(replica(rep_env, self.T, self.n_upd, self.device, continuous=self.continuous, **(replica_kwargs or {})))
        env0 = self.reps[0].env
        self.A, self.nA = env0.num_agents, env0.action_dim
        config.system.num_agents = self.A  # ff_mappo.py:341
        self.Oa = env0.obs_dim
        if centralised_critic:
            self.Oc = env0.state_dim
            self.critic_share = self.A if env0.global_state_shared else 1
        else:
            self.Oc, self.critic_share = self.Oa, 1
        # The gradient kernels are persistent blocks that own a CU each (all of its registers and LDS): with several ranks
        # a few CUs stay free of them, so that RCCL's all-reduce kernel can really run WHILE they do (_slab_count);
        # system.rccl_cus / MAVA_RCCL_CUS, default 8 with a process group (a ~0.3 MB message uses a handful of channels),
        # 0 on a single rank.
        self.rccl_cus = int(s.get("rccl_cus", None) if s.get("rccl_cus", None) is not None
                            else os.environ.get("MAVA_RCCL_CUS", "8" if self.world > 1 else "0"))
        d = self.device
        self.stats = torch.zeros((ops.lib().mava_adv_stats_blocks(), 2), dtype=torch.float64, device=d)
        self.train_metrics = torch.zeros((self.n_upd, self.K, self.M, 4), device=d)
        self.perm_rows = self.T * self.E
        self.perm_count = 0  # epoch permutations drawn so far (counter of mava_permutation_i32)
        self.t_global = 0  # env steps taken per env so far (Philox step counter)
        self.ent_step = 0  # minibatches trained so far: counter of the continuous head's entropy sample
        self.seed = int(s.seed)
        self.timers: Optional[Dict[str, list]] = None  # bench.py (FFLearner._timed): name -> [(start_event, end_event)]
        self._learn_calls = 0  # guards.check_f16_range: the previous call's metrics are checked from the second call on

    def _refuse(self, env, config) -> None:
        pass

    def _slab_count(self, ntiles: int) -> int:
        """Gradient slabs (= persistent blocks) for `ntiles` 32-row tiles: one per CU that RCCL does not keep."""
        return max(1, min(NUM_CU - max(0, min(self.rccl_cus, NUM_CU - 1)), ntiles))

    # ------------------------------------------------------------------- flat parameter storage
    def _alloc_params(self, nets: Sequence[Tuple[Any, float]]) -> None:
        """Flat f32 params / grads / Adam moments over the networks' segments ([actor | critic], or MAT's one), the
        4 loss scalars after the grads (actor_loss, entropy, value_loss, pad), and each segment's learning rate."""
        self.seg_off = [0]
        for net, _ in nets:
            self.seg_off.append(self.seg_off[-1] + net.num_params)
        self.segments = [(net, slice(lo, hi)) for (net, _), lo, hi in zip(nets, self.seg_off, self.seg_off[1:])]
        self.seg_lr = [float(lr) for _, lr in nets]
        self.P = self.seg_off[-1]
        d = self.device
        self.p, self.m, self.v = (torch.zeros(self.P, device=d) for _ in range(3))
        self.g = torch.zeros(self.P + 4, device=d)
        self.count = torch.zeros(2, dtype=torch.int32, device=d)  # (one Adam count per segment; MAT's one segment uses word 0)

    def init_params(self, *seeds: int) -> None:
        for (net, sl), seed in zip(self.segments, seeds):
            self.p[sl].copy_(net.init_flat(seed))
        self.m.zero_()
        self.v.zero_()
        self.count.zero_()

    def reset_envs(self) -> None:
        for rep in self.reps:
            rep.env.step_into(rep.state, 0, rep.obs_slot(0), is_reset=True)
        self.t_global = self.ent_step = self.perm_count = 0

    def _trees(self, flat: torch.Tensor) -> List[Any]:
        return [net.tree(flat[sl], (1, self.U)) for net, sl in self.segments]

    def _adam_states(self) -> List[AdamState]:
        return [AdamState(self.count[i].expand(1, self.U), mu, nu)
                for i, (mu, nu) in enumerate(zip(self._trees(self.m), self._trees(self.v)))]

    def _params_tree(self):
        return Params(*self._trees(self.p))

    def _opt_tree(self):
        return OptStates(*self._adam_states())

    def _state_segments(self, state) -> List[Tuple[Any, AdamState]]:
        """(parameter tree, AdamState) of `state` per segment."""
        return [(state.params.actor_params, state.opt_states.actor_opt_state),
                (state.params.critic_params, state.opt_states.critic_opt_state)]

    def adopt(self, state) -> None:
        """Make the parameter / optimiser buffers equal to `state` (no-op for trees that already alias them), so that
        learn() is a function of its argument like the reference's pure learner_fn - e.g. params restored from a
        checkpoint (rec_mappo.py:558-566).  Environment (and hidden) state stay with the learner."""
        trees = self._state_segments(state)
        leaf = self.segments[0][0].first_leaf(trees[0][0])
        if isinstance(leaf, torch.Tensor) and leaf.data_ptr() == self.p.data_ptr():
            return
        to = lambda tree: tree_to(tree, self.p.device)
        for i, ((net, sl), (params, opt)) in enumerate(zip(self.segments, trees)):
            net.flat_from_tree(to(params), self.p[sl])
            net.flat_from_tree(to(opt.mu), self.m[sl])
            net.flat_from_tree(to(opt.nu), self.v[sl])
            self.count[i] = int(torch.as_tensor(opt.count).reshape(-1)[0])
        self._adopted()

    def _adopted(self) -> None:
        pass

    # ---------------------------------------------------------------------------- state views
    def _stack(self, f) -> torch.Tensor:
        """f(replica) of every replica as one (1, U, ...) leaf."""
        return torch.stack([f(r) for r in self.reps], 0).unsqueeze(0)

    def _observation(self, slot: int = 0):
        av = self._stack(lambda r: r.av_raw[slot])  # (slot 0 or T: see LeanReplica)
        mask = self._stack(lambda r: r.action_mask[slot]).bool()
        sc = self._stack(lambda r: r.step_count[slot])
        if not self.centralised:
            return Observation(av, mask, sc)
        gs = self._stack(lambda r: r.gs_raw[slot].expand(-1, self.A, -1) if r.env.gs_tiles == 1 else r.gs_raw[slot])
        return ObservationGlobalState(av, mask, gs, sc)

    def _key(self) -> torch.Tensor:
        return torch.tensor([[[self.seed, self.t_global]] * self.U], dtype=torch.int64)  # (1, U, 2) host tensor

    def _env_state(self) -> Dict[str, torch.Tensor]:
        return {"step_count": self._stack(lambda r: r.state.step_count), "episode_return": self._stack(lambda r: r.state.ep_return),
                "episode_length": self._stack(lambda r: r.state.ep_length)}

    # ------------------------------------------------------------------------------------ update
    def _adam_kwargs(self, n: int, k: int, mb: int) -> Dict[str, Any]:
        """The hyper-parameter block of ops.clip_adam / ops.ppo_finish for minibatch (k, mb) of update n; grad_scale turns
        the gradient summed over replicas and ranks into their mean (ff_mappo.py:228-238)."""
        s = self.config.system
        return dict(grad_scale=1.0 / (self.U * self.world), max_norm=float(s.max_grad_norm), decay=bool(s.decay_learning_rates),
                    steps_per_update=self.K * self.M, num_updates=int(s.get("num_updates", 1) or 1), vf_coef=float(s.vf_coef),
                    ent_coef=float(s.ent_coef), metrics_out=self.train_metrics[n, k, mb])

    def _clip_adam(self, n: int, k: int, mb: int) -> None:
        ops.clip_adam(self.p, self.g, self.m, self.v, self.count, self.seg_off, self.seg_lr, loss_sums=self.g[self.P :],
                      **self._adam_kwargs(n, k, mb))

    def _epoch(self, n: int, k: int, perm) -> None:
        """The M minibatches of epoch k.  ent_step counts them for the continuous head's entropy draw; the kernels of a
        discrete head (closed-form entropy) never read it, so advancing it there is harmless."""
        for mb in range(self.M):
            self._minibatch(n, k, mb, perm)
            self.ent_step += 1

    def _carry_observation(self) -> None:
        """The bootstrap observation (slot T) becomes the first observation of the next rollout."""
        for rep in self.reps:
            for buf in (rep.agents_view, rep.global_state, rep.action_mask, rep.step_count):
                buf[0].copy_(buf[self.T])

    def update(self, n: int, permutations: Optional[List[torch.Tensor]] = None) -> None:
        self._rollout(n)
        self._bootstrap_and_gae()
        for k in range(self.K):
            if permutations is not None:
                perm = permutations[k]
            else:  # one permutation of perm_rows rows per epoch (ff_mappo.py:272-273, rec_mappo.py:277-279)
                perm = ops.permutation(self.perm_rows, self.seed, self.perm_count)
                self.perm_count += 1
            self._epoch(n, k, perm)
        self._carry_observation()

    def _guard_tensors(self) -> Tuple[torch.Tensor, List[Optional[torch.Tensor]]]:
        """(parameters, observation leaves) for the f16 range guard."""
        return self.p, [t for r in self.reps for t in (r.av_raw[0], r.gs_raw[0] if self.centralised else None)]

    def learn(self, learner_state) -> ExperimentOutput:
        """LearnerFn (mava/types.py:154): num_updates_per_eval updates, asynchronous on the current
        stream - the caller synchronises before reading the clock (ff_mappo.py:497-498)."""
        self.adopt(learner_state)
        if self.matmul_mode == "f16x2":
            params, obs = self._guard_tensors()
            check_f16_range(params, obs, self.train_metrics if self._learn_calls else None, type(self).__name__)
        self._learn_calls += 1
        for n in range(self.n_upd):
            self.update(n)
        episode_metrics = {
            "episode_return": torch.stack([r.info_return for r in self.reps], 1).unsqueeze(0),  # (1,N,U,T,E)
            "episode_length": torch.stack([r.info_length for r in self.reps], 1).unsqueeze(0),
            "is_terminal_step": torch.stack([r.info_terminal for r in self.reps], 1).unsqueeze(0).bool(),
        }
        tm = self.train_metrics.unsqueeze(1).expand(self.n_upd, self.U, self.K, self.M, 4).unsqueeze(0)  # (1,N,U,K,M,4)
        train_metrics = {"total_loss": tm[..., 0], "value_loss": tm[..., 1], "actor_loss": tm[..., 2], "entropy": tm[..., 3]}
        return ExperimentOutput(self.learner_state(), episode_metrics, train_metrics)


def learner_setup(cls, env, keys, config, *cls_args, device=None):
    """Counterpart of learner_setup (ff_mappo.py:333-432, rec_mappo.py:437-576): (learn, actor_network, initial learner
    state).  `keys` = (key, one network seed per parameter segment, ...) integer seeds."""
    key, *net_keys = (int(k) for k in keys)
    learner = cls(env, config, *cls_args, device)
    learner.seed = key
    learner.init_params(*net_keys[: len(learner.segments)])
    parallel.broadcast_(learner.p, src=0)
    learner.reset_envs()
    return bind_learn(learner), learner.actor_network, learner.learner_state()
