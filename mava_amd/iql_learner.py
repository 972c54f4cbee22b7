"""Recurrent independent Q-learning (rec_iql) behind Mava's learner contract.

Reference: mava/systems/q_learning/rec_iql.py:62-212 (init), :215-530 (make_update_fns).  One update = `rollout_length`
epsilon-greedy acting steps that store Transitions in a device replay buffer (:279-322), then `epochs` train steps
(:413-463): sample windows of sample_sequence_length + 1 steps, three recurrent passes from a zero hidden state (online
Q on obs, online and target Q on next_obs), the double-Q TD loss, clip + Adam, then the target update.

Kernels per act step: mava_rec_q_step_f32 (the whole Q network + epsilon-greedy), the env's step with real_view / real_mask
/ terminated (its pre-reset observation), mava_replay_add_f32.  Per train step: mava_replay_sample_f32, three forward_sequence chains
(mava_amd/rec_networks.py; the padded sample batch is Rp single-agent "envs", identity idx), mava_q_td_loss_f32, the
backward_sequence chain, mava_clip_adam and mava_target_update_f32.  The epsilon schedule, the buffer head and fill
level and the train gate are host arithmetic on step counts: nothing synchronises the host per step or per epoch.

Deviation (documented in DESIGN.md): the reference samples without `can_sample`; here an update only trains once every
env row holds max(min_buffer_size, sample_sequence_length + 1) steps, and t_train does not advance before that.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from ._lib import launch, lib, ptr, stream_ptr
from .ppo_learner import NUM_CU
from .learner_common import bind_learn
from .networks import MLPTorso
from .replay_learner import ReplayLearner
from .rec_networks import H, RecQNetwork, RecWorkspace, t32_to_rows
from .systems.q_learning.types import LearnerState, QNetParams, Transition
from .types import AdamState, Observation
from .utils.tree import tree_to


def _default_torso(c) -> bool:
    c = dict(c or {})
    return (list(c.get("layer_sizes", [128])) == [128] and c.get("activation", "relu") == "relu"
            and not c.get("use_layer_norm", False) and str(c.get("_target_", "MLPTorso")).endswith("MLPTorso"))


def epsilon(t: int, eps_min: float, eps_decay: float) -> float:
    """rec_iql.py:263-265 with t the act steps taken before this one (num_envs per step)."""
    return max(float(eps_min), 1.0 - (float(t) / float(eps_decay)) * (1.0 - float(eps_min)))


class IQLLearner(ReplayLearner):
    name = "rec_iql"

    def _refuse(self, env, config) -> None:
        net = config.network
        if int(net.get("hidden_state_dim", 128)) != H:
            raise ValueError(f"rec_iql needs network.hidden_state_dim == {H} (the fused acting step and the scans)")
        qn = net.get("q_network", None)
        if qn is None or not (_default_torso(qn.get("pre_torso")) and _default_torso(qn.get("post_torso"))):
            raise NotImplementedError("rec_iql runs network/rnn.yaml's q_network torsos only (MLPTorso [128] relu)")
        if not getattr(env, "emits_real_next_obs", False):
            raise ValueError(f"rec_iql needs an environment that returns its pre-reset observation (env=lbf); "
                             f"{type(env).__name__} does not")

    def _buffer_sizes(self, s) -> None:
        self.B, self.L = int(s.sample_batch_size), int(s.sample_sequence_length)
        self.S = self.L + 1  # rec_iql.py:167: sample_sequence_length + 1 consecutive steps
        self.cap = int(s.buffer_size)
        if self.cap < self.S:
            raise ValueError(f"buffer_size={self.cap} cannot hold a window of sample_sequence_length + 1 = {self.S} steps")
        self.min_fill = max(int(s.min_buffer_size), self.S)

    def __init__(self, env, config, device: Optional[torch.device] = None):
        super().__init__(env, config, device)  # the shared refusals, then the two hooks above, then the scaffolding
        s, qn = config.system, config.network.get("q_network", None)
        self.nA = env.action_dim
        E, A, O, nA = self.E, self.A, self.O, self.nA
        cfg = lambda c: {k: v for k, v in dict(c).items() if k != "_target_"}
        self.q_network = RecQNetwork(MLPTorso(**cfg(qn["pre_torso"])), MLPTorso(**cfg(qn["post_torso"])), nA, O)
        self.q_network.ctx = self.ctx
        P = self.P = self.Pq = self.q_network.num_params  # (a subclass appends its own parameters after the first Pq)
        d = self.device
        # online / target parameters, Adam moments (optax.chain(clip_by_global_norm, adam(q_lr, eps=1e-5)), :136-140)
        self.p, self.pt = torch.zeros(P, device=d), torch.zeros(P, device=d)
        self.m, self.v = torch.zeros(P, device=d), torch.zeros(P, device=d)
        self.count = torch.zeros(1, dtype=torch.int32, device=d)
        self.g = torch.zeros(P, device=d)
        # ---- acting: ping-pong current / next observation and flags (rows padded with zeros), T32 hidden states
        u8 = torch.uint8
        self.view = [torch.zeros((self.Rpa, O), device=d) for _ in range(2)]
        self.mask = [torch.zeros((self.Rpa, nA), dtype=u8, device=d) for _ in range(2)]
        self.tot = [torch.zeros(self.Rpa, dtype=u8, device=d) for _ in range(2)]  # term_or_trunc entering the step
        self.term = [torch.zeros(E, dtype=u8, device=d) for _ in range(2)]        # terminal of the step that produced obs
        self.h = [torch.zeros(self.Rpa * H, device=d) for _ in range(2)]
        self.action = torch.zeros(self.Rpa, dtype=torch.int32, device=d)
        self.reward = torch.zeros((E, A), device=d)
        self.real_view = torch.zeros((E, A, O), device=d)
        self.real_mask = torch.zeros((E, A, nA), dtype=u8, device=d)
        self.gs = torch.empty((E, 1, env.state_dim), device=d)
        self.sc = [torch.zeros((E, A), dtype=torch.int32, device=d) for _ in range(2)]
        # ---- replay buffer: every field (E, capacity, A, ...), allocated once (size)
        cap = self.cap
        self.buf = Transition(obs=(torch.zeros((E, cap, A, O), device=d), torch.zeros((E, cap, A, nA), dtype=u8, device=d)),
                              action=torch.zeros((E, cap, A), dtype=torch.int32, device=d),
                              reward=torch.zeros((E, cap, A), device=d),
                              terminal=torch.zeros((E, cap, A), dtype=u8, device=d),
                              term_or_trunc=torch.zeros((E, cap, A), dtype=u8, device=d),
                              next_obs=(torch.zeros((E, cap, A, O), device=d), torch.zeros((E, cap, A, nA), dtype=u8, device=d)))
        # ---- one sampled batch, time-major (S, Rp, ...)
        S, Rp = self.S, self.Rp
        self.smp = Transition(obs=(torch.zeros((S, Rp, O), device=d), torch.zeros((S, Rp, nA), dtype=u8, device=d)),
                              action=torch.zeros((S, Rp), dtype=torch.int32, device=d), reward=torch.zeros((S, Rp), device=d),
                              terminal=torch.zeros((S, Rp), dtype=u8, device=d),
                              term_or_trunc=torch.zeros((S, Rp), dtype=u8, device=d),
                              next_obs=(torch.zeros((S, Rp, O), device=d), torch.zeros((S, Rp, nA), dtype=u8, device=d)))
        self.pairs = torch.zeros((self.B, 2), dtype=torch.int32, device=d)
        # ---- training workspaces: the online pass keeps its activations for the backward pass (ws); the two next-obs
        # passes run inference-only in ws_next, the target pass writing its Q-values to q_target
        rows = self.L * Rp
        self.ws = RecWorkspace(rows, nA, d, training=True, din_max=O)
        self.ws_next = RecWorkspace(rows, nA, d, training=False)
        self.q_target = torch.zeros(rows * nA, device=d)
        self.h0 = torch.zeros(Rp * H, device=d)
        n_slab = max(1, min(NUM_CU, rows // 32))
        self.slabs = torch.zeros((n_slab, H * 3 * H + 3 * H + 8), device=d)
        self.loss_blocks = max(1, min(256, -(-rows // 256)))
        self.partials = torch.zeros((self.loss_blocks, 3), device=d)
        self.train_metrics = torch.zeros((self.n_upd, self.K, 3), device=d)
        self.trained = [False] * self.n_upd
        # the backward chain runs in units of a power of two near the row count (f16 range, as in RecLearner)
        self.grad_scale = float(2 ** math.ceil(math.log2(rows)))
        self.seed = int(s.seed)
        self.gamma, self.tau = float(s.gamma), float(s.tau)
        self.hard_update, self.update_period = bool(s.hard_update), int(s.update_period)
        self.q_lr, self.max_grad_norm = float(s.q_lr), float(s.max_grad_norm)
        self.eps_min, self.eps_decay = float(s.eps_min), float(s.eps_decay)
        # env steps taken (num_envs per act step): the epsilon schedule's t.  Of the base's counters, n_added counts the
        # steps stored per env row and t_train is optax.periodic_update's step too; debug takes {"grads", "pairs", "actions"}
        self.t_act = 0

    # ------------------------------------------------------------------------------------ setup
    def init_params(self, q_seed: int) -> None:
        """rec_iql.py:130-131: online and target from the same key, so the target starts as a copy."""
        self.p.copy_(self.q_network.init_flat(q_seed))
        self.pt.copy_(self.p)
        self.m.zero_()
        self.v.zero_()
        self.count.zero_()

    def _obs_slot(self, k: int) -> Dict[str, torch.Tensor]:
        E, A = self.E, self.A
        return {"agents_view": self.view[k][: self.EA].view(E, A, self.O), "global_state": self.gs,
                "action_mask": self.mask[k][: self.EA].view(E, A, self.nA), "step_count": self.sc[k]}

    def reset_envs(self) -> None:
        """rec_iql.py:178-190: first observation, terminal / term_or_trunc False, zero hidden state."""
        super().reset_envs()
        for t in self.tot + self.term + self.h:
            t.zero_()

    @property
    def epsilon(self) -> float:
        return epsilon(self.t_act, self.eps_min, self.eps_decay)

    # ------------------------------------------------------------------------------------ update
    def _act_step(self, n: int, t: int) -> None:
        """rec_iql.py:279-322: epsilon-greedy action, env step, buffer add."""
        L_, s = lib(), stream_ptr()
        E, A, EA = self.E, self.A, self.EA
        c, nx = self.cur, 1 - self.cur
        launch("rec_q_step", L_.mava_rec_q_step_f32, ptr(self.p), self.O, self.nA, ptr(self.view[c]), ptr(self.mask[c]),
               ptr(self.tot[c]), ptr(self.h[0]), ptr(self.h[1]), self.Rpa, self.epsilon, self.seed & (2**64 - 1),
               self.act_steps & 0xFFFFFFFF, 0, ptr(self.action), None, s)
        self.h.reverse()
        act = self.action[:EA].view(E, A)
        if self.debug is not None:
            self.debug["actions"].append(act.clone())
        self.env.step_into(self.state, self.act_steps + 1, self._obs_slot(nx), self.reward, self.tot[nx][:EA].view(E, A),
                           *self._info(n, t), action=act, real_obs={"agents_view": self.real_view, "action_mask": self.real_mask},
                           terminated=self.term[nx])
        b = self.buf
        launch("replay_add", L_.mava_replay_add_f32, E, A, self.O, self.nA, self.cap, self.n_added % self.cap,
               ptr(self.view[c]), ptr(self.mask[c]), ptr(self.action), ptr(self.reward), ptr(self.term[c]), ptr(self.tot[c]),
               ptr(self.real_view), ptr(self.real_mask), ptr(b.obs[0]), ptr(b.obs[1]), ptr(b.action), ptr(b.reward),
               ptr(b.terminal), ptr(b.term_or_trunc), ptr(b.next_obs[0]), ptr(b.next_obs[1]), s)
        self.cur = nx
        self.n_added += 1
        self.t_act += E
        self.act_steps += 1

    def _sample_batch(self) -> None:
        """rec_iql.py:325-340: B windows of S consecutive steps into `smp`, time-major."""
        b, sm = self.buf, self.smp
        launch("replay_sample", lib().mava_replay_sample_f32, self.E, self.A, self.O, self.nA, self.cap, self.n_added, self.B,
               self.S, self.Rp, self.seed & (2**64 - 1), self.t_train & 0xFFFFFFFF, ptr(b.obs[0]), ptr(b.obs[1]), ptr(b.action),
               ptr(b.reward), ptr(b.terminal), ptr(b.term_or_trunc), ptr(b.next_obs[0]), ptr(b.next_obs[1]), ptr(sm.obs[0]),
               ptr(sm.obs[1]), ptr(sm.action), ptr(sm.reward), ptr(sm.terminal), ptr(sm.term_or_trunc), ptr(sm.next_obs[0]),
               ptr(sm.next_obs[1]), ptr(self.pairs), stream_ptr())
        if self.debug is not None:
            self.debug["pairs"].append(self.pairs.clone())

    def _q_passes(self, pq: torch.Tensor, pqt: torch.Tensor):
        """The three recurrent passes from a zero hidden state: online Q on obs (kept for the backward pass), online and
        target Q on next_obs (the target's into q_target).  data_first = [:, :-1], data_next = [:, 1:] (:375-388); the
        padded batch is Rp single-agent envs, identity idx."""
        Lq, Rp, net, sm = self.L, self.Rp, self.q_network, self.smp
        obs, next_obs = sm.obs[0], sm.next_obs[0]
        tot_first, tot_next = sm.term_or_trunc[:Lq], sm.term_or_trunc[1:]
        q = net.forward_sequence(pq, self.ws, obs, 1, tot_first, self.h0, True, None, Lq, Rp, Rp, 1, training=True)
        qn = net.forward_sequence(pq, self.ws_next, next_obs, 1, tot_next, self.h0, True, None, Lq, Rp, Rp, 1, training=False)
        net.forward_sequence(pqt, self.ws_next, next_obs, 1, tot_next, self.h0, True, None, Lq, Rp, Rp, 1, training=False,
                             y_out=self.q_target)
        return q, qn

    def _loss(self, n: int, k: int, q: torch.Tensor, qn: torch.Tensor) -> None:
        """The double-Q TD loss per agent (:390-411): dLoss/dQ into ws.dy, the metrics into train_metrics[n, k]."""
        sm = self.smp
        launch("q_td_loss", lib().mava_q_td_loss_f32, self.L, self.Rp, self.nA, self.B * self.A, ptr(q), ptr(qn),
               ptr(self.q_target), ptr(sm.action), ptr(sm.reward), ptr(sm.terminal[1:]), ptr(sm.next_obs[1]), self.gamma,
               self.grad_scale, ptr(self.ws.dy), ptr(self.partials), self.loss_blocks, stream_ptr())
        ops.slab_reduce(self.partials, 3, self.train_metrics[n, k])

    def _backward_and_apply(self, pq: torch.Tensor) -> None:
        """The Q network's backward pass into g[:Pq], clip + Adam over all P parameters, then the target update."""
        L_, s = lib(), stream_ptr()
        Lq, Rp, sm = self.L, self.Rp, self.smp
        self.q_network.backward_sequence(pq, self.ws, sm.obs[0], 1, sm.term_or_trunc[:Lq], None, Lq, Rp, Rp, 1, self.slabs,
                                         self.g[: self.Pq], accumulate=False, grad_scale=self.grad_scale)
        if self.debug is not None:
            self.debug["grads"].append(self.g.clone())
        ops.clip_adam(self.p, self.g, self.m, self.v, self.count, [0, self.P], [self.q_lr], grad_scale=1.0,
                      max_norm=self.max_grad_norm)
        if self.hard_update:  # optax.periodic_update(new, old, t_train, update_period): copy when t_train % period == 0
            if self.t_train % self.update_period == 0:
                launch("target_update", L_.mava_target_update_f32, self.P, ptr(self.p), ptr(self.pt), 0.0, 1, s)
        else:  # optax.incremental_update(new, old, tau)
            launch("target_update", L_.mava_target_update_f32, self.P, ptr(self.p), ptr(self.pt), self.tau, 0, s)
        self.t_train += 1

    def _train_step(self, n: int, k: int) -> None:
        """rec_iql.py:325-463: sample, three passes, the TD loss (a subclass mixes the agents' Q-values in its own),
        clip + Adam, target update."""
        self._sample_batch()
        pq = self.p[: self.Pq]
        q, qn = self._q_passes(pq, self.pt[: self.Pq])
        self._loss(n, k, q, qn)
        self._backward_and_apply(pq)

    def can_train(self) -> bool:
        """The train gate: every env row holds max(min_buffer_size, sample_sequence_length + 1) steps."""
        return self.n_added >= self.min_fill

    def update(self, n: int) -> None:
        """rec_iql.py:470-519: rollout_length act steps, then `epochs` train steps (once past the gate)."""
        for t in range(self.T):
            self._act_step(n, t)
        self.trained[n] = self.can_train()
        if self.trained[n]:
            for k in range(self.K):
                self._train_step(n, k)

    # ---------------------------------------------------------------------------- state views
    def learner_state(self) -> LearnerState:
        lead = (1, 1)
        net = self.q_network
        E, A, EA, c = self.E, self.A, self.EA, self.cur
        params = QNetParams(net.tree(self.p, lead), net.tree(self.pt, lead))
        opt = AdamState(self.count[0].expand(1, 1), net.tree(self.m, lead), net.tree(self.v, lead))
        obs = Observation(self.view[c][:EA].view(1, 1, E, A, self.O), self.mask[c][:EA].view(1, 1, E, A, self.nA).bool(),
                          self.sc[c].view(1, 1, E, A))
        hs = t32_to_rows(self.h[0], H, self.Rpa)[:EA].view(1, 1, E, A, H)
        scalar = lambda v: torch.tensor([[v]], dtype=torch.int64)
        return LearnerState(obs, self.term[c].view(1, 1, E, 1).bool(), self.tot[c][:EA].view(1, 1, E, A)[..., :1].bool(), hs,
                            self.env_state(), scalar(self.t_act), scalar(self.t_train), opt, self.buffer_state(), params,
                            torch.tensor([[[self.seed, self.act_steps]]], dtype=torch.int64))

    def adopt(self, state: LearnerState) -> None:
        """Make the online / target parameters equal to `state`'s (no-op for trees that alias them), e.g. parameters
        restored from a checkpoint.  Environment, buffer and optimiser state stay with the learner."""
        leaf = state.params.online["params"]["pre_torso"]["Dense_0"]["kernel"]
        if not isinstance(leaf, torch.Tensor) or leaf.data_ptr() != self.p.data_ptr():
            to = lambda tree: tree_to(tree, self.p.device)
            self.q_network.flat_from_tree(to(state.params.online), self.p)
            self.q_network.flat_from_tree(to(state.params.target), self.pt)

    def _guard_tensors(self):
        return self.p, [self.view[self.cur]]

    def _train_metrics(self) -> Dict[str, torch.Tensor]:
        rows = [n for n in range(self.n_upd) if self.trained[n]]  # (update(n) sets trained[n] for every n of a learn() call)
        if not rows:  # no train step ran: no TRAIN metrics (run_experiment skips the event)
            return {}
        tm = self.train_metrics[rows]
        return {"q_loss": tm[..., 0], "mean_q": tm[..., 1], "mean_target": tm[..., 2]}


def learner_setup(env, keys, config, device=None):
    """Counterpart of init + make_update_fns (rec_iql.py:62-212, :215-530): (learn, q_network, initial LearnerState).
    `learn(state)` runs num_updates_per_eval updates."""
    key, q_key = int(keys[0]), int(keys[1])
    learner = IQLLearner(env, config, device)
    learner.seed = key
    learner.init_params(q_key)
    learner.reset_envs()
    return bind_learn(learner), learner.q_network, learner.learner_state()
