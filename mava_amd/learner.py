"""Feed-forward PPO learner (ff_ippo / ff_mappo) behind Mava's LearnerFn contract.

Reference: mava/systems/ppo/ff_mappo.py:45-330 (get_learner_fn: _env_step, _calculate_gae,
_update_epoch, _update_minibatch, learner_fn) and :333-432 (learner_setup); ff_ippo.py is the same
file with a decentralised critic.  The XLA program that `jax.pmap(learn)` compiles
is replaced by hand-written gfx950 kernels (libmavahip.so) launched from this module:

    per update:  T x { policy_step -> env.step }         (rollout, time-major trajectory in HBM)
                 critic forward on the last observation    (bootstrap value)
                 GAE reverse scan                          (mava_gae_f32)
                 K epochs x M minibatches x {adv stats, actor grad, critic grad, slab reduce,
                                             [RCCL all-reduce], clip+Adam}

Data layout (per GPU; U = update_batch_size replicas share parameters, ff_mappo.py:417-426):
    params / grads / Adam moments : flat f32 [actor | critic] (+4 loss scalars after the grads)
    trajectory, per replica       : time-major, (T+1, E, A, .) for observations (slot T is the
                                    bootstrap observation and becomes slot 0 of the next rollout),
                                    (T, E, A) for action / value / reward / log_prob / done
    shuffle                       : an int32 permutation of T*E row ids; minibatches are slices of
                                    it and rows are gathered inside the gradient kernels.
One process drives one GPU; with world_size > 1 the env axis is sharded over ranks and the flat
gradient is summed with one all-reduce per minibatch (ff_mappo.py:224-238 pmean "device").

The replica buffers, the constructor's prologue, the flat parameter storage with init_params / adopt / the state trees,
the slot-0 observation view, the clip+Adam hyper-parameter block, learn() and learner_setup() are PPOLearner's
(mava_amd/ppo_learner.py); the networks, the fused / per-step / graph-captured rollout, the batched permutations and
advantage statistics, the gradient launches and the fused update tail are this module's.
"""
from __future__ import annotations

import math
import contextlib
import os
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import ops, parallel, ppo_learner
from .networks import FeedForwardActor, FeedForwardValueNet, MLPTorso
from .ppo_learner import LeanReplica, PPOLearner
from .types import LearnerState, TimeStep


class FFLearner(PPOLearner):
    def __init__(self, env, config, centralised_critic: bool, device: Optional[torch.device] = None):
        # (critic aggregation is a setting of the learner's context handle, like the arithmetic mode: mava_ctx_*)
        super().__init__(env, config, centralised_critic, device, replica=LeanReplica,
                         ctx_kwargs={"critic_aggregation": os.environ.get("MAVA_CRITIC_AGGREGATION", "1") != "0"})
        s, env0, action_head = config.system, self.reps[0].env, self.action_head

        # networks (ff_mappo.py:347-354) - hydra.utils.instantiate is replaced by direct construction
        net = config.network
        # The default configuration (network/mlp.yaml: [128, 128] relu torsos, observation-independent log_std) runs on the
        # fused kernels; any other torso (layer sizes, tanh, layer norm, CNNTorso) or ContinuousActionHead(
        # independent_std=False) runs on the general layer-wise path (mava_amd/generic_networks.py).
        from . import generic_networks as gn

        self.generic = (not gn.is_default_mlp(net.actor_network.pre_torso) or not gn.is_default_mlp(net.critic_network.pre_torso)
                        or (self.continuous and not action_head.independent_std))
        if self.generic:
            if (self.E * env0.num_agents) % 32 or ((self.T * self.E // self.M) * env0.num_agents) % 32:
                raise ValueError("the general network path needs num_envs * num_agents and the agent rows of a minibatch to be "
                                 "multiples of 32")
            obs_shape = getattr(env0, "obs_shape", None)
            state_shape = getattr(env0, "state_shape", None) if centralised_critic else obs_shape
            self.actor_network = gn.GenericActor(gn.torso_from_config(net.actor_network.pre_torso), action_head, self.Oa, obs_shape)
            self.critic_network = gn.GenericCritic(gn.torso_from_config(net.critic_network.pre_torso), centralised_critic, self.Oc,
                                                   state_shape)
        else:
            a_torso = MLPTorso(**{k: v for k, v in net.actor_network.pre_torso.items() if k != "_target_"})
            c_torso = MLPTorso(**{k: v for k, v in net.critic_network.pre_torso.items() if k != "_target_"})
            self.actor_network = FeedForwardActor(a_torso, action_head, self.Oa)
            self.critic_network = FeedForwardValueNet(c_torso, centralised_critic, self.Oc)
        self.Pa, self.Pc = self.actor_network.num_params, self.critic_network.num_params
        self._alloc_params([(self.actor_network, s.actor_lr), (self.critic_network, s.critic_lr)])

        d = self.device
        self.Rb = self.T * self.E // self.M  # env rows per minibatch
        # (with several ranks the actor's slice is all-reduced WHILE the critic's gradient kernel runs,
        # parallel.allreduce_sum_async below: PPOLearner._slab_count leaves RCCL its CUs)
        self.n_slab = self._slab_count((self.Rb * self.A + 31) // 32)
        self.slab_a = torch.zeros((self.n_slab, self.Pa + 2), device=d)
        self.slab_c = torch.zeros((self.n_slab, self.Pc + 2), device=d)
        # the same counter on the device: the kernels add it to their relative step, so a rollout captured in a HIP
        # graph replays with the next counters
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=d)  # (t_global)
        # Single-rank jobs only: with a process group the replay measured SLOWER (RCCL, one rank, forced exchange:
        # 22.5 vs 22.1 ms per update; two gloo ranks on one card: 100x slower), see tools/graph_pg_rehearsal.py.
        # MAVA_GRAPH_ROLLOUT=0 turns it off, =force keeps it on with several ranks.
        mode = os.environ.get("MAVA_GRAPH_ROLLOUT", "1")
        self.graph_rollout = (mode == "force" or (mode != "0" and self.world == 1)) and not self.generic
        self._graphs: Dict[int, Any] = {}  # keyed by the seed: ONE graph for every update index n
        self._graph_seen: set = set()
        # ("f16x2" here: three f16 MFMAs per product with f32 accumulation - ppo_train_h2.hip, rollout_h2.hip: ~22 mantissa
        # bits per operand, the 1e-4 gradient parity tests run on it - for the shapes those kernels instantiate)
        # MAVA_TRAIN_VARIANT=1: the four-wave gradient kernels only (A/B measurements against the eight-wave actor kernel)
        self.ctx.set(self.ctx.TRAIN_VARIANT, int(os.environ.get("MAVA_TRAIN_VARIANT", "0")))
        for net_ in (self.actor_network, self.critic_network):
            net_.ctx = self.ctx
        # the whole rollout in one launch (rollout_h2.hip) when the shape is instantiated; MAVA_FUSED_ROLLOUT=0 keeps
        # the per-step kernels
        # (mava_rollout_ff_f32 hard-codes the synthetic generator's env phase: only an env that declares the capability -
        # SyntheticRware.supports_fused_rollout - is routed there; any other MarlEnv keeps the per-step kernels)
        self.fused_rollout = (self.matmul_mode == "f16x2" and not self.continuous and not self.generic
                              and os.environ.get("MAVA_FUSED_ROLLOUT", "1") != "0"
                              and bool(getattr(env0, "supports_fused_rollout", False))
                              and int(getattr(env0, "synth_state_dim", 0)) == 0
                              and (not centralised_critic or (env0.gs_tiles == 1 and env0.global_state_shared)))
        # The fused rollout's LDS image of the shared global state is f16 and its f32 record is that image converted; the wide critic
        # gradient kernel converts it back on every launch.  With a shared critic on a multiple of 8 inputs the rollout also keeps
        # the halves themselves (rollout_h2.hip state16: (T + 1) * E * Oc * 2 bytes per replica) and a validity word on the device,
        # and every critic gradient launch of the update is handed both (ppo_train_h2.hip: 16-byte loads, no conversion; same
        # bits).  The word is never read on the host.  MAVA_X16=0 turns the copy off (A/B runs, tests).
        self.x16 = (self.fused_rollout and centralised_critic and self.Oc % 8 == 0 and os.environ.get("MAVA_X16", "1") != "0")
        for rep in self.reps:
            rep.state16 = torch.zeros((self.T + 1, self.E, 1, self.Oc), dtype=torch.float16, device=d) if self.x16 else None
            rep.state16_valid = torch.zeros((1,), dtype=torch.int32, device=d) if self.x16 else None
        # The same for agents_view and the eight-wave gradient kernel (ppo_train_w8.hip): the rollout's actor image rows - the
        # observation, the ones column, zeros: RP = 8 * ceil((Oa + 1) / 8) halves - are kept as view16 ((T + 1) * E * A * RP * 2 bytes
        # per replica: 304 MB at the headline shape) with a word of their own, and handed to every actor gradient launch and, under a
        # decentralised critic, to every critic launch.  MAVA_X16=0 turns both records off, MAVA_X16_ACTOR=0 this one alone.
        self.view16 = (self.fused_rollout and not self.continuous and self.matmul_mode == "f16x2" and self.Oa + 1 <= 128
                       and os.environ.get("MAVA_X16", "1") != "0" and os.environ.get("MAVA_X16_ACTOR", "1") != "0")
        rp = 8 * ((self.Oa + 8) // 8)
        for rep in self.reps:
            rep.view16 = torch.zeros((self.T + 1, self.E, self.A, rp), dtype=torch.float16, device=d) if self.view16 else None
            rep.view16_valid = torch.zeros((1,), dtype=torch.int32, device=d) if self.view16 else None
        # With a record active, every gradient launch of an update reads it instead of the f32 array whenever its word is 1, which
        # on the environment's own observations it always is: the rollout is then told to leave slots 1 .. T - 1 of that f32 array
        # unwritten (_reads_records asks the library whether the launches will read the record; the rule is the library's), and a
        # conditional expand behind it rebuilds them on the device should a word ever end 0.  A host read of the skipped slots goes
        # through LeanReplica's properties.  MAVA_ROLLOUT_LEAN=0 writes everything as before (A/B runs, tests).
        self.lean = os.environ.get("MAVA_ROLLOUT_LEAN", "1") != "0"
        # One rank: nothing sits between the gradient kernels and Adam, so both slab sums, clip + Adam, the count increment and
        # the wide critic's W1 re-split run as TWO launches (ops.ppo_finish) instead of six.  With several replicas every
        # replica's gradient kernels write their own rows of the slab matrices and the one sum runs over all U * n_slab rows
        # (fixed order: replica 0's slabs, then replica 1's, ...; the mean over replicas of ff_mappo.py:232-238 is grad_scale).
        self.fused_tail = (self.world == 1 and not self.generic and os.environ.get("MAVA_FUSED_TAIL", "1") != "0")
        self._finish_ws = ops.ppo_finish_workspace(self.Pa, self.Pc, d) if self.fused_tail else None
        # (several ranks: the slab sums stay separate launches around the split all-reduce; the Adam launch still carries the
        # count increment and the W1 re-split: mava_ppo_finish_f32 with n_slab = 0)
        self._finish_ws_mr = (ops.ppo_finish_workspace(self.Pa, self.Pc, d)
                              if (not self.fused_tail and not self.generic and os.environ.get("MAVA_FUSED_TAIL", "1") != "0") else None)
        if self.fused_tail and self.U > 1:
            self.slab_a = torch.zeros((self.U * self.n_slab, self.Pa + 2), device=d)
            self.slab_c = torch.zeros((self.U * self.n_slab, self.Pc + 2), device=d)

    def _refuse(self, env, config) -> None:
        if (self.T * self.E) % self.M:
            raise ValueError("rollout_length * num_envs must be divisible by num_minibatches (ff_mappo.py:277-279)")

    def _timed(self, name: str, fn, *args, **kwargs):
        """Run one kernel launch, optionally bracketed by HIP events on the launch stream."""
        if self.timers is None:
            return fn(*args, **kwargs)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args, **kwargs)
        b.record()
        self.timers.setdefault(name, []).append((a, b))
        return out

    # ------------------------------------------------------------------------------------ setup
    def reset_envs(self) -> None:
        super().reset_envs()
        self.step_dev.zero_()

    # ---------------------------------------------------------------------------- state <-> views
    def _timestep(self, slot: int) -> TimeStep:
        stack, obs = self._stack, self._observation(slot)
        done = stack(lambda r: r.last_done[:, 0]).bool()
        step_type = torch.where(done, 2, 1).to(torch.int8)
        reward = stack(lambda r: r.last_reward)
        n = max(self.n_upd - 1, 0)
        extras = {"episode_metrics": {
            "episode_return": stack(lambda r: r.info_return[n, -1]),
            "episode_length": stack(lambda r: r.info_length[n, -1]),
            "is_terminal_step": stack(lambda r: r.info_terminal[n, -1]).bool()}}
        return TimeStep(step_type, reward, 1.0 - stack(lambda r: r.last_done).float(), obs, extras)

    def learner_state(self) -> LearnerState:
        env_state = self._env_state()
        env_state["running_count_episode_return"] = self._stack(lambda r: r.state.run_return)
        env_state["running_count_episode_length"] = self._stack(lambda r: r.state.run_length)
        return LearnerState(self._params_tree(), self._opt_tree(), self._key(), env_state, self._timestep(0))

    def _adopted(self) -> None:
        # the same buffer with other contents: the W1 copy the last finish launch left in the handle is stale (the wide
        # critic kernels and their W1 cache are this learner's alone)
        self.ctx.set(self.ctx.W1_SPLIT_FRESH, 0)

    # ------------------------------------------------------------------------------------ update
    def _rollout(self, n: int) -> None:
        """The launch-bound part of an update (2*T + 3 small kernels per replica): rollout, bootstrap value and GAE.
        The first call runs eagerly, the second is captured into a HIP graph, later ones replay it - the kernels
        read the moving step counter from step_dev, everything else they touch (incl. the metrics staging slots)
        is persistent, so the one graph serves every update index."""
        if self.fused_rollout and self._rollout_fused(n):
            self.t_global += self.T
            return
        if not self.graph_rollout or self.timers is not None:
            self._rollout_body()
            self._bootstrap_and_gae()
        else:
            key = self.seed
            graph = self._graphs.get(key)
            if graph is None and key in self._graph_seen:
                # thread_local: every launch of the rollout comes from this thread; RCCL's watchdog thread may query
                # its events meanwhile
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    self._rollout_body()
                    self._bootstrap_and_gae()
                self._graphs[key] = graph
            if graph is None:
                self._graph_seen.add(key)
                self._rollout_body()
                self._bootstrap_and_gae()
            else:
                graph.replay()
        for rep in self.reps:  # episode metrics of update n (ff_mappo.py:95,299); outside the graph: n moves
            rep.info_return[n].copy_(rep.cur_return)
            rep.info_length[n].copy_(rep.cur_length)
            rep.info_terminal[n].copy_(rep.cur_terminal)
        self.t_global += self.T

    def _rollout_fused(self, n: int) -> bool:
        """ff_mappo.py:76-139: one launch per replica for all T acting + env steps, the bootstrap value and GAE
        (mava_rollout_ff_f32).  False when the library does not instantiate the shape."""
        s = self.config.system
        pa, pc = self.p[: self.Pa], self.p[self.Pa :]
        EA = self.E * self.A
        # The replicas' rollouts are independent (ff_mappo.py:389 vmaps over update_batch_size) and one replica of the reference's
        # default shape (2 x 2048 envs) fills half the CUs: replicas 1.. are launched on side streams, under replica 0's.
        main = torch.cuda.current_stream() if self.device.type == "cuda" else None
        side = self.U > 1 and self.timers is None and main is not None and os.environ.get("MAVA_ROLLOUT_STREAMS", "1") != "0"
        if side and not hasattr(self, "_roll_streams"):
            from .streams import overlapping_stream

            self._roll_streams = [overlapping_stream(self.device) for _ in range(self.U - 1)]  # (probed for real concurrency)
            if any(st is None for st in self._roll_streams):
                self._roll_streams = []
        side = side and len(self._roll_streams) == self.U - 1
        if side:
            for st in self._roll_streams:  # (before replica 0's launch is queued: the side streams wait for the parameters only)
                st.wait_stream(main)
        for u, rep in enumerate(self.reps):
            env = rep.env
            skip_av, skip_gs = self._reads_records(rep) if self.lean else (False, False)
            with (torch.cuda.stream(self._roll_streams[u - 1]) if (side and u > 0) else contextlib.nullcontext()):
              ok = self._timed(
                "rollout_fused", ops.rollout_ff, pa, pc, n_actions=self.nA, critic_shared=self.centralised, E=self.E,
                A=self.A, O=env.raw_obs_dim, T=self.T, time_limit=env.time_limit, policy_seed=self.seed,
                env_seed=env.seed, t0=self.t_global, row_offset=(self.rank * self.U + u) * EA, env_offset=env.env_offset,
                reward_mode=1 if env.reward_mode == "match" else 0, env_state=rep.state, agents_view=rep.av_raw,
                global_state=rep.gs_raw, action_mask=rep.action_mask, obs_step_count=rep.step_count,
                action=rep.action, value=rep.value, reward=rep.reward, log_prob=rep.log_prob, done=rep.done,
                last_val=rep.last_val, info_return=rep.info_return[n], info_length=rep.info_length[n],
                info_terminal=rep.info_terminal[n], adv=rep.adv, tgt=rep.tgt, gamma=float(s.gamma),
                gae_lambda=float(s.gae_lambda), last_reward=rep.last_reward, last_done=rep.last_done,
                step_counter=self.step_dev if u == 0 else None,  # (the launch leaves all three: nothing follows it)
                state16=rep.state16, state16_valid=rep.state16_valid, view16=rep.view16, view16_valid=rep.view16_valid,
                skip_agents_view=skip_av, skip_global_state=skip_gs)
              if ok and (skip_av or skip_gs):
                # a word that ended 0 (a slot-0 value with a low f16 term) sends the gradient launches back to the f32 arrays:
                # the launch looks at the words itself and does nothing when they are 1
                self._timed("rollout_expand", ops.rollout_expand, rep.av_raw if skip_av else None, rep.view16 if skip_av else None,
                            rep.view16_valid if skip_av else None, rep.gs_raw if skip_gs else None, rep.state16 if skip_gs else None,
                            rep.state16_valid if skip_gs else None, force=False)
                rep.stale_av, rep.stale_gs = rep.stale_av or skip_av, rep.stale_gs or skip_gs
              if not ok:
                assert u == 0
                self.fused_rollout = self.x16 = self.view16 = False
                for r in self.reps:  # (nobody writes the records: the gradient launches must not be handed them)
                    r.state16 = r.state16_valid = r.view16 = r.view16_valid = None
                return False
        if side:
            for st in self._roll_streams:
                main.wait_stream(st)
        return True

    def _reads_records(self, rep) -> Tuple[bool, bool]:
        """(agents_view, global_state): does EVERY gradient launch of an update that takes the f32 array also take its f16 record
        and, by the library's own launch rule, read the record whenever its word is 1?  Same arguments as _minibatch's launches."""
        T, TEA = self.T, self.T * self.E * self.A
        av = rep.av_raw[:T].view(TEA, self.Oa)
        v16 = rep.view16[:T].view(TEA, -1) if self.view16 else None
        reads_av = v16 is not None and ops.ppo_actor_grad_reads_input16(self.ctx, av, self.nA, self.A, v16)
        reads_gs = False
        if self.centralised:
            reads_gs = self.x16 and ops.ppo_critic_grad_reads_input16(
                self.ctx, rep.gs_raw[:T].view(-1, self.Oc), self.critic_share, self.A, rep.state16[:T].view(-1, self.Oc))
        elif reads_av:  # (the critic's input is agents_view too)
            reads_av = self.critic_share == 1 and ops.ppo_critic_grad_reads_input16(self.ctx, av, 1, self.A, v16)
        return bool(reads_av), bool(reads_gs)

    def _lean_guard(self, rep) -> None:
        """Before a gradient launch: the answer the rollout skipped by ("yes", for a stale array) must still hold - the handle's
        settings can change in between; an array whose record would no longer be read is rebuilt first."""
        if rep.stale_av or rep.stale_gs:
            now = self._reads_records(rep)
            rep.materialise(av=not now[0], gs=not now[1])

    def _rollout_body(self) -> None:
        """ff_mappo.py:76-106: T acting steps, recording the time-major trajectory in place."""
        pa, pc = self.p[: self.Pa], self.p[self.Pa :]
        EA = self.E * self.A
        for t in range(self.T):
            step = t  # relative; the kernels add step_dev (= t_global at the start of this rollout)
            for u, rep in enumerate(self.reps):
                av = rep.agents_view[t].view(EA, self.Oa)
                if self.centralised:
                    cx = rep.global_state[t].view(-1, self.Oc)
                else:
                    cx = av
                # a critic input row shared by the A agents of an env (critic_share == A) is evaluated once and its
                # value written to all A agent slots - the same numbers as A identical forward passes
                shared = self.critic_share == self.A and self.A > 1
                common = dict(critic_share=1 if shared else self.critic_share, critic_rows=self.E if shared else EA,
                              value_broadcast=self.A if shared else 1, seed=self.seed, step=step,
                              step_base=self.step_dev, row_offset=(self.rank * self.U + u) * EA, ctx=self.ctx)
                if self.generic:
                    self._timed("policy_step", self._generic_act, u, rep, t, step)
                elif self.continuous:
                    self._timed("policy_step", ops.policy_step_continuous, pa, pc, av, cx, action_dim=self.nA, min_scale=self.min_scale,
                                out=(rep.action[t].view(EA, self.nA), rep.log_prob[t].view(EA), rep.value[t].view(EA)),
                                **common)
                else:
                    self._timed("policy_step", ops.policy_step, pa, pc, av, rep.action_mask[t].view(EA, self.nA), cx,
                                n_actions=self.nA,
                                out=(rep.action[t].view(EA), rep.log_prob[t].view(EA), rep.value[t].view(EA)), **common)
                last = t == self.T - 1
                self._timed("env_step", rep.env.step_into, rep.state, step + 1, rep.obs_slot(t + 1), rep.reward[t], rep.done[t],
                            rep.cur_return[t], rep.cur_length[t], rep.cur_terminal[t], t_base=self.step_dev,
                            action=rep.action[t] if self._env_reads_action else None)
                if last:
                    rep.last_reward.copy_(rep.reward[t])
                    rep.last_done.copy_(rep.done[t])
        self.step_dev.add_(self.T)

    def _bootstrap_and_gae(self) -> None:
        """ff_mappo.py:109-139."""
        s = self.config.system
        pc = self.p[self.Pa :]
        EA = self.E * self.A
        for rep in self.reps:
            cx = rep.global_state[self.T].view(-1, self.Oc) if self.centralised else rep.agents_view[self.T].view(EA, self.Oa)
            if self.generic:
                v = self.critic_network.net.forward(pc, self._gws_roll[1], cx.view(1, self.E, -1, self.Oc), self.critic_share, None, EA,
                                                    self.E, self.A)[0]
                rep.last_val.view(EA).copy_(v)
            else:
                ops.mlp_forward(pc, self.Oc, 1, cx, rows=EA, x_share=self.critic_share, out=rep.last_val.view(EA, 1), ctx=self.ctx)
            self._timed("gae", ops.gae, rep.reward.view(self.T, EA), rep.value.view(self.T, EA), rep.done.view(self.T, EA),
                        rep.last_val.view(EA), float(s.gamma), float(s.gae_lambda),
                        out=(rep.adv.view(self.T, EA), rep.tgt.view(self.T, EA)), ctx=self.ctx)

    def _minibatch(self, n: int, k: int, mb: int, perm: Optional[torch.Tensor]) -> None:
        """ff_mappo.py:144-266 for minibatch `mb` of epoch `k`."""
        s = self.config.system
        T, E, A = self.T, self.E, self.A
        TEA = T * E * A
        pa, pc = self.p[: self.Pa], self.p[self.Pa :]
        idx = None if perm is None else perm[mb * self.Rb : (mb + 1) * self.Rb]
        base = mb * self.Rb
        if self.generic:
            return self._minibatch_generic(n, k, mb, idx if idx is not None else torch.arange(base, base + self.Rb, dtype=torch.int32,
                                                                                             device=self.device))
        # actor: gradient kernels of every replica, fixed-order slab sum into g[:Pa] (+ actor_loss, entropy)
        ns = self.n_slab
        per_rep = self.fused_tail and self.U > 1  # (each replica's kernels own n_slab rows of the slab matrices)
        for u, rep in enumerate(self.reps):
            slab_a = self.slab_a[u * ns : (u + 1) * ns] if per_rep else self.slab_a
            self._lean_guard(rep)
            av = rep.av_raw[:T].view(TEA, self.Oa)
            if getattr(self, "_stats_batched", False) and perm is self._perm_bufs[k]:
                stats = self._stats_all[u, k * self.M + mb]
            else:
                stats = ops.adv_stats(rep.adv.view(TEA), idx, base, self.Rb, A, out=self.stats)
            if self.continuous:
                self._timed("actor_grad", ops.ppo_actor_grad_continuous, pa, av, rep.action.view(TEA, self.nA),
                            rep.log_prob.view(TEA), rep.adv.view(TEA), stats, idx, base, self.Rb, A, self.nA,
                            float(s.clip_eps), float(s.ent_coef), self.seed, self.ent_step,
                            (self.rank * self.U + u) * TEA, slab_a, min_scale=self.min_scale)
            else:
                self._timed("actor_grad", ops.ppo_actor_grad, pa, av, rep.action_mask[:T].view(TEA, self.nA),
                            rep.action.view(TEA), rep.log_prob.view(TEA), rep.adv.view(TEA), stats, idx, base,
                            self.Rb, A, self.nA, float(s.clip_eps), float(s.ent_coef), slab_a, ctx=self.ctx,
                            input16=rep.view16[:T].view(TEA, -1) if self.view16 else None,
                            input16_valid=rep.view16_valid if self.view16 else None)
            if not self.fused_tail:
                ops.slab_reduce2(self.slab_a, self.Pa, self.g[: self.Pa], 2, self.g[self.P : self.P + 2], accumulate=u > 0)
        # pmean "device" of ff_mappo.py:228-238, RCCL over xGMI: the actor's slice travels on RCCL's stream while
        # the critic's backward kernels run on this one
        w_actor = parallel.allreduce_sum_async(self.g[: self.Pa])
        for u, rep in enumerate(self.reps):
            av = rep.av_raw[:T].view(TEA, self.Oa)
            cx = rep.gs_raw[:T].view(-1, self.Oc) if self.centralised else av
            in16 = in16_valid = None
            if self.x16:
                in16, in16_valid = rep.state16[:T].view(-1, self.Oc), rep.state16_valid
            elif self.view16 and not self.centralised and self.critic_share == 1:  # (the critic reads agents_view, one input row per agent row)
                in16, in16_valid = rep.view16[:T].view(TEA, -1), rep.view16_valid
            self._timed("critic_grad", ops.ppo_critic_grad, pc, cx, self.critic_share, rep.value.view(TEA), rep.tgt.view(TEA),
                        idx, base, self.Rb, A, float(s.clip_eps), float(s.vf_coef),
                        self.slab_c[u * ns : (u + 1) * ns] if per_rep else self.slab_c, ctx=self.ctx,
                        input16=in16, input16_valid=in16_valid)
            if not self.fused_tail:
                ops.slab_reduce2(self.slab_c, self.Pc, self.g[self.Pa : self.P], 1, self.g[self.P + 2 : self.P + 3], accumulate=u > 0)
        if self.fused_tail:
            self._ppo_finish("finish", n, k, mb, self.slab_a, self.slab_c, self._finish_ws)
            return
        w_rest = parallel.allreduce_sum_async(self.g[self.Pa :])  # critic gradient + the loss scalars
        for wk in (w_actor, w_rest):
            if wk is not None:
                wk.wait()
        if self._finish_ws_mr is not None:  # several ranks: Adam + count increment + W1 re-split as one launch on the all-reduced g
            self._ppo_finish("clip_adam", n, k, mb, None, None, self._finish_ws_mr)
        else:
            self._timed("clip_adam", self._clip_adam, n, k, mb)

    def _ppo_finish(self, name: str, n: int, k: int, mb: int, slab_a, slab_c, workspace) -> None:
        """Slab sums (none when slab_a is None), clip + Adam, the count increment and the W1 re-split (ops.ppo_finish)."""
        self._timed(name, ops.ppo_finish, self.ctx, slab_a, slab_c, self.Pa, self.Pc, self.g, self.p, self.m, self.v, self.count,
                    self.seg_lr[0], self.seg_lr[1], critic_din=self.Oc, workspace=workspace, **self._adam_kwargs(n, k, mb))

    # ---------------------------------------------------------------- general network path (mava_amd/generic_networks.py)
    def _generic_setup(self) -> None:
        d = self.device
        EA, Rm = self.E * self.A, self.Rb * self.A
        a, c = self.actor_network.net, self.critic_network.net
        self._gws_roll = (a.workspace(EA, d, False), c.workspace(EA, d, False))
        self._gws = (a.workspace(Rm, d, True), c.workspace(Rm, d, True))
        # the backward chain runs in units of a power of two near the row count (mava_seq_actor_loss_f32: f16 range)
        self._g_scale = float(2 ** math.ceil(math.log2(Rm)))
        self._g_dscale = torch.zeros((self._gws[0].loss_partials.shape[0], max(self.nA, 1)), device=d)

    def _generic_act(self, u: int, rep, t: int, step: int) -> None:
        """ff_mappo.py:76-94 for one replica and step: actor forward -> sample / log-prob, critic forward -> value."""
        if not hasattr(self, "_gws_roll"):
            self._generic_setup()
        L, st = ops.lib(), ops.stream_ptr()
        pa, pc = self.p[: self.Pa], self.p[self.Pa :]
        E, A, EA = self.E, self.A, self.E * self.A
        an = self.actor_network
        outs = an.net.forward(pa, self._gws_roll[0], rep.agents_view[t : t + 1], 1, None, EA, E, A)
        seed, row_off = self.seed & (2**64 - 1), ((self.rank * self.U + u) * EA) & 0xFFFFFFFF
        gstep = (self.t_global + step) & 0xFFFFFFFF  # (the general path is not graph-captured: host-side step counter)
        if self.continuous:
            ind = an.independent_std
            ops.check(L.mava_seq_sample_continuous_f32(EA, self.nA, self.min_scale, ops.ptr(outs[0]), ops.ptr(an.log_std(pa)) if ind else None,
                                                       None if ind else ops.ptr(outs[1]), seed, gstep, row_off, 0, ops.ptr(rep.action[t]),
                                                       ops.ptr(rep.log_prob[t]), st), "mava_seq_sample_continuous_f32")
        else:
            ops.check(L.mava_seq_sample_f32(EA, self.nA, ops.ptr(outs[0]), ops.ptr(rep.action_mask[t]), seed, gstep, row_off, 0,
                                            ops.ptr(rep.action[t]), ops.ptr(rep.log_prob[t]), st), "mava_seq_sample_f32")
        cx = rep.global_state[t : t + 1] if self.centralised else rep.agents_view[t : t + 1]
        v = self.critic_network.net.forward(pc, self._gws_roll[1], cx, self.critic_share, None, EA, E, A)[0]
        rep.value[t].view(EA).copy_(v)  # a (rows x 1) T32 matrix is row-major

    def _minibatch_generic(self, n: int, k: int, mb: int, idx: torch.Tensor) -> None:
        """ff_mappo.py:144-266 on the general path: the (t, e) rows of the minibatch are presented to the sequence kernels
        as T = 1 'sequences' over a flattened env axis of T*E entries (idx = their indices)."""
        if not hasattr(self, "_gws"):
            self._generic_setup()
        s = self.config.system
        T, E, A = self.T, self.E, self.A
        TE, Rm = T * E, self.Rb * A
        L, st = ops.lib(), ops.stream_ptr()
        pa, pc = self.p[: self.Pa], self.p[self.Pa :]
        idx = idx.contiguous()
        wa, wc = self._gws
        an, cn, gs = self.actor_network, self.critic_network, self._g_scale
        nblk = wa.loss_partials.shape[0]
        for u, rep in enumerate(self.reps):
            acc = u > 0
            outs = an.net.forward(pa, wa, rep.agents_view[:T].view(1, TE, A, self.Oa), 1, idx, Rm, TE, A)
            ops.adv_stats(rep.adv.view(-1), idx, 0, self.Rb, A, out=self.stats)
            if self.continuous:
                ind = an.independent_std
                ops.check(L.mava_seq_actor_loss_continuous_f32(
                    1, Rm, TE, A, self.nA, self.min_scale, ops.ptr(idx), ops.ptr(outs[0]), ops.ptr(an.log_std(pa)) if ind else None,
                    None if ind else ops.ptr(outs[1]), ops.ptr(rep.action), ops.ptr(rep.log_prob), ops.ptr(rep.adv), ops.ptr(self.stats),
                    self.stats.shape[0], float(s.clip_eps), float(s.ent_coef), self.seed & (2**64 - 1), self.ent_step & 0xFFFFFFFF,
                    ((self.rank * self.U + u) * TE * A) & 0xFFFFFFFF, gs, ops.ptr(wa.dout[0]), None if ind else ops.ptr(wa.dout[1]),
                    ops.ptr(wa.loss_partials), ops.ptr(self._g_dscale), nblk, st), "mava_seq_actor_loss_continuous_f32")
                if ind:
                    ops.slab_reduce(self._g_dscale, self.nA, an.log_std(self.g[: self.Pa]), accumulate=acc)
            else:
                ops.check(L.mava_seq_actor_loss_f32(1, Rm, TE, A, self.nA, ops.ptr(idx), ops.ptr(outs[0]), ops.ptr(rep.action_mask[:T]),
                                                    ops.ptr(rep.action), ops.ptr(rep.log_prob), ops.ptr(rep.adv), ops.ptr(self.stats),
                                                    self.stats.shape[0], float(s.clip_eps), float(s.ent_coef), gs, ops.ptr(wa.dout[0]),
                                                    ops.ptr(wa.loss_partials), nblk, st), "mava_seq_actor_loss_f32")
            ops.slab_reduce(wa.loss_partials, 2, self.g[self.P : self.P + 2], accumulate=acc)
            an.net.backward(pa, wa, wa.dout[: len(an.net.heads)], self.g[: self.Pa], accumulate=acc, grad_scale=gs)
        w_actor = parallel.allreduce_sum_async(self.g[: self.Pa])
        for u, rep in enumerate(self.reps):
            acc = u > 0
            cx = (rep.global_state[:T].view(1, TE, -1, self.Oc) if self.centralised else rep.agents_view[:T].view(1, TE, A, self.Oa))
            v = cn.net.forward(pc, wc, cx, self.critic_share, idx, Rm, TE, A)[0]
            ops.check(L.mava_seq_critic_loss_f32(1, Rm, TE, A, 1, ops.ptr(idx), ops.ptr(v), ops.ptr(rep.value), ops.ptr(rep.tgt),
                                                 float(s.clip_eps), float(s.vf_coef), gs, ops.ptr(wc.dout[0]), ops.ptr(wc.loss_partials),
                                                 nblk, st), "mava_seq_critic_loss_f32")
            ops.slab_reduce(wc.loss_partials, 1, self.g[self.P + 2 : self.P + 3], accumulate=acc)
            cn.net.backward(pc, wc, [wc.dout[0]], self.g[self.Pa : self.P], accumulate=acc, grad_scale=gs)
        w_rest = parallel.allreduce_sum_async(self.g[self.Pa :])
        for wk in (w_actor, w_rest):
            if wk is not None:
                wk.wait()
        self._clip_adam(n, k, mb)

    def _permutations(self) -> List[torch.Tensor]:
        """ff_mappo.py:272-273: one permutation of the T*E rows per epoch, identical on every replica and rank (the
        reference hands the same PRNG key to all of them, :417-426): mava_permutation_i32 keyed by (seed, a running
        epoch counter) - one launch for the K epochs (up to 16 per launch), where torch.randperm's sort passes were
        ~1 ms of device time per update at T*E = 524 288.  Written into persistent buffers (read by the kernels of this
        update only)."""
        if not hasattr(self, "_perm_bufs"):
            self._perm_all = torch.empty((self.K, self.T * self.E), dtype=torch.int32, device=self.device)
            self._perm_bufs = [self._perm_all[k] for k in range(self.K)]
            self._stats_all = torch.empty((self.U, self.K * self.M, self.stats.shape[0], 2), dtype=torch.float64, device=self.device)
        for k0 in range(0, self.K, 16):  # row k: counter perm_count + k
            ops.permutation_batched(self.T * self.E, self.seed, self.perm_count + k0, self._perm_all[k0 : k0 + 16])
        self.perm_count += self.K
        return self._perm_bufs

    def update(self, n: int, permutations: Optional[List[torch.Tensor]] = None) -> None:
        own = permutations is None
        if own:
            permutations = self._permutations()
        # parameters may have been written from outside since the last minibatch (adopt(), a test): the first wide critic
        # launch of an update always re-splits W1 itself (MAVA_CTX_W1_SPLIT_FRESH)
        self.ctx.set(self.ctx.W1_SPLIT_FRESH, 0)
        self._rollout(n)
        # advantage statistics of ALL K x M minibatches in one launch per replica (the permutations are this learner's
        # own contiguous buffer: minibatch (k, mb) = slice k * M + mb of it); otherwise one launch per minibatch
        self._stats_batched = own and not self.generic and self.T * self.E == self.M * self.Rb  # (slices tile the buffer)
        if self._stats_batched:
            for u, rep in enumerate(self.reps):
                ops.adv_stats_batched(rep.adv.view(-1), self._perm_all.view(-1), self.Rb, self.A, self.K * self.M,
                                      out=self._stats_all[u])
        for k in range(self.K):
            self._epoch(n, k, permutations[k])
        self._carry_observation()

    def _carry_observation(self) -> None:
        for rep in self.reps:  # (one launch per replica)
            ops.rollout_carry(rep.av_raw, rep.gs_raw, rep.action_mask, rep.step_count)  # (slot T -> slot 0: always written)


def learner_setup(env, keys, config, centralised_critic: bool, device=None):
    """Counterpart of learner_setup (ff_mappo.py:333-432): returns (learn, actor_network,
    init_learner_state).  `keys` = (key, actor_net_key, critic_net_key) integer seeds."""
    return ppo_learner.learner_setup(FFLearner, env, keys, config, centralised_critic, device=device)


def get_final_step_metrics(metrics: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], bool]:
    """mava/wrappers/episode_metrics.py:114-132."""
    metrics = dict(metrics)
    is_final = metrics.pop("is_terminal_step").bool()
    has_final = bool(is_final.any())
    if not has_final:
        return {k: torch.zeros_like(v) for k, v in metrics.items()}, False
    return {k: v[is_final] for k, v in metrics.items()}, True
