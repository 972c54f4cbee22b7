"""Value-decomposition Q-learning (rec_qmix, rec_vdn) on top of rec_iql's learner.

One learner, `system.mixer: qmix | vdn`.  Acting, the replay buffer and its sampler, the evaluator, the epsilon schedule,
the train gate and the target-update rule are IQLLearner's (mava_amd/iql_learner.py); what differs is the train step's
loss (`_loss`): the per-agent Q-values of the three recurrent passes are mixed into one Q_tot per sample and time step and
regressed on the TEAM reward (the mean of the agents' rewards; agent 0's terminal flag, which the buffer stores on every
agent row).

  qmix (Rashid et al. 2018):  Q_tot = elu(qa @ |w1(s)| + b1(s)) @ |w2(s)| + b2(s), the four hypernetworks being
      w1 = Dense(A * Em)(relu(Dense(Hh)(s))), b1 = Dense(Em)(s), w2 = Dense(Em)(relu(Dense(Hh)(s))),
      b2 = Dense(1)(relu(Dense(Em)(s)));
  vdn (Sunehag et al. 2017):  Q_tot = sum_j qa_j, no mixer parameters.

The mixer's state s of sample b at step t is the concatenation of the sample's A stored agent views (Ds = A * O):
obs[:L] for the online mixer, next_obs[:L] - the pre-reset observations - for the target mixer.  DESIGN.md §3.24 says
where that deviates from an environment's own global_state.

Parameters are one flat vector [q_network | mixer] for online and for target: one Adam with one global-norm clip, one
target-update launch.  Launches per train step: mava_replay_sample_f32, the three forward_sequence chains,
mava_qmix_state_t32_f32 and the hypernetworks' forward passes (general layer path, `ctx` = this learner's handle) on the
online and the target parameters, mava_qmix_td_f32 (select + argmax, both mixers, TD error, backward through the online
mixer: one launch), the hypernetworks' backward passes, backward_sequence, mava_clip_adam, mava_target_update_f32.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import launch, lib, ptr, stream_ptr
from .generic_networks import GenericMLPTorso, GenericNet
from .iql_learner import IQLLearner
from .learner_common import bind_learn, pad32
from .networks import _orthogonal_
from .systems.q_learning.types import LearnerState, QNetParams
from .utils.tree import tree_to

MIXERS = ("qmix", "vdn")
MAX_AGENTS, MAX_EMBED = 16, 64  # mava_qmix_td_f32's limits
# Scale of the hypernetworks' output kernels (orthogonal).  The states are raw concatenated observations (|s| ~ 10 on LBF);
# at scale 1 the initial |Q_tot| is in the tens against rewards below 1, and the first TD errors, multiplied by grad_scale,
# leave the f16 range of the f16x2 backward chain.  At 0.1 Q_tot starts O(1) with dQ_tot / dqa_j ~ 1, like vdn.
OUT_SCALE = 0.1


class QMixer:
    """The four hypernetworks over one flat parameter vector [w1 net | b1 dense | w2 net | b2 net]; each net's own layout
    is GenericNet's ([Dense_0 kernel | bias | head kernel | head bias])."""

    def __init__(self, A: int, Ds: int, Em: int, Hh: int):
        self.A, self.Ds, self.Em, self.Hh = int(A), int(Ds), int(Em), int(Hh)
        self.w1 = GenericNet(GenericMLPTorso([Hh]), Ds, [("Dense_1", A * Em, OUT_SCALE)])
        self.w2 = GenericNet(GenericMLPTorso([Hh]), Ds, [("Dense_1", Em, OUT_SCALE)])
        self.b2 = GenericNet(GenericMLPTorso([Em]), Ds, [("Dense_1", 1, OUT_SCALE)])
        self.nets = {"hyper_w1": self.w1, "hyper_w2": self.w2, "hyper_b2": self.b2}
        self.off: Dict[str, int] = {}
        off = 0
        for name, n in (("hyper_w1", self.w1.num_params), ("hyper_b1", Ds * Em + Em), ("hyper_w2", self.w2.num_params),
                        ("hyper_b2", self.b2.num_params)):
            self.off[name], off = off, off + n
        self.num_params = off

    def set_ctx(self, ctx) -> None:
        for n in self.nets.values():
            n.ctx = ctx

    def seg(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        n = (self.Ds * self.Em + self.Em) if name == "hyper_b1" else self.nets[name].num_params
        return flat[self.off[name] : self.off[name] + n]

    def b1_leaves(self, flat: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        s = self.seg(flat, "hyper_b1")
        return s[: self.Ds * self.Em], s[self.Ds * self.Em :]

    def init_flat(self, seed: int) -> torch.Tensor:
        """GenericNet's orthogonal init (sqrt 2 hidden kernels, OUT_SCALE output kernels, zero biases): it stands in for
        whatever an upstream QMIX would use (unpinned: the reference has no mixer)."""
        flat = torch.zeros(self.num_params, dtype=torch.float32)
        for i, (name, net) in enumerate(self.nets.items()):
            self.seg(flat, name).copy_(net.init_flat(seed + i))
        gen = torch.Generator().manual_seed((int(seed) + 3) & 0x7FFFFFFFFFFFFFFF)
        _orthogonal_(self.b1_leaves(flat)[0].view(self.Ds, self.Em), OUT_SCALE, gen)
        return flat

    def tree(self, flat: torch.Tensor, lead: Tuple[int, ...] = ()) -> Dict[str, Any]:
        ex = (lambda v: v.expand(*lead, *v.shape)) if lead else (lambda v: v)
        out: Dict[str, Any] = {}
        for name, net in self.nets.items():
            f = self.seg(flat, name)
            out[name] = {"Dense_0": net.torso_tree(f, lead)["Dense_0"], "Dense_1": net.head_leaf(f, 0, lead)}
        k, b = self.b1_leaves(flat)
        out["hyper_b1"] = {"Dense_0": {"kernel": ex(k.view(self.Ds, self.Em)), "bias": ex(b)}}
        return out

    def flat_from_tree(self, tree: Dict[str, Any], out: torch.Tensor) -> torch.Tensor:
        for name, net in self.nets.items():
            f = self.seg(out, name)
            net.load_torso_tree({"Dense_0": tree[name]["Dense_0"]}, f)
            net.load_head_leaf(tree[name]["Dense_1"], 0, f)
        k, b = self.b1_leaves(out)
        for dst, leaf, nd in ((k.view(self.Ds, self.Em), tree["hyper_b1"]["Dense_0"]["kernel"], 2), (b, tree["hyper_b1"]["Dense_0"]["bias"], 1)):
            v = torch.as_tensor(leaf)
            while v.dim() > nd:
                v = v[0]
            dst.copy_(v)
        return out


class _HyperPass:
    """Workspaces and T32 outputs of the four hypernetworks for one parameter set (online: training; target: inference)."""

    def __init__(self, mx: QMixer, rows: int, device, training: bool):
        self.ws = {name: net.workspace(rows, device, training) for name, net in mx.nets.items()}
        self.b1 = torch.empty(rows * mx.Em, device=device)
        self.out: Dict[str, torch.Tensor] = {}


class QMIXLearner(IQLLearner):
    def __init__(self, env, config, device: Optional[torch.device] = None):
        s = config.system
        self.mixer_kind = str(s.get("mixer", "qmix"))
        if self.mixer_kind not in MIXERS:
            raise ValueError(f"system.mixer must be 'qmix' or 'vdn', got {self.mixer_kind!r}")
        super().__init__(env, config, device)  # rec_iql's refusals and buffers
        d, A = self.device, self.A
        self.Em, self.Hh = int(s.get("mixer_embed_dim", 32)), int(s.get("hypernet_hidden_dim", 64))
        if not 1 <= A <= MAX_AGENTS:
            raise NotImplementedError(f"the mixer kernel takes 1..{MAX_AGENTS} agents, the environment has {A}")
        if self.mixer_kind == "qmix" and not (1 <= self.Em <= MAX_EMBED and self.Hh >= 1):
            raise ValueError(f"system.mixer_embed_dim must be in [1, {MAX_EMBED}] and system.hypernet_hidden_dim >= 1, got "
                             f"{self.Em} and {self.Hh}")
        self.Bp = pad32(self.B)       # mixer rows per time step
        self.Ds = A * self.O
        self.Dsp = pad32(self.Ds)
        self.mrows = self.L * self.Bp
        self.mixer = QMixer(A, self.Ds, self.Em, self.Hh) if self.mixer_kind == "qmix" else None
        self.Pm = self.mixer.num_params if self.mixer is not None else 0
        P = self.P = self.Pq + self.Pm
        # one flat vector [q_network | mixer] for the parameters, the target, the Adam moments and the gradient
        self.p, self.pt = torch.zeros(P, device=d), torch.zeros(P, device=d)
        self.m, self.v, self.g = torch.zeros(P, device=d), torch.zeros(P, device=d), torch.zeros(P, device=d)
        self.td_blocks = max(1, min(256, -(-self.mrows // 64)))
        self.partials = torch.zeros((self.td_blocks, 3), device=d)
        if self.mixer is not None:
            self.mixer.set_ctx(self.ctx)
            self.mstate = torch.zeros(self.mrows * self.Dsp, device=d)
            self.mstate_next = torch.zeros(self.mrows * self.Dsp, device=d)
            self.hp = _HyperPass(self.mixer, self.mrows, d, training=True)
            self.hp_target = _HyperPass(self.mixer, self.mrows, d, training=False)
            self.d_w1 = torch.zeros(self.mrows * A * self.Em, device=d)
            self.d_b1 = torch.zeros(self.mrows * self.Em, device=d)
            self.d_w2 = torch.zeros(self.mrows * self.Em, device=d)
            self.d_b2 = torch.zeros(self.mrows, device=d)
            # the hypernetworks' backward runs in the Q network's units (grad_scale); both row counts enter one power of two
            self.grad_scale = float(2 ** math.ceil(math.log2(max(self.L * self.Rp, self.mrows))))

    # ------------------------------------------------------------------------------------ setup
    def init_params(self, q_seed: int) -> None:
        self.p[: self.Pq].copy_(self.q_network.init_flat(q_seed))
        if self.mixer is not None:
            self.p[self.Pq :].copy_(self.mixer.init_flat(q_seed + 101))
        self.pt.copy_(self.p)
        self.m.zero_()
        self.v.zero_()
        self.count.zero_()

    # ------------------------------------------------------------------------------------ update
    def _hyper_forward(self, flat: torch.Tensor, hp: _HyperPass, state: torch.Tensor) -> Dict[str, torch.Tensor]:
        mx, rows = self.mixer, self.mrows
        for name, net in mx.nets.items():
            hp.out[name] = net.forward(mx.seg(flat, name), hp.ws[name], None, 1, None, rows, rows, 1, x_t32=state, x_t32_ld=self.Dsp)[0]
        k, b = mx.b1_leaves(flat)
        mx.w1._dense(state.data_ptr(), self.Dsp, mx.Ds, k, b, hp.b1, mx.Em, rows, what="qmix_b1")
        hp.out["hyper_b1"] = hp.b1
        return hp.out

    def _hyper_backward(self, flat: torch.Tensor, grad: torch.Tensor) -> None:
        mx, hp = self.mixer, self.hp
        for name, d_out in (("hyper_w1", self.d_w1), ("hyper_w2", self.d_w2), ("hyper_b2", self.d_b2)):
            mx.nets[name].backward(mx.seg(flat, name), hp.ws[name], [d_out], mx.seg(grad, name), accumulate=False,
                                   grad_scale=self.grad_scale)
        gk, gb = mx.b1_leaves(grad)
        mx.w1._xty(self.mstate.data_ptr(), self.Dsp, mx.Ds, self.d_b1, mx.Em, self.mrows, hp.ws["hyper_w1"].slabs, gk, gb,
                   1.0 / self.grad_scale, False)

    def _loss(self, n: int, k: int, q: torch.Tensor, qn: torch.Tensor) -> None:
        """The TD loss of Q_tot: the mixer's states and hypernetworks (qmix), mava_qmix_td_f32 - dLoss/dQ per agent into
        ws.dy, the hypernetwork outputs' gradients into d_* - and the hypernetworks' backward into g[Pq:]."""
        L_, s = lib(), stream_ptr()
        Lq, Rp, sm = self.L, self.Rp, self.smp
        hyper: List[Optional[int]] = [None] * 8  # vdn: no hypernetwork outputs
        grads: List[Optional[int]] = [None] * 4
        if self.mixer is not None:
            pm, pmt = self.p[self.Pq :], self.pt[self.Pq :]
            launch("qmix_state", L_.mava_qmix_state_t32_f32, Lq, self.B, self.A, self.O, Rp, self.Dsp, ptr(sm.obs[0]),
                   ptr(sm.next_obs[0]), ptr(self.mstate), ptr(self.mstate_next), s)
            on = self._hyper_forward(pm, self.hp, self.mstate)
            tg = self._hyper_forward(pmt, self.hp_target, self.mstate_next)
            order = ("hyper_w1", "hyper_b1", "hyper_w2", "hyper_b2")
            hyper = [ptr(on[k_]) for k_ in order] + [ptr(tg[k_]) for k_ in order]
            grads = [ptr(self.d_w1), ptr(self.d_b1), ptr(self.d_w2), ptr(self.d_b2)]
        launch("qmix_td", L_.mava_qmix_td_f32, int(self.mixer is not None), Lq, self.B, self.A, Rp, self.nA, self.Em, ptr(q), ptr(qn),
               ptr(self.q_target), ptr(sm.action), ptr(sm.reward), ptr(sm.terminal[1:]), ptr(sm.next_obs[1]), *hyper, self.gamma,
               self.grad_scale, ptr(self.ws.dy), *grads, ptr(self.partials), self.td_blocks, s)
        ops.slab_reduce(self.partials, 3, self.train_metrics[n, k])
        if self.mixer is not None:
            self._hyper_backward(self.p[self.Pq :], self.g[self.Pq :])

    # ---------------------------------------------------------------------------- state views
    def _param_tree(self, flat: torch.Tensor, lead: Tuple[int, ...]) -> Dict[str, Any]:
        return {"q_network": self.q_network.tree(flat[: self.Pq], lead),
                "mixer": self.mixer.tree(flat[self.Pq :], lead) if self.mixer is not None else {}}

    def learner_state(self) -> LearnerState:
        st = super().learner_state()
        lead = (1, 1)
        opt = st.opt_state._replace(mu=self._param_tree(self.m, lead), nu=self._param_tree(self.v, lead))
        return st._replace(params=QNetParams(self._param_tree(self.p, lead), self._param_tree(self.pt, lead)), opt_state=opt)

    def adopt(self, state: LearnerState) -> None:
        leaf = state.params.online["q_network"]["params"]["pre_torso"]["Dense_0"]["kernel"]
        if not isinstance(leaf, torch.Tensor) or leaf.data_ptr() != self.p.data_ptr():
            for tree, flat in ((state.params.online, self.p), (state.params.target, self.pt)):
                tree = tree_to(tree, self.p.device)
                self.q_network.flat_from_tree(tree["q_network"], flat[: self.Pq])
                if self.mixer is not None:
                    self.mixer.flat_from_tree(tree["mixer"], flat[self.Pq :])


class MixedQNetwork:
    """What the evaluator is handed: the recurrent Q network reading the `q_network` branch of the learner's parameter
    trees (evaluation is greedy per agent and never touches the mixer)."""

    def __init__(self, q_network):
        self.q_network = q_network

    def apply(self, params: Any, hstate: torch.Tensor, observation_done, eps: float = 0.0):
        p = params["q_network"] if isinstance(params, dict) and "q_network" in params else params
        return self.q_network.apply(p, hstate, observation_done, eps)


def learner_setup(env, keys, config, device=None):
    """(learn, q_network, initial LearnerState), as mava_amd/iql_learner.py::learner_setup."""
    key, q_key = int(keys[0]), int(keys[1])
    learner = QMIXLearner(env, config, device)
    learner.seed = key
    learner.init_params(q_key)
    learner.reset_envs()
    return bind_learn(learner), MixedQNetwork(learner.q_network), learner.learner_state()
