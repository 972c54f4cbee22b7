"""TEST INFRASTRUCTURE: float64 restatement of rec_qmix / rec_vdn as mava_amd/qmix_learner.py runs them, built like
tests/iql_model.py: oracle.rec_oracle.t_rec_forward + torch autograd for the Q network, plain torch for the mixer,
oracle.ppo_oracle.clip_adam, and IQLModel for everything that is rec_iql's (acting, replay, sampler, epsilon).

Flat parameters: [q_network (oracle.rec_oracle layout) | mixer], the mixer being [w1 net | b1 dense | w2 net | b2 net]
with every net [Dense_0 kernel (K x N) | bias | Dense_1 kernel | bias] and b1 [kernel (Ds x Em) | bias].
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import rec_oracle as ro
from oracle.ppo_oracle import clip_adam
from tests import iql_model as qm

H = 128


def mixer_shapes(Ds: int, A: int, Em: int, Hh: int):
    """[(name, shape)] in flat order."""
    return [("w1_k0", (Ds, Hh)), ("w1_b0", (Hh,)), ("w1_k1", (Hh, A * Em)), ("w1_b1", (A * Em,)),
            ("b1_k", (Ds, Em)), ("b1_b", (Em,)),
            ("w2_k0", (Ds, Hh)), ("w2_b0", (Hh,)), ("w2_k1", (Hh, Em)), ("w2_b1", (Em,)),
            ("b2_k0", (Ds, Em)), ("b2_b0", (Em,)), ("b2_k1", (Em, 1)), ("b2_b1", (1,))]


def mixer_param_count(Ds: int, A: int, Em: int, Hh: int) -> int:
    return sum(int(np.prod(s)) for _, s in mixer_shapes(Ds, A, Em, Hh))


def unpack(flat: torch.Tensor, Ds: int, A: int, Em: int, Hh: int) -> dict:
    out, off = {"A": A, "Em": Em}, 0
    for name, shape in mixer_shapes(Ds, A, Em, Hh):
        n = int(np.prod(shape))
        out[name] = flat[off : off + n].view(shape)
        off += n
    assert off == flat.numel(), (off, flat.numel())
    return out


def hyper(p: dict, state: torch.Tensor):
    """The four hypernetworks' raw (pre-abs) outputs for state (..., Ds)."""
    relu = torch.relu
    w1 = relu(state @ p["w1_k0"] + p["w1_b0"]) @ p["w1_k1"] + p["w1_b1"]
    b1 = state @ p["b1_k"] + p["b1_b"]
    w2 = relu(state @ p["w2_k0"] + p["w2_b0"]) @ p["w2_k1"] + p["w2_b1"]
    b2 = relu(state @ p["b2_k0"] + p["b2_b0"]) @ p["b2_k1"] + p["b2_b1"]
    return w1, b1, w2, b2


def mix_raw(qa: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, with_pre: bool = False):
    """Q_tot (...) from qa (..., A) and raw hypernet outputs w1 (..., A * Em), b1 / w2 (..., Em), b2 (..., 1)."""
    A, Em = qa.shape[-1], b1.shape[-1]
    w1 = w1.abs().reshape(*w1.shape[:-1], A, Em)
    pre = (qa.unsqueeze(-1) * w1).sum(-2) + b1
    hidden = torch.where(pre > 0, pre, torch.expm1(torch.clamp(pre, max=0.0)))  # elu, alpha 1
    tot = (hidden * w2.abs()).sum(-1) + b2[..., 0]
    return (tot, pre) if with_pre else tot


def mix(params, qa: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """Q_tot = mix(Q_1..Q_A, state); params None: vdn, the plain sum."""
    if params is None:
        return qa.sum(-1)
    return mix_raw(qa, *hyper(params, state))


def qmix_loss_grad(online, target, din, nA, smp, L, B, A, gamma, mixer, Em=0, Hh=0):
    """TD loss through the mixer on a sampled batch: (q_loss, mean_q, mean_target, flat gradient of [q | mixer], tie rows).
    Windows and indexing as iql_model.q_loss_grad."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n_real = B * A
    Pq, Ds = ro.rec_param_count(din, nA), A * din
    x, nx = t(smp["obs"][:L, :n_real]).double(), t(smp["next_obs"][:L, :n_real]).double()
    d_first, d_next = t(smp["tot"][:L, :n_real]).bool(), t(smp["tot"][1 : L + 1, :n_real]).bool()
    h0 = torch.zeros((n_real, H), dtype=torch.float64)
    p = t(np.asarray(online, np.float64)).clone().requires_grad_(True)
    pt = t(np.asarray(target, np.float64))
    state, next_state = x.reshape(L, B, Ds), nx.reshape(L, B, Ds)
    mp = unpack(p[Pq:], Ds, A, Em, Hh) if mixer == "qmix" else None
    mpt = unpack(pt[Pq:], Ds, A, Em, Hh) if mixer == "qmix" else None
    with torch.no_grad():
        qn, _ = ro.t_rec_forward(p[:Pq].detach(), din, nA, nx, d_next, h0)
        qt, _ = ro.t_rec_forward(pt[:Pq], din, nA, nx, d_next, h0)
        mask = t(smp["next_mask"][:L, :n_real]).bool()
        z = torch.where(mask, qn, torch.full_like(qn, float(qm.F32_MIN)))
        a_star = z.argmax(-1)
        if nA > 1:
            top2 = z.topk(2, -1).values
            ties = (top2[..., 0] - top2[..., 1]) < 1e-6
        else:
            ties = torch.zeros_like(a_star, dtype=torch.bool)
        next_q = qt.gather(-1, a_star.unsqueeze(-1)).squeeze(-1).reshape(L, B, A)
        q_tot_target = mix(mpt, next_q, next_state)
        reward = t(smp["reward"][:L, :n_real]).double().reshape(L, B, A).mean(-1)
        terminal = t(smp["terminal"][1 : L + 1, :n_real]).double().reshape(L, B, A)[..., 0]
        y = reward + (1.0 - terminal) * gamma * q_tot_target
    q, _ = ro.t_rec_forward(p[:Pq], din, nA, x, d_first, h0)
    qa = q.gather(-1, t(smp["action"][:L, :n_real]).long().unsqueeze(-1)).squeeze(-1).reshape(L, B, A)
    q_tot = mix(mp, qa, state)
    loss = ((q_tot - y) ** 2).mean()
    loss.backward()
    return float(loss.detach()), float(q_tot.detach().mean()), float(y.mean()), p.grad.numpy().copy(), ties.numpy()


class QMIXModel(qm.IQLModel):
    """IQLModel with the value-decomposition train step; `flat` is [q_network | mixer]."""

    def __init__(self, p, cfg, flat, env_state, obs, env_seed, env_offset, seed):
        super().__init__(p, cfg, flat, env_state, obs, env_seed, env_offset, seed)
        s = cfg.system
        self.mixer, self.Em, self.Hh = str(s.mixer), int(s.mixer_embed_dim), int(s.hypernet_hidden_dim)
        self.Pq = ro.rec_param_count(self.O, self.nA)
        want = self.Pq + (mixer_param_count(self.A * self.O, self.A, self.Em, self.Hh) if self.mixer == "qmix" else 0)
        assert self.online.size == want, (self.online.size, want)

    def act(self, gpu_action=None):
        full = self.online
        self.online = full[: self.Pq]  # acting reads the Q network alone
        try:
            return super().act(gpu_action)
        finally:
            self.online = full

    def train(self):
        smp, pairs = self.replay.sample(self.seed, self.t_train, self.B, self.S, self.Rp)
        loss, mq, mt, grad, ties = qmix_loss_grad(self.online, self.target, self.O, self.nA, smp, self.L, self.B, self.A, self.gamma,
                                                  self.mixer, self.Em, self.Hh)
        self.online, self.m, self.v, self.count = clip_adam(self.online, grad, self.m, self.v, self.count, self.lr, self.max_norm)
        if self.hard:
            if self.t_train % self.period == 0:
                self.target = self.online.copy()
        else:
            self.target = self.tau * self.online + (1.0 - self.tau) * self.target
        self.t_train += 1
        return {"q_loss": loss, "mean_q": mq, "mean_target": mt, "grad": grad, "pairs": pairs, "ties": ties}
