"""TEST INFRASTRUCTURE: float64 restatement of rec_iql (mava/systems/q_learning/rec_iql.py) as mava_amd/iql_learner.py
runs it, built from the existing oracles: oracle.rec_oracle.t_rec_forward (+ torch autograd) for the Q network,
oracle.ppo_oracle.clip_adam, oracle.philox for the exploration and sampler draws and tests/lbf_model.py for the env (its
pre-reset observation captured by wrapping lbf_model._regenerate from here, the model file itself unchanged).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from oracle import philox as ph
from oracle import rec_oracle as ro
from oracle.ppo_oracle import clip_adam
from tests import lbf_model as lm

QEPS_STREAM = 0x51455053  # "QEPS"
REPLAY_STREAM = 0x5242534D  # "RBSM"
F32_MIN = -np.finfo(np.float32).max
H = 128


def _key(seed: int):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def eps_greedy(q, mask, eps: float, seed: int, step: int, row_offset: int = 0):
    """MaskedEpsGreedyDistribution sampled as mava_rec_q_step_f32 does: (actions, greedy actions)."""
    mask = np.asarray(mask).astype(bool)
    R = q.shape[0]
    greedy = np.where(mask, q, F32_MIN).argmax(-1)
    nvalid = mask.sum(-1).astype(np.uint64)
    gid = (np.arange(R, dtype=np.uint64) + np.uint64(row_offset)).astype(np.uint32)
    x, y, _, _ = ph.philox4x32_10(gid, step, 0, QEPS_STREAM, *_key(seed))
    explore = (nvalid > 0) & (ph.u01_open(x) < np.float32(eps))
    k = (y.astype(np.uint64) * nvalid) >> np.uint64(32)
    pick = np.argmax((np.cumsum(mask, -1) - 1 == k[:, None].astype(np.int64)) & mask, -1)
    return np.where(explore, pick, greedy), greedy


def windows(seed: int, counter: int, B: int, E: int, cap: int, n_added: int, S: int):
    """(env, start slot) of the B sampled windows (mava_replay_sample_f32)."""
    filled = min(n_added, cap)
    assert filled >= S
    x, y, _, _ = ph.philox4x32_10(np.arange(B, dtype=np.uint32), counter, 0, REPLAY_STREAM, *_key(seed))
    env = (x.astype(np.uint64) * np.uint64(E)) >> np.uint64(32)
    k = (y.astype(np.uint64) * np.uint64(filled - S + 1)) >> np.uint64(32)
    start = (np.uint64(n_added - filled) + k) % np.uint64(cap)
    return env.astype(np.int64), start.astype(np.int64)


@contextlib.contextmanager
def capture_real(store: dict):
    """Record the observation / termination of the state lbf_model.step hands to _regenerate (before any reset)."""
    orig = lm._regenerate

    def wrapped(p, st, envs, seed, env_offset, t):
        o = lm.observe(p, st)
        store["agents_view"], store["action_mask"] = o["agents_view"], o["action_mask"]
        store["terminated"] = (st["food_alive"] == 0).all(-1).astype(np.uint8)
        orig(p, st, envs, seed, env_offset, t)

    lm._regenerate = wrapped
    try:
        yield store
    finally:
        lm._regenerate = orig


def lbf_step_real(p, st, action, seed, env_offset, t):
    """lbf_model.step plus (real_view, real_mask, terminated)."""
    store: dict = {}
    with capture_real(store):
        out = lm.step(p, st, action, seed, env_offset, t)
    return out, store


class Replay:
    """The (E, capacity, A, ...) buffer of mava_replay_add_f32 / mava_replay_sample_f32."""

    def __init__(self, E, A, O, nA, cap):
        self.E, self.A, self.cap = E, A, cap
        self.f = {"obs": np.zeros((E, cap, A, O), np.float32), "mask": np.zeros((E, cap, A, nA), np.uint8),
                  "action": np.zeros((E, cap, A), np.int32), "reward": np.zeros((E, cap, A), np.float32),
                  "terminal": np.zeros((E, cap, A), np.uint8), "tot": np.zeros((E, cap, A), np.uint8),
                  "next_obs": np.zeros((E, cap, A, O), np.float32), "next_mask": np.zeros((E, cap, A, nA), np.uint8)}
        self.n_added = 0

    def add(self, obs, mask, action, reward, terminal_env, tot, next_obs, next_mask):
        s = self.n_added % self.cap
        for k, v in (("obs", obs), ("mask", mask), ("action", action), ("reward", reward), ("tot", tot),
                     ("next_obs", next_obs), ("next_mask", next_mask)):
            self.f[k][:, s] = np.asarray(v).reshape(self.f[k][:, s].shape)
        self.f["terminal"][:, s] = np.repeat(np.asarray(terminal_env, np.uint8).reshape(self.E, 1), self.A, 1)
        self.n_added += 1

    def sample(self, seed, counter, B, S, Rp):
        env, start = windows(seed, counter, B, self.E, self.cap, self.n_added, S)
        out = {}
        for k, v in self.f.items():
            tail = v.shape[3:]
            o = np.zeros((S, Rp) + tail, v.dtype)
            for b in range(B):
                slots = (start[b] + np.arange(S)) % self.cap
                o[:, b * self.A : (b + 1) * self.A] = v[env[b], slots]
            if k == "tot":
                o[:, B * self.A :] = 1
            out[k] = o
        return out, np.stack([env, start], -1).astype(np.int32)


def q_loss_grad(online, target, din, nA, smp, L, n_real, gamma):
    """Double-Q TD loss (rec_iql.py:325-410) on a sampled batch: (q_loss, mean_q, mean_target, flat gradient, tie rows)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x, nx = t(smp["obs"][:L, :n_real]).double(), t(smp["next_obs"][:L, :n_real]).double()
    d_first, d_next = t(smp["tot"][:L, :n_real]).bool(), t(smp["tot"][1 : L + 1, :n_real]).bool()
    h0 = torch.zeros((n_real, H), dtype=torch.float64)
    p = t(np.asarray(online, np.float64)).clone().requires_grad_(True)
    with torch.no_grad():
        qn, _ = ro.t_rec_forward(p.detach(), din, nA, nx, d_next, h0)
        qt, _ = ro.t_rec_forward(t(np.asarray(target, np.float64)), din, nA, nx, d_next, h0)
    mask = t(smp["next_mask"][:L, :n_real]).bool()
    z = torch.where(mask, qn, torch.full_like(qn, float(F32_MIN)))
    a_star = z.argmax(-1)
    top2 = z.topk(2, -1).values
    ties = (top2[..., 0] - top2[..., 1]) < 1e-6
    next_q = qt.gather(-1, a_star.unsqueeze(-1)).squeeze(-1)
    target_q = t(smp["reward"][:L, :n_real]).double() + (1.0 - t(smp["terminal"][1 : L + 1, :n_real]).double()) * gamma * next_q
    q, _ = ro.t_rec_forward(p, din, nA, x, d_first, h0)
    qa = q.gather(-1, t(smp["action"][:L, :n_real]).long().unsqueeze(-1)).squeeze(-1)
    loss = ((qa - target_q) ** 2).mean()
    loss.backward()
    return (float(loss), float(qa.mean()), float(target_q.mean()), p.grad.numpy().copy(), ties.numpy())


class IQLModel:
    """The learner's update loop in float64 from given parameters and env state."""

    def __init__(self, p: lm.Params, cfg, flat, env_state: dict, obs: dict, env_seed: int, env_offset: int, seed: int):
        s = cfg.system
        self.p, self.seed, self.env_seed, self.env_offset = p, int(seed), int(env_seed), int(env_offset)
        self.E, self.A, self.O, self.nA = int(cfg.arch.num_envs), p.A, p.obs_dim, lm.N_ACTIONS
        self.T, self.K, self.B, self.L = int(s.rollout_length), int(s.epochs), int(s.sample_batch_size), int(s.sample_sequence_length)
        self.S, self.cap = self.L + 1, int(s.buffer_size)
        self.min_fill = max(int(s.min_buffer_size), self.S)
        self.Rp = -(-(self.B * self.A) // 32) * 32
        self.gamma, self.tau, self.lr, self.max_norm = float(s.gamma), float(s.tau), float(s.q_lr), float(s.max_grad_norm)
        self.hard, self.period = bool(s.hard_update), int(s.update_period)
        self.eps_min, self.eps_decay = float(s.eps_min), float(s.eps_decay)
        self.online = np.asarray(flat, np.float64).copy()
        self.target = self.online.copy()
        self.m, self.v, self.count = np.zeros_like(self.online), np.zeros_like(self.online), 0
        self.st = {k: np.array(v, copy=True) for k, v in env_state.items()}
        EA = self.E * self.A
        self.view, self.mask = obs["agents_view"].reshape(EA, self.O).copy(), obs["action_mask"].reshape(EA, self.nA).copy()
        self.tot, self.term = np.zeros(EA, np.uint8), np.zeros(self.E, np.uint8)
        self.h = np.zeros((EA, H))
        self.replay = Replay(self.E, self.A, self.O, self.nA, self.cap)
        self.t_act = self.act_steps = self.t_train = 0

    def act(self, gpu_action=None):
        """One act step; returns (model action, greedy-tie rows).  With gpu_action, rows where the model's greedy choice
        is a near tie (top two within 1e-6) follow the GPU's action."""
        EA = self.E * self.A
        eps = max(self.eps_min, 1.0 - (self.t_act / self.eps_decay) * (1.0 - self.eps_min))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        y, h = ro.t_rec_forward(t(self.online), self.O, self.nA, t(self.view[None]).double(), t(self.tot[None]).bool(), t(self.h))
        q = y[0].numpy()
        action, greedy = eps_greedy(q, self.mask, np.float32(eps), self.seed, self.act_steps)
        z = np.sort(np.where(self.mask.astype(bool), q, F32_MIN), -1)
        ties = (z[:, -1] - z[:, -2]) < 1e-6
        if gpu_action is not None:
            g = np.asarray(gpu_action).reshape(EA)
            bad = (g != action) & ~ties
            assert not bad.any(), f"act step {self.act_steps}: actions differ at rows {np.nonzero(bad)[0][:5]}"
            action = np.where(ties, g, action)
        self.h = h.numpy()
        (obs, reward, done, _, _, _), real = lbf_step_real(self.p, self.st, action.reshape(self.E, self.A), self.env_seed,
                                                           self.env_offset, self.act_steps + 1)
        self.replay.add(self.view.reshape(self.E, self.A, self.O), self.mask.reshape(self.E, self.A, self.nA), action, reward,
                        self.term, self.tot, real["agents_view"], real["action_mask"])
        self.view, self.mask = obs["agents_view"].reshape(EA, self.O).copy(), obs["action_mask"].reshape(EA, self.nA).copy()
        self.tot, self.term = done.reshape(EA).copy(), real["terminated"].copy()
        self.t_act += self.E
        self.act_steps += 1
        return action, ties

    def train(self):
        smp, pairs = self.replay.sample(self.seed, self.t_train, self.B, self.S, self.Rp)
        loss, mq, mt, grad, ties = q_loss_grad(self.online, self.target, self.O, self.nA, smp, self.L, self.B * self.A, self.gamma)
        self.online, self.m, self.v, self.count = clip_adam(self.online, grad, self.m, self.v, self.count, self.lr, self.max_norm)
        if self.hard:
            if self.t_train % self.period == 0:
                self.target = self.online.copy()
        else:
            self.target = self.tau * self.online + (1.0 - self.tau) * self.target
        self.t_train += 1
        return {"q_loss": loss, "mean_q": mq, "mean_target": mt, "grad": grad, "pairs": pairs, "ties": ties}
