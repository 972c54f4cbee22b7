"""Multi-Agent Transformer learner (ff_mat; Wen et al. 2022, mava.systems.mat) behind Mava's LearnerFn contract.

The reference checkout has no MAT: nothing here is pinned against upstream; the contract is the float64 model in
tests/mat_model.py (DESIGN.md 3.25 says which upstream conventions were followed from memory).

Network (discrete actions).  One sample is one (t, env) pair with its A agents in order; D = network.n_embd.
  encoder:  x = LN(GELU(Dense(LN_O(obs))));  n_block x { x = LN(x + Attn(x, x));  x = LN(x + MLP(x)) };  rep = x;
            value = Dense(1)(LN(GELU(Dense(rep))))
  decoder:  x = LN(GELU(Dense_nobias(shifted one-hot)));  n_block x { x = LN(x + Attn(x, x, causal));
            x = LN(rep + Attn(q = rep, kv = x, causal));  x = LN(x + MLP(x)) };  logits = Dense(nA)(LN(GELU(Dense(x))))
Acting is autoregressive: A decoder passes per env step, pass i samples agent i (mava_mat_sample_f32) and the next pass
sees its action in the shifted one-hot.  Training is one teacher-forced pass.  With network.acting=fused an env step is one
launch instead (mava_transformer_act_f32, csrc/mat_act.hip: the same network with a key/value cache, f32 dense products
whatever system.matmul_mode); the bootstrap value and training stay on the layer-wise tapes.
With a ContinuousActionHead (network=continuous_transformer; float64 model tests/mat_continuous_model.py) the decoder's input is
the shifted ACTION VECTOR (row 0 zero, no start token; act_dense has a bias and runs in exact f32), head_out gives the d means of
Independent(TanhTransformed(Normal(mean, softplus(log_std) + min_scale))) and decoder/log_std is the flat vector's last leaf;
the three kernels are mava_transformer_shift_action_f32 / _sample_continuous_f32 / _loss_continuous_f32, the fused step
mava_transformer_act_continuous_f32.

Every matrix is T32 with the E * A (acting) or Bm * A (minibatch) agent rows padded to a multiple of 32; the dense products
are GenericNet._dense / _xty (mava_rec_dense_f32 / mava_rec_xty_f32: system.matmul_mode, grad_scale), everything between
them is csrc/mat.hip.  Forward and backward are one tape of layer objects: the backward pass walks it in reverse, a layer
writes the gradient of an input that has none yet and adds to one that has (the dense launch's `accumulate`), and the
residual input of a LayerNorm shares the gradient buffer of the branch it was added to.

Parameters: one flat vector [encoder | decoder], one global-norm clip and one Adam (ops.clip_adam, one segment).

MATLearner is the one-replica, one-segment case of PPOLearner (mava_amd/ppo_learner.py), which owns the replica buffers,
the constructor's prologue, the flat parameter storage with init_params / adopt, update(), the clip+Adam launch, learn() and
learner_setup(); the refusals, the network, the tapes and every launch of the rollout and of a minibatch are this module's.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import ops, ppo_learner
from ._lib import Ctx, MavaHipError, launch, lib, ptr, stream_ptr
from .generic_networks import GenericMLPTorso, GenericNet
from .learner_common import pad32
from .networks import _orthogonal_
from .ppo_learner import PPOLearner
from .types import LearnerState, TimeStep

MAX_AGENTS, MAX_EMBED, MAX_ACTIONS = 32, 128, 64  # csrc/mat.hip's limits
MAX_ACTION_DIM = 16  # ... and of its continuous head (csrc/tanh_normal.h's users)
ACTING = ("layerwise", "fused")  # network.acting: MATPass.act launches layer by layer, or csrc/mat_act.hip once per env step


def check_supported(*, num_agents: int, n_actions: int, n_embd: int, n_head: int, continuous: bool, world: int,
                    update_batch_size: int) -> None:
    """ff_mat's refusals: a MavaHipError with the reason, before anything is allocated or launched."""
    if continuous:
        raise MavaHipError("ff_mat: a continuous action head is not implemented (discrete actions only)")
    if not 1 <= num_agents <= MAX_AGENTS:
        raise MavaHipError(f"ff_mat: the attention kernels take 1..{MAX_AGENTS} agents, the environment has {num_agents}")
    if n_embd < 32 or n_embd % 32 or n_embd > MAX_EMBED:
        raise MavaHipError(f"ff_mat: network.n_embd must be a multiple of 32 up to {MAX_EMBED}, got {n_embd}")
    if n_head < 1 or n_embd % n_head:
        raise MavaHipError(f"ff_mat: network.n_embd={n_embd} must be a multiple of network.n_head={n_head}")
    if not 1 <= n_actions <= MAX_ACTIONS:
        raise MavaHipError(f"ff_mat: at most {MAX_ACTIONS} actions, the environment has {n_actions}")
    if world > 1:
        raise MavaHipError(f"ff_mat runs on one GPU, the process group has {world} ranks")
    if update_batch_size != 1:
        raise MavaHipError(f"ff_mat: system.update_batch_size must be 1, got {update_batch_size}")


def check_supported_continuous(*, num_agents: int, action_dim: int, n_embd: int, n_head: int, independent_std: bool, world: int,
                               update_batch_size: int) -> None:
    """ff_mat's refusals with a ContinuousActionHead (check_supported stays the discrete network's)."""
    if not 1 <= action_dim <= MAX_ACTION_DIM:
        raise MavaHipError(f"ff_mat: continuous actions of 1..{MAX_ACTION_DIM} dimensions, the environment has {action_dim}")
    if not independent_std:
        raise MavaHipError("ff_mat: ContinuousActionHead.independent_std=False is not implemented (one log_std vector only)")
    check_supported(num_agents=num_agents, n_actions=action_dim, n_embd=n_embd, n_head=n_head, continuous=False, world=world,
                    update_batch_size=update_batch_size)


def _attn_leaves(D: int) -> List[Tuple[Tuple[str, ...], Tuple[int, ...], Any]]:
    out = []
    for name in ("query", "key", "value", "proj"):
        out += [((name, "kernel"), (D, D), math.sqrt(2.0)), ((name, "bias"), (D,), 0.0)]
    return out


def _ln_leaves(name: str, N: int):
    return [((name, "scale"), (N,), "ones"), ((name, "bias"), (N,), 0.0)]


def _dense_leaves(name: str, K: int, N: int, scale: float, bias: bool = True):
    out = [((name, "kernel"), (K, N), scale)]
    return out + ([((name, "bias"), (N,), 0.0)] if bias else [])


def param_spec(O: int, nA: int, D: int, n_block: int, continuous: bool = False):
    """[(tree path, shape, init)] of the flat vector [encoder | decoder]; init: an orthogonal scale, 0.0 or "ones".
    continuous (nA = the action dimension): act_dense reads the nA-wide action vector and has a bias, head_out gives the nA
    means, and decoder/log_std (nA zeros) is the last leaf."""
    r2 = math.sqrt(2.0)
    enc = _ln_leaves("obs_ln", O) + _dense_leaves("obs_dense", O, D, r2) + _ln_leaves("ln", D)
    for i in range(n_block):
        b = f"block_{i}"
        blk = [(("attn",) + p, s, k) for p, s, k in _attn_leaves(D)] + _ln_leaves("ln1", D)
        blk += _dense_leaves("mlp_0", D, D, r2) + _dense_leaves("mlp_1", D, D, r2) + _ln_leaves("ln2", D)
        enc += [((b,) + p, s, k) for p, s, k in blk]
    enc += _dense_leaves("head_dense", D, D, r2) + _ln_leaves("head_ln", D) + _dense_leaves("head_out", D, 1, 0.01)
    dec = (_dense_leaves("act_dense", nA, D, r2) if continuous else _dense_leaves("act_dense", nA + 1, D, r2, bias=False)) + _ln_leaves("ln", D)
    for i in range(n_block):
        b = f"block_{i}"
        blk = [(("attn1",) + p, s, k) for p, s, k in _attn_leaves(D)] + _ln_leaves("ln1", D)
        blk += [(("attn2",) + p, s, k) for p, s, k in _attn_leaves(D)] + _ln_leaves("ln2", D)
        blk += _dense_leaves("mlp_0", D, D, r2) + _dense_leaves("mlp_1", D, D, r2) + _ln_leaves("ln3", D)
        dec += [((b,) + p, s, k) for p, s, k in blk]
    dec += _dense_leaves("head_dense", D, D, r2) + _ln_leaves("head_ln", D) + _dense_leaves("head_out", D, nA, 0.01)
    if continuous:
        dec += [(("log_std",), (nA,), 0.0)]
    return [(("encoder",) + p, s, k) for p, s, k in enc] + [(("decoder",) + p, s, k) for p, s, k in dec]


class MATParams(dict):
    """{"encoder": ..., "decoder": ...}.  The experiment driver and the evaluator address the acting parameters of a
    system as `params.actor_params`: for MAT that is the whole tree."""

    @property
    def actor_params(self) -> "MATParams":
        return self


class MATNet:
    """Shapes, flat layout and trees of the network."""

    def __init__(self, O: int, nA: int, A: int, D: int, n_head: int, n_block: int, *, continuous: bool = False,
                 min_scale: float = 1e-3):
        """continuous: nA is the action dimension of a ContinuousActionHead with scale = softplus(log_std) + min_scale."""
        self.O, self.nA, self.A, self.D, self.H, self.n_block = int(O), int(nA), int(A), int(D), int(n_head), int(n_block)
        self.continuous, self.min_scale = bool(continuous), float(min_scale)
        self.spec = param_spec(self.O, self.nA, self.D, self.n_block, self.continuous)
        self.off: Dict[Tuple[str, ...], int] = {}
        off = 0
        for path, shape, _ in self.spec:
            self.off[path], off = off, off + math.prod(shape)
        self.num_params = off

    def init_flat(self, seed: int) -> torch.Tensor:
        gen = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        flat = torch.zeros(self.num_params, dtype=torch.float32)
        for path, shape, init in self.spec:
            v = flat[self.off[path] : self.off[path] + math.prod(shape)].view(shape)
            if init == "ones":
                v.fill_(1.0)
            elif init != 0.0:
                _orthogonal_(v, float(init), gen)
        return flat

    def tree(self, flat: torch.Tensor, lead: Tuple[int, ...] = ()) -> MATParams:
        out = MATParams()
        for path, shape, _ in self.spec:
            node = out
            for k in path[:-1]:
                node = node.setdefault(k, {})
            v = flat[self.off[path] : self.off[path] + math.prod(shape)].view(shape)
            node[path[-1]] = v.expand(*lead, *shape) if lead else v
        return out

    def flat_from_tree(self, tree: Dict[str, Any], out: torch.Tensor) -> torch.Tensor:
        for path, shape, _ in self.spec:
            leaf = tree
            for k in path:
                leaf = leaf[k]
            leaf = torch.as_tensor(leaf)
            while leaf.dim() > len(shape):
                leaf = leaf[0]
            out[self.off[path] : self.off[path] + math.prod(shape)].view(shape).copy_(leaf)
        return out

    def first_leaf(self, tree: Dict[str, Any]) -> torch.Tensor:
        return tree["encoder"]["obs_ln"]["scale"]


class _Buf:
    """A T32 (rows x N) matrix with `ld` features per tile, and its gradient during a backward pass."""

    def __init__(self, rows: int, N: int, device, ld: Optional[int] = None, t: Optional[torch.Tensor] = None):
        self.rows, self.N, self.ld = rows, N, int(ld or N)
        self.t = t if t is not None else torch.zeros(rows * self.ld, device=device)
        self.grad: Optional[torch.Tensor] = None
        self._own: Optional[torch.Tensor] = None

    def own(self) -> torch.Tensor:
        if self._own is None:
            self._own = torch.zeros(self.rows * self.N, device=self.t.device)
        return self._own


class _Graph:
    """The tape of one pass shape: `rows` padded agent rows of B samples.  add_* append a layer and return its output."""

    def __init__(self, net: MATNet, B: int, device, training: bool, ctx):
        self.net, self.B, self.A, self.training, self.device = net, int(B), net.A, training, device
        self.valid = self.B * self.A
        self.rows = pad32(self.valid)
        self.nblk = max(1, min(256, self.rows // 32))
        self.prod = GenericNet(GenericMLPTorso([net.D]), net.D, [])  # the product launches of the general layer path
        self.prod.ctx = ctx
        self._prod32: Optional[GenericNet] = None
        self.bufs: List[_Buf] = []
        if training:
            self.slabs = torch.zeros((self.nblk, 128 * 128 + 128 + 8), device=device)
            self.ln_slab = torch.zeros((self.nblk, 2 * max(net.O, net.D)), device=device)

    def buf(self, N: int, ld: Optional[int] = None) -> _Buf:
        b = _Buf(self.rows, N, self.device, ld)
        self.bufs.append(b)
        return b

    def _p(self, flat: torch.Tensor, path: Tuple[str, ...], n: int) -> torch.Tensor:
        o = self.net.off[path]
        return flat[o : o + n]

    def _exact(self) -> GenericNet:
        """The product launches in exact f32 whatever system.matmul_mode (a context of their own)."""
        if self._prod32 is None:
            self._prod32 = GenericNet(GenericMLPTorso([self.net.D]), self.net.D, [])
            self._prod32.ctx = Ctx("f32")
        return self._prod32

    # ---- layers: (forward closure, backward closure) pairs appended to a tape
    def dense(self, tape, x: _Buf, path: Tuple[str, ...], K: int, N: int, bias: bool = True, x_grad: bool = True,
              exact: bool = False) -> _Buf:
        y = self.buf(N)
        wp, bp = path + ("kernel",), path + ("bias",)
        prod = self._exact() if exact else self.prod

        def fwd(flat):
            prod._dense(x.t.data_ptr(), x.ld, K, self._p(flat, wp, K * N), self._p(flat, bp, N) if bias else None, y.t, N,
                             self.rows, what="mat_dense")

        def bwd(flat, g, inv):
            prod._xty(x.t.data_ptr(), x.ld, K, y.grad, N, self.rows, self.slabs, self._p(g, wp, K * N),
                           self._p(g, bp, N) if bias else None, inv, False)
            if not x_grad:
                return
            wt = self._p(flat, wp, K * N).view(K, N).t().contiguous()
            first = x.grad is None
            if first:
                x.grad = x.own()
            prod._dense(y.grad.data_ptr(), N, N, wt, None, x.grad, K, self.rows, accumulate=not first, what="mat_dense_bwd")

        tape.append((fwd, bwd))
        return y

    def ln(self, tape, x: _Buf, res: Optional[_Buf], path: Tuple[str, ...], N: int) -> _Buf:
        y = self.buf(N)
        xhat = torch.zeros(self.rows * N, device=self.device) if self.training else None
        rstd = torch.zeros(self.rows, device=self.device) if self.training else None
        sp, bp = path + ("scale",), path + ("bias",)
        L = lib()

        def fwd(flat):
            launch("mat_ln", L.mava_mat_ln_fwd_f32, ptr(x.t), ptr(res.t) if res is not None else None, ptr(self._p(flat, sp, N)),
                   ptr(self._p(flat, bp, N)), N, self.rows, self.valid, ptr(y.t), ptr(xhat), ptr(rstd), self.nblk, stream_ptr())

        def bwd(flat, g, inv):
            assert x.grad is None, "a LayerNorm's main input has one consumer"
            x.grad = x.own()
            launch("mat_ln_bwd", L.mava_mat_ln_bwd_f32, ptr(y.grad), ptr(xhat), ptr(rstd), ptr(self._p(flat, sp, N)), N, self.rows,
                   self.valid, inv, ptr(x.grad), ptr(self.ln_slab), self.ln_slab.shape[1], self.ln_slab.shape[0], stream_ptr())
            ops.slab_reduce(self.ln_slab, N, self._p(g, sp, N))
            ops.slab_reduce_cols(self.ln_slab, N, N, self._p(g, bp, N))
            if res is not None:
                if res.grad is None:
                    res.grad = x.grad  # d(x + res): one buffer serves both (x's producer reads it before res's others add)
                else:
                    res.grad.add_(x.grad)

        tape.append((fwd, bwd))
        return y

    def gelu(self, tape, x: _Buf) -> _Buf:
        y = self.buf(x.N)
        n = self.rows * x.N
        L = lib()

        def fwd(flat):
            launch("mat_gelu", L.mava_mat_gelu_f32, ptr(x.t), n, ptr(y.t), stream_ptr())

        def bwd(flat, g, inv):
            assert x.grad is None
            x.grad = x.own()
            launch("mat_gelu_bwd", L.mava_mat_gelu_bwd_f32, ptr(y.grad), ptr(x.t), n, ptr(x.grad), stream_ptr())

        tape.append((fwd, bwd))
        return y

    def attention(self, tape, q_in: _Buf, kv_in: _Buf, path: Tuple[str, ...], causal: bool) -> _Buf:
        D, H, A = self.net.D, self.net.H, self.A
        q = self.dense(tape, q_in, path + ("query",), D, D)
        k = self.dense(tape, kv_in, path + ("key",), D, D)
        v = self.dense(tape, kv_in, path + ("value",), D, D)
        y = self.buf(D)
        L = lib()

        def fwd(flat):
            launch("mat_attn", L.mava_mat_attn_fwd_f32, ptr(q.t), ptr(k.t), ptr(v.t), self.rows, D, self.B, A, H, int(causal), ptr(y.t),
                   None, self.nblk, stream_ptr())

        def bwd(flat, g, inv):
            for b in (q, k, v):
                assert b.grad is None
                b.grad = b.own()
            launch("mat_attn_bwd", L.mava_mat_attn_bwd_f32, ptr(y.grad), ptr(q.t), ptr(k.t), ptr(v.t), self.rows, D, self.B, A, H,
                   int(causal), ptr(q.grad), ptr(k.grad), ptr(v.grad), self.nblk, stream_ptr())

        tape.append((fwd, bwd))
        return self.dense(tape, y, path + ("proj",), D, D)

    def mlp(self, tape, x: _Buf, base: Tuple[str, ...]) -> _Buf:
        D = self.net.D
        return self.dense(tape, self.gelu(tape, self.dense(tape, x, base + ("mlp_0",), D, D)), base + ("mlp_1",), D, D)

    def head(self, tape, x: _Buf, base: Tuple[str, ...], n_out: int) -> _Buf:
        D = self.net.D
        h = self.ln(tape, self.gelu(tape, self.dense(tape, x, base + ("head_dense",), D, D)), None, base + ("head_ln",), D)
        return self.dense(tape, h, base + ("head_out",), D, n_out)


class MATPass(_Graph):
    """Encoder and decoder tapes for B samples, with the gathered observations and the shifted one-hot as inputs."""

    def __init__(self, net: MATNet, B: int, device, training: bool, ctx, acting: str = "layerwise"):
        super().__init__(net, B, device, training, ctx)
        O, nA, D = net.O, net.nA, net.D
        if acting not in ACTING:
            raise MavaHipError(f"ff_mat: network.acting must be one of {ACTING}, got {acting!r}")
        self.acting = acting
        self._act_ws: Optional[torch.Tensor] = None  # the fused step's workspace (its key/value cache), once per pass shape
        if acting == "fused":
            self._act_blocks = max(1, min(256, -(-self.B // max(1, 32 // net.A))))  # one block per group of samples
            need = int(lib().mava_transformer_act_workspace_bytes(self.B, net.A, D, net.n_block, self._act_blocks))
            self._act_ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=device)
        n_in = nA if net.continuous else nA + 1  # the decoder's input: the previous action vector, or [start | one-hot]
        self.Np = pad32(n_in)
        self.obs = self.buf(O)
        self.onehot = self.buf(n_in, ld=self.Np)
        # sample ids of the rows, padded with sample 0 so that the gather of the padding rows stays inside the source
        self.idx = torch.zeros(-(-self.rows // self.A) + 1, dtype=torch.int32, device=device)
        enc: list = []
        e = self.gelu(enc, self.dense(enc, self.ln(enc, self.obs, None, ("encoder", "obs_ln"), O), ("encoder", "obs_dense"), O, D))
        x = self.ln(enc, e, None, ("encoder", "ln"), D)
        for i in range(net.n_block):
            b = ("encoder", f"block_{i}")
            x = self.ln(enc, self.attention(enc, x, x, b + ("attn",), False), x, b + ("ln1",), D)
            x = self.ln(enc, self.mlp(enc, x, b), x, b + ("ln2",), D)
        self.rep = x
        self.value = self.head(enc, x, ("encoder",), 1)
        dec: list = []
        x = self.ln(dec, self.gelu(dec, self.dense(dec, self.onehot, ("decoder", "act_dense"), n_in, D, bias=net.continuous, x_grad=False,
                                                   exact=net.continuous)), None, ("decoder", "ln"), D)
        for i in range(net.n_block):
            b = ("decoder", f"block_{i}")
            x = self.ln(dec, self.attention(dec, x, x, b + ("attn1",), True), x, b + ("ln1",), D)
            x = self.ln(dec, self.attention(dec, self.rep, x, b + ("attn2",), True), self.rep, b + ("ln2",), D)
            x = self.ln(dec, self.mlp(dec, x, b), x, b + ("ln3",), D)
        self.logits = self.head(dec, x, ("decoder",), nA)
        self.enc, self.dec = enc, dec

    def gather_obs(self, agents_view: torch.Tensor, n_samples: int) -> None:
        """agents_view: (n_samples, A, O) row-major; row b * A + j of the pass reads sample idx[b]."""
        net = self.net
        launch("mat_gather", lib().mava_rec_gather_t32_f32, ptr(agents_view), ptr(self.idx), self.rows, n_samples, net.A, 1, net.O, net.O,
               self.rows, net.O, ptr(self.obs.t), stream_ptr())

    def shift_onehot(self, action: torch.Tensor, known: int, use_idx: bool) -> None:
        """The decoder's input from the first `known` agents' actions: shifted one-hots, or the shifted action vectors."""
        if self.net.continuous:
            launch("mat_shift_action", lib().mava_transformer_shift_action_f32, ptr(action), ptr(self.idx) if use_idx else None, self.B,
                   self.A, self.net.nA, known, self.rows, self.Np, ptr(self.onehot.t), stream_ptr())
            return
        launch("mat_onehot", lib().mava_mat_shift_onehot_f32, ptr(action), ptr(self.idx) if use_idx else None, self.B, self.A,
               self.net.nA, known, self.rows, self.Np, ptr(self.onehot.t), stream_ptr())

    def encode(self, flat: torch.Tensor) -> None:
        for fwd, _ in self.enc:
            fwd(flat)

    def decode(self, flat: torch.Tensor) -> None:
        for fwd, _ in self.dec:
            fwd(flat)

    def backward(self, flat: torch.Tensor, g: torch.Tensor, dlogits: torch.Tensor, dvalues: torch.Tensor, grad_scale: float) -> None:
        for b in self.bufs:
            b.grad = None
        self.logits.grad, self.value.grad = dlogits, dvalues
        inv = 1.0 / grad_scale
        for _, bwd in reversed(self.enc + self.dec):
            bwd(flat, g, inv)

    def act(self, flat: torch.Tensor, agents_view: torch.Tensor, mask: torch.Tensor, action: torch.Tensor, log_prob: torch.Tensor,
            seed: int, step: int, row_offset: int, greedy: bool, value_out: Optional[torch.Tensor] = None) -> None:
        """One env step for the B samples of (B, A, O) agents_view: encoder, then A decoder passes; pass i samples agent i.
        Launches: 1 + len(enc) + A * (2 + len(dec)) (+ 1 copy of the values); one when the pass was built with
        acting="fused" and the kernel takes the network's depth."""
        if self.acting == "fused" and self._act_fused(flat, agents_view, mask, action, log_prob, seed, step, row_offset, greedy,
                                                      value_out):
            return
        self.gather_obs(agents_view, self.B)
        self.encode(flat)
        if value_out is not None:
            value_out.view(-1).copy_(self.value.t[: self.valid])
        net = self.net
        for i in range(self.A):
            self.shift_onehot(action, i, False)
            self.decode(flat)
            if net.continuous:  # the logits buffer holds the means; the mask is not read
                launch("mat_sample_cont", lib().mava_transformer_sample_continuous_f32, self.B, self.A, i, net.nA, net.min_scale,
                       ptr(self.logits.t), ptr(self.log_std(flat)), seed & (2**64 - 1), step & 0xFFFFFFFF, row_offset & 0xFFFFFFFF,
                       int(greedy), ptr(action), ptr(log_prob), stream_ptr())
            else:
                launch("mat_sample", lib().mava_mat_sample_f32, self.B, self.A, i, net.nA, ptr(self.logits.t), ptr(mask),
                       seed & (2**64 - 1), step & 0xFFFFFFFF, row_offset & 0xFFFFFFFF, int(greedy), ptr(action), ptr(log_prob), stream_ptr())

    def log_std(self, flat: torch.Tensor) -> torch.Tensor:
        return self._p(flat, ("decoder", "log_std"), self.net.nA)

    def _act_fused(self, flat, agents_view, mask, action, log_prob, seed, step, row_offset, greedy, value_out) -> bool:
        """The env step as one launch; False when the kernel has no instance for this depth (the caller runs layer by layer)."""
        net, L = self.net, lib()
        if net.continuous:
            rc = launch("mat_act", L.mava_transformer_act_continuous_f32, ptr(flat), ptr(agents_view), self.B, net.A, net.O, net.nA, net.D,
                        net.H, net.n_block, net.min_scale, seed & (2**64 - 1), step & 0xFFFFFFFF, row_offset & 0xFFFFFFFF, int(greedy),
                        ptr(action), ptr(log_prob), ptr(value_out), ptr(self._act_ws), self._act_ws.numel(), self._act_blocks,
                        stream_ptr(), ok=(0, 1))
            return rc == 0
        rc = launch("mat_act", L.mava_transformer_act_f32, ptr(flat), ptr(agents_view), ptr(mask), self.B, net.A, net.O, net.nA, net.D,
                    net.H, net.n_block, seed & (2**64 - 1), step & 0xFFFFFFFF, row_offset & 0xFFFFFFFF, int(greedy), ptr(action),
                    ptr(log_prob), ptr(value_out), ptr(self._act_ws), self._act_ws.numel(), self._act_blocks, stream_ptr(), ok=(0, 1))
        return rc == 0


class _MATPolicy:
    """What MATActor.apply returns: the evaluator calls mode() or sample(seed=generator); either runs the autoregressive
    decode on the learner's acting path."""

    def __init__(self, actor: "MATActor", flat: torch.Tensor, observation):
        self.actor, self.flat, self.observation = actor, flat, observation

    def _run(self, greedy: bool, seed: int) -> torch.Tensor:
        return self.actor.act(self.flat, self.observation, greedy, seed)

    def mode(self) -> torch.Tensor:
        return self._run(True, 0)

    def sample(self, seed: Optional[torch.Generator] = None) -> torch.Tensor:
        s = int(torch.randint(0, 2**62, (1,), generator=seed, device=seed.device if seed is not None else "cpu").item())
        return self._run(False, s)


class MATActor:
    """actor_network of the system: apply(params, observation) -> a policy over the joint action (E, A)."""

    def __init__(self, net: MATNet, ctx, device, acting: str = "layerwise"):
        self.net, self.ctx, self.device, self.acting = net, ctx, device, acting
        self._passes: Dict[int, MATPass] = {}
        self._flat = torch.zeros(net.num_params, device=device)
        self._calls = 0

    def pass_for(self, B: int) -> MATPass:
        if B not in self._passes:
            p = MATPass(self.net, B, self.device, False, self.ctx, self.acting)
            p.idx[:B].copy_(torch.arange(B, dtype=torch.int32))
            self._passes[B] = p
        return self._passes[B]

    def apply(self, params: Any, observation) -> _MATPolicy:
        flat = params if isinstance(params, torch.Tensor) else self.net.flat_from_tree(params, self._flat)
        return _MATPolicy(self, flat, observation)

    def act(self, flat: torch.Tensor, observation, greedy: bool, seed: int) -> torch.Tensor:
        av = observation.agents_view
        B = int(av.shape[0])
        av = av.reshape(B, self.net.A, self.net.O).float().contiguous()
        mask = observation.action_mask.reshape(B, self.net.A, self.net.nA).to(torch.uint8).contiguous()
        if self.net.continuous:  # the (B, A, action_dim) f32 action vectors; the (all-ones) mask is not read
            action = torch.zeros((B, self.net.A, self.net.nA), device=av.device)
        else:
            action = torch.zeros((B, self.net.A), dtype=torch.int32, device=av.device)
        log_prob = torch.zeros((B, self.net.A), device=av.device)
        self.pass_for(B).act(flat, av, mask, action, log_prob, seed, self._calls, 0, greedy)
        self._calls += 1
        return action


class MATLearner(PPOLearner):
    def __init__(self, env, config, device: Optional[torch.device] = None):
        net = config.network
        self.D, self.H, self.n_block = int(net.get("n_embd", 64)), int(net.get("n_head", 1)), int(net.get("n_block", 1))
        self.acting = str(net.get("acting", "layerwise"))
        super().__init__(env, config, False, device)
        s, self.rep = config.system, self.reps[0]
        self.O = self.Oa  # (image observations: their flat row)
        if self.O > 1024:
            raise MavaHipError(f"ff_mat: observations of up to 1024 features (mava_rec_gather_t32_f32), got {self.O}")
        self.net = MATNet(self.O, self.nA, self.A, self.D, self.H, self.n_block, continuous=self.continuous, min_scale=self.min_scale)
        # actor_lr is the single learning rate of the one Adam; critic_lr is accepted and unused (encoder and decoder
        # share one optimiser, as upstream MAT does)
        self._alloc_params([(self.net, s.actor_lr)])
        d = self.device
        self.Bm = self.T * self.E // self.M  # (t, env) samples per minibatch
        self.actor_network = MATActor(self.net, self.ctx, d, self.acting)
        self.roll = self.actor_network.pass_for(self.E)
        self.train = MATPass(self.net, self.Bm, d, True, self.ctx)
        rows = self.train.rows
        self.grad_scale = float(2 ** math.ceil(math.log2(rows)))
        self.dlogits = torch.zeros(rows * self.nA, device=d)
        self.dvalues = torch.zeros(rows, device=d)
        self.loss_blocks = max(1, min(256, -(-rows // 256)))
        self.partials = torch.zeros((self.loss_blocks, 3), device=d)
        self.dls_partials = torch.zeros((self.loss_blocks, self.nA), device=d) if self.continuous else None  # d loss / d log_std per block
        self.debug: Optional[Dict[str, list]] = None  # tests: {"grads": [], "perms": [], "state": []} records every minibatch (and "slot0")

    def _refuse(self, env, config) -> None:
        head = dict(config.network.get("action_head", None) or {})
        if "ContinuousActionHead" in str(head.get("_target_", "")):
            if not getattr(env, "continuous_actions", False):  # its step kernel would read the f32 action vectors as int32 indices
                raise MavaHipError("ff_mat: a continuous action head is not implemented for an environment with discrete actions "
                                   "(the environment does not set continuous_actions; env=spread does)")
            check_supported_continuous(num_agents=int(env.num_agents), action_dim=int(env.action_dim), n_embd=self.D, n_head=self.H,
                                       independent_std=bool(head.get("independent_std", True)), world=self.world,
                                       update_batch_size=self.U)
        else:
            check_supported(num_agents=int(env.num_agents), n_actions=int(env.action_dim), n_embd=self.D, n_head=self.H, continuous=False,
                            world=self.world, update_batch_size=self.U)
        if self.n_block < 1:
            raise ValueError(f"network.n_block must be >= 1, got {self.n_block}")
        if self.acting not in ACTING:
            raise MavaHipError(f"ff_mat: network.acting must be one of {ACTING}, got {self.acting!r}")
        if (self.T * self.E) % self.M:
            raise ValueError("rollout_length * num_envs must be divisible by num_minibatches")

    # ---------------------------------------------------------------------------- state views
    def _params_tree(self) -> MATParams:
        return self._trees(self.p)[0]

    def _opt_tree(self):
        return self._adam_states()[0]

    def _state_segments(self, state: LearnerState):
        return [(state.params, state.opt_states)]

    def learner_state(self) -> LearnerState:
        done = self._stack(lambda r: r.last_done)
        ts = TimeStep(torch.where(done[..., 0].bool(), 2, 1).to(torch.int8), self._stack(lambda r: r.last_reward), 1.0 - done.float(),
                      self._observation(), {})
        return LearnerState(self._params_tree(), self._opt_tree(), self._key(), self._env_state(), ts)

    # ------------------------------------------------------------------------------------ update
    def _rollout(self, n: int) -> None:
        rep, T = self.rep, self.T
        for t in range(T):
            step = self.t_global + t
            self.roll.act(self.p, rep.agents_view[t], rep.action_mask[t], rep.action[t], rep.log_prob[t], self.seed, step, 0, False,
                          value_out=rep.value[t])
            rep.env.step_into(rep.state, step + 1, rep.obs_slot(t + 1), rep.reward[t], rep.done[t], rep.info_return[n, t],
                              rep.info_length[n, t], rep.info_terminal[n, t], action=rep.action[t])
        rep.last_reward.copy_(rep.reward[T - 1])
        rep.last_done.copy_(rep.done[T - 1])
        self.t_global += T

    def _bootstrap_and_gae(self) -> None:
        s, rep, T, EA = self.config.system, self.rep, self.T, self.E * self.A
        self.roll.gather_obs(rep.agents_view[T], self.E)
        self.roll.encode(self.p)
        rep.last_val.view(-1).copy_(self.roll.value.t[:EA])
        ops.gae(rep.reward.view(T, EA), rep.value.view(T, EA), rep.done.view(T, EA), rep.last_val.view(EA), float(s.gamma),
                float(s.gae_lambda), out=(rep.adv.view(T, EA), rep.tgt.view(T, EA)), ctx=self.ctx)

    def _minibatch(self, n: int, k: int, mb: int, perm: torch.Tensor) -> None:
        s, rep, tr, T, Bm = self.config.system, self.rep, self.train, self.T, self.Bm
        if self.debug is not None:
            if mb == 0:
                self.debug["perms"].append(perm.clone())
            self.debug["state"].append((self.p.clone(), self.m.clone(), self.v.clone()))
        tr.idx[:Bm].copy_(perm[mb * Bm : (mb + 1) * Bm])
        tr.gather_obs(rep.agents_view[:T], T * self.E)
        tr.shift_onehot(rep.action, self.A - 1, True)
        tr.encode(self.p)
        tr.decode(self.p)
        ops.adv_stats(rep.adv.view(-1), tr.idx, 0, Bm, self.A, out=self.stats)
        if self.continuous:
            self._continuous_loss_and_backward()
        else:
            self._discrete_loss_and_backward()
        if self.debug is not None:
            self.debug["grads"].append(self.g.clone())
        self._clip_adam(n, k, mb)

    def _continuous_loss_and_backward(self) -> None:
        """tr.logits holds the means; the log_std gradient comes from the loss kernel's per-block sums, not from the tape."""
        s, rep, tr, T, nA = self.config.system, self.rep, self.train, self.T, self.nA
        launch("mat_loss_cont", lib().mava_transformer_loss_continuous_f32, self.Bm, self.A, nA, self.min_scale, tr.rows, ptr(tr.idx),
               ptr(tr.logits.t), ptr(tr.log_std(self.p)), ptr(tr.value.t), ptr(rep.action), ptr(rep.log_prob), ptr(rep.adv), ptr(rep.value),
               ptr(rep.tgt), ptr(self.stats), self.stats.shape[0], float(s.clip_eps), float(s.ent_coef), float(s.vf_coef),
               self.seed & (2**64 - 1), self.ent_step & 0xFFFFFFFF, 0, self.grad_scale, ptr(self.dlogits), ptr(self.dvalues),
               ptr(self.partials), ptr(self.dls_partials), self.loss_blocks, stream_ptr())
        ops.slab_reduce(self.partials, 3, self.g[self.P : self.P + 3])
        tr.backward(self.p, self.g, self.dlogits, self.dvalues, self.grad_scale)
        ops.slab_reduce(self.dls_partials, nA, tr.log_std(self.g))

    def _discrete_loss_and_backward(self) -> None:
        s, rep, tr, T, Bm = self.config.system, self.rep, self.train, self.T, self.Bm
        launch("mat_loss", lib().mava_mat_loss_f32, Bm, self.A, self.nA, tr.rows, ptr(tr.idx), ptr(tr.logits.t), ptr(tr.value.t),
               ptr(rep.action_mask[:T]), ptr(rep.action), ptr(rep.log_prob), ptr(rep.adv), ptr(rep.value), ptr(rep.tgt), ptr(self.stats),
               self.stats.shape[0], float(s.clip_eps), float(s.ent_coef), float(s.vf_coef), self.grad_scale, ptr(self.dlogits),
               ptr(self.dvalues), ptr(self.partials), self.loss_blocks, stream_ptr())
        ops.slab_reduce(self.partials, 3, self.g[self.P : self.P + 3])
        tr.backward(self.p, self.g, self.dlogits, self.dvalues, self.grad_scale)

    def _carry_observation(self) -> None:
        if self.debug is not None:  # slot 0 of the trajectory is about to become the next rollout's first observation
            self.debug["slot0"] = (self.rep.agents_view[0].clone(), self.rep.action_mask[0].clone())
        super()._carry_observation()


def learner_setup(env, keys, config, device=None):
    """(learn, actor_network, initial LearnerState), as mava_amd/learner.py::learner_setup; keys[1] seeds the parameters."""
    return ppo_learner.learner_setup(MATLearner, env, keys, config, device=device)
