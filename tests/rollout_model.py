"""TEST INFRASTRUCTURE ONLY.  The fused rollout kernel (mava_amd/csrc/rollout_h2.hip, mava_rollout_ff_f32) as one launch sees
it: a NumPy float64 model of the launch, the table of cases that reaches every template instance at its edges, and a
restatement of the dispatch (the pattern of tests/instances.py).

The model is composed from what oracle/ already holds - SynthRware, philox.policy_uniforms, ppo_oracle's mlp_forward,
masked_logits, log_softmax, gumbel_argmax and gae - in the order of OracleLearner._rollout, which it equals bit for bit when
its seeds and offsets are tied the way that class ties them (tests/test_rollout_model.py).  Unlike that class it keeps
policy_seed, env_seed, t0, row_offset and env_offset apart, as the entry point does, and starts from a caller-given slot 0."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from oracle import philox
from oracle import ppo_oracle as po
from oracle.synth_env import SynthRware

GAMMA, LAMBDA = 0.99, 0.95
NEAR_TIE = 1e-3       # Gumbel-score margin below which two arithmetics may pick different actions (test_gpu_learner._check_traj)
NEAR_TIE_CAP = 0.01   # at most this fraction of a case's rows may be such near-ties (worst of the table: 2 / 576)
FLOAT_TOL = 5e-5      # value / log_prob / last_val / adv / tgt against float64 (test_gpu_learner.py holds the kernel to it)
# A case whose float outputs miss FLOAT_TOL because of the split-f16 arithmetic itself would be listed here with the error of
# a NumPy emulation of the forward pass (operands as f16 hi + lo, float32 accumulation) against float64, and held to four
# times that figure.  No case needed it: every case meets FLOAT_TOL.
F16X2_MEASURED: Dict[str, float] = {}


def float_tolerance(name: str) -> float:
    return 4.0 * F16X2_MEASURED[name] if name in F16X2_MEASURED else FLOAT_TOL


# ------------------------------------------------------------------------------------------------ dispatch
def predict_instance(shared: bool, A: int, O: int, nA: int) -> Optional[int]:
    """NO * 100000 + S1A * 1000 + S1C * 10 + SHARED of the rollout_h2_kernel instance mava_rollout_ff_f32 launches, or None
    when it returns 1 without launching (end of rollout_h2.hip)."""
    if A < 1 or 64 % A != 0 or not 1 <= nA <= 8 or O < 2:
        return None
    if shared and A < 2:
        return None
    s1a = (A + O + 1 + 15) // 16
    s1c = (A * O + 1 + 15) // 16 if shared else s1a
    if shared:
        if s1a == 5 and s1c == 17 and A >= 4:
            return 805171
        if s1a <= 2 and s1c <= 2:
            return 802021
        if s1a <= 2 and s1c <= 4:
            return 802041
        if s1a <= 5 and s1c <= 9:
            return 805091
        return None
    if s1a == 5:
        return 805050
    if s1a <= 2:
        return 802020
    return None


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    shared: bool
    A: int
    O: int
    nA: int
    E: int
    inst: int
    t0: int
    row_offset: int
    env_offset: int
    reward_mode: int
    policy_seed: int
    env_seed: int
    T: int = 8
    time_limit: int = 3

    @property
    def rows(self) -> int:
        return self.T * self.E * self.A

    @property
    def envs_per_block(self) -> int:
        return 64 // self.A


def _case(i, name, shared, A, O, nA, E, inst):
    # offsets: no multiples of 64 or of E, unrelated to each other (test_rollout_model.py checks it).  Seeds: non-zero high
    # words, the two different.  Reward mode 1 ("match": the sampled actions feed the environment phase) in nine cases of
    # fifteen; the one-action case is not among them, its every action matches.
    def clear_of(off):  # the next value that is no multiple of 64 or of E
        while off % 64 == 0 or off % E == 0:
            off += 1
        return off

    return Case(name, shared, A, O, nA, E, inst, t0=(0, 3, 1000003)[i % 3], row_offset=clear_of(1000 * i + 37),
                env_offset=clear_of(137 * i + 11), reward_mode=int(i % 2 == 1 or i in (0, 14)), policy_seed=(0x1234ABCD + i << 32) | (42 + i),
                env_seed=(0x9E3779B9 - i << 32) | (7 + 3 * i))


# T = 8, time_limit = 3 (every environment resets at least twice inside the launch), 500 to 1600 agent rows, E one more than
# a whole number of blocks or otherwise ragged.  What each case pins is in its name's comment.
CASES = [_case(i, *row) for i, row in enumerate([
    ("s-A2-O15-n3", True, 2, 15, 3, 33, 802021),     # 32 envs per block plus 1
    ("s-A8-O3-n8", True, 8, 3, 8, 9, 802021),        # actor s1a = 1 under S1A = 2, NO full
    ("s-A4-O15-n5", True, 4, 15, 5, 17, 802041),     # s1c = 4 exactly
    ("s-A16-O3-n2", True, 16, 3, 2, 5, 802041),      # 4 envs per block, 2 actions
    ("s-A8-O17-n4", True, 8, 17, 4, 9, 805091),      # actor s1a = 2 under S1A = 5
    ("s-A64-O2-n5", True, 64, 2, 5, 3, 805091),      # one env per block, O = 2: the bit-chunk count clamps to 1
    ("s-A32-O4-n7", True, 32, 4, 7, 3, 805091),      # s1a = 3 under 5
    ("s-A4-O64-n8", True, 4, 64, 8, 17, 805171),     # din_c = 256: the bias alone in step 16
    ("s-A4-O67-n1", True, 4, 67, 1, 17, 805171),     # one action, odd widths, A * O % 8 != 0
    ("d-A1-O70-n5", False, 1, 70, 5, 65, 805050),    # 64 envs per block plus 1
    ("d-A64-O15-n6", False, 64, 15, 6, 2, 805050),   # A + O + 1 = 80: the bias on the last k of the last step
    ("d-A16-O48-n3", False, 16, 48, 3, 5, 805050),   # the bias on the first k of step 4
    ("d-A1-O2-n2", False, 1, 2, 2, 70, 802020),      # smallest legal shape
    ("d-A16-O15-n5", False, 16, 15, 5, 6, 802020),   # A + O + 1 = 32
    ("d-A2-O13-n8", False, 2, 13, 8, 33, 802020),    # 8 actions
])]
CASE_BY_NAME = {c.name: c for c in CASES}

# (shared, A, O, nA): mava_rollout_ff_f32 returns 1 and launches nothing.  Shared A = 4: s1c = 18 at O = 68 and 16 at O = 60,
# the 17-step instance is taken for O in 64 .. 67 only.
REFUSED = [(True, 2, 130, 5), (True, 4, 68, 5), (True, 4, 60, 5), (False, 4, 30, 5), (True, 3, 15, 5), (False, 3, 15, 5),
           (True, 4, 15, 9), (False, 4, 15, 9), (True, 1, 15, 5)]


def case_params(c: Case):
    """(actor, critic) parameter vectors in float32: orthogonal weights as the learner initialises them, and biases that are
    NOT the zeros of an initialisation - a bias row that is dropped or read from the wrong k must change the result."""
    rng = np.random.default_rng([c.A, c.O, c.nA, int(c.shared)])

    def net(din, no):
        p = po.init_mlp(rng, din, no, 1.0)
        p = p._replace(b1=0.3 * rng.standard_normal(po.H), b2=0.3 * rng.standard_normal(po.H), b3=0.3 * rng.standard_normal(no))
        return po.mlp_flatten(p).astype(np.float32)

    return net(c.A + c.O, c.nA), net(c.A * c.O if c.shared else c.A + c.O, 1)


def make_env(c: Case) -> SynthRware:
    return SynthRware(c.E, c.A, c.O, c.nA, c.time_limit, c.env_seed, env_offset=c.env_offset,
                      reward_mode="match" if c.reward_mode == 1 else "random")


def case_init(c: Case) -> Dict[str, np.ndarray]:
    """Slot 0 and the env-state words a launch starts from: the environment's own observation at t0, environments part-way
    through episodes (different step counts, running and last-episode metrics that are not zero).  A one-action case has no
    action the environment could mask: there the caller's slot-0 mask leaves every fifth row without a legal action."""
    obs = make_env(c).reset(c.t0)
    e = np.arange(c.E)
    mask = obs["action_mask"].astype(np.uint8)
    if c.nA == 1:
        mask.reshape(-1, 1)[::5] = 0
    return {"agents_view": obs["agents_view"], "global_state": obs["global_state"], "action_mask": mask,
            "step_count": np.repeat((e % c.time_limit).astype(np.int32)[:, None], c.A, 1),
            "run_return": (0.25 * (e % 4)).astype(np.float32), "run_length": (e % c.time_limit).astype(np.int32),
            "ep_return": (0.5 + 0.125 * (e % 3)).astype(np.float32), "ep_length": (1 + e % 3).astype(np.int32)}


def slice_init(init, lo: int, hi: int):
    return {k: v[lo:hi] for k, v in init.items()}


# ------------------------------------------------------------------------------------------------ the launch in float64
def rollout(case: Case, pa, pc, init, forced_action=None) -> Dict[str, np.ndarray]:
    """One launch of mava_rollout_ff_f32: every array the kernel writes, under the kernel's argument names (observation arrays
    with T + 1 slots, slot 0 the caller's; env-state words after the launch as state.*).  forced_action (T, E, A): the sampled
    actions are an input, as in OracleLearner._rollout; the model's own draw is own_action and action_margin its Gumbel score
    minus the forced action's.  runner_up_gap (T, E, A): the model's best score minus its second best (inf for one action)."""
    c = case
    E, A, O, nA, T = c.E, c.A, c.O, c.nA, c.T
    W = A + O
    din_c = A * O if c.shared else W
    env = make_env(c)
    env.step_count[:] = init["step_count"]
    env.run_return[:], env.run_length[:] = init["run_return"], init["run_length"]
    env.ep_return[:], env.ep_length[:] = init["ep_return"], init["ep_length"]
    obs = {"agents_view": np.asarray(init["agents_view"], np.float32), "global_state": np.asarray(init["global_state"], np.float32),
           "action_mask": np.asarray(init["action_mask"]).astype(bool), "step_count": np.asarray(init["step_count"], np.int32)}
    pa_ = po.mlp_unflatten(np.asarray(pa, np.float64).copy(), W, nA)
    pc_ = po.mlp_unflatten(np.asarray(pc, np.float64).copy(), din_c, 1)

    def critic_in(o):
        if c.shared:
            return np.repeat(o["global_state"][:, :1, :], A, 1).astype(np.float64)
        return o["agents_view"].astype(np.float64)

    keys = ("agents_view", "global_state", "action_mask", "obs_step_count", "action", "own_action", "action_margin",
            "runner_up_gap", "value", "reward", "log_prob", "done", "info_return", "info_length", "info_terminal")
    tr = {k: [] for k in keys}

    def record_obs(o):
        tr["agents_view"].append(o["agents_view"])
        tr["global_state"].append(o["global_state"])
        tr["action_mask"].append(o["action_mask"])
        tr["obs_step_count"].append(o["step_count"])

    rows_ = np.arange(E * A)
    for t in range(T):
        step = c.t0 + t
        record_obs(obs)
        av = obs["agents_view"].astype(np.float64)
        z = po.masked_logits(po.mlp_forward(pa_, av.reshape(E * A, -1)), obs["action_mask"].reshape(E * A, nA))
        uni = philox.policy_uniforms(c.policy_seed, step, E * A, nA, row_offset=c.row_offset)
        own = po.gumbel_argmax(z, uni).reshape(E, A)
        with np.errstate(divide="ignore"):
            score = z - np.log(-np.log(uni))
        if nA > 1:
            top = np.sort(score, axis=1)
            gap = top[:, -1] - top[:, -2]
        else:
            gap = np.full(E * A, np.inf)
        action = own
        if forced_action is not None:
            action = np.asarray(forced_action[t]).reshape(E, A).astype(own.dtype)
        margin = score[rows_, own.reshape(-1)] - score[rows_, action.reshape(-1).astype(np.int64)]
        lp = po.log_softmax(z)[rows_, action.reshape(-1)]
        value = po.mlp_forward(pc_, critic_in(obs).reshape(E * A, -1))[:, 0]
        obs, reward, done, info = env.step(step + 1, action=action)
        for k, v in (("action", action), ("own_action", own), ("action_margin", margin.reshape(E, A)),
                     ("runner_up_gap", gap.reshape(E, A)), ("value", value.reshape(E, A)), ("reward", reward.astype(np.float64)),
                     ("log_prob", lp.reshape(E, A)), ("done", done), ("info_return", info["episode_return"]),
                     ("info_length", info["episode_length"]), ("info_terminal", info["is_terminal_step"])):
            tr[k].append(v)
    record_obs(obs)
    out = {k: np.stack(v, 0) for k, v in tr.items()}
    out["last_val"] = po.mlp_forward(pc_, critic_in(obs).reshape(E * A, -1))[:, 0].reshape(E, A)
    out["adv"], out["tgt"] = po.gae(out["reward"], out["value"], out["done"], out["last_val"], GAMMA, LAMBDA)
    out.update({"state.step_count": env.step_count.copy(), "state.run_return": env.run_return.copy(),
                "state.run_length": env.run_length.copy(), "state.ep_return": env.ep_return.copy(),
                "state.ep_length": env.ep_length.copy()})
    return out
