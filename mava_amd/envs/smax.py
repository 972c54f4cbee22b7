"""SMAX (the `env=smax_native` task) on the GPU: mava_smax_step (csrc/smax.hip).

Na allied units - the agents - fight Ne units of a scripted opponent on a 32 x 32 map with continuous positions.  An agent
moves (N, E, S, W), stops or attacks an enemy in range; one env step is eight world sub-steps of move, fire, damage and
cooldown; the opponent attacks the closest ally it sees and otherwise marches towards it or towards the centre.  The
team earns the enemies' lost health fraction, plus 1 for wiping them out.  The complete rules are in DESIGN.md "SMAX",
include/mava_hip.h and, as the contract, tests/smax_model.py; they follow the published SMAX task - parity with JaxMARL's
SMAX itself is UNPINNED (its source is not part of this project).

`agents_view` is the one-hot agent id, one 11-float block per other unit within sight and the viewer's own 10-float
block; `global_state` is every unit's own block with a team one-hot, shared by the agents.  The shapes are the ones the
synthetic `env=smax` stand-in uses: 5 + Ne actions.

SMAX reports a win: `reset` / `step` put `won_episode` (E,) bool into the extras, which the evaluator forwards and the
logger turns into `win_rate` (env.log_win_rate).

The object has the batched MarlEnv surface of Cleaner: `step_into` writes straight into trajectory slots owned by the
learner, `reset` / `step` allocate.  It declares no fused rollout.
"""
from __future__ import annotations

import re
from typing import NamedTuple, Optional, Sequence

import torch

from .._lib import ptr
from .base import COMMON_STATE, BatchedEnv, make_pair

MAX_SIDE = 16  # compile-time maximum of csrc/smax.hip: units per side
NUM_MOVE_ACTIONS = 5  # N, E, S, W, stop; then one attack action per enemy
UNIT_TYPES = ("marine", "marauder", "stalker", "zealot", "zergling", "hydralisk")  # the nibble values of the kernel
_LETTER = {"m": 0, "s": 2, "z": 3, "h": 5}
# allies[_vs_enemies]: a count and a type letter at a time, in unit index order
SCENARIOS = ("3m", "2s3z", "3s5z", "3s5z_vs_3s6z", "5m_vs_6m", "10m_vs_11m", "3s_vs_5z", "6h_vs_8z")


SmaxState = NamedTuple("SmaxState", COMMON_STATE + [
    ("pos", torch.Tensor),  # (E, U, 2) f32 (x, y); units are the allies, then the enemies
    ("health", torch.Tensor),  # (E, U) f32, integer values
    ("cd", torch.Tensor),  # (E, U) i32 weapon cooldown in sub-steps
    ("last_action", torch.Tensor),  # (E, U) i32
])


def _side(text: str) -> tuple:
    return tuple(_LETTER[ch] for n, ch in re.findall(r"(\d+)([a-z])", text) for _ in range(int(n)))


def scenario_units(name: str):
    """(ally types, enemy types) of a scenario of the table."""
    if name == "27m_vs_30m" or str(name).startswith("smacv2"):
        raise ValueError(f"SMAX scenario {name!r} is out of scope: at most {MAX_SIDE} units per side, no smacv2 generation")
    if name not in SCENARIOS:
        raise ValueError(f"unknown SMAX scenario {name!r}: one of {', '.join(SCENARIOS)}")
    allies, _, enemies = name.partition("_vs_")
    return _side(allies), _side(enemies or allies)


def _pack(types: Sequence[int]) -> int:
    return sum(int(t) << (4 * i) for i, t in enumerate(types))


class Smax(BatchedEnv):
    State = SmaxState
    reports_win = True  # info_won / extras["won_episode"]
    step_symbol = "mava_smax_step"  # terminated: a side is wiped out

    def __init__(self, num_envs: int, ally_types: Sequence[int], enemy_types: Sequence[int], time_limit: int = 100,
                 see_enemy_actions: bool = True, walls_cause_death: bool = True, attack_mode: str = "closest",
                 add_global_state: bool = False, seed: int = 42, env_offset: int = 0, device: Optional[torch.device] = None):
        kw = dict(locals())  # the constructor keywords, before any other local exists
        kw["ally_types"], kw["enemy_types"] = tuple(int(t) for t in ally_types), tuple(int(t) for t in enemy_types)
        kw["num_agents"] = len(kw["ally_types"])
        for side, types in (("ally", kw["ally_types"]), ("enemy", kw["enemy_types"])):
            if not (1 <= len(types) <= MAX_SIDE):
                raise ValueError(f"Smax supports 1 to {MAX_SIDE} units per side; got {len(types)} {side} units")
            if any(not (0 <= t < len(UNIT_TYPES)) for t in types):
                raise ValueError(f"Smax {side} unit types must be below {len(UNIT_TYPES)}; got {types}")
        if attack_mode != "closest":
            raise ValueError(f"Smax implements attack_mode 'closest' only; got {attack_mode!r}")
        if int(time_limit) < 1:
            raise ValueError(f"time_limit must be >= 1, got {time_limit}")
        super().__init__(kw)
        del self._ctor_kw["num_agents"]  # the base reads it; the constructor derives it from ally_types
        self.ally_types, self.enemy_types = kw["ally_types"], kw["enemy_types"]
        self.num_enemies = len(self.enemy_types)
        self.see_enemy_actions, self.walls_cause_death = bool(see_enemy_actions), bool(walls_cause_death)

    # ---- specs ----------------------------------------------------------------------------
    @property
    def num_units(self) -> int:
        return self.num_agents + self.num_enemies

    @property
    def action_dim(self) -> int:
        return NUM_MOVE_ACTIONS + self.num_enemies

    @property
    def raw_obs_dim(self) -> int:
        return 11 * (self.num_units - 1) + 10

    @property
    def obs_dim(self) -> int:
        return self.num_agents + self.raw_obs_dim

    @property
    def state_dim(self) -> int:
        return 12 * self.num_units

    def alloc_own_state(self) -> tuple:
        E, U, d = self.num_envs, self.num_units, self.device
        return (torch.zeros((E, U, 2), device=d), torch.zeros((E, U), device=d),
                torch.zeros((E, U), dtype=torch.int32, device=d), torch.zeros((E, U), dtype=torch.int32, device=d))

    def step_args(self, state: SmaxState):
        return ((self.num_enemies, _pack(self.ally_types), _pack(self.enemy_types), self.time_limit,
                 int(self.see_enemy_actions), int(self.walls_cause_death)),
                (ptr(state.pos), ptr(state.health), ptr(state.cd), ptr(state.last_action)))


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """(train_env, eval_env) of an `env=smax_native` configuration, sized by config.arch.num_envs / num_eval_episodes.
    The scenario is looked up by its task_name; env.kwargs carries the reference's three keywords and, optionally,
    time_limit."""
    if not bool(config.system.add_agent_id) or bool(config.env.implicit_agent_id):
        raise ValueError("Smax always prepends the agent one-hot id (add_agent_id=True)")
    allies, enemies = scenario_units(str(config.env.scenario.task_name))
    kwargs = dict(config.env.get("kwargs", None) or {})
    unknown = set(kwargs) - {"see_enemy_actions", "walls_cause_death", "attack_mode", "time_limit"}
    if unknown:
        raise ValueError(f"Smax does not know env.kwargs {sorted(unknown)}")
    kw = dict(ally_types=allies, enemy_types=enemies, time_limit=int(kwargs.get("time_limit", 100)),
              see_enemy_actions=bool(kwargs.get("see_enemy_actions", True)),
              walls_cause_death=bool(kwargs.get("walls_cause_death", True)),
              attack_mode=str(kwargs.get("attack_mode", "closest")), add_global_state=add_global_state, device=device)
    return make_pair(Smax, config, kw, env_offset)
