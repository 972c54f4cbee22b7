"""TEST INFRASTRUCTURE: NumPy / plain-Python statement of the Connector rules of mava_connector_step
(mava_amd/csrc/connector.hip, DESIGN.md "Connector").  This file is the contract: any detail the documents leave open is
fixed by what is written here.  Written independently of the kernel: the board is a (G, G) array, empty cells are found
by scanning Python lists, every environment is stepped by Python loops; no row bit masks, no claim table.

State and outputs use the device layouts: a state is a dict of arrays named like ConnectorState's fields.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.philox import philox4x32_10

RESET_STREAM = 0x434F4E52  # "CONR"
N_ACTIONS = 5
NOOP, UP, RIGHT, DOWN, LEFT = range(5)
_MOVE = {UP: (-1, 0), RIGHT: (0, 1), DOWN: (1, 0), LEFT: (0, -1)}  # (row, col)
PATH, HEAD, TARGET = 1, 2, 3  # grid value of agent k: PATH + 3 k, HEAD + 3 k, TARGET + 3 k; 0 is empty
STATE_FIELDS = ("head", "target", "connected", "grid", "step_count", "run_return", "run_length", "ep_return", "ep_length")
EVENTS = ("moves", "connections", "contested", "terminations", "truncations", "fallbacks")
MAX_GRID, MAX_AGENTS = 16, 32


@dataclass(frozen=True)
class Params:
    G: int
    A: int
    time_limit: int = 50

    @property
    def lmax(self) -> int:
        return max(1, (self.G * self.G - 2) // self.A - 1)

    @property
    def n_draws(self) -> int:  # the most draws one reset can use
        return self.A * (2 + self.lmax)

    @property
    def obs_dim(self) -> int:
        return self.G * self.G * 5

    @property
    def state_dim(self) -> int:
        return self.G * self.G * 3


SCENARIOS = {"con-5x5x3a": (5, 3, 25), "con-7x7x5a": (7, 5, 49), "con-10x10x10a": (10, 10, 100),
             "con-15x15x23a": (15, 23, 225)}  # name: (grid_size, num_agents, time_limit)


def params_of(env) -> Params:
    """The Params of a mava_amd.envs.connector.Connector."""
    return Params(env.grid_size, env.num_agents, env.time_limit)


def rel_table(A: int) -> np.ndarray:
    """(A + 1) f32: entry i is i / A, one correctly rounded f32 division."""
    return np.arange(A + 1, dtype=np.float32) / np.float32(A)


def team_reward(n_connected_now: int, n_open: int) -> np.float32:
    """+1.0 per agent that connects on this step, -0.03 per agent that was not connected at its start, summed over the
    agents: (100 c - 3 o) / 100 with ONE correctly rounded f32 division of two exactly representable integers."""
    return np.float32(100 * int(n_connected_now) - 3 * int(n_open)) / np.float32(100)


def draws(seed: int, g, t: int, n: int) -> np.ndarray:
    """(len(g), n) uint32: draw k of env g is word k % 4 of Philox block k // 4, counter (g, t, k // 4, "CONR")."""
    g = np.atleast_1d(np.asarray(g, np.uint32))
    slo, shi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    out = np.empty((g.size, 4 * ((n + 3) // 4)), np.uint32)
    for k in range((n + 3) // 4):
        w = philox4x32_10(g, np.uint32(t & 0xFFFFFFFF), k, RESET_STREAM, slo, shi)
        for q in range(4):
            out[:, 4 * k + q] = w[q]
    return out[:, :n]


def _neighbours(p: Params, cell):
    """The on-grid 4-neighbours of (row, col), listed UP, RIGHT, DOWN, LEFT."""
    r, c = cell
    return [(r + dr, c + dc) for dr, dc in (_MOVE[UP], _MOVE[RIGHT], _MOVE[DOWN], _MOVE[LEFT])
            if 0 <= r + dr < p.G and 0 <= c + dc < p.G]


def generate(p: Params, dr) -> dict:
    """One environment's reset board from its draw sequence (the draws are used in order, none is skipped).  Returns
    head / target (A, 2), grid (G, G) and, for the tests, the walks and how often the no-candidate fallback ran."""
    d = iter(int(x) for x in dr)
    cells = [(r, c) for r in range(p.G) for c in range(p.G)]  # row-major
    taken = set()
    walks, fallbacks = [], 0
    for _k in range(p.A):
        cand = [c for c in cells if c not in taken and any(n not in taken for n in _neighbours(p, c))]
        if cand:
            cur = cand[next(d) % len(cand)]
            length = 1 + next(d) % p.lmax
            walk = [cur]
            taken.add(cur)
            for _ in range(length):
                free = [n for n in _neighbours(p, cur) if n not in taken]
                if not free:
                    break
                cur = free[next(d) % len(free)]
                walk.append(cur)
                taken.add(cur)
        else:
            walk = [c for c in cells if c not in taken][:2]
            taken.update(walk)
            fallbacks += 1
        walks.append(walk)
    grid = np.zeros((p.G, p.G), np.uint8)
    for k, w in enumerate(walks):  # the cells between head and target are cleared
        grid[w[0]] = HEAD + 3 * k
        grid[w[-1]] = TARGET + 3 * k
    return {"head": np.array([w[0] for w in walks], np.int32), "target": np.array([w[-1] for w in walks], np.int32),
            "grid": grid, "walks": walks, "fallbacks": fallbacks}


def alloc_state(p: Params, E: int) -> dict:
    return {"head": np.zeros((E, p.A, 2), np.int32), "target": np.zeros((E, p.A, 2), np.int32),
            "connected": np.zeros((E, p.A), np.uint8), "grid": np.zeros((E, p.G, p.G), np.uint8),
            "step_count": np.zeros((E, p.A), np.int32), "run_return": np.zeros(E, np.float32),
            "run_length": np.zeros(E, np.int32), "ep_return": np.zeros(E, np.float32), "ep_length": np.zeros(E, np.int32)}


def _regenerate(p: Params, st: dict, envs: np.ndarray, seed: int, env_offset: int, t: int) -> int:
    if envs.size == 0:
        return 0
    g = (envs.astype(np.uint64) + np.uint64(env_offset)).astype(np.uint32)
    dr = draws(seed, g, t, p.n_draws)
    fallbacks = 0
    for i, e in enumerate(envs):
        gen = generate(p, dr[i])
        for k in ("head", "target", "grid"):
            st[k][e] = gen[k]
        st["connected"][e] = 0
        st["step_count"][e] = 0
        fallbacks += gen["fallbacks"]
    return fallbacks


def _can_enter(p: Params, grid, k: int, cell) -> bool:
    """Rule 1's test on a destination: on the grid, and empty or agent k's own target."""
    r, c = cell
    return 0 <= r < p.G and 0 <= c < p.G and int(grid[r, c]) in (0, TARGET + 3 * k)


def mask_env(p: Params, head, connected, grid) -> np.ndarray:
    mask = np.zeros((p.A, N_ACTIONS), np.uint8)
    mask[:, NOOP] = 1
    for k in range(p.A):
        if connected[k]:
            continue
        for m, (dr, dc) in _MOVE.items():
            mask[k, m] = _can_enter(p, grid, k, (int(head[k][0]) + dr, int(head[k][1]) + dc))
    return mask


def observe(p: Params, st: dict) -> dict:
    """agents_view (E, A, G G 5), global_state (E, 1, G G 3), action_mask (E, A, 5), step_count of the current state."""
    E, A, G = st["grid"].shape[0], p.A, p.G
    grid = st["grid"].astype(np.int64)
    owner, kind = (grid - 1) // 3, (grid - 1) % 3 + 1  # kind: PATH, HEAD or TARGET where grid > 0
    occupied = grid > 0
    tab = rel_table(A)
    av = np.zeros((E, A, G, G, 5), np.float32)
    for j in range(A):
        rel = tab[np.where(occupied, (owner - j) % A + 1, 0)]
        av[:, j, :, :, 0] = np.where(occupied & (kind == HEAD), rel, np.float32(0))
        av[:, j, :, :, 1] = np.where(occupied & (kind == TARGET), rel, np.float32(0))
        av[:, j, :, :, 2] = occupied & (kind == PATH)
        av[:, j, :, :, 3] = grid == HEAD + 3 * j
        av[:, j, :, :, 4] = grid == TARGET + 3 * j
    mask = np.stack([mask_env(p, st["head"][e], st["connected"][e], st["grid"][e]) for e in range(E)]) if E else \
        np.zeros((0, A, N_ACTIONS), np.uint8)
    return {"agents_view": av.reshape(E, A, -1), "global_state": av[:, 0, :, :, :3].reshape(E, 1, -1).copy(),
            "action_mask": mask, "step_count": st["step_count"].copy()}


def reset(p: Params, E: int, seed: int, env_offset: int = 0, t: int = 0):
    st = alloc_state(p, E)
    _regenerate(p, st, np.arange(E), seed, env_offset, t)
    return st, observe(p, st)


def _rules_env(p: Params, st: dict, e: int, act, ev: dict):
    """Rules 1-3 of one environment, in place.  Returns (agents that connected, agents open at the start)."""
    head, target, conn, grid = st["head"][e], st["target"][e], st["connected"][e], st["grid"][e]
    start = grid.copy()  # every test is made against the grid at the start of the step
    n_open = int((conn == 0).sum())
    dest = {}
    for k in range(p.A):
        a = int(act[k])
        if conn[k] or a not in _MOVE:
            continue
        cell = (int(head[k, 0]) + _MOVE[a][0], int(head[k, 1]) + _MOVE[a][1])
        if _can_enter(p, start, k, cell):
            dest[k] = cell
    wanted = list(dest.values())
    n_conn = 0
    for k, cell in dest.items():
        if wanted.count(cell) > 1:
            ev["contested"] += 1
            continue
        grid[tuple(head[k])] = PATH + 3 * k
        grid[cell] = HEAD + 3 * k  # a head standing on its own target is stored as head
        head[k] = cell
        ev["moves"] += 1
        if cell == tuple(int(v) for v in target[k]):
            conn[k] = 1
            n_conn += 1
            ev["connections"] += 1
    return n_conn, n_open


def step(p: Params, st: dict, action: np.ndarray, seed: int, env_offset: int, t: int):
    """One step of every environment, in place on `st`.  Returns (obs, reward (E, A) f32, done (E, A) u8,
    info_return (E,) f32, info_length (E,) i32, info_terminal (E,) u8, extra) with extra = {"real_view", "real_mask"
    (the observation before any auto-reset), "terminated" (E,) u8, "events": counts of what happened}."""
    E, A = st["grid"].shape[0], p.A
    act = np.asarray(action, np.int32).reshape(E, A)
    ev = {k: 0 for k in EVENTS}
    rew = np.zeros(E, np.float32)
    for e in range(E):
        rew[e] = team_reward(*_rules_env(p, st, e, act[e], ev))
    reward = np.repeat(rew[:, None], A, 1)
    sc_new = st["step_count"][:, 0] + 1
    st["step_count"][:] = sc_new[:, None]
    real = observe(p, st)
    terminated = ~real["action_mask"][:, :, 1:].any((1, 2))  # every agent is connected or has no legal move
    term = terminated | (sc_new >= p.time_limit)
    ev["terminations"] = int(terminated.sum())
    ev["truncations"] = int((term & ~terminated).sum())
    new_ret = (st["run_return"] + rew).astype(np.float32)
    new_len = st["run_length"] + 1
    info_return = np.where(term, new_ret, st["ep_return"]).astype(np.float32)
    info_length = np.where(term, new_len, st["ep_length"]).astype(np.int32)
    st["run_return"][:] = np.where(term, np.float32(0), new_ret)
    st["run_length"][:] = np.where(term, 0, new_len)
    st["ep_return"][:] = info_return
    st["ep_length"][:] = info_length
    st["step_count"][:] = np.where(term, 0, sc_new)[:, None]
    real["step_count"] = st["step_count"].copy()
    # auto-reset at this step's counter; only the environments that ended are observed again
    ends = np.nonzero(term)[0]
    ev["fallbacks"] = _regenerate(p, st, ends, seed, env_offset, t)
    obs = {k: v.copy() for k, v in real.items()}
    if ends.size:
        sub = observe(p, {k: st[k][ends] for k in STATE_FIELDS})
        for k in obs:
            obs[k][ends] = sub[k]
    done = np.repeat(term.astype(np.uint8)[:, None], A, 1)
    extra = {"real_view": real["agents_view"], "real_mask": real["action_mask"], "terminated": terminated.astype(np.uint8),
             "events": ev}
    return obs, reward, done, info_return, info_length, term.astype(np.uint8), extra


# ---- hand-built states (tests/test_connector.py on this model, tests/test_gpu_connector.py on the kernel) -------------
def make_state(p: Params, agents, step_count: int = 0, run_return: float = 0.0, run_length: int = 0) -> dict:
    """One environment: agents [(head (r, c), target (r, c), [path cells])]; an agent whose head is its target is
    connected."""
    st = alloc_state(p, 1)
    for k, (head, target, path) in enumerate(agents):
        st["head"][0, k], st["target"][0, k] = head, target
        st["connected"][0, k] = head == target
        for cell in path:
            st["grid"][0][cell] = PATH + 3 * k
        st["grid"][0][target] = TARGET + 3 * k
        st["grid"][0][head] = HEAD + 3 * k
    st["step_count"][0] = step_count
    st["run_return"][0] = run_return
    st["run_length"][0] = run_length
    return st


SCRIPT_SEED = 0x1234


def run_case(p: Params, st: dict, action, t: int) -> dict:
    st = {k: v.copy() for k, v in st.items()}
    obs, reward, done, ir, il, it, extra = step(p, st, np.asarray(action, np.int32)[None], SCRIPT_SEED, 0, t)
    return {"state": st, "obs": obs, "reward": reward, "done": done, "info_return": ir, "info_length": il,
            "info_terminal": it, "real_view": extra["real_view"], "real_mask": extra["real_mask"],
            "terminated": extra["terminated"]}


def _view(res, p, j):
    return res["real_view"][0, j].reshape(p.G, p.G, 5)


def scripted_cases():
    """[(name, Params, state, action (A,), t, expect(result))]: one rule each.  `expect` reads only the transition and
    the pre-reset observation (real_view / real_mask / terminated), so it holds on a terminal step too."""
    P = Params(5, 3, 25)
    far = [((4, 0), (4, 4), []), ((0, 4), (0, 0), [])]  # agents 1 and 2, out of the way
    cases = []

    def add(name, p, agents, action, expect, **kw):
        cases.append((name, p, make_state(p, agents, **kw), np.array(action, np.int32), 7, expect))

    def moved(r):
        v = _view(r, P, 0)
        assert v[2, 2, 2] == 1 and v[2, 2, 3] == 0 and v[1, 2, 3] == 1 and v[1, 2, 0] == np.float32(1) / np.float32(3)
        assert _view(r, P, 1)[1, 2, 0] == np.float32(3) / np.float32(3) and _view(r, P, 2)[1, 2, 0] == np.float32(2) / np.float32(3)
        assert (r["reward"] == team_reward(0, 3)).all() and abs(float(r["reward"][0, 0]) + 0.09) < 1e-6
        assert not r["done"].any() and not r["terminated"].any() and r["real_mask"][0, 0].tolist() == [1, 1, 1, 0, 1]

    add("move-leaves-path", P, [((2, 2), (3, 4), [])] + far, [UP, NOOP, NOOP], moved)

    def stayed(cell, mask_bit, n_path=0):
        def expect(r):
            v = _view(r, P, 0)
            assert v[cell][3] == 1 and v[..., 2].sum() == n_path and v[..., 3].sum() == 1
            assert r["real_mask"][0, 0, mask_bit] == 0 and (r["reward"] == team_reward(0, 3)).all()
        return expect

    add("wall", P, [((0, 2), (3, 4), [])] + far, [UP, NOOP, NOOP], stayed((0, 2), UP))
    blockers = [((2, 3), (4, 4), [(1, 2)]), ((0, 0), (3, 2), [])]  # 1: path above, head right; 2: target below
    for name, a in (("blocked-by-path", UP), ("blocked-by-head", RIGHT), ("blocked-by-target", DOWN)):
        add(name, P, [((2, 2), (0, 4), [])] + blockers, [a, NOOP, NOOP], stayed((2, 2), a, 1))

    def connected(r):
        v = _view(r, P, 0)
        assert v[2, 3, 3] == 1 and v[2, 3, 4] == 0 and v[2, 3, 1] == 0 and v[2, 2, 2] == 1  # stored as head
        assert r["state"]["connected"][0].tolist() == [1, 0, 0] or r["done"].all()
        assert (r["reward"] == team_reward(1, 3)).all() and abs(float(r["reward"][0, 0]) - (1 - 0.03 * 3)) < 1e-6
        assert r["real_mask"][0, 0].tolist() == [1, 0, 0, 0, 0]

    add("own-target-connects", P, [((2, 2), (2, 3), [])] + far, [RIGHT, NOOP, NOOP], connected)

    def contested(n):
        def expect(r):
            assert all(_view(r, P, j)[..., 2].sum() == 0 for j in range(3)) and _view(r, P, 0)[2, 2].sum() == 0
            assert _view(r, P, 0)[2, 1, 3] == 1 and _view(r, P, 1)[2, 3, 3] == 1 and (r["reward"] == team_reward(0, 3)).all()
            assert r["real_mask"][0, 0, RIGHT] == 1 and r["real_mask"][0, 1, LEFT] == 1 and n in (2, 3)
        return expect

    add("two-contest-a-cell", P, [((2, 1), (4, 4), []), ((2, 3), (0, 0), []), ((0, 2), (4, 0), [])], [RIGHT, LEFT, NOOP],
        contested(2))
    add("three-contest-a-cell", P, [((2, 1), (4, 4), []), ((2, 3), (0, 0), []), ((1, 2), (4, 0), [])], [RIGHT, LEFT, DOWN],
        contested(3))

    def ignores(r):
        v = _view(r, P, 0)
        assert v[2, 2, 3] == 1 and v[..., 2].sum() == 1 and r["real_mask"][0, 0].tolist() == [1, 0, 0, 0, 0]
        assert (r["reward"] == team_reward(0, 2)).all() and abs(float(r["reward"][0, 0]) + 0.06) < 1e-6

    add("connected-agent-ignores-action", P, [((2, 2), (2, 2), [(2, 1)])] + far, [UP, NOOP, NOOP], ignores)

    Q = Params(3, 1, 25)
    boxed = [((0, 0), (2, 2), [(0, 1), (1, 0)])]  # its own path blocks it

    def ends(terminated, length):
        def expect(r):
            assert r["done"].all() and r["info_terminal"].all() and r["terminated"].tolist() == [terminated]
            assert r["info_length"].tolist() == [length] and r["info_return"][0] == np.float32(1.5) + r["reward"][0, 0]
        return expect

    add("all-blocked-terminates", Q, boxed, [NOOP], ends(1, 4), step_count=3, run_return=1.5, run_length=3)
    add("time-limit-truncates", Q, [((0, 0), (2, 2), [])], [NOOP], ends(0, 25), step_count=24, run_return=1.5, run_length=24)
    add("blocked-at-the-time-limit-terminates", Q, boxed, [RIGHT], ends(1, 25), step_count=24, run_return=1.5, run_length=24)
    return cases
