"""TEST INFRASTRUCTURE: NumPy / plain-Python restatement of the Robot Warehouse rules of mava_rware_step
(mava_amd/csrc/rware.hip, DESIGN.md "Robot Warehouse"), written independently of the kernel: the warehouse is a set of
highway cells and a list of home cells, shelves and agents are looked up in dictionaries of cells, every environment is
stepped by Python loops.  No row bit masks, no slot tables.

State and outputs use the device layouts: a state is a dict of arrays named like RwareState's fields.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.philox import philox4x32_10

RESET_STREAM = 0x52575253  # "RWRS"
QUEUE_STREAM = 0x52575251  # "RWRQ"
N_ACTIONS = 5
NOOP, FORWARD, LEFT, RIGHT, TOGGLE = range(5)
UP, EAST, DOWN, WEST = range(4)  # directions: y - 1, x + 1, y + 1, x - 1
_STEP = {UP: (0, -1), EAST: (1, 0), DOWN: (0, 1), WEST: (-1, 0)}
STATE_FIELDS = ("agent_pos", "agent_dir", "agent_carry", "shelf_pos", "request_queue", "step_count", "run_return",
                "run_length", "ep_return", "ep_length")
EVENTS = ("deliveries", "refills", "pickups", "putdowns", "collisions", "truncations")


@dataclass
class Params:
    column_height: int
    shelf_rows: int
    shelf_columns: int
    A: int
    sensor_range: int
    R: int
    time_limit: int = 500
    collision_mode: str = "terminate"

    def __post_init__(self):
        ch = self.column_height
        self.H = (ch + 1) * self.shelf_rows + 2
        self.W = 3 * self.shelf_columns + 1
        H, W = self.H, self.W
        self.goals = [(W // 2 - 1, H - 1), (W // 2, H - 1)]
        self.highway = {(x, y) for y in range(H) for x in range(W)
                        if x % 3 == 0 or y % (ch + 1) == 0 or y == H - 1 or (y > H - (ch + 3) and x in (W // 2 - 1, W // 2))}
        self.homes = [(x, y) for y in range(H) for x in range(W) if (x, y) not in self.highway]  # row-major
        self.S = len(self.homes)

    @property
    def raw_dim(self) -> int:
        return 8 + 7 * (2 * self.sensor_range + 1) ** 2

    @property
    def obs_dim(self) -> int:
        return self.A + self.raw_dim

    def cell(self, x, y) -> int:
        return y * self.W + x

    def shelf_of_home(self, x, y) -> int:
        return self.homes.index((x, y))


SCENARIOS = {  # name: (column_height, shelf_rows, shelf_columns, agents, sensor_range, request queue)
    "tiny-2ag": (8, 1, 3, 2, 1, 2), "tiny-4ag": (8, 1, 3, 4, 1, 4), "tiny-4ag-easy": (8, 1, 3, 4, 1, 8),
    "small-4ag": (8, 2, 3, 4, 1, 4),
}


def params_of(env) -> Params:
    """The Params of a mava_amd.envs.rware.RobotWarehouse."""
    return Params(env.column_height, env.shelf_rows, env.shelf_columns, env.num_agents, env.sensor_range,
                  env.request_queue_size, env.time_limit, env.collision_mode)


def draws(seed: int, g, t: int, n: int, stream: int) -> np.ndarray:
    """(len(g), n) uint32: draw k of env g is word k % 4 of Philox block k // 4, counter (g, t, k // 4, stream)."""
    g = np.atleast_1d(np.asarray(g, np.uint32))
    slo, shi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    out = np.empty((g.size, 4 * ((n + 3) // 4)), np.uint32)
    for k in range((n + 3) // 4):
        w = philox4x32_10(g, np.uint32(t & 0xFFFFFFFF), k, stream, slo, shi)
        for q in range(4):
            out[:, 4 * k + q] = w[q]
    return out[:, :n]


def generate(p: Params, dr) -> dict:
    """One environment's reset state from its 2 A + R draws."""
    d = iter(int(x) for x in dr)
    cells = [(x, y) for y in range(p.H) for x in range(p.W)]
    pos, dirs = [], []
    for _ in range(p.A):
        cand = [c for c in cells if c not in pos]
        pos.append(cand[next(d) % len(cand)])
        dirs.append(next(d) % 4)
    queue = []
    for _ in range(p.R):
        cand = [s for s in range(p.S) if s not in queue]
        queue.append(cand[next(d) % len(cand)])
    return {"agent_pos": np.array(pos, np.int32), "agent_dir": np.array(dirs, np.int32),
            "agent_carry": np.full(p.A, -1, np.int32), "shelf_pos": np.array([p.cell(x, y) for x, y in p.homes], np.int32),
            "request_queue": np.array(queue, np.int32)}


def alloc_state(p: Params, E: int) -> dict:
    return {"agent_pos": np.zeros((E, p.A, 2), np.int32), "agent_dir": np.zeros((E, p.A), np.int32),
            "agent_carry": np.full((E, p.A), -1, np.int32), "shelf_pos": np.zeros((E, p.S), np.int32),
            "request_queue": np.zeros((E, p.R), np.int32), "step_count": np.zeros((E, p.A), np.int32),
            "run_return": np.zeros(E, np.float32), "run_length": np.zeros(E, np.int32),
            "ep_return": np.zeros(E, np.float32), "ep_length": np.zeros(E, np.int32)}


def _regenerate(p: Params, st: dict, envs: np.ndarray, seed: int, env_offset: int, t: int) -> None:
    if envs.size == 0:
        return
    g = (envs.astype(np.uint64) + np.uint64(env_offset)).astype(np.uint32)
    dr = draws(seed, g, t, 2 * p.A + p.R, RESET_STREAM)
    for i, e in enumerate(envs):
        for k, v in generate(p, dr[i]).items():
            st[k][e] = v
        st["step_count"][e] = 0


def _forward_target(p: Params, pos, d, carrying, ground):
    """The cell a FORWARD takes the agent to, or None when rule 1 refuses the move."""
    tx, ty = pos[0] + _STEP[d][0], pos[1] + _STEP[d][1]
    if not (0 <= tx < p.W and 0 <= ty < p.H):
        return None
    if carrying and (tx, ty) in ground:
        return None
    return (tx, ty)


def _ground(p: Params, carry, shelf_pos) -> dict:
    """{(x, y): [shelf ids on the ground there]}."""
    out = {}
    for sid in range(p.S):
        if sid not in carry:
            c = int(shelf_pos[sid])
            out.setdefault((c % p.W, c // p.W), []).append(sid)
    return out


def observe_env(p: Params, pos, dirs, carry, shelf_pos, queue):
    """raw views (A, raw_dim) and action mask (A, 5) of one environment."""
    s = p.sensor_range
    carry = [int(c) for c in carry]
    ground = _ground(p, carry, shelf_pos)
    shelves_at = {}  # every shelf, ground or carried
    for sid in range(p.S):
        c = int(shelf_pos[sid])
        shelves_at.setdefault((c % p.W, c // p.W), []).append(sid)
    raw = np.zeros((p.A, p.raw_dim), np.float32)
    mask = np.ones((p.A, N_ACTIONS), np.uint8)
    for j in range(p.A):
        x, y = pos[j]
        head = [x, y, carry[j] >= 0] + [dirs[j] == k for k in range(4)] + [(x, y) in p.highway]
        raw[j, :8] = head
        o = 8
        for dy in range(-s, s + 1):
            for dx in range(-s, s + 1):
                c = (x + dx, y + dy)
                if 0 <= c[0] < p.W and 0 <= c[1] < p.H:
                    who = j if (dx, dy) == (0, 0) else next((k for k in range(p.A) if tuple(pos[k]) == c), None)
                    if who is not None:
                        raw[j, o] = 1
                        raw[j, o + 1 + dirs[who]] = 1
                    here = shelves_at.get(c, [])
                    raw[j, o + 5] = len(here) > 0
                    raw[j, o + 6] = any(sid in queue for sid in here)
                o += 7
        mask[j, FORWARD] = _forward_target(p, (x, y), dirs[j], carry[j] >= 0, ground) is not None
    return raw, mask


def observe(p: Params, st: dict) -> dict:
    """agents_view (E, A, A + raw), global_state (E, 1, A raw), action_mask (E, A, 5) of the current state."""
    E = st["agent_pos"].shape[0]
    av = np.zeros((E, p.A, p.obs_dim), np.float32)
    gs = np.zeros((E, 1, p.A * p.raw_dim), np.float32)
    mask = np.zeros((E, p.A, N_ACTIONS), np.uint8)
    eye = np.eye(p.A, dtype=np.float32)
    for e in range(E):
        pos = [tuple(int(v) for v in q) for q in st["agent_pos"][e]]
        raw, mask[e] = observe_env(p, pos, [int(d) for d in st["agent_dir"][e]], st["agent_carry"][e], st["shelf_pos"][e],
                                   [int(q) for q in st["request_queue"][e]])
        av[e] = np.concatenate([eye, raw], -1)
        gs[e, 0] = raw.reshape(-1)
    return {"agents_view": av, "global_state": gs, "action_mask": mask, "step_count": st["step_count"].copy()}


def reset(p: Params, E: int, seed: int, env_offset: int = 0, t: int = 0):
    st = alloc_state(p, E)
    _regenerate(p, st, np.arange(E), seed, env_offset, t)
    return st, observe(p, st)


def _rules_env(p: Params, st: dict, e: int, act, seed: int, g: int, t: int, ev: dict):
    """Rules 1-5 of one environment, in place.  Returns (deliveries, collided)."""
    A = p.A
    pos = [tuple(int(v) for v in q) for q in st["agent_pos"][e]]
    dirs = [int(d) for d in st["agent_dir"][e]]
    carry = [int(c) for c in st["agent_carry"][e]]
    shelf_pos = st["shelf_pos"][e]
    queue = [int(q) for q in st["request_queue"][e]]
    start = list(pos)
    ground = _ground(p, carry, shelf_pos)  # the state at the start of the step
    # 1. turns and moves
    for j in range(A):
        a = int(act[j])
        if a == LEFT:
            dirs[j] = (dirs[j] + 3) % 4
        elif a == RIGHT:
            dirs[j] = (dirs[j] + 1) % 4
        elif a == FORWARD:
            tgt = _forward_target(p, pos[j], dirs[j], carry[j] >= 0, ground)
            if tgt is not None:
                pos[j] = tgt
    # 2. collision
    collided = False
    for j in range(A):
        for k in range(j):
            if pos[j] == pos[k] or (pos[j] == start[k] and pos[k] == start[j] and start[j] != start[k]):
                collided = True
    # 3. carried shelves follow
    for j in range(A):
        if carry[j] >= 0:
            shelf_pos[carry[j]] = p.cell(*pos[j])
    # 4. toggle, in index order
    for j in range(A):
        if int(act[j]) != TOGGLE:
            continue
        here = _ground(p, carry, shelf_pos).get(pos[j], [])
        if carry[j] < 0:
            if here:
                carry[j] = here[0]
                ev["pickups"] += 1
        elif pos[j] not in p.highway and not here:
            carry[j] = -1
            ev["putdowns"] += 1
    # 5. deliveries, in index order
    n = 0
    for j in range(A):
        if carry[j] >= 0 and pos[j] in p.goals and carry[j] in queue:
            n += 1
            d = int(draws(seed, [g], t, j + 1, QUEUE_STREAM)[0, j])
            cand = [s for s in range(p.S) if s not in queue]
            queue[queue.index(carry[j])] = cand[d % (p.S - p.R)]
            ev["deliveries"] += 1
            ev["refills"] += 1
    st["agent_pos"][e] = pos
    st["agent_dir"][e] = dirs
    st["agent_carry"][e] = carry
    st["request_queue"][e] = queue
    return n, collided


def step(p: Params, st: dict, action: np.ndarray, seed: int, env_offset: int, t: int):
    """One step of every environment, in place on `st`.  Returns (obs, reward (E, A) f32, done (E, A) u8,
    info_return (E,) f32, info_length (E,) i32, info_terminal (E,) u8, extra) with extra = {"real_view", "real_mask"
    (the observation before any auto-reset), "terminated" (E,) u8, "events": counts of what happened}."""
    E, A = st["agent_pos"].shape[0], p.A
    act = np.asarray(action, np.int32).reshape(E, A)
    ev = {k: 0 for k in EVENTS}
    n_del = np.zeros(E, np.float32)
    coll = np.zeros(E, bool)
    for e in range(E):
        g = (e + env_offset) & 0xFFFFFFFF
        n_del[e], coll[e] = _rules_env(p, st, e, act[e], seed, g, t, ev)
    ev["collisions"] = int(coll.sum())
    # 6. reward, terminal + RecordEpisodeMetrics
    reward = np.repeat(n_del[:, None], A, 1)
    sc_new = st["step_count"][:, 0] + 1
    terminated = coll & (p.collision_mode == "terminate")
    term = terminated | (sc_new >= p.time_limit)
    ev["truncations"] = int((term & ~terminated).sum())
    new_ret = (st["run_return"] + n_del).astype(np.float32)
    new_len = st["run_length"] + 1
    info_return = np.where(term, new_ret, st["ep_return"]).astype(np.float32)
    info_length = np.where(term, new_len, st["ep_length"]).astype(np.int32)
    st["run_return"][:] = np.where(term, np.float32(0), new_ret)
    st["run_length"][:] = np.where(term, 0, new_len)
    st["ep_return"][:] = info_return
    st["ep_length"][:] = info_length
    st["step_count"][:] = np.where(term, 0, sc_new)[:, None]
    real = observe(p, st)
    # auto-reset at this step's counter; only the environments that ended are observed again
    ends = np.nonzero(term)[0]
    _regenerate(p, st, ends, seed, env_offset, t)
    obs = {k: v.copy() for k, v in real.items()}
    if ends.size:
        sub = observe(p, {k: st[k][ends] for k in STATE_FIELDS})
        for k in obs:
            obs[k][ends] = sub[k]
    done = np.repeat(term.astype(np.uint8)[:, None], A, 1)
    extra = {"real_view": real["agents_view"], "real_mask": real["action_mask"], "terminated": terminated.astype(np.uint8),
             "events": ev}
    return obs, reward, done, info_return, info_length, term.astype(np.uint8), extra


# ---- hand-built states (tests/test_rware.py on this model, tests/test_gpu_rware.py on the kernel) ---------------------
def make_state(p: Params, agents, queue, step_count: int = 0, run_return: float = 0.0, run_length: int = 0,
               moved=None) -> dict:
    """One environment: agents [(x, y, direction, carried shelf or -1)], the request queue, `moved` {shelf: (x, y)} for
    ground shelves away from their homes.  A carried shelf takes its carrier's cell."""
    st = alloc_state(p, 1)
    st["agent_pos"][0] = [(x, y) for x, y, _, _ in agents]
    st["agent_dir"][0] = [d for _, _, d, _ in agents]
    st["agent_carry"][0] = [c for _, _, _, c in agents]
    st["shelf_pos"][0] = [p.cell(x, y) for x, y in p.homes]
    for sid, (x, y) in (moved or {}).items():
        st["shelf_pos"][0, sid] = p.cell(x, y)
    for x, y, _, c in agents:
        if c >= 0:
            st["shelf_pos"][0, c] = p.cell(x, y)
    st["request_queue"][0] = queue
    st["step_count"][0] = step_count
    st["run_return"][0] = run_return
    st["run_length"][0] = run_length
    return st


def _agent(res, j):
    s = res["state"]
    return (int(s["agent_pos"][0, j, 0]), int(s["agent_pos"][0, j, 1]), int(s["agent_dir"][0, j]), int(s["agent_carry"][0, j]))


SCRIPT_SEED = 0x1234


def scripted_cases():
    """[(name, Params, state, action (1, A), t, expect(res))]: res holds state (after the step), obs, reward, done,
    info_return, info_length, info_terminal, real_view, real_mask, terminated."""
    p = Params(8, 1, 3, 2, 1, 2)  # tiny-2ag: 11 rows x 10 columns, homes at x in {1, 2, 7, 8}, y in 1 .. 8
    po = Params(8, 1, 3, 2, 1, 2, collision_mode="overlap")
    pt = Params(8, 1, 3, 2, 1, 2, time_limit=20)
    sh = p.shelf_of_home
    far = (9, 0, UP, -1)  # a bystander in the top right corner
    q0 = [sh(7, 7), sh(8, 8)]  # requests nobody touches
    cases = []

    def add(name, pp, agents, queue, action, expect, t=5, **kw):
        cases.append((name, pp, make_state(pp, agents, queue, **kw), np.array([action], np.int32), t, expect))

    def quiet(res):
        assert not res["reward"].any() and not res["done"].any() and not res["terminated"].any()
        assert res["info_terminal"][0] == 0 and res["state"]["step_count"][0].tolist() == [1, 1]

    def forward(res):
        quiet(res)
        assert _agent(res, 0) == (0, 4, UP, -1) and _agent(res, 1) == (8, 0, WEST, -1)
        assert np.array_equal(res["state"]["shelf_pos"][0], [p.cell(x, y) for x, y in p.homes])
    add("forward_moves", p, [(0, 5, UP, -1), (9, 0, WEST, -1)], q0, [FORWARD, FORWARD], forward)

    def off_grid(res):
        quiet(res)
        assert _agent(res, 0) == (0, 0, UP, -1) and _agent(res, 1) == (9, 10, EAST, -1)
        assert res["obs"]["action_mask"][0].tolist() == [[1, 0, 1, 1, 1]] * 2
    add("forward_off_grid_refused", p, [(0, 0, UP, -1), (9, 10, EAST, -1)], q0, [FORWARD, FORWARD], off_grid)

    def under(res):  # an unloaded agent drives under a ground shelf
        quiet(res)
        assert _agent(res, 0) == (2, 2, WEST, -1)
    add("unloaded_agent_passes_under_shelf", p, [(3, 2, WEST, -1), far], q0, [FORWARD, NOOP], under)

    def blocked(res):  # shelf (2, 1) carried at (3, 2); the shelf of (2, 2) stands in the way
        quiet(res)
        assert _agent(res, 0) == (3, 2, WEST, sh(2, 1)) and res["state"]["shelf_pos"][0, sh(2, 1)] == p.cell(3, 2)
        assert res["obs"]["action_mask"][0, 0].tolist() == [1, 0, 1, 1, 1]
    add("carrier_blocked_by_ground_shelf", p, [(3, 2, WEST, sh(2, 1)), far], q0, [FORWARD, NOOP], blocked)

    def free(res):  # the carried shelf's own home is empty: nothing in the way
        quiet(res)
        assert _agent(res, 0) == (2, 1, WEST, sh(2, 1)) and res["state"]["shelf_pos"][0, sh(2, 1)] == p.cell(2, 1)
    add("carrier_passes_over_empty_home", p, [(3, 1, WEST, sh(2, 1)), far], q0, [FORWARD, NOOP], free)

    def turns(res):
        quiet(res)
        assert _agent(res, 0) == (0, 5, WEST, -1) and _agent(res, 1) == (9, 0, UP, -1)
        assert res["obs"]["agents_view"][0, 0, 2:10].tolist() == [0, 5, 0, 0, 0, 0, 1, 1]
    add("turn_left_and_right", p, [(0, 5, UP, -1), (9, 0, WEST, -1)], q0, [LEFT, RIGHT], turns)

    def pickup(res):
        quiet(res)
        assert _agent(res, 0) == (1, 1, UP, sh(1, 1)) and _agent(res, 1) == (0, 5, UP, -1)  # nothing to lift at (0, 5)
        assert res["obs"]["agents_view"][0, 0, 2:5].tolist() == [1, 1, 1]
    add("pick_up", p, [(1, 1, UP, -1), (0, 5, UP, -1)], q0, [TOGGLE, TOGGLE], pickup)

    def highway(res):
        quiet(res)
        assert _agent(res, 0) == (3, 1, UP, sh(2, 1))
    add("put_down_refused_on_highway", p, [(3, 1, UP, sh(2, 1)), far], q0, [TOGGLE, NOOP], highway)

    def putdown(res):  # onto a foreign, empty home: (1, 1)'s shelf is away with agent 1
        quiet(res)
        assert _agent(res, 0) == (1, 1, UP, -1) and res["state"]["shelf_pos"][0, sh(2, 1)] == p.cell(1, 1)
        v = res["obs"]["agents_view"][0, 0, 2:]
        assert v[2] == 0 and v[8 + 7 * 4 + 5] == 1  # not carrying; a shelf on the centre cell
    add("put_down_on_empty_home", p, [(1, 1, UP, sh(2, 1)), (0, 5, UP, sh(1, 1))], q0, [TOGGLE, NOOP], putdown)

    def toggle_order(res):  # overlap mode, two carriers on one empty home: the lower index unloads, the other cannot
        assert _agent(res, 0)[3] == -1 and _agent(res, 1)[3] == sh(2, 1) and not res["done"].any()
    add("toggle_in_index_order", po, [(1, 1, UP, sh(1, 1)), (1, 1, DOWN, sh(2, 1))], q0, [TOGGLE, TOGGLE], toggle_order)

    def expect_refill(queue, slot_draws):
        """The queue after refilling, in order, [(delivered shelf, draw)]."""
        queue = list(queue)
        for sid, d in slot_draws:
            cand = sorted(set(range(p.S)) - set(queue))
            queue[queue.index(sid)] = cand[d % (p.S - p.R)]
        return queue

    def delivery(res):
        d = int(draws(SCRIPT_SEED, [0], 5, 1, QUEUE_STREAM)[0, 0])
        want = expect_refill([sh(1, 1), sh(8, 8)], [(sh(1, 1), d)])
        q = res["state"]["request_queue"][0].tolist()
        assert q == want and sh(1, 1) not in q and len(set(q)) == 2 and q[1] == sh(8, 8)
        assert res["reward"][0].tolist() == [1.0, 1.0] and not res["done"].any()
        assert _agent(res, 0) == (4, 10, DOWN, sh(1, 1))  # keeps the shelf
        assert res["state"]["run_return"][0] == 1.0 and res["info_return"][0] == 0.0
    add("delivery_refills_the_queue", p, [(4, 9, DOWN, sh(1, 1)), far], [sh(1, 1), sh(8, 8)], [FORWARD, NOOP], delivery)

    def no_request(res):
        quiet(res)
        assert _agent(res, 0) == (4, 10, DOWN, sh(1, 1)) and res["state"]["request_queue"][0].tolist() == q0
    add("unrequested_shelf_scores_nothing", p, [(4, 9, DOWN, sh(1, 1)), far], q0, [FORWARD, NOOP], no_request)

    def two(res):  # agent 1's refill sees agent 0's
        dr = draws(SCRIPT_SEED, [0], 5, 2, QUEUE_STREAM)[0]
        want = expect_refill([sh(2, 2), sh(1, 1)], [(sh(1, 1), int(dr[0])), (sh(2, 2), int(dr[1]))])
        q = res["state"]["request_queue"][0].tolist()
        assert q == want and len(set(q)) == 2 and q[1] != sh(1, 1) and q[0] != sh(2, 2)
        assert res["reward"][0].tolist() == [2.0, 2.0]
    add("two_deliveries_in_one_step", p, [(4, 9, DOWN, sh(1, 1)), (6, 10, WEST, sh(2, 2))], [sh(2, 2), sh(1, 1)],
        [FORWARD, FORWARD], two)

    def ended(res, pp, t, terminated, length):
        assert res["done"][0].tolist() == [1, 1] and res["info_terminal"][0] == 1 and res["terminated"][0] == terminated
        assert res["info_length"][0] == length and res["state"]["run_length"][0] == 0
        assert res["obs"]["step_count"][0].tolist() == [0, 0]
        fresh, fobs = reset(pp, 1, SCRIPT_SEED, 0, t)
        for k in ("agent_pos", "agent_dir", "agent_carry", "shelf_pos", "request_queue"):
            assert np.array_equal(res["state"][k], fresh[k]), k
        for k in ("agents_view", "global_state", "action_mask"):
            assert np.array_equal(res["obs"][k], fobs[k]), k

    def same_cell(res):
        ended(res, p, 5, 1, 4)
        assert res["real_view"][0, :, 2:4].tolist() == [[0, 5], [0, 5]]  # the pre-reset view: both on (0, 5)
        assert res["real_view"][0, 1, 2 + 8 + 7 * 4: 2 + 8 + 7 * 4 + 5].tolist() == [1, 1, 0, 0, 0]  # centre: itself (UP)
    add("same_cell_collision_terminates", p, [(0, 4, DOWN, -1), (0, 6, UP, -1)], q0, [FORWARD, FORWARD], same_cell,
        step_count=3, run_length=3)

    def same_cell_overlap(res):
        quiet(res)
        assert _agent(res, 0)[:2] == (0, 5) and _agent(res, 1)[:2] == (0, 5)
        # agent 1 sees itself on the centre cell, agent 0 (the lowest index) is what agent 1's neighbours would see
        assert res["obs"]["agents_view"][0, 1, 2 + 8 + 7 * 4: 2 + 8 + 7 * 4 + 5].tolist() == [1, 1, 0, 0, 0]
    add("same_cell_overlap_mode", po, [(0, 4, DOWN, -1), (0, 6, UP, -1)], q0, [FORWARD, FORWARD], same_cell_overlap)

    def swap(res):
        ended(res, p, 5, 1, 1)
        assert res["real_view"][0, :, 2:4].tolist() == [[0, 5], [0, 4]]
    add("swap_collision_terminates", p, [(0, 4, DOWN, -1), (0, 5, UP, -1)], q0, [FORWARD, FORWARD], swap)

    def swap_overlap(res):
        quiet(res)
        assert _agent(res, 0)[:2] == (0, 5) and _agent(res, 1)[:2] == (0, 4)
    add("swap_overlap_mode", po, [(0, 4, DOWN, -1), (0, 5, UP, -1)], q0, [FORWARD, FORWARD], swap_overlap)

    def truncation(res):
        ended(res, pt, 9, 0, 20)
        assert res["info_return"][0] == 3.0 and res["real_view"][0, 0, 2:4].tolist() == [0, 5]
    add("time_limit_is_a_truncation", pt, [(0, 5, UP, -1), far], q0, [NOOP, NOOP], truncation, t=9, step_count=19,
        run_length=19, run_return=3.0)

    def view(res):  # agent 0 at (3, 2) facing EAST; agent 1 to its west on (2, 2), under a requested ground shelf
        quiet(res)
        v = res["obs"]["agents_view"][0, 0]
        assert v[:2].tolist() == [1, 0] and v[2:10].tolist() == [3, 2, 0, 0, 1, 0, 0, 1]
        cell = lambda c: v[10 + 7 * c: 17 + 7 * c].tolist()  # noqa: E731
        assert cell(3) == [1, 0, 0, 1, 0, 1, 1]  # west: agent 1 facing DOWN, shelf, requested
        assert cell(0) == [0, 0, 0, 0, 0, 1, 0]  # north-west (2, 1): a shelf nobody asked for
        assert cell(4) == [1, 0, 1, 0, 0, 0, 0] and cell(5) == [0] * 7  # itself; east (4, 2) is empty
        g = res["obs"]["global_state"][0, 0]
        assert np.array_equal(g[:71], v[2:]) and np.array_equal(g[71:], res["obs"]["agents_view"][0, 1, 2:])
        w = res["obs"]["agents_view"][0, 1]
        assert w[:2].tolist() == [0, 1] and w[2:10].tolist() == [2, 2, 0, 0, 0, 1, 0, 0]
    add("view_contents", p, [(3, 2, EAST, -1), (2, 2, DOWN, -1)], [sh(2, 2), sh(8, 8)], [NOOP, NOOP], view)

    def edge(res):  # the corner agent's off-grid cells are zeros
        v = res["obs"]["agents_view"][0, 0, 10:]
        for c in (0, 1, 2, 3, 6):
            assert v[7 * c: 7 * c + 7].tolist() == [0] * 7
        assert v[7 * 4: 7 * 4 + 5].tolist() == [1, 1, 0, 0, 0]
    add("view_off_grid_cells", p, [(0, 0, UP, -1), (9, 10, EAST, -1)], q0, [NOOP, NOOP], edge)
    return cases


def run_case(p: Params, st: dict, action, t: int) -> dict:
    st = {k: v.copy() for k, v in st.items()}
    obs, rew, done, ir, il, it, extra = step(p, st, action, SCRIPT_SEED, 0, t)
    return {"state": st, "obs": obs, "reward": rew, "done": done, "info_return": ir, "info_length": il,
            "info_terminal": it, "real_view": extra["real_view"], "real_mask": extra["real_mask"],
            "terminated": extra["terminated"]}


# ---- crafted starts for the random-action comparison (random walks almost never deliver) ------------------------------
def craft(p: Params, st: dict, envs, kind: str) -> None:
    """Overwrite the given environments of a reset state: "deliver" - agent 0 one step above the left goal, facing it,
    carrying the first requested shelf; "collide" - agents 0 and 1 two cells apart on the top row, facing each other."""
    for e in envs:
        if kind == "deliver":
            gx, gy = p.goals[0]
            sid = int(st["request_queue"][e, 0])
            st["agent_pos"][e, 0] = (gx, gy - 1)
            st["agent_dir"][e, 0] = DOWN
            st["agent_carry"][e, 0] = sid
            st["shelf_pos"][e, sid] = p.cell(gx, gy - 1)
            for j in range(1, p.A):  # the others wait in the top row, apart
                st["agent_pos"][e, j] = (3 * (j - 1), 0)
                st["agent_carry"][e, j] = -1
        elif kind == "collide" and p.A >= 2:
            st["agent_pos"][e, 0], st["agent_dir"][e, 0] = (0, 0), EAST
            st["agent_pos"][e, 1], st["agent_dir"][e, 1] = (2, 0), WEST
            for j in range(2, p.A):
                st["agent_pos"][e, j] = (3 * j, p.H - 1)
            st["agent_carry"][e] = -1
