// Connector environment step (DESIGN.md "Connector"; the rules are the contract of mava_connector_step in
// include/mava_hip.h and are stated in NumPy in tests/connector_model.py).  A G x G board, A agents that each grow a path
// from their head towards their own target; a cell holds 0 (empty) or 1 + 3k / 2 + 3k / 3 + 3k (path / head / target of
// agent k).  Wrapper semantics of the reference's ConnectorWrapper: image observations (G, G, 5) per agent WITHOUT a
// prepended agent id (the channels encode the agent index relative to the viewer), global_state = agent 0's first three
// channels, team reward repeated per agent, AutoResetWrapper and RecordEpisodeMetrics bookkeeping (env_common.h).
//
// The rules are small and the output is large (con-10x10x10a: 21 KB of observation per env and step), so the kernel is
// shaped by its stores.  A workgroup of THREADS = 64 NE threads owns NE environments:
//   state load    - wave w copies environment w's board into LDS as bytes (256 B) and clears its claim table; lane k < A
//                   holds agent k.  Every loaded value is clamped to its range: a corrupt state cannot index outside a table;
//   rule phase    - one lane per agent.  A mover adds 1 to the byte of its destination in the claim table (G G bytes per
//                   env, updated through 32-bit LDS atomics on the containing word: at most four agents can want one
//                   cell, a byte cannot overflow); after a barrier it moves iff that byte is 1.  No A x A compare.  The
//                   counts the reward needs come from two wave ballots;
//   mask / end    - lane k tests its four destinations on the new board; a ballot says whether anybody can move;
//   reset         - the rare case: lane 0 of the wave runs the generator on 16-bit occupancy row masks (candidates =
//                   empty & (left | right | up | down of empty), counted with popcount), then all lanes clear the walks;
//   output phase  - all threads.  A wave writes whole (env, agent) rows of G G 5 consecutive floats (G G 3 for the
//                   global state), each lane four consecutive floats decoded from the LDS bytes of the one or two cells
//                   they belong to, as one aligned float4 store; G G 5 is no multiple of 4 and a trajectory slot need not
//                   be 16-byte aligned, so each row starts with up to three scalar stores to reach alignment and ends
//                   with up to three.  The only divisions are by the constants 5 and 3.
// Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays from a captured
// graph.  The REAL instantiation of the same body (real_view given) also writes the pre-reset
// agents_view / action_mask and the `terminated` flag (nobody can move; a time-limit end alone is a truncation).
#include "env_common.h"

namespace {

constexpr uint32_t CON_RESET = 0x434F4E52u;  // "CONR"
constexpr int MAXG = 16, MAXA = 32, MAXGG = MAXG * MAXG;
constexpr int NE = 4;             // environments per workgroup, one wave each in the rule phase
constexpr int THREADS = 64 * NE;
constexpr int N_ACT = 5;          // NOOP UP RIGHT DOWN LEFT
constexpr int NCH = 5, NGS = 3;   // channels of agents_view / global_state

struct ConTable {
  float rel[MAXA + 1];  // rel[i] = i / A, divided on the host
};

struct ConArgs {
  int E, A, G, time_limit;
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  int32_t* head;             // (E, A, 2) (row, col)
  int32_t* target;           // (E, A, 2)
  uint8_t* connected;        // (E, A)
  uint8_t* grid;             // (E, G, G)
  int32_t* step_count;       // (E, A)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, A, G G 5)
  float* global_state;       // (E, 1, G G 3)
  uint8_t* action_mask;      // (E, A, 5)
  int32_t* obs_step_count;   // (E, A)
  float* reward;             // (E, A) or null (reset)
  uint8_t* done;
  float* info_return;
  int32_t* info_length;
  uint8_t* info_terminal;
  const int32_t* action;     // (E, A) or null (reset)
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct ConReal {
  float* view;               // (E, A, G G 5) pre-reset agents_view
  uint8_t* mask;             // (E, A, 5) pre-reset action_mask
  uint8_t* terminated;       // (E)
};

struct Tile {
  uint8_t grid[NE][MAXGG];
  uint32_t claim[NE][MAXGG / 4];
  uint16_t occ[NE][MAXG];      // the generator's occupancy row masks
  uint8_t hc[NE][MAXA], tc[NE][MAXA], conn[NE][MAXA];  // head / target cell (row * G + col), connected
  uint8_t mask[NE][MAXA * N_ACT];
  float rel[MAXA + 1];
  int sc[NE], term[NE], rst[NE];
  float rew[NE];
};

// the cell a move takes (r, c) to, or -1 off the grid
__device__ __forceinline__ int dest_of(int r, int c, int m, int G) {
  const int nr = r + (m == 3) - (m == 1), nc = c + (m == 2) - (m == 4);
  return (nr < 0 || nr >= G || nc < 0 || nc >= G) ? -1 : nr * G + nc;
}

// rule 1's test on a destination: on the grid, and empty or agent k's own target
__device__ __forceinline__ bool can_enter(const uint8_t* grid, int d, int k) {
  if (d < 0) return false;
  const int v = grid[d];
  return v == 0 || v == 3 + 3 * k;
}

// lane k < A: the action mask of agent k on the board in LDS; returns whether any move is legal
__device__ __forceinline__ bool build_mask(Tile& s, int le, int k, int G) {
  const int cell = s.hc[le][k], r = (unsigned)cell / (unsigned)G, c = cell - r * G;
  const bool open = !s.conn[le][k];
  bool any = false;
  s.mask[le][k * N_ACT] = 1;
#pragma unroll
  for (int m = 1; m < N_ACT; ++m) {
    const bool ok = open && can_enter(s.grid[le], dest_of(r, c, m, G), k);
    s.mask[le][k * N_ACT + m] = ok ? 1 : 0;
    any |= ok;
  }
  return any;
}

// the reset rule (one lane per environment): for every agent a start among the empty cells that have an empty
// neighbour, a length, and a self-avoiding walk; draw n = word n % 4 of Philox block n / 4, every draw is used.  The walk
// cells stay marked as paths until the caller clears them; the caller has emptied s.grid and s.occ.
__device__ void generate(const ConArgs& a, Tile& s, int le, uint32_t g, uint32_t t) {
  const int G = a.G, A = a.A;
  const uint32_t full = (1u << G) - 1u;
  const uint32_t lmax = (uint32_t)max(1, (G * G - 2) / A - 1);
  Philox4 p = {0u, 0u, 0u, 0u};
  int nd = 0;
  auto draw = [&]() -> uint32_t {
    if ((nd & 3) == 0) p = philox4x32_10(g, t, (uint32_t)(nd >> 2), CON_RESET, a.seed_lo, a.seed_hi);
    const uint32_t w = word_of(p, nd & 3);
    ++nd;
    return w;
  };
  for (int k = 0; k < A; ++k) {
    uint32_t emp[MAXG], cand[MAXG];
    int n = 0;
#pragma unroll
    for (int r = 0; r < MAXG; ++r) emp[r] = r < G ? (~(uint32_t)s.occ[le][r] & full) : 0u;
#pragma unroll
    for (int r = 0; r < MAXG; ++r) {
      const uint32_t up = r > 0 ? emp[r - 1] : 0u, dn = r < MAXG - 1 ? emp[r + 1] : 0u;
      cand[r] = emp[r] & ((emp[r] << 1) | (emp[r] >> 1) | up | dn);
      n += __popc(cand[r]);
    }
    const bool walk = n > 0;
    // the (idx)-th cell in row-major order of `cand` (a start) or of `emp` (the fallback's first empty cell)
    auto nth = [&](const uint32_t* rows, int idx) -> int {
      int rr = 0, rem = idx;
      uint32_t m = 0u;
      bool found = false;
#pragma unroll
      for (int r = 0; r < MAXG; ++r) {
        const int c = __popc(rows[r]);
        if (!found) {
          if (rem < c) { rr = r; m = rows[r]; found = true; }
          else rem -= c;
        }
      }
      for (int b = 0; b < rem; ++b) m &= m - 1u;
      return rr * G + (m ? __ffs(m) - 1 : 0);
    };
    int start, cur;
    if (walk) {
      start = nth(cand, (int)(draw() % (uint32_t)n));
      const int len = 1 + (int)(draw() % lmax);
      cur = start;
      int r = (unsigned)cur / (unsigned)G, c = cur - r * G;
      s.occ[le][r] |= (uint16_t)(1u << c);
      for (int st = 0; st < len; ++st) {
        // empty neighbours listed UP, RIGHT, DOWN, LEFT
        const uint32_t here = s.occ[le][r];
        const bool f0 = r > 0 && !((s.occ[le][max(r - 1, 0)] >> c) & 1u);
        const bool f1 = c < G - 1 && !((here >> (c + 1)) & 1u);
        const bool f2 = r < G - 1 && !((s.occ[le][min(r + 1, G - 1)] >> c) & 1u);
        const bool f3 = c > 0 && !((here >> max(c - 1, 0)) & 1u);
        const int cnt = f0 + f1 + f2 + f3;
        if (cnt == 0) break;
        int pick = (int)(draw() % (uint32_t)cnt);
        int m = 0;  // the pick-th free direction
        if (f0) { if (pick == 0) m = 1; --pick; }
        if (f1 && m == 0) { if (pick == 0) m = 2; --pick; }
        if (f2 && m == 0) { if (pick == 0) m = 3; --pick; }
        if (f3 && m == 0) { if (pick == 0) m = 4; --pick; }
        r += (m == 3) - (m == 1);
        c += (m == 2) - (m == 4);
        cur = r * G + c;
        s.occ[le][r] |= (uint16_t)(1u << c);
        s.grid[le][cur] = (uint8_t)(1 + 3 * k);
      }
    } else {  // no candidate: the first two empty cells (the scenario bound 2 A <= G G - 2 guarantees them)
      start = nth(emp, 0);
      cur = nth(emp, 1);
      s.occ[le][(unsigned)start / (unsigned)G] |= (uint16_t)(1u << (start - ((unsigned)start / (unsigned)G) * G));
      s.occ[le][(unsigned)cur / (unsigned)G] |= (uint16_t)(1u << (cur - ((unsigned)cur / (unsigned)G) * G));
    }
    s.grid[le][start] = (uint8_t)(2 + 3 * k);
    s.grid[le][cur] = (uint8_t)(3 + 3 * k);
    s.hc[le][k] = (uint8_t)start;
    s.tc[le][k] = (uint8_t)cur;
    s.conn[le][k] = 0;
  }
  s.sc[le] = 0;
}

// one observation value: channel ch of the cell byte v as agent j sees it
__device__ __forceinline__ float channel(unsigned v, int ch, int j, int A, const float* rel) {
  if (v == 0u) return 0.0f;
  const int k = (int)((v - 1u) / 3u), kind = (int)(v - 1u) - 3 * k;  // kind 0 path, 1 head, 2 target
  if (ch == 2) return kind == 0 ? 1.0f : 0.0f;
  if (ch >= 3) return (k == j && kind == ch - 2) ? 1.0f : 0.0f;
  return kind == ch + 1 ? rel[k - j + (k < j ? A : 0) + 1] : 0.0f;
}

// one wave writes one row of GG * C consecutive floats at `o`: the C channels of every cell as agent j sees them.  Lanes
// take four consecutive floats each and store them as one aligned float4; up to three scalar stores in front reach the
// alignment and up to three finish the row.
template <int C>
__device__ __forceinline__ void write_row(float* o, const uint8_t* grid, const float* rel, int GG, int j, int A, int lane) {
  const int RL = GG * C;
  const int lead = min((int)((4u - (unsigned)(((uintptr_t)o >> 2) & 3u)) & 3u), RL);
  const int nvec = (RL - lead) >> 2, tail0 = lead + 4 * nvec;
  auto value = [&](int q) -> float {
    const int cell = (unsigned)q / (unsigned)C;
    return channel(grid[cell], q - cell * C, j, A, rel);
  };
  for (int i = lane; i < nvec; i += 64) {
    const int q0 = lead + 4 * i;
    int cell = (unsigned)q0 / (unsigned)C, ch = q0 - cell * C;
    unsigned v = grid[cell];
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = channel(v, ch, j, A, rel);
      if (++ch == C) {
        ch = 0;
        cell = min(cell + 1, GG - 1);
        v = grid[cell];
      }
    }
    *reinterpret_cast<float4*>(o + q0) = make_float4(x[0], x[1], x[2], x[3]);
  }
  if (lane < lead) o[lane] = value(lane);
  if (lane >= 32 && lane - 32 < RL - tail0) o[tail0 + lane - 32] = value(tail0 + lane - 32);
}

// all threads: the agents_view rows (and, when gs is not null, the global_state rows) and masks of the workgroup
__device__ __forceinline__ void write_obs(const ConArgs& a, const Tile& s, float* av, float* gs, uint8_t* mk, int e0, int ne,
                                          int tid) {
  const int A = a.A, GG = a.G * a.G, lane = tid & 63, wave = tid >> 6;
  const long RLa = (long)GG * NCH, RLg = (long)GG * NGS;
  for (int row = wave; row < ne * A; row += NE) {
    const int le = (unsigned)row / (unsigned)A, j = row - le * A;
    write_row<NCH>(av + ((long)e0 * A + row) * RLa, s.grid[le], s.rel, GG, j, A, lane);
  }
  if (gs != nullptr)
    for (int le = wave; le < ne; le += NE) write_row<NGS>(gs + (long)(e0 + le) * RLg, s.grid[le], s.rel, GG, 0, A, lane);
  const int nm = A * N_ACT;
  for (int le = wave; le < ne; le += NE)
    for (int i = lane; i < nm; i += 64) mk[(long)(e0 + le) * nm + i] = s.mask[le][i];
}

template <bool REAL>
__device__ __forceinline__ void connector_step_body(const ConArgs& a, const ConTable& tab, const ConReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x, lane = tid & 63, le = tid >> 6;  // wave le owns environment e0 + le
  const int A = a.A, G = a.G, GG = G * G;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);
  if (ne <= 0) return;
  const bool live = le < ne;            // wave-uniform
  const bool agent = live && lane < A;  // lane k holds agent k
  const int e = e0 + le;
  const long ka = (long)e * A + lane;

  // ---------------------------------------------------------------- state load
  for (int i = tid; i <= A; i += THREADS) s.rel[i] = tab.rel[i];
  for (int i = lane; i < MAXGG / 4; i += 64) s.claim[le][i] = 0u;
  if (lane == 0) { s.rst[le] = (live && a.is_reset) ? 1 : 0; s.term[le] = 0; s.rew[le] = 0.0f; s.sc[le] = 0; }
  int act = 0;
  if (live && !a.is_reset) {
    for (int i = lane; i < GG; i += 64) {
      const unsigned v = a.grid[(long)e * GG + i];
      s.grid[le][i] = (uint8_t)(v <= 3u * (unsigned)A ? v : 0u);
    }
    if (agent) {
      const int hr = min(max(a.head[2 * ka], 0), G - 1), hcol = min(max(a.head[2 * ka + 1], 0), G - 1);
      const int tr = min(max(a.target[2 * ka], 0), G - 1), tcol = min(max(a.target[2 * ka + 1], 0), G - 1);
      s.hc[le][lane] = (uint8_t)(hr * G + hcol);
      s.tc[le][lane] = (uint8_t)(tr * G + tcol);
      s.conn[le][lane] = a.connected[ka] ? 1 : 0;
      act = a.action[ka];
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- rule phase: one lane per agent
  const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);
  int dst = -1;
  bool was_open = false;
  if (agent && !a.is_reset) {
    const int cell = s.hc[le][lane], r = (unsigned)cell / (unsigned)G, c = cell - r * G;
    was_open = !s.conn[le][lane];
    // 1. wants to move: not connected, a move, onto the grid, into an empty cell or its own target
    if (was_open && act >= 1 && act <= 4) {
      const int d = dest_of(r, c, act, G);
      if (can_enter(s.grid[le], d, lane)) {
        dst = d;
        atomicAdd(&s.claim[le][d >> 2], 1u << (8 * (d & 3)));
      }
    }
  }
  __syncthreads();
  bool connects = false;
  if (dst >= 0 && ((s.claim[le][dst >> 2] >> (8 * (dst & 3))) & 0xFFu) == 1u) {
    // 2./3. the only mover into this cell: leave a path, take the cell; a head on its own target is stored as head
    s.grid[le][s.hc[le][lane]] = (uint8_t)(1 + 3 * lane);
    s.grid[le][dst] = (uint8_t)(2 + 3 * lane);
    s.hc[le][lane] = (uint8_t)dst;
    connects = dst == s.tc[le][lane];
    if (connects) s.conn[le][lane] = 1;
  }
  // 4./5. the counts of the team reward (wave ballots: this wave is the environment)
  const int n_conn = __popcll(__ballot(connects)), n_open = __popcll(__ballot(was_open));
  __syncthreads();
  if (!a.is_reset) {
    // 6. the mask of the new state; 7. nobody can move: terminated
    const bool any = agent ? build_mask(s, le, lane, G) : false;
    const bool terminated = __ballot(any) == 0ull;
    if (live && lane == 0) {
      // (100 c - 3 o) / 100: both operands exact, one correctly rounded division
      const float rew = __fdiv_rn((float)(100 * n_conn - 3 * n_open), 100.0f);
      if constexpr (REAL) rn.terminated[e] = terminated ? 1 : 0;
      const EpisodeEnd end = episode_step(episode_book(a), e, a.step_count[(long)e * A], rew, terminated, a.time_limit);
      s.rew[le] = rew;
      s.term[le] = end.term ? 1 : 0;
      s.rst[le] = end.term ? 1 : 0;
      s.sc[le] = end.step_count;
    }
  } else if (live && lane == 0) {
    episode_clear(episode_book(a), e);
  }
  __syncthreads();
  if constexpr (REAL) {
    // the pre-reset observation of every env (equal to the returned one where the step did not end)
    if (!a.is_reset) {
      write_obs(a, s, rn.view, nullptr, rn.mask, e0, ne, tid);
      __syncthreads();
    }
  }

  // ---------------------------------------------------------------- (auto-)reset at this step's counter
  const bool rst = s.rst[le] != 0;  // wave-uniform
  if (rst) {
    for (int i = lane; i < GG; i += 64) s.grid[le][i] = 0;
    if (lane < MAXG) s.occ[le][lane] = 0;
  }
  __syncthreads();
  if (rst && lane == 0) generate(a, s, le, a.env_offset + (uint32_t)e, t);
  __syncthreads();
  if (rst)  // the cells between head and target are cleared
    for (int i = lane; i < GG; i += 64) {
      const unsigned v = s.grid[le][i];
      if (v != 0u && (v - 1u) % 3u == 0u) s.grid[le][i] = 0;
    }
  __syncthreads();
  if (rst && agent) build_mask(s, le, lane, G);
  __syncthreads();

  // ---------------------------------------------------------------- output phase (all threads)
  write_obs(a, s, a.agents_view, a.global_state, a.action_mask, e0, ne, tid);
  // the advanced state
  if (live) {
    for (int i = lane; i < GG; i += 64) a.grid[(long)e * GG + i] = s.grid[le][i];
    if (agent) {
      const int h = s.hc[le][lane], tg = s.tc[le][lane];
      const int hr = (unsigned)h / (unsigned)G, tr = (unsigned)tg / (unsigned)G;
      a.head[2 * ka] = hr;
      a.head[2 * ka + 1] = h - hr * G;
      a.target[2 * ka] = tr;
      a.target[2 * ka + 1] = tg - tr * G;
      a.connected[ka] = s.conn[le][lane];
      a.step_count[ka] = s.sc[le];
      a.obs_step_count[ka] = s.sc[le];
      if (!a.is_reset) {
        a.reward[ka] = s.rew[le];
        a.done[ka] = (uint8_t)s.term[le];
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void connector_step_kernel(ConArgs a, ConTable tab) {
  connector_step_body<false>(a, tab, ConReal{});
}

__global__ __launch_bounds__(THREADS) void connector_step_real_kernel(ConArgs a, ConTable tab, ConReal rn) {
  connector_step_body<true>(a, tab, rn);
}

}  // namespace

extern "C" int mava_connector_step(int E, int A, int G, int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base,
                                   uint32_t env_offset, int is_reset, int32_t* head, int32_t* target, uint8_t* connected,
                                   uint8_t* grid, int32_t* step_count, float* run_return, int32_t* run_length,
                                   float* ep_return, int32_t* ep_length, float* agents_view, float* global_state,
                                   uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                                   float* info_return, int32_t* info_length, uint8_t* info_terminal, const int32_t* action,
                                   float* real_view, uint8_t* real_mask, uint8_t* terminated, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && A <= MAXA && G >= 3 && G <= MAXG, 0,
                 "mava_connector_step: bad shape E=%d A=%d G=%d (1 <= A <= %d, 3 <= G <= %d)", E, A, G, MAXA, MAXG);
  MAVA_ARG_CHECK(2 * A <= G * G - 2 && time_limit >= 1, 1,
                 "mava_connector_step: bad scenario num_agents=%d grid_size=%d time_limit=%d (2 A <= G G - 2, time_limit >= 1)", A, G,
                 time_limit);
  MAVA_ARG_CHECK((long)E * A * G * G * NCH < (1L << 31), 3, "mava_connector_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(head && target && connected && grid && step_count && run_return && run_length && ep_return && ep_length &&
                     agents_view && global_state && action_mask && obs_step_count,
                 4, "mava_connector_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_connector_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_connector_step: a step needs the (E, A) action array");
  ConArgs a;
  a.E = E; a.A = A; a.G = G; a.time_limit = time_limit;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.head = head; a.target = target; a.connected = connected; a.grid = grid; a.step_count = step_count;
  a.run_return = run_return; a.run_length = run_length; a.ep_return = ep_return; a.ep_length = ep_length;
  a.agents_view = agents_view; a.global_state = global_state; a.action_mask = action_mask;
  a.obs_step_count = obs_step_count; a.reward = reward; a.done = done; a.info_return = info_return;
  a.info_length = info_length; a.info_terminal = info_terminal; a.action = action;
  ConTable tab;
  for (int i = 0; i <= MAXA; ++i) tab.rel[i] = i <= A ? (float)i / (float)A : 0.0f;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 0 || n_real == 3, 7,
                 "mava_connector_step: real_view, real_mask and terminated go together (all three or none)");
  if (n_real == 0) {
    hipLaunchKernelGGL(connector_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, tab);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask), 8,
                   "mava_connector_step: real_view / real_mask must not alias agents_view / action_mask");
    const ConReal rn = {real_view, real_mask, terminated};
    hipLaunchKernelGGL(connector_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, tab, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
