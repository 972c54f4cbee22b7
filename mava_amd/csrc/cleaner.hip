// Cleaner environment step (DESIGN.md "Cleaner"; the rules are the contract of mava_cleaner_step in include/mava_hip.h
// and are stated in NumPy in tests/cleaner_model.py).  An R x C maze of dirty (0), clean (1) and wall (2) cells, A agents
// that may share cells; a move onto a dirty cell cleans it, the team earns (cells cleaned) - 0.5 per step, and the episode
// ends when nothing is dirty (won), when some agent moves into a wall or off the board, or at the time limit.  Wrapper
// semantics of the reference's CleanerWrapper: image observations (R, C, 4) per agent WITHOUT a prepended agent id,
// global_state = the first three channels (the same for every agent), AutoResetWrapper and RecordEpisodeMetrics
// bookkeeping (env_common.h), plus the won flag the evaluator turns into a win rate.
//
// The rules are small and the output is large (clean-30x30x30a: 432 KB of observation per env and step), so the kernel
// is shaped by its stores.  A workgroup of THREADS = 64 NE threads owns NE environments:
//   state load    - wave w copies environment w's board into LDS as bytes and clears its per-cell agent-count table; lane
//                   k < A holds agent k.  Every loaded value is clamped to its range: a corrupt state cannot index
//                   outside a table;
//   rule phase    - one lane per agent.  A valid mover takes its destination; every agent adds 1 to the count byte of
//                   its cell (32-bit LDS atomics on the containing word: A <= 32 fits a byte) and ORs 1 into the board
//                   byte of its cell, which turns dirty into clean and leaves clean as it is; the lane that read 0 back
//                   was the first arrival, so a ballot of those lanes counts cleaned CELLS, not agents.  A second ballot
//                   says whether any action was invalid, a third whether dirt is left;
//   reset         - the maze is the minimum spanning tree of the room graph under the weight (Philox draw, edge id).  The
//                   wave draws the keys, ranks them by counting (every lane counts the keys below its own edges: a sort
//                   without data-dependent control flow), then walks the sorted edges once: component labels live in
//                   registers, four rooms per lane, an edge whose ends carry different labels is opened and one label
//                   is rewritten by all lanes.  Kruskal's tree, so the board equals the model's bit for bit;
//   output phase  - all threads.  The agents_view rows of a workgroup's environments are one contiguous run of 16-byte
//                   cells; thread i writes cell i, i + THREADS, ... as one float4 decoded from two LDS bytes (cell value,
//                   agent count) and the own-cell test.  Four consecutive lanes read one LDS word (a broadcast, no bank
//                   conflict).  Only when the slot base is not 16-byte aligned, and for the 3-channel global_state, a
//                   span is written as scalar head + aligned float4 body + scalar tail.  Divisions are multiplications
//                   by host-computed reciprocals with one correction step (exact below 2^24).
// Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays from a captured
// graph.  The REAL instantiation of the same body (real_view given) also writes the pre-reset agents_view /
// action_mask and the `terminated` flag (won or invalid; a time-limit end alone is a truncation).
#include "env_common.h"

namespace {

constexpr uint32_t CLN_RESET = 0x434C4E52u;  // "CLNR"
constexpr int MAXS = 32, MAXA = 32, MAXRC = MAXS * MAXS;
constexpr int MAXROOM = (MAXS / 2) * (MAXS / 2), MAXID = 2 * MAXROOM;  // rooms, edge ids (two per room)
constexpr int NE = 4;             // environments per workgroup, one wave each in the rule phase
constexpr int THREADS = 64 * NE;
constexpr int N_ACT = 4;          // UP RIGHT DOWN LEFT
constexpr int NCH = 4, NGS = 3;   // channels of agents_view / global_state
constexpr int DIRTY = 0, WALL = 2;

struct ClnArgs {
  int E, A, R, C, time_limit;
  float inv_c, inv_rc, inv_a, inv_nc;  // reciprocals for quot()
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  int32_t* pos;              // (E, A, 2) (row, col)
  uint8_t* grid;             // (E, R, C)
  int32_t* step_count;       // (E, A)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, A, R C 4)
  float* global_state;       // (E, 1, R C 3)
  uint8_t* action_mask;      // (E, A, 4)
  int32_t* obs_step_count;   // (E, A)
  float* reward;             // (E, A) or null (reset)
  uint8_t* done;
  float* info_return;
  int32_t* info_length;
  uint8_t* info_terminal;
  uint8_t* info_won;         // (E) or null
  const int32_t* action;     // (E, A) or null (reset)
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct ClnReal {
  float* view;               // (E, A, R C 4) pre-reset agents_view
  uint8_t* mask;             // (E, A, 4) pre-reset action_mask
  uint8_t* terminated;       // (E)
};

struct Tile {
  uint32_t grid[NE][MAXRC / 4];   // one byte per cell
  uint32_t count[NE][MAXRC / 4];  // agents in the cell, one byte per cell
  uint64_t wkey[NE][MAXID];       // the generator's edge weights (draw << 32 | id), all ones where no edge exists
  uint16_t sorted[NE][MAXID];     // edge ids by rising weight
  uint16_t pc[NE][MAXA];          // agent cell (row * C + col)
  uint8_t mask[NE][MAXA * N_ACT];
  int sc[NE], term[NE], rst[NE];
  float rew[NE];
};

// i / d for 0 <= i < 2^24 and 1 <= d <= 1024, inv = 1.0f / d: the float product is off by at most one
__device__ __forceinline__ int quot(int i, int d, float inv) {
  int q = (int)((float)i * inv);
  const int r = i - q * d;
  q += (r >= d) - (r < 0);
  return q;
}

__device__ __forceinline__ unsigned byte_of(const uint32_t* words, int i) { return (words[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// the cell a move takes (r, c) to, or -1 off the board (or for a value that is no action)
__device__ __forceinline__ int dest_of(int r, int c, int m, int R, int C) {
  if (m < 0 || m >= N_ACT) return -1;
  const int nr = r + (m == 2) - (m == 0), nc = c + (m == 1) - (m == 3);
  return (nr < 0 || nr >= R || nc < 0 || nc >= C) ? -1 : nr * C + nc;
}

// rule 1's test on a destination: on the board and not a wall
__device__ __forceinline__ bool can_enter(const uint32_t* grid, int d) { return d >= 0 && byte_of(grid, d) != (unsigned)WALL; }

// lane k < A: the action mask of agent k on the board in LDS.  Every agent always has a legal move: the open cells are a
// connected tree of at least two cells (3 <= R, C gives at least four rooms), so each open cell has an open neighbour.
__device__ __forceinline__ void build_mask(Tile& s, const ClnArgs& a, int le, int k) {
  const int cell = s.pc[le][k], r = quot(cell, a.C, a.inv_c), c = cell - r * a.C;
#pragma unroll
  for (int m = 0; m < N_ACT; ++m) s.mask[le][k * N_ACT + m] = can_enter(s.grid[le], dest_of(r, c, m, a.R, a.C)) ? 1 : 0;
}

// one observation value: channel ch of cell `cell` of environment le as agent j sees it
__device__ __forceinline__ float channel(const Tile& s, int le, int j, int cell, int ch) {
  if (ch == 2) return (float)byte_of(s.count[le], cell);
  if (ch == 3) return cell == (int)s.pc[le][j] ? 1.0f : 0.0f;
  return byte_of(s.grid[le], cell) == (unsigned)(ch == 0 ? DIRTY : WALL) ? 1.0f : 0.0f;
}

// all threads write n consecutive floats at `o`, value(q) being float q: up to three scalar stores reach 16-byte
// alignment, the body is aligned float4 stores of four consecutive floats per thread, up to three scalar stores finish.
template <class F>
__device__ __forceinline__ void write_span(float* o, int n, int tid, F value) {
  const int lead = min((int)((4u - (unsigned)(((uintptr_t)o >> 2) & 3u)) & 3u), n);
  const int nvec = (n - lead) >> 2, tail0 = lead + 4 * nvec;
  for (int i = tid; i < nvec; i += THREADS) {
    const int q0 = lead + 4 * i;
    *reinterpret_cast<float4*>(o + q0) = make_float4(value(q0), value(q0 + 1), value(q0 + 2), value(q0 + 3));
  }
  if (tid < lead) o[tid] = value(tid);
  if (tid >= 64 && tid - 64 < n - tail0) o[tail0 + tid - 64] = value(tail0 + tid - 64);
}

// all threads: the agents_view rows (and, when gs is not null, the global_state rows) and masks of the workgroup
__device__ __forceinline__ void write_obs(const ClnArgs& a, const Tile& s, float* av, float* gs, uint8_t* mk, int e0, int ne,
                                          int tid) {
  const int A = a.A, RC = a.R * a.C;
  const int ncell = ne * A * RC;  // <= 4 * 32 * 1024 = 2^17
  float* o = av + (long)e0 * A * RC * NCH;
  if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0u) {
    float4* o4 = reinterpret_cast<float4*>(o);
#pragma unroll 2
    for (int i = tid; i < ncell; i += THREADS) {
      const int row = quot(i, RC, a.inv_rc), cell = i - row * RC;
      const int le = quot(row, A, a.inv_a), j = row - le * A;
      const unsigned v = byte_of(s.grid[le], cell);
      o4[i] = make_float4(v == (unsigned)DIRTY ? 1.0f : 0.0f, v == (unsigned)WALL ? 1.0f : 0.0f,
                          (float)byte_of(s.count[le], cell), cell == (int)s.pc[le][j] ? 1.0f : 0.0f);
    }
  } else {
    write_span(o, ncell * NCH, tid, [&](int q) -> float {
      const int i = q >> 2, row = quot(i, RC, a.inv_rc), le = quot(row, A, a.inv_a);
      return channel(s, le, row - le * A, i - row * RC, q & 3);
    });
  }
  if (gs != nullptr)
    write_span(gs + (long)e0 * RC * NGS, ne * RC * NGS, tid, [&](int q) -> float {
      const int i = (unsigned)q / (unsigned)NGS, le = quot(i, RC, a.inv_rc);
      return channel(s, le, 0, i - le * RC, q - i * NGS);
    });
  const int nm = A * N_ACT;
  for (int i = tid; i < ne * nm; i += THREADS) {
    const int le = quot(i >> 2, A, a.inv_a);
    mk[(long)e0 * nm + i] = s.mask[le][i - le * nm];
  }
}

template <bool REAL>
__device__ __forceinline__ void cleaner_step_body(const ClnArgs& a, const ClnReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x, lane = tid & 63, le = tid >> 6;  // wave le owns environment e0 + le
  const int A = a.A, R = a.R, C = a.C, RC = R * C;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);
  if (ne <= 0) return;
  const bool live = le < ne;            // wave-uniform
  const bool agent = live && lane < A;  // lane k holds agent k
  const int e = e0 + le;
  const long ka = (long)e * A + lane;
  uint8_t* gb = reinterpret_cast<uint8_t*>(s.grid[le]);

  // ---------------------------------------------------------------- state load
  for (int i = lane; i < MAXRC / 4; i += 64) s.count[le][i] = 0u;
  if (lane == 0) { s.rst[le] = (live && a.is_reset) ? 1 : 0; s.term[le] = 0; s.rew[le] = 0.0f; s.sc[le] = 0; }
  if (lane < MAXA) s.pc[le][lane] = 0;
  int act = -1;
  if (live && !a.is_reset) {
    for (int i = lane; i < RC; i += 64) {
      const unsigned v = a.grid[(long)e * RC + i];
      gb[i] = (uint8_t)(v <= (unsigned)WALL ? v : (unsigned)WALL);
    }
    if (agent) {
      const int r = min(max(a.pos[2 * ka], 0), R - 1), c = min(max(a.pos[2 * ka + 1], 0), C - 1);
      s.pc[le][lane] = (uint16_t)(r * C + c);
      act = a.action[ka];
    }
  } else {
    for (int i = lane; i < RC; i += 64) gb[i] = (uint8_t)WALL;
  }
  __syncthreads();

  // ---------------------------------------------------------------- rule phase: one lane per agent
  const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);
  const bool stepping = agent && !a.is_reset;
  bool inval = false;
  int cell = 0;
  if (stepping) {
    // 1. a valid agent moves, an invalid one stays
    const int cur = s.pc[le][lane], r = quot(cur, C, a.inv_c), c = cur - r * C;
    const int d = dest_of(r, c, act, R, C);
    inval = !can_enter(s.grid[le], d);
    cell = inval ? cur : d;
    s.pc[le][lane] = (uint16_t)cell;
    atomicAdd(&s.count[le][cell >> 2], 1u << (8 * (cell & 3)));
  }
  __syncthreads();
  // 2. dirty | 1 = clean, clean | 1 = clean: the lane that reads dirty back is the cell's first arrival
  bool first = false;
  if (stepping && byte_of(s.grid[le], cell) != (unsigned)WALL) {
    const uint32_t old = atomicOr(&s.grid[le][cell >> 2], 1u << (8 * (cell & 3)));
    first = ((old >> (8 * (cell & 3))) & 0xFFu) == (unsigned)DIRTY;
  }
  const int n_clean = __popcll(__ballot(first));
  const bool any_inval = __ballot(inval) != 0ull;
  __syncthreads();
  bool dirty = false;
  if (live)
    for (int i = lane; i < RC; i += 64) dirty |= gb[i] == (uint8_t)DIRTY;
  const bool won = __ballot(dirty) == 0ull;
  if (!a.is_reset) {
    if (agent) build_mask(s, a, le, lane);  // the mask of the new board
    if (live && lane == 0) {
      const float rew = (float)n_clean - 0.5f;  // 3. exact in f32
      const bool terminated = won || any_inval;
      if constexpr (REAL) rn.terminated[e] = terminated ? 1 : 0;
      const EpisodeEnd end = episode_step(episode_book(a), e, a.step_count[(long)e * A], rew, terminated, a.time_limit);
      if (a.info_won != nullptr) a.info_won[e] = (end.term && won) ? 1 : 0;
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
  const int nrm = (R + 1) >> 1, ncm = (C + 1) >> 1, nroom = nrm * ncm, nid = 2 * nroom;
  if (rst) {
    // rooms (even row, even column) are dirty, everything else starts as a wall; nobody stands anywhere yet
    for (int i = lane; i < RC; i += 64) {
      const int r = quot(i, C, a.inv_c), c = i - r * C;
      gb[i] = (uint8_t)(((r | c) & 1) ? WALL : DIRTY);
    }
    for (int i = lane; i < MAXRC / 4; i += 64) s.count[le][i] = 0u;
    // draw n (the key of edge id n) is word n % 4 of Philox block n / 4
    const uint32_t g = a.env_offset + (uint32_t)e;
    for (int b = lane; 4 * b < nid; b += 64) {
      const Philox4 p = philox4x32_10(g, t, (uint32_t)b, CLN_RESET, a.seed_lo, a.seed_hi);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = 4 * b + u;
        if (n < nid) {
          const int q = n >> 1, i = quot(q, ncm, a.inv_nc), j = q - i * ncm;
          const bool exists = (n & 1) ? (i + 1 < nrm) : (j + 1 < ncm);  // to the room below / to the right
          s.wkey[le][n] = exists ? (((uint64_t)word_of(p, u) << 32) | (uint64_t)n) : ~0ull;
        }
      }
    }
  }
  __syncthreads();
  if (rst) {
    // rank by counting: the position of an edge in the sorted order is the number of lighter edges
    constexpr int PER = MAXID / 64;
    const int nu = (nid + 63) >> 6;
    uint64_t my[PER];
    int rank[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int n = lane + 64 * u;
      my[u] = n < nid ? s.wkey[le][n] : ~0ull;
      rank[u] = 0;
    }
    for (int m = 0; m < nid; ++m) {
      const uint64_t w = s.wkey[le][m];
#pragma unroll
      for (int u = 0; u < PER; ++u)
        if (u < nu) rank[u] += w < my[u] ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u)
      if (my[u] != ~0ull) s.sorted[le][rank[u]] = (uint16_t)(lane + 64 * u);
  }
  __syncthreads();
  if (rst) {
    // Kruskal over the sorted edges; lane l holds the component labels of rooms l, l + 64, l + 128, l + 192
    constexpr int PER = MAXROOM / 64;
    int lbl[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) lbl[u] = lane + 64 * u;
    // the label of a (wave-uniform) room: read its lane of all four registers, then choose among the four scalars
    auto label_of = [&](int room) -> int {
      const int l = __builtin_amdgcn_readfirstlane(room & 63), u = __builtin_amdgcn_readfirstlane(room >> 6);
      int x = __builtin_amdgcn_readlane(lbl[0], l);
#pragma unroll
      for (int k = 1; k < PER; ++k) {
        const int y = __builtin_amdgcn_readlane(lbl[k], l);
        x = u == k ? y : x;
      }
      return x;
    };
    const int n_edges = nrm * (ncm - 1) + (nrm - 1) * ncm;
    int need = nroom - 1;
    for (int k = 0; k < n_edges && need > 0; ++k) {
      const int id = __builtin_amdgcn_readfirstlane((int)s.sorted[le][k]);
      const int q = min(id >> 1, nroom - 1), q2 = min((id & 1) ? q + ncm : q + 1, nroom - 1);
      const int lu = label_of(q), lv = label_of(q2);
      if (lu != lv) {
#pragma unroll
        for (int u = 0; u < PER; ++u) lbl[u] = lbl[u] == lv ? lu : lbl[u];
        --need;
        if (lane == 0) {
          const int i = quot(q, ncm, a.inv_nc), j = q - i * ncm;
          const int open = (id & 1) ? (2 * i + 1) * C + 2 * j : 2 * i * C + 2 * j + 1;
          gb[min(open, RC - 1)] = (uint8_t)DIRTY;
        }
      }
    }
    // all agents start at (0, 0), which is cleaned at once (s.pc is rewritten below, after the barrier)
    if (lane == 0) {
      s.count[le][0] = (uint32_t)A;
      s.sc[le] = 0;
    }
  }
  __syncthreads();
  if (rst) {
    if (lane == 0) gb[0] = 1;
    if (lane < MAXA) s.pc[le][lane] = 0;
  }
  __syncthreads();
  if (rst && agent) build_mask(s, a, le, lane);
  __syncthreads();

  // ---------------------------------------------------------------- output phase (all threads)
  write_obs(a, s, a.agents_view, a.global_state, a.action_mask, e0, ne, tid);
  // the advanced state
  if (live) {
    for (int i = lane; i < RC; i += 64) a.grid[(long)e * RC + i] = gb[i];
    if (agent) {
      const int p = s.pc[le][lane], r = quot(p, C, a.inv_c);
      a.pos[2 * ka] = r;
      a.pos[2 * ka + 1] = p - r * C;
      a.step_count[ka] = s.sc[le];
      a.obs_step_count[ka] = s.sc[le];
      if (!a.is_reset) {
        a.reward[ka] = s.rew[le];
        a.done[ka] = (uint8_t)s.term[le];
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void cleaner_step_kernel(ClnArgs a) { cleaner_step_body<false>(a, ClnReal{}); }

__global__ __launch_bounds__(THREADS) void cleaner_step_real_kernel(ClnArgs a, ClnReal rn) { cleaner_step_body<true>(a, rn); }

}  // namespace

extern "C" int mava_cleaner_step(int E, int A, int R, int C, int time_limit, uint64_t seed, uint32_t t,
                                 const uint32_t* t_base, uint32_t env_offset, int is_reset, int32_t* pos, uint8_t* grid,
                                 int32_t* step_count, float* run_return, int32_t* run_length, float* ep_return,
                                 int32_t* ep_length, float* agents_view, float* global_state, uint8_t* action_mask,
                                 int32_t* obs_step_count, float* reward, uint8_t* done, float* info_return,
                                 int32_t* info_length, uint8_t* info_terminal, uint8_t* info_won, const int32_t* action,
                                 float* real_view, uint8_t* real_mask, uint8_t* terminated, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && A <= MAXA && R >= 3 && R <= MAXS && C >= 3 && C <= MAXS, 0,
                 "mava_cleaner_step: bad shape E=%d A=%d R=%d C=%d (1 <= A <= %d, 3 <= R, C <= %d)", E, A, R, C, MAXA, MAXS);
  MAVA_ARG_CHECK(time_limit >= 1, 1, "mava_cleaner_step: bad scenario time_limit=%d (time_limit >= 1)", time_limit);
  MAVA_ARG_CHECK((long)E * A * R * C * NCH < (1L << 31), 3, "mava_cleaner_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(pos && grid && step_count && run_return && run_length && ep_return && ep_length && agents_view &&
                     global_state && action_mask && obs_step_count,
                 4, "mava_cleaner_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_cleaner_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_cleaner_step: a step needs the (E, A) action array");
  ClnArgs a;
  a.E = E; a.A = A; a.R = R; a.C = C; a.time_limit = time_limit;
  a.inv_c = 1.0f / (float)C; a.inv_rc = 1.0f / (float)(R * C); a.inv_a = 1.0f / (float)A;
  a.inv_nc = 1.0f / (float)((C + 1) / 2);
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.pos = pos; a.grid = grid; a.step_count = step_count;
  a.run_return = run_return; a.run_length = run_length; a.ep_return = ep_return; a.ep_length = ep_length;
  a.agents_view = agents_view; a.global_state = global_state; a.action_mask = action_mask;
  a.obs_step_count = obs_step_count; a.reward = reward; a.done = done; a.info_return = info_return;
  a.info_length = info_length; a.info_terminal = info_terminal; a.info_won = is_reset ? nullptr : info_won;
  a.action = action;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 0 || n_real == 3, 7,
                 "mava_cleaner_step: real_view, real_mask and terminated go together (all three or none)");
  if (n_real == 0) {
    hipLaunchKernelGGL(cleaner_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask), 8,
                   "mava_cleaner_step: real_view / real_mask must not alias agents_view / action_mask");
    const ClnReal rn = {real_view, real_mask, terminated};
    hipLaunchKernelGGL(cleaner_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
