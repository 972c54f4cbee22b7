// Level-Based Foraging environment step (DESIGN.md "Level-Based Foraging"; the rules are the contract of
// mava_lbf_step in include/mava_hip.h and are restated in NumPy in tests/lbf_model.py).  A G x G grid, A agents and
// F foods with levels; an agent moves (UP/DOWN/LEFT/RIGHT), waits (NOOP) or LOADs; a food is eaten when the LOADing
// agents 4-adjacent to it together reach its level, and its reward is split in proportion to their levels.
// Wrapper semantics as in synth_rware.hip: one-hot agent id prepended to agents_view, global_state = the concatenated
// raw views, team reward repeated per agent, AutoResetWrapper (a terminal step returns the reset observation with
// step_count 0) and RecordEpisodeMetrics bookkeeping.
//
// Shape of the kernel: a workgroup of 256 threads owns NE = 16 environments.
//   state load    - all 256 threads copy the workgroup's contiguous state ranges into LDS ([field][index][env]: lane e
//                   of every rule-phase access hits bank e);
//   rule phase    - thread e < NE runs environment e's rules on the LDS state, including the rare divergent reset
//                   (cells chosen by popcounts over 32-bit row masks, no grid array);
//   output phase  - all 256 threads write the workgroup's contiguous output ranges and the advanced state element by
//                   element from LDS (agents_view, global_state, action_mask, per-agent words), so every store
//                   instruction covers consecutive addresses instead of lanes a whole observation apart.
// Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays from a captured
// graph.
//
// The REAL instantiation (real_view given) also writes what AutoResetWrapper keeps in
// extras["real_next_obs"] (mava/wrappers/auto_reset_wrapper.py:52-101): the agents_view / action_mask of the state the
// rules produced, BEFORE the auto-reset, and a per-env `terminated` flag (every food eaten).  The reset of ending envs
// then moves behind one more output pass over the same LDS tile; the plain kernel is the same code with those parts
// compiled out.
#include "env_common.h"

namespace {

constexpr uint32_t LBF_STREAM = 0x4C424653u;  // "LBFS"
constexpr int MAXG = 32, MAXA = 16, MAXF = 16;
constexpr int NE = 16;        // environments per workgroup
constexpr int THREADS = 256;
constexpr int N_ACT = 6;      // NOOP UP DOWN LEFT RIGHT LOAD
constexpr int LOAD = 5;

struct LbfArgs {
  int E, A, F, G, fov, max_level, force_coop, individual, time_limit;
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  int32_t* agent_pos;        // (E, A, 2)
  int32_t* agent_level;      // (E, A)
  int32_t* food_pos;         // (E, F, 2)
  int32_t* food_level;       // (E, F)
  uint8_t* food_alive;       // (E, F)
  float* total_food_level;   // (E)
  int32_t* step_count;       // (E, A)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, A, A + 3 (F + A))
  float* global_state;       // (E, 1, A * 3 (F + A))
  uint8_t* action_mask;      // (E, A, 6)
  int32_t* obs_step_count;   // (E, A)
  float* reward;             // (E, A) or null (reset)
  uint8_t* done;             // (E, A) or null
  float* info_return;        // (E) or null
  int32_t* info_length;
  uint8_t* info_terminal;
  const int32_t* action;     // (E, A) or null (reset)
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct LbfReal {
  float* view;               // (E, A, A + 3 (F + A)) pre-reset agents_view
  uint8_t* mask;             // (E, A, 6) pre-reset action_mask
  uint8_t* terminated;       // (E) 1 when every food was eaten (a time-limit end is a truncation: 0)
};

struct Tile {
  int ar[MAXA][NE], ac[MAXA][NE], al[MAXA][NE], act[MAXA][NE], mv[MAXA][NE];
  int fr[MAXF][NE], fc[MAXF][NE], fl[MAXF][NE], fa[MAXF][NE];
  float rew[MAXA][NE];
  uint32_t occ[MAXG][NE];
  float team[NE];
  int sc[NE], term[NE];
};

__device__ __forceinline__ int cheb(int r0, int c0, int r1, int c1) { return max(abs(r0 - r1), abs(c0 - c1)); }

// cell number k (0-based, row-major) among the cells of rows [r0, r1) whose bit is set in (row_mask & ~occ[r])
__device__ int kth_free_cell(const Tile& s, int le, int r0, int r1, uint32_t row_mask, uint32_t k, int& row, int& col) {
  for (int r = r0; r < r1; ++r) {
    uint32_t m = row_mask & ~s.occ[r][le];
    const uint32_t n = __popc(m);
    if (k < n) {
      for (; k > 0; --k) m &= m - 1;  // drop the k lowest set bits
      row = r;
      col = __ffs(m) - 1;
      return 1;
    }
    k -= n;
  }
  return 0;
}

__device__ uint32_t free_cells(const Tile& s, int le, int r0, int r1, uint32_t row_mask) {
  uint32_t n = 0;
  for (int r = r0; r < r1; ++r) n += __popc(row_mask & ~s.occ[r][le]);
  return n;
}

// the reset rule: foods, agents, agent levels, food levels (draw k = word k % 4 of Philox block k / 4); returns the
// total food level
__device__ int generate(const LbfArgs& a, Tile& s, int le, uint32_t g, uint32_t t) {
  const int G = a.G;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  int nd = 0;
  auto draw = [&]() -> uint32_t {
    if ((nd & 3) == 0) {
      const Philox4 p = philox4x32_10(g, t, (uint32_t)(nd >> 2), LBF_STREAM, a.seed_lo, a.seed_hi);
      w[0] = p.x; w[1] = p.y; w[2] = p.z; w[3] = p.w;
    }
    return w[nd++ & 3];
  };
  const uint32_t full = G == 32 ? 0xFFFFFFFFu : ((1u << G) - 1u);
  const uint32_t inner = full & ~1u & ~(1u << (G - 1));  // columns 1 .. G-2
  // 1. foods: interior cells not within Chebyshev distance 1 of an earlier food (occ = blocked cells)
  for (int r = 0; r < G; ++r) s.occ[r][le] = 0u;
  for (int i = 0; i < a.F; ++i) {
    const uint32_t d = draw();
    const uint32_t n = free_cells(s, le, 1, G - 1, inner);  // >= 1: (G-2)^2 >= 9 (F-1) + 1 is checked on the host
    int r = 1, c = 1;
    kth_free_cell(s, le, 1, G - 1, inner, d % n, r, c);
    s.fr[i][le] = r;
    s.fc[i][le] = c;
    for (int rr = r - 1; rr <= r + 1; ++rr) s.occ[rr][le] |= 7u << (c - 1);
  }
  // 2. agents: any cell holding neither a food nor an earlier agent (occ = occupied cells)
  for (int r = 0; r < G; ++r) s.occ[r][le] = 0u;
  for (int i = 0; i < a.F; ++i) s.occ[s.fr[i][le]][le] |= 1u << s.fc[i][le];
  for (int j = 0; j < a.A; ++j) {
    const uint32_t d = draw();
    const uint32_t n = free_cells(s, le, 0, G, full);  // >= 1: G^2 >= F + A is checked on the host
    int r = 0, c = 0;
    kth_free_cell(s, le, 0, G, full, d % n, r, c);
    s.ar[j][le] = r;
    s.ac[j][le] = c;
    s.occ[r][le] |= 1u << c;
  }
  // 3. agent levels; 4. food levels (max_food = sum of the min(3, A) largest agent levels)
  int m1 = 0, m2 = 0, m3 = 0;
  for (int j = 0; j < a.A; ++j) {
    const int l = 1 + (int)(draw() % (uint32_t)a.max_level);
    s.al[j][le] = l;
    if (l > m1) { m3 = m2; m2 = m1; m1 = l; }
    else if (l > m2) { m3 = m2; m2 = l; }
    else if (l > m3) { m3 = l; }
  }
  const int max_food = m1 + m2 + m3;  // (levels >= 1: for A < 3 the missing terms are 0)
  int total = 0;
  for (int i = 0; i < a.F; ++i) {
    const uint32_t d = draw();
    const int l = a.force_coop ? max_food : 1 + (int)(d % (uint32_t)max_food);
    s.fl[i][le] = l;
    s.fa[i][le] = 1;
    total += l;
  }
  s.sc[le] = 0;
  return total;
}

__device__ __forceinline__ bool agent_at(const Tile& s, int le, int A, int r, int c) {
  bool hit = false;
  for (int k = 0; k < A; ++k) hit |= (s.ar[k][le] == r) & (s.ac[k][le] == c);
  return hit;
}

__device__ __forceinline__ bool food_at(const Tile& s, int le, int F, int r, int c) {
  bool hit = false;
  for (int f = 0; f < F; ++f) hit |= (s.fa[f][le] != 0) & (s.fr[f][le] == r) & (s.fc[f][le] == c);
  return hit;
}

// feature q of agent j's raw view: entity q / 3 (foods, then j itself, then the other agents in index order)
__device__ __forceinline__ float view_value(const Tile& s, int le, int j, int q, int F, int fov) {
  const int ent = q / 3, comp = q - 3 * ent;
  const int r0 = s.ar[j][le], c0 = s.ac[j][le];
  int r, c, l;
  bool vis;
  if (ent < F) {
    r = s.fr[ent][le]; c = s.fc[ent][le]; l = s.fl[ent][le];
    vis = s.fa[ent][le] != 0 && cheb(r0, c0, r, c) <= fov;
  } else {
    const int k = ent - F;
    const int src = k == 0 ? j : (k - 1 < j ? k - 1 : k);
    r = s.ar[src][le]; c = s.ac[src][le]; l = s.al[src][le];
    vis = cheb(r0, c0, r, c) <= fov;
  }
  const int v = comp == 0 ? r : (comp == 1 ? c : l);
  return vis ? (float)v : (comp < 2 ? -1.0f : 0.0f);
}

// agents_view / action_mask of the workgroup's rows [e0 * A, (e0 + ne) * A) from the LDS state (all threads, stores to
// consecutive addresses); av / mk point at row e0 * A
__device__ __forceinline__ void write_view(const LbfArgs& a, const Tile& s, float* av, int ne, int tid) {
  const int A = a.A, F = a.F;
  const int W = A + 3 * (F + A);
  const int n = ne * A * W;
  for (int i = tid; i < n; i += THREADS) {
    const int row = (unsigned)i / (unsigned)W, f = i - row * W;
    const int le = (unsigned)row / (unsigned)A, j = row - le * A;
    av[i] = f < A ? (f == j ? 1.0f : 0.0f) : view_value(s, le, j, f - A, F, a.fov);
  }
}

__device__ __forceinline__ void write_mask(const LbfArgs& a, const Tile& s, uint8_t* mk, int ne, int tid) {
  const int A = a.A, F = a.F, G = a.G;
  {
    const int n = ne * A * N_ACT;
    for (int i = tid; i < n; i += THREADS) {
      const int row = (unsigned)i / (unsigned)N_ACT, act = i - row * N_ACT;
      const int le = (unsigned)row / (unsigned)A, j = row - le * A;
      const int r = s.ar[j][le], c = s.ac[j][le];
      bool ok;
      if (act == 0) {
        ok = true;
      } else if (act == LOAD) {
        ok = false;
        for (int f = 0; f < F; ++f) ok |= (s.fa[f][le] != 0) & (abs(s.fr[f][le] - r) + abs(s.fc[f][le] - c) == 1);
      } else {
        const int tr = r + (act == 2) - (act == 1), tc = c + (act == 4) - (act == 3);
        ok = tr >= 0 && tr < G && tc >= 0 && tc < G && !food_at(s, le, F, tr, tc) && !agent_at(s, le, A, tr, tc);
      }
      mk[i] = ok ? 1 : 0;
    }
  }
}

template <bool REAL>
__device__ __forceinline__ void lbf_step_body(const LbfArgs& a, const LbfReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x;
  const int A = a.A, F = a.F, G = a.G;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);

  // ---------------------------------------------------------------- state load: the workgroup's contiguous ranges
  // (all threads, element by element, into the bank-conflict-free LDS layout the rule phase reads)
  if (!a.is_reset && ne > 0) {
    const long ka = (long)e0 * A, kf = (long)e0 * F;
    for (int i = tid; i < ne * A * 2; i += THREADS) {
      const int k = i >> 1, le = (unsigned)k / (unsigned)A, j = k - le * A;
      const int v = a.agent_pos[2 * ka + i];
      if (i & 1) s.ac[j][le] = v; else s.ar[j][le] = v;
    }
    for (int i = tid; i < ne * A; i += THREADS) {
      const int le = (unsigned)i / (unsigned)A, j = i - le * A;
      s.al[j][le] = a.agent_level[ka + i];
      s.act[j][le] = a.action[ka + i];
    }
    for (int i = tid; i < ne * F * 2; i += THREADS) {
      const int k = i >> 1, le = (unsigned)k / (unsigned)F, f = k - le * F;
      const int v = a.food_pos[2 * kf + i];
      if (i & 1) s.fc[f][le] = v; else s.fr[f][le] = v;
    }
    for (int i = tid; i < ne * F; i += THREADS) {
      const int le = (unsigned)i / (unsigned)F, f = i - le * F;
      s.fl[f][le] = a.food_level[kf + i];
      s.fa[f][le] = a.food_alive[kf + i];
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- rule phase: one thread per environment
  if (tid < ne) {
    const int le = tid, e = e0 + tid;
    const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);
    const uint32_t g = a.env_offset + (uint32_t)e;
    const EpisodeBook bk = episode_book(a);
    bool reset = a.is_reset != 0;
    float total = 0.0f;
    if (!a.is_reset) {
      total = a.total_food_level[e];
      const int sc_old = a.step_count[(long)e * A];
      const EpisodeRun run = episode_load(bk, e);  // used at the end of the rule phase
      // 1. targets: cancelled outside the grid, onto an alive food, onto any agent's cell at the start of the step
      for (int j = 0; j < A; ++j) {
        const int ac = s.act[j][le];
        const int r = s.ar[j][le] + (ac == 2) - (ac == 1);
        const int c = s.ac[j][le] + (ac == 4) - (ac == 3);
        const bool ok = ac >= 1 && ac <= 4 && r >= 0 && r < G && c >= 0 && c < G && !food_at(s, le, F, r, c) &&
                        !agent_at(s, le, A, r, c);
        s.mv[j][le] = ok ? r * G + c : -1;
      }
      // 2. + 3. a target shared by two or more surviving moves cancels all of them; the others are applied
      for (int j = 0; j < A; ++j) {
        const int m = s.mv[j][le];
        if (m < 0) continue;
        int same = 0;
        for (int k = 0; k < A; ++k) same += s.mv[k][le] == m;
        if (same == 1) {
          s.ar[j][le] = m / G;
          s.ac[j][le] = m - (m / G) * G;
        }
      }
      // 4. loading, foods in index order; reward (level_f * level_j) / (sum of loaders' levels * total food level)
      for (int j = 0; j < A; ++j) s.rew[j][le] = 0.0f;
      int left = 0;
      for (int f = 0; f < F; ++f) {
        if (!s.fa[f][le]) continue;
        const int fr = s.fr[f][le], fc = s.fc[f][le], fl = s.fl[f][le];
        int sum = 0;
        for (int j = 0; j < A; ++j) {
          const bool adj = s.act[j][le] == LOAD && abs(s.ar[j][le] - fr) + abs(s.ac[j][le] - fc) == 1;
          sum += adj ? s.al[j][le] : 0;
        }
        if (sum >= fl) {
          s.fa[f][le] = 0;
          const float den = (float)sum * total;
          for (int j = 0; j < A; ++j) {
            const bool adj = s.act[j][le] == LOAD && abs(s.ar[j][le] - fr) + abs(s.ac[j][le] - fc) == 1;
            if (adj) s.rew[j][le] = s.rew[j][le] + (float)(fl * s.al[j][le]) / den;
          }
        } else {
          ++left;
        }
      }
      // 5. team reward: the agents' rewards summed in index order
      float team = s.rew[0][le];
      for (int j = 1; j < A; ++j) team = team + s.rew[j][le];
      s.team[le] = team;
      const float mean_rew = a.individual ? team / (float)A : team;
      // 6. terminal, RecordEpisodeMetrics
      if constexpr (REAL) rn.terminated[e] = left == 0 ? 1 : 0;  // Jumanji: termination vs truncation
      const EpisodeEnd end = episode_commit(bk, e, run, sc_old, mean_rew, left == 0, a.time_limit);
      s.term[le] = end.term ? 1 : 0;
      s.sc[le] = end.step_count;
      reset = end.term;
    } else {
      episode_clear(bk, e);
      s.term[le] = 0;
    }
    // 7. (auto-)reset at this step's counter
    if constexpr (!REAL) {  // (REAL: after the pre-reset output pass below)
      if (reset) total = (float)generate(a, s, le, g, t);
      a.total_food_level[e] = total;
    }
  }
  if constexpr (REAL) {
    // the pre-reset observation of every env (equal to the returned one where the step did not end), then the reset
    __syncthreads();
    if (!a.is_reset && ne > 0) {
      write_view(a, s, rn.view + (long)e0 * A * (A + 3 * (F + A)), ne, tid);
      write_mask(a, s, rn.mask + (long)e0 * A * N_ACT, ne, tid);
    }
    __syncthreads();
    if (tid < ne && (a.is_reset || s.term[tid])) {  // (a continuing env keeps its total food level)
      const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);
      a.total_food_level[e0 + tid] = (float)generate(a, s, tid, a.env_offset + (uint32_t)(e0 + tid), t);
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- output phase: the workgroup's contiguous ranges
  if (ne <= 0) return;
  const int R = 3 * (F + A), W = A + R;
  const int rows = ne * A;  // (env, agent) rows of this workgroup
  {
    float* av = a.agents_view + (long)e0 * A * W;
    const int n = rows * W;
    for (int i = tid; i < n; i += THREADS) {
      const int row = (unsigned)i / (unsigned)W, f = i - row * W;
      const int le = (unsigned)row / (unsigned)A, j = row - le * A;
      av[i] = f < A ? (f == j ? 1.0f : 0.0f) : view_value(s, le, j, f - A, F, a.fov);
    }
  }
  {
    float* gs = a.global_state + (long)e0 * A * R;
    const int n = rows * R;
    for (int i = tid; i < n; i += THREADS) {
      const int row = (unsigned)i / (unsigned)R, q = i - row * R;
      const int le = (unsigned)row / (unsigned)A, j = row - le * A;
      gs[i] = view_value(s, le, j, q, F, a.fov);
    }
  }
  {
    uint8_t* mk = a.action_mask + (long)e0 * A * N_ACT;
    const int n = rows * N_ACT;
    for (int i = tid; i < n; i += THREADS) {
      const int row = (unsigned)i / (unsigned)N_ACT, act = i - row * N_ACT;
      const int le = (unsigned)row / (unsigned)A, j = row - le * A;
      const int r = s.ar[j][le], c = s.ac[j][le];
      bool ok;
      if (act == 0) {
        ok = true;
      } else if (act == LOAD) {
        ok = false;
        for (int f = 0; f < F; ++f) ok |= (s.fa[f][le] != 0) & (abs(s.fr[f][le] - r) + abs(s.fc[f][le] - c) == 1);
      } else {
        const int tr = r + (act == 2) - (act == 1), tc = c + (act == 4) - (act == 3);
        ok = tr >= 0 && tr < G && tc >= 0 && tc < G && !food_at(s, le, F, tr, tc) && !agent_at(s, le, A, tr, tc);
      }
      mk[i] = ok ? 1 : 0;
    }
  }
  // the advanced state
  const long k0 = (long)e0 * A, kf = (long)e0 * F;
  for (int i = tid; i < rows * 2; i += THREADS) {
    const int k = i >> 1, le = (unsigned)k / (unsigned)A, j = k - le * A;
    a.agent_pos[2 * k0 + i] = (i & 1) ? s.ac[j][le] : s.ar[j][le];
  }
  for (int i = tid; i < ne * F * 2; i += THREADS) {
    const int k = i >> 1, le = (unsigned)k / (unsigned)F, f = k - le * F;
    a.food_pos[2 * kf + i] = (i & 1) ? s.fc[f][le] : s.fr[f][le];
  }
  for (int i = tid; i < ne * F; i += THREADS) {
    const int le = (unsigned)i / (unsigned)F, f = i - le * F;
    a.food_level[kf + i] = s.fl[f][le];
    a.food_alive[kf + i] = (uint8_t)s.fa[f][le];
  }
  for (int i = tid; i < rows; i += THREADS) {
    const int le = (unsigned)i / (unsigned)A, j = i - le * A;
    a.agent_level[k0 + i] = s.al[j][le];
    a.obs_step_count[k0 + i] = s.sc[le];
    a.step_count[k0 + i] = s.sc[le];
    if (!a.is_reset) {
      a.reward[k0 + i] = a.individual ? s.rew[j][le] : s.team[le];
      a.done[k0 + i] = (uint8_t)s.term[le];
    }
  }
}

__global__ __launch_bounds__(THREADS) void lbf_step_kernel(LbfArgs a) { lbf_step_body<false>(a, LbfReal{}); }

__global__ __launch_bounds__(THREADS) void lbf_step_real_kernel(LbfArgs a, LbfReal rn) { lbf_step_body<true>(a, rn); }

}  // namespace

extern "C" int mava_lbf_step(int E, int A, int F, int G, int fov, int max_agent_level, int force_coop,
                             int individual_rewards, int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base,
                             uint32_t env_offset, int is_reset, int32_t* agent_pos, int32_t* agent_level, int32_t* food_pos,
                             int32_t* food_level, uint8_t* food_alive, float* total_food_level, int32_t* step_count,
                             float* run_return, int32_t* run_length, float* ep_return, int32_t* ep_length,
                             float* agents_view, float* global_state, uint8_t* action_mask, int32_t* obs_step_count,
                             float* reward, uint8_t* done, float* info_return, int32_t* info_length, uint8_t* info_terminal,
                             const int32_t* action, float* real_view, uint8_t* real_mask, uint8_t* terminated,
                             hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && A <= MAXA && F >= 1 && F <= MAXF && G >= 3 && G <= MAXG, 0,
                 "mava_lbf_step: bad shape E=%d A=%d F=%d G=%d (1 <= A <= %d, 1 <= F <= %d, 3 <= G <= %d)", E, A, F, G,
                 MAXA, MAXF, MAXG);
  MAVA_ARG_CHECK(fov >= 0 && max_agent_level >= 1 && max_agent_level <= 1000 && time_limit >= 1 &&
                     (force_coop == 0 || force_coop == 1) && (individual_rewards == 0 || individual_rewards == 1),
                 1, "mava_lbf_step: bad scenario fov=%d max_agent_level=%d time_limit=%d force_coop=%d individual=%d",
                 fov, max_agent_level, time_limit, force_coop, individual_rewards);
  MAVA_ARG_CHECK((G - 2) * (G - 2) >= 9 * (F - 1) + 1 && G * G >= F + A, 2,
                 "mava_lbf_step: a %dx%d grid cannot place %d foods and %d agents", G, G, F, A);
  MAVA_ARG_CHECK((long)E * A * (A + 3 * (F + A)) < (1L << 31), 3, "mava_lbf_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(agent_pos && agent_level && food_pos && food_level && food_alive && total_food_level && step_count &&
                     run_return && run_length && ep_return && ep_length && agents_view && global_state && action_mask &&
                     obs_step_count,
                 4, "mava_lbf_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_lbf_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_lbf_step: a step needs the (E, A) action array");
  LbfArgs a;
  a.E = E; a.A = A; a.F = F; a.G = G; a.fov = fov; a.max_level = max_agent_level; a.force_coop = force_coop;
  a.individual = individual_rewards; a.time_limit = time_limit;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.agent_pos = agent_pos; a.agent_level = agent_level; a.food_pos = food_pos; a.food_level = food_level;
  a.food_alive = food_alive; a.total_food_level = total_food_level;
  a.step_count = step_count; a.run_return = run_return; a.run_length = run_length; a.ep_return = ep_return;
  a.ep_length = ep_length; a.agents_view = agents_view; a.global_state = global_state; a.action_mask = action_mask;
  a.obs_step_count = obs_step_count; a.reward = reward; a.done = done; a.info_return = info_return;
  a.info_length = info_length; a.info_terminal = info_terminal; a.action = action;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 0 || n_real == 3, 7,
                 "mava_lbf_step: real_view, real_mask and terminated go together (all three or none)");
  if (n_real == 0) {
    hipLaunchKernelGGL(lbf_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask), 8,
                   "mava_lbf_step: real_view / real_mask must not alias agents_view / action_mask");
    const LbfReal rn = {real_view, real_mask, terminated};
    hipLaunchKernelGGL(lbf_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
