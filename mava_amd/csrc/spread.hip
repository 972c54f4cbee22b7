// Spread environment step (DESIGN.md "Spread"; the rules are the contract of mava_spread_step in include/mava_hip.h and are
// stated in NumPy in tests/spread_model.py).  This project's own continuous-action task, modelled on MPE simple_spread:
// A agents and A landmarks in [-1, 1]^2; an action is a displacement (A, 2) f32, clamped to [-1, 1] and scaled by 0.1;
// the team is paid minus the mean over landmarks of the distance to the closest agent and fined 0.5 / A per pair of
// agents closer than 0.15.  The rules never end an episode: the time limit truncates it.  Wrapper semantics as the other
// environments: an optional one-hot agent id in front of agents_view, a shared global_state, AutoResetWrapper and
// RecordEpisodeMetrics bookkeeping (env_common.h).
//
// A workgroup of THREADS = 8 NE threads owns NE environments; lane u < A of an 8-lane group holds agent u and landmark u
// in registers from the one state load to the one state store:
//   rule phase    - lane u moves agent u and publishes it to LDS; then lane u takes landmark u's distance to the closest
//                   agent and counts the agents v > u closer than 0.15 to agent u; lane 0 of the group sums both in
//                   ascending index and does the bookkeeping;
//   reset         - a lane draws its own four Philox words (agent u: draws 2u, 2u + 1; landmark u: 2A + 2u, 2A + 2u + 1);
//   output phase  - all threads, from the table in LDS: the agents_view rows, the masks and the global_state rows of a
//                   workgroup's environments are one contiguous run each, a thread one float of every THREADS.
// Bit-exactness against the model: every float expression is one rounded operation.  The file is built with
// -ffp-contract=fast, under which a product may be fused into a following sum, so every product that feeds a sum passes
// through rounded().  Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays
// from a captured graph.  The REAL instantiation of the same body (real_view given) also writes the pre-reset
// agents_view / action_mask (and global_state, when asked for) and the `terminated` flag, which is always 0.
#include "env_common.h"

namespace {

constexpr uint32_t SPREAD_RESET = 0x53505244u;  // "SPRD"
constexpr int MINA = 2, MAXA = 8;
constexpr int NE = 32;             // environments per workgroup, 8 lanes each
constexpr int THREADS = MAXA * NE;
constexpr int ACT = 2;             // action components
constexpr float STEP_SIZE = 0.1f, COLLISION_DIST = 0.15f, COLLISION_COST = 0.5f;

struct SpreadArgs {
  int E, A, add_id, time_limit;
  float inv_a;               // 1 / A
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  float* agent_pos;          // (E, A, 2) (x, y)
  float* landmark_pos;       // (E, A, 2)
  int32_t* step_count;       // (E, A)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, A, [A +] 4 A)
  float* global_state;       // (E, 1, 4 A)
  uint8_t* action_mask;      // (E, A, 2)
  int32_t* obs_step_count;   // (E, A)
  float* reward;             // (E, A) or null (reset)
  uint8_t* done;
  float* info_return;
  int32_t* info_length;
  uint8_t* info_terminal;
  const float* action;       // (E, A, 2) or null (reset)
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct SpreadReal {
  float* view;               // (E, A, obs_dim) pre-reset agents_view
  uint8_t* mask;             // (E, A, 2) pre-reset action_mask
  uint8_t* terminated;       // (E)
  float* state;              // (E, 1, 4 A) pre-reset global_state, or null
};

struct Tile {
  float px[NE][MAXA], py[NE][MAXA];  // agents
  float lx[NE][MAXA], ly[NE][MAXA];  // landmarks
  float near[NE][MAXA];              // landmark u's distance to the closest agent
  int pairs[NE][MAXA];               // agents v > u closer than COLLISION_DIST to agent u
  int sc[NE], term[NE], rst[NE];
  float rew[NE];
};

// The value is rounded to f32 here: a product that went through cannot be fused into the sum that uses it.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ float dist(float xa, float ya, float xb, float yb) {
  const float dx = xa - xb, dy = ya - yb;
  return sqrtf(rounded(dx * dx) + rounded(dy * dy));
}

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// column `col` of the agents_view row of agent i: [one-hot id,] own position, landmarks - self, other agents - self
__device__ __forceinline__ float view_value(const SpreadArgs& a, const Tile& s, int le, int i, int col) {
  const int A = a.A;
  int c = col;
  if (a.add_id) {
    if (c < A) return c == i ? 1.0f : 0.0f;
    c -= A;
  }
  if (c < 2) return c == 0 ? s.px[le][i] : s.py[le][i];
  c -= 2;
  const int k = c & 1;
  if (c < 2 * A) {
    const int l = c >> 1;
    return k == 0 ? s.lx[le][l] - s.px[le][i] : s.ly[le][l] - s.py[le][i];
  }
  const int b = (c - 2 * A) >> 1;
  const int j = b + (b >= i ? 1 : 0);
  return k == 0 ? s.px[le][j] - s.px[le][i] : s.py[le][j] - s.py[le][i];
}

// all threads: the agents_view rows, the masks and (when gs is not null) the global_state rows of the workgroup
__device__ __forceinline__ void write_obs(const SpreadArgs& a, const Tile& s, float* av, float* gs, uint8_t* mk, int e0, int ne,
                                          int tid) {
  const int A = a.A;
  const int OD = (a.add_id ? A : 0) + 4 * A;
  for (int q = tid; q < ne * A * OD; q += THREADS) {
    const int row = q / OD, le = row / A;
    av[(long)e0 * A * OD + q] = view_value(a, s, le, row - le * A, q - row * OD);
  }
  for (int q = tid; q < ne * A * ACT; q += THREADS) mk[(long)e0 * A * ACT + q] = 1;
  if (gs != nullptr) {
    const int SD = 4 * A;
    for (int q = tid; q < ne * SD; q += THREADS) {
      const int le = q / SD, c = q - le * SD, j = (c >> 1) % A, k = c & 1;
      gs[(long)e0 * SD + q] = c < 2 * A ? (k == 0 ? s.px[le][j] : s.py[le][j]) : (k == 0 ? s.lx[le][j] : s.ly[le][j]);
    }
  }
}

template <bool REAL>
__device__ __forceinline__ void spread_step_body(const SpreadArgs& a, const SpreadReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x, u = tid & (MAXA - 1), le = tid / MAXA;  // lane u of group le: agent / landmark u of env e0 + le
  const int A = a.A;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);
  if (ne <= 0) return;
  const bool live = le < ne;
  const bool unit = live && u < A;
  const int e = e0 + le;
  const long ka = (long)e * A + u;

  // ---------------------------------------------------------------- state load
  float x = 0.0f, y = 0.0f, gx = 0.0f, gy = 0.0f, ax = 0.0f, ay = 0.0f;
  if (unit && !a.is_reset) {
    x = a.agent_pos[2 * ka]; y = a.agent_pos[2 * ka + 1];
    gx = a.landmark_pos[2 * ka]; gy = a.landmark_pos[2 * ka + 1];
    ax = a.action[2 * ka]; ay = a.action[2 * ka + 1];
  }
  if (u == 0) { s.rst[le] = (live && a.is_reset) ? 1 : 0; s.term[le] = 0; s.rew[le] = 0.0f; s.sc[le] = 0; }
  const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);

  if (!a.is_reset) {  // (a kernel argument: every thread takes the same side, the barriers inside are uniform)
    // -------------------------------------------------------------- the move
    x = clamp1(x + rounded(STEP_SIZE * clamp1(ax)));
    y = clamp1(y + rounded(STEP_SIZE * clamp1(ay)));
    s.px[le][u] = x; s.py[le][u] = y; s.lx[le][u] = gx; s.ly[le][u] = gy;
    __syncthreads();

    // -------------------------------------------------------------- reward: per landmark, per agent, then lane 0
    if (unit) {
      float m = dist(s.px[le][0], s.py[le][0], gx, gy);
      for (int i = 1; i < A; ++i) m = fminf(m, dist(s.px[le][i], s.py[le][i], gx, gy));
      int n = 0;
      for (int v = u + 1; v < A; ++v) n += dist(x, y, s.px[le][v], s.py[le][v]) < COLLISION_DIST ? 1 : 0;
      s.near[le][u] = m;
      s.pairs[le][u] = n;
    }
    __syncthreads();
    if (live && u == 0) {
      float acc = 0.0f;
      int n = 0;
      for (int l = 0; l < A; ++l) {
        acc = acc + s.near[le][l];
        n += s.pairs[le][l];
      }
      const float cover = rounded(acc * a.inv_a);
      const float fine = rounded(rounded(COLLISION_COST * (float)n) * a.inv_a);
      const float rew = -cover - fine;
      if constexpr (REAL) rn.terminated[e] = 0;
      const EpisodeEnd end = episode_step(episode_book(a), e, a.step_count[(long)e * A], rew, false, a.time_limit);
      s.rew[le] = rew;
      s.term[le] = end.term ? 1 : 0;
      s.rst[le] = end.term ? 1 : 0;
      s.sc[le] = end.step_count;
    }
    __syncthreads();
    if constexpr (REAL) {
      // the pre-reset observation of every env (equal to the returned one where the step did not end)
      write_obs(a, s, rn.view, rn.state, rn.mask, e0, ne, tid);
      __syncthreads();
    }
  } else {
    if (live && u == 0) episode_clear(episode_book(a), e);
    __syncthreads();
  }

  // ---------------------------------------------------------------- (auto-)reset at this step's counter
  if (unit && s.rst[le] != 0) {
    const uint32_t g = a.env_offset + (uint32_t)e;
    const Philox4 pa = philox4x32_10(g, t, (uint32_t)(u >> 1), SPREAD_RESET, a.seed_lo, a.seed_hi);
    const Philox4 pl = philox4x32_10(g, t, (uint32_t)((A + u) >> 1), SPREAD_RESET, a.seed_lo, a.seed_hi);
    const int wa = (2 * u) & 3, wl = (2 * (A + u)) & 3;
    x = rounded(2.0f * ((float)(word_of(pa, wa) >> 8) * 0x1.0p-24f)) - 1.0f;
    y = rounded(2.0f * ((float)(word_of(pa, wa + 1) >> 8) * 0x1.0p-24f)) - 1.0f;
    gx = rounded(2.0f * ((float)(word_of(pl, wl) >> 8) * 0x1.0p-24f)) - 1.0f;
    gy = rounded(2.0f * ((float)(word_of(pl, wl + 1) >> 8) * 0x1.0p-24f)) - 1.0f;
  }
  if (unit) { s.px[le][u] = x; s.py[le][u] = y; s.lx[le][u] = gx; s.ly[le][u] = gy; }
  __syncthreads();

  // ---------------------------------------------------------------- output phase (all threads)
  write_obs(a, s, a.agents_view, a.global_state, a.action_mask, e0, ne, tid);
  if (unit) {  // the advanced state, from this lane's registers
    a.agent_pos[2 * ka] = x; a.agent_pos[2 * ka + 1] = y;
    a.landmark_pos[2 * ka] = gx; a.landmark_pos[2 * ka + 1] = gy;
    a.step_count[ka] = s.sc[le];
    a.obs_step_count[ka] = s.sc[le];
    if (!a.is_reset) {
      a.reward[ka] = s.rew[le];
      a.done[ka] = (uint8_t)s.term[le];
    }
  }
}

__global__ __launch_bounds__(THREADS) void spread_step_kernel(SpreadArgs a) { spread_step_body<false>(a, SpreadReal{}); }

__global__ __launch_bounds__(THREADS) void spread_step_real_kernel(SpreadArgs a, SpreadReal rn) { spread_step_body<true>(a, rn); }

}  // namespace

extern "C" int mava_spread_step(int E, int A, int add_agent_id, int time_limit, uint64_t seed, uint32_t t,
                                const uint32_t* t_base, uint32_t env_offset, int is_reset, float* agent_pos,
                                float* landmark_pos, int32_t* step_count, float* run_return, int32_t* run_length,
                                float* ep_return, int32_t* ep_length, float* agents_view, float* global_state,
                                uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                                float* info_return, int32_t* info_length, uint8_t* info_terminal, const float* action,
                                float* real_view, uint8_t* real_mask, uint8_t* terminated, float* real_state,
                                hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= MINA && A <= MAXA, 0, "mava_spread_step: bad shape E=%d A=%d (%d <= A <= %d)", E, A, MINA, MAXA);
  MAVA_ARG_CHECK(time_limit >= 1, 1, "mava_spread_step: bad scenario time_limit=%d (time_limit >= 1)", time_limit);
  MAVA_ARG_CHECK((long)E * A * 5 * A < (1L << 31), 3, "mava_spread_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(agent_pos && landmark_pos && step_count && run_return && run_length && ep_return && ep_length && agents_view &&
                     global_state && action_mask && obs_step_count,
                 4, "mava_spread_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_spread_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_spread_step: a step needs the (E, A, 2) f32 action array");
  SpreadArgs a;
  a.E = E; a.A = A; a.add_id = add_agent_id ? 1 : 0; a.time_limit = time_limit;
  a.inv_a = 1.0f / (float)A;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.agent_pos = agent_pos; a.landmark_pos = landmark_pos; a.step_count = step_count;
  a.run_return = run_return; a.run_length = run_length; a.ep_return = ep_return; a.ep_length = ep_length;
  a.agents_view = agents_view; a.global_state = global_state; a.action_mask = action_mask;
  a.obs_step_count = obs_step_count; a.reward = reward; a.done = done; a.info_return = info_return;
  a.info_length = info_length; a.info_terminal = info_terminal; a.action = action;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 3 || (n_real == 0 && real_state == nullptr), 7,
                 "mava_spread_step: real_view, real_mask and terminated go together (all three or none), real_state only with them");
  if (n_real == 0) {
    hipLaunchKernelGGL(spread_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask && real_state != global_state), 8,
                   "mava_spread_step: real_view / real_mask / real_state must not alias agents_view / action_mask / global_state");
    const SpreadReal rn = {real_view, real_mask, terminated, real_state};
    hipLaunchKernelGGL(spread_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
