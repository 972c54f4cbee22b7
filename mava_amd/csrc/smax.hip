// SMAX environment step (DESIGN.md "SMAX"; the rules are the contract of mava_smax_step in include/mava_hip.h and are
// stated in NumPy in tests/smax_model.py).  Na allies against Ne scripted enemies on a 32 x 32 map with continuous
// positions: a unit moves (N, E, S, W), stops or attacks an opposing unit; an env step is eight world sub-steps of move,
// fire, damage and cooldown; the team earns the enemies' lost health fraction plus 1 for a win.  Wrapper semantics of the
// reference's SmaxWrapper: one-hot agent id prepended to agents_view, a shared global_state, AutoResetWrapper and
// RecordEpisodeMetrics bookkeeping (env_common.h), plus the won flag the evaluator turns into a win rate.
//
// A workgroup of THREADS = 32 NE threads owns NE environments; lane u < Na + Ne of a 32-lane group holds unit u (allies
// first) in registers from the one state load to the one state store:
//   state load    - position, health, cooldown and last action into registers, a copy of what the others read into LDS;
//   rule phase    - one lane per unit.  An ally checks its action against the state at the start of the step, an enemy
//                   scans the allies in LDS in ascending index for the closest one in sight.  Then eight sub-steps with
//                   two barriers each: movers publish their new position and health, every lane tests its own target
//                   and publishes "I fire at v", every lane sums the damage aimed at it over the lanes in ascending
//                   index.  Lane 0 of the group sums the reward in ascending enemy index and does the bookkeeping;
//   reset         - a lane draws its own two Philox words (unit u uses draws 2u and 2u + 1 of block u / 2);
//   output phase  - all threads, from the unit table in LDS.  A wave writes one agents_view row at a time, a lane one
//                   float of every 64 (consecutive lanes, consecutive addresses: rows are Na + 11 (U - 1) + 10 floats, an
//                   odd count for most scenarios, so there is no 16-byte path); global_state and the mask of a
//                   workgroup's environments are one contiguous run each.
// Bit-exactness against the model: every float expression is one rounded operation.  The file is built with
// -ffp-contract=fast, under which a product may be fused into a following sum, so every product that feeds a sum passes
// through rounded(); distances stay squared and every division is a multiplication by a reciprocal from the host's table.
// Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays from a captured
// graph.  The REAL instantiation of the same body (real_view given) also writes the pre-reset agents_view /
// action_mask and the `terminated` flag (a side wiped out; a time-limit end alone is a truncation).
#include "env_common.h"

namespace {

constexpr uint32_t SMAX_RESET = 0x534D4158u;  // "SMAX"
constexpr int MAXSIDE = 16, MAXU = 2 * MAXSIDE;
constexpr int NE = 8;              // environments per workgroup, 32 lanes each
constexpr int THREADS = 32 * NE;
constexpr int NT = 6;              // unit types: marine marauder stalker zealot zergling hydralisk
constexpr int SUBSTEPS = 8;
constexpr int NORTH = 0, EAST = 1, SOUTH = 2, WEST = 3, STOP = 4, ATTACK = 5;
constexpr int BLK = 11, OWN = 10, GSU = 12;  // floats of another unit's block, of the own block, of a global_state unit
constexpr float MAP = 32.0f, INV_MAP = 0.03125f, CENTRE = 16.0f;

// the unit table, filled on the host (reciprocals are host divisions: the kernel only multiplies)
struct UnitTable {
  float health[NT], damage[NT], range2[NT], sight2[NT], step[NT];  // step = speed / 16: one sub-step's move
  float inv_health[NT], inv_sight[NT], inv_cd[NT];
  int cooldown[NT];
};

struct SmaxArgs {
  int E, Na, Ne, time_limit, see_enemy_actions, walls_cause_death;
  uint64_t ally_types, enemy_types;  // one nibble per unit
  float inv_ne, inv_act;             // 1 / Ne, 1 / (5 + max(Na, Ne))
  UnitTable tab;
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  float* pos;                // (E, U, 2) (x, y)
  float* health;             // (E, U)
  int32_t* cd;               // (E, U) weapon cooldown in sub-steps
  int32_t* last_action;      // (E, U)
  int32_t* step_count;       // (E, Na)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, Na, Na + 11 (U - 1) + 10)
  float* global_state;       // (E, 1, 12 U)
  uint8_t* action_mask;      // (E, Na, 5 + Ne)
  int32_t* obs_step_count;   // (E, Na)
  float* reward;             // (E, Na) or null (reset)
  uint8_t* done;
  float* info_return;
  int32_t* info_length;
  uint8_t* info_terminal;
  uint8_t* info_won;         // (E) or null
  const int32_t* action;     // (E, Na) or null (reset)
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct SmaxReal {
  float* view;               // (E, Na, obs_dim) pre-reset agents_view
  uint8_t* mask;             // (E, Na, 5 + Ne) pre-reset action_mask
  uint8_t* terminated;       // (E)
};

struct Tile {
  UnitTable tab;
  float x[NE][MAXU], y[NE][MAXU], h[NE][MAXU];
  float part[NE][MAXU];      // an enemy's lost health fraction of this step
  int cd[NE][MAXU], la[NE][MAXU], ty[NE][MAXU];
  int fire[NE][MAXU];        // the unit this lane fires at in the current sub-step, or -1
  int sc[NE], term[NE], rst[NE];
  float rew[NE];
};

// The value is rounded to f32 here: a product that went through cannot be fused into the sum that uses it.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ float dist2(float xu, float yu, float xv, float yv) {
  const float dx = xv - xu, dy = yv - yu;
  return rounded(dx * dx) + rounded(dy * dy);
}

// the move that closes the larger of |dx|, |dy| (ties go to x)
__device__ __forceinline__ int toward(float dx, float dy) {
  return fabsf(dx) >= fabsf(dy) ? (dx > 0.0f ? EAST : WEST) : (dy > 0.0f ? NORTH : SOUTH);
}

// rule 2: enemy lane (position x, y, type t) chooses among the allies of environment le as they stand in LDS
__device__ __forceinline__ int enemy_action(const Tile& s, int le, int Na, float x, float y, int t) {
  int best = -1;
  float bd = 0.0f;
  for (int i = 0; i < Na; ++i) {
    if (!(s.h[le][i] > 0.0f)) continue;
    const float d = dist2(x, y, s.x[le][i], s.y[le][i]);
    if (d <= s.tab.sight2[t] && (best < 0 || d < bd)) { best = i; bd = d; }
  }
  if (best >= 0 && bd <= s.tab.range2[t]) return ATTACK + best;
  const float dx = (best >= 0 ? s.x[le][best] : CENTRE) - x, dy = (best >= 0 ? s.y[le][best] : CENTRE) - y;
  if (best < 0 && fabsf(dx) < 0.5f && fabsf(dy) < 0.5f) return STOP;
  return toward(dx, dy);
}

// float f of the own block of unit j: [health / max, x / 32, y / 32, cd / type cd, type one-hot]
__device__ __forceinline__ float own_value(const Tile& s, int le, int j, int f) {
  const int t = s.ty[le][j];
  if (f == 0) return s.h[le][j] * s.tab.inv_health[t];
  if (f == 1) return s.x[le][j] * INV_MAP;
  if (f == 2) return s.y[le][j] * INV_MAP;
  if (f == 3) return (float)s.cd[le][j] * s.tab.inv_cd[t];
  return t == f - 4 ? 1.0f : 0.0f;
}

// column `col` of the agents_view row of ally i
__device__ __forceinline__ float view_value(const SmaxArgs& a, const Tile& s, int le, int i, int col) {
  const int Na = a.Na, U = Na + a.Ne;
  if (col < Na) return col == i ? 1.0f : 0.0f;
  if (!(s.h[le][i] > 0.0f)) return 0.0f;  // a dead viewer sees nothing, not even itself
  const int c = col - Na;
  if (c >= BLK * (U - 1)) return own_value(s, le, i, c - BLK * (U - 1));
  const int b = c / BLK, f = c - b * BLK;
  const int j = b + (b >= i ? 1 : 0);  // the other allies in ascending index, then the enemies
  const int ti = s.ty[le][i], tj = s.ty[le][j];
  const float xi = s.x[le][i], yi = s.y[le][i], xj = s.x[le][j], yj = s.y[le][j];
  if (!(s.h[le][j] > 0.0f) || !(dist2(xi, yi, xj, yj) <= s.tab.sight2[ti])) return 0.0f;
  if (f == 0) return s.h[le][j] * s.tab.inv_health[tj];
  if (f == 1) return (xj - xi) * s.tab.inv_sight[ti];
  if (f == 2) return (yj - yi) * s.tab.inv_sight[ti];
  if (f == 3) return (j >= Na && !a.see_enemy_actions) ? 0.0f : (float)(s.la[le][j] + 1) * a.inv_act;
  if (f == 4) return (float)s.cd[le][j] * s.tab.inv_cd[tj];
  return tj == f - 5 ? 1.0f : 0.0f;
}

// entry `act` of the mask of ally i
__device__ __forceinline__ uint8_t mask_value(const SmaxArgs& a, const Tile& s, int le, int i, int act) {
  if (act == STOP) return 1;
  if (!(s.h[le][i] > 0.0f)) return 0;
  if (act < STOP) return 1;
  const int v = a.Na + act - ATTACK;
  return (s.h[le][v] > 0.0f && dist2(s.x[le][i], s.y[le][i], s.x[le][v], s.y[le][v]) <= s.tab.range2[s.ty[le][i]]) ? 1 : 0;
}

// all threads: the agents_view rows, the masks and (when gs is not null) the global_state rows of the workgroup
__device__ __forceinline__ void write_obs(const SmaxArgs& a, const Tile& s, float* av, float* gs, uint8_t* mk, int e0, int ne,
                                          int tid) {
  const int Na = a.Na, U = Na + a.Ne, nA = ATTACK + a.Ne;
  const int OD = Na + BLK * (U - 1) + OWN;
  const int wave = tid >> 6, lane = tid & 63;
  for (int row = wave; row < ne * Na; row += THREADS / 64) {
    const int le = row / Na, i = row - le * Na;
    float* o = av + ((long)e0 * Na + row) * OD;
    for (int col = lane; col < OD; col += 64) o[col] = view_value(a, s, le, i, col);
  }
  for (int q = tid; q < ne * Na * nA; q += THREADS) {
    const int row = q / nA, le = row / Na;
    mk[(long)e0 * Na * nA + q] = mask_value(a, s, le, row - le * Na, q - row * nA);
  }
  if (gs != nullptr) {
    for (int q = tid; q < ne * U * GSU; q += THREADS) {
      const int ju = q / GSU, f = q - ju * GSU, le = ju / U, j = ju - le * U;
      float v = 0.0f;
      if (s.h[le][j] > 0.0f) v = f < OWN ? own_value(s, le, j, f) : (((f == OWN) == (j < Na)) ? 1.0f : 0.0f);
      gs[(long)e0 * U * GSU + q] = v;
    }
  }
}

template <bool REAL>
__device__ __forceinline__ void smax_step_body(const SmaxArgs& a, const SmaxReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x, u = tid & 31, le = tid >> 5;  // lane u of group le: unit u of environment e0 + le
  const int Na = a.Na, Ne = a.Ne, U = Na + Ne;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);
  if (ne <= 0) return;
  const bool live = le < ne;
  const bool unit = live && u < U, ally = unit && u < Na;
  const int e = e0 + le;
  const long ku = (long)e * U + u, ka = (long)e * Na + u;
  const uint64_t nibbles = u < Na ? a.ally_types >> (4 * u) : a.enemy_types >> (4 * ((u - Na) & 15));
  const int ty = min((int)(nibbles & 15u), NT - 1);

  // ---------------------------------------------------------------- state load
  if (tid < NT) {
    s.tab.health[tid] = a.tab.health[tid]; s.tab.damage[tid] = a.tab.damage[tid]; s.tab.range2[tid] = a.tab.range2[tid];
    s.tab.sight2[tid] = a.tab.sight2[tid]; s.tab.step[tid] = a.tab.step[tid]; s.tab.inv_health[tid] = a.tab.inv_health[tid];
    s.tab.inv_sight[tid] = a.tab.inv_sight[tid]; s.tab.inv_cd[tid] = a.tab.inv_cd[tid]; s.tab.cooldown[tid] = a.tab.cooldown[tid];
  }
  float x = 0.0f, y = 0.0f, h = 0.0f;
  int cd = 0, exe = STOP, raw = STOP;
  if (unit && !a.is_reset) {
    x = a.pos[2 * ku]; y = a.pos[2 * ku + 1]; h = a.health[ku]; cd = a.cd[ku];
    if (ally) raw = a.action[ka];
  }
  s.x[le][u] = x; s.y[le][u] = y; s.h[le][u] = h; s.ty[le][u] = ty; s.fire[le][u] = -1; s.part[le][u] = 0.0f;
  if (u == 0) { s.rst[le] = (live && a.is_reset) ? 1 : 0; s.term[le] = 0; s.rew[le] = 0.0f; s.sc[le] = 0; }
  __syncthreads();
  const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);

  if (!a.is_reset) {  // (a kernel argument: every thread takes the same side, the barriers inside are uniform)
    // -------------------------------------------------------------- rules 1 and 2: the action each unit executes
    const float range2 = s.tab.range2[ty], step = s.tab.step[ty];
    int tgt = -1;
    if (unit && h > 0.0f) {
      if (ally) {
        if (raw >= 0 && raw < ATTACK) {
          exe = raw;
        } else if (raw >= ATTACK && raw < ATTACK + Ne) {
          const int v = Na + raw - ATTACK;  // a dead or out-of-range target: a stop
          if (s.h[le][v] > 0.0f && dist2(x, y, s.x[le][v], s.y[le][v]) <= range2) exe = raw;
        }
      } else {
        exe = enemy_action(s, le, Na, x, y, ty);
      }
      if (exe >= ATTACK) tgt = ally ? Na + exe - ATTACK : exe - ATTACK;
    }
    const float h0 = h;
    __syncthreads();  // the decisions read the start-of-step table: nobody publishes a move before all have decided

    // -------------------------------------------------------------- rule 3: eight sub-steps
    for (int ss = 0; ss < SUBSTEPS; ++ss) {
      if (unit && h > 0.0f && exe < STOP) {  // move: one add of the precomputed speed / 16
        const float nx = exe == EAST ? x + step : (exe == WEST ? x - step : x);
        const float ny = exe == NORTH ? y + step : (exe == SOUTH ? y - step : y);
        if (a.walls_cause_death && (nx < 0.0f || nx > MAP || ny < 0.0f || ny > MAP)) h = 0.0f;
        x = fminf(fmaxf(nx, 0.0f), MAP);
        y = fminf(fmaxf(ny, 0.0f), MAP);
      }
      s.x[le][u] = x; s.y[le][u] = y; s.h[le][u] = h;
      __syncthreads();
      const bool alive = unit && h > 0.0f;  // after the move
      const bool fires = alive && tgt >= 0 && cd == 0 && s.h[le][tgt] > 0.0f &&
                         dist2(x, y, s.x[le][tgt], s.y[le][tgt]) <= range2;
      s.fire[le][u] = fires ? tgt : -1;
      __syncthreads();
      float total = 0.0f;  // integers: exact in any order, summed in ascending attacker index all the same
      for (int v = 0; v < U; ++v)
        if (s.fire[le][v] == u) total += s.tab.damage[s.ty[le][v]];
      h = fmaxf(0.0f, h - total);
      cd = fires ? s.tab.cooldown[ty] : (alive ? max(0, cd - 1) : cd);
    }
    s.h[le][u] = h; s.cd[le][u] = cd; s.la[le][u] = exe;
    if (unit && !ally) s.part[le][u] = (h0 - h) * s.tab.inv_health[ty];
    __syncthreads();

    // -------------------------------------------------------------- rules 4 and 5: reward and bookkeeping
    if (live && u == 0) {
      float acc = 0.0f;
      bool enemy_alive = false, ally_alive = false;
      for (int k = 0; k < Ne; ++k) {
        acc = acc + s.part[le][Na + k];
        enemy_alive |= s.h[le][Na + k] > 0.0f;
      }
      for (int i = 0; i < Na; ++i) ally_alive |= s.h[le][i] > 0.0f;
      const bool won = !enemy_alive && ally_alive;
      const float rew = rounded(acc * a.inv_ne) + (won ? 1.0f : 0.0f);
      const bool terminated = !enemy_alive || !ally_alive;
      if constexpr (REAL) rn.terminated[e] = terminated ? 1 : 0;
      const EpisodeEnd end = episode_step(episode_book(a), e, a.step_count[(long)e * Na], rew, terminated, a.time_limit);
      if (a.info_won != nullptr) a.info_won[e] = (end.term && won) ? 1 : 0;
      s.rew[le] = rew;
      s.term[le] = end.term ? 1 : 0;
      s.rst[le] = end.term ? 1 : 0;
      s.sc[le] = end.step_count;
    }
    __syncthreads();
    if constexpr (REAL) {
      // the pre-reset observation of every env (equal to the returned one where the step did not end)
      write_obs(a, s, rn.view, nullptr, rn.mask, e0, ne, tid);
      __syncthreads();
    }
  } else if (live && u == 0) {
    episode_clear(episode_book(a), e);
  }

  // ---------------------------------------------------------------- (auto-)reset at this step's counter
  if (unit && s.rst[le] != 0) {
    const Philox4 p = philox4x32_10(a.env_offset + (uint32_t)e, t, (uint32_t)(u >> 1), SMAX_RESET, a.seed_lo, a.seed_hi);
    const int w = (2 * u) & 3;  // draws 2u and 2u + 1
    const float ux = (float)(word_of(p, w) >> 8) * 0x1.0p-24f, uy = (float)(word_of(p, w + 1) >> 8) * 0x1.0p-24f;
    x = (ally ? 6.0f : 22.0f) + rounded(4.0f * ux);
    y = 14.0f + rounded(4.0f * uy);
    h = s.tab.health[ty]; cd = 0; exe = STOP;
    s.x[le][u] = x; s.y[le][u] = y; s.h[le][u] = h; s.cd[le][u] = cd; s.la[le][u] = exe;
  }
  __syncthreads();

  // ---------------------------------------------------------------- output phase (all threads)
  write_obs(a, s, a.agents_view, a.global_state, a.action_mask, e0, ne, tid);
  if (unit) {  // the advanced state, from this lane's registers
    a.pos[2 * ku] = x; a.pos[2 * ku + 1] = y; a.health[ku] = h; a.cd[ku] = cd; a.last_action[ku] = exe;
    if (ally) {
      a.step_count[ka] = s.sc[le];
      a.obs_step_count[ka] = s.sc[le];
      if (!a.is_reset) {
        a.reward[ka] = s.rew[le];
        a.done[ka] = (uint8_t)s.term[le];
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void smax_step_kernel(SmaxArgs a) { smax_step_body<false>(a, SmaxReal{}); }

__global__ __launch_bounds__(THREADS) void smax_step_real_kernel(SmaxArgs a, SmaxReal rn) { smax_step_body<true>(a, rn); }

// health, damage, attack range, sight range, speed, weapon cooldown (sub-steps) of the six unit types
const float UNIT_HEALTH[NT] = {45.0f, 125.0f, 160.0f, 150.0f, 35.0f, 80.0f};
const float UNIT_DAMAGE[NT] = {9.0f, 10.0f, 13.0f, 8.0f, 5.0f, 12.0f};
const float UNIT_RANGE[NT] = {5.0f, 6.0f, 6.0f, 2.0f, 2.0f, 5.0f};
const float UNIT_SIGHT[NT] = {9.0f, 10.0f, 10.0f, 9.0f, 8.0f, 9.0f};
const float UNIT_SPEED[NT] = {3.15f, 2.25f, 4.13f, 3.15f, 4.13f, 3.15f};
const int UNIT_COOLDOWN[NT] = {10, 18, 30, 14, 8, 10};

bool types_ok(uint64_t types, int n) {
  for (int i = 0; i < n; ++i)
    if (((types >> (4 * i)) & 15u) >= (uint64_t)NT) return false;
  return true;
}

}  // namespace

extern "C" int mava_smax_step(int E, int A, int Ne, uint64_t ally_types, uint64_t enemy_types, int time_limit,
                              int see_enemy_actions, int walls_cause_death, uint64_t seed, uint32_t t,
                              const uint32_t* t_base, uint32_t env_offset, int is_reset, float* pos, float* health,
                              int32_t* cd, int32_t* last_action, int32_t* step_count, float* run_return,
                              int32_t* run_length, float* ep_return, int32_t* ep_length, float* agents_view,
                              float* global_state, uint8_t* action_mask, int32_t* obs_step_count, float* reward,
                              uint8_t* done, float* info_return, int32_t* info_length, uint8_t* info_terminal,
                              uint8_t* info_won, const int32_t* action, float* real_view, uint8_t* real_mask,
                              uint8_t* terminated, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && A <= MAXSIDE && Ne >= 1 && Ne <= MAXSIDE, 0,
                 "mava_smax_step: bad shape E=%d A=%d Ne=%d (1 <= A, Ne <= %d)", E, A, Ne, MAXSIDE);
  MAVA_ARG_CHECK(time_limit >= 1, 1, "mava_smax_step: bad scenario time_limit=%d (time_limit >= 1)", time_limit);
  MAVA_ARG_CHECK(types_ok(ally_types, A) && types_ok(enemy_types, Ne), 2, "mava_smax_step: a unit type nibble is not below %d", NT);
  MAVA_ARG_CHECK((long)E * A * (A + BLK * (A + Ne - 1) + OWN) < (1L << 31), 3, "mava_smax_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(pos && health && cd && last_action && step_count && run_return && run_length && ep_return && ep_length &&
                     agents_view && global_state && action_mask && obs_step_count,
                 4, "mava_smax_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_smax_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_smax_step: a step needs the (E, A) action array");
  SmaxArgs a;
  a.E = E; a.Na = A; a.Ne = Ne; a.time_limit = time_limit;
  a.see_enemy_actions = see_enemy_actions ? 1 : 0; a.walls_cause_death = walls_cause_death ? 1 : 0;
  a.ally_types = ally_types; a.enemy_types = enemy_types;
  a.inv_ne = 1.0f / (float)Ne; a.inv_act = 1.0f / (float)(ATTACK + (A > Ne ? A : Ne));
  for (int k = 0; k < NT; ++k) {
    a.tab.health[k] = UNIT_HEALTH[k]; a.tab.damage[k] = UNIT_DAMAGE[k];
    a.tab.range2[k] = UNIT_RANGE[k] * UNIT_RANGE[k]; a.tab.sight2[k] = UNIT_SIGHT[k] * UNIT_SIGHT[k];
    a.tab.step[k] = UNIT_SPEED[k] * 0.0625f;
    a.tab.inv_health[k] = 1.0f / UNIT_HEALTH[k]; a.tab.inv_sight[k] = 1.0f / UNIT_SIGHT[k];
    a.tab.inv_cd[k] = 1.0f / (float)UNIT_COOLDOWN[k]; a.tab.cooldown[k] = UNIT_COOLDOWN[k];
  }
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.pos = pos; a.health = health; a.cd = cd; a.last_action = last_action; a.step_count = step_count;
  a.run_return = run_return; a.run_length = run_length; a.ep_return = ep_return; a.ep_length = ep_length;
  a.agents_view = agents_view; a.global_state = global_state; a.action_mask = action_mask;
  a.obs_step_count = obs_step_count; a.reward = reward; a.done = done; a.info_return = info_return;
  a.info_length = info_length; a.info_terminal = info_terminal; a.info_won = is_reset ? nullptr : info_won;
  a.action = action;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 0 || n_real == 3, 7,
                 "mava_smax_step: real_view, real_mask and terminated go together (all three or none)");
  if (n_real == 0) {
    hipLaunchKernelGGL(smax_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask), 8,
                   "mava_smax_step: real_view / real_mask must not alias agents_view / action_mask");
    const SmaxReal rn = {real_view, real_mask, terminated};
    hipLaunchKernelGGL(smax_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
