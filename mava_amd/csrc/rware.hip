// Robot Warehouse environment step (DESIGN.md "Robot Warehouse"; the rules are the contract of mava_rware_step in
// include/mava_hip.h and are restated in NumPy in tests/rware_model.py).  An H x W warehouse of highways and shelf
// homes, A robots that turn, drive forward and load / unload shelves, S shelves and a queue of R requested shelves; a
// robot standing on a goal cell with a requested shelf scores 1 for the team and the request is replaced.
// Wrapper semantics as in lbf.hip: one-hot agent id prepended to agents_view, global_state = the concatenated raw
// views, team reward repeated per agent, AutoResetWrapper and RecordEpisodeMetrics bookkeeping.
//
// The layout (highway row masks, the shelves' home cells) is a pure function of the scenario: the host builds it once
// and passes it by value (RwLayout, 640 bytes of kernel arguments); no thread recomputes it.
//
// Shape of the kernel: a workgroup of 1024 threads owns NE = 16 environments (one workgroup per CU at 4096 envs; measured
// 23.4 / 16.7 / 14.9 us per launch with 256 / 512 / 1024 threads: the cooperative phases are latency-bound).
//   state load    - all threads copy the workgroup's contiguous state ranges into LDS ([field][index][env]) and clamp
//                   every index to its range, so that a corrupt state cannot index outside a table;
//   ground tables - all threads, one (env, shelf) each: the row bit masks of the shelves standing on the ground and the
//                   home-slot -> shelf table the load / unload rule needs (a ground shelf always stands on a home cell:
//                   unloading on a highway is refused);
//   rule phase    - thread e < NE runs environment e's rules on the LDS state (no loop over the shelves: masks and the
//                   slot table answer "is there a ground shelf" and "which one"), then the rare reset draws;
//   reset fill    - all threads put the shelves of the environments that reset back on their homes;
//   row bytes     - all threads, one byte each: per (env, agent) row the 8 header features, the FORWARD mask bit and one
//                   packed code per view cell (agent?, its direction, shelf?, requested?) from the row masks and a
//                   scan over the A agents;
//   output phase  - a wave writes whole (env, agent) rows of agents_view and global_state from the row bytes, its lanes
//                   the consecutive features (no division by a run-time width per element), then all threads the masks
//                   and the advanced state: every store instruction covers consecutive addresses.
// Everything is a pure function of the device state and (seed, t + *t_base, env id): the step replays from a captured
// graph.  The REAL instantiation of the same body (real_view given) also writes the pre-reset agents_view /
// action_mask and the `terminated` flag (a collision in collision mode "terminate"; a time-limit end is a truncation).
#include "env_common.h"

namespace {

#ifdef MAVA_STAMPS
#define STAMP_DECL unsigned long long st_prev = __builtin_readcyclecounter(), st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define STAMP(i)                                                    \
  do {                                                              \
    __builtin_amdgcn_sched_barrier(0);                              \
    const unsigned long long st_now = __builtin_readcyclecounter(); \
    st_acc[i] += st_now - st_prev;                                  \
    st_prev = st_now;                                               \
    __builtin_amdgcn_sched_barrier(0);                              \
  } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#endif

constexpr uint32_t RW_RESET = 0x52575253u;  // "RWRS"
constexpr uint32_t RW_QUEUE = 0x52575251u;  // "RWRQ"
constexpr int MAXW = 32, MAXH = 32, MAXA = 16, MAXS = 256, MAXR = 16, MAXSR = 2;
constexpr int MAXC = (2 * MAXSR + 1) * (2 * MAXSR + 1);  // view cells per agent
constexpr int NE = 16;        // environments per workgroup
constexpr int THREADS = 1024;  // 16 waves: four per SIMD hide the LDS / store latency of the cooperative phases
constexpr int N_ACT = 5;      // NOOP FORWARD LEFT RIGHT TOGGLE_LOAD
constexpr int HEAD = 8, CELL = 7;  // raw view = [x, y, carrying, dir one-hot (4), on_highway] + 7 per view cell
constexpr int ROWB = HEAD + 1;     // bytes of a Tile::code row in front of the view cells' codes

struct RwLayout {
  uint32_t hw[MAXH];     // bit x of row y: cell (x, y) is a highway
  uint16_t home[MAXS];   // home cell (y * W + x) of shelf s, increasing
};

struct RwArgs {
  int E, A, S, R, H, W, sr, time_limit, terminate;
  uint32_t seed_lo, seed_hi;
  uint32_t t;
  const uint32_t* t_base;
  uint32_t env_offset;
  int is_reset;
  int32_t* agent_pos;        // (E, A, 2) (x, y)
  int32_t* agent_dir;        // (E, A)
  int32_t* agent_carry;      // (E, A) shelf id or -1
  int32_t* shelf_pos;        // (E, S) cell
  int32_t* request_queue;    // (E, R) shelf ids
  int32_t* step_count;       // (E, A)
  float* run_return;
  int32_t* run_length;
  float* ep_return;
  int32_t* ep_length;
  float* agents_view;        // (E, A, A + raw)
  float* global_state;       // (E, 1, A * raw)
  uint8_t* action_mask;      // (E, A, 5)
  int32_t* obs_step_count;   // (E, A)
  float* reward;             // (E, A) or null (reset)
  uint8_t* done;
  float* info_return;
  int32_t* info_length;
  uint8_t* info_terminal;
  const int32_t* action;     // (E, A) or null (reset)
  unsigned long long* stamps;  // diagnostic builds (-DMAVA_STAMPS): per-phase cycle sums of block 0, thread 0
};

// extra outputs of the REAL instantiation (not written on a reset call)
struct RwReal {
  float* view;               // (E, A, A + raw) pre-reset agents_view
  uint8_t* mask;             // (E, A, 5) pre-reset action_mask
  uint8_t* terminated;       // (E) 1 on a collision termination (a time-limit end is a truncation: 0)
};

struct Tile {
  int ax[MAXA][NE], ay[MAXA][NE], ad[MAXA][NE], ac[MAXA][NE], act[MAXA][NE];
  int oc[MAXA][NE];            // the agents' cells at the start of the step (the reset's taken cells)
  int rq[MAXR][NE];
  int16_t sp[MAXS][NE];        // shelf -> cell
  int16_t slot[MAXS][NE];      // home slot -> ground shelf standing there
  uint32_t gnd[MAXH][NE];      // row masks: a shelf stands on the ground
  uint32_t req[MAXH][NE];      // row masks: a requested shelf (ground or carried)
  uint8_t code[NE * MAXA * (ROWB + MAXC)];  // build_codes
  uint32_t hw[MAXH];
  uint16_t home[MAXS];
  uint8_t slot_of[MAXW * MAXH];  // home cell -> slot
  int sc[NE], term[NE], rst[NE];
  float rew[NE];
};

// the k-th (0-based) non-negative integer that is not among the n distinct values arr[0 .. n) (stride NE): the least
// fixed point of v = k + #{arr <= v}
__device__ int kth_not_in(int k, const int* arr, int n) {
  int v = k;
  for (;;) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += arr[i * NE] <= v;
    if (k + c == v) return v;
    v = k + c;
  }
}

__device__ __forceinline__ void build_req(const RwArgs& a, Tile& s, int le, bool homes) {
  for (int y = 0; y < a.H; ++y) s.req[y][le] = 0u;
  for (int k = 0; k < a.R; ++k) {
    const int q = s.rq[k][le];
    const unsigned cell = homes ? s.home[q] : (unsigned)s.sp[q][le];
    const unsigned y = cell / (unsigned)a.W;
    s.req[y][le] |= 1u << (cell - y * a.W);
  }
}

// the reset rule: agents (cell, direction), then the request queue; draw n = word n % 4 of Philox block n / 4.  The
// shelves go home in the cooperative reset fill (s.rst)
__device__ void generate(const RwArgs& a, Tile& s, int le, uint32_t g, uint32_t t) {
  Philox4 p = {0u, 0u, 0u, 0u};
  int nd = 0;
  auto draw = [&]() -> uint32_t {
    if ((nd & 3) == 0) p = philox4x32_10(g, t, (uint32_t)(nd >> 2), RW_RESET, a.seed_lo, a.seed_hi);
    const uint32_t w = word_of(p, nd & 3);
    ++nd;
    return w;
  };
  const int HW = a.H * a.W;
  for (int j = 0; j < a.A; ++j) {
    const uint32_t d = draw();
    const int cell = kth_not_in((int)(d % (uint32_t)(HW - j)), &s.oc[0][le], j);
    s.oc[j][le] = cell;
    const int y = (unsigned)cell / (unsigned)a.W;
    s.ax[j][le] = cell - y * a.W;
    s.ay[j][le] = y;
    s.ad[j][le] = (int)(draw() & 3u);
    s.ac[j][le] = -1;
  }
  for (int k = 0; k < a.R; ++k) {
    const uint32_t d = draw();
    s.rq[k][le] = kth_not_in((int)(d % (uint32_t)(a.S - k)), &s.rq[0][le], k);
  }
  build_req(a, s, le, true);
  s.sc[le] = 0;
  s.rst[le] = 1;
}

// rule 1's test: would a FORWARD move agent j (position x, y, facing d)?
__device__ __forceinline__ bool forward_ok(const RwArgs& a, const Tile& s, int le, int x, int y, int d, bool carrying,
                                           int& tx, int& ty) {
  tx = x + (d == 1) - (d == 3);
  ty = y + (d == 2) - (d == 0);
  if (tx < 0 || tx >= a.W || ty < 0 || ty >= a.H) return false;
  return !(carrying && ((s.gnd[ty][le] >> tx) & 1u));
}

// all threads: the ground-shelf row masks and the home slot -> shelf table of the loaded state
__device__ __forceinline__ void build_ground(const RwArgs& a, Tile& s, int ne, int tid) {
  const int n = ne * a.S;
  for (int i = tid; i < n; i += THREADS) {
    const int sh = (unsigned)i / (unsigned)ne, le = i - sh * ne;
    bool carried = false;
    for (int k = 0; k < a.A; ++k) carried |= s.ac[k][le] == sh;
    if (!carried) {
      const unsigned cell = (unsigned)s.sp[sh][le];
      const unsigned y = cell / (unsigned)a.W;
      atomicOr(&s.gnd[y][le], 1u << (cell - y * a.W));
      s.slot[s.slot_of[cell]][le] = (int16_t)sh;
    }
  }
}

// all threads: ROWB + C bytes per (env, agent) row, everything the output phase needs of that agent:
//   bytes 0 .. 7  the header features [x, y, carrying, direction one-hot (4), on_highway];
//   byte 8        rule 1's test for the action mask: a FORWARD would move the agent;
//   bytes 9 ..    one packed code per view cell: bit 0 an agent stands there, bits 1-2 its direction, bit 3 a shelf
//                 (ground or carried), bit 4 a requested shelf.  The centre cell describes the viewing agent itself,
//                 any other cell the lowest-index agent on it.
__device__ __forceinline__ void build_codes(const RwArgs& a, Tile& s, int ne, int tid) {
  const int A = a.A, side = 2 * a.sr + 1, C = side * side, RS = ROWB + C;
  const int n = ne * A * RS;
  for (int i = tid; i < n; i += THREADS) {
    const int r = (unsigned)i / (unsigned)ne, le = i - r * ne;
    const int j = (unsigned)r / (unsigned)RS, b = r - j * RS;
    const int x0 = s.ax[j][le], y0 = s.ay[j][le];
    unsigned code = 0u;
    if (b < HEAD) {
      if (b == 0) code = x0;
      else if (b == 1) code = y0;
      else if (b == 2) code = s.ac[j][le] >= 0;
      else if (b < 7) code = s.ad[j][le] == b - 3;
      else code = (s.hw[y0] >> x0) & 1u;
    } else if (b == HEAD) {
      int tx, ty;
      code = forward_ok(a, s, le, x0, y0, s.ad[j][le], s.ac[j][le] >= 0, tx, ty);
    } else {
      const int c = b - ROWB;
      const int cy = (unsigned)c / (unsigned)side, cx = c - cy * side;
      const int x = x0 + cx - a.sr, y = y0 + cy - a.sr;
      if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
        int ag = -1;
        bool shelf = (s.gnd[y][le] >> x) & 1u;
        for (int k = A - 1; k >= 0; --k) {
          const bool m = s.ax[k][le] == x && s.ay[k][le] == y;
          ag = m ? k : ag;
          shelf |= m && s.ac[k][le] >= 0;
        }
        if (c == (C >> 1)) ag = j;
        const unsigned rq = (s.req[y][le] >> x) & 1u;
        code = (ag >= 0 ? 1u | ((unsigned)s.ad[ag < 0 ? 0 : ag][le] << 1) : 0u) | (shelf ? 8u : 0u) | (rq << 4);
      }
    }
    s.code[(le * A + j) * RS + b] = (uint8_t)code;
  }
}

// agents_view (and, when gs is not null, global_state) rows of the workgroup from the row bytes: a wave takes whole
// (env, agent) rows, its lanes the consecutive features of the row, so no thread divides by a run-time width and every
// store instruction covers consecutive addresses; av / gs point at row e0 * A
__device__ __forceinline__ void write_rows(const RwArgs& a, const Tile& s, float* av, float* gs, int ne, int tid) {
  const int A = a.A, side = 2 * a.sr + 1, C = side * side, RS = ROWB + C;
  const int RAW = HEAD + CELL * C, Wd = A + RAW;
  const int lane = tid & 63;
  for (int row = tid >> 6; row < ne * A; row += THREADS / 64) {
    const int j = row - ((unsigned)row / (unsigned)A) * A;
    const uint8_t* rb = s.code + row * RS;
    float* o = av + (long)row * Wd;
    if (lane < A) o[lane] = lane == j ? 1.0f : 0.0f;
    for (int q = lane; q < RAW; q += 64) {
      const int c = (unsigned)(q - HEAD) / (unsigned)CELL, f = q - HEAD - c * CELL;  // (meaningless for q < HEAD)
      const unsigned b = rb[q < HEAD ? q : ROWB + c];
      unsigned v;
      if (q < HEAD) v = b;
      else if (f == 0) v = b & 1u;
      else if (f < 5) v = (b & 1u) & (((b >> 1) & 3u) == (unsigned)(f - 1));
      else v = (b >> (f - 2)) & 1u;  // f 5 -> bit 3, f 6 -> bit 4
      const float x = (float)v;
      o[A + q] = x;
      if (gs != nullptr) gs[(long)row * RAW + q] = x;
    }
  }
}

__device__ __forceinline__ void write_mask(const RwArgs& a, const Tile& s, uint8_t* mk, int ne, int tid) {
  const int C = (2 * a.sr + 1) * (2 * a.sr + 1), RS = ROWB + C;
  const int n = ne * a.A * N_ACT;
  for (int i = tid; i < n; i += THREADS) {
    const int row = (unsigned)i / (unsigned)N_ACT, act = i - row * N_ACT;
    mk[i] = act == 1 ? s.code[row * RS + HEAD] : 1;
  }
}

template <bool REAL>
__device__ __forceinline__ void rware_step_body(const RwArgs& a, const RwLayout& lay, const RwReal& rn) {
  __shared__ Tile s;
  const int tid = threadIdx.x;
  const int A = a.A, S = a.S, R = a.R, H = a.H, W = a.W;
  const int HW = H * W;
  const int e0 = blockIdx.x * NE;
  const int ne = min(NE, a.E - e0);
  if (ne <= 0) return;
  STAMP_DECL

  // ---------------------------------------------------------------- layout and state load (all threads)
  for (int i = tid; i < H; i += THREADS) s.hw[i] = lay.hw[i];
  for (int i = tid; i < HW; i += THREADS) s.slot_of[i] = 0;
  for (int i = tid; i < NE * MAXH; i += THREADS) (&s.gnd[0][0])[i] = 0u;
  for (int i = tid; i < NE; i += THREADS) s.rst[i] = 0;
  __syncthreads();
  for (int i = tid; i < S; i += THREADS) {
    const int cell = min((int)lay.home[i], HW - 1);
    s.home[i] = (uint16_t)cell;
    s.slot_of[cell] = (uint8_t)i;
  }
  if (!a.is_reset) {
    const long ka = (long)e0 * A;
    for (int i = tid; i < ne * A * 2; i += THREADS) {
      const int k = i >> 1, le = (unsigned)k / (unsigned)A, j = k - le * A;
      const int v = a.agent_pos[2 * ka + i];
      if (i & 1) s.ay[j][le] = min(max(v, 0), H - 1); else s.ax[j][le] = min(max(v, 0), W - 1);
    }
    for (int i = tid; i < ne * A; i += THREADS) {
      const int le = (unsigned)i / (unsigned)A, j = i - le * A;
      s.ad[j][le] = a.agent_dir[ka + i] & 3;
      s.ac[j][le] = min(max(a.agent_carry[ka + i], -1), S - 1);
      s.act[j][le] = a.action[ka + i];
    }
    const long ks = (long)e0 * S, kr = (long)e0 * R;
    for (int i = tid; i < ne * S; i += THREADS) {
      const int le = (unsigned)i / (unsigned)S, sh = i - le * S;
      s.sp[sh][le] = (int16_t)min(max(a.shelf_pos[ks + i], 0), HW - 1);
      s.slot[sh][le] = 0;
    }
    for (int i = tid; i < ne * R; i += THREADS) {
      const int le = (unsigned)i / (unsigned)R, k = i - le * R;
      s.rq[k][le] = min(max(a.request_queue[kr + i], 0), S - 1);
    }
  }
  __syncthreads();
  STAMP(0);
  if (!a.is_reset) build_ground(a, s, ne, tid);
  __syncthreads();
  STAMP(1);

  // ---------------------------------------------------------------- rule phase: one thread per environment
  const uint32_t t = a.t + (a.t_base ? *a.t_base : 0u);
  if (tid < ne) {
    const int le = tid, e = e0 + tid;
    const uint32_t g = a.env_offset + (uint32_t)e;
    const EpisodeBook bk = episode_book(a);
    bool reset = a.is_reset != 0;
    if (!a.is_reset) {
      const int sc_old = a.step_count[(long)e * A];
      const EpisodeRun run = episode_load(bk, e);  // used at the end of the rule phase
      // 1. turns; FORWARD unless off the grid or a carried shelf would meet a ground shelf
      for (int j = 0; j < A; ++j) {
        const int ac = s.act[j][le];
        int x = s.ax[j][le], y = s.ay[j][le], d = s.ad[j][le];
        s.oc[j][le] = y * W + x;
        if (ac == 2) d = (d + 3) & 3;
        if (ac == 3) d = (d + 1) & 3;
        if (ac == 1) {
          int tx, ty;
          if (forward_ok(a, s, le, x, y, d, s.ac[j][le] >= 0, tx, ty)) { x = tx; y = ty; }
        }
        s.ax[j][le] = x; s.ay[j][le] = y; s.ad[j][le] = d;
      }
      // 2. collision: two agents on one cell after the moves, or two agents that exchanged cells
      bool coll = false;
      for (int j = 1; j < A; ++j) {
        const int cj = s.ay[j][le] * W + s.ax[j][le], oj = s.oc[j][le];
        for (int k = 0; k < j; ++k) {
          const int ck = s.ay[k][le] * W + s.ax[k][le], ok = s.oc[k][le];
          coll |= (cj == ck) | ((cj == ok) & (ck == oj) & (oj != ok));
        }
      }
      // 3. carried shelves follow their carriers
      for (int j = 0; j < A; ++j) {
        const int c = s.ac[j][le];
        if (c >= 0) s.sp[c][le] = (int16_t)(s.ay[j][le] * W + s.ax[j][le]);
      }
      // 4. TOGGLE_LOAD in index order
      for (int j = 0; j < A; ++j) {
        if (s.act[j][le] != 4) continue;
        const int x = s.ax[j][le], y = s.ay[j][le], cell = y * W + x, c = s.ac[j][le];
        const uint32_t bit = 1u << x, row = s.gnd[y][le];
        if (c < 0) {
          if (row & bit) {
            s.ac[j][le] = s.slot[s.slot_of[cell]][le];
            s.gnd[y][le] = row & ~bit;
          }
        } else if (!(s.hw[y] & bit) && !(row & bit)) {
          s.slot[s.slot_of[cell]][le] = (int16_t)c;
          s.gnd[y][le] = row | bit;
          s.ac[j][le] = -1;
        }
      }
      // 5. deliveries in index order; the request's slot is refilled with a shelf outside the current queue
      int n_del = 0;
      for (int j = 0; j < A; ++j) {
        const int c = s.ac[j][le], x = s.ax[j][le];
        if (c < 0 || s.ay[j][le] != H - 1 || (x != W / 2 - 1 && x != W / 2)) continue;
        int q = -1;
        for (int k = 0; k < R; ++k) q = s.rq[k][le] == c ? k : q;
        if (q < 0) continue;
        ++n_del;
        const Philox4 p = philox4x32_10(g, t, (uint32_t)(j >> 2), RW_QUEUE, a.seed_lo, a.seed_hi);
        s.rq[q][le] = kth_not_in((int)(word_of(p, j & 3) % (uint32_t)(S - R)), &s.rq[0][le], R);
      }
      // 6. team reward, terminal, RecordEpisodeMetrics
      const float rew = (float)n_del;
      s.rew[le] = rew;
      const bool terminated = coll && a.terminate;
      if constexpr (REAL) rn.terminated[e] = terminated ? 1 : 0;
      const EpisodeEnd end = episode_commit(bk, e, run, sc_old, rew, terminated, a.time_limit);
      s.term[le] = end.term ? 1 : 0;
      s.sc[le] = end.step_count;
      reset = end.term;
      build_req(a, s, le, false);
    } else {
      episode_clear(bk, e);
      s.term[le] = 0;
      s.rew[le] = 0.0f;
    }
    // 7. (auto-)reset at this step's counter (REAL: after the pre-reset output pass below)
    if constexpr (!REAL) {
      if (reset) generate(a, s, le, g, t);
    }
  }
  STAMP(2);
  if constexpr (REAL) {
    // the pre-reset observation of every env (equal to the returned one where the step did not end), then the reset
    if (!a.is_reset) {
      __syncthreads();
      build_codes(a, s, ne, tid);
      __syncthreads();
      const int C = (2 * a.sr + 1) * (2 * a.sr + 1);
      write_rows(a, s, rn.view + (long)e0 * A * (A + HEAD + CELL * C), nullptr, ne, tid);
      write_mask(a, s, rn.mask + (long)e0 * A * N_ACT, ne, tid);
      __syncthreads();
    }
    if (tid < ne && (a.is_reset || s.term[tid])) generate(a, s, tid, a.env_offset + (uint32_t)(e0 + tid), t);
  }
  __syncthreads();
  STAMP(3);

  // ---------------------------------------------------------------- reset fill: shelves home (all threads)
  for (int i = tid; i < ne * S; i += THREADS) {
    const int sh = (unsigned)i / (unsigned)ne, le = i - sh * ne;
    if (s.rst[le]) s.sp[sh][le] = (int16_t)s.home[sh];
  }
  for (int i = tid; i < ne * H; i += THREADS) {
    const int y = (unsigned)i / (unsigned)ne, le = i - y * ne;
    if (s.rst[le]) s.gnd[y][le] = ~s.hw[y] & (W == 32 ? 0xFFFFFFFFu : ((1u << W) - 1u));
  }
  __syncthreads();
  STAMP(4);
  build_codes(a, s, ne, tid);
  __syncthreads();
  STAMP(5);

  // ---------------------------------------------------------------- output phase: the workgroup's contiguous ranges
  const int C = (2 * a.sr + 1) * (2 * a.sr + 1);
  const int RAW = HEAD + CELL * C;
  const int rows = ne * A;  // (env, agent) rows of this workgroup
  write_rows(a, s, a.agents_view + (long)e0 * A * (A + RAW), a.global_state + (long)e0 * A * RAW, ne, tid);
  write_mask(a, s, a.action_mask + (long)e0 * A * N_ACT, ne, tid);
  STAMP(6);
  // the advanced state
  const long k0 = (long)e0 * A, ks = (long)e0 * S, kr = (long)e0 * R;
  for (int i = tid; i < rows * 2; i += THREADS) {
    const int k = i >> 1, le = (unsigned)k / (unsigned)A, j = k - le * A;
    a.agent_pos[2 * k0 + i] = (i & 1) ? s.ay[j][le] : s.ax[j][le];
  }
  for (int i = tid; i < ne * S; i += THREADS) {
    const int le = (unsigned)i / (unsigned)S, sh = i - le * S;
    a.shelf_pos[ks + i] = s.sp[sh][le];
  }
  for (int i = tid; i < ne * R; i += THREADS) {
    const int le = (unsigned)i / (unsigned)R, k = i - le * R;
    a.request_queue[kr + i] = s.rq[k][le];
  }
  for (int i = tid; i < rows; i += THREADS) {
    const int le = (unsigned)i / (unsigned)A, j = i - le * A;
    a.agent_dir[k0 + i] = s.ad[j][le];
    a.agent_carry[k0 + i] = s.ac[j][le];
    a.obs_step_count[k0 + i] = s.sc[le];
    a.step_count[k0 + i] = s.sc[le];
    if (!a.is_reset) {
      a.reward[k0 + i] = s.rew[le];
      a.done[k0 + i] = (uint8_t)s.term[le];
    }
  }
  STAMP(7);
#ifdef MAVA_STAMPS
  if (a.stamps != nullptr && blockIdx.x == 0 && tid == 0)
    for (int i = 0; i < 8; ++i) a.stamps[i] += st_acc[i];
#endif
}

__global__ __launch_bounds__(THREADS) void rware_step_kernel(RwArgs a, RwLayout lay) {
  rware_step_body<false>(a, lay, RwReal{});
}

__global__ __launch_bounds__(THREADS) void rware_step_real_kernel(RwArgs a, RwLayout lay, RwReal rn) {
  rware_step_body<true>(a, lay, rn);
}

}  // namespace

static unsigned long long* g_rware_stamps = nullptr;
// Diagnostic hook (not part of include/mava_hip.h): device buffer of 8 u64 for -DMAVA_STAMPS builds.
extern "C" int mava_debug_set_rware_stamps(unsigned long long* p) {
  g_rware_stamps = p;
  return MAVA_OK;
}

extern "C" int mava_rware_step(int E, int A, int S, int R, int H, int W, int sensor_range, int time_limit,
                               int collision_terminates, const uint32_t* highway_rows, const int32_t* shelf_home,
                               uint64_t seed, uint32_t t, const uint32_t* t_base, uint32_t env_offset, int is_reset,
                               int32_t* agent_pos, int32_t* agent_dir, int32_t* agent_carry, int32_t* shelf_pos,
                               int32_t* request_queue, int32_t* step_count, float* run_return, int32_t* run_length,
                               float* ep_return, int32_t* ep_length, float* agents_view, float* global_state,
                               uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                               float* info_return, int32_t* info_length, uint8_t* info_terminal, const int32_t* action,
                               float* real_view, uint8_t* real_mask, uint8_t* terminated, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && A <= MAXA && S >= 2 && S <= MAXS && H >= 2 && H <= MAXH && W >= 2 && W <= MAXW, 0,
                 "mava_rware_step: bad shape E=%d A=%d S=%d H=%d W=%d (1 <= A <= %d, 2 <= S <= %d, H <= %d, W <= %d)", E, A, S,
                 H, W, MAXA, MAXS, MAXH, MAXW);
  MAVA_ARG_CHECK(R >= 1 && R <= MAXR && R < S && sensor_range >= 1 && sensor_range <= MAXSR && time_limit >= 1 &&
                     (collision_terminates == 0 || collision_terminates == 1) && A <= H * W,
                 1, "mava_rware_step: bad scenario request_queue_size=%d (1 .. min(%d, S - 1)) sensor_range=%d (1 .. %d) "
                 "time_limit=%d collision_terminates=%d num_agents=%d", R, MAXR, sensor_range, MAXSR, time_limit,
                 collision_terminates, A);
  MAVA_ARG_CHECK(highway_rows && shelf_home, 2, "mava_rware_step: null layout (highway_rows, shelf_home are host arrays)");
  RwLayout lay;
  for (int y = 0; y < MAXH; ++y) lay.hw[y] = y < H ? highway_rows[y] : 0u;
  for (int i = 0; i < MAXS; ++i) lay.home[i] = 0;
  for (int i = 0; i < S; ++i) {
    const int c = shelf_home[i];
    MAVA_ARG_CHECK(c >= 0 && c < H * W && (i == 0 || c > shelf_home[i - 1]) && !((lay.hw[c / W] >> (c % W)) & 1u), 2,
                   "mava_rware_step: bad layout: shelf_home[%d]=%d must be an increasing non-highway cell of the %dx%d grid", i,
                   c, H, W);
    lay.home[i] = (uint16_t)c;
  }
  MAVA_ARG_CHECK(((lay.hw[H - 1] >> (W / 2 - 1)) & 3u) == 3u, 2, "mava_rware_step: bad layout: the goal cells must be highways");
  const int C = (2 * sensor_range + 1) * (2 * sensor_range + 1);
  MAVA_ARG_CHECK((long)E * A * (A + HEAD + CELL * C) < (1L << 31) && (long)E * S < (1L << 31), 3,
                 "mava_rware_step: E=%d exceeds 32-bit indexing", E);
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(agent_pos && agent_dir && agent_carry && shelf_pos && request_queue && step_count && run_return &&
                     run_length && ep_return && ep_length && agents_view && global_state && action_mask && obs_step_count,
                 4, "mava_rware_step: null state/observation pointer");
  MAVA_ARG_CHECK(is_reset || (reward && done && info_return && info_length && info_terminal), 5,
                 "mava_rware_step: null transition pointer");
  MAVA_ARG_CHECK(is_reset || action, 6, "mava_rware_step: a step needs the (E, A) action array");
  RwArgs a;
  a.E = E; a.A = A; a.S = S; a.R = R; a.H = H; a.W = W; a.sr = sensor_range; a.time_limit = time_limit;
  a.terminate = collision_terminates;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.t = t; a.t_base = t_base; a.env_offset = env_offset;
  a.is_reset = is_reset;
  a.agent_pos = agent_pos; a.agent_dir = agent_dir; a.agent_carry = agent_carry; a.shelf_pos = shelf_pos;
  a.request_queue = request_queue; a.step_count = step_count; a.run_return = run_return; a.run_length = run_length;
  a.ep_return = ep_return; a.ep_length = ep_length; a.agents_view = agents_view; a.global_state = global_state;
  a.action_mask = action_mask; a.obs_step_count = obs_step_count; a.reward = reward; a.done = done;
  a.info_return = info_return; a.info_length = info_length; a.info_terminal = info_terminal; a.action = action;
  a.stamps = g_rware_stamps;
  // all three null: the plain instance; all three given: the REAL instance (which writes none of them on a reset)
  const int n_real = (real_view != nullptr) + (real_mask != nullptr) + (terminated != nullptr);
  MAVA_ARG_CHECK(n_real == 0 || n_real == 3, 7,
                 "mava_rware_step: real_view, real_mask and terminated go together (all three or none)");
  if (n_real == 0) {
    hipLaunchKernelGGL(rware_step_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, lay);
  } else {
    MAVA_ARG_CHECK(is_reset || (real_view != agents_view && real_mask != action_mask), 8,
                   "mava_rware_step: real_view / real_mask must not alias agents_view / action_mask");
    const RwReal rn = {real_view, real_mask, terminated};
    hipLaunchKernelGGL(rware_step_real_kernel, dim3(mava_cdiv(E, NE)), dim3(THREADS), 0, s, a, lay, rn);
  }
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
