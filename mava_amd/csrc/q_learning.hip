// Off-policy pieces of rec_iql (mava/systems/q_learning/rec_iql.py): the device replay buffer (flashbax
// make_trajectory_buffer, :165-175), its window sampler (:425-429), the double-Q TD loss (:325-410) and the target-network
// update (:411-418).  The acting step is mava_rec_q_step_f32 (rec_step.hip); the Q network's sequence forward / backward
// are the recurrent training kernels (rec_dense.hip, rec_gru.hip).
//
// Replay layout: every field is (E, capacity, A, ...) - flashbax's (add_batch, time) - and one launch writes time slot
// `slot` of all E envs.  The flags are stored per agent row, so a sampled block is the scan's `done` input as it is.
// All kernels are element-parallel, bandwidth-bound copies / reductions; every index is checked against the shapes on
// the host before the launch.
#include <cfloat>

#include "common.h"

namespace {

constexpr uint32_t REPLAY_STREAM = 0x5242534Du;  // "RBSM"
constexpr int THREADS = 256;

struct ReplayBuf {
  float* obs;          // (E, cap, A, O)
  uint8_t* mask;       // (E, cap, A, nA)
  int32_t* action;     // (E, cap, A)
  float* reward;       // (E, cap, A)
  uint8_t* terminal;   // (E, cap, A)
  uint8_t* tot;        // (E, cap, A) term_or_trunc
  float* next_obs;     // (E, cap, A, O)
  uint8_t* next_mask;  // (E, cap, A, nA)
};

struct ReplayIn {
  const float* obs;           // (E, A, O)
  const uint8_t* mask;        // (E, A, nA)
  const int32_t* action;      // (E, A)
  const float* reward;        // (E, A)
  const uint8_t* terminal;    // (E) one flag per env
  const uint8_t* tot;         // (E, A)
  const float* next_obs;      // (E, A, O)
  const uint8_t* next_mask;   // (E, A, nA)
};

__global__ __launch_bounds__(THREADS) void replay_add_kernel(ReplayIn in, ReplayBuf b, int E, int A, int O, int nA, int cap,
                                                             int slot) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const long AO = (long)A * O, AN = (long)A * nA;
  if (i < (long)E * AO) {
    const long e = i / AO, r = i - e * AO;
    const long d = (e * cap + slot) * AO + r;
    b.obs[d] = in.obs[i];
    b.next_obs[d] = in.next_obs[i];
  }
  if (i < (long)E * AN) {
    const long e = i / AN, r = i - e * AN;
    const long d = (e * cap + slot) * AN + r;
    b.mask[d] = in.mask[i];
    b.next_mask[d] = in.next_mask[i];
  }
  if (i < (long)E * A) {
    const long e = i / A, j = i - e * A;
    const long d = (e * cap + slot) * A + j;
    b.action[d] = in.action[i];
    b.reward[d] = in.reward[i];
    b.terminal[d] = in.terminal[e];
    b.tot[d] = in.tot[i];
  }
}

struct Window {
  int env, start;  // env row, buffer slot of the window's first step
};

// sample b's (env, start slot): Philox (b, counter, 0, "RBSM"), word x -> env, word y -> window start among the
// n_valid = filled - S + 1 windows of consecutive steps that lie in the filled region without crossing the head
__device__ __forceinline__ Window draw_window(int b, uint32_t counter, uint32_t seed_lo, uint32_t seed_hi, int E, int cap,
                                              uint32_t n_added, int S) {
  const uint32_t filled = n_added < (uint32_t)cap ? n_added : (uint32_t)cap;
  const Philox4 r = philox4x32_10((uint32_t)b, counter, 0u, REPLAY_STREAM, seed_lo, seed_hi);
  Window w;
  w.env = (int)__umulhi(r.x, (uint32_t)E);
  const uint32_t k = __umulhi(r.y, filled - (uint32_t)S + 1u);
  w.start = (int)((n_added - filled + k) % (uint32_t)cap);
  return w;
}

struct SampleOut {
  float* obs;          // (S, Rp, O)
  uint8_t* mask;       // (S, Rp, nA)
  int32_t* action;     // (S, Rp)
  float* reward;       // (S, Rp)
  uint8_t* terminal;   // (S, Rp)
  uint8_t* tot;        // (S, Rp)
  float* next_obs;     // (S, Rp, O)
  uint8_t* next_mask;  // (S, Rp, nA)
  int32_t* pairs;      // (B, 2) (env, start slot)
};

__global__ __launch_bounds__(THREADS) void replay_sample_kernel(ReplayBuf b, SampleOut o, int E, int A, int O, int nA, int cap,
                                                                uint32_t n_added, int B, int S, int Rp, uint32_t counter,
                                                                uint32_t seed_lo, uint32_t seed_hi) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const int BA = B * A;
  // (time step s, output row r, feature f) -> source element of sample r / A, agent r % A
  auto src_row = [&](int s, int r) -> long {  // row (env, slot, agent) of the buffer, -1 for a padding row
    if (r >= BA) return -1;
    const int bb = r / A, j = r - bb * A;
    const Window w = draw_window(bb, counter, seed_lo, seed_hi, E, cap, n_added, S);
    const int slot = (w.start + s) % cap;
    return ((long)w.env * cap + slot) * A + j;
  };
  if (i < (long)S * Rp * O) {
    const long sr = i / O;
    const int f = (int)(i - sr * O), s = (int)(sr / Rp), r = (int)(sr - (long)s * Rp);
    const long q = src_row(s, r);
    o.obs[i] = q < 0 ? 0.0f : b.obs[q * O + f];
    o.next_obs[i] = q < 0 ? 0.0f : b.next_obs[q * O + f];
  }
  if (i < (long)S * Rp * nA) {
    const long sr = i / nA;
    const int f = (int)(i - sr * nA), s = (int)(sr / Rp), r = (int)(sr - (long)s * Rp);
    const long q = src_row(s, r);
    o.mask[i] = q < 0 ? 0 : b.mask[q * nA + f];
    o.next_mask[i] = q < 0 ? 0 : b.next_mask[q * nA + f];
  }
  if (i < (long)S * Rp) {
    const int s = (int)(i / Rp), r = (int)(i - (long)s * Rp);
    const long q = src_row(s, r);
    o.action[i] = q < 0 ? 0 : b.action[q];
    o.reward[i] = q < 0 ? 0.0f : b.reward[q];
    o.terminal[i] = q < 0 ? 0 : b.terminal[q];
    o.tot[i] = q < 0 ? 1 : b.tot[q];  // padding rows: done = 1 (their hidden state stays zero)
  }
  if (i < B) {
    const Window w = draw_window((int)i, counter, seed_lo, seed_hi, E, cap, n_added, S);
    o.pairs[2 * i] = w.env;
    o.pairs[2 * i + 1] = w.start;
  }
}

// T32 element (row, f) of a (rows x N) matrix
__device__ __forceinline__ long t32(long row, int f, int N) { return ((row >> 5) * N + f) * 32 + (row & 31); }

__global__ __launch_bounds__(THREADS) void q_td_loss_kernel(int L, int Rp, int nA, int n_real, const float* __restrict__ q,
                                                            const float* __restrict__ qn, const float* __restrict__ qt,
                                                            const int32_t* __restrict__ action, const float* __restrict__ reward,
                                                            const uint8_t* __restrict__ term_next, const uint8_t* __restrict__ next_mask,
                                                            float gamma, float inv_n, float grad_scale, float* __restrict__ dq,
                                                            float* __restrict__ partials) {
  __shared__ float red[3][THREADS];
  const long rows = (long)L * Rp;
  float s_err = 0.0f, s_q = 0.0f, s_t = 0.0f;
  for (long row = (long)blockIdx.x * THREADS + threadIdx.x; row < rows; row += (long)gridDim.x * THREADS) {
    const int m = (int)(row % Rp);
    if (m >= n_real) {  // padding rows: no loss, no gradient
      for (int o = 0; o < nA; ++o) dq[t32(row, o, nA)] = 0.0f;
      continue;
    }
    // a* = argmax of the masked online next-Q (first index on ties, finfo.min where masked)
    const uint8_t* mk = next_mask + row * nA;
    int as = 0;
    float best = -FLT_MAX;
    for (int o = 0; o < nA; ++o) {
      const float z = mk[o] ? qn[t32(row, o, nA)] : -FLT_MAX;
      if (o == 0 || z > best) { best = z; as = o; }
    }
    const float next_q = qt[t32(row, as, nA)];
    // target = r + (1 - terminal') * gamma * Q_target(next, a*), evaluated in that order (no contraction)
    const float disc = __fmul_rn(1.0f - (float)term_next[row], gamma);
    const float target = __fadd_rn(reward[row], __fmul_rn(disc, next_q));
    const int a = action[row];
    float qa = 0.0f;
    for (int o = 0; o < nA; ++o) {
      const float v = q[t32(row, o, nA)];
      if (o == a) qa = v;
    }
    const float d = qa - target;
    for (int o = 0; o < nA; ++o) dq[t32(row, o, nA)] = o == a ? 2.0f * d * inv_n * grad_scale : 0.0f;
    s_err += d * d;
    s_q += qa;
    s_t += target;
  }
  red[0][threadIdx.x] = s_err;
  red[1][threadIdx.x] = s_q;
  red[2][threadIdx.x] = s_t;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) partials[blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0] * inv_n;
}

__global__ __launch_bounds__(THREADS) void target_update_kernel(long n, const float* __restrict__ online, float* __restrict__ target,
                                                                float tau, int hard) {
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long)gridDim.x * THREADS) {
    const float o = online[i];
    // optax.incremental_update: step_size * new + (1 - step_size) * old
    target[i] = hard ? o : __fadd_rn(__fmul_rn(tau, o), __fmul_rn(1.0f - tau, target[i]));
  }
}

}  // namespace

extern "C" int mava_replay_add_f32(int E, int A, int O, int n_actions, int capacity, int slot, const float* obs,
                                   const uint8_t* action_mask, const int32_t* action, const float* reward,
                                   const uint8_t* terminal, const uint8_t* term_or_trunc, const float* next_obs,
                                   const uint8_t* next_mask, float* b_obs, uint8_t* b_mask, int32_t* b_action,
                                   float* b_reward, uint8_t* b_terminal, uint8_t* b_term_or_trunc, float* b_next_obs,
                                   uint8_t* b_next_mask, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && O >= 1 && n_actions >= 1 && capacity >= 1, 0,
                 "mava_replay_add_f32: bad shape E=%d A=%d O=%d n_actions=%d capacity=%d", E, A, O, n_actions, capacity);
  MAVA_ARG_CHECK(slot >= 0 && slot < capacity, 1, "mava_replay_add_f32: slot %d outside [0, %d)", slot, capacity);
  MAVA_ARG_CHECK((long)E * capacity * A * (O > n_actions ? O : n_actions) < (1L << 40), 2,
                 "mava_replay_add_f32: buffer too large");
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(obs && action_mask && action && reward && terminal && term_or_trunc && next_obs && next_mask, 3,
                 "mava_replay_add_f32: null input pointer");
  MAVA_ARG_CHECK(b_obs && b_mask && b_action && b_reward && b_terminal && b_term_or_trunc && b_next_obs && b_next_mask, 4,
                 "mava_replay_add_f32: null buffer pointer");
  const ReplayIn in = {obs, action_mask, action, reward, terminal, term_or_trunc, next_obs, next_mask};
  const ReplayBuf b = {b_obs, b_mask, b_action, b_reward, b_terminal, b_term_or_trunc, b_next_obs, b_next_mask};
  const long n = (long)E * A * (O > n_actions ? O : n_actions);
  hipLaunchKernelGGL(replay_add_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, in, b, E, A, O,
                     n_actions, capacity, slot);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_replay_sample_f32(int E, int A, int O, int n_actions, int capacity, uint32_t n_added, int B, int S, int Rp,
                                      uint64_t seed, uint32_t counter, const float* b_obs, const uint8_t* b_mask,
                                      const int32_t* b_action, const float* b_reward, const uint8_t* b_terminal,
                                      const uint8_t* b_term_or_trunc, const float* b_next_obs, const uint8_t* b_next_mask,
                                      float* obs, uint8_t* action_mask, int32_t* action, float* reward, uint8_t* terminal,
                                      uint8_t* term_or_trunc, float* next_obs, uint8_t* next_mask, int32_t* pairs,
                                      hipStream_t s) {
  MAVA_ARG_CHECK(E >= 1 && A >= 1 && O >= 1 && n_actions >= 1 && capacity >= 1 && B >= 1 && S >= 1, 0,
                 "mava_replay_sample_f32: bad shape E=%d A=%d O=%d n_actions=%d capacity=%d B=%d S=%d", E, A, O, n_actions,
                 capacity, B, S);
  MAVA_ARG_CHECK(Rp % 32 == 0 && (long)B * A <= Rp, 1, "mava_replay_sample_f32: Rp=%d must be a multiple of 32 holding B*A=%ld rows",
                 Rp, (long)B * A);
  MAVA_ARG_CHECK(S <= capacity && (n_added < (uint32_t)capacity ? n_added : (uint32_t)capacity) >= (uint32_t)S, 2,
                 "mava_replay_sample_f32: %u steps added per env (capacity %d) hold no window of %d steps", n_added, capacity, S);
  MAVA_ARG_CHECK((long)S * Rp * (O > n_actions ? O : n_actions) < (1L << 40), 3, "mava_replay_sample_f32: batch too large");
  MAVA_ARG_CHECK(b_obs && b_mask && b_action && b_reward && b_terminal && b_term_or_trunc && b_next_obs && b_next_mask, 4,
                 "mava_replay_sample_f32: null buffer pointer");
  MAVA_ARG_CHECK(obs && action_mask && action && reward && terminal && term_or_trunc && next_obs && next_mask && pairs, 5,
                 "mava_replay_sample_f32: null output pointer");
  const ReplayBuf b = {const_cast<float*>(b_obs), const_cast<uint8_t*>(b_mask), const_cast<int32_t*>(b_action),
                       const_cast<float*>(b_reward), const_cast<uint8_t*>(b_terminal), const_cast<uint8_t*>(b_term_or_trunc),
                       const_cast<float*>(b_next_obs), const_cast<uint8_t*>(b_next_mask)};
  const SampleOut o = {obs, action_mask, action, reward, terminal, term_or_trunc, next_obs, next_mask, pairs};
  long n = (long)S * Rp * (O > n_actions ? O : n_actions);
  if (n < B) n = B;
  hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, b, o, E, A, O,
                     n_actions, capacity, n_added, B, S, Rp, counter, (uint32_t)seed, (uint32_t)(seed >> 32));
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_q_td_loss_f32(int L, int Rp, int n_actions, int n_real, const float* q, const float* q_next_online,
                                  const float* q_next_target, const int32_t* action, const float* reward,
                                  const uint8_t* terminal_next, const uint8_t* next_mask, float gamma, float grad_scale,
                                  float* dq, float* partials, int nblk, hipStream_t s) {
  MAVA_ARG_CHECK(L >= 1 && Rp >= 32 && Rp % 32 == 0 && n_actions >= 1 && n_actions <= 32, 0,
                 "mava_q_td_loss_f32: bad shape L=%d Rp=%d n_actions=%d (Rp a multiple of 32, 1..32 actions)", L, Rp, n_actions);
  MAVA_ARG_CHECK(n_real >= 1 && n_real <= Rp, 1, "mava_q_td_loss_f32: n_real=%d outside [1, Rp=%d]", n_real, Rp);
  MAVA_ARG_CHECK(nblk >= 1 && nblk <= 4096, 2, "mava_q_td_loss_f32: nblk=%d outside [1, 4096]", nblk);
  MAVA_ARG_CHECK(q && q_next_online && q_next_target && action && reward && terminal_next && next_mask && dq && partials, 3,
                 "mava_q_td_loss_f32: null pointer");
  MAVA_ARG_CHECK(dq != q && dq != q_next_online && dq != q_next_target, 4, "mava_q_td_loss_f32: dq must not alias a Q input");
  const float inv_n = 1.0f / (float)((double)L * n_real);
  hipLaunchKernelGGL(q_td_loss_kernel, dim3(nblk), dim3(THREADS), 0, s, L, Rp, n_actions, n_real, q, q_next_online,
                     q_next_target, action, reward, terminal_next, next_mask, gamma, inv_n, grad_scale, dq, partials);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_target_update_f32(long n, const float* online, float* target, float tau, int hard, hipStream_t s) {
  MAVA_ARG_CHECK(n >= 0 && (hard == 0 || hard == 1), 0, "mava_target_update_f32: bad arguments n=%ld hard=%d", n, hard);
  MAVA_ARG_CHECK(hard || (tau >= 0.0f && tau <= 1.0f), 1, "mava_target_update_f32: tau=%g outside [0, 1]", (double)tau);
  if (n == 0) return MAVA_OK;
  MAVA_ARG_CHECK(online && target && online != target, 2, "mava_target_update_f32: null or aliased pointers");
  long nb = (n + THREADS - 1) / THREADS;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(target_update_kernel, dim3((unsigned)nb), dim3(THREADS), 0, s, n, online, target, tau, hard);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
