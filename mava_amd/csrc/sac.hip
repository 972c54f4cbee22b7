// Soft actor-critic (ff_isac / ff_masac): the kernels around the network products (include/mava_hip.h, "SAC").
// Reference: mava/systems/sac/ff_isac.py:245-384 (step, q_loss_fn, actor_loss_fn, alpha_loss_fn, update_q,
// update_actor_and_alpha), ff_masac.py and mava/utils/centralised_training.py (joint actions), flashbax's item buffer.
// The networks themselves run on the general layer path (mava_amd/generic_networks.py): these kernels produce and consume
// its T32 matrices (element (row, f) of a (rows x N) matrix at ((row / 32) N + f) 32 + row % 32).  Everything else -
// buffer fields, sampled batches, actions, noise - is row-major.  Rows of a batch are b * A + agent; rows from n_real
// on are padding and get zeros.  All kernels are elementwise or one-block-per-slice reductions with a fixed order: the
// same inputs give the same bits.
#include <float.h>

#include "tanh_normal.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_D = 16;                          // action components
constexpr uint32_t STREAM_ITEM = 0x53414342u;      // "SACB": replay item draws
constexpr uint32_t STREAM_NOISE = 0x5341434eu;     // "SACN": reparameterisation noise

__device__ __forceinline__ long t32(long row, int f, int N) { return ((row >> 5) * N + f) * 32 + (row & 31); }

// item k of the ring, oldest first: (n_added - filled + k) mod capacity
__device__ __forceinline__ int item_of(int b, uint32_t counter, uint32_t k0, uint32_t k1, int cap, uint32_t n_added) {
  const uint32_t filled = n_added < (uint32_t)cap ? n_added : (uint32_t)cap;
  const Philox4 r = philox4x32_10((uint32_t)b, counter, 0u, STREAM_ITEM, k0, k1);
  const uint32_t k = (uint32_t)(((uint64_t)r.x * filled) >> 32);
  return (int)(((uint64_t)(n_added - filled) + k) % (uint64_t)cap);
}

struct Item {  // one side of a copy: the acting step's arrays (E items) or the ring (capacity items)
  float* obs;        // (n, A, O)
  float* action;     // (n, A, D)
  float* reward;     // (n, A)
  uint8_t* done;     // (n, A); the acting side has one flag per env, (n)
  float* next_obs;   // (n, A, O)
  float* gs;         // (n, S) or null
  float* next_gs;    // (n, S) or null
};

__global__ __launch_bounds__(THREADS) void sac_add_kernel(Item in, Item b, int E, int A, int O, int D, int S, int cap, int head) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const long AO = (long)A * O, AD = (long)A * D;
  if (i < E * AO) {
    const long e = i / AO, slot = (head + e) % cap, q = slot * AO + (i - e * AO);
    b.obs[q] = in.obs[i];
    b.next_obs[q] = in.next_obs[i];
  }
  if (i < E * AD) {
    const long e = i / AD, slot = (head + e) % cap;
    b.action[slot * AD + (i - e * AD)] = in.action[i];
  }
  if (i < (long)E * A) {
    const long e = i / A, slot = (head + e) % cap, q = slot * A + (i - e * A);
    b.reward[q] = in.reward[i];
    b.done[q] = in.done[e];
  }
  if (S > 0 && i < (long)E * S) {
    const long e = i / S, slot = (head + e) % cap, q = slot * S + (i - e * S);
    b.gs[q] = in.gs[i];
    b.next_gs[q] = in.next_gs[i];
  }
}

__global__ __launch_bounds__(THREADS) void sac_sample_items_kernel(Item b, Item o, int32_t* __restrict__ index, int A, int O, int D, int S,
                                                                   int cap, uint32_t n_added, int B, int Rp, uint32_t counter,
                                                                   uint32_t k0, uint32_t k1) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const int BA = B * A;
  if (i < (long)Rp * O) {
    const int r = (int)(i / O), f = (int)(i - (long)r * O);
    float x = 0.0f, y = 0.0f;
    if (r < BA) {
      const long q = ((long)item_of(r / A, counter, k0, k1, cap, n_added) * A + r % A) * O + f;
      x = b.obs[q];
      y = b.next_obs[q];
    }
    o.obs[i] = x;
    o.next_obs[i] = y;
  }
  if (i < (long)Rp * D) {
    const int r = (int)(i / D), f = (int)(i - (long)r * D);
    o.action[i] = r < BA ? b.action[((long)item_of(r / A, counter, k0, k1, cap, n_added) * A + r % A) * D + f] : 0.0f;
  }
  if (i < Rp) {
    const int r = (int)i;
    const long q = r < BA ? (long)item_of(r / A, counter, k0, k1, cap, n_added) * A + r % A : 0;
    o.reward[i] = r < BA ? b.reward[q] : 0.0f;
    o.done[i] = r < BA ? b.done[q] : 1;
  }
  if (S > 0 && i < (long)B * S) {
    const int bb = (int)(i / S);
    const long q = (long)item_of(bb, counter, k0, k1, cap, n_added) * S + (i - (long)bb * S);
    o.gs[i] = b.gs[q];
    o.next_gs[i] = b.next_gs[q];
  }
  if (i < B) index[i] = item_of((int)i, counter, k0, k1, cap, n_added);
}

// a = tanh(mean + scale eps), logp = sum_d TanhTransformedDistribution.log_prob(a_d)
__global__ __launch_bounds__(THREADS) void sac_sample_kernel(int rows, int n_real, int D, float min_scale, const float* __restrict__ mean,
                                                             const float* __restrict__ log_std, uint32_t k0, uint32_t k1, uint32_t step,
                                                             uint32_t row_offset, float* __restrict__ action, float* __restrict__ logp,
                                                             float* __restrict__ eps_out) {
  const int row = blockIdx.x * THREADS + threadIdx.x;
  if (row >= rows) return;
  float lp = 0.0f;
  for (int d = 0; d < D; ++d) {
    float a = 0.0f, eps = 0.0f;
    if (row < n_real) {
      const float mu = mean[t32(row, d, D)], scale = tn::scale_of(log_std[t32(row, d, D)], min_scale);
      eps = tn::noise(row_offset + (uint32_t)row, step, d, STREAM_NOISE, k0, k1);
      a = tanhf(mu + scale * eps);
      lp += tn::log_prob(a, mu, scale).lp;
    }
    action[(long)row * D + d] = a;
    if (eps_out != nullptr) eps_out[(long)row * D + d] = eps;
  }
  if (logp != nullptr) logp[row] = lp;
}

// x = [state row | action block] as a T32 matrix of x_ld >= O + W features per tile (zeros past O + W).  joint 0: W = D,
// the row's own action.  joint 1: W = A D, every agent's action of the row's item, the row's own slot taken from
// action_new when given.
__global__ __launch_bounds__(THREADS) void sac_concat_kernel(int rows, int n_real, int O, int x_share, int A, int D, int joint,
                                                             const float* __restrict__ state, const float* __restrict__ action,
                                                             const float* __restrict__ action_new, float* __restrict__ x, int x_ld) {
  const int K = O + (joint ? A * D : D);
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (long)rows * x_ld) return;
  // (consecutive threads take consecutive rows of one feature: the T32 writes are contiguous)
  const long tile = i / (32L * x_ld);
  const int rem = (int)(i - tile * 32L * x_ld), f = rem >> 5, row = (int)(tile * 32 + (rem & 31));
  float v = 0.0f;
  if (row < n_real && f < K) {
    if (f < O) {
      v = state[(long)(row / x_share) * O + f];
    } else if (!joint) {
      v = (action_new != nullptr ? action_new : action)[(long)row * D + (f - O)];
    } else {
      const int j = (f - O) / D, d = (f - O) - j * D, item = row / A;
      v = (j == row % A && action_new != nullptr) ? action_new[(long)row * D + d] : action[((long)item * A + j) * D + d];
    }
  }
  x[i] = v;
}

// update_q: the target, both Q gradients and the loss partials [q1_loss, q2_loss, mean q1, mean q2]
__global__ __launch_bounds__(THREADS) void sac_q_loss_kernel(int rows, int n_real, int A, const float* __restrict__ q1,
                                                             const float* __restrict__ q2, const float* __restrict__ q1_t,
                                                             const float* __restrict__ q2_t, const float* __restrict__ logp_next,
                                                             const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                             const float* __restrict__ log_alpha, float gamma, float inv_n,
                                                             float grad_scale, float* __restrict__ dq1, float* __restrict__ dq2,
                                                             float* __restrict__ target_out, float* __restrict__ partials) {
  __shared__ float red[4][THREADS];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int row = blockIdx.x * THREADS + threadIdx.x; row < rows; row += gridDim.x * THREADS) {
    float g1 = 0.0f, g2 = 0.0f, target = 0.0f;
    if (row < n_real) {
      const float alpha = expf(log_alpha[row % A]);
      const float next_q = fminf(q1_t[row], q2_t[row]) - alpha * logp_next[row];
      target = reward[row] + (1.0f - (float)done[row]) * gamma * next_q;
      const float e1 = q1[row] - target, e2 = q2[row] - target;
      g1 = 2.0f * e1 * inv_n * grad_scale;
      g2 = 2.0f * e2 * inv_n * grad_scale;
      s[0] += e1 * e1; s[1] += e2 * e2; s[2] += q1[row]; s[3] += q2[row];
    }
    dq1[row] = g1;
    dq2[row] = g2;
    if (target_out != nullptr) target_out[row] = target;
  }
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 4) partials[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0] * inv_n;
}

// actor_loss_fn differentiated through the sample: d mean, d raw log_std and the loss partials [actor loss, mean logp]
__global__ __launch_bounds__(THREADS) void sac_actor_grad_kernel(int rows, int n_real, int A, int D, float min_scale,
                                                                 const float* __restrict__ mean, const float* __restrict__ log_std,
                                                                 const float* __restrict__ eps, const float* __restrict__ action,
                                                                 const float* __restrict__ log_alpha, const float* __restrict__ q1,
                                                                 const float* __restrict__ q2, const float* __restrict__ dx1,
                                                                 const float* __restrict__ dx2, int K, int a_off, int joint,
                                                                 float inv_q_scale, float inv_n, float grad_scale,
                                                                 float* __restrict__ dmean, float* __restrict__ dlog_std,
                                                                 float* __restrict__ partials) {
  __shared__ float red[2][THREADS];
  float s_loss = 0.0f, s_lp = 0.0f;
  for (int row = blockIdx.x * THREADS + threadIdx.x; row < rows; row += gridDim.x * THREADS) {
    if (row >= n_real) {
      for (int d = 0; d < D; ++d) { dmean[t32(row, d, D)] = 0.0f; dlog_std[t32(row, d, D)] = 0.0f; }
      continue;
    }
    const float alpha = expf(log_alpha[row % A]);
    const bool first = q1[row] <= q2[row];  // min(q1, q2): the gradient goes to the smaller one
    const float* dx = first ? dx1 : dx2;
    const int off = a_off + (joint ? (row % A) * D : 0);
    float lp = 0.0f;
    for (int d = 0; d < D; ++d) {
      const float mu = mean[t32(row, d, D)], raw = log_std[t32(row, d, D)], scale = tn::scale_of(raw, min_scale);
      const float a = action[(long)row * D + d], e = eps[(long)row * D + d];
      const tn::LogProb o = tn::log_prob(a, mu, scale);
      lp += o.lp;
      float lm, ls;  // d logp / d mean, d logp / d scale along the sample
      if (a <= -tn::THRESH || a >= tn::THRESH) {
        lm = o.dmean; ls = o.dscale;  // the tail mass: nothing flows through the clipped action
      } else {
        lm = 2.0f * a; ls = -1.0f / scale + 2.0f * a * e;
      }
      const float dq_da = dx[t32(row, off + d, K)] * inv_q_scale * (1.0f - a * a);  // d Q / d x
      const float gm = alpha * lm - dq_da, gs = alpha * ls - dq_da * e;
      dmean[t32(row, d, D)] = gm * inv_n * grad_scale;
      dlog_std[t32(row, d, D)] = gs * tn::sigmoid(raw) * inv_n * grad_scale;
    }
    s_loss += alpha * lp - fminf(q1[row], q2[row]);
    s_lp += lp;
  }
  red[0][threadIdx.x] = s_loss;
  red[1][threadIdx.x] = s_lp;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { red[0][threadIdx.x] += red[0][threadIdx.x + w]; red[1][threadIdx.x] += red[1][threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x < 2) partials[blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0] * inv_n;
}

// alpha_loss_fn: block a owns agent a.  grad[a] = d loss / d log_alpha_a, loss_parts[a] = agent a's share of the loss
__global__ __launch_bounds__(THREADS) void sac_alpha_kernel(int n_real, int A, const float* __restrict__ logp,
                                                            const float* __restrict__ log_alpha, float target_entropy, float inv_n,
                                                            float* __restrict__ grad, float* __restrict__ loss_parts) {
  __shared__ float red[THREADS];
  const int a = blockIdx.x;
  float s = 0.0f;
  for (int b = threadIdx.x; b * A + a < n_real; b += THREADS) s += logp[b * A + a] + target_entropy;
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = -expf(log_alpha[a]) * red[0] * inv_n;  // d/d log_alpha of -exp(log_alpha) x is itself
    grad[a] = v;
    loss_parts[a] = v;
  }
}

inline unsigned blocks_for(long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int mava_sac_replay_add_f32(int E, int A, int O, int D, int S, int capacity, int head, const float* obs,
                                       const float* action, const float* reward, const uint8_t* done, const float* next_obs,
                                       const float* gs, const float* next_gs, float* b_obs, float* b_action, float* b_reward,
                                       uint8_t* b_done, float* b_next_obs, float* b_gs, float* b_next_gs, hipStream_t s) {
  MAVA_ARG_CHECK(E >= 0 && A >= 1 && O >= 1 && D >= 1 && D <= MAX_D && S >= 0 && capacity >= 1, 0,
                 "mava_sac_replay_add_f32: bad shape E=%d A=%d O=%d D=%d S=%d capacity=%d", E, A, O, D, S, capacity);
  MAVA_ARG_CHECK(head >= 0 && head < capacity && E <= capacity, 1, "mava_sac_replay_add_f32: head %d / E=%d outside capacity %d",
                 head, E, capacity);
  MAVA_ARG_CHECK((long)capacity * A * (O > D ? O : D) < (1L << 40) && (long)capacity * S < (1L << 40), 2,
                 "mava_sac_replay_add_f32: buffer too large");
  if (E == 0) return MAVA_OK;
  MAVA_ARG_CHECK(obs && action && reward && done && next_obs && b_obs && b_action && b_reward && b_done && b_next_obs, 3,
                 "mava_sac_replay_add_f32: null pointer");
  MAVA_ARG_CHECK(S == 0 || (gs && next_gs && b_gs && b_next_gs), 4, "mava_sac_replay_add_f32: S=%d needs the global-state arrays", S);
  const Item in = {const_cast<float*>(obs), const_cast<float*>(action), const_cast<float*>(reward), const_cast<uint8_t*>(done),
                   const_cast<float*>(next_obs), const_cast<float*>(gs), const_cast<float*>(next_gs)};
  const Item b = {b_obs, b_action, b_reward, b_done, b_next_obs, b_gs, b_next_gs};
  long n = (long)E * A * (O > D ? O : D);
  if (n < (long)E * S) n = (long)E * S;
  hipLaunchKernelGGL(sac_add_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, s, in, b, E, A, O, D, S, capacity, head);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_replay_sample_f32(int A, int O, int D, int S, int capacity, uint32_t n_added, int B, int Rp, uint64_t seed,
                                          uint32_t counter, const float* b_obs, const float* b_action, const float* b_reward,
                                          const uint8_t* b_done, const float* b_next_obs, const float* b_gs, const float* b_next_gs,
                                          float* obs, float* action, float* reward, uint8_t* done, float* next_obs, float* gs,
                                          float* next_gs, int32_t* index, hipStream_t s) {
  MAVA_ARG_CHECK(A >= 1 && O >= 1 && D >= 1 && D <= MAX_D && S >= 0 && capacity >= 1 && B >= 1, 0,
                 "mava_sac_replay_sample_f32: bad shape A=%d O=%d D=%d S=%d capacity=%d B=%d", A, O, D, S, capacity, B);
  MAVA_ARG_CHECK(Rp % 32 == 0 && (long)B * A <= Rp, 1, "mava_sac_replay_sample_f32: Rp=%d must be a multiple of 32 holding B*A=%ld rows",
                 Rp, (long)B * A);
  MAVA_ARG_CHECK(n_added >= 1, 2, "mava_sac_replay_sample_f32: the buffer is empty");
  MAVA_ARG_CHECK((long)Rp * (O > D ? O : D) < (1L << 31) && (long)B * S < (1L << 31), 3, "mava_sac_replay_sample_f32: batch too large");
  MAVA_ARG_CHECK(b_obs && b_action && b_reward && b_done && b_next_obs && obs && action && reward && done && next_obs && index, 4,
                 "mava_sac_replay_sample_f32: null pointer");
  MAVA_ARG_CHECK(S == 0 || (b_gs && b_next_gs && gs && next_gs), 5, "mava_sac_replay_sample_f32: S=%d needs the global-state arrays", S);
  const Item b = {const_cast<float*>(b_obs), const_cast<float*>(b_action), const_cast<float*>(b_reward), const_cast<uint8_t*>(b_done),
                  const_cast<float*>(b_next_obs), const_cast<float*>(b_gs), const_cast<float*>(b_next_gs)};
  const Item o = {obs, action, reward, done, next_obs, gs, next_gs};
  long n = (long)Rp * (O > D ? O : D);
  if (n < (long)B * S) n = (long)B * S;
  hipLaunchKernelGGL(sac_sample_items_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, s, b, o, index, A, O, D, S, capacity, n_added, B,
                     Rp, counter, (uint32_t)seed, (uint32_t)(seed >> 32));
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_sample_f32(int rows, int n_real, int action_dim, float min_scale, const float* mean, const float* log_std,
                                   uint64_t seed, uint32_t step, uint32_t row_offset, float* action, float* log_prob, float* eps,
                                   hipStream_t s) {
  MAVA_ARG_CHECK(rows >= 32 && rows % 32 == 0 && n_real >= 0 && n_real <= rows && action_dim >= 1 && action_dim <= MAX_D, 0,
                 "mava_sac_sample_f32: bad shape rows=%d n_real=%d action_dim=%d (rows a multiple of 32, 1..%d components)", rows,
                 n_real, action_dim, MAX_D);
  MAVA_ARG_CHECK(min_scale >= 0.0f, 1, "mava_sac_sample_f32: min_scale=%g is negative", (double)min_scale);
  MAVA_ARG_CHECK(mean && log_std && action, 2, "mava_sac_sample_f32: null pointer");
  hipLaunchKernelGGL(sac_sample_kernel, dim3(blocks_for(rows)), dim3(THREADS), 0, s, rows, n_real, action_dim, min_scale, mean, log_std,
                     (uint32_t)seed, (uint32_t)(seed >> 32), step, row_offset, action, log_prob, eps);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_concat_f32(int rows, int n_real, int O, int x_share, int A, int action_dim, int joint, const float* state,
                                   const float* action, const float* action_new, float* x, int x_ld, hipStream_t s) {
  MAVA_ARG_CHECK(rows >= 32 && rows % 32 == 0 && n_real >= 0 && n_real <= rows && O >= 1 && A >= 1 && action_dim >= 1 &&
                     action_dim <= MAX_D && x_share >= 1,
                 0, "mava_sac_concat_f32: bad shape rows=%d n_real=%d O=%d x_share=%d A=%d action_dim=%d", rows, n_real, O, x_share, A,
                 action_dim);
  MAVA_ARG_CHECK(!joint || n_real % A == 0, 1, "mava_sac_concat_f32: joint actions need whole items (n_real=%d, A=%d)", n_real, A);
  MAVA_ARG_CHECK(x_ld >= O + (joint ? A : 1) * action_dim && (long)rows * x_ld < (1L << 31), 2,
                 "mava_sac_concat_f32: x_ld=%d is below the %d features of a row, or the matrix is too large", x_ld,
                 O + (joint ? A : 1) * action_dim);
  MAVA_ARG_CHECK(state && action && x, 3, "mava_sac_concat_f32: null pointer");
  hipLaunchKernelGGL(sac_concat_kernel, dim3(blocks_for((long)rows * x_ld)), dim3(THREADS), 0, s, rows, n_real, O, x_share, A,
                     action_dim, joint ? 1 : 0, state, action, action_new, x, x_ld);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_q_loss_f32(int rows, int n_real, int A, const float* q1, const float* q2, const float* q1_target,
                                   const float* q2_target, const float* log_prob_next, const float* reward, const uint8_t* done,
                                   const float* log_alpha, float gamma, float grad_scale, float* dq1, float* dq2, float* target,
                                   float* partials, int nblk, hipStream_t s) {
  MAVA_ARG_CHECK(rows >= 32 && rows % 32 == 0 && n_real >= 1 && n_real <= rows && A >= 1, 0,
                 "mava_sac_q_loss_f32: bad shape rows=%d n_real=%d A=%d", rows, n_real, A);
  MAVA_ARG_CHECK(nblk >= 1 && nblk <= 4096, 1, "mava_sac_q_loss_f32: nblk=%d outside [1, 4096]", nblk);
  MAVA_ARG_CHECK(q1 && q2 && q1_target && q2_target && log_prob_next && reward && done && log_alpha && dq1 && dq2 && partials, 2,
                 "mava_sac_q_loss_f32: null pointer");
  MAVA_ARG_CHECK(dq1 != q1 && dq2 != q2 && dq1 != dq2, 3, "mava_sac_q_loss_f32: dq1 / dq2 must not alias q1 / q2 or each other");
  hipLaunchKernelGGL(sac_q_loss_kernel, dim3(nblk), dim3(THREADS), 0, s, rows, n_real, A, q1, q2, q1_target, q2_target, log_prob_next,
                     reward, done, log_alpha, gamma, 1.0f / (float)n_real, grad_scale, dq1, dq2, target, partials);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_actor_grad_f32(int rows, int n_real, int A, int action_dim, float min_scale, const float* mean,
                                       const float* log_std, const float* eps, const float* action, const float* log_alpha,
                                       const float* q1, const float* q2, const float* dx1, const float* dx2, int K, int action_offset,
                                       int joint, float q_scale, float grad_scale, float* dmean, float* dlog_std, float* partials,
                                       int nblk, hipStream_t s) {
  MAVA_ARG_CHECK(rows >= 32 && rows % 32 == 0 && n_real >= 1 && n_real <= rows && A >= 1 && action_dim >= 1 && action_dim <= MAX_D, 0,
                 "mava_sac_actor_grad_f32: bad shape rows=%d n_real=%d A=%d action_dim=%d", rows, n_real, A, action_dim);
  MAVA_ARG_CHECK(action_offset >= 0 && action_offset + (joint ? A : 1) * action_dim <= K, 1,
                 "mava_sac_actor_grad_f32: the action slice [%d, +%d) leaves the K=%d input features", action_offset,
                 (joint ? A : 1) * action_dim, K);
  MAVA_ARG_CHECK(nblk >= 1 && nblk <= 4096 && q_scale > 0.0f, 2, "mava_sac_actor_grad_f32: nblk=%d outside [1, 4096] or q_scale=%g <= 0",
                 nblk, (double)q_scale);
  MAVA_ARG_CHECK(mean && log_std && eps && action && log_alpha && q1 && q2 && dx1 && dx2 && dmean && dlog_std && partials, 3,
                 "mava_sac_actor_grad_f32: null pointer");
  MAVA_ARG_CHECK(dmean != mean && dlog_std != log_std && dmean != dlog_std, 4, "mava_sac_actor_grad_f32: outputs must not alias inputs");
  hipLaunchKernelGGL(sac_actor_grad_kernel, dim3(nblk), dim3(THREADS), 0, s, rows, n_real, A, action_dim, min_scale, mean, log_std, eps,
                     action, log_alpha, q1, q2, dx1, dx2, K, action_offset, joint ? 1 : 0, 1.0f / q_scale, 1.0f / (float)n_real,
                     grad_scale, dmean, dlog_std, partials);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_alpha_loss_f32(int n_real, int A, const float* log_prob, const float* log_alpha, float target_entropy,
                                       float* grad, float* loss_parts, hipStream_t s) {
  MAVA_ARG_CHECK(n_real >= 1 && A >= 1 && A <= 1024 && n_real % A == 0, 0, "mava_sac_alpha_loss_f32: bad shape n_real=%d A=%d", n_real, A);
  MAVA_ARG_CHECK(log_prob && log_alpha && grad && loss_parts, 1, "mava_sac_alpha_loss_f32: null pointer");
  hipLaunchKernelGGL(sac_alpha_kernel, dim3(A), dim3(THREADS), 0, s, n_real, A, log_prob, log_alpha, target_entropy,
                     1.0f / (float)n_real, grad, loss_parts);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
