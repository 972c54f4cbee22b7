// Value decomposition on top of rec_iql's per-agent Q (rec_qmix / rec_vdn, mava/systems/q_learning/rec_qmix.py): the
// mixer's state matrices and the TD loss through the mixer.  The Q network's three passes, the hypernetworks (general
// layer path, generic_layers.hip + rec_dense.hip), clip + Adam and the target update are existing launches.
//
// Rows.  Agent rows are t * Rp + b * A + j as in q_learning.hip (Rp a multiple of 32 holding B * A rows).  A MIXER row is
// (t, b) = t * Bp + b with Bp = ceil32(B); rows with b >= B are padding.  Every matrix here is T32: 32 consecutive rows of
// one feature are 128 contiguous bytes.
//
// Lane mapping of the TD kernel: a block owns 64 consecutive mixer rows (two tiles) at a time; lane l of every wave is row l
// of them, so each load / store instruction of a wave touches two 128-byte segments.  The four waves split the features:
// wave g takes the agents j = g, g + 4, .. in the select / argmax and dq phases and the embedding columns k = g, g + 4, ..
// in the mixer's forward and backward passes (one lane per row alone leaves a chain of A * Em dependent memory round trips:
// measured 145 us per launch whatever the batch).  The agent-row accesses stride by A rows between
// lanes, which stays inside A adjacent segments.
//
// Determinism: the split is fixed (it does not depend on the grid), every partial sum goes through LDS and is added in wave
// order by every lane that needs it, so the gradients are bit-identical for any block count; the metric partial sums are
// reduced by a fixed LDS tree and written per block (no atomics).
#include <cfloat>

#include "common.h"

namespace {

constexpr int ROWS = 64;             // mixer rows per block step = lanes of a wave
constexpr int KG = 4;                // waves: feature groups
constexpr int THREADS = ROWS * KG;
constexpr int MAX_A = 16;
constexpr int MAX_EM = 64;

// T32 element (row, f) of a (rows x N) matrix
__device__ __forceinline__ long t32(long row, int f, int N) { return ((row >> 5) * N + f) * 32 + (row & 31); }

__global__ __launch_bounds__(256) void qmix_state_kernel(int L, int B, int Bp, int A, int O, int Rp, int KP,
                                                         const float* __restrict__ obs, const float* __restrict__ next_obs,
                                                         float* __restrict__ state, float* __restrict__ next_state) {
  const int Ds = A * O;
  const long n = (long)L * Bp * KP;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long tile = i / ((long)KP * 32);
    const int in_tile = (int)(i - tile * KP * 32);
    const int f = in_tile >> 5;
    const long row = tile * 32 + (in_tile & 31);
    const int t = (int)(row / Bp), b = (int)(row - (long)t * Bp);
    float s = 0.0f, ns = 0.0f;
    if (b < B && f < Ds) {  // the A agent rows of sample b are contiguous: feature j * O + f' is element f of that block
      const long src = ((long)t * Rp + (long)b * A) * O + f;
      s = obs[src];
      ns = next_obs[src];
    }
    state[i] = s;
    next_state[i] = ns;
  }
}

struct QmixTd {
  int qmix, L, B, Bp, A, Rp, nA, Em;
  const float *q, *qn, *qt;
  const int32_t* action;
  const float* reward;
  const uint8_t *term_next, *next_mask;
  const float *w1, *b1, *w2, *b2;      // online hypernet outputs, pre-abs
  const float *w1t, *b1t, *w2t, *b2t;  // target hypernet outputs, pre-abs
  float gamma, inv_n, grad_scale;
  float *dq, *d_w1, *d_b1, *d_w2, *d_b2, *partials;
};

__device__ __forceinline__ float sgn(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : expm1f(x); }

// pre-activation k of the mixing layer: sum_j qa_j |w1[j, k]| + b1[k].  This sum and the ones over k run in f64: Q_tot - y
// cancels, and f32 sums alone use up the 1e-6 the gradients are held to against the float64 model (measured 9.9e-7); the
// elu and every stored value stay f32.
__device__ __forceinline__ float mix_pre(const float* __restrict__ w1, const float* __restrict__ b1, const float (*qa)[ROWS], int lane,
                                         long row, int k, int A, int Em) {
  double pre = 0.0;
  for (int j = 0; j < A; ++j) pre += (double)qa[j][lane] * (double)fabsf(w1[t32(row, j * Em + k, A * Em)]);
  return (float)(pre + (double)b1[t32(row, k, Em)]);
}

__global__ __launch_bounds__(THREADS) void qmix_td_kernel(QmixTd a) {
  __shared__ float s_qa[MAX_A][ROWS];        // chosen online Q per agent
  __shared__ float s_qx[MAX_A][ROWS];        // target Q at the online argmax per agent
  __shared__ float s_rw[MAX_A][ROWS];        // reward per agent
  __shared__ double s_tot[2][KG][ROWS];      // per-wave partial sums of Q_tot (online, target)
  __shared__ double s_dqa[KG][MAX_A][ROWS];  // per-wave partial sums of dLoss / d qa_j
  __shared__ float red[3][THREADS];
  const int tid = threadIdx.x, lane = tid & (ROWS - 1), grp = tid / ROWS;
  const int A = a.A, nA = a.nA, Em = a.Em, AE = a.A * a.Em;
  const long rows = (long)a.L * a.Bp;
  float s_err = 0.0f, s_q = 0.0f, s_t = 0.0f;
  for (long row0 = (long)blockIdx.x * ROWS; row0 < rows; row0 += (long)gridDim.x * ROWS) {
    const long row = row0 + lane;
    const bool in = row < rows;  // (rows is a multiple of 32, not of 64)
    const int t = (int)(row / a.Bp), b = (int)(row - (long)t * a.Bp);
    const bool real = in && b < a.B;
    // ---- select and argmax: wave grp takes the agents grp, grp + KG, ..
    for (int j = grp; j < A; j += KG) {
      if (!real) continue;
      const long arow = (long)t * a.Rp + (long)b * A + j;
      // a* = argmax of the masked online next-Q (first index on ties, -FLT_MAX where masked)
      const uint8_t* mk = a.next_mask + arow * nA;
      int as = 0;
      float best = -FLT_MAX;
      for (int o = 0; o < nA; ++o) {
        const float z = mk[o] ? a.qn[t32(arow, o, nA)] : -FLT_MAX;
        if (o == 0 || z > best) { best = z; as = o; }
      }
      const int act = a.action[arow];
      float qa = 0.0f;
      for (int o = 0; o < nA; ++o) {
        const float v = a.q[t32(arow, o, nA)];
        if (o == act) qa = v;
      }
      s_qa[j][lane] = qa;
      s_qx[j][lane] = a.qt[t32(arow, as, nA)];
      s_rw[j][lane] = a.reward[arow];
    }
    __syncthreads();
    // ---- both mixer forwards: wave grp takes the columns grp, grp + KG, ..
    if (a.qmix) {
      double tot = 0.0, tot_t = 0.0;
      if (real) {
#pragma unroll 2
        for (int k = grp; k < Em; k += KG) {
          tot += (double)elu(mix_pre(a.w1, a.b1, s_qa, lane, row, k, A, Em)) * (double)fabsf(a.w2[t32(row, k, Em)]);
          tot_t += (double)elu(mix_pre(a.w1t, a.b1t, s_qx, lane, row, k, A, Em)) * (double)fabsf(a.w2t[t32(row, k, Em)]);
        }
      }
      s_tot[0][grp][lane] = tot;
      s_tot[1][grp][lane] = tot_t;
      __syncthreads();
    }
    // ---- the TD error (every wave computes its rows' g in the same order)
    float g = 0.0f;
    if (real) {
      double q_tot = 0.0, q_tot_t = 0.0;
      float r_sum = 0.0f;
      for (int j = 0; j < A; ++j) r_sum += s_rw[j][lane];
      if (a.qmix) {
        for (int w = 0; w < KG; ++w) {
          q_tot += s_tot[0][w][lane];
          q_tot_t += s_tot[1][w][lane];
        }
        q_tot += (double)a.b2[t32(row, 0, 1)];
        q_tot_t += (double)a.b2t[t32(row, 0, 1)];
      } else {
        for (int j = 0; j < A; ++j) {
          q_tot += (double)s_qa[j][lane];
          q_tot_t += (double)s_qx[j][lane];
        }
      }
      // y = r + (1 - terminal') * gamma * Q_tot_target, evaluated in that order (no contraction); agent 0's flag
      const float r = r_sum / (float)A;
      const float disc = __fmul_rn(1.0f - (float)a.term_next[(long)t * a.Rp + (long)b * A], a.gamma);
      const float y = __fadd_rn(r, __fmul_rn(disc, (float)q_tot_t));
      const float d = (float)(q_tot - (double)y);
      g = 2.0f * d * a.inv_n * a.grad_scale;
      if (grp == 0) {
        s_err += d * d;
        s_q += (float)q_tot;
        s_t += y;
      }
    }
    // ---- backward through the online mixer (padding rows: the row's gradients are exact zeros)
    if (a.qmix) {
      for (int j = 0; j < A; ++j) s_dqa[grp][j][lane] = 0.0;
      if (in) {
        if (grp == 0) a.d_b2[t32(row, 0, 1)] = g;
#pragma unroll 2
        for (int k = grp; k < Em; k += KG) {
          float d_w2 = 0.0f, d_pre = 0.0f;
          if (real) {
            const float pre = mix_pre(a.w1, a.b1, s_qa, lane, row, k, A, Em);
            const float w2r = a.w2[t32(row, k, Em)];
            d_w2 = g * elu(pre) * sgn(w2r);
            d_pre = g * fabsf(w2r) * (pre > 0.0f ? 1.0f : expf(pre));  // elu' = exp(x) for x <= 0
          }
          a.d_w2[t32(row, k, Em)] = d_w2;
          a.d_b1[t32(row, k, Em)] = d_pre;
          for (int j = 0; j < A; ++j) {
            float d_w1 = 0.0f;
            if (real) {
              const float w = a.w1[t32(row, j * Em + k, AE)];
              d_w1 = d_pre * s_qa[j][lane] * sgn(w);
              s_dqa[grp][j][lane] += (double)d_pre * (double)fabsf(w);
            }
            a.d_w1[t32(row, j * Em + k, AE)] = d_w1;
          }
        }
      }
      __syncthreads();
    }
    // ---- dq: every element of these mixer rows' agent rows; wave grp takes the agents grp, grp + KG, ..
    if (in) {
      for (int j = grp; j < A; j += KG) {
        const long m = (long)b * A + j;
        if (m >= a.Rp) break;  // (Bp * A may exceed Rp: those agent rows do not exist)
        const long arow = (long)t * a.Rp + m;
        const int act = real ? a.action[arow] : -1;
        float dqa = 0.0f;
        if (real) {
          if (a.qmix) {
            double sum = 0.0;
            for (int w = 0; w < KG; ++w) sum += s_dqa[w][j][lane];
            dqa = (float)sum;
          } else {
            dqa = g;
          }
        }
        for (int o = 0; o < nA; ++o) a.dq[t32(arow, o, nA)] = o == act ? dqa : 0.0f;
      }
    }
    __syncthreads();  // the LDS rows are rewritten by the next step
  }
  red[0][tid] = s_err;
  red[1][tid] = s_q;
  red[2][tid] = s_t;
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (tid < w)
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + w];
    __syncthreads();
  }
  if (tid < 3) a.partials[blockIdx.x * 3 + tid] = red[tid][0] * a.inv_n;
}

}  // namespace

extern "C" int mava_qmix_state_t32_f32(int L, int B, int A, int O, int Rp, int k_pad, const float* obs, const float* next_obs,
                                       float* state, float* next_state, hipStream_t s) {
  MAVA_ARG_CHECK(L >= 1 && B >= 1 && A >= 1 && O >= 1, 0, "mava_qmix_state_t32_f32: bad shape L=%d B=%d A=%d O=%d", L, B, A, O);
  MAVA_ARG_CHECK(Rp >= 32 && Rp % 32 == 0 && (long)B * A <= Rp, 1,
                 "mava_qmix_state_t32_f32: Rp=%d must be a multiple of 32 holding B*A=%ld rows", Rp, (long)B * A);
  MAVA_ARG_CHECK((long)A * O <= k_pad && k_pad <= (1 << 20), 2, "mava_qmix_state_t32_f32: k_pad=%d must hold A*O=%ld features", k_pad,
                 (long)A * O);
  const int Bp = (B + 31) / 32 * 32;
  MAVA_ARG_CHECK((long)L * Bp * k_pad < (1L << 40) && (long)L * Rp * O < (1L << 40), 3, "mava_qmix_state_t32_f32: batch too large");
  MAVA_ARG_CHECK(obs && next_obs && state && next_state, 4, "mava_qmix_state_t32_f32: null pointer");
  MAVA_ARG_CHECK(state != next_state && state != obs && state != next_obs && next_state != obs && next_state != next_obs, 5,
                 "mava_qmix_state_t32_f32: outputs must not alias each other or an input");
  const long n = (long)L * Bp * k_pad;
  long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(qmix_state_kernel, dim3((unsigned)nb), dim3(256), 0, s, L, B, Bp, A, O, Rp, k_pad, obs, next_obs, state,
                     next_state);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_qmix_td_f32(int mode, int L, int B, int A, int Rp, int n_actions, int Em, const float* q,
                                const float* q_next_online, const float* q_next_target, const int32_t* action, const float* reward,
                                const uint8_t* terminal_next, const uint8_t* next_mask, const float* w1, const float* b1,
                                const float* w2, const float* b2, const float* w1_target, const float* b1_target,
                                const float* w2_target, const float* b2_target, float gamma, float grad_scale, float* dq,
                                float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* partials, int nblk, hipStream_t s) {
  MAVA_ARG_CHECK(mode == 0 || mode == 1, 0, "mava_qmix_td_f32: mode=%d (0 = vdn, 1 = qmix)", mode);
  MAVA_ARG_CHECK(L >= 1 && B >= 1 && A >= 1 && A <= MAX_A && n_actions >= 1 && n_actions <= 32, 1,
                 "mava_qmix_td_f32: bad shape L=%d B=%d A=%d n_actions=%d (1..16 agents, 1..32 actions)", L, B, A, n_actions);
  MAVA_ARG_CHECK(mode == 0 || (Em >= 1 && Em <= MAX_EM), 2, "mava_qmix_td_f32: Em=%d outside [1, 64]", Em);
  MAVA_ARG_CHECK(Rp >= 32 && Rp % 32 == 0 && (long)B * A <= Rp, 3,
                 "mava_qmix_td_f32: Rp=%d must be a multiple of 32 holding B*A=%ld rows", Rp, (long)B * A);
  MAVA_ARG_CHECK(nblk >= 1 && nblk <= 4096, 4, "mava_qmix_td_f32: nblk=%d outside [1, 4096]", nblk);
  MAVA_ARG_CHECK((long)L * Rp * n_actions < (1L << 40) && (long)L * (B + 31) * A * MAX_EM < (1L << 40), 5,
                 "mava_qmix_td_f32: batch too large");
  MAVA_ARG_CHECK(q && q_next_online && q_next_target && action && reward && terminal_next && next_mask && dq && partials, 6,
                 "mava_qmix_td_f32: null pointer");
  MAVA_ARG_CHECK(dq != q && dq != q_next_online && dq != q_next_target, 7, "mava_qmix_td_f32: dq must not alias a Q input");
  if (mode == 1) {
    MAVA_ARG_CHECK(w1 && b1 && w2 && b2 && w1_target && b1_target && w2_target && b2_target && d_w1 && d_b1 && d_w2 && d_b2, 8,
                   "mava_qmix_td_f32: null hypernet pointer in qmix mode");
    MAVA_ARG_CHECK(d_w1 != w1 && d_b1 != b1 && d_w2 != w2 && d_b2 != b2, 9,
                   "mava_qmix_td_f32: a hypernet gradient must not alias its input");
  }
  QmixTd a = {};
  a.qmix = mode; a.L = L; a.B = B; a.Bp = (B + 31) / 32 * 32; a.A = A; a.Rp = Rp; a.nA = n_actions; a.Em = mode ? Em : 0;
  a.q = q; a.qn = q_next_online; a.qt = q_next_target; a.action = action; a.reward = reward; a.term_next = terminal_next;
  a.next_mask = next_mask;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w1t = w1_target; a.b1t = b1_target; a.w2t = w2_target; a.b2t = b2_target;
  a.gamma = gamma; a.inv_n = 1.0f / (float)((double)L * B); a.grad_scale = grad_scale;
  a.dq = dq; a.d_w1 = d_w1; a.d_b1 = d_b1; a.d_w2 = d_w2; a.d_b2 = d_b2; a.partials = partials;
  hipLaunchKernelGGL(qmix_td_kernel, dim3(nblk), dim3(THREADS), 0, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
