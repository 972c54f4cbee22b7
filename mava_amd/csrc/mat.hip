// Multi-Agent Transformer (ff_mat, Wen et al. 2022): everything that sits between the dense products of the encoder and
// the decoder.  The products themselves (q / k / v / output projections, the MLPs, the heads) are mava_rec_dense_f32 /
// mava_rec_xty_f32 launches; this file adds attention over the A agents of a sample, LayerNorm with a learned scale and a
// residual input, GELU, the decoder's shifted one-hot input, the per-agent sampling step of the autoregressive decode and
// the PPO loss over agent rows; for the continuous head (tanh-normal, tanh_normal.h) the shifted action vectors, the
// per-agent sampling step and the loss (mava_transformer_*_f32 at the end of this file).
//
// Rows.  Every matrix is T32 (generic_layers.hip): element (row, f) of a (rows x N) matrix at
// ((row / 32) * N + f) * 32 + row % 32, `rows` a multiple of 32.  Agent row b * A + j belongs to sample b; rows past B * A
// are padding and every kernel writes exact zeros there.  A does not divide 32 in general, so samples straddle tiles.
//
// Lane mappings (DESIGN.md 3.25 has the resource table).
//  * attention: a work item is (group of S = max(1, 32 / A) consecutive samples, head): R = S * A <= 32 rows x hd <= 128
//    features of q and k (then v; in the backward pass q and k, dy and v, q and k again) are staged in two LDS tiles, thread e of the
//    256 reading row e % R of feature e / R, so a wave's load is runs of R consecutive rows of one feature.  The R * A scores
//    of the item are one thread each (a dot product over hd from LDS), the softmax is one thread per row over <= 32 keys,
//    the R * hd outputs are one thread each (a sum over the A keys).  Items are dealt to blocks round robin; an item is
//    computed the same way whichever block takes it, so the outputs are bit-identical for any grid.
//  * LayerNorm: a block owns a 32-row tile at a time; lane l of each of the 8 feature groups is row l, group g takes the
//    features g, g + 8, ..: every load of a half wave is one 128-byte run.  The 8 partial sums of a row meet in LDS and are
//    added in group order by every thread of the row.  The backward pass adds the per-block column sums of dy * xhat and dy
//    (one thread per feature, rows in order) for the scale and bias gradients.
//  * GELU, shifted one-hot: one thread per element in storage order.  Sampling: one thread per sample.  Loss: one thread per
//    agent row.
//
// Arithmetic.  Storage is f32.  The sums (dot products over hd, the softmax over the keys, LayerNorm's moments, the
// backward pass's row sums) and the two transcendental functions that enter them (exp of the softmax, tanh of GELU) run in
// f64: the softmax backward and LayerNorm's backward subtract sums of nearly equal size, and f32 sums alone use up the 1e-6
// the outputs are held to against the float64 model (as in qmix.hip).  gfx950 issues f64 FMAs at the f32 rate and the
// kernels are bound by launch latency at every size the learner uses.
//
// Determinism: no atomics; every sum has a fixed order that does not depend on the grid.  The per-block slabs of the
// LayerNorm backward depend on n_slab like every slab of this library (fixed by the learner); a block without tiles writes
// exact zeros.
#include <cfloat>

#include "common.h"
#include "mat_rows.h"
#include "tanh_normal.h"

namespace {

constexpr int TILE = 32;
constexpr int MAX_A = 32;
constexpr int MAX_D = 128;
constexpr int LDQ = MAX_D + 1;   // LDS row stride of a staged (rows x hd) tile: rows fall on different banks
constexpr int LDP = MAX_A + 1;   // LDS row stride of the (rows x A) score tile
constexpr int MAX_ACT = 64;
constexpr int MAX_DIM = 16;       // action dimensions of the continuous head (the limit of the other continuous kernels)
constexpr double LN_EPS = 1e-6;  // flax.linen.LayerNorm default epsilon

__device__ __forceinline__ long t32(long row, long f, long N) { return ((row >> 5) * N + f) * 32 + (row & 31); }

struct AttnTask {
  const float *q, *k, *v, *dy;
  float *y, *p, *dq, *dk, *dv;
  long rows;
  int D, B, A, H, hd, causal, S;
};

// stage rows [row0, row0 + nr) x features [f0, f0 + hd) of a T32 (rows x D) matrix into dst[r * LDQ + d]
__device__ __forceinline__ void stage(float* dst, const float* __restrict__ src, long row0, int nr, int f0, int hd, int D) {
  for (int e = threadIdx.x; e < nr * hd; e += 256) {
    const int d = e / nr, r = e - d * nr;
    dst[r * LDQ + d] = src[t32(row0 + r, f0 + d, D)];
  }
}

// exact zeros on the padding rows [valid, rows) of a T32 (rows x N) matrix
__device__ __forceinline__ void zero_padding(float* __restrict__ m, long valid, long rows, int N) {
  const long npad = rows - valid;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < npad * N; e += (long)gridDim.x * 256) {
    const long f = e / npad;
    m[t32(valid + (e - f * npad), f, N)] = 0.0f;
  }
}

// s_s[r][j] = softmax_j(q_r . k_j / sqrt(hd)) of the item's rows, in f64; q and k are staged into s_a and s_b.  Ends on a barrier.
__device__ __forceinline__ void probabilities(const AttnTask& a, float* s_a, float* s_b, double* s_s, long row0, int nr, int h) {
  const int tid = threadIdx.x, A = a.A, hd = a.hd;
  const double scale = 1.0 / sqrt((double)hd);
  stage(s_a, a.q, row0, nr, h * hd, hd, a.D);
  stage(s_b, a.k, row0, nr, h * hd, hd, a.D);
  __syncthreads();
  for (int e = tid; e < nr * A; e += 256) {
    const int r = e / A, j = e - r * A;
    const int kr = r - (r % A) + j;
    double s = 0.0;
    for (int d = 0; d < hd; ++d) s = fma((double)s_a[r * LDQ + d], (double)s_b[kr * LDQ + d], s);
    s_s[r * LDP + j] = s * scale;
  }
  __syncthreads();
  if (tid < nr) {
    const int r = tid;
    const int last = a.causal ? (r % A) : (A - 1);  // agent i sees the keys j <= i
    double mx = s_s[r * LDP];
    for (int j = 1; j <= last; ++j) mx = fmax(mx, s_s[r * LDP + j]);
    double se = 0.0;
    for (int j = 0; j <= last; ++j) {
      const double ex = exp(s_s[r * LDP + j] - mx);
      s_s[r * LDP + j] = ex;
      se += ex;
    }
    const double inv = 1.0 / se;
    for (int j = 0; j < A; ++j) s_s[r * LDP + j] = (j <= last) ? s_s[r * LDP + j] * inv : 0.0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnTask a) {
  __shared__ float s_a[TILE * LDQ];   // q, then v
  __shared__ float s_b[TILE * LDQ];   // k
  __shared__ double s_s[TILE * LDP];  // scores, then probabilities
  const int tid = threadIdx.x;
  const int A = a.A, hd = a.hd, R = a.S * A, HA = a.H * A;
  const long valid = (long)a.B * A;
  const long items = (long)((a.B + a.S - 1) / a.S) * a.H;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long g = it / a.H;
    const int h = (int)(it - g * a.H);
    const long row0 = g * R;
    const int nr = (int)((valid - row0 < R) ? (valid - row0) : R);  // a multiple of A
    probabilities(a, s_a, s_b, s_s, row0, nr, h);
    if (a.p != nullptr)
      for (int e = tid; e < nr * A; e += 256) {
        const int j = e / nr, r = e - j * nr;
        a.p[t32(row0 + r, h * A + j, HA)] = (float)s_s[r * LDP + j];
      }
    stage(s_a, a.v, row0, nr, h * hd, hd, a.D);
    __syncthreads();
    for (int e = tid; e < nr * hd; e += 256) {
      const int d = e / nr, r = e - d * nr;
      const int base = r - (r % A);
      double acc = 0.0;
      for (int j = 0; j < A; ++j) acc = fma(s_s[r * LDP + j], (double)s_a[(base + j) * LDQ + d], acc);
      a.y[t32(row0 + r, h * hd + d, a.D)] = (float)acc;
    }
    __syncthreads();
  }
  zero_padding(a.y, valid, a.rows, a.D);
  if (a.p != nullptr) zero_padding(a.p, valid, a.rows, HA);
}

// P = softmax(S), S = scale q k^T, y = P v.  P is computed again from q and k in f64 rather than read back: the f32 copy the
// forward pass may save is rounded at 6e-8, and dS subtracts two sums of size |dP| - measured 4.7e-6 of dq's max-abs.
//   dv = P^T dy;  dP = dy v^T;  dS = P (dP - rowsum(P dP)) scale;  dq = dS k;  dk = dS^T q
__global__ __launch_bounds__(256) void attn_bwd_kernel(AttnTask a) {
  __shared__ float s_a[TILE * LDQ];   // q, then dy, then q again
  __shared__ float s_b[TILE * LDQ];   // k, then v, then k again
  __shared__ double s_s[TILE * LDP];  // P
  __shared__ double s_d[TILE * LDP];  // dP, then dS
  const int tid = threadIdx.x;
  const int A = a.A, hd = a.hd, R = a.S * A;
  const long valid = (long)a.B * A;
  const long items = (long)((a.B + a.S - 1) / a.S) * a.H;
  const double scale = 1.0 / sqrt((double)hd);
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long g = it / a.H;
    const int h = (int)(it - g * a.H);
    const long row0 = g * R;
    const int nr = (int)((valid - row0 < R) ? (valid - row0) : R);
    probabilities(a, s_a, s_b, s_s, row0, nr, h);
    stage(s_a, a.dy, row0, nr, h * hd, hd, a.D);
    stage(s_b, a.v, row0, nr, h * hd, hd, a.D);
    __syncthreads();
    for (int e = tid; e < nr * A; e += 256) {
      const int r = e / A, j = e - r * A;
      const int kr = r - (r % A) + j;
      double s = 0.0;
      for (int d = 0; d < hd; ++d) s = fma((double)s_a[r * LDQ + d], (double)s_b[kr * LDQ + d], s);
      s_d[r * LDP + j] = s;
    }
    for (int e = tid; e < nr * hd; e += 256) {  // dv: row r is the KEY row here
      const int d = e / nr, r = e - d * nr;
      const int j = r % A, base = r - j;
      double acc = 0.0;
      for (int i = 0; i < A; ++i) acc = fma(s_s[(base + i) * LDP + j], (double)s_a[(base + i) * LDQ + d], acc);
      a.dv[t32(row0 + r, h * hd + d, a.D)] = (float)acc;
    }
    __syncthreads();
    if (tid < nr) {
      const int r = tid;
      double dot = 0.0;
      for (int j = 0; j < A; ++j) dot = fma(s_s[r * LDP + j], s_d[r * LDP + j], dot);
      for (int j = 0; j < A; ++j) s_d[r * LDP + j] = s_s[r * LDP + j] * (s_d[r * LDP + j] - dot) * scale;
    }
    stage(s_a, a.q, row0, nr, h * hd, hd, a.D);
    stage(s_b, a.k, row0, nr, h * hd, hd, a.D);
    __syncthreads();
    for (int e = tid; e < nr * hd; e += 256) {
      const int d = e / nr, r = e - d * nr;
      const int i = r % A, base = r - i;
      double accq = 0.0, acck = 0.0;
      for (int j = 0; j < A; ++j) {
        accq = fma(s_d[r * LDP + j], (double)s_b[(base + j) * LDQ + d], accq);         // row r as the query, keys j
        acck = fma(s_d[(base + j) * LDP + i], (double)s_a[(base + j) * LDQ + d], acck);  // row r as the key, queries j
      }
      a.dq[t32(row0 + r, h * hd + d, a.D)] = (float)accq;
      a.dk[t32(row0 + r, h * hd + d, a.D)] = (float)acck;
    }
    __syncthreads();
  }
  zero_padding(a.dq, valid, a.rows, a.D);
  zero_padding(a.dk, valid, a.rows, a.D);
  zero_padding(a.dv, valid, a.rows, a.D);
}

// sum over the 8 feature groups of a row, in group order, seen by every thread of the row
__device__ __forceinline__ double row_sum(double (*red)[TILE], double part, int lane, int grp) {
  __syncthreads();  // (the previous sum has been read)
  red[grp][lane] = part;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int g = 0; g < 8; ++g) tot += red[g][lane];
  return tot;
}

__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                     const float* __restrict__ scale, const float* __restrict__ bias, int N,
                                                     long rows, long valid, float* __restrict__ y, float* __restrict__ xhat,
                                                     float* __restrict__ rstd) {
  __shared__ double red[8][TILE];
  const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
  for (long tile = blockIdx.x; tile < rows / 32; tile += gridDim.x) {
    const long row = tile * 32 + lane, base = tile * N * 32 + lane;
    const bool real = row < valid;
    double s = 0.0;
    for (int f = grp; f < N; f += 8) {
      const long i = base + (long)f * 32;
      s += (double)(res != nullptr ? x[i] + res[i] : x[i]);
    }
    const double mean = row_sum(red, s, lane, grp) / (double)N;
    double v = 0.0;
    for (int f = grp; f < N; f += 8) {
      const long i = base + (long)f * 32;
      const double d = (double)(res != nullptr ? x[i] + res[i] : x[i]) - mean;
      v = fma(d, d, v);
    }
    const double r = 1.0 / sqrt(row_sum(red, v, lane, grp) / (double)N + LN_EPS);
    for (int f = grp; f < N; f += 8) {
      const long i = base + (long)f * 32;
      const double xh = ((double)(res != nullptr ? x[i] + res[i] : x[i]) - mean) * r;
      if (xhat != nullptr) xhat[i] = real ? (float)xh : 0.0f;
      y[i] = real ? (float)fma(xh, (double)scale[f], (double)bias[f]) : 0.0f;
    }
    if (grp == 0 && rstd != nullptr) rstd[row] = real ? (float)r : 0.0f;
  }
}

// g = dy * scale;  dx = rstd (g - mean(g) - xhat mean(g xhat));  slab[b] = out_scale [colsum(dy xhat) | colsum(dy)] of b's tiles
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                     const float* __restrict__ rstd, const float* __restrict__ scale, int N,
                                                     long rows, long valid, float out_scale, float* __restrict__ dx,
                                                     float* __restrict__ slab, long slab_stride) {
  __shared__ double red[8][TILE];
  const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const long ntiles = rows / 32;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row = tile * 32 + lane, base = tile * N * 32 + lane;
    const bool real = row < valid;
    double s1 = 0.0, s2 = 0.0;
    for (int f = grp; f < N; f += 8) {
      const long i = base + (long)f * 32;
      const double g = (double)dy[i] * (double)scale[f];
      s1 += g;
      s2 = fma(g, (double)xhat[i], s2);
    }
    const double m1 = row_sum(red, s1, lane, grp) / (double)N;
    const double m2 = row_sum(red, s2, lane, grp) / (double)N;
    const double r = (double)rstd[row];
    for (int f = grp; f < N; f += 8) {
      const long i = base + (long)f * 32;
      const double g = (double)dy[i] * (double)scale[f];
      dx[i] = real ? (float)(r * (g - m1 - (double)xhat[i] * m2)) : 0.0f;
    }
  }
  for (int f = threadIdx.x; f < N; f += 256) {
    double ds = 0.0, db = 0.0;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const long left = valid - tile * 32;
      const int n = (int)(left < 0 ? 0 : (left > 32 ? 32 : left));
      const long base = (tile * N + f) * 32;
      for (int l = 0; l < n; ++l) {
        const double g = (double)dy[base + l];
        ds = fma(g, (double)xhat[base + l], ds);
        db += g;
      }
    }
    slab[(long)blockIdx.x * slab_stride + f] = (float)(ds * (double)out_scale);
    slab[(long)blockIdx.x * slab_stride + N + f] = (float)(db * (double)out_scale);
  }
}

// flax nn.gelu(approximate=True): 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))
constexpr double GELU_C = 0.7978845608028654, GELU_K = 0.044715;

__global__ __launch_bounds__(256) void gelu_kernel(const float* __restrict__ x, long n, float* __restrict__ y) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double v = (double)x[i];
    y[i] = (float)(0.5 * v * (1.0 + tanh(GELU_C * (v + GELU_K * v * v * v))));
  }
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, long n,
                                                       float* __restrict__ dx) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double v = (double)x[i];
    const double t = tanh(GELU_C * (v + GELU_K * v * v * v));
    const double d = 0.5 * (1.0 + t) + 0.5 * v * (1.0 - t * t) * GELU_C * (1.0 + 3.0 * GELU_K * v * v);
    dx[i] = (float)((double)dy[i] * d);
  }
}

// s[b, 0] = e_0 (start token); s[b, i] = [0 | onehot(action[b, i - 1])] for 1 <= i <= known; zero rows after that
__global__ __launch_bounds__(256) void shift_onehot_kernel(const int32_t* __restrict__ action, const int32_t* __restrict__ idx,
                                                           int B, int A, int known, long rows, int Np, float* __restrict__ out) {
  const long total = rows * Np, valid = (long)B * A;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long tile = e / ((long)Np * 32);
    const int rem = (int)(e - tile * Np * 32);
    const int f = rem >> 5;
    const long row = tile * 32 + (rem & 31);
    float v = 0.0f;
    if (row < valid) {
      const long b = row / A;
      const int i = (int)(row - b * A);
      if (i == 0) {
        v = (f == 0) ? 1.0f : 0.0f;
      } else if (i - 1 < known) {
        const long sb = idx != nullptr ? idx[b] : b;
        v = (f == 1 + action[sb * A + (i - 1)]) ? 1.0f : 0.0f;
      }
    }
    out[e] = v;
  }
}

struct SampleTask {
  int B, A, agent, n;
  const float* logits;
  const uint8_t* mask;
  uint32_t seed_lo, seed_hi, step, row_offset;
  int greedy;
  int32_t* action;
  float* log_prob;
};

// agent `agent` of every sample: Gumbel-max on the Philox stream of mava_seq_sample_f32 (counter (row_offset + row, step,
// action / 4, "POLI"), word action % 4), or the argmax when greedy (first index on ties)
__global__ __launch_bounds__(256) void mat_sample_kernel(SampleTask tk) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= tk.B) return;
  const long row = (long)b * tk.A + tk.agent;
  RowLogits rl = {tk.logits + (row >> 5) * tk.n * 32 + (row & 31), tk.mask ? tk.mask + row * tk.n : nullptr, tk.n};
  const RowStats st = row_stats(rl);
  const int a = row_draw(rl, tk.greedy, tk.row_offset + (uint32_t)row, tk.step, tk.seed_lo, tk.seed_hi);
  tk.action[row] = a;
  tk.log_prob[row] = row_log_prob(rl, st, a);
}

struct LossTask {
  int Bm, A, n;
  long rows;
  const int32_t* idx;
  const float *logits, *values;
  const uint8_t* mask;
  const int32_t* action;
  const float *old_log_prob, *adv, *old_value, *targets;
  const double* stats;
  int n_stats;
  float clip_eps, ent_coef, vf_coef, grad_scale;
  float *dlogits, *dvalues, *partials;
};

// the formulas of mava_seq_actor_loss_f32 / mava_seq_critic_loss_f32 on the rows of a minibatch of (t, env) samples:
// agent row q = b * A + j reads the trajectory at sample idx[b]; means over the Bm * A agent rows
__global__ __launch_bounds__(256) void mat_loss_kernel(LossTask tk) {
  __shared__ float red[3][4];
  __shared__ float st[2];
  const long R = (long)tk.Bm * tk.A;
  const float invR = 1.0f / (float)R, gs = tk.grad_scale;
  if (threadIdx.x == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < tk.n_stats; ++i) { s1 += tk.stats[2 * i]; s2 += tk.stats[2 * i + 1]; }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    st[0] = (float)mean;
    st[1] = 1.0f / ((float)sqrt(var) + 1e-8f);
  }
  __syncthreads();
  float la = 0.0f, lb = 0.0f, lc = 0.0f;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < tk.rows; q += (long)gridDim.x * 256) {
    const long tb = (q >> 5) * tk.n * 32 + (q & 31);
    if (q >= R) {  // padding
      for (int o = 0; o < tk.n; ++o) tk.dlogits[tb + (long)o * 32] = 0.0f;
      tk.dvalues[q] = 0.0f;
      continue;
    }
    const long b = q / tk.A;
    const long er = (long)tk.idx[b] * tk.A + (q - b * tk.A);
    RowLogits rl = {tk.logits + tb, tk.mask ? tk.mask + er * tk.n : nullptr, tk.n};
    const RowStats rs = row_stats(rl);
    const int act = tk.action[er];
    float lp = 0.0f, entropy = 0.0f;
    for (int o = 0; o < tk.n; ++o) {
      const float logp = (rs.none ? 0.0f : rl.z(o)) - rs.lse;
      const float p = expf(logp);
      entropy -= (p > 0.0f) ? p * logp : 0.0f;
      if (o == act) lp = logp;
    }
    const float gae = (tk.adv[er] - st[0]) * st[1];
    const float ratio = expf(lp - tk.old_log_prob[er]);
    const float lo = 1.0f - tk.clip_eps, hi = 1.0f + tk.clip_eps;
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float l1 = ratio * gae, l2 = rc * gae;
    const bool inside = (ratio >= lo) && (ratio <= hi);
    const float g1 = (l1 < l2) ? 1.0f : ((l1 == l2) ? 0.5f : 0.0f);
    const float g2 = inside ? (1.0f - g1) : 0.0f;
    const float dlp = -(g1 + g2) * gae * ratio * invR;
    const float ec = tk.ent_coef * invR;
    for (int o = 0; o < tk.n; ++o) {
      const float logp = (rs.none ? 0.0f : rl.z(o)) - rs.lse;
      const float p = expf(logp);
      const float oh = (o == act) ? 1.0f : 0.0f;
      const float pl = (p > 0.0f) ? logp : 0.0f;
      float d = dlp * (oh - p) + ec * p * (pl + entropy);
      if (rl.z(o) == -FLT_MAX) d = 0.0f;
      tk.dlogits[tb + (long)o * 32] = d * gs;
    }
    la += -fminf(l1, l2) * invR;
    lb += entropy * invR;
    // value: rec_mappo.py:244-266
    const float v = tk.values[q];
    const float ov = tk.old_value[er], tg = tk.targets[er];
    const float diff = v - ov;
    const float vclip = ov + fminf(fmaxf(diff, -tk.clip_eps), tk.clip_eps);
    const float e1 = v - tg, e2 = vclip - tg;
    const float v1 = e1 * e1, v2 = e2 * e2;
    const bool vin = (diff >= -tk.clip_eps) && (diff <= tk.clip_eps);
    const float h1 = (v1 > v2) ? 1.0f : ((v1 == v2) ? 0.5f : 0.0f);
    const float h2 = vin ? (1.0f - h1) : 0.0f;
    tk.dvalues[q] = tk.vf_coef * (h1 * e1 + h2 * e2) * invR * gs;
    lc += 0.5f * fmaxf(v1, v2) * invR;
  }
  for (int o = 32; o > 0; o >>= 1) {
    la += __shfl_down(la, o, 64);
    lb += __shfl_down(lb, o, 64);
    lc += __shfl_down(lc, o, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[0][w] = la; red[1][w] = lb; red[2][w] = lc; }
  __syncthreads();
  if (threadIdx.x < 3)
    tk.partials[3 * blockIdx.x + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// ---- continuous head ------------------------------------------------------------------------------------------------------
// s[b, 0] = 0; s[b, i] = action[b, i - 1] (d features) for 1 <= i <= known; zero rows after that, zero features past d
__global__ __launch_bounds__(256) void shift_action_kernel(const float* __restrict__ action, const int32_t* __restrict__ idx, int B,
                                                           int A, int d, int known, long rows, int Np, float* __restrict__ out) {
  const long total = rows * Np, valid = (long)B * A;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long tile = e / ((long)Np * 32);
    const int rem = (int)(e - tile * Np * 32);
    const int f = rem >> 5;
    const long row = tile * 32 + (rem & 31);
    float v = 0.0f;
    if (row < valid && f < d) {
      const long b = row / A;
      const int i = (int)(row - b * A);
      if (i >= 1 && i - 1 < known) {
        const long sb = idx != nullptr ? idx[b] : b;
        v = action[(sb * A + (i - 1)) * d + f];
      }
    }
    out[e] = v;
  }
}

struct SampleContTask {
  int B, A, agent, d;
  float min_scale;
  const float *mean, *log_std;
  uint32_t seed_lo, seed_hi, step, row_offset;
  int greedy;
  float *action, *log_prob;
};

// agent `agent` of every sample: a = tanh(mean + scale * eps), eps on the Philox stream of mava_seq_sample_continuous_f32
// (counter (row_offset + row, step, dim / 2, "TNSA")), 0 when greedy; the log-prob is that of the action written
__global__ __launch_bounds__(256) void mat_sample_cont_kernel(SampleContTask tk) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= tk.B) return;
  const long row = (long)b * tk.A + tk.agent;
  const float* mp = tk.mean + (row >> 5) * tk.d * 32 + (row & 31);
  const uint32_t gid = tk.row_offset + (uint32_t)row;
  float lp = 0.0f;
  for (int o = 0; o < tk.d; ++o) {
    const float mean = mp[(long)o * 32];
    const float sc = tn::scale_of(tk.log_std[o], tk.min_scale);
    const float eps = tk.greedy ? 0.0f : tn::noise(gid, tk.step, o, tn::STREAM_SAMPLE, tk.seed_lo, tk.seed_hi);
    const float a = tanhf(fmaf(sc, eps, mean));
    lp += tn::log_prob(a, mean, sc).lp;
    tk.action[row * tk.d + o] = a;
  }
  tk.log_prob[row] = lp;
}

struct LossContTask {
  int Bm, A, d;
  float min_scale;
  long rows;
  const int32_t* idx;
  const float *mean, *log_std, *values, *action;
  const float *old_log_prob, *adv, *old_value, *targets;
  const double* stats;
  int n_stats;
  float clip_eps, ent_coef, vf_coef, grad_scale;
  uint32_t seed_lo, seed_hi, ent_step, row_offset;
  float *dmean, *dvalues, *partials, *dls_partials;
};

// mat_loss_kernel's row walk, value loss and padding handling with the actor part of mava_seq_actor_loss_continuous_f32
// (rec_gru.hip): a thread owns all d action dimensions of its agent row
template <int NO>
__global__ __launch_bounds__(256) void mat_loss_cont_kernel(LossContTask tk) {
  __shared__ float red[3 + NO][4];
  __shared__ float st[2];
  const long R = (long)tk.Bm * tk.A;
  const float invR = 1.0f / (float)R, gs = tk.grad_scale;
  if (threadIdx.x == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < tk.n_stats; ++i) { s1 += tk.stats[2 * i]; s2 += tk.stats[2 * i + 1]; }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    st[0] = (float)mean;
    st[1] = 1.0f / ((float)sqrt(var) + 1e-8f);
  }
  __syncthreads();
  float sc[NO], ds[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    sc[o] = tn::scale_of(tk.log_std[o < tk.d ? o : 0], tk.min_scale);
    ds[o] = 0.0f;
  }
  float la = 0.0f, lb = 0.0f, lc = 0.0f;
  const float lo = 1.0f - tk.clip_eps, hi = 1.0f + tk.clip_eps;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < tk.rows; q += (long)gridDim.x * 256) {
    const long tb = (q >> 5) * tk.d * 32 + (q & 31);
    if (q >= R) {  // padding
      for (int o = 0; o < tk.d; ++o) tk.dmean[tb + (long)o * 32] = 0.0f;
      tk.dvalues[q] = 0.0f;
      continue;
    }
    const long b = q / tk.A;
    const long er = (long)tk.idx[b] * tk.A + (q - b * tk.A);
    float dm[NO], dsl[NO], th[NO], ep[NO];
    float lp = 0.0f, ent = 0.0f;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      dm[o] = dsl[o] = th[o] = ep[o] = 0.0f;
      if (o < tk.d) {
        const float mean = tk.mean[tb + (long)o * 32];
        const tn::LogProb l = tn::log_prob(tk.action[er * tk.d + o], mean, sc[o]);
        lp += l.lp;
        dm[o] = l.dmean;
        dsl[o] = l.dscale;
        ep[o] = tn::noise(tk.row_offset + (uint32_t)er, tk.ent_step, o, tn::STREAM_ENTROPY, tk.seed_lo, tk.seed_hi);
        const float x = fmaf(sc[o], ep[o], mean);
        th[o] = tanhf(x);
        ent += 0.5f + tn::HALF_LOG_2PI + logf(sc[o]) + tn::tanh_fldj(x);
      }
    }
    const float gae = (tk.adv[er] - st[0]) * st[1];
    const float ratio = expf(lp - tk.old_log_prob[er]);
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float l1 = ratio * gae, l2 = rc * gae;
    const bool inside = (ratio >= lo) && (ratio <= hi);
    const float g1 = (l1 < l2) ? 1.0f : ((l1 == l2) ? 0.5f : 0.0f);
    const float g2 = inside ? (1.0f - g1) : 0.0f;
    const float dlp = -(g1 + g2) * gae * ratio * invR;
    const float ec = tk.ent_coef * invR;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      if (o < tk.d) {
        tk.dmean[tb + (long)o * 32] = (dlp * dm[o] + ec * 2.0f * th[o]) * gs;
        ds[o] += dlp * dsl[o] - ec * (1.0f / sc[o] - 2.0f * th[o] * ep[o]);
      }
    }
    la += -fminf(l1, l2) * invR;
    lb += ent * invR;
    // value: as mat_loss_kernel
    const float v = tk.values[q];
    const float ov = tk.old_value[er], tg = tk.targets[er];
    const float diff = v - ov;
    const float vclip = ov + fminf(fmaxf(diff, -tk.clip_eps), tk.clip_eps);
    const float e1 = v - tg, e2 = vclip - tg;
    const float v1 = e1 * e1, v2 = e2 * e2;
    const bool vin = (diff >= -tk.clip_eps) && (diff <= tk.clip_eps);
    const float h1 = (v1 > v2) ? 1.0f : ((v1 == v2) ? 0.5f : 0.0f);
    const float h2 = vin ? (1.0f - h1) : 0.0f;
    tk.dvalues[q] = tk.vf_coef * (h1 * e1 + h2 * e2) * invR * gs;
    lc += 0.5f * fmaxf(v1, v2) * invR;
  }
  for (int o = 32; o > 0; o >>= 1) {
    la += __shfl_down(la, o, 64);
    lb += __shfl_down(lb, o, 64);
    lc += __shfl_down(lc, o, 64);
#pragma unroll
    for (int k = 0; k < NO; ++k) ds[k] += __shfl_down(ds[k], o, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][w] = la; red[1][w] = lb; red[2][w] = lc;
#pragma unroll
    for (int k = 0; k < NO; ++k) red[3 + k][w] = ds[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 3) tk.partials[3 * blockIdx.x + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
  if (k < tk.d)  // d scale / d log_std = sigmoid(log_std)
    tk.dls_partials[(long)blockIdx.x * tk.d + k] =
        (((red[3 + k][0] + red[3 + k][1]) + red[3 + k][2]) + red[3 + k][3]) * tn::sigmoid(tk.log_std[k]);
}

int blocks_for(long total, int cap) {
  long b = (total + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

int attn_task(AttnTask& a, const char* who, long rows, int D, int B, int A, int n_head, int n_blocks) {
  MAVA_ARG_CHECK(rows >= 32 && rows % 32 == 0 && B >= 1 && A >= 1 && A <= MAX_A && (long)B * A <= rows, 0,
                 "%s: rows=%ld B=%d A=%d (rows a multiple of 32 holding B * A rows, A <= %d)", who, rows, B, A, MAX_A);
  MAVA_ARG_CHECK(n_head >= 1 && D >= n_head && D % n_head == 0 && D / n_head <= MAX_D, 1,
                 "%s: D=%d n_head=%d (D a multiple of n_head, D / n_head <= %d)", who, D, n_head, MAX_D);
  MAVA_ARG_CHECK(n_blocks >= 1 && n_blocks <= 65536, 2, "%s: n_blocks=%d", who, n_blocks);
  a.rows = rows; a.D = D; a.B = B; a.A = A; a.H = n_head; a.hd = D / n_head;
  a.S = A >= TILE ? 1 : TILE / A;
  return MAVA_OK;
}

}  // namespace

extern "C" int mava_mat_attn_fwd_f32(const float* q, const float* k, const float* v, long rows, int D, int B, int A, int n_head,
                                     int causal, float* y, float* p, int n_blocks, hipStream_t s) {
  AttnTask a = {};
  const int rc = attn_task(a, "mava_mat_attn_fwd_f32", rows, D, B, A, n_head, n_blocks);
  if (rc != MAVA_OK) return rc;
  MAVA_ARG_CHECK(q && k && v && y, 3, "mava_mat_attn_fwd_f32: null pointer argument");
  a.q = q; a.k = k; a.v = v; a.y = y; a.p = p; a.causal = causal != 0;
  hipLaunchKernelGGL(attn_fwd_kernel, dim3(n_blocks), dim3(256), 0, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_attn_bwd_f32(const float* dy, const float* q, const float* k, const float* v, long rows, int D, int B,
                                     int A, int n_head, int causal, float* dq, float* dk, float* dv, int n_blocks,
                                     hipStream_t s) {
  AttnTask a = {};
  const int rc = attn_task(a, "mava_mat_attn_bwd_f32", rows, D, B, A, n_head, n_blocks);
  if (rc != MAVA_OK) return rc;
  MAVA_ARG_CHECK(dy && q && k && v && dq && dk && dv, 3, "mava_mat_attn_bwd_f32: null pointer argument");
  a.causal = causal != 0; a.dy = dy; a.q = q; a.k = k; a.v = v; a.dq = dq; a.dk = dk; a.dv = dv;
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(n_blocks), dim3(256), 0, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_ln_fwd_f32(const float* x, const float* res, const float* scale, const float* bias, int N, long rows,
                                   long valid_rows, float* y, float* xhat, float* rstd, int n_blocks, hipStream_t s) {
  MAVA_ARG_CHECK(N >= 1 && rows >= 32 && rows % 32 == 0 && valid_rows >= 0 && valid_rows <= rows && n_blocks >= 1 && n_blocks <= 65536,
                 0, "mava_mat_ln_fwd_f32: N=%d rows=%ld valid_rows=%ld n_blocks=%d", N, rows, valid_rows, n_blocks);
  MAVA_ARG_CHECK(x && scale && bias && y && ((xhat == nullptr) == (rstd == nullptr)), 1,
                 "mava_mat_ln_fwd_f32: null pointer argument (xhat and rstd come together)");
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(n_blocks), dim3(256), 0, s, x, res, scale, bias, N, rows, valid_rows, y, xhat, rstd);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_ln_bwd_f32(const float* dy, const float* xhat, const float* rstd, const float* scale, int N, long rows,
                                   long valid_rows, float out_scale, float* dx, float* slab, long slab_stride, int n_slab,
                                   hipStream_t s) {
  MAVA_ARG_CHECK(N >= 1 && rows >= 32 && rows % 32 == 0 && valid_rows >= 0 && valid_rows <= rows, 0,
                 "mava_mat_ln_bwd_f32: N=%d rows=%ld valid_rows=%ld", N, rows, valid_rows);
  MAVA_ARG_CHECK(n_slab >= 1 && n_slab <= 65536 && slab_stride >= 2L * N, 1,
                 "mava_mat_ln_bwd_f32: n_slab=%d slab_stride=%ld (a slab holds 2 N floats)", n_slab, slab_stride);
  MAVA_ARG_CHECK(dy && xhat && rstd && scale && dx && slab, 2, "mava_mat_ln_bwd_f32: null pointer argument");
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(n_slab), dim3(256), 0, s, dy, xhat, rstd, scale, N, rows, valid_rows, out_scale, dx, slab,
                     slab_stride);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_gelu_f32(const float* x, long n, float* y, hipStream_t s) {
  MAVA_ARG_CHECK(n >= 0, 0, "mava_mat_gelu_f32: n=%ld", n);
  if (n == 0) return MAVA_OK;
  MAVA_ARG_CHECK(x && y, 1, "mava_mat_gelu_f32: null pointer argument");
  hipLaunchKernelGGL(gelu_kernel, dim3(blocks_for(n, 4096)), dim3(256), 0, s, x, n, y);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_gelu_bwd_f32(const float* dy, const float* x, long n, float* dx, hipStream_t s) {
  MAVA_ARG_CHECK(n >= 0, 0, "mava_mat_gelu_bwd_f32: n=%ld", n);
  if (n == 0) return MAVA_OK;
  MAVA_ARG_CHECK(dy && x && dx, 1, "mava_mat_gelu_bwd_f32: null pointer argument");
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks_for(n, 4096)), dim3(256), 0, s, dy, x, n, dx);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_shift_onehot_f32(const int32_t* action, const int32_t* idx, int B, int A, int n_actions, int known,
                                         long rows, int n_pad, float* out, hipStream_t s) {
  MAVA_ARG_CHECK(B >= 1 && A >= 1 && rows >= 32 && rows % 32 == 0 && (long)B * A <= rows, 0,
                 "mava_mat_shift_onehot_f32: B=%d A=%d rows=%ld", B, A, rows);
  MAVA_ARG_CHECK(n_actions >= 1 && n_pad >= n_actions + 1 && n_pad % 32 == 0 && known >= 0 && known <= A - 1, 1,
                 "mava_mat_shift_onehot_f32: n_actions=%d n_pad=%d known=%d (n_pad a multiple of 32 holding n_actions + 1, known <= A - 1)",
                 n_actions, n_pad, known);
  MAVA_ARG_CHECK(out && (action || known == 0), 2, "mava_mat_shift_onehot_f32: null pointer argument");
  hipLaunchKernelGGL(shift_onehot_kernel, dim3(blocks_for(rows * n_pad, 4096)), dim3(256), 0, s, action, idx, B, A, known, rows, n_pad,
                     out);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_sample_f32(int B, int A, int agent, int n_actions, const float* logits, const uint8_t* mask, uint64_t seed,
                                   uint32_t step, uint32_t row_offset, int greedy, int32_t* action, float* log_prob,
                                   hipStream_t s) {
  MAVA_ARG_CHECK(B >= 1 && A >= 1 && agent >= 0 && agent < A && n_actions >= 1 && n_actions <= MAX_ACT, 0,
                 "mava_mat_sample_f32: B=%d A=%d agent=%d n_actions=%d (n_actions <= %d)", B, A, agent, n_actions, MAX_ACT);
  MAVA_ARG_CHECK(logits && action && log_prob, 1, "mava_mat_sample_f32: null pointer argument");
  SampleTask tk = {};
  tk.B = B; tk.A = A; tk.agent = agent; tk.n = n_actions; tk.logits = logits; tk.mask = mask;
  tk.seed_lo = (uint32_t)seed; tk.seed_hi = (uint32_t)(seed >> 32); tk.step = step; tk.row_offset = row_offset;
  tk.greedy = greedy; tk.action = action; tk.log_prob = log_prob;
  hipLaunchKernelGGL(mat_sample_kernel, dim3(mava_cdiv(B, 256)), dim3(256), 0, s, tk);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_mat_loss_f32(int Bm, int A, int n_actions, long rows, const int32_t* idx, const float* logits,
                                 const float* values, const uint8_t* mask, const int32_t* action, const float* old_log_prob,
                                 const float* advantages, const float* old_value, const float* targets, const double* adv_stats,
                                 int n_stats, float clip_eps, float ent_coef, float vf_coef, float grad_scale, float* dlogits,
                                 float* dvalues, float* loss_partials, int n_blocks, hipStream_t s) {
  MAVA_ARG_CHECK(Bm >= 1 && A >= 1 && n_actions >= 1 && n_actions <= MAX_ACT && rows >= 32 && rows % 32 == 0 && (long)Bm * A <= rows &&
                 n_blocks >= 1 && n_blocks <= 65536 && n_stats >= 1, 0,
                 "mava_mat_loss_f32: Bm=%d A=%d n_actions=%d rows=%ld n_blocks=%d", Bm, A, n_actions, rows, n_blocks);
  MAVA_ARG_CHECK(idx && logits && values && action && old_log_prob && advantages && old_value && targets && adv_stats && dlogits &&
                 dvalues && loss_partials, 1, "mava_mat_loss_f32: null pointer argument");
  LossTask tk = {};
  tk.Bm = Bm; tk.A = A; tk.n = n_actions; tk.rows = rows; tk.idx = idx; tk.logits = logits; tk.values = values; tk.mask = mask;
  tk.action = action; tk.old_log_prob = old_log_prob; tk.adv = advantages; tk.old_value = old_value; tk.targets = targets;
  tk.stats = adv_stats; tk.n_stats = n_stats; tk.clip_eps = clip_eps; tk.ent_coef = ent_coef; tk.vf_coef = vf_coef;
  tk.grad_scale = grad_scale; tk.dlogits = dlogits; tk.dvalues = dvalues; tk.partials = loss_partials;
  hipLaunchKernelGGL(mat_loss_kernel, dim3(n_blocks), dim3(256), 0, s, tk);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_transformer_shift_action_f32(const float* action, const int32_t* idx, int B, int A, int action_dim, int known,
                                                 long rows, int n_pad, float* out, hipStream_t s) {
  const char* who = "mava_transformer_shift_action_f32";
  MAVA_ARG_CHECK(B >= 1 && A >= 1 && A <= MAX_A && rows >= 32 && rows % 32 == 0 && (long)B * A <= rows, 0,
                 "%s: B=%d A=%d rows=%ld (A <= %d, rows a multiple of 32 holding B * A rows)", who, B, A, rows, MAX_A);
  MAVA_ARG_CHECK(action_dim >= 1 && action_dim <= MAX_DIM && n_pad >= action_dim && n_pad % 32 == 0 && known >= 0 && known <= A - 1, 1,
                 "%s: action_dim=%d n_pad=%d known=%d (1 <= action_dim <= %d, n_pad a multiple of 32 holding it, known <= A - 1)", who,
                 action_dim, n_pad, known, MAX_DIM);
  MAVA_ARG_CHECK(out && (action || known == 0), 2, "%s: null pointer argument", who);
  hipLaunchKernelGGL(shift_action_kernel, dim3(blocks_for(rows * n_pad, 4096)), dim3(256), 0, s, action, idx, B, A, action_dim, known,
                     rows, n_pad, out);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_transformer_sample_continuous_f32(int B, int A, int agent, int action_dim, float min_scale, const float* mean,
                                                      const float* log_std, uint64_t seed, uint32_t step, uint32_t row_offset,
                                                      int greedy, float* action, float* log_prob, hipStream_t s) {
  const char* who = "mava_transformer_sample_continuous_f32";
  MAVA_ARG_CHECK(B >= 1 && A >= 1 && A <= MAX_A && agent >= 0 && agent < A && action_dim >= 1 && action_dim <= MAX_DIM, 0,
                 "%s: B=%d A=%d agent=%d action_dim=%d (A <= %d, agent < A, 1 <= action_dim <= %d)", who, B, A, agent, action_dim, MAX_A,
                 MAX_DIM);
  MAVA_ARG_CHECK(min_scale >= 0.0f, 1, "%s: min_scale=%g", who, (double)min_scale);
  MAVA_ARG_CHECK(mean && log_std && action && log_prob, 2, "%s: null pointer argument", who);
  SampleContTask tk = {};
  tk.B = B; tk.A = A; tk.agent = agent; tk.d = action_dim; tk.min_scale = min_scale; tk.mean = mean; tk.log_std = log_std;
  tk.seed_lo = (uint32_t)seed; tk.seed_hi = (uint32_t)(seed >> 32); tk.step = step; tk.row_offset = row_offset;
  tk.greedy = greedy != 0; tk.action = action; tk.log_prob = log_prob;
  hipLaunchKernelGGL(mat_sample_cont_kernel, dim3(mava_cdiv(B, 256)), dim3(256), 0, s, tk);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_transformer_loss_continuous_f32(int Bm, int A, int action_dim, float min_scale, long rows, const int32_t* idx,
                                                    const float* mean, const float* log_std, const float* values, const float* action,
                                                    const float* old_log_prob, const float* advantages, const float* old_value,
                                                    const float* targets, const double* adv_stats, int n_stats, float clip_eps,
                                                    float ent_coef, float vf_coef, uint64_t seed, uint32_t ent_step, uint32_t row_offset,
                                                    float grad_scale, float* dmean, float* dvalues, float* loss_partials,
                                                    float* dlog_std_partials, int n_blocks, hipStream_t s) {
  const char* who = "mava_transformer_loss_continuous_f32";
  MAVA_ARG_CHECK(Bm >= 1 && A >= 1 && A <= MAX_A && rows >= 32 && rows % 32 == 0 && (long)Bm * A <= rows && n_blocks >= 1 &&
                 n_blocks <= 65536 && n_stats >= 1, 0, "%s: Bm=%d A=%d rows=%ld n_blocks=%d (A <= %d, rows a multiple of 32 holding Bm * A)",
                 who, Bm, A, rows, n_blocks, MAX_A);
  MAVA_ARG_CHECK(action_dim >= 1 && action_dim <= MAX_DIM && min_scale >= 0.0f, 1, "%s: action_dim=%d min_scale=%g (1 <= action_dim <= %d)",
                 who, action_dim, (double)min_scale, MAX_DIM);
  MAVA_ARG_CHECK(idx && mean && log_std && values && action && old_log_prob && advantages && old_value && targets && adv_stats && dmean &&
                 dvalues && loss_partials && dlog_std_partials, 2, "%s: null pointer argument", who);
  LossContTask tk = {};
  tk.Bm = Bm; tk.A = A; tk.d = action_dim; tk.min_scale = min_scale; tk.rows = rows; tk.idx = idx; tk.mean = mean; tk.log_std = log_std;
  tk.values = values; tk.action = action; tk.old_log_prob = old_log_prob; tk.adv = advantages; tk.old_value = old_value;
  tk.targets = targets; tk.stats = adv_stats; tk.n_stats = n_stats; tk.clip_eps = clip_eps; tk.ent_coef = ent_coef; tk.vf_coef = vf_coef;
  tk.grad_scale = grad_scale; tk.seed_lo = (uint32_t)seed; tk.seed_hi = (uint32_t)(seed >> 32); tk.ent_step = ent_step;
  tk.row_offset = row_offset; tk.dmean = dmean; tk.dvalues = dvalues; tk.partials = loss_partials; tk.dls_partials = dlog_std_partials;
  if (action_dim <= 8) hipLaunchKernelGGL((mat_loss_cont_kernel<8>), dim3(n_blocks), dim3(256), 0, s, tk);
  else hipLaunchKernelGGL((mat_loss_cont_kernel<16>), dim3(n_blocks), dim3(256), 0, s, tk);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
