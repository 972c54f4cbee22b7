// ff_mat, fused acting: one env step of the Multi-Agent Transformer's autoregressive decode in one launch.
//
// What mat_learner.MATPass.act does in 1 + 18 + A * 25 launches (gather, encoder, then per agent the shifted one-hot, the
// whole decoder over every row and the sampling step) runs here per group of samples inside one workgroup: the encoder over
// the group's rows, then for i = 0 .. A - 1 the decoder for row i of each sample only.  Causality makes that exact: row i of
// every decoder layer depends on rows <= i alone, so the keys and values of the rows < i are kept (the cache) and row i's
// are appended.  The decoder's input row is a row of decoder/act_dense/kernel (row 0, or row 1 + the previous agent's
// action): the product with a one-hot is a row read.
//
// Work split.  A group is S = max(1, 32 / A) consecutive samples, R = S * A <= 32 agent rows (mat.hip's attention item).
// Groups are dealt to the blocks round robin in a persistent loop; a group is computed the same way whichever block takes
// it, every sum has a fixed order, there are no atomics: the outputs are bit-identical for any grid.  Every barrier sits
// under block-uniform control flow (the loops run over groups, agents, layers and heads; nr and ns are per-group numbers).
//
// Lane mappings (256 threads, D = 32 * D32 a template argument).
//  * dense D -> D: thread t owns output column t % D of the rows t / D, t / D + NS, .. (NS = 256 / D row slices; D = 96 leaves
//    64 threads idle).  The k loop reads W[k][n] straight from L2, coalesced along n, and the activations from LDS as
//    broadcasts; plain f32 FMAs in k order.  The number of rows per thread is a template argument picked per call from the
//    (block-uniform) row count, so a decoder step with few rows does not walk 16 accumulators.
//  * LayerNorm: 8 threads per row, thread g takes the features g, g + 8, ..; the 8 partial sums meet in a butterfly of
//    shuffles (the same value on all 8 lanes).  Moments in f64.
//  * attention: encoder one head at a time - one thread per (row, key) score, per row softmax, per (row, feature) output,
//    all from LDS.  Decoder (row i of each sample, keys j <= i from the cache): up to 32 heads at a time, 8 lanes per
//    (sample, head, key) score (lane g the features g, g + 8, .., summed in a butterfly), one thread per (sample, head)
//    softmax and per (sample, feature) output.  Dot products, softmax and the weighted sum in f64 as in mat.hip.
//  * logits: one thread per (sample, action); sampling: one thread per sample (mat_rows.h, the Philox counters of
//    mava_mat_sample_f32).
//
// Memory.  LDS: five (32 x (D + 1)) f32 tiles (x / rep, q, k, v, t), the score tile (32 x 33 f64), the logits (32 x 64),
// the observations' moments and the group's actions: 99 840 bytes at D = 128, 58 368 at D = 64 (dynamic LDS, the attribute
// is raised).  The key/value cache (self- and cross-attention of every decoder block: n_block * 4 * 32 * D floats per block
// of the grid) does not fit next to that at D = 128 and lives in the caller's workspace; a block writes a cache row before
// any of its threads reads it (a barrier in between), nothing is read that this launch has not written.
//
// Arithmetic (mat.hip's): storage f32; softmax with its exp, LayerNorm's moments and GELU's tanh in f64; dense products
// in f32 FMAs whatever the context's matmul mode.
#include <cfloat>

#include "common.h"
#include "mat_rows.h"
#include "tanh_normal.h"

namespace {

constexpr int ROWS = 32;
constexpr int MAX_A = 32;
constexpr int MAX_D = 128;
constexpr int MAX_ACT = 64;
constexpr int MAX_DIM = 16;    // action dimensions of the continuous head
constexpr int MAX_O = 1024;
constexpr int MAX_NBLOCK = 4;  // decoder blocks the kernel takes; beyond that the caller runs layer by layer
constexpr int LDP = MAX_A + 1;
constexpr double LN_EPS = 1e-6;
constexpr double GELU_C = 0.7978845608028654, GELU_K = 0.044715;

struct ActTask {
  const float* params;
  const float* obs;
  const uint8_t* mask;
  int B, A, O, nA, H, hd, nb, S, greedy;
  uint32_t seed_lo, seed_hi, step, row_offset;
  int32_t* action;
  float* log_prob;
  float* value;
  float* cache;
  float* action_f;  // continuous head: (B, A, nA) f32 actions, nA = the action dimension
  float min_scale;
};

__host__ __device__ inline long enc_block_size(long D) { return 6 * D * D + 10 * D; }
__host__ __device__ inline long dec_block_size(long D) { return 10 * D * D + 16 * D; }
__host__ __device__ inline long enc_size(long O, long D, long nb) {
  return 2 * O + O * D + D + 2 * D + nb * enc_block_size(D) + D * D + D + 2 * D + D + 1;
}
__host__ __device__ inline long dec_size(long nA, long D, long nb) {
  return (nA + 1) * D + 2 * D + nb * dec_block_size(D) + D * D + D + 2 * D + D * nA + nA;
}

__device__ __forceinline__ float gelu_f(float x) {
  const double v = (double)x;
  return (float)(0.5 * v * (1.0 + tanh(GELU_C * (v + GELU_K * v * v * v))));
}

// sum over the 8 lanes of a row, the same bits on each of them
__device__ __forceinline__ double sum8(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// out[o0 + r * os][n] = f(bias[n] + sum_k in[i0 + r * is][k] W[k][n]), r < nr <= NJ * NS.  `in` rows have stride D + 1 (LDS).
template <int D, int NJ, bool GELU>
__device__ __forceinline__ void dense_impl(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int i0, int is,
                                           float* out, int old, int o0, int os, int nr) {
  constexpr int NS = 256 / D, LD = D + 1;
  const int n = threadIdx.x % D, sl = threadIdx.x / D;
  if (sl >= NS) return;
  float acc[NJ];
  int xo[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int r = sl + j * NS;
    xo[j] = (i0 + (r < nr ? r : nr - 1) * is) * LD;
    acc[j] = 0.0f;
  }
#pragma unroll 8
  for (int k = 0; k < D; ++k) {
    const float w = W[k * D + n];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = fmaf(in[xo[j] + k], w, acc[j]);
  }
  const float b = bias[n];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int r = sl + j * NS;
    if (r < nr) {
      const float v = acc[j] + b;
      out[(long)(o0 + r * os) * old + n] = GELU ? gelu_f(v) : v;
    }
  }
}

template <int D, bool GELU>
__device__ __forceinline__ void dense(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int i0, int is,
                                      float* out, int old, int o0, int os, int nr) {
  constexpr int NS = 256 / D, RPT = ROWS / NS;
  const int nj = (nr + NS - 1) / NS;  // block-uniform
  if (nj <= 1) dense_impl<D, 1, GELU>(W, bias, in, i0, is, out, old, o0, os, nr);
  else if (nj <= 2) dense_impl<D, 2, GELU>(W, bias, in, i0, is, out, old, o0, os, nr);
  else if (nj <= 4) dense_impl<D, 4, GELU>(W, bias, in, i0, is, out, old, o0, os, nr);
  else dense_impl<D, RPT, GELU>(W, bias, in, i0, is, out, old, o0, os, nr);
}

// out[r] = LayerNorm(x[x0 + r * xs] (+ res[r0 + r * rs])) * scale + bias, r < nr; all row strides D + 1.  A thread reads and
// writes its own features only, so `out` may be `x` or `res`.
template <int D>
__device__ __forceinline__ void ln_rows(const float* x, int x0, int xs, const float* res, int r0, int rs, float* out,
                                        const float* __restrict__ scale, const float* __restrict__ bias, int nr) {
  constexpr int LD = D + 1;
  const int r = threadIdx.x >> 3, g = threadIdx.x & 7;
  const bool real = r < nr;
  const int rr = real ? r : 0;
  const float* xp = x + (x0 + rr * xs) * LD;
  const float* rp = res != nullptr ? res + (r0 + rr * rs) * LD : nullptr;
  double s = 0.0;
  for (int f = g; f < D; f += 8) s += (double)(rp != nullptr ? xp[f] + rp[f] : xp[f]);
  const double mean = sum8(s) / (double)D;
  double v = 0.0;
  for (int f = g; f < D; f += 8) {
    const double d = (double)(rp != nullptr ? xp[f] + rp[f] : xp[f]) - mean;
    v = fma(d, d, v);
  }
  const double rstd = 1.0 / sqrt(sum8(v) / (double)D + LN_EPS);
  if (real)
    for (int f = g; f < D; f += 8) {
      const double xh = ((double)(rp != nullptr ? xp[f] + rp[f] : xp[f]) - mean) * rstd;
      out[r * LD + f] = (float)fma(xh, (double)scale[f], (double)bias[f]);
    }
}

struct AttnW {
  const float *qw, *qb, *kw, *kb, *vw, *vb, *pw, *pb;
};

template <int D>
__device__ __forceinline__ AttnW attn_w(const float* a) {
  constexpr long DD = (long)D * D;
  return {a, a + DD, a + DD + D, a + 2 * DD + D, a + 2 * DD + 2 * D, a + 3 * DD + 2 * D, a + 3 * DD + 3 * D, a + 4 * DD + 3 * D};
}

// softmax in place over s[0 .. n), f64
__device__ __forceinline__ void softmax_row(double* s, int n) {
  double mx = s[0];
  for (int j = 1; j < n; ++j) mx = fmax(mx, s[j]);
  double se = 0.0;
  for (int j = 0; j < n; ++j) {
    const double ex = exp(s[j] - mx);
    s[j] = ex;
    se += ex;
  }
  const double inv = 1.0 / se;
  for (int j = 0; j < n; ++j) s[j] *= inv;
}

// Encoder self-attention over the nr rows staged in Q, K, V (LDS): y replaces q.  Ends on a barrier.
template <int D>
__device__ __forceinline__ void attn_full(const ActTask& a, float* Q, const float* K, const float* V, double* s_sc, int nr) {
  constexpr int LD = D + 1;
  const int tid = threadIdx.x, A = a.A, hd = a.hd;
  const double scale = 1.0 / sqrt((double)hd);
  for (int h = 0; h < a.H; ++h) {
    const int f0 = h * hd;
    for (int e = tid; e < nr * A; e += 256) {
      const int r = e / A, j = e - r * A;
      const int kr = r - (r % A) + j;
      double s = 0.0;
      for (int d = 0; d < hd; ++d) s = fma((double)Q[r * LD + f0 + d], (double)K[kr * LD + f0 + d], s);
      s_sc[r * LDP + j] = s * scale;
    }
    __syncthreads();
    if (tid < nr) softmax_row(s_sc + tid * LDP, A);
    __syncthreads();
    for (int e = tid; e < nr * hd; e += 256) {
      const int r = e / hd, d = e - r * hd;
      const int base = r - (r % A);
      double acc = 0.0;
      for (int j = 0; j < A; ++j) acc = fma(s_sc[r * LDP + j], (double)V[(base + j) * LD + f0 + d], acc);
      Q[r * LD + f0 + d] = (float)acc;
    }
    __syncthreads();
  }
}

// Decoder attention of row i of each of the ns samples: q in Q[s] (LDS), keys and values of the rows j <= i of sample s at
// kc / vc[(s * A + j) * D] (the cache, row i included).  y replaces q.  Ends on a barrier.
template <int D>
__device__ __forceinline__ void attn_cached(const ActTask& a, float* Q, const float* kc, const float* vc, double* s_sc, int ns, int i) {
  constexpr int LD = D + 1;
  const int tid = threadIdx.x, A = a.A, hd = a.hd, n = i + 1;
  const double scale = 1.0 / sqrt((double)hd);
  for (int h0 = 0; h0 < a.H; h0 += 32) {
    const int hc = (a.H - h0 < 32) ? (a.H - h0) : 32;
    // 8 lanes per (sample, head, key) score, lane g the features g, g + 8, ..; the trip count is block-uniform
    const int items = ns * hc * n, g = tid & 7;
    for (int e0 = 0; e0 < items; e0 += 32) {
      const int e = e0 + (tid >> 3);
      const bool real = e < items;
      const int ee = real ? e : 0;
      const int sh = ee / n, j = ee - sh * n;
      const int s = sh / hc, f0 = (h0 + sh - s * hc) * hd;
      const float* kp = kc + (long)(s * A + j) * D + f0;
      double acc = 0.0;
      for (int d = g; d < hd; d += 8) acc = fma((double)Q[s * LD + f0 + d], (double)kp[d], acc);
      acc = sum8(acc);
      if (real && g == 0) s_sc[sh * A + j] = acc * scale;
    }
    __syncthreads();
    for (int sh = tid; sh < ns * hc; sh += 256) softmax_row(s_sc + sh * A, n);
    __syncthreads();
    for (int e = tid; e < ns * hc * hd; e += 256) {
      const int s = e / (hc * hd), fd = e - s * (hc * hd);
      const int hh = fd / hd, f = h0 * hd + fd;
      const double* p = s_sc + (s * hc + hh) * A;
      double acc = 0.0;
      for (int j = 0; j < n; ++j) acc = fma(p[j], (double)vc[(long)(s * A + j) * D + f], acc);
      Q[s * LD + f] = (float)acc;
    }
    __syncthreads();
  }
}

constexpr size_t lds_bytes(int D) {
  return (size_t)(ROWS * LDP + 2 * ROWS) * sizeof(double) + (size_t)(5 * ROWS * (D + 1) + ROWS * MAX_ACT) * sizeof(float) +
         ROWS * sizeof(int);
}

// CONT: the continuous head (tanh-normal, tanh_normal.h).  Three places differ, each under `if constexpr`: the decoder's input
// row is GELU(bias + sum_k previous action[k] * W[k][:]) (GELU(bias) for agent 0), the head writes nA = action_dim means, and
// the sampling step is mava_transformer_sample_continuous_f32's.  The logits tile holds the step's means ([32][16]) and, from
// float 512 on, the group's actions so far ([32 rows][16]).
template <int D, bool CONT>
__global__ __launch_bounds__(256) void mat_act_kernel(ActTask a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int LD = D + 1, NS = 256 / D, RPT = ROWS / NS;
  constexpr long DD = (long)D * D;
  double* const s_sc = reinterpret_cast<double*>(lds);  // [32][33] scores / probabilities
  double* const s_mom = s_sc + ROWS * LDP;               // [32] mean, [32] rstd of the observation rows
  float* const X = reinterpret_cast<float*>(s_mom + 2 * ROWS);  // encoder: x, then rep
  float* const Q = X + ROWS * LD;
  float* const K = Q + ROWS * LD;
  float* const V = K + ROWS * LD;
  float* const T = V + ROWS * LD;
  float* const s_log = T + ROWS * LD;                    // [32][64] logits of the step's rows
  int* const s_act = reinterpret_cast<int*>(s_log + ROWS * MAX_ACT);  // [R] the group's actions so far
  float* const s_prev = s_log + ROWS * MAX_DIM;          // CONT: [R][16] the group's action vectors so far
  const int tid = threadIdx.x;
  const int A = a.A, O = a.O, nA = a.nA, nb = a.nb, S = a.S;

  const float* const enc = a.params;
  const float* const e_obs_w = enc + 2 * (long)O;
  const float* const e_obs_b = e_obs_w + (long)O * D;
  const float* const e_ln = e_obs_b + D;
  const float* const e_blk = e_ln + 2 * D;
  const float* const e_head = e_blk + nb * enc_block_size(D);
  const float* const dec = enc + enc_size(O, D, nb);
  const float* const d_ln = dec + (long)(nA + 1) * D;
  const float* const d_blk = d_ln + 2 * D;
  const float* const d_head = d_blk + nb * dec_block_size(D);
  float* const cache = a.cache + (long)blockIdx.x * nb * 4 * ROWS * D;

  const long groups = ((long)a.B + S - 1) / S;
  for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const long b0 = grp * S;
    const int ns = (int)((a.B - b0 < S) ? (a.B - b0) : S);
    const int nr = ns * A;
    const long row0 = b0 * A;

    // ---------------------------------------------------------------- encoder
    {  // moments of the observation rows (f64, two passes as LayerNorm has them)
      const int r = tid >> 3, g = tid & 7;
      const float* op = a.obs + (row0 + (r < nr ? r : 0)) * O;
      double s = 0.0;
      for (int f = g; f < O; f += 8) s += (double)op[f];
      const double mean = sum8(s) / (double)O;
      double v = 0.0;
      for (int f = g; f < O; f += 8) {
        const double d = (double)op[f] - mean;
        v = fma(d, d, v);
      }
      const double rstd = 1.0 / sqrt(sum8(v) / (double)O + LN_EPS);
      if (g == 0) {
        s_mom[r] = mean;
        s_mom[ROWS + r] = rstd;
      }
    }
    __syncthreads();
    {  // T = GELU(Dense(LN_O(obs))): the normalised observations are staged D features at a time in Q
      const int n = tid % D, sl = tid / D;
      float acc[RPT];
#pragma unroll
      for (int j = 0; j < RPT; ++j) acc[j] = 0.0f;
      for (int c0 = 0; c0 < O; c0 += D) {
        const int kc = (O - c0 < D) ? (O - c0) : D;
        for (int e = tid; e < ROWS * kc; e += 256) {
          const int r = e / kc, k = e - r * kc;
          float val = 0.0f;
          if (r < nr) {
            const double xh = ((double)a.obs[(row0 + r) * O + c0 + k] - s_mom[r]) * s_mom[ROWS + r];
            val = (float)fma(xh, (double)enc[c0 + k], (double)enc[O + c0 + k]);
          }
          Q[r * LD + k] = val;
        }
        __syncthreads();
        if (sl < NS)
          for (int k = 0; k < kc; ++k) {
            const float w = e_obs_w[(long)(c0 + k) * D + n];
#pragma unroll
            for (int j = 0; j < RPT; ++j) acc[j] = fmaf(Q[(sl + j * NS) * LD + k], w, acc[j]);
          }
        __syncthreads();
      }
      if (sl < NS) {
        const float b = e_obs_b[n];
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
          const int r = sl + j * NS;
          if (r < nr) T[r * LD + n] = gelu_f(acc[j] + b);
        }
      }
    }
    __syncthreads();
    ln_rows<D>(T, 0, 1, nullptr, 0, 0, X, e_ln, e_ln + D, nr);
    __syncthreads();
    for (int l = 0; l < nb; ++l) {
      const float* const bp = e_blk + l * enc_block_size(D);
      const AttnW w = attn_w<D>(bp);
      dense<D, false>(w.qw, w.qb, X, 0, 1, Q, LD, 0, 1, nr);
      dense<D, false>(w.kw, w.kb, X, 0, 1, K, LD, 0, 1, nr);
      dense<D, false>(w.vw, w.vb, X, 0, 1, V, LD, 0, 1, nr);
      __syncthreads();
      attn_full<D>(a, Q, K, V, s_sc, nr);
      dense<D, false>(w.pw, w.pb, Q, 0, 1, T, LD, 0, 1, nr);
      __syncthreads();
      ln_rows<D>(T, 0, 1, X, 0, 1, X, bp + 4 * DD + 4 * D, bp + 4 * DD + 5 * D, nr);
      __syncthreads();
      dense<D, true>(bp + 4 * DD + 6 * D, bp + 5 * DD + 6 * D, X, 0, 1, Q, LD, 0, 1, nr);
      __syncthreads();
      dense<D, false>(bp + 5 * DD + 7 * D, bp + 6 * DD + 7 * D, Q, 0, 1, T, LD, 0, 1, nr);
      __syncthreads();
      ln_rows<D>(T, 0, 1, X, 0, 1, X, bp + 6 * DD + 8 * D, bp + 6 * DD + 9 * D, nr);
      __syncthreads();
    }
    // value = Dense(1)(LN(GELU(Dense(rep))))
    dense<D, true>(e_head, e_head + DD, X, 0, 1, Q, LD, 0, 1, nr);
    __syncthreads();
    ln_rows<D>(Q, 0, 1, nullptr, 0, 0, T, e_head + DD + D, e_head + DD + 2 * D, nr);
    __syncthreads();
    if (a.value != nullptr && tid < nr) {
      const float* hw = e_head + DD + 3 * D;
      float acc = 0.0f;
      for (int k = 0; k < D; ++k) acc = fmaf(T[tid * LD + k], hw[k], acc);
      a.value[row0 + tid] = acc + hw[D];
    }
    // (T is next written two barriers from here)

    // ---------------------------------------------------------------- decoder, one agent at a time
    float* const XR = K;  // the step's rows, one per sample: current x
    float* const QR = Q;  // q / attention output / hidden
    float* const TR = T;  // branch output
    for (int i = 0; i < A; ++i) {
      if constexpr (CONT) {
        const float* const ab = dec + (long)nA * D;  // act_dense's bias follows its (nA x D) kernel
        for (int e = tid; e < ns * D; e += 256) {
          const int s = e / D, d = e - s * D;
          float acc = 0.0f;
          if (i > 0) {
            const float* pa = s_prev + (s * A + i - 1) * MAX_DIM;
            for (int k = 0; k < nA; ++k) acc = fmaf(pa[k], dec[(long)k * D + d], acc);
          }
          QR[s * LD + d] = gelu_f(acc + ab[d]);
        }
      } else {
        for (int e = tid; e < ns * D; e += 256) {
          const int s = e / D, d = e - s * D;
          const int tok = (i == 0) ? 0 : 1 + s_act[s * A + i - 1];
          QR[s * LD + d] = gelu_f(dec[(long)tok * D + d]);
        }
      }
      __syncthreads();
      ln_rows<D>(QR, 0, 1, nullptr, 0, 0, XR, d_ln, d_ln + D, ns);
      __syncthreads();
      for (int l = 0; l < nb; ++l) {
        const float* const bp = d_blk + l * dec_block_size(D);
        float* const ck = cache + (long)l * 4 * ROWS * D;
        const AttnW w1 = attn_w<D>(bp);
        dense<D, false>(w1.qw, w1.qb, XR, 0, 1, QR, LD, 0, 1, ns);
        dense<D, false>(w1.kw, w1.kb, XR, 0, 1, ck, D, i, A, ns);
        dense<D, false>(w1.vw, w1.vb, XR, 0, 1, ck + ROWS * D, D, i, A, ns);
        __syncthreads();
        attn_cached<D>(a, QR, ck, ck + ROWS * D, s_sc, ns, i);
        dense<D, false>(w1.pw, w1.pb, QR, 0, 1, TR, LD, 0, 1, ns);
        __syncthreads();
        ln_rows<D>(TR, 0, 1, XR, 0, 1, XR, bp + 4 * DD + 4 * D, bp + 4 * DD + 5 * D, ns);
        __syncthreads();
        const AttnW w2 = attn_w<D>(bp + 4 * DD + 6 * D);
        dense<D, false>(w2.qw, w2.qb, X, i, A, QR, LD, 0, 1, ns);
        dense<D, false>(w2.kw, w2.kb, XR, 0, 1, ck + 2 * ROWS * D, D, i, A, ns);
        dense<D, false>(w2.vw, w2.vb, XR, 0, 1, ck + 3 * ROWS * D, D, i, A, ns);
        __syncthreads();
        attn_cached<D>(a, QR, ck + 2 * ROWS * D, ck + 3 * ROWS * D, s_sc, ns, i);
        dense<D, false>(w2.pw, w2.pb, QR, 0, 1, TR, LD, 0, 1, ns);
        __syncthreads();
        ln_rows<D>(TR, 0, 1, X, i, A, XR, bp + 8 * DD + 10 * D, bp + 8 * DD + 11 * D, ns);
        __syncthreads();
        dense<D, true>(bp + 8 * DD + 12 * D, bp + 9 * DD + 12 * D, XR, 0, 1, QR, LD, 0, 1, ns);
        __syncthreads();
        dense<D, false>(bp + 9 * DD + 13 * D, bp + 10 * DD + 13 * D, QR, 0, 1, TR, LD, 0, 1, ns);
        __syncthreads();
        ln_rows<D>(TR, 0, 1, XR, 0, 1, XR, bp + 10 * DD + 14 * D, bp + 10 * DD + 15 * D, ns);
        __syncthreads();
      }
      dense<D, true>(d_head, d_head + DD, XR, 0, 1, QR, LD, 0, 1, ns);
      __syncthreads();
      ln_rows<D>(QR, 0, 1, nullptr, 0, 0, TR, d_head + DD + D, d_head + DD + 2 * D, ns);
      __syncthreads();
      {
        const float* hw = d_head + DD + 3 * D;
        const float* hb = hw + (long)D * nA;
        for (int e = tid; e < ns * nA; e += 256) {
          const int s = e / nA, o = e - s * nA;
          float acc = 0.0f;
          for (int k = 0; k < D; ++k) acc = fmaf(TR[s * LD + k], hw[k * nA + o], acc);
          s_log[s * (CONT ? MAX_DIM : MAX_ACT) + o] = acc + hb[o];
        }
      }
      __syncthreads();
      if constexpr (CONT) {
        if (tid < ns) {
          const long row = (b0 + tid) * A + i;
          const float* const ls = d_head + DD + 3 * D + (long)D * nA + nA;  // decoder/log_std: the last leaf
          const uint32_t gid = a.row_offset + (uint32_t)row;
          float lp = 0.0f;
          for (int o = 0; o < nA; ++o) {
            const float mean = s_log[tid * MAX_DIM + o];
            const float sc = tn::scale_of(ls[o], a.min_scale);
            const float eps = a.greedy ? 0.0f : tn::noise(gid, a.step, o, tn::STREAM_SAMPLE, a.seed_lo, a.seed_hi);
            const float act = tanhf(fmaf(sc, eps, mean));
            lp += tn::log_prob(act, mean, sc).lp;
            a.action_f[row * nA + o] = act;
            s_prev[(tid * A + i) * MAX_DIM + o] = act;
          }
          a.log_prob[row] = lp;
        }
      } else if (tid < ns) {
        const long row = (b0 + tid) * A + i;
        const RowLogitsT<1> rl = {s_log + tid * MAX_ACT, a.mask != nullptr ? a.mask + row * nA : nullptr, nA};
        const RowStats st = row_stats(rl);
        const int act = row_draw(rl, a.greedy, a.row_offset + (uint32_t)row, a.step, a.seed_lo, a.seed_hi);
        a.action[row] = act;
        a.log_prob[row] = row_log_prob(rl, st, act);
        s_act[tid * A + i] = act;
      }
      __syncthreads();
    }
  }
}

template <int D, bool CONT = false>
int launch_act(const ActTask& a, int n_blocks, hipStream_t s) {
  static bool attr_set = false;
  constexpr size_t lb = lds_bytes(D);
  if (!attr_set) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)mat_act_kernel<D, CONT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
    attr_set = true;
  }
  hipLaunchKernelGGL((mat_act_kernel<D, CONT>), dim3(n_blocks), dim3(256), lb, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

}  // namespace

extern "C" long mava_transformer_param_count(int O, int n_actions, int D, int n_block) {
  if (O < 1 || n_actions < 1 || D < 1 || n_block < 0) return -1;
  return enc_size(O, D, n_block) + dec_size(n_actions, D, n_block);
}

extern "C" size_t mava_transformer_act_workspace_bytes(int B, int A, int D, int n_block, int n_blocks) {
  (void)B;
  (void)A;
  if (D < 1 || n_block < 1 || n_block > MAX_NBLOCK || n_blocks < 1) return 0;
  return (size_t)n_blocks * n_block * 4 * ROWS * D * sizeof(float);
}

extern "C" int mava_transformer_act_f32(const float* params, const float* agents_view, const uint8_t* mask, int B, int A, int O,
                                        int n_actions, int D, int n_head, int n_block, uint64_t seed, uint32_t step,
                                        uint32_t row_offset, int greedy, int32_t* action, float* log_prob, float* value,
                                        void* workspace, size_t workspace_bytes, int n_blocks, hipStream_t s) {
  const char* who = "mava_transformer_act_f32";
  MAVA_ARG_CHECK(B >= 1 && (long)B * MAX_A < (1L << 31), 0, "%s: B=%d (at least one sample, B * 32 below 2^31)", who, B);
  MAVA_ARG_CHECK(A >= 1 && A <= MAX_A, 1, "%s: A=%d (1..%d agents)", who, A, MAX_A);
  MAVA_ARG_CHECK(D >= 32 && D % 32 == 0 && D <= MAX_D, 2, "%s: D=%d (a multiple of 32 up to %d)", who, D, MAX_D);
  MAVA_ARG_CHECK(n_head >= 1 && D % n_head == 0, 3, "%s: D=%d n_head=%d (D a multiple of n_head)", who, D, n_head);
  MAVA_ARG_CHECK(n_actions >= 1 && n_actions <= MAX_ACT, 4, "%s: n_actions=%d (1..%d)", who, n_actions, MAX_ACT);
  MAVA_ARG_CHECK(O >= 1 && O <= MAX_O, 5, "%s: O=%d (1..%d observation features)", who, O, MAX_O);
  MAVA_ARG_CHECK(n_block >= 1, 6, "%s: n_block=%d", who, n_block);
  MAVA_ARG_CHECK(n_blocks >= 1 && n_blocks <= 65536, 7, "%s: n_blocks=%d", who, n_blocks);
  MAVA_ARG_CHECK(params && agents_view && action && log_prob, 8, "%s: null pointer argument", who);
  if (n_block > MAX_NBLOCK) return 1;  // not instantiated: the caller runs the layer-wise path
  const size_t need = mava_transformer_act_workspace_bytes(B, A, D, n_block, n_blocks);
  MAVA_ARG_CHECK(workspace != nullptr && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, 9,
                 "%s: workspace of %zu bytes (16-byte aligned) required, got %zu", who, need, workspace_bytes);
  ActTask a = {};
  a.params = params; a.obs = agents_view; a.mask = mask;
  a.B = B; a.A = A; a.O = O; a.nA = n_actions; a.H = n_head; a.hd = D / n_head; a.nb = n_block;
  a.S = A >= ROWS ? 1 : ROWS / A;
  a.greedy = greedy != 0;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.step = step; a.row_offset = row_offset;
  a.action = action; a.log_prob = log_prob; a.value = value; a.cache = static_cast<float*>(workspace);
  switch (D) {
    case 32: return launch_act<32>(a, n_blocks, s);
    case 64: return launch_act<64>(a, n_blocks, s);
    case 96: return launch_act<96>(a, n_blocks, s);
    default: return launch_act<128>(a, n_blocks, s);
  }
}

extern "C" long mava_transformer_param_count_continuous(int O, int action_dim, int D, int n_block) {
  if (O < 1 || action_dim < 1 || D < 1 || n_block < 0) return -1;
  return enc_size(O, D, n_block) + dec_size(action_dim, D, n_block) + action_dim;
}

extern "C" int mava_transformer_act_continuous_f32(const float* params, const float* agents_view, int B, int A, int O, int action_dim,
                                                   int D, int n_head, int n_block, float min_scale, uint64_t seed, uint32_t step,
                                                   uint32_t row_offset, int greedy, float* action, float* log_prob, float* value,
                                                   void* workspace, size_t workspace_bytes, int n_blocks, hipStream_t s) {
  const char* who = "mava_transformer_act_continuous_f32";
  MAVA_ARG_CHECK(B >= 1 && (long)B * MAX_A < (1L << 31), 0, "%s: B=%d (at least one sample, B * 32 below 2^31)", who, B);
  MAVA_ARG_CHECK(A >= 1 && A <= MAX_A, 1, "%s: A=%d (1..%d agents)", who, A, MAX_A);
  MAVA_ARG_CHECK(D >= 32 && D % 32 == 0 && D <= MAX_D, 2, "%s: D=%d (a multiple of 32 up to %d)", who, D, MAX_D);
  MAVA_ARG_CHECK(n_head >= 1 && D % n_head == 0, 3, "%s: D=%d n_head=%d (D a multiple of n_head)", who, D, n_head);
  MAVA_ARG_CHECK(action_dim >= 1 && action_dim <= MAX_DIM && min_scale >= 0.0f, 4, "%s: action_dim=%d min_scale=%g (1..%d dimensions)", who,
                 action_dim, (double)min_scale, MAX_DIM);
  MAVA_ARG_CHECK(O >= 1 && O <= MAX_O, 5, "%s: O=%d (1..%d observation features)", who, O, MAX_O);
  MAVA_ARG_CHECK(n_block >= 1, 6, "%s: n_block=%d", who, n_block);
  MAVA_ARG_CHECK(n_blocks >= 1 && n_blocks <= 65536, 7, "%s: n_blocks=%d", who, n_blocks);
  MAVA_ARG_CHECK(params && agents_view && action && log_prob, 8, "%s: null pointer argument", who);
  if (n_block > MAX_NBLOCK) return 1;  // not instantiated: the caller runs the layer-wise path
  const size_t need = mava_transformer_act_workspace_bytes(B, A, D, n_block, n_blocks);
  MAVA_ARG_CHECK(workspace != nullptr && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, 9,
                 "%s: workspace of %zu bytes (16-byte aligned) required, got %zu", who, need, workspace_bytes);
  ActTask a = {};
  a.params = params; a.obs = agents_view;
  a.B = B; a.A = A; a.O = O; a.nA = action_dim; a.H = n_head; a.hd = D / n_head; a.nb = n_block;
  a.S = A >= ROWS ? 1 : ROWS / A;
  a.greedy = greedy != 0; a.min_scale = min_scale;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.step = step; a.row_offset = row_offset;
  a.action_f = action; a.log_prob = log_prob; a.value = value; a.cache = static_cast<float*>(workspace);
  switch (D) {
    case 32: return launch_act<32, true>(a, n_blocks, s);
    case 64: return launch_act<64, true>(a, n_blocks, s);
    case 96: return launch_act<96, true>(a, n_blocks, s);
    default: return launch_act<128, true>(a, n_blocks, s);
  }
}
