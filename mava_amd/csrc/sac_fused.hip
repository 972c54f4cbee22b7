// Soft actor-critic (ff_isac / ff_masac): the Q update and the actor update of one train step as one launch each
// (include/mava_hip.h, "soft actor-critic", mava_sac_q_update_f32 / mava_sac_actor_update_f32).
// Reference: mava/systems/sac/ff_isac.py:305-340 (update_q) and :342-365 (update_actor_and_alpha), ff_masac.py.
//
// Networks: MLPTorso [128, 128] relu without layer norm, GenericNet's flat layout [W1 (K,128) | b1 | W2 | b2 | heads].
// Arithmetic is f16x2: every product is three v_mfma_f32_32x32x16_f16 on hi + lo f16 operands with f32 accumulation
// (h2::mfma3); the Dense(1) head of a Q network and everything per row (sample, log-prob, target, loss) is f32 VALU work.
//
// Work split.  A workgroup of four waves owns one tile of 32 rows that holds IT = 32 / A whole items (IT A real rows, the
// rest zero padding), so MASAC's joint action of an item never crosses workgroups; wave w owns hidden features 32 w .. + 31
// of every layer.  Products are computed transposed (Z^T = W^T X^T): the accumulator has the batch row on the lane and the
// feature on the register (mlp_feat).  Weights are not staged: a lane reads its 8 k-values of a k-step from memory / L2 in
// operand order and splits them in registers.  Activations live in LDS in two plain layouts, written from the accumulator:
//   row image  [32 rows][128 features] f16, hi and lo plane, 272-byte rows (h2::write_image): the B operand of a product that
//              sums over features (forward layers, dX = dZ W^T) - one 16-byte read per plane;
//   col image  [128 features][32 rows] f16, hi and lo plane, 80-byte rows: both operands of X^T dZ, which sums over rows -
//              again one 16-byte read per plane, no transposed reads.
// ReLU masks are kept as 16 bits per lane and layer, so no activation stays in registers across phases.  The backward
// chains run in units of gscale = 2^ceil(log2(n_real)) (f16 low terms stay normal) and are unscaled in f32 at the slab
// store.  A padding row has dq = 0 (d head = 0), so it adds exact zeros to every gradient.
#include <float.h>

#include "h2_core.h"
#include "tanh_normal.h"

namespace {

using h2::Frag;
using h2::u8;

constexpr int THREADS = 256;
constexpr int H = 128;                          // hidden width
constexpr int MAX_D = 16, MAX_A = 16, MAX_K = 127;
constexpr uint32_t STREAM_NOISE = 0x5341434eu;  // "SACN", as mava_sac_sample_f32

constexpr int R_ROW = h2::IMG_ROW, R_PLANE = h2::IMG_PLANE, R_BYTES = h2::IMG_BYTES;  // row image
constexpr int T_ROW = 80, T_PLANE = H * T_ROW, T_BYTES = 2 * T_PLANE;                 // col image
constexpr int TY_PLANE = 32 * T_ROW, TY_BYTES = 2 * TY_PLANE;                         // col image of the 32 head outputs

// LDS map (bytes)
constexpr int L_RA = 0, L_RB = L_RA + R_BYTES;
constexpr int L_TX = L_RB + R_BYTES, L_TH1 = L_TX + T_BYTES, L_TH2 = L_TH1 + T_BYTES, L_TD2 = L_TH2 + T_BYTES, L_TD1 = L_TD2 + T_BYTES;
constexpr int L_TY = L_TD1 + T_BYTES;
constexpr int L_F32 = L_TY + TY_BYTES;
// f32 region (floats)
constexpr int F_HOUT = 0;                // [32 rows][32 head outputs]: mean | raw log_std
constexpr int F_ANEW = F_HOUT + 1024;    // [32][16] sampled action
constexpr int F_EPS = F_ANEW + 512;      // [32][16] noise
constexpr int F_LPP = F_EPS + 512;       // [8][32] log-prob partials
constexpr int F_LOGP = F_LPP + 256;      // [32]
constexpr int F_QV = F_LOGP + 32;        // [2][32] two Q values per row
constexpr int F_TGT = F_QV + 64;         // [32]
constexpr int F_DQ = F_TGT + 32;         // [32]
constexpr int F_RED = F_DQ + 32;         // [4 waves][32]
constexpr int F_DXA = F_RED + 128;       // [2][32][16] own-action slice of dQ / dx
constexpr int F_END = F_DXA + 1024;
constexpr int LDS_BYTES = L_F32 + 4 * F_END;
static_assert(LDS_BYTES <= 163840, "LDS");

#ifdef __HIP_DEVICE_COMPILE__
#define NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PACKED_F32
#endif

__device__ __forceinline__ int featq(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

struct Net {  // offsets of one [128, 128] network in the flat layout
  const float *w1, *b1, *w2, *b2, *head;
};
__device__ __forceinline__ Net net_of(const float* p, int K) {
  Net n;
  n.w1 = p;
  n.b1 = p + (long)K * H;
  n.w2 = n.b1 + H;
  n.b2 = n.w2 + H * H;
  n.head = n.b2 + H;
  return n;
}
struct GNet {  // the same offsets in a gradient slab
  float *w1, *b1, *w2, *b2, *head;
};
__device__ __forceinline__ GNet gnet_of(float* p, int K) {
  GNet n;
  n.w1 = p;
  n.b1 = p + (long)K * H;
  n.w2 = n.b1 + H;
  n.b2 = n.w2 + H * H;
  n.head = n.b2 + H;
  return n;
}
__host__ __device__ __forceinline__ long q_params(int K) { return (long)K * H + H + H * H + H + H + 1; }
__host__ __device__ __forceinline__ long actor_params(int O, int D) { return (long)O * H + H + H * H + H + 2L * (H * D + D); }

// ---- the x images ------------------------------------------------------------------------------------------------------
struct XSrc {
  const float* state;   // (., sdim) row-major
  int sdim, per_item;   // state row = item (a global state) or real row
  const float* act_g;   // stored actions (B A, D), or null
  const float* act_l;   // LDS [32][16]: the tile's new actions, or null
  int joint, all_new;   // joint: every agent's action of the item; all_new: all from act_l, else the row's own slot alone
};
__device__ __forceinline__ float x_value(const XSrc& x, int row0, int lr, int f, int A, int D) {
  if (f < x.sdim) return x.state[(long)(x.per_item ? (row0 + lr) / A : row0 + lr) * x.sdim + f];
  const int kk = f - x.sdim;
  if (!x.joint) return x.act_l != nullptr ? x.act_l[lr * 16 + kk] : x.act_g[(long)(row0 + lr) * D + kk];
  const int j = kk / D, d = kk - j * D, lj = (lr / A) * A + j;
  const bool local = x.act_l != nullptr && (x.all_new || j == lr % A);
  return local ? x.act_l[lj * 16 + d] : x.act_g[(long)(row0 + lj) * D + d];
}
// all 128 features of all 32 rows are written: zeros past K and in the padding rows
__device__ __forceinline__ void build_x(u8* R, u8* T, const XSrc& x, int K, int row0, int nrows, int A, int D, int tid) {
  for (int i = tid; i < 32 * H; i += THREADS) {
    const int lr = i >> 7, f = i & 127;
    const float v = (lr < nrows && f < K) ? x_value(x, row0, lr, f, A, D) : 0.0f;
    _Float16 a, b;
    h2::split1(v, a, b);
    *reinterpret_cast<_Float16*>(R + lr * R_ROW + 2 * f) = a;
    *reinterpret_cast<_Float16*>(R + R_PLANE + lr * R_ROW + 2 * f) = b;
    if (T != nullptr) {
      *reinterpret_cast<_Float16*>(T + f * T_ROW + 2 * lr) = a;
      *reinterpret_cast<_Float16*>(T + T_PLANE + f * T_ROW + 2 * lr) = b;
    }
  }
}

// ---- products ----------------------------------------------------------------------------------------------------------
// Z^T[32 w + f][row] = bias + sum_k W[k][32 w + f] X[row][k], X from a row image
__device__ __forceinline__ f32x16 fwd_layer(const float* __restrict__ W, const float* __restrict__ bias, int K, const u8* img, int w,
                                            int r, int h) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = bias[32 * w + featq(q, h)];
  const int steps = (K + 15) >> 4;
  float carry = 0.0f;
  for (int s = 0; s < steps; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 16 * s + 8 * h + e;
      v[e] = W[(long)(k < K ? k : K - 1) * H + 32 * w + r];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (16 * s + 8 * h + e >= K) v[e] = 0.0f;
    const Frag a = h2::split8_carry(v, carry);
    const Frag b = h2::read_row_frag(img, R_PLANE, r * R_ROW + 2 * (16 * s + 8 * h));
    acc = h2::mfma3(a, b, acc);
  }
  return acc;
}
__device__ __forceinline__ uint32_t relu_mask(f32x16& acc) {
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    if (acc[q] > 0.0f) m |= 1u << q;
    else acc[q] = 0.0f;
  }
  return m;
}
__device__ __forceinline__ void apply_mask(f32x16& acc, uint32_t m) {
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (!((m >> q) & 1u)) acc[q] = 0.0f;
}
// accumulator tile -> row image and / or col image
__device__ __forceinline__ void put_images(const f32x16& acc, u8* R, u8* T, int w, int r, int h) {
  if (R != nullptr) {
    h2::half4 ph[4], pl[4];
    h2::write_image(R, r, 32 * w + 4 * h, acc, ph, pl);
  }
  if (T != nullptr) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      _Float16 a, b;
      h2::split1(acc[q], a, b);
      u8* p = T + (32 * w + featq(q, h)) * T_ROW + 2 * r;
      *reinterpret_cast<_Float16*>(p) = a;
      *reinterpret_cast<_Float16*>(p + T_PLANE) = b;
    }
  }
}
// dX^T[32 w + i][row] = sum_n W2[32 w + i][n] dZ[row][n], dZ from a row image
__device__ __forceinline__ f32x16 bwd_w2(const float* __restrict__ W2, const u8* img, int w, int r, int h) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll 2
  for (int s = 0; s < 8; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = W2[(32 * w + r) * H + 16 * s + 8 * h + e];
    const Frag a = h2::split8(v);
    const Frag b = h2::read_row_frag(img, R_PLANE, r * R_ROW + 2 * (16 * s + 8 * h));
    acc = h2::mfma3(a, b, acc);
  }
  return acc;
}
// out[k][32 w + n] = unscale sum_row X[row][k] dZ[row][32 w + n] for k < K: both operands from col images
__device__ __forceinline__ void wgrad(const u8* TA, const u8* TB, int K, float* __restrict__ out, float unscale, int w, int r, int h) {
  const Frag b0 = h2::read_row_frag(TB, T_PLANE, (32 * w + r) * T_ROW + 16 * h);
  const Frag b1 = h2::read_row_frag(TB, T_PLANE, (32 * w + r) * T_ROW + 32 + 16 * h);
  const int tiles = (K + 31) >> 5;
  for (int t = 0; t < tiles; ++t) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    acc = h2::mfma3(h2::read_row_frag(TA, T_PLANE, (32 * t + r) * T_ROW + 16 * h), b0, acc);
    acc = h2::mfma3(h2::read_row_frag(TA, T_PLANE, (32 * t + r) * T_ROW + 32 + 16 * h), b1, acc);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int k = 32 * t + featq(q, h);
      if (k < K) out[(long)k * H + 32 * w + r] = acc[q] * unscale;
    }
  }
}
// out[f] = unscale sum_row dZ[row][f], f < n, from a col image
__device__ __forceinline__ void bias_grad(const u8* T, int plane, int n, float* __restrict__ out, float unscale, int tid) {
  if (tid < n) {
    float s = 0.0f;
#pragma unroll 8
    for (int row = 0; row < 32; ++row)
      s += (float)*reinterpret_cast<const _Float16*>(T + tid * T_ROW + 2 * row) +
           (float)*reinterpret_cast<const _Float16*>(T + plane + tid * T_ROW + 2 * row);
    out[tid] = s * unscale;
  }
}
// the Dense(1) head: each wave's share of sum_f h2[row][f] w3[f] -> red[w][row]
__device__ __forceinline__ void q_head_partial(const f32x16& a, const float* __restrict__ w3, float* red, int w, int r, int h) {
  float p = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; ++q) p = fmaf(a[q], w3[32 * w + featq(q, h)], p);
  p += __shfl_xor(p, 32, 64);
  if (h == 0) red[w * 32 + r] = p;
}

// the actor's two heads as one 32-wide output o: mean (o < D) | raw log_std (D <= o < 2 D) | zeros
struct Heads {
  const float *wm, *bm, *ws, *bs;
};
__device__ __forceinline__ Heads heads_of(const float* head, int D) {
  Heads x;
  x.wm = head;
  x.bm = head + H * D;
  x.ws = x.bm + D;
  x.bs = x.ws + H * D;
  return x;
}
__device__ __forceinline__ float head_w(const Heads& x, int f, int o, int D) {
  return o < D ? x.wm[f * D + o] : (o < 2 * D ? x.ws[f * D + o - D] : 0.0f);
}
__device__ __forceinline__ f32x16 head_fwd(const Heads& x, int D, const u8* img, int r, int h) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int o = featq(q, h);
    acc[q] = o < D ? x.bm[o] : (o < 2 * D ? x.bs[o - D] : 0.0f);
  }
#pragma unroll 2
  for (int s = 0; s < 8; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = head_w(x, 16 * s + 8 * h + e, r, D);
    acc = h2::mfma3(h2::split8(v), h2::read_row_frag(img, R_PLANE, r * R_ROW + 2 * (16 * s + 8 * h)), acc);
  }
  return acc;
}

// the actor on a row image of its input -> F_HOUT; h1 / h2 images and masks where asked.  RA holds x on entry, h2 on exit.
__device__ __forceinline__ void actor_forward(const float* actor, int O, int D, u8* lds, float* f32, u8* TH1, u8* TH2, uint32_t& m1,
                                              uint32_t& m2, int w, int r, int h) {
  const Net n = net_of(actor, O);
  f32x16 acc = fwd_layer(n.w1, n.b1, O, lds + L_RA, w, r, h);
  m1 = relu_mask(acc);
  put_images(acc, lds + L_RB, TH1, w, r, h);
  __syncthreads();
  acc = fwd_layer(n.w2, n.b2, H, lds + L_RB, w, r, h);
  m2 = relu_mask(acc);
  put_images(acc, lds + L_RA, TH2, w, r, h);  // (every wave has left layer 1, which read RA, at the barrier above)
  __syncthreads();
  if (w == 0) {
    const f32x16 y = head_fwd(heads_of(n.head, D), D, lds + L_RA, r, h);
#pragma unroll
    for (int q = 0; q < 16; ++q) f32[F_HOUT + r * 32 + featq(q, h)] = y[q];
  }
  __syncthreads();
}
// a = tanh(mean + scale eps) and the summed log-prob per row: F_ANEW, F_EPS, F_LOGP (zeros in padding rows)
__device__ __forceinline__ void sample_rows(float* f32, int D, float min_scale, int row0, int nrows, uint32_t k0, uint32_t k1,
                                            uint32_t step, float* __restrict__ eps_out, int tid) {
  const int row = tid & 31, g = tid >> 5;
  const bool valid = row < nrows;
  float lp = 0.0f;
  for (int d = g; d < D; d += 8) {
    float a = 0.0f, e = 0.0f;
    if (valid) {
      const float mu = f32[F_HOUT + row * 32 + d], scale = tn::scale_of(f32[F_HOUT + row * 32 + D + d], min_scale);
      e = tn::noise((uint32_t)(row0 + row), step, d, STREAM_NOISE, k0, k1);
      a = tanhf(mu + scale * e);
      lp += tn::log_prob(a, mu, scale).lp;
      if (eps_out != nullptr) eps_out[(long)(row0 + row) * D + d] = e;
    }
    f32[F_ANEW + row * 16 + d] = a;
    f32[F_EPS + row * 16 + d] = e;
  }
  f32[F_LPP + g * 32 + row] = lp;
  __syncthreads();
  if (tid < 32) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += f32[F_LPP + k * 32 + tid];
    f32[F_LOGP + tid] = s;
  }
  __syncthreads();
}
__device__ __forceinline__ float half_sum32(float v) {  // over lanes 0..31 of a wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Batch {
  const float *obs, *next_obs, *action, *reward, *gs, *next_gs;
  const uint8_t* done;
};

// ---- kernel 1: update_q up to the gradients.  Block (t, i): tile t, online network Q_i ------------------------------------
__global__ __launch_bounds__(THREADS) NO_PACKED_F32 void sac_q_update_kernel(
    int joint, int BA, int A, int O, int D, int S, int IT, Batch b, const float* __restrict__ actor, const float* __restrict__ qon,
    const float* __restrict__ qtg, const float* __restrict__ log_alpha, float gamma, float min_scale, float gscale, uint32_t k0,
    uint32_t k1, uint32_t step, float* __restrict__ slab, long slab_stride, float* __restrict__ partials, float* __restrict__ target_out,
    float* __restrict__ eps_out) {
  extern __shared__ __attribute__((aligned(16))) u8 lds[];
  float* f32 = reinterpret_cast<float*>(lds + L_F32);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int t = blockIdx.x, qi = blockIdx.y;
  const int row0 = t * IT * A, nrows = min(IT * A, BA - row0);
  const int Kq = joint ? S + A * D : O + D;
  const long Pq = q_params(Kq);
  const float inv_n = 1.0f / (float)BA;

  // the actor on next_obs, its sample and log-prob
  XSrc xs = {b.next_obs, O, 0, nullptr, nullptr, 0, 0};
  build_x(lds + L_RA, nullptr, xs, O, row0, nrows, A, D, tid);
  __syncthreads();
  uint32_t m1, m2;
  actor_forward(actor, O, D, lds, f32, nullptr, nullptr, m1, m2, w, r, h);
  sample_rows(f32, D, min_scale, row0, nrows, k0, k1, step, qi == 0 ? eps_out : nullptr, tid);

  // [next state | next (joint) action] through both target networks
  XSrc xn = {joint ? b.next_gs : b.next_obs, joint ? S : O, joint, nullptr, f32 + F_ANEW, joint, 1};
  build_x(lds + L_RA, nullptr, xn, Kq, row0, nrows, A, D, tid);
  __syncthreads();
  for (int k = 0; k < 2; ++k) {
    const Net n = net_of(qtg + k * Pq, Kq);
    f32x16 acc = fwd_layer(n.w1, n.b1, Kq, lds + L_RA, w, r, h);
    relu_mask(acc);
    put_images(acc, lds + L_RB, nullptr, w, r, h);
    __syncthreads();
    acc = fwd_layer(n.w2, n.b2, H, lds + L_RB, w, r, h);
    relu_mask(acc);
    q_head_partial(acc, n.head, f32 + F_RED, w, r, h);
    __syncthreads();  // (also: every wave has left layer 2, so RB may be written again)
    if (tid < 32) f32[F_QV + k * 32 + tid] = f32[F_RED + tid] + f32[F_RED + 32 + tid] + f32[F_RED + 64 + tid] + f32[F_RED + 96 + tid] + n.head[H];
    __syncthreads();
  }
  if (tid < 32) {
    float tg = 0.0f;
    if (tid < nrows) {
      const int row = row0 + tid;
      const float next_q = fminf(f32[F_QV + tid], f32[F_QV + 32 + tid]) - expf(log_alpha[row % A]) * f32[F_LOGP + tid];
      tg = b.reward[row] + (1.0f - (float)b.done[row]) * gamma * next_q;
      if (target_out != nullptr && qi == 0) target_out[row] = tg;
    }
    f32[F_TGT + tid] = tg;
  }

  // [state | stored (joint) action] through the online network Q_i, activations kept
  XSrc xq = {joint ? b.gs : b.obs, joint ? S : O, joint, b.action, nullptr, joint, 0};
  build_x(lds + L_RA, lds + L_TX, xq, Kq, row0, nrows, A, D, tid);
  __syncthreads();
  const Net n = net_of(qon + qi * Pq, Kq);
  const GNet gn = gnet_of(slab + (long)t * slab_stride + qi * Pq, Kq);
  f32x16 acc = fwd_layer(n.w1, n.b1, Kq, lds + L_RA, w, r, h);
  m1 = relu_mask(acc);
  put_images(acc, lds + L_RB, lds + L_TH1, w, r, h);
  __syncthreads();
  acc = fwd_layer(n.w2, n.b2, H, lds + L_RB, w, r, h);
  m2 = relu_mask(acc);
  put_images(acc, nullptr, lds + L_TH2, w, r, h);
  q_head_partial(acc, n.head, f32 + F_RED, w, r, h);
  __syncthreads();
  if (tid < 64) {  // wave 0: the loss, dq and the metric partials
    float e2 = 0.0f, qs = 0.0f, dq = 0.0f;
    if (tid < nrows) {
      const float q = f32[F_RED + tid] + f32[F_RED + 32 + tid] + f32[F_RED + 64 + tid] + f32[F_RED + 96 + tid] + n.head[H];
      const float e = q - f32[F_TGT + tid];
      e2 = e * e;
      qs = q;
      dq = 2.0f * e * inv_n * gscale;
    }
    if (tid < 32) f32[F_DQ + tid] = dq;
    e2 = half_sum32(e2);
    qs = half_sum32(qs);
    if (tid == 0) {
      partials[t * 4 + qi] = e2 * inv_n;
      partials[t * 4 + 2 + qi] = qs * inv_n;
    }
  }
  __syncthreads();

  // backward: head, layer 2, layer 1
  const float unscale = 1.0f / gscale;
  if (tid < H) {  // d W3[f] = sum_row h2[row][f] dq[row]; d b3 = sum_row dq[row]
    float s = 0.0f, sb = 0.0f;
    const u8* T = lds + L_TH2;
    for (int row = 0; row < 32; ++row) {
      const float dq = f32[F_DQ + row];
      s += ((float)*reinterpret_cast<const _Float16*>(T + tid * T_ROW + 2 * row) +
            (float)*reinterpret_cast<const _Float16*>(T + T_PLANE + tid * T_ROW + 2 * row)) * dq;
      sb += dq;
    }
    gn.head[tid] = s * unscale;
    if (tid == 0) gn.head[H] = sb * unscale;
  }
  {
    const float dq = f32[F_DQ + r];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = ((m2 >> q) & 1u) ? dq * n.head[32 * w + featq(q, h)] : 0.0f;
  }
  put_images(acc, lds + L_RB, lds + L_TD2, w, r, h);  // (RB: layer 2 was left at the barrier after the head)
  __syncthreads();
  wgrad(lds + L_TH1, lds + L_TD2, H, gn.w2, unscale, w, r, h);
  bias_grad(lds + L_TD2, T_PLANE, H, gn.b2, unscale, tid);
  acc = bwd_w2(n.w2, lds + L_RB, w, r, h);
  apply_mask(acc, m1);
  put_images(acc, nullptr, lds + L_TD1, w, r, h);
  __syncthreads();
  wgrad(lds + L_TX, lds + L_TD1, Kq, gn.w1, unscale, w, r, h);
  bias_grad(lds + L_TD1, T_PLANE, H, gn.b1, unscale, tid);
}

// ---- kernel 2: the actor update up to the gradients (mode 0), or forward + sample + log-prob alone (mode 1) ---------------------
__global__ __launch_bounds__(THREADS) NO_PACKED_F32 void sac_actor_update_kernel(
    int mode, int joint, int BA, int A, int O, int D, int S, int IT, Batch b, const float* __restrict__ actor,
    const float* __restrict__ qon, const float* __restrict__ log_alpha, float min_scale, float gscale, uint32_t k0, uint32_t k1,
    uint32_t step, float* __restrict__ slab, long slab_stride, float* __restrict__ partials, float* __restrict__ logp_out,
    float* __restrict__ eps_out) {
  extern __shared__ __attribute__((aligned(16))) u8 lds[];
  float* f32 = reinterpret_cast<float*>(lds + L_F32);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int t = blockIdx.x;
  const int row0 = t * IT * A, nrows = min(IT * A, BA - row0);
  const int Kq = joint ? S + A * D : O + D, a_off = joint ? S : O, Wact = joint ? A * D : D;
  const long Pq = q_params(Kq);
  const float inv_n = 1.0f / (float)BA;

  XSrc xs = {b.obs, O, 0, nullptr, nullptr, 0, 0};
  build_x(lds + L_RA, mode == 0 ? lds + L_TX : nullptr, xs, O, row0, nrows, A, D, tid);
  __syncthreads();
  uint32_t m1, m2;
  actor_forward(actor, O, D, lds, f32, mode == 0 ? lds + L_TH1 : nullptr, mode == 0 ? lds + L_TH2 : nullptr, m1, m2, w, r, h);
  sample_rows(f32, D, min_scale, row0, nrows, k0, k1, step, eps_out, tid);
  if (mode != 0) {
    if (tid < nrows && logp_out != nullptr) logp_out[row0 + tid] = f32[F_LOGP + tid];
    return;
  }

  // both online Q networks on [obs | new action] / [state | joint action, own slot new]: Q and d Q / d own action
  XSrc xq = {joint ? b.gs : b.obs, joint ? S : O, joint, b.action, f32 + F_ANEW, joint, 0};
  build_x(lds + L_RA, nullptr, xq, Kq, row0, nrows, A, D, tid);
  __syncthreads();
  for (int k = 0; k < 2; ++k) {
    const Net n = net_of(qon + k * Pq, Kq);
    f32x16 acc = fwd_layer(n.w1, n.b1, Kq, lds + L_RA, w, r, h);
    const uint32_t q1m = relu_mask(acc);
    put_images(acc, lds + L_RB, nullptr, w, r, h);
    __syncthreads();
    acc = fwd_layer(n.w2, n.b2, H, lds + L_RB, w, r, h);
    const uint32_t q2m = relu_mask(acc);
    q_head_partial(acc, n.head, f32 + F_RED, w, r, h);
    __syncthreads();
    if (tid < 32) f32[F_QV + k * 32 + tid] = f32[F_RED + tid] + f32[F_RED + 32 + tid] + f32[F_RED + 64 + tid] + f32[F_RED + 96 + tid] + n.head[H];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = ((q2m >> q) & 1u) ? n.head[32 * w + featq(q, h)] : 0.0f;  // d sum(Q) / d z2
    put_images(acc, lds + L_RB, nullptr, w, r, h);
    __syncthreads();
    acc = bwd_w2(n.w2, lds + L_RB, w, r, h);
    apply_mask(acc, q1m);
    __syncthreads();  // every wave has read dz2 before dz1 replaces it
    put_images(acc, lds + L_RB, nullptr, w, r, h);
    __syncthreads();
    if (32 * w < Wact) {  // wave w: action features a_off + 32 w .. + 31 of dX = dZ1 W1^T
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
      const int kx = a_off + 32 * w + r;
#pragma unroll 2
      for (int s = 0; s < 8; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = n.w1[(long)(kx < Kq ? kx : Kq - 1) * H + 16 * s + 8 * h + e];
        if (kx >= Kq) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0.0f;
        }
        acc = h2::mfma3(h2::split8(v), h2::read_row_frag(lds + L_RB, R_PLANE, r * R_ROW + 2 * (16 * s + 8 * h)), acc);
      }
      const int own0 = joint ? (r % A) * D : 0;  // (row0 is a multiple of A: the agent of tile row r is r % A)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int d = 32 * w + featq(q, h) - own0;
        if (d >= 0 && d < D) f32[F_DXA + k * 512 + r * 16 + d] = acc[q];
      }
    }
    __syncthreads();
  }

  // actor_loss_fn differentiated through the sample (as mava_sac_actor_grad_f32): d mean | d raw log_std -> RA, TY
  for (int i = tid; i < 32 * 32; i += THREADS) {
    const int a = i >> 5, c = i & 31;
    *reinterpret_cast<_Float16*>(lds + L_RA + a * R_ROW + 2 * c) = (_Float16)0.0f;
    *reinterpret_cast<_Float16*>(lds + L_RA + R_PLANE + a * R_ROW + 2 * c) = (_Float16)0.0f;
    *reinterpret_cast<_Float16*>(lds + L_TY + a * T_ROW + 2 * c) = (_Float16)0.0f;
    *reinterpret_cast<_Float16*>(lds + L_TY + TY_PLANE + a * T_ROW + 2 * c) = (_Float16)0.0f;
  }
  __syncthreads();
  {
    const int row = tid & 31, g = tid >> 5;
    const bool valid = row < nrows;
    const float alpha = expf(log_alpha[row % A]);
    const bool first = f32[F_QV + row] <= f32[F_QV + 32 + row];
    for (int d = g; d < D; d += 8) {
      float gm = 0.0f, gs = 0.0f;
      if (valid) {
        const float mu = f32[F_HOUT + row * 32 + d], raw = f32[F_HOUT + row * 32 + D + d], scale = tn::scale_of(raw, min_scale);
        const float a = f32[F_ANEW + row * 16 + d], e = f32[F_EPS + row * 16 + d];
        const tn::LogProb o = tn::log_prob(a, mu, scale);
        float lm, ls;
        if (a <= -tn::THRESH || a >= tn::THRESH) {
          lm = o.dmean; ls = o.dscale;
        } else {
          lm = 2.0f * a; ls = -1.0f / scale + 2.0f * a * e;
        }
        const float dq_da = f32[F_DXA + (first ? 0 : 512) + row * 16 + d] * (1.0f - a * a);
        gm = (alpha * lm - dq_da) * inv_n * gscale;
        gs = (alpha * ls - dq_da * e) * tn::sigmoid(raw) * inv_n * gscale;
      }
      _Float16 hi, lo;
      h2::split1(gm, hi, lo);
      *reinterpret_cast<_Float16*>(lds + L_RA + row * R_ROW + 2 * d) = hi;
      *reinterpret_cast<_Float16*>(lds + L_RA + R_PLANE + row * R_ROW + 2 * d) = lo;
      *reinterpret_cast<_Float16*>(lds + L_TY + d * T_ROW + 2 * row) = hi;
      *reinterpret_cast<_Float16*>(lds + L_TY + TY_PLANE + d * T_ROW + 2 * row) = lo;
      h2::split1(gs, hi, lo);
      *reinterpret_cast<_Float16*>(lds + L_RA + row * R_ROW + 2 * (D + d)) = hi;
      *reinterpret_cast<_Float16*>(lds + L_RA + R_PLANE + row * R_ROW + 2 * (D + d)) = lo;
      *reinterpret_cast<_Float16*>(lds + L_TY + (D + d) * T_ROW + 2 * row) = hi;
      *reinterpret_cast<_Float16*>(lds + L_TY + TY_PLANE + (D + d) * T_ROW + 2 * row) = lo;
    }
    if (tid < 64) {
      float v1 = 0.0f, v2 = 0.0f;
      if (tid < nrows) {
        v2 = f32[F_LOGP + tid];
        v1 = alpha * v2 - fminf(f32[F_QV + tid], f32[F_QV + 32 + tid]);
      }
      v1 = half_sum32(v1);
      v2 = half_sum32(v2);
      if (tid == 0) {
        partials[t * 2] = v1 * inv_n;
        partials[t * 2 + 1] = v2 * inv_n;
      }
    }
  }
  __syncthreads();

  // the actor's backward chain: heads, layer 2, layer 1
  const float unscale = 1.0f / gscale;
  const Net n = net_of(actor, O);
  const GNet gn = gnet_of(slab + (long)t * slab_stride, O);
  const Heads hd = heads_of(n.head, D);
  float* gwm = gn.head;
  float* gbm = gwm + H * D;
  float* gws = gbm + D;
  float* gbs = gws + H * D;
  {  // d Wm / d Ws[32 w + f][o] = sum_row h2[row][f] dY[row][o]
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      acc = h2::mfma3(h2::read_row_frag(lds + L_TH2, T_PLANE, (32 * w + r) * T_ROW + 32 * s + 16 * h),
                      h2::read_row_frag(lds + L_TY, TY_PLANE, r * T_ROW + 32 * s + 16 * h), acc);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int f = 32 * w + featq(q, h);
      if (r < D) gwm[f * D + r] = acc[q] * unscale;
      else if (r < 2 * D) gws[f * D + r - D] = acc[q] * unscale;
    }
    bias_grad(lds + L_TY, TY_PLANE, D, gbm, unscale, tid);
    bias_grad(lds + L_TY + D * T_ROW, TY_PLANE, D, gbs, unscale, tid);
    // d h2 = dY Wh^T, masked
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = head_w(hd, 32 * w + r, 16 * s + 8 * h + e, D);
      acc = h2::mfma3(h2::split8(v), h2::read_row_frag(lds + L_RA, R_PLANE, r * R_ROW + 2 * (16 * s + 8 * h)), acc);
    }
    apply_mask(acc, m2);
    put_images(acc, lds + L_RB, lds + L_TD2, w, r, h);
  }
  __syncthreads();
  wgrad(lds + L_TH1, lds + L_TD2, H, gn.w2, unscale, w, r, h);
  bias_grad(lds + L_TD2, T_PLANE, H, gn.b2, unscale, tid);
  f32x16 acc = bwd_w2(n.w2, lds + L_RB, w, r, h);
  apply_mask(acc, m1);
  put_images(acc, nullptr, lds + L_TD1, w, r, h);
  __syncthreads();
  wgrad(lds + L_TX, lds + L_TD1, O, gn.w1, unscale, w, r, h);
  bias_grad(lds + L_TD1, T_PLANE, H, gn.b1, unscale, tid);
}

inline bool served(int A, int O, int D, int S, int joint) {
  const int Kq = joint ? S + A * D : O + D;
  return D <= MAX_D && A <= MAX_A && O <= MAX_K && Kq <= MAX_K;
}
inline float pow2_at_least(int n) {
  float s = 1.0f;
  while (s < (float)n) s *= 2.0f;
  return s;
}

}  // namespace

extern "C" int mava_sac_q_update_f32(int joint, int B, int A, int O, int action_dim, int S, const float* obs, const float* next_obs,
                                     const float* action, const float* reward, const uint8_t* done, const float* gs,
                                     const float* next_gs, const float* actor, const float* q, const float* q_target,
                                     const float* log_alpha, float gamma, float min_scale, uint64_t seed, uint32_t step, float* slab,
                                     long slab_stride, float* partials, float* target, float* eps, hipStream_t s) {
  const int D = action_dim;
  MAVA_ARG_CHECK(B >= 1 && A >= 1 && O >= 1 && D >= 1 && S >= 0 && (long)B * A < (1L << 24), 0,
                 "mava_sac_q_update_f32: bad shape B=%d A=%d O=%d action_dim=%d S=%d", B, A, O, D, S);
  MAVA_ARG_CHECK(!joint || S >= 1, 1, "mava_sac_q_update_f32: joint needs a global state (S=%d)", S);
  if (!served(A, O, D, S, joint)) return 1;
  const int Kq = joint ? S + A * D : O + D;
  MAVA_ARG_CHECK(slab_stride >= 2 * q_params(Kq), 2, "mava_sac_q_update_f32: slab_stride=%ld is below the %ld parameters of [q1 | q2]",
                 slab_stride, 2 * q_params(Kq));
  MAVA_ARG_CHECK(obs && next_obs && action && reward && done && actor && q && q_target && log_alpha && slab && partials, 3,
                 "mava_sac_q_update_f32: null pointer");
  MAVA_ARG_CHECK(!joint || (gs && next_gs), 4, "mava_sac_q_update_f32: joint needs gs / next_gs");
  MAVA_ARG_CHECK(min_scale >= 0.0f, 5, "mava_sac_q_update_f32: min_scale=%g is negative", (double)min_scale);
  const int IT = 32 / A, n_tiles = (B + IT - 1) / IT;
  static bool attr = false;
  if (!attr) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)sac_q_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr = true;
  }
  const Batch b = {obs, next_obs, action, reward, gs, next_gs, done};
  hipLaunchKernelGGL(sac_q_update_kernel, dim3(n_tiles, 2), dim3(THREADS), LDS_BYTES, s, joint ? 1 : 0, B * A, A, O, D, S, IT, b, actor, q,
                     q_target, log_alpha, gamma, min_scale, pow2_at_least(B * A), (uint32_t)seed, (uint32_t)(seed >> 32), step, slab,
                     slab_stride, partials, target, eps);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_sac_actor_update_f32(int mode, int joint, int B, int A, int O, int action_dim, int S, const float* obs,
                                         const float* action, const float* gs, const float* actor, const float* q,
                                         const float* log_alpha, float min_scale, uint64_t seed, uint32_t step, float* slab,
                                         long slab_stride, float* partials, float* log_prob, float* eps, hipStream_t s) {
  const int D = action_dim;
  MAVA_ARG_CHECK((mode == 0 || mode == 1) && B >= 1 && A >= 1 && O >= 1 && D >= 1 && S >= 0 && (long)B * A < (1L << 24), 0,
                 "mava_sac_actor_update_f32: bad shape mode=%d B=%d A=%d O=%d action_dim=%d S=%d", mode, B, A, O, D, S);
  MAVA_ARG_CHECK(!joint || S >= 1, 1, "mava_sac_actor_update_f32: joint needs a global state (S=%d)", S);
  if (!served(A, O, D, S, joint)) return 1;
  MAVA_ARG_CHECK(obs && actor, 2, "mava_sac_actor_update_f32: null pointer");
  if (mode == 0) {
    MAVA_ARG_CHECK(action && q && log_alpha && slab && partials && (!joint || gs), 3, "mava_sac_actor_update_f32: mode 0: null pointer");
    MAVA_ARG_CHECK(slab_stride >= actor_params(O, D), 4, "mava_sac_actor_update_f32: slab_stride=%ld is below the actor's %ld parameters",
                   slab_stride, actor_params(O, D));
  } else {
    MAVA_ARG_CHECK(log_prob != nullptr, 3, "mava_sac_actor_update_f32: mode 1 needs log_prob");
  }
  MAVA_ARG_CHECK(min_scale >= 0.0f, 5, "mava_sac_actor_update_f32: min_scale=%g is negative", (double)min_scale);
  const int IT = 32 / A, n_tiles = (B + IT - 1) / IT;
  static bool attr = false;
  if (!attr) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)sac_actor_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr = true;
  }
  const Batch b = {obs, nullptr, action, nullptr, gs, nullptr, nullptr};
  hipLaunchKernelGGL(sac_actor_update_kernel, dim3(n_tiles), dim3(THREADS), LDS_BYTES, s, mode, joint ? 1 : 0, B * A, A, O, D, S, IT, b,
                     actor, q, log_alpha, min_scale, pow2_at_least(B * A), (uint32_t)seed, (uint32_t)(seed >> 32), step, slab, slab_stride,
                     partials, log_prob, eps);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
