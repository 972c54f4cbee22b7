// rec_qmix: everything QMIXLearner._loss does for the state-conditioned mixer as ONE launch (include/mava_hip.h, "value
// decomposition", mava_qmix_mixer_update_f32): select / argmax, the four hypernetworks on the online parameters and `state`
// and on the target parameters and `next_state`, both mixers, the TD error, dq, and the backward pass through the online
// mixer and its hypernetworks into per-block gradient slabs.  Semantics of the per-row part are mava_qmix_td_f32's (qmix.hip).
//
// Arithmetic is f16x2: every product is three v_mfma_f32_32x32x16_f16 on hi + lo f16 operands with f32 accumulation
// (h2::mfma3); the Em -> 1 head of the b2 net and everything per row is f32 VALU work, the sums over agents and over the
// embedding run in f64 as in qmix.hip.
//
// Rows.  Agent rows are t * Rp + b * A + j, a mixer row is t * Bp + b (Bp = ceil32(B), b >= B padding).  The A agent rows of a
// sample are contiguous, so a mixer row's state is A * O consecutive floats of obs: the kernel stages it from the sample, no
// state matrix exists.
//
// Work split.  A workgroup of four waves owns one tile of 32 mixer rows at a time (tiles blockIdx.x, + gridDim.x, ..: a
// persistent block owns ONE gradient slab and adds its tiles into it in tile order, so the result does not depend on timing).
// The four first layers are one product over the concatenated, 32-padded output columns
//   [w1 hidden Hp | b1 Ep | w2 hidden Hp | b2 hidden Ep]     (Hp = ceil32(Hh), Ep = ceil32(Em), at most 12 column tiles):
// wave w owns column tiles w, w + 4, w + 8 of it - in the forward product (accumulators stay in registers while Ds is streamed
// through LDS in 64-feature chunks), in the dHidden products (its ReLU masks stay in registers as 16 bits per tile) and in the
// first-layer weight gradients.  Second-layer column tiles (A * Em and Em wide) and weight-gradient tiles are dealt round-robin.
// Products are computed transposed (Z^T = W^T X^T): the batch row is on the lane, the feature on the register.  Weights are
// not staged: a lane reads its 8 k-values of a k-step from memory / L2 and splits them in registers.
//
// LDS.  One layout serves every operand: a COLUMN image, [column][32 rows] 4-byte words in 144-byte columns (36 words: the
// 16-byte row reads of 32 lanes fall on 16 distinct bank groups).  A word is either an f32 or the split pair (hi | lo << 16).
//   sum over rows   (X^T dZ):        8 consecutive rows of column c0 + r: two 16-byte reads;
//   sum over columns (layers, dZ W^T): rows r of columns k0 + 8 h + 0..7: eight conflict-free 4-byte reads.
//   X   64 columns   the current state chunk (split)
//   Z1  384 columns  first-layer outputs: hidden (split), b1 and the b2 hidden as f32; later the mixer's pre-activation in
//                    b1's place; in the backward pass dZ1 (split) in place
//   O2  576 columns  second-layer outputs w1 | w2 as f32; in the backward pass d_w1 | d_w2 (split) in place
// d_w1 .. d_b2 therefore never reach memory.  The backward chain runs in units of grad_scale and is unscaled at the slab store.
#include <cfloat>

#include "h2_core.h"
#include "qmix_fused.h"

namespace {

using h2::Frag;

constexpr int THREADS = 256;
constexpr int CS = 36;  // words per image column
constexpr int KC = 64;  // state features per chunk
constexpr int Z1_COLS = 2 * QMIX_FUSED_MAX_HH + 2 * QMIX_FUSED_MAX_EM, O2_COLS = QMIX_FUSED_MAX_AE + QMIX_FUSED_MAX_EM;
// LDS map (words)
constexpr int W_X = 0;
constexpr int W_Z1 = W_X + KC * CS;
constexpr int W_O2 = W_Z1 + Z1_COLS * CS;
constexpr int W_QA = W_O2 + O2_COLS * CS;   // [16][32] chosen online Q per agent
constexpr int W_QX = W_QA + 512;            // [16][32] target Q at the online argmax
constexpr int W_DPRE = W_QX + 512;          // [64][32] dLoss / d pre-activation, f32
constexpr int W_PART = W_DPRE + 2048;       // [8][32] f64 partial sums of Q_tot
constexpr int W_ROW = W_PART + 512;         // per row: g, Q_tot_target, mean reward, discount
constexpr int W_END = W_ROW + 128;
constexpr int LDS_BYTES = 4 * W_END;
static_assert(W_PART % 2 == 0, "f64 alignment");
static_assert(LDS_BYTES <= 163840, "LDS");

#ifdef __HIP_DEVICE_COMPILE__
#define NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PACKED_F32
#endif

struct Dims {
  int A, O, Ds, Em, Hh, AE, Hp, Ep, AEp, nA, NT1, cB1, cH2, cHB;
  // offsets in the flat layout (QMixer / tests/qmix_model.mixer_shapes)
  int w1k0, w1b0, w1k1, w1b1, b1k, b1b, w2k0, w2b0, w2k1, w2b1, b2k0, b2b0, b2k1, b2b1, Pm;
};

struct Args {
  Dims d;
  int L, B, Bp, Rp;
  const float *obs, *next_obs;
  const int32_t* action;
  const float* reward;
  const uint8_t *term_next, *next_mask;
  const float *q, *qn, *qt, *p, *pt;
  float gamma, inv_n, grad_scale;
  float *dq, *slab;
  long slab_stride;
};

__device__ __forceinline__ int featq(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }
__device__ __forceinline__ long t32(long row, int f, int N) { return ((row >> 5) * N + f) * 32 + (row & 31); }
__device__ __forceinline__ float sgn(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : expm1f(x); }

__device__ __forceinline__ uint32_t pack(float v) {
  _Float16 hi, lo;
  h2::split1(v, hi, lo);
  return (uint32_t)__builtin_bit_cast(uint16_t, hi) | ((uint32_t)__builtin_bit_cast(uint16_t, lo) << 16);
}
__device__ __forceinline__ float unpack(uint32_t u) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu)) + (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
}
__device__ __forceinline__ Frag frag_of(const uint32_t (&u)[8]) {
  Frag f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f.hi[e] = __builtin_bit_cast(_Float16, (uint16_t)(u[e] & 0xffffu));
    f.lo[e] = __builtin_bit_cast(_Float16, (uint16_t)(u[e] >> 16));
  }
  return f;
}
// operand of a product that sums over the image's columns: row r of columns col0 .. col0 + 7
__device__ __forceinline__ Frag frag_cols(const uint32_t* img, int col0, int r) {
  uint32_t u[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e] = img[(col0 + e) * CS + r];
  return frag_of(u);
}
// operand of a product that sums over the image's rows: rows row0 .. row0 + 7 of column col
__device__ __forceinline__ Frag frag_rows(const uint32_t* img, int col, int row0) {
  const uint4 a = *reinterpret_cast<const uint4*>(img + col * CS + row0);
  const uint4 b = *reinterpret_cast<const uint4*>(img + col * CS + row0 + 4);
  const uint32_t u[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return frag_of(u);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  return acc;
}
// a slab entry: stored by the block's first tile, added to by the later ones (one thread per entry, tile order)
__device__ __forceinline__ void slab_put(float* p, float v, bool first) { *p = first ? v : *p + v; }
__device__ __forceinline__ float half_sum32(float v) {  // over lanes 0..31 of a wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// column tile ct of the concatenated first layers
struct Col1 {
  int w, b, ld, n0, nv, kind;  // kernel / bias offsets, kernel row length, first column in its net, the net's width; 0..3
};
__device__ __forceinline__ Col1 col1_of(const Dims& d, int ct) {
  int c = 32 * ct;
  if (c < d.Hp) return {d.w1k0, d.w1b0, d.Hh, c, d.Hh, 0};
  c -= d.Hp;
  if (c < d.Ep) return {d.b1k, d.b1b, d.Em, c, d.Em, 1};
  c -= d.Ep;
  if (c < d.Hp) return {d.w2k0, d.w2b0, d.Hh, c, d.Hh, 2};
  c -= d.Hp;
  return {d.b2k0, d.b2b0, d.Em, c, d.Em, 3};
}

// chunk [c0, c0 + KC) of the tile's states -> X (split); zeros past Ds and in padding rows
__device__ __forceinline__ void stage_x(uint32_t* X, const float* __restrict__ src, int Ds, int c0, int nreal, int tid) {
  for (int i = tid; i < 32 * KC; i += THREADS) {
    const int f = i & (KC - 1), lr = i / KC, k = c0 + f;
    const bool ok = lr < nreal && k < Ds;
    const float v = src[ok ? (long)lr * Ds + k : 0];
    X[f * CS + lr] = pack(ok ? v : 0.0f);
  }
}

// the four first layers on parameters P and the tile's states `src` -> Z1; ReLU masks of the wave's column tiles
__device__ __forceinline__ void layer1(const Dims& d, const float* __restrict__ P, const float* __restrict__ src, int nreal, uint32_t* lds,
                                       uint32_t (&mask)[3], int tid, int w, int r, int h) {
  f32x16 acc[3];
  float carry[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int ct = w + 4 * i;
    acc[i] = zero16();
    if (ct < d.NT1) {
      const Col1 c = col1_of(d, ct);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = c.n0 + featq(q, h);
        const float b = P[c.b + (n < c.nv ? n : 0)];
        acc[i][q] = n < c.nv ? b : 0.0f;
      }
    }
  }
  for (int c0 = 0; c0 < d.Ds; c0 += KC) {
    __syncthreads();  // X (and, the first time, whatever the caller read last) is free
    stage_x(lds + W_X, src, d.Ds, c0, nreal, tid);
    __syncthreads();
    const int steps = (min(KC, d.Ds - c0) + 15) >> 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ct = w + 4 * i;
      if (ct >= d.NT1) continue;
      const Col1 c = col1_of(d, ct);
      const int n = c.n0 + r;
      for (int s = 0; s < steps; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = c0 + 16 * s + 8 * h + e;
          const bool ok = k < d.Ds && n < c.nv;
          const float x = P[c.w + (ok ? k * c.ld + n : 0)];
          v[e] = ok ? x : 0.0f;
        }
        const Frag a = h2::split8_carry(v, carry[i]);
        acc[i] = h2::mfma3(a, frag_cols(lds + W_X, 16 * s + 8 * h, r), acc[i]);
      }
    }
  }
  // (every wave is past the caller's last read of Z1: at least one barrier pair lies behind)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int ct = w + 4 * i;
    mask[i] = 0;
    if (ct >= d.NT1) continue;
    const Col1 c = col1_of(d, ct);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float v = acc[i][q];
      if (c.kind != 1) {  // ReLU; the b1 block is linear
        if (v > 0.0f) mask[i] |= 1u << q;
        else v = 0.0f;
      }
      lds[W_Z1 + (32 * ct + featq(q, h)) * CS + r] = (c.kind & 1) ? __builtin_bit_cast(uint32_t, v) : pack(v);
    }
  }
  __syncthreads();
}

// the two MFMA second layers: O2 = [H1 K1(w1) + bias | H2 K1(w2) + bias] as f32
__device__ __forceinline__ void layer2(const Dims& d, const float* __restrict__ P, uint32_t* lds, int w, int r, int h) {
  const int nt1 = d.AEp >> 5, nt = nt1 + (d.Ep >> 5);
  for (int ct = w; ct < nt; ct += 4) {
    const bool first = ct < nt1;
    const int wp = first ? d.w1k1 : d.w2k1, bp = first ? d.w1b1 : d.w2b1, nv = first ? d.AE : d.Em;
    const int n0 = first ? 32 * ct : 32 * (ct - nt1), xcol = first ? 0 : d.cH2, ocol = first ? n0 : d.AEp + n0;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = n0 + featq(q, h);
      const float b = P[bp + (n < nv ? n : 0)];
      acc[q] = n < nv ? b : 0.0f;
    }
    const int n = n0 + r;
    float carry = 0.0f;
    for (int s = 0; s < (d.Hp >> 4); ++s) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 16 * s + 8 * h + e;
        const bool ok = k < d.Hh && n < nv;
        const float x = P[wp + (ok ? k * nv + n : 0)];
        v[e] = ok ? x : 0.0f;
      }
      const Frag a = h2::split8_carry(v, carry);
      acc = h2::mfma3(a, frag_cols(lds + W_Z1 + xcol * CS, 16 * s + 8 * h, r), acc);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float v = acc[q];  // (a bit cast of the vector element itself reads element 0)
      lds[W_O2 + (ocol + featq(q, h)) * CS + r] = __builtin_bit_cast(uint32_t, v);
    }
  }
  __syncthreads();
}

// Q_tot of the tile's rows from Q ([16][32]) and the hypernet outputs in Z1 / O2; leaves the pre-activation in b1's place
__device__ __forceinline__ double mix_forward(const Dims& d, const float* __restrict__ P, float* f, const float* Q, int lr, int g) {
  double tot = 0.0;
  for (int k = g; k < d.Em; k += 8) {
    double pre = 0.0;
    for (int j = 0; j < d.A; ++j) pre += (double)Q[j * 32 + lr] * (double)fabsf(f[W_O2 + (j * d.Em + k) * CS + lr]);
    const float pf = (float)(pre + (double)f[W_Z1 + (d.cB1 + k) * CS + lr]);
    f[W_Z1 + (d.cB1 + k) * CS + lr] = pf;
    tot += (double)elu(pf) * (double)fabsf(f[W_O2 + (d.AEp + k) * CS + lr]);
  }
  float b2 = 0.0f;  // the Em -> 1 head of the b2 net
  for (int e = g; e < d.Em; e += 8) b2 = fmaf(f[W_Z1 + (d.cHB + e) * CS + lr], P[d.b2k1 + e], b2);
  double* part = reinterpret_cast<double*>(f + W_PART);
  part[g * 32 + lr] = tot + (double)b2;
  __syncthreads();
  double q_tot = (double)P[d.b2b1];
#pragma unroll
  for (int k = 0; k < 8; ++k) q_tot += part[k * 32 + lr];
  __syncthreads();  // (part is written again by the next pass)
  return q_tot;
}

__global__ __launch_bounds__(THREADS) NO_PACKED_F32 void qmix_mixer_update_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  float* f = reinterpret_cast<float*>(lds);
  const Dims& d = a.d;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int lr = tid & 31, g = tid >> 5;  // per-row phases: row lr of the tile, feature group g of 8
  const int A = d.A, nA = d.nA, Em = d.Em;
  float* slab = a.slab + (long)blockIdx.x * a.slab_stride;
  const long ntiles = (long)a.L * a.Bp / 32;
  if (blockIdx.x >= ntiles) {  // a slab without tiles holds zeros
    for (int i = tid; i < d.Pm + 3; i += THREADS) slab[i] = 0.0f;
    return;
  }
  const float unscale = 1.0f / a.grad_scale;
  float s_err = 0.0f, s_q = 0.0f, s_t = 0.0f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const bool first = tile == blockIdx.x;
    const int t = (int)(tile * 32 / a.Bp), b0 = (int)(tile * 32 - (long)t * a.Bp);
    const int nreal = max(0, min(32, a.B - b0)), b = b0 + lr;
    const bool real = lr < nreal;
    const long arow0 = (long)t * a.Rp + (long)b0 * A;  // the tile's first agent row
    // ---- select and argmax (mava_qmix_td_f32's): group g takes the agents g, g + 8
    for (int j = g; j < A; j += 8) {
      float qa = 0.0f, qx = 0.0f;
      if (real) {
        const long arow = arow0 + (long)lr * A + j;
        const uint8_t* mk = a.next_mask + arow * nA;
        int as = 0;
        float best = -FLT_MAX;
        for (int o = 0; o < nA; ++o) {
          const float z = mk[o] ? a.qn[t32(arow, o, nA)] : -FLT_MAX;
          if (o == 0 || z > best) { best = z; as = o; }
        }
        const int act = a.action[arow];
        for (int o = 0; o < nA; ++o) {
          const float v = a.q[t32(arow, o, nA)];
          if (o == act) qa = v;
        }
        qx = a.qt[t32(arow, as, nA)];
      }
      f[W_QA + j * 32 + lr] = qa;
      f[W_QX + j * 32 + lr] = qx;
    }
    if (g == 0) {
      float r_sum = 0.0f, disc = 0.0f;
      if (real) {
        for (int j = 0; j < A; ++j) r_sum += a.reward[arow0 + (long)lr * A + j];
        disc = __fmul_rn(1.0f - (float)a.term_next[arow0 + (long)lr * A], a.gamma);
      }
      f[W_ROW + 64 + lr] = r_sum / (float)A;
      f[W_ROW + 96 + lr] = disc;
    }
    uint32_t mask[3];
    // ---- the target mixer on next_state
    layer1(d, a.pt, a.next_obs + arow0 * d.O, nreal, lds, mask, tid, w, r, h);
    layer2(d, a.pt, lds, w, r, h);
    const double q_tot_t = mix_forward(d, a.pt, f, f + W_QX, lr, g);
    // ---- the online mixer on state, activations kept
    layer1(d, a.p, a.obs + arow0 * d.O, nreal, lds, mask, tid, w, r, h);
    layer2(d, a.p, lds, w, r, h);
    const double q_tot = mix_forward(d, a.p, f, f + W_QA, lr, g);
    // ---- the TD error (every group computes its row's g in the same order)
    float gv = 0.0f;
    if (real) {
      // y = r + (1 - terminal') * gamma * Q_tot_target, evaluated in that order (no contraction)
      const float y = __fadd_rn(f[W_ROW + 64 + lr], __fmul_rn(f[W_ROW + 96 + lr], (float)q_tot_t));
      const float e = (float)(q_tot - (double)y);
      gv = 2.0f * e * a.inv_n * a.grad_scale;
      if (g == 0) {
        s_err += e * e;
        s_q += (float)q_tot;
        s_t += y;
      }
    }
    if (g == 0) f[W_ROW + lr] = gv;
    __syncthreads();
    // ---- the b2 net's head: d K1[e] = sum_row g h[row][e], d bias = sum_row g
    if (tid <= Em) {
      float s = 0.0f;
      for (int row = 0; row < 32; ++row) s += f[W_ROW + row] * (tid < Em ? f[W_Z1 + (d.cHB + tid) * CS + row] : 1.0f);
      slab_put(slab + d.b2k1 + tid, s * unscale, first);  // (b2b1 = b2k1 + Em)
    }
    __syncthreads();
    // ---- backward through the mixer, per row: d_w2, d_b1 = d pre, the b2 hidden's dZ (split, in place)
    for (int k = g; k < Em; k += 8) {
      const float pre = f[W_Z1 + (d.cB1 + k) * CS + lr], w2r = f[W_O2 + (d.AEp + k) * CS + lr];
      const float d_w2 = gv * elu(pre) * sgn(w2r);
      const float d_pre = gv * fabsf(w2r) * (pre > 0.0f ? 1.0f : expf(pre));  // elu' = exp(x) for x <= 0
      f[W_DPRE + k * 32 + lr] = d_pre;
      lds[W_O2 + (d.AEp + k) * CS + lr] = pack(d_w2);
      lds[W_Z1 + (d.cB1 + k) * CS + lr] = pack(d_pre);
      const float hb = f[W_Z1 + (d.cHB + k) * CS + lr];
      lds[W_Z1 + (d.cHB + k) * CS + lr] = pack(hb > 0.0f ? gv * a.p[d.b2k1 + k] : 0.0f);
    }
    __syncthreads();
    // ---- dq: every element of the tile's agent rows; group g takes the agents g, g + 8
    for (int j = g; j < A; j += 8) {
      const long m = (long)b * A + j;
      if (m >= a.Rp) break;  // (Bp * A may exceed Rp: those agent rows do not exist)
      const long arow = (long)t * a.Rp + m;
      int act = -1;
      float dqa = 0.0f;
      if (real) {
        act = a.action[arow];
        double sum = 0.0;
        for (int k = 0; k < Em; ++k) sum += (double)f[W_DPRE + k * 32 + lr] * (double)fabsf(f[W_O2 + (j * Em + k) * CS + lr]);
        dqa = (float)sum;
      }
      for (int o = 0; o < nA; ++o) a.dq[t32(arow, o, nA)] = o == act ? dqa : 0.0f;
    }
    __syncthreads();
    // ---- d_w1 (split) in w1's place
    for (int j = 0; j < A; ++j) {
      const float qa = f[W_QA + j * 32 + lr];
      for (int k = g; k < Em; k += 8) {
        const int c = W_O2 + (j * Em + k) * CS + lr;
        lds[c] = pack(f[W_DPRE + k * 32 + lr] * qa * sgn(f[c]));
      }
    }
    __syncthreads();
    // ---- second-layer weight gradients H^T d_out, tiles dealt round-robin; their bias gradients
    {
      const int kt_n = d.Hp >> 5, nt1 = d.AEp >> 5, nt = nt1 + (d.Ep >> 5);
      for (int idx = w; idx < kt_n * nt; idx += 4) {
        const int kt = idx % kt_n, ct = idx / kt_n;
        const bool one = ct < nt1;
        const int nv = one ? d.AE : Em, n0 = one ? 32 * ct : 32 * (ct - nt1);
        const int xcol = (one ? 0 : d.cH2) + 32 * kt + r, dcol = (one ? 0 : d.AEp) + n0 + r;
        float* out = slab + (one ? d.w1k1 : d.w2k1);
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < 2; ++s)
          acc = h2::mfma3(frag_rows(lds + W_Z1, xcol, 16 * s + 8 * h), frag_rows(lds + W_O2, dcol, 16 * s + 8 * h), acc);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int k = 32 * kt + featq(q, h), n = n0 + r;
          if (k < d.Hh && n < nv) slab_put(out + k * nv + n, acc[q] * unscale, first);
        }
      }
      for (int i = tid; i < d.AE + Em; i += THREADS) {
        const bool one = i < d.AE;
        const int col = one ? i : d.AEp + i - d.AE;
        float s = 0.0f;
        for (int row = 0; row < 32; ++row) s += unpack(lds[W_O2 + col * CS + row]);
        slab_put(slab + (one ? d.w1b1 + i : d.w2b1 + i - d.AE), s * unscale, first);
      }
    }
    __syncthreads();  // H1 / H2 have been read: dZ1 replaces them
    // ---- dHidden = d_out K1^T, masked, on the wave's own column tiles of the w1 and w2 nets
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ct = w + 4 * i;
      if (ct >= d.NT1) continue;
      const Col1 c = col1_of(d, ct);
      if (c.kind & 1) continue;
      const bool one = c.kind == 0;
      const int wp = one ? d.w1k1 : d.w2k1, nv = one ? d.AE : Em, ocol = one ? 0 : d.AEp, steps = (one ? d.AEp : d.Ep) >> 4;
      const int hc = c.n0 + r;
      f32x16 acc = zero16();
      for (int s = 0; s < steps; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int n = 16 * s + 8 * h + e;
          const bool ok = hc < d.Hh && n < nv;
          const float x = a.p[wp + (ok ? hc * nv + n : 0)];
          v[e] = ok ? x : 0.0f;
        }
        acc = h2::mfma3(h2::split8(v), frag_cols(lds + W_O2 + ocol * CS, 16 * s + 8 * h, r), acc);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q)
        lds[W_Z1 + (32 * ct + featq(q, h)) * CS + r] = pack(((mask[i] >> q) & 1u) ? acc[q] : 0.0f);
    }
    __syncthreads();
    // ---- first-layer bias and weight gradients: X^T dZ1 against re-staged state chunks
    for (int i = tid; i < 32 * d.NT1; i += THREADS) {
      const Col1 c = col1_of(d, i >> 5);
      const int n = c.n0 + (i & 31);
      if (n < c.nv) {
        float s = 0.0f;
        for (int row = 0; row < 32; ++row) s += unpack(lds[W_Z1 + i * CS + row]);
        slab_put(slab + c.b + n, s * unscale, first);
      }
    }
    for (int c0 = 0; c0 < d.Ds; c0 += KC) {
      __syncthreads();
      stage_x(lds + W_X, a.obs + arow0 * d.O, d.Ds, c0, nreal, tid);
      __syncthreads();
      const int kts = (min(KC, d.Ds - c0) + 31) >> 5;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int ct = w + 4 * i;
        if (ct >= d.NT1) continue;
        const Col1 c = col1_of(d, ct);
        const Frag z0 = frag_rows(lds + W_Z1, 32 * ct + r, 8 * h), z1 = frag_rows(lds + W_Z1, 32 * ct + r, 16 + 8 * h);
        const int n = c.n0 + r;
        for (int kt = 0; kt < kts; ++kt) {
          f32x16 acc = zero16();
          acc = h2::mfma3(frag_rows(lds + W_X, 32 * kt + r, 8 * h), z0, acc);
          acc = h2::mfma3(frag_rows(lds + W_X, 32 * kt + r, 16 + 8 * h), z1, acc);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int k = c0 + 32 * kt + featq(q, h);
            if (k < d.Ds && n < c.nv) slab_put(slab + c.w + k * c.ld + n, acc[q] * unscale, first);
          }
        }
      }
    }
    __syncthreads();  // the images and the row arrays are rewritten by the next tile
  }
  if (tid < 32) {  // the metric partial sums: lanes in row order per tile, then a fixed butterfly
    s_err = half_sum32(s_err);
    s_q = half_sum32(s_q);
    s_t = half_sum32(s_t);
    if (tid == 0) {
      slab[d.Pm] = s_err * a.inv_n;
      slab[d.Pm + 1] = s_q * a.inv_n;
      slab[d.Pm + 2] = s_t * a.inv_n;
    }
  }
}

inline int ceil32(int n) { return (n + 31) / 32 * 32; }

}  // namespace

int mava_qmix_fused_launch(const QmixFusedArgs& x, hipStream_t s) {
  Args a = {};
  Dims& d = a.d;
  d.A = x.A; d.O = x.O; d.Ds = x.A * x.O; d.Em = x.Em; d.Hh = x.Hh; d.AE = x.A * x.Em; d.nA = x.nA;
  d.Hp = ceil32(d.Hh); d.Ep = ceil32(d.Em); d.AEp = ceil32(d.AE);
  d.NT1 = (2 * d.Hp + 2 * d.Ep) / 32; d.cB1 = d.Hp; d.cH2 = d.Hp + d.Ep; d.cHB = 2 * d.Hp + d.Ep;
  int off = 0;
  const int sizes[14] = {d.Ds * d.Hh, d.Hh, d.Hh * d.AE, d.AE, d.Ds * d.Em, d.Em, d.Ds * d.Hh, d.Hh, d.Hh * d.Em, d.Em, d.Ds * d.Em, d.Em, d.Em, 1};
  int* offs[14] = {&d.w1k0, &d.w1b0, &d.w1k1, &d.w1b1, &d.b1k, &d.b1b, &d.w2k0, &d.w2b0, &d.w2k1, &d.w2b1, &d.b2k0, &d.b2b0, &d.b2k1, &d.b2b1};
  for (int i = 0; i < 14; ++i) {
    *offs[i] = off;
    off += sizes[i];
  }
  d.Pm = off;
  a.L = x.L; a.B = x.B; a.Bp = ceil32(x.B); a.Rp = x.Rp;
  a.obs = x.obs; a.next_obs = x.next_obs; a.action = x.action; a.reward = x.reward; a.term_next = x.term_next; a.next_mask = x.next_mask;
  a.q = x.q; a.qn = x.qn; a.qt = x.qt; a.p = x.mixer; a.pt = x.mixer_target;
  a.gamma = x.gamma; a.inv_n = 1.0f / (float)((double)x.L * x.B); a.grad_scale = x.grad_scale;
  a.dq = x.dq; a.slab = x.slab; a.slab_stride = x.slab_stride;
  static bool attr = false;
  if (!attr) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)qmix_mixer_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr = true;
  }
  hipLaunchKernelGGL(qmix_mixer_update_kernel, dim3(x.n_slab), dim3(THREADS), LDS_BYTES, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}
