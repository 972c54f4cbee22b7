// ff_mat, fused training pass: the teacher-forced forward pass of the Multi-Agent Transformer in one launch and its backward
// pass (with the forward recomputed) in a second one.
//
// What MATPass.encode + decode + backward do in about 175 launches per minibatch - every activation a (rows x D) T32 matrix in
// HBM, written by one launch and read by the next - runs here per group of samples inside one workgroup.  A sample's A agent
// rows only interact with each other (attention over the agents), so a group never needs another group's rows.
//
// Work split (mat_act.hip's).  A group is S = max(1, 32 / A) consecutive minibatch samples, R = S * A <= 32 agent rows; the padding
// rows of a partial group are exact zeros in every tile.  Groups are dealt to the workgroups round robin in a persistent loop; a
// group is computed the same way whichever workgroup takes it and every sum has a fixed order: logits and values are bit-identical
// for any grid.  No grid barrier, no atomics; every barrier sits under block-uniform control flow (nr is a per-group number).
//
// Inputs in place.  Row b * A + j of the minibatch reads agent j of trajectory sample idx[b]; the decoder's input row is row 0
// (start token) or row 1 + action[idx[b]][j - 1] of decoder/act_dense/kernel, and its gradient is a row scatter-add into the
// slab in row order.  Observations wider than D are normalised and staged D features at a time.
//
// Dense products on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32; 256 threads = 4 waves; the group's 32 rows are one tile).
//  * Y = X W (Grp::xw): C[row][n]; A operand X from an LDS tile (row stride D + 1), B operand W[k][n0 + lane % 32] straight from
//    L2, 128-byte runs.  Wave w owns column tile w % NT (NT = D / 32) and, for NT < 4, the slice w / NT of the k range (KS = 4, 2,
//    1, 1 slices at D = 32, 64, 96, 128; D = 96 leaves one wave idle).
//  * dX = dY W^T (Grp::dywt): C[row][k]; W is staged through LDS 32 of its columns at a time ([D][33] floats, coalesced reads,
//    the transposed operand read walks an odd stride), so no instruction walks W a row per lane.  Same wave roles, the k split
//    runs inside a 32-column chunk.
//  * dW += X^T dY (Grp::xtdy): C[k][n], the 32 rows are the summation index, both operands from LDS tiles (X read transposed on the
//    odd stride).  The (D / 32)^2 accumulator tiles are dealt to the waves round robin; a lane loads its 16 accumulators from the
//    workgroup's slab row, runs 16 MFMAs and stores them back with plain vector loads and stores, in group order.
//  The partial tiles of the k slices meet in LDS and are added in slice order by the pass that also adds the bias, applies
//  GELU, saves the activation and zeroes the padding rows (Grp::take).
//  Like mat_act.hip the kernel does not follow the context's matmul mode: its products are exact f32.
//
// Between the products: mat.hip's arithmetic.  f32 storage; LayerNorm's moments (8 lanes per row, a butterfly of shuffles), its
// backward row sums, the softmax with its exp, the attention dot products over hd and GELU's tanh in f64; the probabilities are
// computed again in the backward half.  The two heads' last layers (D x 1 and D x n_actions) are plain f32 FMA loops.
//
// BWD instance.  It recomputes the group's forward pass, saves every activation the backward half needs in a workgroup-private
// region of the caller's workspace (mat_layout.h's slots, overwritten group after group; a slot is read for rows < nr only and
// after this launch wrote it), then walks the network in reverse.  dlogits / dvalues are scaled by 1 / grad_scale as they are read
// (a power of two in the learner: exact), so the slab holds the gradient itself.  The slab row is zeroed in the prologue (a
// workgroup without groups leaves exact zeros) and every element of it is only ever touched by the one lane that owns it.
//
// LDS: six (32 x (D + 1)) tiles, the KS partial tiles, the two f64 score tiles (32 x 33; the staged W chunk aliases them),
// the logits tile (32 x 64): 141 568 bytes at D = 128, 92 544 at D = 64 (dynamic, the attribute is raised).
#include <cfloat>

#include "mat_layout.h"
#include "mlp_core.h"

namespace {

using namespace mat;

// phases of the stamps: recomputed forward, dW products on the slab row (with their staging), dX products (with W's staging and the
// partial-tile pass), LayerNorm and GELU backward, attention backward (with the q / k / v loads), the rest
enum { ST_FWD, ST_DW, ST_DX, ST_ELEM, ST_ATTN, ST_OTHER, ST_N };

struct TrainTask {
  const float* params;
  const float* obs;       // (n_samples, A, O)
  const int32_t* idx;     // [Bm]
  const int32_t* action;  // (n_samples, A)
  long n_samples;
  int Bm, A, O, nA, H, hd, nb, S;
  float* logits;          // FWD: T32 (rows x nA)
  float* value;           // FWD: rows
  long rows;
  const float* dlogits;   // BWD: T32 (rows x nA), times grad_scale
  const float* dvalues;   // BWD: rows, times grad_scale
  float inv_scale;
  float* ws;              // BWD: n_blocks x slots x (32 D + 32)
  float* slab;            // BWD: n_blocks x slab_stride
  long slab_stride, P;
};

// The thread index behind an empty asm: address arithmetic derived from it stays next to its use.  Without it the compiler hoists
// every helper call's per-thread LDS addresses out of the group loop and keeps hundreds of them live across it (scratch).
__device__ __forceinline__ int tidx() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// the same for a block-uniform pointer
template <typename T>
__device__ __forceinline__ T* fresh(T* q) {
  asm volatile("" : "+s"(q));
  return q;
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.0f;
  return c;
}

// accumulator register r of lane-half h holds row (r & 3) + 8 * (r >> 2) + 4 * h of the 32 x 32 tile, column lane % 32
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The state of one group of samples inside a workgroup: its row count, the LDS scratch and the saved-activation slots.
template <int D>
struct Grp {
  static constexpr int LD = D + 1, NT = D / 32, KS = NT == 1 ? 4 : (NT == 2 ? 2 : 1), TILE = ROWS * LD, SL = ROWS * D + ROWS;
  float* pb;    // KS partial tiles
  float* wst;   // [D][33]: 32 columns of a weight matrix (aliases sc and sd)
  double* sc;   // [32][33] scores, then probabilities
  double* sd;   // [32][33] dP, then dS
  float* ws;    // this workgroup's slots (nullptr in the FWD instance)
  int nr, A, H, hd;
#ifdef MAVA_STAMPS
  // cycles of thread 0 per phase of the BWD instance (a diagnostic build: tools/mat_train_stamps.py reads them behind the slab row)
  mutable unsigned long long st_prev, st_acc[ST_N];
  __device__ __forceinline__ void stamp(int i) const {
    const unsigned long long now = __builtin_readcyclecounter();
    st_acc[i] += now - st_prev;
    st_prev = now;
  }
#else
  __device__ __forceinline__ void stamp(int) const {}
#endif

  __device__ __forceinline__ float* slot(int i) const { return ws != nullptr ? ws + (long)i * SL : nullptr; }

  // ---- Y = X W: C[row][n] += sum over this wave's k slice of X[row][k] W[k][n]; rows k >= kc of W read as zero
  __device__ __forceinline__ void xw(f32x16& C, const float* X, const float* __restrict__ W, int kc) const {
    const int lane = tidx() & 63, w = tidx() >> 6, j = lane & 31, h = lane >> 5;
    const int ct = w % NT, ks = w / NT;
    if (ks >= KS) return;
    const int kb = ks * (D / KS), kend = kc + (kc & 1);
    const int ke = kb + D / KS < kend ? kb + D / KS : kend;
    const float* xp = X + j * LD + h;
    const float* wp = W + 32 * ct + j;
    for (int k0 = kb; k0 < ke; k0 += 2) {
      const int k = k0 + h;
      const float b = k < kc ? wp[(long)k * D] : 0.0f;
      C = MFMA32(xp[k0], b, C);
    }
  }

  // this wave's accumulator tile -> its partial tile
  __device__ __forceinline__ void put(const f32x16& C) const {
    const int lane = tidx() & 63, w = tidx() >> 6, j = lane & 31, h = lane >> 5;
    const int ct = w % NT, ks = w / NT;
    if (ks >= KS) return;
    float* p = pb + ks * TILE + 32 * ct + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[acc_row(r, h) * LD] = C[r];
  }

  // out[r][n] = f((acc ? out[r][n] : 0) + the partial tiles in slice order + bias[n]) on the group's rows, exact zeros below
  // them; `pre` / `post` save the value before / after GELU
  template <bool GELU>
  __device__ __forceinline__ void take(float* out, bool acc, const float* __restrict__ bias, float* pre, float* post) const {
    for (int e = tidx(); e < ROWS * D; e += 256) {
      const int r = e / D, n = e - r * D;
      float v = pb[r * LD + n];
#pragma unroll
      for (int s = 1; s < KS; ++s) v += pb[s * TILE + r * LD + n];
      if (bias != nullptr) v += bias[n];
      if (acc) v += out[r * LD + n];
      const bool real = r < nr;
      if (pre != nullptr && real) pre[e] = v;
      if (GELU && real) v = gelu_f(v);
      if (post != nullptr && real) post[e] = v;
      out[r * LD + n] = real ? v : 0.0f;
    }
  }

  // out = f(X W + b).  X is ready and the partial tiles are free on entry; ends on a barrier.
  template <bool GELU>
  __device__ __forceinline__ void dense(const float* X, const float* __restrict__ W, const float* __restrict__ b, float* out,
                                        float* pre, float* post) const {
    f32x16 C = zero16();
    xw(C, X, W, D);
    put(C);
    __syncthreads();
    take<GELU>(out, false, b, pre, post);
    __syncthreads();
  }

  // ---- dX = dY W^T: C[row][k] += sum_n G[row][n] W[k][n], k in this wave's column tile, rows k >= krows of W read as zero
  __device__ __forceinline__ void dywt(f32x16& C, const float* G, const float* __restrict__ W, int krows) const {
    const int lane = tidx() & 63, w = tidx() >> 6, j = lane & 31, h = lane >> 5;
    const int ct = w % NT, ks = w / NT;
    for (int nc = 0; nc < D; nc += 32) {
      __syncthreads();  // (the previous chunk, or the score tiles, have been read)
      for (int e = tidx(); e < D * 32; e += 256) {
        const int jj = e >> 5, nn = e & 31;
        wst[jj * LDP + nn] = jj < krows ? W[(long)jj * D + nc + nn] : 0.0f;
      }
      __syncthreads();
      if (ks < KS) {
        const float* gp = G + j * LD + nc + ks * (32 / KS) + h;
        const float* wp = wst + (32 * ct + j) * LDP + ks * (32 / KS) + h;
#pragma unroll
        for (int s = 0; s < 16 / KS; ++s) C = MFMA32(gp[2 * s], wp[2 * s], C);
      }
    }
  }

  // out (+)= G W^T; ends on a barrier
  __device__ __forceinline__ void dx(const float* G, const float* __restrict__ W, float* out, bool acc) const {
    stamp(ST_OTHER);
    f32x16 C = zero16();
    dywt(C, G, W, D);
    put(C);
    __syncthreads();
    take<false>(out, acc, nullptr, nullptr, nullptr);
    __syncthreads();
    stamp(ST_DX);
  }

  // ---- dW[k][n] += sum_r X[r][k] G[r][n] for k < kc: accumulators from and to the slab, by the lane that owns them
  __device__ __forceinline__ void xtdy(const float* X, const float* G, float* dW, int kc) const {
    const int lane = tidx() & 63, w = tidx() >> 6, j = lane & 31, h = lane >> 5;
    for (int t = w; t < NT * NT; t += 4) {
      const int kt = t / NT, nt = t - kt * NT;
      if (32 * kt >= kc) continue;
      float* dp = dW + (long)(32 * kt) * D + 32 * nt + j;
      f32x16 C;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = acc_row(r, h);
        C[r] = (32 * kt + i < kc) ? dp[(long)i * D] : 0.0f;
      }
      const float* xp = X + h * LD + 32 * kt + j;
      const float* gp = G + h * LD + 32 * nt + j;
#pragma unroll
      for (int s = 0; s < 16; ++s) C = MFMA32(xp[2 * s * LD], gp[2 * s * LD], C);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = acc_row(r, h);
        if (32 * kt + i < kc) dp[(long)i * D] = C[r];
      }
    }
  }

  // db[n] += sum_r G[r][n]
  __device__ __forceinline__ void colsum(const float* G, float* db) const {
    if (tidx() < D) {
      double s = 0.0;
      for (int r = 0; r < nr; ++r) s += (double)G[r * LD + tidx()];
      db[tidx()] += (float)s;
    }
  }

  // a saved activation -> a tile, zeros on the padding rows (a slot is never read there)
  __device__ __forceinline__ void load(float* T, const float* src) const {
    for (int e = tidx(); e < ROWS * D; e += 256) {
      const int r = e / D, n = e - r * D;
      T[r * LD + n] = r < nr ? src[e] : 0.0f;
    }
  }

  // weight and bias gradients of Y = X W + b: X from its slot through the tile xs, G = dY.  xs is free on entry; ends on a barrier.
  __device__ __forceinline__ void dense_dw(const float* xslot, float* xs, const float* G, float* dW, float* db) const {
    stamp(ST_OTHER);
    load(xs, xslot);
    __syncthreads();
    xtdy(xs, G, dW, D);
    colsum(G, db);
    __syncthreads();
    stamp(ST_DW);
  }

  // ---- LayerNorm: out[r] = LN(x[r] (+ res[r])) * scale + bias; sb = [scale | bias]; out may be x or res
  // (here and in ln_bwd the 8 lanes of a padding row walk row 0 so that the shuffles stay uniform; with out == x they may read
  // row 0 while its own lanes overwrite it - any f32 they see is finite and their results are discarded)
  __device__ __forceinline__ void ln(const float* x, const float* res, float* out, const float* __restrict__ sb, float* xh_slot,
                                     float* y_slot) const {
    const int r = tidx() >> 3, g = tidx() & 7;
    const bool real = r < nr;
    const int rr = real ? r : 0;
    const float* xp = x + rr * LD;
    const float* rp = res != nullptr ? res + rr * LD : nullptr;
    double s = 0.0;
    for (int f = g; f < D; f += 8) s += (double)(rp != nullptr ? xp[f] + rp[f] : xp[f]);
    const double mean = sum8(s) / (double)D;
    double v = 0.0;
    for (int f = g; f < D; f += 8) {
      const double d = (double)(rp != nullptr ? xp[f] + rp[f] : xp[f]) - mean;
      v = fma(d, d, v);
    }
    const double rstd = 1.0 / sqrt(sum8(v) / (double)D + LN_EPS);
    for (int f = g; f < D; f += 8) {
      const double xh = ((double)(rp != nullptr ? xp[f] + rp[f] : xp[f]) - mean) * rstd;
      const float y = (float)fma(xh, (double)sb[f], (double)sb[D + f]);
      if (real && xh_slot != nullptr) {
        xh_slot[r * D + f] = (float)xh;
        y_slot[r * D + f] = y;
      }
      out[r * LD + f] = real ? y : 0.0f;
    }
    if (real && g == 0 && xh_slot != nullptr) xh_slot[ROWS * D + r] = (float)rstd;
  }

  // G = dy -> dx in place; dsb (slab) += [colsum(dy xhat) | colsum(dy)].  Ends on a barrier.
  __device__ __forceinline__ void ln_bwd(float* G, const float* xh_slot, const float* __restrict__ scale, float* dsb) const {
    stamp(ST_OTHER);
    if (tidx() < D) {
      const int f = tidx();
      double ds = 0.0, db = 0.0;
      for (int r = 0; r < nr; ++r) {
        const double g = (double)G[r * LD + f];
        ds = fma(g, (double)xh_slot[r * D + f], ds);
        db += g;
      }
      dsb[f] += (float)ds;
      dsb[D + f] += (float)db;
    }
    __syncthreads();
    const int r = tidx() >> 3, g8 = tidx() & 7;
    const bool real = r < nr;
    const int rr = real ? r : 0;
    double s1 = 0.0, s2 = 0.0;
    for (int f = g8; f < D; f += 8) {
      const double g = (double)G[rr * LD + f] * (double)scale[f];
      s1 += g;
      s2 = fma(g, (double)xh_slot[rr * D + f], s2);
    }
    const double m1 = sum8(s1) / (double)D, m2 = sum8(s2) / (double)D;
    const double rs = (double)xh_slot[ROWS * D + rr];
    if (real)
      for (int f = g8; f < D; f += 8) {
        const double g = (double)G[r * LD + f] * (double)scale[f];
        G[r * LD + f] = (float)(rs * (g - m1 - (double)xh_slot[r * D + f] * m2));
      }
    __syncthreads();
    stamp(ST_ELEM);
  }

  // G *= gelu'(h), h a saved pre-activation
  __device__ __forceinline__ void gelu_bwd(float* G, const float* hslot) const {
    stamp(ST_OTHER);
    for (int e = tidx(); e < ROWS * D; e += 256) {
      const int r = e / D, n = e - r * D;
      if (r < nr) G[r * LD + n] = (float)((double)G[r * LD + n] * gelu_d(hslot[e]));
    }
    stamp(ST_ELEM);
  }

  // ---- attention over the A agents of each sample of the group
  // sc[r][j] = softmax_j(q_r . k_j / sqrt(hd)) of head columns [f0, f0 + hd), zero for the keys a causal row does not see.
  // Ends on a barrier.
  __device__ __forceinline__ void probs(const float* Q, const float* K, int f0, bool causal) const {
    const double scale = 1.0 / sqrt((double)hd);
    for (int e = tidx(); e < nr * A; e += 256) {
      const int r = e / A, j = e - r * A;
      const int kr = r - (r % A) + j;
      double s = 0.0;
      for (int d = 0; d < hd; ++d) s = fma((double)Q[r * LD + f0 + d], (double)K[kr * LD + f0 + d], s);
      sc[r * LDP + j] = s * scale;
    }
    __syncthreads();
    if (tidx() < nr) {
      double* p = sc + tidx() * LDP;
      const int last = causal ? (tidx() % A) : (A - 1);
      double mx = p[0];
      for (int j = 1; j <= last; ++j) mx = fmax(mx, p[j]);
      double se = 0.0;
      for (int j = 0; j <= last; ++j) {
        const double ex = exp(p[j] - mx);
        p[j] = ex;
        se += ex;
      }
      const double inv = 1.0 / se;
      for (int j = 0; j < A; ++j) p[j] = (j <= last) ? p[j] * inv : 0.0;
    }
    __syncthreads();
  }

  // y = softmax(q k^T / sqrt(hd)) v per head; y replaces q.  Ends on a barrier.
  __device__ __forceinline__ void attn(float* Q, const float* K, const float* V, bool causal, float* yslot) const {
    for (int h = 0; h < H; ++h) {
      const int f0 = h * hd;
      probs(Q, K, f0, causal);
      for (int e = tidx(); e < nr * hd; e += 256) {
        const int r = e / hd, d = e - r * hd;
        const int base = r - (r % A);
        double acc = 0.0;
        for (int j = 0; j < A; ++j) acc = fma(sc[r * LDP + j], (double)V[(base + j) * LD + f0 + d], acc);
        Q[r * LD + f0 + d] = (float)acc;
        if (yslot != nullptr) yslot[r * D + f0 + d] = (float)acc;
      }
      __syncthreads();
    }
  }

  // mat.hip's attn_bwd_kernel on tiles: G = dy becomes dq, V becomes dk, DV receives dv (zeros on the padding rows).
  //   dv = P^T dy;  dP = dy v^T;  dS = P (dP - rowsum(P dP)) scale;  dq = dS k;  dk = dS^T q.  Ends on a barrier.
  __device__ __forceinline__ void attn_bwd(float* G, const float* Q, const float* K, float* V, float* DV, bool causal) const {
    const double scale = 1.0 / sqrt((double)hd);
    for (int h = 0; h < H; ++h) {
      const int f0 = h * hd;
      probs(Q, K, f0, causal);
      for (int e = tidx(); e < nr * A; e += 256) {
        const int r = e / A, j = e - r * A;
        const int kr = r - (r % A) + j;
        double s = 0.0;
        for (int d = 0; d < hd; ++d) s = fma((double)G[r * LD + f0 + d], (double)V[kr * LD + f0 + d], s);
        sd[r * LDP + j] = s;
      }
      for (int e = tidx(); e < ROWS * hd; e += 256) {  // dv: row r is the KEY row here
        const int r = e / hd, d = e - r * hd;
        double acc = 0.0;
        if (r < nr) {
          const int j = r % A, base = r - j;
          for (int i = 0; i < A; ++i) acc = fma(sc[(base + i) * LDP + j], (double)G[(base + i) * LD + f0 + d], acc);
        }
        DV[r * LD + f0 + d] = (float)acc;
      }
      __syncthreads();
      if (tidx() < nr) {
        const double* p = sc + tidx() * LDP;
        double* dp = sd + tidx() * LDP;
        double dot = 0.0;
        for (int j = 0; j < A; ++j) dot = fma(p[j], dp[j], dot);
        for (int j = 0; j < A; ++j) dp[j] = p[j] * (dp[j] - dot) * scale;
      }
      __syncthreads();
      for (int e = tidx(); e < nr * hd; e += 256) {
        const int r = e / hd, d = e - r * hd;
        const int i = r % A, base = r - i;
        double accq = 0.0, acck = 0.0;
        for (int j = 0; j < A; ++j) {
          accq = fma(sd[r * LDP + j], (double)K[(base + j) * LD + f0 + d], accq);         // row r as the query, keys j
          acck = fma(sd[(base + j) * LDP + i], (double)Q[(base + j) * LD + f0 + d], acck);  // row r as the key, queries j
        }
        G[r * LD + f0 + d] = (float)accq;
        V[r * LD + f0 + d] = (float)acck;
      }
      __syncthreads();
    }
  }

  // Backward of attention(q_in, kv_in) up to its projection: G = d(output of proj) on entry.  aw / as: the attention's
  // parameters and their slab; s0: its slots q, k, v, y.  On exit (a barrier) G = dq, V = dk, DV = dv, and proj's gradients are in.
  __device__ __forceinline__ void attn_core_bwd(float* G, float* B, float* Q, float* K, float* V, float* DV, const float* aw, float* as,
                                                int s0, bool causal) const {
    dense_dw(slot(s0 + AS::y), Q, G, as + Attn<D>::proj_w, as + Attn<D>::proj_b);
    dx(G, aw + Attn<D>::proj_w, B, false);
    load(Q, slot(s0 + AS::q));
    load(K, slot(s0 + AS::k));
    load(V, slot(s0 + AS::v));
    __syncthreads();
    attn_bwd(B, Q, K, V, DV, causal);
    stamp(ST_ATTN);
  }
};

constexpr size_t lds_bytes(int D) {
  const int NT = D / 32, KS = NT == 1 ? 4 : (NT == 2 ? 2 : 1);
  return (size_t)(2 * ROWS * LDP + 2 * ROWS) * sizeof(double) +
         (size_t)((6 + KS) * ROWS * (D + 1) + ROWS * MAX_ACT + ROWS) * sizeof(float) + 2 * ROWS * sizeof(int);
}

template <int D, bool BWD>
__global__ __launch_bounds__(256) void mat_train_kernel(TrainTask a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  using G_ = Grp<D>;
  constexpr int LD = G_::LD, TILE = G_::TILE;
  using At = Attn<D>;
  using EB = EncBlock<D>;
  using DB = DecBlock<D>;
  using HD = Head<D>;
  double* const s_sc = reinterpret_cast<double*>(lds);
  double* const s_sd = s_sc + ROWS * LDP;
  double* const s_mom = s_sd + ROWS * LDP;  // [32] mean, [32] rstd of the observation rows
  float* const X = reinterpret_cast<float*>(s_mom + 2 * ROWS);  // forward: x, then rep;      backward: GX, the stream's gradient
  float* const Y = X + TILE;                                    // forward: the decoder's x;  backward: B, a branch's gradient
  float* const Q = Y + TILE;
  float* const K = Q + TILE;
  float* const V = K + TILE;
  float* const T = V + TILE;                                    // forward: branch output;    backward: DV
  float* const s_pb = T + TILE;
  float* const s_log = s_pb + G_::KS * TILE;                    // [32][64] logits / dlogits
  float* const s_dv = s_log + ROWS * MAX_ACT;                   // [32] dvalues
  int* const s_rowi = reinterpret_cast<int*>(s_dv + ROWS);      // [32] trajectory agent row of each row
  int* const s_tok = s_rowi + ROWS;                             // [32] the decoder's input token of each row
  const int tid0 = threadIdx.x;
  const int A = a.A, O = a.O, nA = a.nA, nb = a.nb, S = a.S;

  const long oE_w0 = 2 * (long)O, oE_b0 = oE_w0 + (long)O * D, oE_ln = oE_b0 + D, oE_blk = oE_ln + 2 * D;
  const long oE_head = oE_blk + nb * EB::size, oDec = oE_head + head_size(D, 1);
  const long oD_ln = oDec + (long)(nA + 1) * D, oD_blk = oD_ln + 2 * D, oD_head = oD_blk + nb * DB::size;
  const int eh = slot::enc_head(nb), db0 = slot::dec_in(eh), dh = slot::dec_head(db0, nb), s_grep = slot::d_rep(dh);
  const int s_rep = slot::enc_blk(nb - 1) + ES::x2;  // the encoder's output

  G_ g;
  g.pb = s_pb;
  g.wst = reinterpret_cast<float*>(s_sc);
  g.sc = s_sc;
  g.sd = s_sd;
  g.ws = BWD ? a.ws + (long)blockIdx.x * n_slots(nb) * G_::SL : nullptr;
  g.A = A;
  g.H = a.H;
  g.hd = a.hd;
#ifdef MAVA_STAMPS
  g.st_prev = __builtin_readcyclecounter();
  for (int i = 0; i < ST_N; ++i) g.st_acc[i] = 0;
#endif
  float* const sl0 = BWD ? a.slab + (long)blockIdx.x * a.slab_stride : nullptr;
  if constexpr (BWD) {
    for (long e = tid0; e < a.P; e += 256) sl0[e] = 0.0f;
    __syncthreads();
  }

  const long groups = ((long)a.Bm + S - 1) / S;
  for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int tid = tidx();
    const float* const p = fresh(a.params);
    float* const sl = BWD ? fresh(sl0) : nullptr;
    const long b0 = grp * S;
    const int ns = (int)((a.Bm - b0 < S) ? (a.Bm - b0) : S);
    const int nr = ns * A;
    const long row0 = b0 * A;
    g.nr = nr;
    g.stamp(ST_OTHER);
    if (tid < ROWS) {
      int ri = 0, tok = 0;
      if (tid < nr) {
        const int sidx = tid / A, j = tid - sidx * A;
        long sb = a.idx[b0 + sidx];
        sb = sb < 0 ? 0 : (sb >= a.n_samples ? a.n_samples - 1 : sb);
        ri = (int)(sb * A + j);
        if (j > 0) {
          const int act = a.action[sb * A + j - 1];
          tok = 1 + (act < 0 ? 0 : (act >= nA ? nA - 1 : act));
        }
      }
      s_rowi[tid] = ri;
      s_tok[tid] = tok;
    }
    __syncthreads();

    // ================================================================ forward
    auto moments = [&]() {  // of the observation rows (f64, two passes as LayerNorm has them)
      const int r = tid >> 3, g8 = tid & 7;
      const float* op = a.obs + (long)s_rowi[r < nr ? r : 0] * O;
      double s = 0.0;
      for (int f = g8; f < O; f += 8) s += (double)op[f];
      const double mean = sum8(s) / (double)O;
      double v = 0.0;
      for (int f = g8; f < O; f += 8) {
        const double d = (double)op[f] - mean;
        v = fma(d, d, v);
      }
      const double rstd = 1.0 / sqrt(sum8(v) / (double)O + LN_EPS);
      if (g8 == 0) {
        s_mom[r] = mean;
        s_mom[ROWS + r] = rstd;
      }
    };
    // features [c0, c0 + kc) of LN_O(obs) -> dst (zeros past kc and on the padding rows); xh: the same without scale and bias
    auto stage_obs = [&](float* dst, float* xh, int c0, int kc) {
      for (int e = tid; e < ROWS * D; e += 256) {
        const int r = e / D, k = e - r * D;
        float val = 0.0f, h = 0.0f;
        if (r < nr && k < kc) {
          const double x = ((double)a.obs[(long)s_rowi[r] * O + c0 + k] - s_mom[r]) * s_mom[ROWS + r];
          val = (float)fma(x, (double)p[c0 + k], (double)p[O + c0 + k]);
          h = (float)x;
        }
        dst[r * LD + k] = val;
        if (xh != nullptr) xh[r * LD + k] = h;
      }
    };
    moments();
    __syncthreads();
    {  // T = GELU(Dense(LN_O(obs))), the normalised observations D features at a time through Q
      f32x16 C = zero16();
      for (int c0 = 0; c0 < O; c0 += D) {
        const int kc = (O - c0 < D) ? (O - c0) : D;
        stage_obs(Q, nullptr, c0, kc);
        __syncthreads();
        g.xw(C, Q, p + oE_w0 + (long)c0 * D, kc);
        __syncthreads();
      }
      g.put(C);
      __syncthreads();
      g.template take<true>(T, false, p + oE_b0, g.slot(slot::enc_h0), nullptr);
      __syncthreads();
    }
    g.ln(T, nullptr, X, p + oE_ln, g.slot(slot::enc_xhat0), g.slot(slot::enc_x0));
    __syncthreads();
    for (int l = 0; l < nb; ++l) {
      const float* const bp = p + oE_blk + l * EB::size;
      const int s0 = slot::enc_blk(l);
      g.template dense<false>(X, bp, bp + At::q_b, Q, nullptr, g.slot(s0 + ES::q));
      g.template dense<false>(X, bp + At::k_w, bp + At::k_b, K, nullptr, g.slot(s0 + ES::k));
      g.template dense<false>(X, bp + At::v_w, bp + At::v_b, V, nullptr, g.slot(s0 + ES::v));
      g.attn(Q, K, V, false, g.slot(s0 + ES::y));
      g.template dense<false>(Q, bp + At::proj_w, bp + At::proj_b, T, nullptr, nullptr);
      g.ln(T, X, X, bp + EB::ln1, g.slot(s0 + ES::xhat1), g.slot(s0 + ES::x1));
      __syncthreads();
      g.template dense<true>(X, bp + EB::mlp0_w, bp + EB::mlp0_b, Q, g.slot(s0 + ES::h), g.slot(s0 + ES::g));
      g.template dense<false>(Q, bp + EB::mlp1_w, bp + EB::mlp1_b, T, nullptr, nullptr);
      g.ln(T, X, X, bp + EB::ln2, g.slot(s0 + ES::xhat2), g.slot(s0 + ES::x2));
      __syncthreads();
    }
    {  // value = Dense(1)(LN(GELU(Dense(rep))))
      const float* const hp = p + oE_head;
      g.template dense<true>(X, hp, hp + HD::dense_b, Q, g.slot(eh + HS::h), nullptr);
      g.ln(Q, nullptr, T, hp + HD::ln, g.slot(eh + HS::xhat), g.slot(eh + HS::y));
      __syncthreads();
      if constexpr (!BWD) {
        if (tid < nr) {
          const float* hw = hp + HD::out_w;
          float acc = 0.0f;
          for (int k = 0; k < D; ++k) acc = fmaf(T[tid * LD + k], hw[k], acc);
          a.value[row0 + tid] = acc + hw[D];
        }
        __syncthreads();
      }
    }
    // decoder: the input row is a row of act_dense's kernel
    for (int e = tid; e < ROWS * D; e += 256) {
      const int r = e / D, n = e - r * D;
      T[r * LD + n] = r < nr ? gelu_f(p[oDec + (long)s_tok[r] * D + n]) : 0.0f;
    }
    __syncthreads();
    g.ln(T, nullptr, Y, p + oD_ln, g.slot(db0), g.slot(slot::dec_x0(db0)));
    __syncthreads();
    for (int l = 0; l < nb; ++l) {
      const float* const bp = p + oD_blk + l * DB::size;
      const float* const a2 = bp + DB::attn2;
      const int s0 = slot::dec_blk(db0, l);
      g.template dense<false>(Y, bp, bp + At::q_b, Q, nullptr, g.slot(s0 + DS::q1));
      g.template dense<false>(Y, bp + At::k_w, bp + At::k_b, K, nullptr, g.slot(s0 + DS::k1));
      g.template dense<false>(Y, bp + At::v_w, bp + At::v_b, V, nullptr, g.slot(s0 + DS::v1));
      g.attn(Q, K, V, true, g.slot(s0 + DS::y1));
      g.template dense<false>(Q, bp + At::proj_w, bp + At::proj_b, T, nullptr, nullptr);
      g.ln(T, Y, Y, bp + DB::ln1, g.slot(s0 + DS::xhat1), g.slot(s0 + DS::x1));
      __syncthreads();
      g.template dense<false>(X, a2, a2 + At::q_b, Q, nullptr, g.slot(s0 + DS::q2));
      g.template dense<false>(Y, a2 + At::k_w, a2 + At::k_b, K, nullptr, g.slot(s0 + DS::k2));
      g.template dense<false>(Y, a2 + At::v_w, a2 + At::v_b, V, nullptr, g.slot(s0 + DS::v2));
      g.attn(Q, K, V, true, g.slot(s0 + DS::y2));
      g.template dense<false>(Q, a2 + At::proj_w, a2 + At::proj_b, T, nullptr, nullptr);
      g.ln(T, X, Y, bp + DB::ln2, g.slot(s0 + DS::xhat2), g.slot(s0 + DS::x2));
      __syncthreads();
      g.template dense<true>(Y, bp + DB::mlp0_w, bp + DB::mlp0_b, Q, g.slot(s0 + DS::h), g.slot(s0 + DS::g));
      g.template dense<false>(Q, bp + DB::mlp1_w, bp + DB::mlp1_b, T, nullptr, nullptr);
      g.ln(T, Y, Y, bp + DB::ln3, g.slot(s0 + DS::xhat3), g.slot(s0 + DS::x3));
      __syncthreads();
    }
    {
      const float* const hp = p + oD_head;
      g.template dense<true>(Y, hp, hp + HD::dense_b, Q, g.slot(dh + HS::h), nullptr);
      g.ln(Q, nullptr, T, hp + HD::ln, g.slot(dh + HS::xhat), g.slot(dh + HS::y));
      __syncthreads();
      if constexpr (!BWD) {
        const float* hw = hp + HD::out_w;
        const float* hb = hw + (long)D * nA;  // HD::out_b(nA)
        for (int e = tid; e < nr * nA; e += 256) {
          const int r = e / nA, o = e - r * nA;
          float acc = 0.0f;
          for (int k = 0; k < D; ++k) acc = fmaf(T[r * LD + k], hw[k * nA + o], acc);
          a.logits[t32(row0 + r, o, nA)] = acc + hb[o];
        }
        __syncthreads();
      }
    }

    // ================================================================ backward
    if constexpr (BWD) {
      g.stamp(ST_FWD);
      float* const GX = X;
      float* const B = Y;
      float* const DV = T;
      float* const grep = g.slot(s_grep);
      // ---- value head: d rep starts here
      if (tid < ROWS) s_dv[tid] = tid < nr ? a.dvalues[row0 + tid] * a.inv_scale : 0.0f;
      g.load(Q, g.slot(eh + HS::y));
      __syncthreads();
      {
        const long oo = oE_head + HD::out_w;
        if (tid < D) {
          float s = 0.0f;
          for (int r = 0; r < nr; ++r) s = fmaf(s_dv[r], Q[r * LD + tid], s);
          sl[oo + tid] += s;
        } else if (tid == 255) {
          float s = 0.0f;
          for (int r = 0; r < nr; ++r) s += s_dv[r];
          sl[oo + D] += s;
        }
        for (int e = tid; e < ROWS * D; e += 256) {
          const int r = e / D, n = e - r * D;
          GX[r * LD + n] = s_dv[r] * p[oo + n];
        }
      }
      __syncthreads();
      g.ln_bwd(GX, g.slot(eh + HS::xhat), p + oE_head + HD::ln, sl + oE_head + HD::ln);
      g.gelu_bwd(GX, g.slot(eh + HS::h));
      __syncthreads();
      g.dense_dw(g.slot(s_rep), Q, GX, sl + oE_head, sl + oE_head + HD::dense_b);
      g.dx(GX, p + oE_head, B, false);
      for (int e = tid; e < ROWS * D; e += 256) {
        const int r = e / D, n = e - r * D;
        if (r < nr) grep[e] = B[r * LD + n];
      }
      // ---- decoder head
      for (int e = tid; e < ROWS * nA; e += 256) {
        const int r = e / nA, o = e - r * nA;
        s_log[r * MAX_ACT + o] = r < nr ? a.dlogits[t32(row0 + r, o, nA)] * a.inv_scale : 0.0f;
      }
      g.load(Q, g.slot(dh + HS::y));
      __syncthreads();
      {
        const long ow = oD_head + HD::out_w;
        for (int e = tid; e < D * nA; e += 256) {
          const int k = e / nA, o = e - k * nA;
          float s = 0.0f;
          for (int r = 0; r < nr; ++r) s = fmaf(Q[r * LD + k], s_log[r * MAX_ACT + o], s);
          sl[ow + e] += s;
        }
        if (tid < nA) {
          float s = 0.0f;
          for (int r = 0; r < nr; ++r) s += s_log[r * MAX_ACT + tid];
          sl[ow + (long)D * nA + tid] += s;
        }
        for (int e = tid; e < ROWS * D; e += 256) {
          const int r = e / D, n = e - r * D;
          float s = 0.0f;
          for (int o = 0; o < nA; ++o) s = fmaf(s_log[r * MAX_ACT + o], p[ow + (long)n * nA + o], s);
          GX[r * LD + n] = s;
        }
      }
      __syncthreads();
      g.ln_bwd(GX, g.slot(dh + HS::xhat), p + oD_head + HD::ln, sl + oD_head + HD::ln);
      g.gelu_bwd(GX, g.slot(dh + HS::h));
      __syncthreads();
      g.dense_dw(g.slot(slot::dec_blk(db0, nb - 1) + DS::x3), Q, GX, sl + oD_head, sl + oD_head + HD::dense_b);
      g.dx(GX, p + oD_head, GX, false);
      // ---- decoder blocks
      for (int l = nb - 1; l >= 0; --l) {
        const long ob = oD_blk + l * DB::size, o2 = ob + DB::attn2;
        const float* const bp = p + ob;
        float* const bs = sl + ob;
        const int s0 = slot::dec_blk(db0, l), xin = l == 0 ? slot::dec_x0(db0) : s0 - 1;  // x0, or the block before's x3
        g.ln_bwd(GX, g.slot(s0 + DS::xhat3), bp + DB::ln3, bs + DB::ln3);
        g.dense_dw(g.slot(s0 + DS::g), Q, GX, bs + DB::mlp1_w, bs + DB::mlp1_b);
        g.dx(GX, bp + DB::mlp1_w, B, false);
        g.gelu_bwd(B, g.slot(s0 + DS::h));
        __syncthreads();
        g.dense_dw(g.slot(s0 + DS::x2), Q, B, bs + DB::mlp0_w, bs + DB::mlp0_b);
        g.dx(B, bp + DB::mlp0_w, GX, true);
        g.ln_bwd(GX, g.slot(s0 + DS::xhat2), bp + DB::ln2, bs + DB::ln2);  // GX = d(rep + attn2)
        for (int e = tid; e < ROWS * D; e += 256) {
          const int r = e / D, n = e - r * D;
          if (r < nr) grep[e] += GX[r * LD + n];
        }
        g.attn_core_bwd(GX, B, Q, K, V, DV, p + o2, sl + o2, s0 + DS::q2, true);
        g.dense_dw(g.slot(s_rep), Q, B, sl + o2, sl + o2 + At::q_b);  // the query reads rep
        g.dx(B, p + o2, K, false);
        for (int e = tid; e < ROWS * D; e += 256) {
          const int r = e / D, n = e - r * D;
          if (r < nr) grep[e] += K[r * LD + n];
        }
        g.stamp(ST_OTHER);
        g.load(Q, g.slot(s0 + DS::x1));  // keys and values read x1
        __syncthreads();
        g.xtdy(Q, V, sl + o2 + At::k_w, D);
        g.colsum(V, sl + o2 + At::k_b);
        g.xtdy(Q, DV, sl + o2 + At::v_w, D);
        g.colsum(DV, sl + o2 + At::v_b);
        g.stamp(ST_DW);
        {
          f32x16 C = zero16();
          g.dywt(C, V, p + o2 + At::k_w, D);
          g.dywt(C, DV, p + o2 + At::v_w, D);
          g.put(C);
          __syncthreads();
          g.template take<false>(GX, false, nullptr, nullptr, nullptr);  // GX = d x1
          __syncthreads();
          g.stamp(ST_DX);
        }
        g.ln_bwd(GX, g.slot(s0 + DS::xhat1), bp + DB::ln1, bs + DB::ln1);
        g.attn_core_bwd(GX, B, Q, K, V, DV, bp, bs, s0 + DS::q1, true);
        g.stamp(ST_OTHER);
        g.load(Q, g.slot(xin));
        __syncthreads();
        g.xtdy(Q, B, bs, D);
        g.colsum(B, bs + At::q_b);
        g.xtdy(Q, V, bs + At::k_w, D);
        g.colsum(V, bs + At::k_b);
        g.xtdy(Q, DV, bs + At::v_w, D);
        g.colsum(DV, bs + At::v_b);
        g.stamp(ST_DW);
        {
          f32x16 C = zero16();
          g.dywt(C, B, bp, D);
          g.dywt(C, V, bp + At::k_w, D);
          g.dywt(C, DV, bp + At::v_w, D);
          g.put(C);
          __syncthreads();
          g.template take<false>(GX, true, nullptr, nullptr, nullptr);
          __syncthreads();
          g.stamp(ST_DX);
        }
      }
      // ---- decoder input: LayerNorm, GELU, then the embedding rows' scatter-add in row order
      g.ln_bwd(GX, g.slot(db0), p + oD_ln, sl + oD_ln);
      for (int e = tid; e < ROWS * D; e += 256) {
        const int r = e / D, n = e - r * D;
        if (r < nr) GX[r * LD + n] = (float)((double)GX[r * LD + n] * gelu_d(p[oDec + (long)s_tok[r] * D + n]));
      }
      __syncthreads();
      if (tid < D)
        for (int r = 0; r < nr; ++r) sl[oDec + (long)s_tok[r] * D + tid] += GX[r * LD + tid];
      __syncthreads();
      // ---- encoder blocks
      g.load(GX, grep);
      __syncthreads();
      for (int l = nb - 1; l >= 0; --l) {
        const long ob = oE_blk + l * EB::size;
        const float* const bp = p + ob;
        float* const bs = sl + ob;
        const int s0 = slot::enc_blk0 + ES::n * l, xin = l == 0 ? slot::enc_x0 : s0 - 1;  // slot::enc_blk(l); x0, or the block before's x2
        g.ln_bwd(GX, g.slot(s0 + ES::xhat2), bp + EB::ln2, bs + EB::ln2);
        g.dense_dw(g.slot(s0 + ES::g), Q, GX, bs + EB::mlp1_w, bs + EB::mlp1_b);
        g.dx(GX, bp + EB::mlp1_w, B, false);
        g.gelu_bwd(B, g.slot(s0 + ES::h));
        __syncthreads();
        g.dense_dw(g.slot(s0 + ES::x1), Q, B, bs + EB::mlp0_w, bs + EB::mlp0_b);
        g.dx(B, bp + EB::mlp0_w, GX, true);
        g.ln_bwd(GX, g.slot(s0 + ES::xhat1), bp + EB::ln1, bs + EB::ln1);
        g.attn_core_bwd(GX, B, Q, K, V, DV, bp, bs, s0 + ES::q, false);
        g.stamp(ST_OTHER);
        g.load(Q, g.slot(xin));
        __syncthreads();
        g.xtdy(Q, B, bs, D);
        g.colsum(B, bs + At::q_b);
        g.xtdy(Q, V, bs + At::k_w, D);
        g.colsum(V, bs + At::k_b);
        g.xtdy(Q, DV, bs + At::v_w, D);
        g.colsum(DV, bs + At::v_b);
        g.stamp(ST_DW);
        {
          f32x16 C = zero16();
          g.dywt(C, B, bp, D);
          g.dywt(C, V, bp + At::k_w, D);
          g.dywt(C, DV, bp + At::v_w, D);
          g.put(C);
          __syncthreads();
          g.template take<false>(GX, true, nullptr, nullptr, nullptr);
          __syncthreads();
          g.stamp(ST_DX);
        }
      }
      // ---- encoder input: LayerNorm, GELU, obs_dense and obs_ln D features at a time
      g.ln_bwd(GX, g.slot(slot::enc_xhat0), p + oE_ln, sl + oE_ln);
      g.gelu_bwd(GX, g.slot(slot::enc_h0));
      __syncthreads();
      g.colsum(GX, sl + oE_b0);
      for (int c0 = 0; c0 < O; c0 += D) {
        const int kc = (O - c0 < D) ? (O - c0) : D;
        stage_obs(Q, K, c0, kc);  // (s_mom still holds this group's moments)
        __syncthreads();
        g.xtdy(Q, GX, sl + oE_w0 + (long)c0 * D, kc);
        {
          f32x16 C = zero16();
          g.dywt(C, GX, p + oE_w0 + (long)c0 * D, kc);
          g.put(C);
          __syncthreads();
          g.template take<false>(B, false, nullptr, nullptr, nullptr);  // B = d LN_O(obs), this chunk
          __syncthreads();
        }
        if (tid < kc) {
          double ds = 0.0, dbi = 0.0;
          for (int r = 0; r < nr; ++r) {
            const double gv = (double)B[r * LD + tid];
            ds = fma(gv, (double)K[r * LD + tid], ds);
            dbi += gv;
          }
          sl[c0 + tid] += (float)ds;
          sl[O + c0 + tid] += (float)dbi;
        }
        __syncthreads();
      }
    }
  }
#ifdef MAVA_STAMPS
  if constexpr (BWD) {
    g.stamp(ST_OTHER);
    if (tid0 == 0 && a.slab_stride >= a.P + ST_N)
      for (int i = 0; i < ST_N; ++i) sl0[a.P + i] = (float)g.st_acc[i];
  }
#endif
  if constexpr (!BWD) {  // exact zeros on the padding rows of the two outputs
    const long valid = (long)a.Bm * A, npad = a.rows - valid;
    for (long e = (long)blockIdx.x * 256 + tid0; e < npad * (nA + 1); e += (long)gridDim.x * 256) {
      const long o = e / npad, row = valid + (e - o * npad);
      if (o < nA) a.logits[t32(row, o, nA)] = 0.0f;
      else a.value[row] = 0.0f;
    }
  }
}

template <int D, bool BWD>
int launch_train(const TrainTask& a, int n_blocks, hipStream_t s) {
  static bool attr_set = false;
  constexpr size_t lb = lds_bytes(D);
  static_assert(lb <= 163840, "LDS");
  if (!attr_set) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)mat_train_kernel<D, BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
    attr_set = true;
  }
  hipLaunchKernelGGL((mat_train_kernel<D, BWD>), dim3(n_blocks), dim3(256), lb, s, a);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

template <bool BWD>
int launch_for(int D, const TrainTask& a, int n_blocks, hipStream_t s) {
  switch (D) {
    case 32: return launch_train<32, BWD>(a, n_blocks, s);
    case 64: return launch_train<64, BWD>(a, n_blocks, s);
    case 96: return launch_train<96, BWD>(a, n_blocks, s);
    default: return launch_train<128, BWD>(a, n_blocks, s);
  }
}

// the checks both entry points share; 1 = no instance for this shape (nothing launched)
int train_task(TrainTask& a, const char* who, const float* params, const float* agents_view, long n_samples, const int32_t* idx,
               const int32_t* action, int Bm, int A, int O, int n_actions, int D, int n_head, int n_block, int n_blocks) {
  MAVA_ARG_CHECK(Bm >= 1 && (long)Bm * MAX_A < (1L << 31), 0, "%s: Bm=%d (at least one sample, Bm * 32 below 2^31)", who, Bm);
  MAVA_ARG_CHECK(A >= 1 && A <= MAX_A, 1, "%s: A=%d (1..%d agents)", who, A, MAX_A);
  MAVA_ARG_CHECK(D >= 1 && n_head >= 1 && D % n_head == 0, 2, "%s: D=%d n_head=%d (D a multiple of n_head)", who, D, n_head);
  MAVA_ARG_CHECK(n_actions >= 1 && n_actions <= MAX_ACT, 3, "%s: n_actions=%d (1..%d)", who, n_actions, MAX_ACT);
  MAVA_ARG_CHECK(O >= 1 && O <= MAX_O, 4, "%s: O=%d (1..%d observation features)", who, O, MAX_O);
  MAVA_ARG_CHECK(n_block >= 1, 5, "%s: n_block=%d", who, n_block);
  MAVA_ARG_CHECK(n_blocks >= 1 && n_blocks <= 65536, 6, "%s: n_blocks=%d", who, n_blocks);
  MAVA_ARG_CHECK(n_samples >= 1 && n_samples * MAX_A < (1L << 31), 7, "%s: n_samples=%ld (at least one, n_samples * 32 below 2^31)", who,
                 n_samples);
  MAVA_ARG_CHECK(params && agents_view && idx && action, 8, "%s: null pointer argument", who);
  if ((D != 32 && D != 64 && D != 96 && D != 128) || n_block > MAX_NBLOCK) return 1;
  a.params = params; a.obs = agents_view; a.n_samples = n_samples; a.idx = idx; a.action = action;
  a.Bm = Bm; a.A = A; a.O = O; a.nA = n_actions; a.H = n_head; a.hd = D / n_head; a.nb = n_block;
  a.S = A >= ROWS ? 1 : ROWS / A;
  a.rows = ((long)Bm * A + 31) / 32 * 32;
  a.P = Layout(O, n_actions, D, n_block, false).total;
  return MAVA_OK;
}

}  // namespace

extern "C" size_t mava_transformer_train_workspace_bytes(int Bm, int A, int O, int D, int n_block, int n_blocks) {
  (void)Bm;
  (void)A;
  (void)O;
  if ((D != 32 && D != 64 && D != 96 && D != 128) || n_block < 1 || n_block > MAX_NBLOCK || n_blocks < 1) return 0;
  return (size_t)n_blocks * n_slots(n_block) * (ROWS * D + ROWS) * sizeof(float);
}

extern "C" int mava_transformer_train_fwd_f32(const float* params, const float* agents_view, long n_samples, const int32_t* idx,
                                              const int32_t* action, int Bm, int A, int O, int n_actions, int D, int n_head,
                                              int n_block, float* logits, float* value, int n_blocks, hipStream_t s) {
  const char* who = "mava_transformer_train_fwd_f32";
  TrainTask a = {};
  const int rc = train_task(a, who, params, agents_view, n_samples, idx, action, Bm, A, O, n_actions, D, n_head, n_block, n_blocks);
  if (rc != MAVA_OK) return rc;
  MAVA_ARG_CHECK(logits && value, 9, "%s: null pointer argument", who);
  a.logits = logits; a.value = value;
  return launch_for<false>(D, a, n_blocks, s);
}

extern "C" int mava_transformer_train_bwd_f32(const float* params, const float* agents_view, long n_samples, const int32_t* idx,
                                              const int32_t* action, int Bm, int A, int O, int n_actions, int D, int n_head,
                                              int n_block, const float* dlogits, const float* dvalues, float grad_scale, float* slab,
                                              long slab_stride, void* workspace, size_t workspace_bytes, int n_blocks, hipStream_t s) {
  const char* who = "mava_transformer_train_bwd_f32";
  TrainTask a = {};
  const int rc = train_task(a, who, params, agents_view, n_samples, idx, action, Bm, A, O, n_actions, D, n_head, n_block, n_blocks);
  if (rc != MAVA_OK) return rc;
  MAVA_ARG_CHECK(dlogits && dvalues && slab && grad_scale > 0.0f, 9, "%s: null pointer argument or grad_scale=%g", who, (double)grad_scale);
  MAVA_ARG_CHECK(slab_stride >= a.P, 10, "%s: slab_stride=%ld (a slab row holds the %ld parameters)", who, slab_stride, a.P);
  const size_t need = mava_transformer_train_workspace_bytes(Bm, A, O, D, n_block, n_blocks);
  MAVA_ARG_CHECK(workspace != nullptr && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, 11,
                 "%s: workspace of %zu bytes (16-byte aligned) required, got %zu", who, need, workspace_bytes);
  a.dlogits = dlogits; a.dvalues = dvalues; a.inv_scale = 1.0f / grad_scale;
  a.slab = slab; a.slab_stride = slab_stride; a.ws = static_cast<float*>(workspace);
  return launch_for<true>(D, a, n_blocks, s);
}
