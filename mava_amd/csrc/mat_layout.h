// ff_mat on the C side: what mat.hip, mat_act.hip and mat_train.hip share - the envelope constants, the device helpers, the
// layout of the flat parameter vector (the mirror of mat_learner.param_spec) and the fused training pass's slot map.
#pragma once
#include "common.h"

namespace mat {
constexpr int ROWS = 32;       // agent rows of a group of samples: one MFMA tile
constexpr int MAX_A = 32, MAX_D = 128, MAX_ACT = 64;
constexpr int MAX_DIM = 16;    // action dimensions of the continuous head (the limit of the other continuous kernels)
constexpr int MAX_O = 1024;
constexpr int MAX_NBLOCK = 4;  // blocks the fused kernels take; beyond that the caller runs layer by layer
constexpr int LDP = MAX_A + 1;   // LDS row stride of a (rows x A) score tile
constexpr double LN_EPS = 1e-6;  // flax.linen.LayerNorm default epsilon
// flax nn.gelu(approximate=True): 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))
constexpr double GELU_C = 0.7978845608028654, GELU_K = 0.044715;
// element (row, f) of a T32 (rows x N) matrix
__device__ __forceinline__ long t32(long row, long f, long N) { return ((row >> 5) * N + f) * 32 + (row & 31); }

__device__ __forceinline__ float gelu_f(float x) {
  const double v = (double)x;
  return (float)(0.5 * v * (1.0 + tanh(GELU_C * (v + GELU_K * v * v * v))));
}
__device__ __forceinline__ double gelu_d(float x) {
  const double v = (double)x;
  const double t = tanh(GELU_C * (v + GELU_K * v * v * v));
  return 0.5 * (1.0 + t) + 0.5 * v * (1.0 - t * t) * GELU_C * (1.0 + 3.0 * GELU_K * v * v);
}
// sum over the 8 lanes of a row, the same bits on each of them
__device__ __forceinline__ double sum8(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}
// ---- the flat parameter vector, in mat_learner.param_spec's order: the one place on the C side that knows it.  A Dense is
// [kernel | bias], a LayerNorm [scale | bias] (a `ln` member is its scale, the bias follows at + D).  Offsets count floats.
constexpr long enc_block_size(long D) { return 6 * D * D + 10 * D; }
constexpr long dec_block_size(long D) { return 10 * D * D + 16 * D; }
constexpr long head_size(long D, long n_out) { return D * D + 3 * D + D * n_out + n_out; }
template <int D> constexpr long SQ = (long)D * D;
template <int D> struct Attn {  // query, key, value, proj
  static constexpr long q_w = 0, q_b = q_w + SQ<D>, k_w = q_b + D, k_b = k_w + SQ<D>, v_w = k_b + D, v_b = v_w + SQ<D>, proj_w = v_b + D,
                        proj_b = proj_w + SQ<D>, size = proj_b + D;
  static_assert(size == 4 * SQ<D> + 4 * D, "attention");
};
template <int D> struct EncBlock {  // attn, ln1, mlp_0, mlp_1, ln2
  static constexpr long attn = 0, ln1 = attn + Attn<D>::size, mlp0_w = ln1 + 2 * D, mlp0_b = mlp0_w + SQ<D>, mlp1_w = mlp0_b + D,
                        mlp1_b = mlp1_w + SQ<D>, ln2 = mlp1_b + D, size = ln2 + 2 * D;
  static_assert(size == enc_block_size(D), "encoder block");
};
template <int D> struct DecBlock {  // attn1 (causal self-attention), ln1, attn2 (the query reads rep), ln2, mlp_0, mlp_1, ln3
  static constexpr long attn1 = 0, ln1 = attn1 + Attn<D>::size, attn2 = ln1 + 2 * D, ln2 = attn2 + Attn<D>::size, mlp0_w = ln2 + 2 * D,
                        mlp0_b = mlp0_w + SQ<D>, mlp1_w = mlp0_b + D, mlp1_b = mlp1_w + SQ<D>, ln3 = mlp1_b + D, size = ln3 + 2 * D;
  static_assert(size == dec_block_size(D), "decoder block");
};
template <int D> struct Head {  // head_dense, head_ln, head_out (D x n_out: one value, or the nA logits / means)
  static constexpr long dense_w = 0, dense_b = dense_w + SQ<D>, ln = dense_b + D, out_w = ln + 2 * D;
  __host__ __device__ static constexpr long out_b(long n_out) { return out_w + D * n_out; }
  static_assert(out_b(1) + 1 == head_size(D, 1) && out_b(7) + 7 == head_size(D, 7), "head");
};
// Where the pieces start, in floats from the vector's first: encoder (obs_ln, obs_dense, ln, the blocks, the value head), then
// decoder (act_dense, ln, the blocks, the action head and, under the continuous head, log_std).  act_dense takes (nA + 1) * D
// floats under both heads: a bias-free (nA + 1) x D kernel, or an nA x D kernel and its bias (act_bias, continuous only).
struct Layout {
  long obs_ln, obs_w, obs_b, enc_ln, enc_blk, enc_head, dec, act_bias, dec_ln, dec_blk, dec_head, log_std, total;
  __host__ __device__ Layout(int O, int nA, int D, int n_block, bool continuous) {
    obs_ln = 0, obs_w = obs_ln + 2 * (long)O, obs_b = obs_w + (long)O * D, enc_ln = obs_b + D, enc_blk = enc_ln + 2 * D;
    enc_head = enc_blk + n_block * enc_block_size(D), dec = enc_head + head_size(D, 1);
    dec_ln = dec + (long)(nA + 1) * D, dec_blk = dec_ln + 2 * D, dec_head = dec_blk + n_block * dec_block_size(D);
    act_bias = dec + (long)nA * D, log_std = dec_head + head_size(D, nA), total = log_std + (continuous ? nA : 0);
  }
};
// ---- mat_train.hip's saved activations, one (32 x D + 32) slot each: encoder [h0 xhat0 x0 | per block ES | head HS], decoder
// [xhat0 x0 | per block DS | head HS], d rep.  An attention's four slots are consecutive (AS); a block's input is the slot before it.
struct AS { enum : int { q, k, v, y }; };
struct ES { enum : int { q, k, v, y, xhat1, x1, h, g, xhat2, x2, n }; };
struct DS { enum : int { q1, k1, v1, y1, xhat1, x1, q2, k2, v2, y2, xhat2, x2, h, g, xhat3, x3, n }; };
struct HS { enum : int { h, xhat, y, n }; };
namespace slot {  // the decoder's slots follow the encoder's: dec_in takes the encoder head's slot, the rest the decoder's first
enum : int { enc_h0, enc_xhat0, enc_x0, enc_blk0 };
__host__ __device__ constexpr int enc_blk(int l) { return enc_blk0 + ES::n * l; }
__host__ __device__ constexpr int enc_head(int nb) { return enc_blk(nb); }
__host__ __device__ constexpr int dec_in(int enc_head) { return enc_head + HS::n; }  // xhat0, then x0
__host__ __device__ constexpr int dec_x0(int dec_in) { return dec_in + 1; }
__host__ __device__ constexpr int dec_blk(int dec_in, int l) { return dec_in + 2 + DS::n * l; }
__host__ __device__ constexpr int dec_head(int dec_in, int nb) { return dec_blk(dec_in, nb); }
__host__ __device__ constexpr int d_rep(int dec_head) { return dec_head + HS::n; }
}  // namespace slot
__host__ __device__ constexpr int n_slots(int nb) { return slot::d_rep(slot::dec_head(slot::dec_in(slot::enc_head(nb)), nb)) + 1; }
static_assert(n_slots(0) == 12 && n_slots(1) == 12 + 26 && n_slots(MAX_NBLOCK) == 12 + 26 * MAX_NBLOCK, "slots");
static_assert(ES::y - ES::q == AS::y && DS::y1 - DS::q1 == AS::y && DS::y2 - DS::q2 == AS::y, "q k v y");
}  // namespace mat
