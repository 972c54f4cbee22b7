// Arguments of one fused PPO minibatch launch, shared by the exact-f32 kernel (ppo_train.hip) and the
// split-f16 kernel (ppo_train_h2.hip).
#pragma once
#include <stdint.h>

#include "common.h"

struct TrainTask {
  const float* params;
  const float* x;          // (rows_x, din)
  int din, no, xshare, xv;
  int A;                   // agent rows per (t,e) index
  int agg;                 // critic only: 1, or A when the A agents of an index share one input row and are
                           // aggregated into it (one network pass per (t,e) row instead of A identical ones)
  const int32_t* idx;      // minibatch (t*E+e) indices, or null => idx_base + b
  long idx_base;
  int Rb;                  // (t,e) rows in the minibatch; agent rows R = Rb * A
  const uint8_t* mask;     // (TE*A, no) or null
  const int32_t* action;   // (TE*A)
  const float* action_f;   // continuous head: (TE*A, no) actions in (-1, 1); the raw scales follow the MLP in params
  uint32_t seed_lo, seed_hi, ent_step, row_offset;  // continuous head: Philox key / counters of the entropy sample
  float min_scale;         // continuous head: scale = softplus(log_std) + min_scale
  const float* old_logp;   // (TE*A)
  const float* adv;        // (TE*A)
  const double* stats;     // STATS_BLOCKS x {sum, sumsq} partials of the minibatch advantages
  const float* old_value;  // (TE*A)
  const float* targets;    // (TE*A)
  float clip_eps, ent_coef, vf_coef;
  float* slab;
  long slab_stride;
  unsigned long long* stamps;  // diagnostic builds only (-DMAVA_STAMPS): per-phase cycle sums of block 0
  int force_xlo;           // f16x2 kernels: always run the x_lo products (MAVA_CTX_TRAIN_VARIANT bit 1; tests: same bits either way)
  unsigned long long* exact_tiles;  // wide f16x2 kernels: device word every block adds its exact-loop tiles to (MAVA_CTX_EXACT_TILES), or null
  // Wide f16x2 critic: an f16 copy of x (rows_x, din), 16-byte aligned rows (din % 8 == 0), and the device word that says
  // whether it may be read: 1 = x16 is the f16 high term of x and the low term is zero everywhere.  Both null: no copy.  The launch stages x from the copy - 16-byte
  // loads, no conversion, every tile in the exact-input loop - when the word reads 1 (ppo_train_h2.hip), and from x otherwise.
  const _Float16* x16;
  const uint32_t* x16_valid;
  unsigned long long* x16_launches;  // device word block 0 of a launch that read the copy adds 1 to (MAVA_CTX_X16_LAUNCHES), or null
  // The eight-wave kernel (ppo_train_w8.hip) reads the same three through its second staging body, from a record whose rows are
  // x16_ld halves apart (0: din) and, where x16_ld > din, laid out like the kernel's x image row: din values, 1.0 (the ones
  // column), zeros up to a multiple of 8 halves.  Its x16_launches is the word behind MAVA_CTX_X16_W8_LAUNCHES.
  int x16_ld;
  // ... and, on its role-split instances, runs the tile loop in the deferred-dW1 form when it stages from the record (the dW1
  // product of tile n inside the loss phase of tile n + 1): no_defer != 0 keeps the record path on the schedule with dW1 at
  // the tile's end (MAVA_CTX_TRAIN_VARIANT bit 2); defer_launches is the word behind MAVA_CTX_W8_DEFER_LAUNCHES, or null.
  int no_defer;
  unsigned long long* defer_launches;
  // ... and, in that form, issues the row gathers and advances the cursors a tile further ahead, off the path to barrier A
  // (w8_body, AH): no_ahead != 0 keeps them where they were (MAVA_CTX_TRAIN_VARIANT bit 3); ahead_launches is the word behind
  // MAVA_CTX_W8_AHEAD_LAUNCHES, or null.
  int no_ahead;
  unsigned long long* ahead_launches;
};

// ppo_train_h2.hip: the same fused kernel on v_mfma_f32_32x32x16_f16 with every operand split into two f16 terms
// (hi + lo, f32 accumulation).  Returns MAVA_OK, or 1 when the shape is not instantiated (the caller then runs the
// exact-f32 kernel), or a negative error code.
struct mava_ctx;
// ppo_train_w8.hip: the discrete actor's kernel on eight waves (two per SIMD, 16 features per wave, 16x16x32 MFMAs); same
// return convention.  Tried first by mava_train_h2_launch unless the handle's MAVA_CTX_TRAIN_VARIANT is 1.
int mava_train_w8_launch(const TrainTask& tk, int n_slab, bool actor, hipStream_t s);
int mava_train_h2_launch(mava_ctx* ctx, const TrainTask& tk, int n_slab, bool actor, hipStream_t s);

// The launch rule of the f16 record, asked without launching (mava_ppo_*_grad_reads_input16): while this thread's pointer is
// set, the launchers above go through their dispatch as for a launch, and the launcher that would take the task stores ITS OWN
// x16_ok - would this launch read x16 if the word is 1 - there and returns MAVA_OK with no launch, allocation or counter touched.
// One rule: the expression the launch itself hands the record to the kernel by.
extern thread_local int* g_x16_query;

// Diagnostic (ppo_train.hip: mava_debug_train_last_instance): the template instance the last gradient launch of this
// process used, as FAMILY * 1000000 + ROLE * 100000 + NO * 1000 + K * 10 + XV - FAMILY 1: ppo_train_kernel (exact f32, K = KT1),
// 2: ppo_train_h2_kernel (K = S1), 3: ppo_train_w8_kernel (K = S1); ROLE = ACTOR + 2 * CONT + 4 * WIDE.
extern int g_train_last_instance;
constexpr int train_instance_id(int family, bool actor, bool cont, bool wide, int no, int k, int xv) {
  return family * 1000000 + ((actor ? 1 : 0) + (cont ? 2 : 0) + (wide ? 4 : 0)) * 100000 + no * 1000 + k * 10 + xv;
}
