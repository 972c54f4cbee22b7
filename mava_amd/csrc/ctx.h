// Per-learner context of libmavahip.so (include/mava_hip.h "context"): every setting that used to be a process-wide
// knob (arithmetic of the matrix products, critic aggregation, kernel variants) and every workspace the library
// allocates on its own (the pre-split W1 copies of the wide f16x2 gradient kernels) lives in a handle the caller
// creates, passes to the calls that depend on it and destroys.  A NULL handle means the defaults (exact f32,
// aggregation on, default variants); nothing in the library is shared between two handles.
#pragma once
#include "common.h"

struct mava_ctx {
  int matmul_mode;         // 0: exact-f32 MFMA kernels; 1: split-f16 ("f16x2") kernels where instantiated
  int critic_aggregation;  // 1: a critic input row shared by the A agents of an index is evaluated once
  int gae_variant;         // 0: default chunk / lane mapping of mava_gae_f32 (others: tools/gae_sweep.py)
  int policy_variant;      // 0: default acting-step launch (others: tools/policy_bench.py)
  int train_variant;       // f16x2 gradient kernels: bit 0 = four-wave kernels only (default: eight-wave actor kernel where instantiated); bit 1 = never skip the x_lo products;
                           // bit 2 = the eight-wave kernel on an f16 record keeps dW1 at the tile's end (no deferred-dW1 tile loop);
                           // bit 3 = its deferred-dW1 tile loop keeps the row gathers in front of barrier A (no gathers-ahead form)
  long h2_launches;        // diagnostic: gradient launches of this handle that ran on the f16x2 kernels
  long w8_launches;        // diagnostic: ... of which on the eight-wave kernel (ppo_train_w8.hip)
  void* w1_split[2];       // f16x2, inputs wider than 95: pre-split W1 in fragment order (actor, critic), lazily allocated
  int w1_fresh[2];         // one-shot: the copy holds W1 of the parameters named by w1_key (written by the Adam launch of
                           // mava_ppo_finish_f32).  Cleared by the next gradient launch of that kind, whichever kernel it runs on,
                           // by mava_ctx_set(MAVA_CTX_MATMUL_MODE), and by the caller (MAVA_CTX_W1_SPLIT_FRESH)
  const float* w1_key_params[2];  // ... key of that copy: the network's parameters, its input width and 16-input steps (the
  int w1_key_din[2];              // instantiation's, 12 or 18); a wide launch skips its own pack only when all three match.  What the
  int w1_key_steps[2];            // key cannot see: a caller who rewrites the CONTENTS of the same buffer between the finish launch and
                                  // the next gradient launch must clear the flag
  unsigned long long* exact_tiles;  // five device words (allocated by the first launch that may add to one, null before).  [0]: 32-row tiles
                                    // that the wide kernels' blocks ran in their exact-input tile loop (ppo_train_h2.hip), summed over
                                    // launches; [1]: wide critic launches that staged x from the caller's f16 copy (TrainTask::x16);
                                    // [2]: eight-wave launches (ppo_train_w8.hip) that did; [3]: ... of which in the deferred-dW1 form; [4]: ... of which with the row gathers a tile ahead
};

static inline int mava_ctx_matmul_mode(const mava_ctx* c) { return c ? c->matmul_mode : 0; }
static inline int mava_ctx_critic_aggregation(const mava_ctx* c) { return c ? c->critic_aggregation : 1; }
static inline int mava_ctx_gae_variant(const mava_ctx* c) { return c ? c->gae_variant : 0; }
static inline int mava_ctx_policy_variant(const mava_ctx* c) { return c ? c->policy_variant : 0; }
