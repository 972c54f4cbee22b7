/* libmavahip.so - C ABI of the MI355X-native PPO hot path (gfx950 only).
 *
 * Drop-in boundary: Mava has no FFI; the reusable seam is the Python
 * learner contract  learn(LearnerState) -> ExperimentOutput  (mava/types.py:146-154,
 * call site mava/systems/ppo/ff_mappo.py:497).  mava_amd/learner.py keeps that contract and
 * drives the device work through the entry points below with ctypes.  Every pointer is a
 * DEVICE pointer (torch.Tensor.data_ptr()) unless marked "host"; buffers are caller-owned,
 * contiguous, and never retained past the call.  Every function is asynchronous on the given
 * stream and returns 0 on success, -(hipError_t) for a runtime failure or -1000-k for a
 * rejected argument; the message is available from mava_last_error().
 *
 * Each entry cites the reference code it replaces (paths relative to the Mava repository).
 */
#ifndef MAVA_HIP_H
#define MAVA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mava_stream_t; /* hipStream_t */

/* ---- library ---------------------------------------------------------------------------- */
const char* mava_last_error(void); /* thread-local text of the last failure */
int mava_abi_version(void);

/* ---- context handle: the library keeps NO process-wide state ("no hidden globals except handles").
 * Everything that selects behaviour - the arithmetic of the matrix products, the critic aggregation, kernel variants for
 * bench sweeps - and every workspace the library allocates itself (the pre-split W1 copy of the wide f16x2 gradient
 * kernels) belongs to a handle the caller creates per learner and passes as the first argument of the entry points that
 * depend on it.  NULL is accepted everywhere and means the defaults (exact f32, aggregation on, default variants).  Two
 * handles share nothing; launches that share one handle must be issued on one stream (they share its W1 workspace).
 * In Mava the same choices are properties of the jitted learner function (mava/systems/ppo/ff_mappo.py:388-389). */
typedef struct mava_ctx mava_ctx;
enum {
  MAVA_CTX_MATMUL_MODE = 0,        /* 0 (default): exact-f32 MFMA; 1: "f16x2" - every matrix operand split into two f16 terms
                                      (hi + lo), three f16 MFMAs per product, f32 accumulation: 5.3x less matrix-pipe time, the
                                      same 1e-4 gradient parity tests; applies where a split-f16 kernel is instantiated
                                      (ppo_train_h2.hip, rec_dense_h2.hip, rec_gru_h2.hip), other shapes run exact f32 */
  MAVA_CTX_CRITIC_AGGREGATION = 1, /* 1 (default): a critic input row shared by the A agents of a (t,e) index (RWARE's global
                                      state, mava/wrappers/jumanji.py:53-59) is evaluated once and the sum of its agents' loss
                                      gradients back-propagated - the same gradient as A identical passes; 0: one pass per agent */
  MAVA_CTX_GAE_VARIANT = 2,        /* bench sweeps (tools/gae_sweep.py): chunk / lane mapping of mava_gae_f32, 0 = default */
  MAVA_CTX_POLICY_VARIANT = 3,     /* 0 = per-wave acting kernel / hybrid launch (default), 1 = per-wave only, 2 = block-cooperative */
  MAVA_CTX_H2_LAUNCHES = 4,        /* diagnostic counter: gradient launches of this handle that ran on the f16x2 kernels */
  MAVA_CTX_TRAIN_VARIANT = 5,      /* f16x2 gradient kernels, bit 0: 0 (default) = the eight-wave actor kernel (ppo_train_w8.hip) where it
                                      is instantiated, 1 = the four-wave kernels (ppo_train_h2.hip) only; bit 1: always run the x_lo
                                      products that inputs exact in f16 skip (same bits either way: tests); bit 2: the eight-wave kernel
                                      staging from an f16 record keeps the layer-1 weight gradient at the end of each tile instead of
                                      running it under the next tile's loss phase (same bits either way: tests); bit 3: that deferred form
                                      keeps its row gathers and cursor updates in front of barrier A instead of a tile further ahead
                                      (same bits either way: tests); for A/B measurements */
  MAVA_CTX_W8_LAUNCHES = 6,        /* diagnostic counter: ... of which on the eight-wave kernel */
  MAVA_CTX_W1_SPLIT_FRESH = 7,     /* read: 1 while the handle's pre-split W1 copy (wide f16x2 critic, 96..287 inputs) holds the W1 that
                                      mava_ppo_finish_f32 wrote for the critic at p + Pa, critic_din inputs.  The next
                                      mava_ppo_critic_grad_f32 of the handle clears it, whichever kernel it runs on, and skips its own
                                      re-split only when its params pointer and din are that key's; mava_ctx_set(MATMUL_MODE) clears it
                                      too.  Contract left to the caller: whoever rewrites the CONTENTS of that same parameter buffer
                                      between the finish call and the next critic launch (a copy-in, another optimiser step) must
                                      write 0 here - the next launch then re-splits W1 itself */
  MAVA_CTX_EXACT_TILES = 8,        /* diagnostic counter on the device: 32-row tiles that the blocks of the handle's wide f16x2
                                      gradient launches (96..287 inputs) ran in the exact-input tile loop - inputs exact in f16: hi plane
                                      only, two MFMAs per product, the next x tile staged beside this one (ppo_train_h2.hip) -, summed
                                      over launches.  Reading it waits for the device; 0 is the only value that can be written */
  MAVA_CTX_X16_LAUNCHES = 9,       /* diagnostic counter on the device: wide f16x2 critic launches of the handle that staged their input
                                      from the caller's f16 copy (mava_ppo_critic_grad_f32 with a valid input16).  Reading it waits for
                                      the device; 0 is the only value that can be written */
  MAVA_CTX_X16_W8_LAUNCHES = 10,   /* the same for the eight-wave f16x2 kernel (discrete actor <= 16 actions, value network on <= 127
                                      inputs): launches of mava_ppo_actor_grad_f32 / mava_ppo_critic_grad_f32 that staged their
                                      input from the f16 record */
  MAVA_CTX_W8_DEFER_LAUNCHES = 11, /* ... of which ran the deferred-dW1 tile loop (role-split instances, <= 8 actions, unless
                                      MAVA_CTX_TRAIN_VARIANT bit 2 is set).  Reading it waits for the device; 0 is the only value that
                                      can be written */
  MAVA_CTX_W8_AHEAD_LAUNCHES = 12  /* ... of which issued the x gathers a tile further ahead (the discrete actor's instances, unless
                                      MAVA_CTX_TRAIN_VARIANT bit 3 is set; the value network keeps its gathers).  Likewise */
};
int mava_ctx_create(mava_ctx** out);
int mava_ctx_destroy(mava_ctx* ctx); /* frees the handle's workspaces; NULL is a no-op */
int mava_ctx_set(mava_ctx* ctx, int key, long value);
int mava_ctx_get(const mava_ctx* ctx, int key, long* value);

/* ---- GAE: mava/systems/ppo/ff_mappo.py:112-139 (_calculate_gae);
 *           mava/systems/ppo/rec_mappo.py:177-199 when last_done != NULL.
 * reward,value,adv,tgt: (T,N) f32 time-major; done: (T,N) u8; last_val: (N) f32;
 * last_done: (N) u8 or NULL.  Recurrent mode: done[t] is the flag ENTERING step t and the mask
 * of step t is done[t+1] (done[T] := last_done). */
int mava_gae_f32(const mava_ctx* ctx, const float* reward, const float* value, const uint8_t* done,
                 const float* last_val, const uint8_t* last_done, int T, int N, float gamma,
                 float lambda, float* adv, float* tgt, mava_stream_t s);

/* ---- epoch permutation: jax.random.permutation(key, batch_size) of ff_mappo.py:272-273 / rec_mappo.py:277-279.
 * out[0..n) = a bijection of [0, n) determined by (seed, counter): 16-round keyed Feistel network over [0, 2^ceil(log2 n))
 * with cycle walking (mava_amd/csrc/permutation.hip; bit-exact restatement oracle/permutation.py).  1 <= n < 2^31. */
int mava_permutation_i32(long n, uint64_t seed, uint64_t counter, int32_t* out, mava_stream_t s);
/* The n_perm (1..16) epoch permutations of an update in one launch: out[k * out_stride + i] = what
 * mava_permutation_i32(n, seed, counter + k, .) writes at i, bit for bit.  out_stride >= n. */
int mava_permutation_batched_i32(long n, uint64_t seed, uint64_t counter, int n_perm, int32_t* out, long out_stride,
                                 mava_stream_t s);

/* ---- optimiser: optax.chain(clip_by_global_norm, adam(eps=1e-5)) per network,
 *      mava/systems/ppo/ff_mappo.py:359-366 (definition) and :241-250 (application);
 *      LR schedule mava/utils/training.py:20-64; pmean scaling ff_mappo.py:224-238.
 * p,g,m,v: flat f32 over all segments (networks); seg_off: host int[n_seg+1]; seg_lr: host
 * float[n_seg]; count: device int32[n_seg] (incremented).  g holds the SUM over replicas and
 * ranks; grad_scale = 1/(update_batch_size * n_devices).  loss_sums (device, 3 floats:
 * actor_loss, entropy, value_loss - same summation) and metrics_out (device, 4 floats:
 * total_loss, value_loss, actor_loss, entropy; ff_mappo.py:255-265) may both be NULL. */
int mava_clip_adam(float* p, const float* g, float* m, float* v, int32_t* count,
                   const int* seg_off, const float* seg_lr, int n_seg, float grad_scale,
                   float max_norm, int decay, int steps_per_update, int num_updates, float b1,
                   float b2, float eps, const float* loss_sums, float vf_coef, float ent_coef,
                   float* metrics_out, mava_stream_t s);

/* Tail of one minibatch on ONE rank with ONE update-batch replica (ff_mappo.py:224-266 with trivial pmeans) in two launches
 * instead of six: (1) the fixed-order sums of BOTH networks' gradient slabs (slab_a rows [Pa grads | actor_loss, entropy],
 * slab_c rows [Pc grads | value_loss]) into g = [actor | critic | actor_loss, entropy, value_loss, pad] - bit-identical to
 * two mava_slab_reduce2_f32 calls - leaving each block's squared-norm partial in the workspace; (2) clip + Adam as
 * mava_clip_adam (norms from those partials), the step-count increment and, through an arrival ticket, the re-split of a
 * wide f16x2 critic's W1 (critic_din in [96, 287], handle in f16x2 mode; 0 = none) for the handle's next gradient launch by
 * the block that finishes last.  workspace: mava_ppo_finish_workspace_bytes(Pa, Pc) bytes, 8-byte aligned, zeroed once by
 * the caller and owned by this call sequence afterwards. */
size_t mava_ppo_finish_workspace_bytes(int Pa, int Pc);
/* (n_slab = 0: `g` already holds the summed gradient and loss sums - the multi-rank path, whose all-reduce sits between the slab
 * sums and Adam: only the Adam launch runs, norms from g, still carrying the count increment and the W1 re-split.) */
int mava_ppo_finish_f32(mava_ctx* ctx, const float* slab_a, long stride_a, const float* slab_c, long stride_c, int n_slab,
                        int Pa, int Pc, float* g, float* p, float* m, float* v, int32_t* count, float lr_a, float lr_c,
                        float grad_scale, float max_norm, int decay, int steps_per_update, int num_updates, float b1,
                        float b2, float eps, float vf_coef, float ent_coef, float* metrics_out, int critic_din,
                        void* workspace, size_t workspace_bytes, mava_stream_t s);

/* out[i] = (accumulate ? out[i] : 0) + sum_b slab[b*slab_stride + i], b ascending.  n_slab == 0: the sum is zero and
 * slab is not read (it may be NULL); the same holds for mava_slab_reduce2_f32. */
int mava_slab_reduce_f32(const float* slab, int n_slab, long slab_stride, int n, int accumulate,
                         float* out, mava_stream_t s);

/* Same, with row columns [0,n_main) summed into out_main and [n_main, n_main+n_tail) into out_tail
 * (the loss sums that follow a gradient in a slab row). */
int mava_slab_reduce2_f32(const float* slab, int n_slab, long slab_stride, int n_main,
                          float* out_main, int n_tail, float* out_tail, int accumulate,
                          mava_stream_t s);

/* ---- networks: mava/networks.py:39-58 (MLPTorso [128,128] relu), :88-124
 *      (DiscreteActionHead), :172-207 (FeedForwardActor / FeedForwardValueNet).
 * Flat parameter layout [W1(din,128) | b1 | W2(128,128) | b2 | W3(128,n_out) | b3], kernels
 * row-major (in,out) as in flax.linen.Dense. */
int mava_mlp_param_count(int din, int n_out);

/* out (rows, n_out) = net(x[row / x_share]);  x: (ceil(rows/x_share), din). */
int mava_mlp_forward_f32(const mava_ctx* ctx, const float* params, int din, int n_out, const float* x, int x_share,
                         int rows, float* out, mava_stream_t s);

/* (Every *_continuous entry point and mava_rec_step_packed_f32 take ContinuousActionHead.min_scale - mava/networks.py:134,162,
 * default 1e-3: scale = softplus(log_std) + min_scale - right after the action dimension.)
 * One acting step, mava/systems/ppo/ff_mappo.py:80-85: actor forward + action mask
 * (networks.py:116-120) + Categorical sample / log_prob (distributions.py:146-165), and critic
 * forward, in one launch.  rows = envs*agents.  agents_view (rows, actor_din);
 * action_mask (rows, n_actions) u8 or NULL; critic_input (critic_rows/critic_share.., critic_din)
 * with critic row r reading input row r / critic_share; each critic output is written
 * value_broadcast times (value index r*value_broadcast + b).  Sampling: Gumbel-max on
 * Philox4x32-10 keyed by seed with counter (row_offset + row, step, word-group, "POLI").
 * forced_action (rows) i32 or NULL: score these actions instead of sampling.
 * logits (rows, n_actions) or NULL: raw (unmasked) logits out.
 * step_base (device, or NULL): a word added to `step` on the device, so that a captured HIP graph of a whole rollout
 * replays with the next counters (mava_synth_rware_step takes t_base likewise).
 * rows == 0 or critic_rows == 0 skips that half (its pointers may then be NULL): the learner runs the actor
 * half on the acting stream and the value half (mava_mlp_forward_f32) on a side stream. */
int mava_policy_step_f32(const mava_ctx* ctx, const float* actor_params, int actor_din, int n_actions,
                         const float* agents_view, const uint8_t* action_mask,
                         const float* critic_params, int critic_din, const float* critic_input,
                         int critic_share, int critic_rows, int value_broadcast, int rows,
                         uint64_t seed, uint32_t step, const uint32_t* step_base, uint32_t row_offset, int greedy,
                         const int32_t* forced_action, int32_t* action, float* log_prob,
                         float* value, float* logits, mava_stream_t s);

/* ---- PPO minibatch gradients: mava/systems/ppo/ff_mappo.py:150-218 (losses + value_and_grad)
 *      with the shuffle of :268-285 applied as an index vector (no shuffled copy).
 * The trajectory is the flat time-major batch of TE = T*E env rows with A agent rows each:
 * every per-agent array is (TE*A, ...).  A minibatch is Rb env rows: idx[b] (int32, a slice of the
 * epoch permutation) or idx_base + b when idx is NULL.  Each of the n_slab persistent blocks
 * writes one partial slab of slab_stride floats: [gradient in parameter layout | loss sums];
 * mava_slab_reduce_f32 sums the slabs in a fixed order.  All sums are already divided by the
 * minibatch element count Rb*A (the .mean() of the reference).  Row arithmetic is 32-bit: TE*A < 2^31. */

int mava_adv_stats_blocks(void); /* number of (sum, sumsq) f64 pairs mava_adv_stats_f64 writes */

/* advantage statistics for ff_mappo.py:164 (mean / population std over the whole minibatch) */
int mava_adv_stats_f64(const float* advantages, const int32_t* idx, long idx_base, int Rb, int A,
                       double* partials, mava_stream_t s);
/* the same for n_batch minibatches in one launch: minibatch j uses idx[j * idx_stride ...) and writes
 * partials[j][mava_adv_stats_blocks()][2] (all epochs x minibatches of an update, once GAE has run) */
int mava_adv_stats_batched_f64(const float* advantages, const int32_t* idx, long idx_stride, int Rb, int A,
                               int n_batch, double* partials, mava_stream_t s);

/* _actor_loss_fn, ff_mappo.py:150-180.  slab tail: [actor_loss, entropy].
 * input16 / input16_valid / input16_ld (NULL, NULL, 0: none): an f16 record of agents_view under the contract stated at
 * mava_ppo_critic_grad_f32: input16 (rows of agents_view, input16_ld) IEEE binary16, input16_valid its device word.  The
 * eight-wave kernel reads the word once per block and with 1 stages its input with 16-byte loads and LDS stores of the
 * halves - no conversion; the gradient has the same bits either way. */
int mava_ppo_actor_grad_f32(mava_ctx* ctx, const float* params, int din, int n_actions, const float* agents_view,
                            const uint8_t* action_mask, const int32_t* action, const float* old_log_prob,
                            const float* advantages, const double* adv_stats, const int32_t* idx, long idx_base, int Rb,
                            int A, float clip_eps, float ent_coef, float* slab, long slab_stride, int n_slab,
                            const uint16_t* input16, const uint32_t* input16_valid, int input16_ld, mava_stream_t s);

/* Continuous action head: Independent(TanhTransformed(Normal(loc, softplus(log_std) + 1e-3))),
 * mava/networks.py:127-169 + mava/distributions.py:24-91 (log_prob clipped at +-0.999, sampled entropy).
 * actor_params = [MLP(actor_din -> 128 -> 128 -> action_dim) | log_std(action_dim)], action_dim <= 16.
 *
 * mava_policy_step_continuous_f32: the acting step of mava_policy_step_f32 with action (rows, action_dim) float in
 * (-1, 1) = tanh(loc + scale * noise) (greedy: the mode tanh(loc), distributions.py:75-77); forced_action (or NULL)
 * scores given actions instead; mean (or NULL) receives loc.  The critic half is unchanged.
 *
 * mava_ppo_actor_grad_continuous_f32: _actor_loss_fn ff_mappo.py:150-180 for this head; the entropy sample of
 * ff_mappo.py:176-177 is drawn from Philox(counter (row_offset + trajectory row, ent_step, dim/2), key seed).
 * slab row = [MLP gradient | d/d log_std | actor_loss, entropy]. */
int mava_policy_step_continuous_f32(const mava_ctx* ctx, const float* actor_params, int actor_din, int action_dim, float min_scale,
                                    const float* agents_view, const float* critic_params, int critic_din,
                                    const float* critic_input, int critic_share, int critic_rows,
                                    int value_broadcast, int rows, uint64_t seed, uint32_t step,
                                    const uint32_t* step_base, uint32_t row_offset, int greedy,
                                    const float* forced_action, float* action, float* log_prob, float* value,
                                    float* mean, mava_stream_t s);
int mava_ppo_actor_grad_continuous_f32(const float* params, int din, int action_dim, float min_scale, const float* agents_view,
                                       const float* action, const float* old_log_prob, const float* advantages,
                                       const double* adv_stats, const int32_t* idx, long idx_base, int Rb, int A,
                                       float clip_eps, float ent_coef, uint64_t seed, uint32_t ent_step,
                                       uint32_t row_offset, float* slab, long slab_stride, int n_slab,
                                       mava_stream_t s);

/* _critic_loss_fn, ff_mappo.py:182-201.  critic_input row = agent_row / x_share.
 * slab tail: [value_loss, unused].
 * input16 / input16_valid / input16_ld (NULL, NULL, 0: none): an f16 copy of critic_input: input16 (rows of critic_input, din)
 * IEEE binary16, contiguous, 16-byte aligned, and input16_valid, one 32-bit device word written by whoever wrote the copy
 * (mava_rollout_ff_f32's state16_valid): 1 = input16 holds, for every element, the f16 high term f16(critic_input) that the
 * kernel would form itself, and the low term f16(critic_input - high) is zero everywhere (an input whose remainder
 * underflows f16, such as 1 + 2^-30, counts as exact there too: the f32 path drops the same remainder).  The wide f16x2
 * critic kernel (96..287 inputs) then reads the word on the device, once per block, and with 1 stages its input from the
 * copy - half the bytes, no conversion, every tile in the exact-input loop (MAVA_CTX_X16_LAUNCHES counts such launches);
 * the gradient has the same bits either way.  The copy is NOT read when the word is not 1, when either pointer is NULL,
 * din % 8 != 0, critic_input is not 16-byte aligned, MAVA_CTX_TRAIN_VARIANT bit 1 is set, or another kernel takes the
 * launch.  The host never reads the word.  Arguments rather than handle keys: the rollout takes no handle, and a learner
 * with several replicas has one copy per replica.
 * input16_ld: halves between rows of input16; 0 = din (all the wide kernel takes).  The eight-wave kernel (din <= 127,
 * x_share == 1, no aggregation) reads a record with input16_ld % 8 == 0 and input16_ld >= din on a 16-byte aligned base;
 * where input16_ld > din the row is laid out like mava_rollout_ff_f32's view16 (din values, 1.0, zeros to a multiple of
 * 8).  Such launches are counted by MAVA_CTX_X16_W8_LAUNCHES.  Odd din, a misaligned base or row, MAVA_CTX_TRAIN_VARIANT
 * bit 1, a word that is not 1: the record is not read. */
int mava_ppo_critic_grad_f32(mava_ctx* ctx, const float* params, int din, const float* critic_input, int x_share,
                             const float* old_value, const float* targets, const int32_t* idx,
                             long idx_base, int Rb, int A, float clip_eps, float vf_coef,
                             float* slab, long slab_stride, int n_slab, const uint16_t* input16,
                             const uint32_t* input16_valid, int input16_ld, mava_stream_t s);

/* Both gradient kernels read MAVA_CTX_MATMUL_MODE, the critic also MAVA_CTX_CRITIC_AGGREGATION, from their handle. */

/* Host only, no launch: 1 when a mava_ppo_actor_grad_f32 / mava_ppo_critic_grad_f32 call with this handle, input and record
 * would stage its input from input16 whenever input16_valid reads 1; 0 when it would read the f32 input whatever the word
 * says (another kernel takes the launch, alignment, input16_ld, MAVA_CTX_TRAIN_VARIANT, sharing / aggregation, a NULL
 * record); negative on an argument error.  The launchers answer with the expression they launch by: the rule is stated once,
 * in the library.  A caller that leaves the f32 input unwritten (mava_rollout_ff_flags_f32) asks here first. */
int mava_ppo_actor_grad_reads_input16(const mava_ctx* ctx, int din, int n_actions, const float* agents_view, int A,
                                      const uint16_t* input16, int input16_ld);
int mava_ppo_critic_grad_reads_input16(const mava_ctx* ctx, int din, const float* critic_input, int x_share, int A,
                                       const uint16_t* input16, int input16_ld);

/* ---- synthetic RWARE-shaped environment (measurement stand-in for the third-party Jumanji
 *      RobotWarehouse stepped at mava/systems/ppo/ff_mappo.py:88).  Wrapper semantics follow
 *      mava/wrappers/observation.py:41-53, jumanji.py:53-59,128-143, auto_reset_wrapper.py:88-101
 *      and episode_metrics.py:78-111.  One call = one vectorised env.step (or reset when is_reset).
 * state: step_count (E,A) i32, run_return/ep_return (E) f32, run_length/ep_length (E) i32.
 * outputs: agents_view (E,A,A+O), global_state (E,gs_tiles,W) with gs_tiles in {1,A} and W = A*O (concatenated
 * raw views, RWARE) when state_dim == 0 or W = state_dim (independent state vector, SMAX-shaped),
 * action_mask (E,A,n_actions) u8, obs_step_count (E,A) i32; transition: reward (E,A) f32,
 * done (E,A) u8, info_return (E) f32, info_length (E) i32, info_terminal (E) u8.
 * reward_mode 0: team reward Bernoulli(0.02), independent of the actions (the measurement workload);
 * reward_mode 1 ("match", for learning tests): team reward = fraction of the env's agents whose `action` (E,A) i32 -
 * taken on the previous observation - equals (that observation's first grid coordinate) mod n_actions. */
int mava_synth_rware_step(int E, int A, int O, int n_actions, int gs_tiles, int state_dim, int time_limit,
                          uint64_t seed, uint32_t t, const uint32_t* t_base, uint32_t env_offset, int is_reset,
                          int32_t* step_count, float* run_return, int32_t* run_length,
                          float* ep_return, int32_t* ep_length, float* agents_view,
                          float* global_state, uint8_t* action_mask, int32_t* obs_step_count,
                          float* reward, uint8_t* done, float* info_return, int32_t* info_length,
                          uint8_t* info_terminal, const int32_t* action, int reward_mode, mava_stream_t s);

/* ---- Level-Based Foraging environment step (mava_amd/csrc/lbf.hip; rules in DESIGN.md "Level-Based Foraging",
 *      restated in tests/lbf_model.py).  E environments of a G x G grid with A agents and F foods (A, F <= 16, G <= 32,
 *      (G-2)^2 >= 9 (F-1) + 1, G^2 >= F + A, max_agent_level <= 1000).  Actions (E, A) int32: 0 NOOP, 1 UP, 2 DOWN,
 *      3 LEFT, 4 RIGHT, 5 LOAD.  State (struct of arrays, advanced in place): agent_pos (E, A, 2), agent_level (E, A),
 *      food_pos (E, F, 2), food_level (E, F), food_alive (E, F) u8, total_food_level (E) f32, step_count (E, A) and the
 *      RecordEpisodeMetrics words run_return / run_length / ep_return / ep_length (E), as mava_synth_rware_step.
 *      Outputs: agents_view (E, A, A + 3 (F + A)) = [one-hot id | raw view], global_state (E, 1, A * 3 (F + A)) = the
 *      concatenated raw views, action_mask (E, A, 6) u8, obs_step_count (E, A); reward (E, A) (team: the agents' summed
 *      reward repeated per agent; individual_rewards 1: each agent's own), done (E, A), info_* (E).
 *      is_reset 1 generates every env (reward, done, info_* and action may then be NULL); a terminal step regenerates
 *      that env and returns the reset observation (AutoResetWrapper).  Randomness: Philox4x32-10 with key `seed`, counter
 *      (env_offset + e, t + *t_base, block, "LBFS"); t_base (a device word, may be NULL) is added on the device, so the
 *      step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL): what AutoResetWrapper keeps in extras["real_next_obs"]
 *      (mava/wrappers/auto_reset_wrapper.py:52-101), for rec_iql's replay buffer: real_view (E, A, A + 3 (F + A)) /
 *      real_mask (E, A, 6) are the observation of the state the rules produced BEFORE any auto-reset (equal to agents_view
 *      / action_mask where the step did not end), and terminated (E) is 1 only when every food was eaten - a time-limit end
 *      is a truncation (termination vs truncation as in Jumanji's LBF).  Every other output is the same with or without
 *      them.  None of the three is written on a reset call.  All three NULL: none of this is computed (the plain kernel
 *      instance); one or two of them NULL is an argument error; on a step they must not alias agents_view / action_mask. */
int mava_lbf_step(int E, int A, int F, int G, int fov, int max_agent_level, int force_coop, int individual_rewards,
                  int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base, uint32_t env_offset, int is_reset,
                  int32_t* agent_pos, int32_t* agent_level, int32_t* food_pos, int32_t* food_level, uint8_t* food_alive,
                  float* total_food_level, int32_t* step_count, float* run_return, int32_t* run_length, float* ep_return,
                  int32_t* ep_length, float* agents_view, float* global_state, uint8_t* action_mask,
                  int32_t* obs_step_count, float* reward, uint8_t* done, float* info_return, int32_t* info_length,
                  uint8_t* info_terminal, const int32_t* action, float* real_view, uint8_t* real_mask, uint8_t* terminated,
                  mava_stream_t s);

/* ---- Robot Warehouse environment step (mava_amd/csrc/rware.hip; rules in DESIGN.md "Robot Warehouse", restated in
 *      tests/rware_model.py; parity with Jumanji's RobotWarehouse is unpinned).  E environments of an H x W grid
 *      (H, W <= 32; coordinates (x = column, y = row), y grows downward) with A agents (<= 16), S shelves (<= 256) and
 *      R requested shelves (1 <= R <= 16, R < S); sensor_range in {1, 2}.  The layout is the caller's (HOST arrays, copied
 *      into the launch): highway_rows[H] - bit x of word y set when cell (x, y) is a highway - and shelf_home[S], the
 *      increasing non-highway cells (y * W + x) of shelves 0 .. S-1; the goals are (W/2 - 1, H - 1) and (W/2, H - 1).
 *      Actions (E, A) int32: 0 NOOP, 1 FORWARD, 2 LEFT, 3 RIGHT, 4 TOGGLE_LOAD; directions 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT.
 *      State (struct of arrays, advanced in place): agent_pos (E, A, 2) (x, y), agent_dir (E, A), agent_carry (E, A)
 *      (shelf id or -1), shelf_pos (E, S) (cell; a carried shelf has its carrier's cell, a ground shelf stands on a
 *      home cell), request_queue (E, R) (distinct shelf ids), step_count (E, A) and the RecordEpisodeMetrics words, as
 *      mava_lbf_step.  One step: turns and FORWARD moves (refused off the grid, or when a carried shelf would meet a
 *      ground shelf; agents do not block each other); a collision (two agents on one cell after the moves, or two that
 *      exchanged cells) ends the episode when collision_terminates is 1 and is ignored when 0; carried shelves follow;
 *      TOGGLE_LOAD in agent order (pick up the ground shelf of the cell / put down on a non-highway cell without one);
 *      deliveries in agent order (a carried, requested shelf on a goal scores 1 and its queue slot is refilled with the
 *      (draw mod (S - R))-th shelf outside the queue); reward = deliveries, the same for every agent; the episode also
 *      ends (a truncation) at time_limit.  Outputs: agents_view (E, A, A + raw) = [one-hot id | raw view], raw =
 *      8 + 7 (2 sensor_range + 1)^2: [x, y, carrying, direction one-hot (4), on_highway] then per view cell (rows outer)
 *      [agent, its direction one-hot (4), shelf, shelf requested]; global_state (E, 1, A * raw); action_mask (E, A, 5)
 *      u8 (FORWARD iff it would move); obs_step_count, reward, done (E, A); info_* (E).  is_reset 1 generates every env
 *      (reward, done, info_* and action may then be NULL); a terminal step regenerates that env and returns the reset
 *      observation.  Randomness: Philox4x32-10, key `seed`, counter (env_offset + e, t + *t_base, block, "RWRS") for a
 *      reset and (.., agent / 4, "RWRQ") word agent % 4 for a refill; t_base (a device word, may be NULL) is added on the
 *      device, so the step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL), as in mava_lbf_step: real_view (E, A, A + raw) /
 *      real_mask (E, A, 5) observe the state the rules produced BEFORE any auto-reset, and terminated (E) is 1 only on a
 *      collision termination - a time-limit end is a truncation.  None of the three is written on a reset call.  All three
 *      NULL: none of this is computed (the plain kernel instance); one or two of them NULL is an argument error; on a step
 *      they must not alias agents_view / action_mask. */
int mava_rware_step(int E, int A, int S, int R, int H, int W, int sensor_range, int time_limit, int collision_terminates,
                    const uint32_t* highway_rows, const int32_t* shelf_home, uint64_t seed, uint32_t t,
                    const uint32_t* t_base, uint32_t env_offset, int is_reset, int32_t* agent_pos, int32_t* agent_dir,
                    int32_t* agent_carry, int32_t* shelf_pos, int32_t* request_queue, int32_t* step_count,
                    float* run_return, int32_t* run_length, float* ep_return, int32_t* ep_length, float* agents_view,
                    float* global_state, uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                    float* info_return, int32_t* info_length, uint8_t* info_terminal, const int32_t* action,
                    float* real_view, uint8_t* real_mask, uint8_t* terminated, mava_stream_t s);

/* ---- Connector environment step (mava_amd/csrc/connector.hip; rules in DESIGN.md "Connector", stated in
 *      tests/connector_model.py, which is the contract; parity with Jumanji's MaConnector is unpinned).  E environments
 *      of a G x G board (3 <= G <= 16) with A agents (1 <= A <= 32, 2 A <= G G - 2).  Actions (E, A) int32: 0 NOOP, 1 UP
 *      (row - 1), 2 RIGHT (col + 1), 3 DOWN (row + 1), 4 LEFT (col - 1).  State (struct of arrays, advanced in place):
 *      head (E, A, 2) and target (E, A, 2) as (row, col), connected (E, A) u8, grid (E, G, G) u8 with 0 empty and
 *      1 + 3k / 2 + 3k / 3 + 3k a path cell / the head / the target of agent k (a head on its own target is stored as
 *      head), step_count (E, A) and the RecordEpisodeMetrics words, as mava_lbf_step.  One step, every test made on the
 *      grid at its start: an unconnected agent moves iff its destination is on the grid and empty or its own target, and
 *      no other agent wants the same cell; it leaves a path cell behind and is connected on its target.  Team reward
 *      (repeated per agent) = (100 c - 3 o) / 100 with c the agents that connected on this step and o those not
 *      connected at its start.  The episode terminates when no agent has a legal move (all connected or blocked) and is
 *      truncated at time_limit.  Outputs: agents_view (E, A, G G 5), cell-major with the channels last and NO agent id in
 *      front: for a cell of agent k seen by agent j, rel = ((k - j) mod A) + 1, [rel / A on a head, rel / A on a target,
 *      1 on a path, 1 on j's own head, 1 on j's own target]; global_state (E, 1, G G 3) = agent 0's channels 0..2;
 *      action_mask (E, A, 5) u8 (NOOP always, a move iff it would be allowed); obs_step_count, reward, done (E, A);
 *      info_* (E).  is_reset 1 generates every env (reward, done, info_* and action may then be NULL); a terminal step
 *      regenerates that env and returns the reset observation.  Randomness: Philox4x32-10, key `seed`, counter
 *      (env_offset + e, t + *t_base, block, "CONR"); t_base (a device word, may be NULL) is added on the device, so the
 *      step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL), as in mava_lbf_step: real_view (E, A, G G 5) / real_mask
 *      (E, A, 5) observe the state the rules produced BEFORE any auto-reset, and terminated (E) is 1 when no agent has a
 *      legal move - a time-limit end alone is a truncation.  None of the three is written on a reset call.  All three NULL:
 *      none of this is computed (the plain kernel instance); one or two of them NULL is an argument error; on a step they
 *      must not alias agents_view / action_mask. */
int mava_connector_step(int E, int A, int G, int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base,
                        uint32_t env_offset, int is_reset, int32_t* head, int32_t* target, uint8_t* connected,
                        uint8_t* grid, int32_t* step_count, float* run_return, int32_t* run_length, float* ep_return,
                        int32_t* ep_length, float* agents_view, float* global_state, uint8_t* action_mask,
                        int32_t* obs_step_count, float* reward, uint8_t* done, float* info_return, int32_t* info_length,
                        uint8_t* info_terminal, const int32_t* action, float* real_view, uint8_t* real_mask,
                        uint8_t* terminated, mava_stream_t s);

/* ---- Cleaner environment step (mava_amd/csrc/cleaner.hip; rules in DESIGN.md "Cleaner", stated in
 *      tests/cleaner_model.py, which is the contract; parity with Jumanji's Cleaner is unpinned).  E environments of an
 *      R x C board (3 <= R, C <= 32, rectangles allowed) with A agents (1 <= A <= 32) that may share a cell.  One byte
 *      per cell: 0 dirty, 1 clean, 2 wall.  Actions (E, A) int32: 0 UP (row - 1), 1 RIGHT (col + 1), 2 DOWN (row + 1),
 *      3 LEFT (col - 1); there is no no-op, and any other value is an invalid action.  State (struct of arrays, advanced
 *      in place): pos (E, A, 2) as (row, col), grid (E, R, C) u8, step_count (E, A) and the RecordEpisodeMetrics words,
 *      as mava_lbf_step.
 *      Reset: rooms are the cells with even row and even column, nr = (R + 1) / 2 by nc = (C + 1) / 2 of them; every
 *      other cell starts as a wall.  Room q = i nc + j has the edge 2q to room (i, j + 1) through cell (2i, 2j + 1) and
 *      the edge 2q + 1 to room (i + 1, j) through cell (2i + 1, 2j), each only where that room exists (ids are skipped,
 *      not renumbered).  Edge n has the key "draw n" = word n % 4 of Philox block n / 4; the maze opens exactly the cells
 *      of the minimum spanning tree under the weight (key, id), compared lexicographically: 2 nr nc - 1 open cells, an
 *      even R (C) leaves a solid last row (column).  All open cells are dirty, all agents start at (0, 0), which is
 *      cleaned at once, step_count = 0.
 *      One step: (1) an agent whose destination is on the board and not a wall moves, any other stays and its action
 *      was invalid; (2) every dirty cell that now holds an agent becomes clean, n = the number of such CELLS; (3) team
 *      reward n - 0.5, repeated per agent; (4) step_count += 1; won = no dirty cell left, invalid = some action was
 *      invalid; done = won | invalid | step_count >= time_limit; terminated = won | invalid (a time-limit end alone is
 *      a truncation); info_won = done & won.  Outputs: agents_view (E, A, R C 4), cell-major with the channels last and
 *      NO agent id in front: [dirty, wall, agents in the cell as a float, 1 on the viewer's own cell]; global_state
 *      (E, 1, R C 3) = the first three channels; action_mask (E, A, 4) u8 = validity of each move on the new board (every
 *      agent always has a legal move); obs_step_count, reward, done (E, A); info_* (E); info_won (E) u8 may be NULL.
 *      is_reset 1 generates every env (reward, done, info_* and action may then be NULL, info_won is not written); a
 *      terminal step regenerates that env and returns the reset observation.  Randomness: Philox4x32-10, key `seed`,
 *      counter (env_offset + e, t + *t_base, block, "CLNR"); t_base (a device word, may be NULL) is added on the device,
 *      so the step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL), as in mava_lbf_step: real_view (E, A, R C 4) / real_mask
 *      (E, A, 4) observe the state the rules produced BEFORE any auto-reset, and terminated (E) is won | invalid - a time-
 *      limit end alone is a truncation.  None of the three is written on a reset call.  All three NULL: none of this is
 *      computed (the plain kernel instance); one or two of them NULL is an argument error; on a step they must not alias
 *      agents_view / action_mask. */
int mava_cleaner_step(int E, int A, int R, int C, int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base,
                      uint32_t env_offset, int is_reset, int32_t* pos, uint8_t* grid, int32_t* step_count,
                      float* run_return, int32_t* run_length, float* ep_return, int32_t* ep_length, float* agents_view,
                      float* global_state, uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                      float* info_return, int32_t* info_length, uint8_t* info_terminal, uint8_t* info_won,
                      const int32_t* action, float* real_view, uint8_t* real_mask, uint8_t* terminated, mava_stream_t s);

/* ---- SMAX environment step (mava_amd/csrc/smax.hip; rules in DESIGN.md "SMAX", stated in tests/smax_model.py, which is
 *      the contract; parity with JaxMARL's SMAX is unpinned).  E environments of A allies (the agents, 1 <= A <= 16)
 *      against Ne scripted enemies (1 <= Ne <= 16) on a 32 x 32 map; U = A + Ne units, allies first.  ally_types /
 *      enemy_types hold one nibble per unit: 0 marine, 1 marauder, 2 stalker, 3 zealot, 4 zergling, 5 hydralisk, with
 *      (health, damage, attack range, sight range, speed, weapon cooldown in sub-steps) = (45, 9, 5, 9, 3.15, 10),
 *      (125, 10, 6, 10, 2.25, 18), (160, 13, 6, 10, 4.13, 30), (150, 8, 2, 9, 3.15, 14), (35, 5, 2, 8, 4.13, 8),
 *      (80, 12, 5, 9, 3.15, 10).  Actions (E, A) int32, 5 + Ne of them: 0 N (y+), 1 E (x+), 2 S (y-), 3 W (x-), 4 stop,
 *      5 + k attack enemy k.  State (struct of arrays, advanced in place): pos (E, U, 2) f32 (x, y), health (E, U) f32
 *      (integer values), cd (E, U) i32, last_action (E, U) i32, step_count (E, A) and the RecordEpisodeMetrics words, as
 *      mava_lbf_step.  All float arithmetic is f32, one rounded operation at a time; distances are compared squared.
 *      Reset: unit j uses draws 2j and 2j + 1 ("draw n" = word n % 4 of Philox block n / 4), u = (word >> 8) 2^-24;
 *      allies start at (6 + 4u, 14 + 4u'), enemies at (22 + 4u, 14 + 4u'), health full, cd 0, last_action 4.
 *      One step: (1) a dead ally's action becomes 4; a value that is no action, or an attack on a dead enemy or on one
 *      farther than the ally's range, is executed as 4.  (2) A living enemy takes the closest living ally within its
 *      sight (ties to the lowest index): within its range it attacks it (5 + ally), otherwise it moves along the axis
 *      with the larger |delta| (ties to x) towards it; with no ally in sight it moves the same way towards (16, 16) and
 *      stops once both |delta| < 0.5.  Both from the state at the start of the step.  (3) Eight sub-steps of 1/16 time
 *      units: MOVE - a living unit with action 0..3 adds speed / 16 to one coordinate; with walls_cause_death a mover
 *      whose new coordinate leaves [0, 32] dies; positions are clipped to [0, 32]; FIRE - unit u fires at its target v
 *      iff both are alive after the move, d2(u, v) <= range_u^2 and cd_u = 0; DAMAGE - health = max(0, health - the sum
 *      of the damage of the units firing at it), for all targets at once; COOLDOWN - a unit that fired sets cd to its
 *      type's value, every other unit alive after the move counts cd down to 0.  (4) Team reward, repeated per agent:
 *      (sum over enemies k, ascending, of fl(lost health_k / max health_k)) / Ne, plus 1 iff every enemy is dead and an
 *      ally lives.  (5) step_count += 1; terminated = a side is wiped out; done = terminated | step_count >=
 *      time_limit; info_won = done & (every enemy dead & an ally alive).  (6) last_action = the action executed.
 *      Outputs, on the new state: agents_view (E, A, A + 11 (U - 1) + 10) = the one-hot agent id, then for a living
 *      viewer i one block per other ally (ascending) and per enemy, [health / max, dx / sight_i, dy / sight_i,
 *      (last_action + 1) / (5 + max(A, Ne)), cd / type cd, type one-hot (6)] with (dx, dy) = other - viewer, all zero
 *      if the other is dead or farther than sight_i, the last_action entry zero for enemies unless see_enemy_actions;
 *      then the own block [health / max, x / 32, y / 32, cd / type cd, type one-hot (6)]; a dead viewer has zeros after
 *      the id.  global_state (E, 1, 12 U): per unit the own block and a team one-hot (ally, enemy), zero for the dead.
 *      action_mask (E, A, 5 + Ne) u8: a dead ally only 4; a living one 0..4 and 5 + k iff enemy k is alive and in
 *      range.  obs_step_count, reward, done (E, A); info_* (E); info_won (E) u8 may be NULL.
 *      is_reset 1 generates every env (reward, done, info_* and action may then be NULL, info_won is not written); a
 *      terminal step regenerates that env and returns the reset observation.  Randomness: Philox4x32-10, key `seed`,
 *      counter (env_offset + e, t + *t_base, block, "SMAX"); t_base (a device word, may be NULL) is added on the device,
 *      so the step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL), as in mava_lbf_step: real_view (E, A, obs_dim) /
 *      real_mask (E, A, 5 + Ne) observe the state the rules produced BEFORE any auto-reset, and terminated (E) says that a
 *      side was wiped out - a time-limit end alone is a truncation.  None of the three is written on a reset call.  All
 *      three NULL: none of this is computed (the plain kernel instance); one or two of them NULL is an argument error; on a
 *      step they must not alias agents_view / action_mask. */
int mava_smax_step(int E, int A, int Ne, uint64_t ally_types, uint64_t enemy_types, int time_limit, int see_enemy_actions,
                   int walls_cause_death, uint64_t seed, uint32_t t, const uint32_t* t_base, uint32_t env_offset,
                   int is_reset, float* pos, float* health, int32_t* cd, int32_t* last_action, int32_t* step_count,
                   float* run_return, int32_t* run_length, float* ep_return, int32_t* ep_length, float* agents_view,
                   float* global_state, uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                   float* info_return, int32_t* info_length, uint8_t* info_terminal, uint8_t* info_won,
                   const int32_t* action, float* real_view, uint8_t* real_mask, uint8_t* terminated, mava_stream_t s);

/* ---- Spread environment step (mava_amd/csrc/spread.hip; rules in DESIGN.md "Spread", stated in tests/spread_model.py,
 *      which is the contract).  This project's own continuous-action task, modelled on MPE simple_spread; it restates no
 *      environment of the reference.  E environments of A agents and A landmarks (2 <= A <= 8) in [-1, 1]^2.  Actions
 *      (E, A, 2) f32.  State (struct of arrays, advanced in place): agent_pos, landmark_pos (E, A, 2) f32 (x, y),
 *      step_count (E, A) and the RecordEpisodeMetrics words, as mava_lbf_step.  All float arithmetic is f32, one rounded
 *      operation at a time.  Reset: agent i uses draws 2i, 2i + 1 and landmark l draws 2A + 2l, 2A + 2l + 1 ("draw n" =
 *      word n % 4 of Philox block n / 4); a coordinate is 2u - 1 with u = (word >> 8) 2^-24.
 *      One step: (1) c = fmin(fmax(a, -1), 1) per component, p = fmin(fmax(p + fl(0.1 c), -1), 1); there are no
 *      velocities.  (2) Team reward, repeated per agent: with d(p, q) = sqrt(fl(fl(dx dx) + fl(dy dy))), near_l = min
 *      over agents of d(agent, landmark l), n = the number of agent pairs u < v with d < 0.15:
 *      -fl((sum over l, ascending, of near_l) / A) - fl(fl(0.5 n) / A), the divisions being products with fl(1 / A).
 *      (3) step_count += 1; terminated = 0 (the rules never end an episode); done = step_count >= time_limit.
 *      Outputs, on the new state: agents_view (E, A, [A +] 2 + 2A + 2(A - 1)) = the one-hot agent id (only with
 *      add_agent_id), the own position, the landmarks minus self (ascending), the other agents minus self (ascending,
 *      skipping self).  global_state (E, 1, 4A): the agent positions, then the landmark positions.  action_mask
 *      (E, A, 2) u8: all ones.  obs_step_count, reward, done (E, A); info_* (E).
 *      is_reset 1 generates every env (reward, done, info_* and action may then be NULL); a step that reaches the time
 *      limit regenerates that env and returns the reset observation.  Randomness: Philox4x32-10, key `seed`, counter
 *      (env_offset + e, t + *t_base, block, "SPRD"); t_base (a device word, may be NULL) is added on the device, so the
 *      step replays from a captured graph.  No host state, no synchronisation.
 *      real_view / real_mask / terminated (all three or all NULL), as in mava_lbf_step, for an off-policy replay: real_view
 *      (E, A, obs_dim) / real_mask (E, A, 2) observe the state the rules produced BEFORE any auto-reset; terminated (E) is
 *      always 0 - a time-limit end is a truncation; real_state (E, 1, 4A), which may be NULL with them given and must be
 *      NULL without them, is the pre-reset global_state (ff_masac's next state).  None of them is written on a reset call.
 *      The three NULL: none of this is computed (the plain kernel instance); one or two of them NULL is an argument error;
 *      on a step they must not alias agents_view / action_mask / global_state. */
int mava_spread_step(int E, int A, int add_agent_id, int time_limit, uint64_t seed, uint32_t t, const uint32_t* t_base,
                     uint32_t env_offset, int is_reset, float* agent_pos, float* landmark_pos, int32_t* step_count,
                     float* run_return, int32_t* run_length, float* ep_return, int32_t* ep_length, float* agents_view,
                     float* global_state, uint8_t* action_mask, int32_t* obs_step_count, float* reward, uint8_t* done,
                     float* info_return, int32_t* info_length, uint8_t* info_terminal, const float* action,
                     float* real_view, uint8_t* real_mask, uint8_t* terminated, float* real_state, mava_stream_t s);

/* ---- fused rollout: the whole `lax.scan(_env_step, length=T)` of mava/systems/ppo/ff_mappo.py:76-106 for one
 *      update-batch replica on the synthetic RWARE-shaped environment, plus the bootstrap value of :109-110, in ONE
 *      launch (mava_amd/csrc/rollout_h2.hip): every workgroup owns 64 / A environments for all T steps (environments
 *      are independent, the parameters fixed), weights register-resident, observations handed from the env phase to
 *      the next acting step through LDS.  Same Philox streams as mava_policy_step_f32 (seed policy_seed, counter
 *      (row_offset + row, t0 + t, ., "POLI")) and mava_synth_rware_step (seed env_seed, step t0 + t + 1): bit-identical
 *      observations / masks / rewards / dones / metrics; networks in split-f16 arithmetic (see MAVA_CTX_MATMUL_MODE).
 *      critic_shared 1: centralised critic on global_state (T+1, E, A*O), one value per env broadcast to its agents;
 *      0: decentralised critic on agents_view (global_state unused).  Slot 0 of agents_view / global_state /
 *      action_mask must hold the current observation; slots 1..T are written, the env state is advanced in place.
 *      adv / tgt (T, E, A) or both NULL: when given, every (env, agent) column's GAE (ff_mappo.py:112-139, sequential
 *      f32 recurrence) runs in the kernel's tail on the rewards / values / dones just written - no separate pass.
 *      Three optional groups of outputs, each NULL or given on its own:
 *      last_reward / last_done (E, A) = reward[T-1] / done[T-1], what a caller otherwise copies after the launch; only with
 *      them, step_counter: when not NULL, *step_counter += T (one thread, at the kernel's end: pass it for ONE replica of
 *      an update; the launch counts from t0 and never reads it).
 *      state16 / state16_valid, an f16 copy of the shared global state for mava_ppo_critic_grad_f32's input16: state16
 *      (T+1, E, A*O) IEEE binary16, contiguous, 16-byte aligned - every slot, slot 0 included, is written by the launch
 *      with the halves the kernel's LDS image holds (global_state is their conversion to f32) - and state16_valid, one
 *      32-bit device word that must hold 0 or 1 on entry (allocate it zeroed) and is left 1 when every value the launch
 *      loaded from slot 0 of global_state had a zero low f16 term f16(x - f16(x)), else 0; with 1, state16[t] is the f16
 *      high term of global_state[t] that the critic kernel would form itself, for every t < T (slots 1 .. T-1 are
 *      float(state16[t]) == global_state[t] bit for bit always; slot 0 is the caller's, and a value there whose remainder
 *      underflows f16 counts as exact, as it does in the f32 staging path).  (Between entry and the end of the launch the
 *      word counts blocks; the last block stores the result.)  Needs critic_shared and A*O % 8 == 0.
 *      view16 / view16_valid, an f16 record of agents_view for mava_ppo_actor_grad_f32's input16 (and
 *      mava_ppo_critic_grad_f32's under a decentralised critic): view16 (T+1, E, A, RP) IEEE binary16 with RP =
 *      8 * ceil((A + O + 1) / 8), contiguous, 16-byte aligned - every slot's row is the row of the kernel's LDS image:
 *      halves [0, A+O) the observation (agents_view is their conversion to f32), half A+O 1.0, the rest 0 - and
 *      view16_valid, a device word under state16_valid's protocol (0 or 1 on entry; left 1 when every slot-0 value of
 *      agents_view had a zero low f16 term, else 0).  Every instance takes it, shared critic or not.
 *      Returns 0, a negative error, or 1 when the shape is not instantiated (the caller then runs mava_policy_step_f32
 *      + mava_synth_rware_step per step): needs 64 % A == 0, n_actions <= 8, the RWARE-style global state. */
int mava_rollout_ff_f32(const float* actor_params, int n_actions, const float* critic_params, int critic_shared,
                        int E, int A, int O, int T, int time_limit, uint64_t policy_seed, uint64_t env_seed,
                        uint32_t t0, uint32_t row_offset, uint32_t env_offset, int reward_mode,
                        int32_t* step_count, float* run_return, int32_t* run_length, float* ep_return,
                        int32_t* ep_length, float* agents_view, float* global_state, uint8_t* action_mask,
                        int32_t* obs_step_count, int32_t* action, float* value, float* reward, float* log_prob,
                        uint8_t* done, float* last_val, float* info_return, int32_t* info_length,
                        uint8_t* info_terminal, float* adv, float* tgt, float gamma, float gae_lambda,
                        float* last_reward, uint8_t* last_done, int32_t* step_counter, uint16_t* state16,
                        uint32_t* state16_valid, uint16_t* view16, uint32_t* view16_valid, mava_stream_t s);
/* mava_rollout_ff_f32 with flags (mava_rollout_ff_f32 is this entry point with flags 0; the twin is to be folded into one
 * entry point at the next ABI bump).  A set bit leaves the f32 record of slots 1 .. T-1 of one array UNWRITTEN - the launch
 * does not touch those bytes - where the f16 record of the same array holds the same values:
 *   MAVA_ROLLOUT_SKIP_AGENTS_VIEW (bit 0): agents_view; needs view16 / view16_valid.
 *   MAVA_ROLLOUT_SKIP_GLOBAL_STATE (bit 1): global_state; needs state16 / state16_valid.
 * A bit without its record, or an unknown bit, is an argument error: nothing is launched.  Slot T is always written in f32,
 * slot 0 stays the caller's, and every other output - both records and both words included - has the bits it has with
 * flags 0.  The skipped slots are float(record) by the records' contract whatever the words say; the words say whether
 * the gradient kernels may read the records INSTEAD of the f32 arrays.  A caller that skips therefore runs
 * mava_rollout_expand_f32 (force 0) behind the launch - it rebuilds the slots only when a word is not 1 - and skips an
 * array only when every gradient launch that follows would read its record (mava_ppo_actor_grad_reads_input16,
 * mava_ppo_critic_grad_reads_input16). */
#define MAVA_ROLLOUT_SKIP_AGENTS_VIEW 1u
#define MAVA_ROLLOUT_SKIP_GLOBAL_STATE 2u
int mava_rollout_ff_flags_f32(const float* actor_params, int n_actions, const float* critic_params, int critic_shared,
                              int E, int A, int O, int T, int time_limit, uint64_t policy_seed, uint64_t env_seed,
                              uint32_t t0, uint32_t row_offset, uint32_t env_offset, int reward_mode,
                              int32_t* step_count, float* run_return, int32_t* run_length, float* ep_return,
                              int32_t* ep_length, float* agents_view, float* global_state, uint8_t* action_mask,
                              int32_t* obs_step_count, int32_t* action, float* value, float* reward, float* log_prob,
                              uint8_t* done, float* last_val, float* info_return, int32_t* info_length,
                              uint8_t* info_terminal, float* adv, float* tgt, float gamma, float gae_lambda,
                              float* last_reward, uint8_t* last_done, int32_t* step_counter, uint16_t* state16,
                              uint32_t* state16_valid, uint16_t* view16, uint32_t* view16_valid, uint32_t flags,
                              mava_stream_t s);
/* Slots 1 .. T-1 of the f32 arrays rebuilt from the f16 records of a fused rollout, in one launch: agents_view[t] = the
 * conversion of halves [0, A+O) of every view16 row, global_state[t] = the conversion of state16[t] - exact, by the records'
 * contract.  Each group (agents_view, view16, view16_valid) / (global_state, state16, state16_valid) is given whole or NULL
 * whole.  force 0: an array is rebuilt only when its word is not 1 (read on the device, once per block: with 1 the launch
 * does nothing); force != 0: always.  Slots 0 and T are not touched. */
int mava_rollout_expand_f32(int T, int E, int A, int O, float* agents_view, const uint16_t* view16,
                            const uint32_t* view16_valid, float* global_state, const uint16_t* state16,
                            const uint32_t* state16_valid, int force, mava_stream_t s);
/* The bootstrap observation becomes the first observation of the next rollout: slot T -> slot 0 of agents_view
 * (T+1, E, A, obs_dim) f32, global_state (T+1, E, gs_dim) f32 (NULL with gs_dim 0: none), action_mask (T+1, E, A,
 * n_actions) u8 and step_count (T+1, E, A) i32, in one launch.  Slots 1..T are not touched. */
int mava_rollout_carry(int T, int E, int A, int obs_dim, long gs_dim, int n_actions, float* agents_view,
                       float* global_state, uint8_t* action_mask, int32_t* step_count, mava_stream_t s);

/* ---- recurrent systems (rec_ippo / rec_mappo): mava/networks.py:238-331 (ScannedRNN GRU with
 *      reset-on-done, RecurrentActor, RecurrentValueNet), mava/systems/ppo/rec_mappo.py:91-149,
 *      :210-266, :334-365.  Internal activations use the "T32" tile layout: element (row, f) of a
 *      (rows x N) matrix lives at ((row/32)*N + f)*32 + row%32; rows is a multiple of 32.  A sequence batch
 *      is time-major: row = t*Rm + m, m = (local env)*A + agent; external trajectory arrays are (T,E,A,..)
 *      and env ids come from idx (Rm/A entries, a slice of the env permutation) or the identity. */

/* Y = act(X W + b) [masked by gate > 0]; X is T32 (x_ld >= K features per 32-row tile, the first K used; x_ld <= 0
 * means K) or, with x_rowmajor, the external row-major source (row stride x_ld >= K, so a call can read a column
 * block) gathered per batch row; W (K x N) row-major with row stride ldw; Y T32 (rows x N).  accumulate: start from
 * the existing Y (K-chunked products for inputs wider than 384).  With MAVA_CTX_MATMUL_MODE = 1 T32 inputs run on
 * split-f16 operands (rec_dense_h2.hip: 3 f16 MFMAs per product, f32 accumulate, operands must sit in f16 range -
 * see grad_scale below); row-major inputs, N in 129..256 and K above 288 with a bias always run the exact-f32 kernel
 * ("Support envelope of the dense and X^T Y products").  y_ld (<= 0: N) is the feature count of the
 * y / gate tiles: a call with a column block of W and y + 32 * n0 writes features [n0, n0 + N) of a wider matrix. */
int mava_rec_dense_f32(const mava_ctx* ctx, const float* x, int x_rowmajor, const int32_t* idx, int Rm, int E, int A,
                       int x_share, int x_ld, int accumulate, const float* w, int ldw, const float* bias,
                       const float* gate, float* y, int y_ld, int K, int N, int rows, int relu, mava_stream_t s);

/* per-block slabs of out_scale * dW = X^T Y (K x N row-major) followed by out_scale * db = colsum(Y) when want_bias;
 * y_ld (<= 0: N) = features per y tile (y + 32 * n0 reads a column block of a wider matrix).
 * out_scale undoes the grad_scale the backward chain was started with (1.0f when none). */
int mava_rec_xty_f32(const mava_ctx* ctx, const float* x, int x_rowmajor, const int32_t* idx, int Rm, int E, int A,
                     int x_share, int x_ld, const float* y, int y_ld, const float* y_tail, int y_split, int y_tail_ld, int K, int N,
                     int rows, int want_bias, float out_scale, float* slab, long slab_stride, int n_slab, mava_stream_t s);
/* (y_tail, round 3: when not NULL, features [y_split, N) of Y are features [0, N - y_split) of the T32 matrix y_tail with
 * y_tail_ld features per tile; y_split a multiple of 32.  The BPTT scan's dgh is [dgi's r and z thirds | its own n third].) */
/* Row-major, env-permuted observation slice of a minibatch (same gather description as mava_rec_dense_f32 with
 * x_rowmajor) -> T32 matrix `out` with k_pad >= K features per tile (zeros past K): done once per minibatch, read by
 * the pre-torso product and by its weight-gradient product as a plain T32 operand. */
int mava_rec_gather_t32_f32(const float* x, const int32_t* idx, int Rm, int E, int A, int x_share, int x_ld, int K,
                            int rows, int k_pad, float* out, mava_stream_t s);

/* GRU over T steps (flax GRUCell; hidden state zeroed where done enters the step).  gi = W_i x + b_i
 * precomputed (T32, T*Rm x 384); wh (128 x 384) = [hr|hz|hn]; outputs hs (T32, h after each step) and,
 * for training, hprev (masked h entering each step) and saved (T*Rm x 512 = [r|z|n|W_hn h + b_hn]). */
int mava_gru_scan_fwd_f32(const mava_ctx* ctx, int T, int Rm, int E, int A, const int32_t* idx, const uint8_t* done,
                          const float* h0, int h0_t32, const float* wh, const float* bhn,
                          const float* gi, float* hs, float* hprev, float* saved, mava_stream_t s);

/* BPTT through the same scan: dh_out (T32) is the gradient reaching each h_t from the output path;
 * writes dgi and dgh (T32, T*Rm x 384: gradients w.r.t. the input-side and hidden-side gate pre-activations). */
int mava_gru_scan_bwd_f32(const mava_ctx* ctx, int T, int Rm, int E, int A, const int32_t* idx, const uint8_t* done,
                          const float* wh, const float* saved, const float* hprev, const float* dh_out,
                          float* dgi, float* dgh, int dgh_n_only, mava_stream_t s);
/* (dgh_n_only != 0: dgh is T32 (T*Rm x 128) and receives the n third of the hidden-side gate gradient alone - its r and z
 * thirds equal dgi's, since the gates add the two pre-activations (flax GRUCell); the scan is HBM-bound, the two thirds
 * were a sixth of its traffic.) */

/* sequence losses on T32 logits / values: rec_mappo.py:210-242 and :244-266 (after the re-unroll);
 * loss_partials: (n_blocks, 2) partial sums already divided by the element count.  The gradient w.r.t. the network
 * outputs is written TIMES grad_scale: loss gradients are O(1 / rows), below f16's normal range at 10^6 rows, so the
 * backward chain (dense, BPTT scan - all linear in the gradient) runs in units of a power of two near `rows` and
 * mava_rec_xty_f32(out_scale = 1 / grad_scale) returns to true units; exact in f32, 1.0f for none. */
int mava_seq_actor_loss_f32(int T, int Rm, int E, int A, int n_actions, const int32_t* idx,
                            const float* logits, const uint8_t* mask, const int32_t* action,
                            const float* old_log_prob, const float* advantages, const double* adv_stats,
                            int n_stats, float clip_eps, float ent_coef, float grad_scale, float* dlogits,
                            float* loss_partials, int n_blocks, mava_stream_t s);
/* Continuous head on the recurrent systems (rec_mappo.py:210-242 with networks.py:127-169): `mean` / `dmean` are T32
 * (T*Rm x action_dim) like logits / dlogits of mava_seq_actor_loss_f32, `action` is the external (T, E, A, action_dim)
 * buffer, `log_std` the action_dim raw scales; dscale_partials (n_blocks x action_dim) receives d loss / d log_std
 * partials (already times sigmoid(log_std)).  Entropy noise: Philox counter (row_offset + trajectory row, ent_step, dim/2).
 * ContinuousActionHead(independent_std=False) (networks.py:140,161): log_std_rows is the T32 (T*Rm x action_dim) output
 * of the log_std layer (log_std may then be NULL) and dlog_std_rows receives its gradient (times grad_scale) instead of
 * dscale_partials; both NULL for the observation-independent scale. */
int mava_seq_actor_loss_continuous_f32(int T, int Rm, int E, int A, int action_dim, float min_scale, const int32_t* idx,
                                       const float* mean, const float* log_std, const float* log_std_rows,
                                       const float* action, const float* old_log_prob, const float* advantages,
                                       const double* adv_stats, int n_stats, float clip_eps, float ent_coef, uint64_t seed,
                                       uint32_t ent_step, uint32_t row_offset, float grad_scale, float* dmean,
                                       float* dlog_std_rows, float* loss_partials, float* dscale_partials, int n_blocks,
                                       mava_stream_t s);
/* rollout epilogue: T32 means of one step -> action (rows, action_dim) = tanh(loc + scale * noise), log_prob (rows) */
int mava_seq_sample_continuous_f32(int rows, int action_dim, float min_scale, const float* mean, const float* log_std,
                                   const float* log_std_rows, uint64_t seed,
                                   uint32_t step, uint32_t row_offset, int greedy, float* action, float* log_prob,
                                   mava_stream_t s);
/* agents_per_row = 1: one value per agent row (T, E, A).  agents_per_row = n > 1 (then A must be 1): the rows are
 * (t, env) rows whose n agents share the critic input (centralised critic on a tiled global state); old_value /
 * targets are (T, E, n) and the row's gradient is the sum of its agents' loss gradients - the same gradient as n
 * identical network passes. */
int mava_seq_critic_loss_f32(int T, int Rm, int E, int A, int agents_per_row, const int32_t* idx, const float* values,
                             const float* old_value, const float* targets, float clip_eps, float vf_coef,
                             float grad_scale, float* dvalues, float* loss_partials, int n_blocks, mava_stream_t s);

/* The OUTPUT PATH of a recurrent network in one launch on split-f16 operands (rec_out_h2.hip): post_torso -> head ->
 * PPO loss (rec_mappo.py:210-242 actor / :244-266 critic) -> backward through both layers.  hs: T32 (T*Rm x 128) hidden
 * states; params_post_head: [Wpost | bpost | Whead | bhead] (the tail of the flat parameters); is_actor: f0 / f1 =
 * old_log_prob / advantages (+ mask, action, adv_stats), else old_value / targets with agents_per_row as in
 * mava_seq_critic_loss_f32.  Writes dh (T32, d loss / d hs TIMES grad_scale) and per-block slabs [dWpost | dbpost | dWhead |
 * dbhead | loss sums (2)] in true units.  Returns 1 (nothing launched) for shapes it does not instantiate: more than 16
 * outputs, n_slab > tiles - the caller then runs the layer-wise kernels. */
int mava_rec_out_f32(int T, int Rm, int E, int A, int n_out, int agents_per_row, const int32_t* idx, const float* hs,
                     const float* params_post_head, const uint8_t* mask, const int32_t* action, const float* f0,
                     const float* f1, const double* adv_stats, int n_stats, float clip_eps, float coef, float grad_scale,
                     int is_actor, float* dh, float* slab, long slab_stride, int n_slab, mava_stream_t s);

/* rollout epilogue: masked Categorical sample + log_prob from T32 logits of one step (rows = E*A). */
int mava_seq_sample_f32(int rows, int n_actions, const float* logits, const uint8_t* mask, uint64_t seed,
                        uint32_t step, uint32_t row_offset, int greedy, int32_t* action, float* log_prob,
                        mava_stream_t s);

/* Fused recurrent ACTING step: rec_mappo.py:108-129 (_env_step) for both networks in one launch -
 * pre_torso -> GRU cell with reset-on-done (networks.py:238-266) -> post_torso -> head, then mask / Gumbel-max
 * sample / log-prob (actor; same Philox stream as mava_seq_sample_f32) or the value (critic).
 * Parameters: the recurrent flat layout [Wpre | bpre | Wi | bi | Wh | bhn | Wpost | bpost | Whead | bhead].
 * agents_view (rows_a, actor_din), critic_input (ceil(rows_c / critic_share), critic_din) row-major;
 * done_* u8 flags entering the step, one per row (critic row r reads done_c[r * done_c_stride]: stride A reads the
 * per-agent flags of an env's first agent when the critic runs once per env); h_*_in / h_*_out: T32 (rows x 128)
 * hidden states, distinct buffers;
 * rows_* multiples of 32 (0 skips that network); value (rows_c * value_broadcast). */
int mava_rec_step_f32(const float* actor_params, int actor_din, int n_actions, const float* agents_view,
                      const uint8_t* action_mask, const uint8_t* done_a, const float* h_actor_in,
                      float* h_actor_out, int rows_a, uint64_t seed, uint32_t step, uint32_t row_offset,
                      int greedy, int32_t* action, float* log_prob, const float* critic_params, int critic_din,
                      const float* critic_input, int critic_share, const uint8_t* done_c, int done_c_stride,
                      const float* h_critic_in, float* h_critic_out, int rows_c, int value_broadcast,
                      float* value, mava_stream_t s);
/* the same fused acting step with ContinuousActionHead: actor_params = [recurrent network | log_std(action_dim)],
 * action (rows_a, action_dim) float = tanh(loc + scale * noise) (noise stream of mava_seq_sample_continuous_f32). */
int mava_rec_step_continuous_f32(const float* actor_params, int actor_din, int action_dim, float min_scale, const float* agents_view,
                                 const uint8_t* done_a, const float* h_actor_in, float* h_actor_out, int rows_a,
                                 uint64_t seed, uint32_t step, uint32_t row_offset, int greedy, float* action,
                                 float* log_prob, const float* critic_params, int critic_din,
                                 const float* critic_input, int critic_share, const uint8_t* done_c, int done_c_stride,
                                 const float* h_critic_in, float* h_critic_out, int rows_c, int value_broadcast,
                                 float* value, mava_stream_t s);

/* The same acting step on split-f16 operands with PRE-PACKED weights (rec_step_h2.hip): mava_rec_step_pack_f32 splits
 * one network's [Wpre | Wi | Wh | Wpost] into f16 hi / lo planes in MFMA-fragment order (mava_rec_step_pack_bytes(din)
 * bytes); do it once per rollout, after the parameters changed.  mava_rec_step_packed_f32 takes both packs plus the
 * arguments of mava_rec_step_f32 (action_f != NULL selects the continuous head: then action / action_mask are unused and
 * n_actions is the action dimension); a block multiplies each weight fragment with up to three 32-row tiles.  More than
 * 16 head outputs run the exact-f32 kernel. */
long mava_rec_step_pack_bytes(int din);
int mava_rec_step_pack_f32(const float* params, int din, void* pack, mava_stream_t s);
int mava_rec_step_packed_f32(const void* pack_a, const void* pack_c, const float* actor_params, int actor_din,
                             int n_actions, float min_scale, const float* agents_view, const uint8_t* action_mask, const uint8_t* done_a,
                             const float* h_actor_in, float* h_actor_out, int rows_a, uint64_t seed, uint32_t step,
                             uint32_t row_offset, int greedy, int32_t* action, float* action_f, float* log_prob,
                             const float* critic_params, int critic_din, const float* critic_input, int critic_share,
                             const uint8_t* done_c, int done_c_stride, const float* h_critic_in, float* h_critic_out,
                             int rows_c, int value_broadcast, float* value, mava_stream_t s);

/* ---- rec_iql (mava/systems/q_learning/rec_iql.py; csrc/rec_step.hip, csrc/q_learning.hip) ----
 * Acting step (:241-276): the recurrent Q network of mava_rec_step_f32's actor (same flat parameters, same T32 hidden
 * state, reset where done), then MaskedEpsGreedyDistribution (mava/distributions.py:94-138): greedy action = the first
 * argmax of where(mask, q, finfo(f32).min); with probability eps a uniformly drawn valid action instead.  Word x of Philox
 * (row_offset + row, step, 0, "QEPS") with key seed decides (u01_open(x) < eps), word y picks the valid action
 * floor(y * n_valid / 2^32).  rows a multiple of 32, 1 <= n_actions <= 16; q_out (rows, n_actions) or NULL. */
int mava_rec_q_step_f32(const float* params, int din, int n_actions, const float* agents_view, const uint8_t* action_mask,
                        const uint8_t* done, const float* h_in, float* h_out, int rows, float eps, uint64_t seed, uint32_t step,
                        uint32_t row_offset, int32_t* action, float* q_out, mava_stream_t s);
/* Replay add (flashbax add with a time axis of 1): writes time slot `slot` of every field for all E envs into buffers laid
 * out (E, capacity, A, ...): obs / next_obs (.., O) f32, action_mask / next_mask (.., n_actions) u8, action i32, reward
 * f32, terminal u8 (the per-env flag `terminal` (E) repeated per agent), term_or_trunc u8.  Inputs are (E, A, ...). */
int mava_replay_add_f32(int E, int A, int O, int n_actions, int capacity, int slot, const float* obs, const uint8_t* action_mask,
                        const int32_t* action, const float* reward, const uint8_t* terminal, const uint8_t* term_or_trunc,
                        const float* next_obs, const uint8_t* next_mask, float* b_obs, uint8_t* b_mask, int32_t* b_action,
                        float* b_reward, uint8_t* b_terminal, uint8_t* b_term_or_trunc, float* b_next_obs,
                        uint8_t* b_next_mask, mava_stream_t s);
/* Replay sample: B windows of S consecutive steps.  Sample b draws Philox (b, counter, 0, "RBSM") with key seed: env =
 * floor(x E / 2^32), k = floor(y n_win / 2^32) with filled = min(n_added, capacity) and n_win = filled - S + 1; the window
 * starts at step n_added - filled + k (slot modulo capacity), so it lies in the filled region and never crosses the write
 * head.  Every field is gathered time-major (S, Rp, ...) with rows b * A + agent; rows from B * A to Rp (a multiple of 32)
 * are zero with term_or_trunc = 1.  pairs (B, 2) i32 = (env, start slot). */
int mava_replay_sample_f32(int E, int A, int O, int n_actions, int capacity, uint32_t n_added, int B, int S, int Rp, uint64_t seed,
                           uint32_t counter, const float* b_obs, const uint8_t* b_mask, const int32_t* b_action,
                           const float* b_reward, const uint8_t* b_terminal, const uint8_t* b_term_or_trunc,
                           const float* b_next_obs, const uint8_t* b_next_mask, float* obs, uint8_t* action_mask, int32_t* action,
                           float* reward, uint8_t* terminal, uint8_t* term_or_trunc, float* next_obs, uint8_t* next_mask,
                           int32_t* pairs, mava_stream_t s);
/* Double-Q TD loss (:368-410) on three T32 (L*Rp x n_actions) Q arrays, rows t * Rp + m, real where m < n_real:
 * a* = first argmax of where(next_mask, q_next_online, finfo.min), target = reward + (1 - terminal_next) * gamma *
 * q_next_target[a*], dq (T32, same shape) = 2 (q[a] - target) / N * grad_scale at the taken action a and 0 elsewhere
 * (N = L * n_real; padding rows get 0).  partials (nblk, 3): per-block sums of (q_loss, mean_q, mean_target), each
 * already divided by N (their column sums are the metrics).  action / reward / terminal_next (L, Rp), next_mask
 * (L, Rp, n_actions). */
int mava_q_td_loss_f32(int L, int Rp, int n_actions, int n_real, const float* q, const float* q_next_online,
                       const float* q_next_target, const int32_t* action, const float* reward, const uint8_t* terminal_next,
                       const uint8_t* next_mask, float gamma, float grad_scale, float* dq, float* partials, int nblk,
                       mava_stream_t s);
/* Target network update (:411-418): hard = 0: target = tau * online + (1 - tau) * target (optax.incremental_update);
 * hard = 1: target = online (optax.periodic_update on a step where it fires; the caller decides when). */
int mava_target_update_f32(long n, const float* online, float* target, float tau, int hard, mava_stream_t s);

/* ---- value decomposition (rec_qmix / rec_vdn, mava/systems/q_learning/rec_qmix.py; mava_amd/csrc/qmix.hip).  Agent rows
 *      are t * Rp + b * A + j as above (Rp a multiple of 32 with B * A <= Rp); a MIXER row is t * Bp + b with
 *      Bp = ceil32(B), padding where b >= B.  All matrices are T32.
 * The mixer's state: state / next_state (T32, L * Bp rows x k_pad features, k_pad >= A * O) from the time-major sample
 * obs / next_obs (>= L, Rp, O): row (t, b), feature j * O + f = obs[t, b * A + j, f]; padding rows and the features from
 * A * O on are 0.  A pure gather (bit exact).  The outputs must not alias each other or an input. */
int mava_qmix_state_t32_f32(int L, int B, int A, int O, int Rp, int k_pad, const float* obs, const float* next_obs, float* state,
                            float* next_state, mava_stream_t s);
/* TD loss through the mixer in one launch.  q / q_next_online / q_next_target: T32 (L * Rp x n_actions); action / reward /
 * terminal_next (L, Rp), next_mask (L, Rp, n_actions) as for mava_q_td_loss_f32.  Per real mixer row: qa_j = q[action_j],
 * a*_j = first argmax of where(next_mask, q_next_online, finfo.min), qnext_j = q_next_target[a*_j], r = mean_j reward,
 * terminal = agent 0's flag, y = r + (1 - terminal) * gamma * Q_tot_target(qnext), loss = mean (Q_tot(qa) - y)^2 over the
 * N = L * B real mixer rows.  mode 1 (qmix): Q_tot = sum_k elu(sum_j qa_j |w1[j * Em + k]| + b1[k]) |w2[k]| + b2 with the
 * hypernet outputs w1 (L * Bp x A * Em), b1, w2 (x Em), b2 (x 1), pre-abs, and the target ones likewise; mode 0 (vdn):
 * Q_tot = sum_j qa_j, every hypernet pointer may be NULL and Em is ignored.  Outputs in units of grad_scale: dq (T32, every
 * element written: 0 off the taken action and on padding agent rows) and, in mode 1, d_w1 / d_b1 / d_w2 / d_b2 (T32, the
 * gradient w.r.t. the pre-abs outputs; d|x|/dx = 0 at 0; padding mixer rows 0).  partials (nblk, 3): per-block sums of
 * (q_loss, mean_q, mean_target) already divided by N; a block without rows writes zeros.  The gradients do not depend on
 * nblk.  Refused: A outside [1, 16], Em outside [1, 64] (mode 1), n_actions outside [1, 32], Rp not a multiple of 32 holding
 * B * A, nblk outside [1, 4096], a NULL pointer (hypernet pointers in mode 1), dq aliasing a Q input, a hypernet gradient
 * aliasing its input. */
int mava_qmix_td_f32(int mode, int L, int B, int A, int Rp, int n_actions, int Em, const float* q, const float* q_next_online,
                     const float* q_next_target, const int32_t* action, const float* reward, const uint8_t* terminal_next,
                     const uint8_t* next_mask, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w1_target, const float* b1_target, const float* w2_target, const float* b2_target, float gamma,
                     float grad_scale, float* dq, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* partials, int nblk,
                     mava_stream_t s);

/* ---- soft actor-critic (ff_isac / ff_masac): mava/systems/sac/ff_isac.py:245-384, ff_masac.py,
 *      mava/utils/centralised_training.py (mava_amd/csrc/sac.hip).  The actor (ContinuousActionHead with
 *      independent_std = False) and the two Q networks (torso -> Dense(1) on [state | action]) run on the general layer
 *      path; these kernels produce and consume its T32 matrices.  Buffer fields, sampled batches, actions and noise are
 *      row-major; the rows of a batch are b * A + agent, `rows` is a multiple of 32 and the rows from n_real on are padding:
 *      every kernel writes zeros there.  A (rows x 1) T32 matrix (a Q value) is a plain vector.
 *
 * Item replay, fbx.make_item_buffer(add_batches=True) (ff_isac.py:171-176, :257-258): a ring of `capacity` items, an item
 * being one env's transition for all agents: obs (A, O), action (A, D), reward (A), done (A) u8, next_obs (A, O) and, with
 * S > 0 (MASAC), global_state and next_global_state (S), stored once per item.  Add writes the E items of one acting step to
 * slots (head + e) mod capacity (E <= capacity); its `done` is one flag per env (E), stored for every agent. */
int mava_sac_replay_add_f32(int E, int A, int O, int D, int S, int capacity, int head, const float* obs, const float* action,
                            const float* reward, const uint8_t* done, const float* next_obs, const float* gs,
                            const float* next_gs, float* b_obs, float* b_action, float* b_reward, uint8_t* b_done,
                            float* b_next_obs, float* b_gs, float* b_next_gs, mava_stream_t s);
/* Sample B items with replacement (:395): item b draws word 0 of the Philox block with key `seed` and counter
 * (b, counter, 0, "SACB"); k = floor(word * filled / 2^32) with filled = min(n_added, capacity) (n_added: items added so
 * far); the item is slot (n_added - filled + k) mod capacity (k counts from the oldest).  Gathers to rows b * A + agent of
 * obs / next_obs (Rp, O), action (Rp, D), reward / done (Rp) (padding: zeros, done 1), gs / next_gs (B, S), and writes
 * the chosen slots to index (B). */
int mava_sac_replay_sample_f32(int A, int O, int D, int S, int capacity, uint32_t n_added, int B, int Rp, uint64_t seed,
                               uint32_t counter, const float* b_obs, const float* b_action, const float* b_reward,
                               const uint8_t* b_done, const float* b_next_obs, const float* b_gs, const float* b_next_gs,
                               float* obs, float* action, float* reward, uint8_t* done, float* next_obs, float* gs,
                               float* next_gs, int32_t* index, mava_stream_t s);
/* Reparameterised sample (pi.sample + pi.log_prob of :291-293, :310-312, :369-371, :425-426): mean / log_std T32
 * (rows x action_dim), scale = softplus(log_std) + min_scale, eps = the standard normal of (row_offset + row, step,
 * component) in the stream "SACN" of key `seed`, action = tanh(mean + scale eps), log_prob = the sum over components of
 * TanhTransformedDistribution.log_prob(action) (clip to +-0.999, tail masses beyond it).  action / eps (rows, action_dim),
 * log_prob (rows); log_prob and eps may be NULL.  1 <= action_dim <= 16. */
int mava_sac_sample_f32(int rows, int n_real, int action_dim, float min_scale, const float* mean, const float* log_std,
                        uint64_t seed, uint32_t step, uint32_t row_offset, float* action, float* log_prob, float* eps,
                        mava_stream_t s);
/* The Q-network input [state | action block] as a T32 matrix of x_ld >= O + W features per tile (zeros past O + W, as
 * mava_rec_gather_t32_f32's k_pad); row r reads state row r / x_share of the
 * row-major (., O) array (x_share = A for a global state stored once per item).  joint 0 (ISAC): W = action_dim, the row's
 * own action - action_new when given, else action.  joint 1 (MASAC): W = A action_dim, the actions of all agents of the
 * row's item from `action` (get_joint_action); with action_new the row's OWN slot comes from action_new
 * (get_updated_joint_actions).  action / action_new (rows, action_dim). */
int mava_sac_concat_f32(int rows, int n_real, int O, int x_share, int A, int action_dim, int joint, const float* state,
                        const float* action, const float* action_new, float* x, int x_ld, mava_stream_t s);
/* update_q (:305-340): target = reward + (1 - done) gamma (min(q1_target, q2_target) - exp(log_alpha[agent])
 * log_prob_next), agent = row % A; dq1 = 2 (q1 - target) / n_real * grad_scale, dq2 likewise; target (rows, may be NULL);
 * partials (nblk, 4): per-block sums of [q1_loss, q2_loss, mean q1, mean q2] (their sum over blocks is the value). */
int mava_sac_q_loss_f32(int rows, int n_real, int A, const float* q1, const float* q2, const float* q1_target,
                        const float* q2_target, const float* log_prob_next, const float* reward, const uint8_t* done,
                        const float* log_alpha, float gamma, float grad_scale, float* dq1, float* dq2, float* target,
                        float* partials, int nblk, mava_stream_t s);
/* actor_loss_fn (:284-299) differentiated through the sample: L = mean(exp(log_alpha) logp - min(q1, q2)).  Inputs: the
 * sample (mean, log_std T32; eps, action row-major), q1 / q2, and dx1 / dx2: T32 (rows x K) gradients of sum(q1) / sum(q2)
 * w.r.t. the Q input in units of q_scale, whose features [action_offset (+ agent * action_dim when joint), + action_dim)
 * are the row's own action.  Unclipped components: d logp / d mean = 2 a, d logp / d scale = -1 / scale + 2 a eps; clipped
 * ones (|a| >= 0.999): the tail mass's derivatives alone.  The Q path carries (1 - a^2) and goes to the smaller of q1, q2.
 * Writes dmean / dlog_std T32 (rows x action_dim) times grad_scale (dlog_std w.r.t. the raw log_std: times sigmoid) and
 * partials (nblk, 2): per-block sums of [actor loss, mean log_prob]. */
int mava_sac_actor_grad_f32(int rows, int n_real, int A, int action_dim, float min_scale, const float* mean,
                            const float* log_std, const float* eps, const float* action, const float* log_alpha,
                            const float* q1, const float* q2, const float* dx1, const float* dx2, int K, int action_offset,
                            int joint, float q_scale, float grad_scale, float* dmean, float* dlog_std, float* partials,
                            int nblk, mava_stream_t s);
/* alpha_loss_fn (:301-302): loss = mean over (B, A) of -exp(log_alpha[a]) (log_prob + target_entropy).  grad (A) =
 * d loss / d log_alpha; loss_parts (A): each agent's share (their sum is the loss). */
int mava_sac_alpha_loss_f32(int n_real, int A, const float* log_prob, const float* log_alpha, float target_entropy,
                            float* grad, float* loss_parts, mava_stream_t s);

/* T32 <-> row-major conversion of a (rows x N) matrix. */
int mava_t32_convert_f32(const float* src, int N, int rows, int to_t32, float* dst, mava_stream_t s);

/* ---- general network path (torsos the fused kernels do not instantiate): mava/networks.py:39-58 MLPTorso with any
 *      layer_sizes, activation relu | tanh and use_layer_norm, mava/networks.py:61-85 CNNTorso.  Products run on
 *      mava_rec_dense_f32 / mava_rec_xty_f32; these are the kernels between them.  act: 0 none, 1 relu, 2 tanh. */
/* y = act(LayerNorm(x) + ln_bias) (flax LayerNorm over the last axis, eps 1e-6, no scale) or act(x); xhat (T32) and
 * rstd (rows) are saved for the backward pass when use_layer_norm. */
int mava_t32_norm_act_f32(const float* x, int N, long rows, int use_layer_norm, const float* ln_bias, int act, float* y,
                          float* xhat, float* rstd, mava_stream_t s);
/* dz = dy * act'(y) (the bias gradient is its column sum); dx = gradient w.r.t. the layer-norm input (= dz without it) */
int mava_t32_norm_act_bwd_f32(const float* dy, const float* y, int N, long rows, int use_layer_norm, const float* xhat,
                              const float* rstd, int act, float* dz, float* dx, mava_stream_t s);
/* GRU cell one time step at a time, for network.hidden_state_dim != 128 (mava/networks.py:222-266: ScannedRNN over flax
 * GRUCell; the register-resident scans mava_gru_scan_* serve 128).  All matrices T32 over the `rows` sequences of the step;
 * done_t / done_next: the external (E, A) u8 flags ENTERING that step, rows mapped through idx like the scans; the
 * recurrent products (h W_h, dgh W_h^T) are mava_rec_dense_f32 launches between these kernels.
 *   mask:      hprev = done_t ? 0 : h
 *   gates:     hs = GRUCell(gi, gh = hprev W_h, b_hn, hprev); saved (rows x 4 Hd) = [r | z | n | gh_n + b_hn] or NULL;
 *              hprev_next (or NULL) = done_next ? 0 : hs
 *   gates_bwd: dh = dh_out + (done_next ? 0 : acc_next + dhp_next) (acc_next = dgh_{t+1} W_h^T; NULL at the last step);
 *              dgi, dgh (rows x 3 Hd) and dhp = dh z */
int mava_t32_gru_mask_f32(const float* h, const uint8_t* done_t, const int32_t* idx, int E, int A, int Hd, long rows,
                          float* hprev, mava_stream_t s);
int mava_t32_gru_gates_f32(const float* gi, const float* gh, const float* bhn, const float* hprev, int Hd, long rows, float* hs,
                           float* saved, float* hprev_next, const uint8_t* done_next, const int32_t* idx, int E, int A,
                           mava_stream_t s);
int mava_t32_gru_gates_bwd_f32(const float* saved, const float* hprev, const float* dh_out, const float* acc_next,
                               const float* dhp_next, const uint8_t* done_next, const int32_t* idx, int E, int A, int Hd,
                               long rows, float* dgi, float* dgh, float* dhp, mava_stream_t s);
/* per-block partial column sums of a T32 matrix times `scale`: slab (n_slab, slab_stride >= N) */
int mava_t32_colsum_f32(const float* y, int N, long rows, float scale, float* slab, long slab_stride, int n_slab,
                        mava_stream_t s);
/* nn.Conv(padding='SAME') as a product: patches of (Hin, Win, C) images -> T32 (samples*Hout*Wout x k*k*C), feature
 * (ky*k + kx)*C + c = a row of the flattened (k, k, C, Cout) kernel.  src_flat = 1: source T32 (samples x Hin*Win*C) (the
 * gathered observations); 0: source T32 (samples*Hin*Win x C) (the previous conv layer).  col2im is its adjoint. */
int mava_t32_im2col_f32(const float* src, int src_flat, long samples, int Hin, int Win, int C, int k, int stride,
                        float* dst, mava_stream_t s);
int mava_t32_col2im_f32(const float* dcol, int src_flat, long samples, int Hin, int Win, int C, int k, int stride,
                        float* dsrc, mava_stream_t s);
/* jax.lax.collapse(x, -3): T32 (samples*P x C) -> T32 (samples x P*C) (to_flat = 1) and back (0) */
int mava_t32_flatten_f32(const float* src, long samples, int P, int C, int to_flat, float* dst, mava_stream_t s);

/* ---- Multi-Agent Transformer (ff_mat; csrc/mat.hip): what sits between the dense products of the encoder and the
 *      decoder.  All matrices T32 with `rows` a multiple of 32; agent row b * A + j belongs to sample b, rows past B * A
 *      (valid_rows) are padding and come out exact zero.  Sums in f64, storage f32, no atomics; outputs bit-identical for
 *      any n_blocks. */
/* y = concat_heads(softmax(q k^T / sqrt(D / n_head)) v) over the A <= 32 agents of each sample, D / n_head <= 128; with
 * `causal` agent i sees the keys j <= i.  q may come from another matrix than k and v (cross-attention).  p (or NULL):
 * T32 (rows x n_head * A) receives the probabilities, feature h * A + j, exact zero above the diagonal when causal. */
int mava_mat_attn_fwd_f32(const float* q, const float* k, const float* v, long rows, int D, int B, int A, int n_head,
                          int causal, float* y, float* p, int n_blocks, mava_stream_t s);
/* dq, dk, dv from dy and the saved q, k, v (linear in dy: a grad_scale passes through).  The probabilities are computed
 * again in f64 from q and k: the softmax backward cancels, and the f32 copy in p is not accurate enough for it. */
int mava_mat_attn_bwd_f32(const float* dy, const float* q, const float* k, const float* v, long rows, int D, int B, int A,
                          int n_head, int causal, float* dq, float* dk, float* dv, int n_blocks, mava_stream_t s);
/* y = LayerNorm(x + res) * scale + bias over the last axis (flax: eps 1e-6, biased variance); res may be NULL, any N >= 1;
 * xhat (T32) and rstd (rows) are saved for the backward pass (both NULL for inference). */
int mava_mat_ln_fwd_f32(const float* x, const float* res, const float* scale, const float* bias, int N, long rows,
                        long valid_rows, float* y, float* xhat, float* rstd, int n_blocks, mava_stream_t s);
/* dx (= dres) and per-block slabs (n_slab, slab_stride >= 2 N) of out_scale * [dscale (N) | dbias (N)], to be summed by
 * mava_slab_reduce_f32; a block without tiles writes exact zeros. */
int mava_mat_ln_bwd_f32(const float* dy, const float* xhat, const float* rstd, const float* scale, int N, long rows,
                        long valid_rows, float out_scale, float* dx, float* slab, long slab_stride, int n_slab, mava_stream_t s);
/* flax nn.gelu (tanh approximation) on n floats, and dx = dy * gelu'(x) */
int mava_mat_gelu_f32(const float* x, long n, float* y, mava_stream_t s);
int mava_mat_gelu_bwd_f32(const float* dy, const float* x, long n, float* dx, mava_stream_t s);
/* The decoder's input, T32 (rows x n_pad), n_pad = ceil32(n_actions + 1): row (b, 0) = e_0, row (b, i) = [0 | onehot(action[
 * sample, i - 1])] for 1 <= i <= known, zero rows after that (acting: known = agents decoded so far; training: A - 1).
 * action: (samples, A) i32; sample = idx[b], or b when idx is NULL. */
int mava_mat_shift_onehot_f32(const int32_t* action, const int32_t* idx, int B, int A, int n_actions, int known, long rows,
                              int n_pad, float* out, mava_stream_t s);
/* One step of the autoregressive decode: agent `agent` of each of the B samples draws from the masked Categorical of its
 * T32 logits row (rows x n_actions, n_actions <= 64; mask (B, A, n_actions) u8 or NULL) exactly as mava_seq_sample_f32
 * does for row b * A + agent - same masking, same Philox counters - and writes action / log_prob[b * A + agent]. */
int mava_mat_sample_f32(int B, int A, int agent, int n_actions, const float* logits, const uint8_t* mask, uint64_t seed,
                        uint32_t step, uint32_t row_offset, int greedy, int32_t* action, float* log_prob, mava_stream_t s);
/* mava_seq_actor_loss_f32's and mava_seq_critic_loss_f32's formulas on a minibatch of Bm (t, env) samples whose A agent
 * rows are contiguous: row b * A + j reads the (samples, A[, n_actions]) trajectory arrays at sample idx[b].  Means over
 * the Bm * A agent rows; adv_stats from mava_adv_stats_f64 over the same rows.  Writes dlogits (T32) and dvalues (rows),
 * both times grad_scale (dvalues includes vf_coef), zero on padding rows, and loss_partials (n_blocks, 3) =
 * [actor_loss, entropy, value_loss] partial means. */
int mava_mat_loss_f32(int Bm, int A, int n_actions, long rows, const int32_t* idx, const float* logits, const float* values,
                      const uint8_t* mask, const int32_t* action, const float* old_log_prob, const float* advantages,
                      const float* old_value, const float* targets, const double* adv_stats, int n_stats, float clip_eps,
                      float ent_coef, float vf_coef, float grad_scale, float* dlogits, float* dvalues, float* loss_partials,
                      int n_blocks, mava_stream_t s);

/* ---- ff_mat, fused acting (csrc/mat_act.hip): one env step of the autoregressive decode in ONE launch, with a per-sample
 *      key/value cache.  Equal to mava_rec_gather_t32_f32 + the encoder + A x (mava_mat_shift_onehot_f32 + the decoder +
 *      mava_mat_sample_f32) up to the summation order of the dense products, which are plain f32 FMAs here whatever the
 *      context's matmul mode; same masking and same Philox counters as mava_mat_sample_f32. */
/* length of the flat vector [encoder | decoder] (mat_learner.param_spec); the kernel derives every leaf's offset from these
 * four numbers */
long mava_transformer_param_count(int O, int n_actions, int D, int n_block);
/* bytes of the caller's device workspace (the decoder's key/value cache of every block of the grid) */
size_t mava_transformer_act_workspace_bytes(int B, int A, int D, int n_block, int n_blocks);
/* agents_view (B, A, O) row-major; mask (B, A, n_actions) u8 or NULL; action, log_prob (B, A); value (B, A) or NULL.
 * 1 <= A <= 32, D a multiple of 32 up to 128 and of n_head, 1 <= n_actions <= 64, 1 <= O <= 1024.  workspace: at least
 * mava_transformer_act_workspace_bytes(B, A, D, n_block, n_blocks) bytes, 16-byte aligned, never read before it is
 * written in the same launch.  Outputs are bit-identical for any n_blocks.  Returns 1 ("not instantiated", nothing
 * launched) when n_block > 4. */
int mava_transformer_act_f32(const float* params, const float* agents_view, const uint8_t* mask, int B, int A, int O,
                             int n_actions, int D, int n_head, int n_block, uint64_t seed, uint32_t step, uint32_t row_offset,
                             int greedy, int32_t* action, float* log_prob, float* value, void* workspace,
                             size_t workspace_bytes, int n_blocks, mava_stream_t s);

/* ---- ff_mat, continuous action head (csrc/mat.hip, csrc/mat_act.hip): the decoder reads the previous agents' action
 *      vectors instead of one-hots and emits the means of Independent(TanhTransformed(Normal(mean, softplus(log_std) +
 *      min_scale))) with one log_std vector (csrc/tanh_normal.h); 1 <= action_dim <= 16, A <= 32, no action mask. */
/* The decoder's input, T32 (rows x n_pad), n_pad = ceil32(action_dim): row (b, 0) = 0, row (b, i) = action[sample, i - 1]
 * for 1 <= i <= known, zero rows after that, zero features past action_dim.  action: (samples, A, action_dim) f32;
 * sample = idx[b], or b when idx is NULL. */
int mava_transformer_shift_action_f32(const float* action, const int32_t* idx, int B, int A, int action_dim, int known,
                                      long rows, int n_pad, float* out, mava_stream_t s);
/* One step of the autoregressive decode: agent `agent` of each of the B samples draws a = tanh(mean + scale * eps) from its
 * T32 means row (rows x action_dim), eps from the Philox counter (row_offset + b * A + agent, step, dim / 2, "TNSA") as
 * mava_seq_sample_continuous_f32 has it, eps = 0 when greedy; writes action[b, agent, :] and log_prob[b, agent] (the
 * log-prob of the action written, summed over dimensions) and nothing else. */
int mava_transformer_sample_continuous_f32(int B, int A, int agent, int action_dim, float min_scale, const float* mean,
                                           const float* log_std, uint64_t seed, uint32_t step, uint32_t row_offset, int greedy,
                                           float* action, float* log_prob, mava_stream_t s);
/* mava_mat_loss_f32 with the actor part of mava_seq_actor_loss_continuous_f32: row b * A + j reads the (samples, A[,
 * action_dim]) trajectory arrays at agent row er = idx[b] * A + j; the entropy sample of that row uses the Philox counter
 * (row_offset + er, ent_step, dim / 2, "TNEN").  Writes dmean (T32, times grad_scale), dvalues (rows, times grad_scale,
 * includes vf_coef), zero on padding rows, loss_partials (n_blocks, 3) = [actor_loss, entropy, value_loss] partial means and
 * dlog_std_partials (n_blocks, action_dim): the log_std gradient's per-block sums, already times sigmoid(log_std) and
 * without grad_scale. */
int mava_transformer_loss_continuous_f32(int Bm, int A, int action_dim, float min_scale, long rows, const int32_t* idx,
                                         const float* mean, const float* log_std, const float* values, const float* action,
                                         const float* old_log_prob, const float* advantages, const float* old_value,
                                         const float* targets, const double* adv_stats, int n_stats, float clip_eps,
                                         float ent_coef, float vf_coef, uint64_t seed, uint32_t ent_step, uint32_t row_offset,
                                         float grad_scale, float* dmean, float* dvalues, float* loss_partials,
                                         float* dlog_std_partials, int n_blocks, mava_stream_t s);
/* length of the continuous network's flat vector: mava_transformer_param_count at n_actions = action_dim (act_dense has a
 * bias row where the discrete network has the start token's) plus the action_dim entries of decoder/log_std at the end */
long mava_transformer_param_count_continuous(int O, int action_dim, int D, int n_block);
/* mava_transformer_act_f32 for the continuous head: action (B, A, action_dim) f32; the same Philox counters as
 * mava_transformer_sample_continuous_f32; the workspace is mava_transformer_act_workspace_bytes'. */
int mava_transformer_act_continuous_f32(const float* params, const float* agents_view, int B, int A, int O, int action_dim,
                                        int D, int n_head, int n_block, float min_scale, uint64_t seed, uint32_t step,
                                        uint32_t row_offset, int greedy, float* action, float* log_prob, float* value,
                                        void* workspace, size_t workspace_bytes, int n_blocks, mava_stream_t s);

/* ---- exchange step: replaces the jax.lax.pmean calls of mava/systems/ppo/ff_mappo.py:224-238
 *      (actor and critic (grads, loss_info) over the "batch" and "device" axes) for a host without torch.distributed.
 *      One process per GPU: rank 0 obtains a 128-byte id (mava_comm_unique_id) and hands it to the other ranks by any
 *      host channel; every rank then creates its communicator on ITS current HIP device.  mava_allreduce_sum_f32 sums
 *      the flat [actor grads | critic grads | loss scalars] buffer over the ranks in place, asynchronously on stream s
 *      (RCCL over xGMI); the 1 / (update_batch_size * world) of the two pmeans is mava_clip_adam_f32's grad_scale.
 *      mava_broadcast_f32 replicates rank `root`'s parameters (flax.jax_utils.replicate, ff_mappo.py:426).
 *      librccl.so is dlopen-ed at the first call (MAVA_RCCL_LIB overrides the name), so a host that already carries an
 *      RCCL shares it.  RCCL errors come back as -2000 - ncclResult_t. */
int mava_comm_unique_id(uint8_t* id128);
int mava_comm_create(void** h, int rank, int world, const uint8_t* id128);
int mava_allreduce_sum_f32(void* h, float* buf, size_t n, mava_stream_t s);
int mava_broadcast_f32(void* h, float* buf, size_t n, int root, mava_stream_t s);
int mava_comm_destroy(void* h);

#ifdef __cplusplus
}
#endif
#endif /* MAVA_HIP_H */
