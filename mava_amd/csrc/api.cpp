// libmavahip.so: error channel and version of the C ABI declared in include/mava_hip.h.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "ctx.h"

static thread_local char g_err[512] = "";

void mava_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* mava_last_error(void) { return g_err; }

extern "C" int mava_abi_version(void) { return 4; }  // 4: one entry point per operation (optional outputs are trailing arguments that may be null)

// ---- context handle (ctx.h) -------------------------------------------------------------------------------------------
enum { CTX_MATMUL_MODE = 0, CTX_CRITIC_AGGREGATION = 1, CTX_GAE_VARIANT = 2, CTX_POLICY_VARIANT = 3, CTX_H2_LAUNCHES = 4, CTX_TRAIN_VARIANT = 5, CTX_W8_LAUNCHES = 6, CTX_W1_SPLIT_FRESH = 7, CTX_EXACT_TILES = 8, CTX_X16_LAUNCHES = 9, CTX_X16_W8_LAUNCHES = 10, CTX_W8_DEFER_LAUNCHES = 11, CTX_W8_AHEAD_LAUNCHES = 12 };
// word of the handle's device counters (ctx.h exact_tiles) behind a key
static int ctx_counter_word(int key) {
  return key == CTX_W8_AHEAD_LAUNCHES ? 4 : key == CTX_W8_DEFER_LAUNCHES ? 3 : key == CTX_X16_W8_LAUNCHES ? 2 : key == CTX_X16_LAUNCHES ? 1 : 0;
}

extern "C" int mava_ctx_create(mava_ctx** out) {
  MAVA_ARG_CHECK(out != nullptr, 0, "mava_ctx_create: null output pointer");
  mava_ctx* c = new mava_ctx();
  c->matmul_mode = 0;
  c->critic_aggregation = 1;
  c->gae_variant = 0;
  c->policy_variant = 0;
  c->h2_launches = 0;
  c->train_variant = 0;
  c->w8_launches = 0;
  c->w1_split[0] = c->w1_split[1] = nullptr;
  for (int i = 0; i < 2; ++i) {
    c->w1_fresh[i] = 0;
    c->w1_key_params[i] = nullptr;
    c->w1_key_din[i] = c->w1_key_steps[i] = 0;
  }
  c->exact_tiles = nullptr;
  *out = c;
  return MAVA_OK;
}

extern "C" int mava_ctx_destroy(mava_ctx* c) {
  if (c == nullptr) return MAVA_OK;
  for (int i = 0; i < 2; ++i)
    if (c->w1_split[i] != nullptr) (void)hipFree(c->w1_split[i]);  // (synchronises with the launches that read it)
  if (c->exact_tiles != nullptr) (void)hipFree(c->exact_tiles);
  delete c;
  return MAVA_OK;
}

extern "C" int mava_ctx_set(mava_ctx* c, int key, long value) {
  MAVA_ARG_CHECK(c != nullptr, 0, "mava_ctx_set: null context");
  switch (key) {
    case CTX_MATMUL_MODE:
      MAVA_ARG_CHECK(value == 0 || value == 1, 1, "mava_ctx_set: matmul mode %ld (0 = exact f32, 1 = f16x2)", value);
      c->matmul_mode = (int)value;
      c->w1_fresh[0] = c->w1_fresh[1] = 0;  // (launches of the other arithmetic do not read the copy: it may go stale meanwhile)
      return MAVA_OK;
    case CTX_CRITIC_AGGREGATION: c->critic_aggregation = value ? 1 : 0; return MAVA_OK;
    case CTX_GAE_VARIANT: c->gae_variant = (int)value; return MAVA_OK;
    case CTX_POLICY_VARIANT: c->policy_variant = (int)value; return MAVA_OK;
    case CTX_H2_LAUNCHES: c->h2_launches = value; return MAVA_OK;
    case CTX_TRAIN_VARIANT: c->train_variant = (int)value; return MAVA_OK;
    case CTX_W8_LAUNCHES: c->w8_launches = value; return MAVA_OK;
    case CTX_W1_SPLIT_FRESH:
      MAVA_ARG_CHECK(value == 0, 1, "mava_ctx_set: MAVA_CTX_W1_SPLIT_FRESH can only be cleared (0) by the caller");
      c->w1_fresh[0] = c->w1_fresh[1] = 0;
      return MAVA_OK;
    case CTX_EXACT_TILES:
      MAVA_ARG_CHECK(value == 0, 1, "mava_ctx_set: MAVA_CTX_EXACT_TILES can only be reset (0) by the caller");
      if (c->exact_tiles != nullptr) {  // (the launches that add to the word first)
        MAVA_HIP_CHECK(hipDeviceSynchronize());
        MAVA_HIP_CHECK(hipMemset(c->exact_tiles, 0, sizeof(unsigned long long)));
      }
      return MAVA_OK;
    case CTX_X16_LAUNCHES:
    case CTX_X16_W8_LAUNCHES:
    case CTX_W8_DEFER_LAUNCHES:
    case CTX_W8_AHEAD_LAUNCHES:
      MAVA_ARG_CHECK(value == 0, 1, "mava_ctx_set: MAVA_CTX_X16_LAUNCHES / _W8_LAUNCHES / MAVA_CTX_W8_DEFER_LAUNCHES / _AHEAD_LAUNCHES can only be reset (0) by the caller");
      if (c->exact_tiles != nullptr) {  // (the second .. fifth word of the same allocation)
        MAVA_HIP_CHECK(hipDeviceSynchronize());
        MAVA_HIP_CHECK(hipMemset(c->exact_tiles + ctx_counter_word(key), 0, sizeof(unsigned long long)));
      }
      return MAVA_OK;
    default: mava_set_error("mava_ctx_set: unknown key %d", key); return MAVA_EARG(2);
  }
}

extern "C" int mava_ctx_get(const mava_ctx* c, int key, long* value) {
  MAVA_ARG_CHECK(c != nullptr && value != nullptr, 0, "mava_ctx_get: null argument");
  switch (key) {
    case CTX_MATMUL_MODE: *value = c->matmul_mode; return MAVA_OK;
    case CTX_CRITIC_AGGREGATION: *value = c->critic_aggregation; return MAVA_OK;
    case CTX_GAE_VARIANT: *value = c->gae_variant; return MAVA_OK;
    case CTX_POLICY_VARIANT: *value = c->policy_variant; return MAVA_OK;
    case CTX_H2_LAUNCHES: *value = c->h2_launches; return MAVA_OK;
    case CTX_TRAIN_VARIANT: *value = c->train_variant; return MAVA_OK;
    case CTX_W8_LAUNCHES: *value = c->w8_launches; return MAVA_OK;
    case CTX_W1_SPLIT_FRESH: *value = c->w1_fresh[1]; return MAVA_OK;
    case CTX_EXACT_TILES:
    case CTX_X16_LAUNCHES:
    case CTX_X16_W8_LAUNCHES:
    case CTX_W8_DEFER_LAUNCHES:
    case CTX_W8_AHEAD_LAUNCHES: {  // a device word: waits for the launches that add to it
      unsigned long long n = 0;
      if (c->exact_tiles != nullptr) {
        MAVA_HIP_CHECK(hipDeviceSynchronize());
        MAVA_HIP_CHECK(hipMemcpy(&n, c->exact_tiles + ctx_counter_word(key), sizeof(n), hipMemcpyDeviceToHost));
      }
      *value = (long)n;
      return MAVA_OK;
    }
    default: mava_set_error("mava_ctx_get: unknown key %d", key); return MAVA_EARG(2);
  }
}

// ---- rec_qmix: the fused mixer update (qmix_fused.hip).  The envelope is checked here: nothing is launched on refusal.
#include "qmix_fused.h"

extern "C" int mava_qmix_mixer_update_f32(const mava_ctx* ctx, int L, int B, int A, int O, int Rp, int n_actions, int Em, int Hh,
                                          const float* obs, const float* next_obs, const int32_t* action, const float* reward,
                                          const uint8_t* terminal_next, const uint8_t* next_mask, const float* q,
                                          const float* q_next_online, const float* q_next_target, const float* mixer,
                                          const float* mixer_target, float gamma, float grad_scale, float* dq, float* slab,
                                          long slab_stride, int n_slab, hipStream_t s) {
  MAVA_ARG_CHECK(ctx != nullptr && ctx->matmul_mode == 1, 0, "mava_qmix_mixer_update_f32: f16x2 products only (a context in f16x2 mode)");
  MAVA_ARG_CHECK(L >= 1 && B >= 1 && O >= 1 && A >= 1 && A <= QMIX_FUSED_MAX_A && n_actions >= 1 && n_actions <= QMIX_FUSED_MAX_ACTIONS, 1,
                 "mava_qmix_mixer_update_f32: bad shape L=%d B=%d A=%d O=%d n_actions=%d (1..16 agents, 1..32 actions)", L, B, A, O,
                 n_actions);
  MAVA_ARG_CHECK(Em >= 1 && Em <= QMIX_FUSED_MAX_EM, 2, "mava_qmix_mixer_update_f32: Em=%d outside [1, 64]", Em);
  MAVA_ARG_CHECK(Hh >= 1 && Hh <= QMIX_FUSED_MAX_HH, 3, "mava_qmix_mixer_update_f32: Hh=%d outside [1, 128]", Hh);
  MAVA_ARG_CHECK(A * Em <= QMIX_FUSED_MAX_AE, 4, "mava_qmix_mixer_update_f32: A*Em=%d above 512", A * Em);
  MAVA_ARG_CHECK(Rp >= 32 && Rp % 32 == 0 && (long)B * A <= Rp, 5,
                 "mava_qmix_mixer_update_f32: Rp=%d must be a multiple of 32 holding B*A=%ld rows", Rp, (long)B * A);
  MAVA_ARG_CHECK((long)A * O <= (1L << 20) && (long)L * Rp * (O > n_actions ? O : n_actions) < (1L << 40), 6,
                 "mava_qmix_mixer_update_f32: state or batch too large");
  const long Pm = qmix_mixer_params((long)A * O, A, Em, Hh);
  MAVA_ARG_CHECK(n_slab >= 1 && n_slab <= QMIX_FUSED_MAX_SLABS && slab_stride >= Pm + 3, 7,
                 "mava_qmix_mixer_update_f32: n_slab=%d outside [1, 1024] or slab_stride=%ld below the mixer's %ld parameters + 3 metrics",
                 n_slab, slab_stride, Pm);
  MAVA_ARG_CHECK(obs && next_obs && action && reward && terminal_next && next_mask && q && q_next_online && q_next_target && mixer &&
                     mixer_target && dq && slab, 8, "mava_qmix_mixer_update_f32: null pointer");
  MAVA_ARG_CHECK(dq != q && dq != q_next_online && dq != q_next_target, 9, "mava_qmix_mixer_update_f32: dq must not alias a Q input");
  MAVA_ARG_CHECK(gamma >= 0.0f && grad_scale > 0.0f, 10, "mava_qmix_mixer_update_f32: gamma=%g or grad_scale=%g out of range", (double)gamma,
                 (double)grad_scale);
  const QmixFusedArgs a = {L, B, A, O, Rp, n_actions, Em, Hh, obs, next_obs, action, reward, terminal_next, next_mask, q, q_next_online,
                           q_next_target, mixer, mixer_target, gamma, grad_scale, dq, slab, slab_stride, n_slab};
  return mava_qmix_fused_launch(a, s);
}
