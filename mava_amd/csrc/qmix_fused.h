// Arguments of the fused rec_qmix mixer update (qmix_fused.hip); the envelope is checked by its C entry point in api.cpp.
#pragma once
#include <stdint.h>

#include "common.h"

struct QmixFusedArgs {
  int L, B, A, O, Rp, nA, Em, Hh;
  const float *obs, *next_obs;
  const int32_t* action;
  const float* reward;
  const uint8_t *term_next, *next_mask;
  const float *q, *qn, *qt;
  const float *mixer, *mixer_target;
  float gamma, grad_scale;
  float *dq, *slab;
  long slab_stride;
  int n_slab;
};

constexpr int QMIX_FUSED_MAX_A = 16, QMIX_FUSED_MAX_ACTIONS = 32, QMIX_FUSED_MAX_EM = 64, QMIX_FUSED_MAX_HH = 128,
              QMIX_FUSED_MAX_AE = 512, QMIX_FUSED_MAX_SLABS = 1024;

// parameters of the mixer's flat layout [w1 net | b1 dense | w2 net | b2 net]
static inline long qmix_mixer_params(long Ds, long A, long Em, long Hh) {
  return (Ds * Hh + Hh + Hh * A * Em + A * Em) + (Ds * Em + Em) + (Ds * Hh + Hh + Hh * Em + Em) + (Ds * Em + Em + Em + 1);
}

int mava_qmix_fused_launch(const QmixFusedArgs& a, hipStream_t s);
