// The masked Categorical of one agent row as ff_mat's kernels see it (mat.hip, mat_act.hip): the masked logits, the row's
// log-sum-exp and the Gumbel-max / greedy choice on the Philox stream of mava_seq_sample_f32.  Device code only.
#pragma once
#include <cfloat>

#include "common.h"

// masked logits as every Categorical of this library sees them (mlp_core.h): illegal -> -FLT_MAX; a row without a legal
// action is uniform over its n real slots.  No per-action arrays: up to 64 actions are walked from memory again.
// STRIDE: distance between two logits of the row (32 in a T32 matrix, 1 in a row-major one).
template <int STRIDE>
struct RowLogitsT {
  const float* y;       // the row's logits: feature o at y[o * STRIDE]
  const uint8_t* mask;  // the row's n flags or null
  int n;
  __device__ __forceinline__ bool legal(int o) const { return mask == nullptr || mask[o] != 0; }
  __device__ __forceinline__ float z(int o) const { return legal(o) ? y[(long)o * STRIDE] : -FLT_MAX; }
};

using RowLogits = RowLogitsT<32>;  // T32 logits, already offset to (tile, lane)

struct RowStats {
  float lse;
  bool none;
};

template <int STRIDE>
__device__ __forceinline__ RowStats row_stats(const RowLogitsT<STRIDE>& rl) {
  float mx = -FLT_MAX;
  for (int o = 0; o < rl.n; ++o) mx = fmaxf(mx, rl.z(o));
  float se = 0.0f;
  for (int o = 0; o < rl.n; ++o) se += expf(rl.z(o) - mx);
  RowStats st;
  st.none = (mx == -FLT_MAX);
  st.lse = st.none ? logf((float)rl.n) : mx + logf(se);
  return st;
}

// Gumbel-max on the Philox stream of mava_seq_sample_f32 (counter (gid, step, action / 4, "POLI"), word action % 4), or
// the argmax when greedy (first index on ties)
template <int STRIDE>
__device__ __forceinline__ int row_draw(const RowLogitsT<STRIDE>& rl, int greedy, uint32_t gid, uint32_t step, uint32_t seed_lo,
                                        uint32_t seed_hi) {
  int a = 0;
  float best = -FLT_MAX;
  if (greedy) {
    for (int o = 0; o < rl.n; ++o) {
      const float z = rl.z(o);
      if (z > best) { best = z; a = o; }
    }
  } else {
    for (int c = 0; c < (rl.n + 3) / 4; ++c) {
      const Philox4 rnd = philox4x32_10(gid, step, (uint32_t)c, 0x504f4c49u, seed_lo, seed_hi);
      for (int k = 0; k < 4; ++k) {
        const int o = 4 * c + k;
        if (o < rl.n) {
          const uint32_t w = k == 0 ? rnd.x : (k == 1 ? rnd.y : (k == 2 ? rnd.z : rnd.w));
          const float sc = rl.z(o) - logf(-logf(u01_open(w)));
          if (sc > best) { best = sc; a = o; }
        }
      }
    }
  }
  return a;
}

// log-prob of action a of the row
template <int STRIDE>
__device__ __forceinline__ float row_log_prob(const RowLogitsT<STRIDE>& rl, const RowStats& st, int a) {
  return (st.none ? 0.0f : rl.z(a)) - st.lse;
}
