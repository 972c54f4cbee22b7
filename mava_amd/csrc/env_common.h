// What the environment step kernels share: the RecordEpisodeMetrics / auto-reset bookkeeping of one environment
// (mava/wrappers/episode_metrics.py:88-111), done by the one thread that owns the environment in the rule phase, and
// the Philox word selector.  An environment keeps its own `terminated` store, its LDS writes and its reset.
#pragma once
#include "common.h"

__device__ __forceinline__ uint32_t word_of(const Philox4& p, int i) {
  return i == 0 ? p.x : (i == 1 ? p.y : (i == 2 ? p.z : p.w));
}

struct EpisodeBook {
  int32_t* step_count;     // (E, A)
  float* run_return;       // (E) return of the running episode
  int32_t* run_length;
  float* ep_return;        // (E) return of the last finished episode
  int32_t* ep_length;
  float* info_return;      // (E) or null (reset): what the step reports
  int32_t* info_length;
  uint8_t* info_terminal;
};

// every step kernel's argument struct names the eight pointers alike
template <class Args>
__device__ __forceinline__ EpisodeBook episode_book(const Args& a) {
  return {a.step_count, a.run_return, a.run_length, a.ep_return, a.ep_length, a.info_return, a.info_length, a.info_terminal};
}

struct EpisodeRun { float run_ret, ep_ret; int run_len, ep_len; };
struct EpisodeEnd { bool term; int step_count; };  // the step ended its episode; the step count after it (0 where it did)

// The two halves of a step's bookkeeping.  A kernel with a long rule phase loads at its top and commits at its end, so
// that the loads are not waited for; the others call episode_step.
__device__ __forceinline__ EpisodeRun episode_load(const EpisodeBook& b, int e) {
  return {b.run_return[e], b.ep_return[e], b.run_length[e], b.ep_length[e]};
}

// `sc_old`: the step count before the step; `mean_rew`: the agents' mean reward; `terminated`: the rules ended the episode
// (the time limit is applied here)
__device__ __forceinline__ EpisodeEnd episode_commit(const EpisodeBook& b, int e, const EpisodeRun& r, int sc_old, float mean_rew,
                                                     bool terminated, int time_limit) {
  // (scalar copies: a conditional on struct members is compiled as a branch, and the ep_* loads then sink into it and
  // wait for the run_* loads instead of flying with them)
  const float run_ret = r.run_ret, ep_ret = r.ep_ret;
  const int run_len = r.run_len, ep_len = r.ep_len;
  const int sc_new = sc_old + 1;
  const bool term = terminated || sc_new >= time_limit;
  const float new_ret = run_ret + mean_rew;
  const int new_len = run_len + 1;
  const float ret_info = term ? new_ret : ep_ret;
  const int len_info = term ? new_len : ep_len;
  b.info_return[e] = ret_info;
  b.info_length[e] = len_info;
  b.info_terminal[e] = term ? 1 : 0;
  b.run_return[e] = term ? 0.0f : new_ret;
  b.run_length[e] = term ? 0 : new_len;
  b.ep_return[e] = ret_info;
  b.ep_length[e] = len_info;
  return {term, term ? 0 : sc_new};
}

__device__ __forceinline__ EpisodeEnd episode_step(const EpisodeBook& b, int e, int sc_old, float mean_rew, bool terminated,
                                                   int time_limit) {
  return episode_commit(b, e, episode_load(b, e), sc_old, mean_rew, terminated, time_limit);
}

// a reset call: no episode is running, none has finished
__device__ __forceinline__ void episode_clear(const EpisodeBook& b, int e) {
  b.run_return[e] = 0.0f;
  b.run_length[e] = 0;
  b.ep_return[e] = 0.0f;
  b.ep_length[e] = 0;
}
