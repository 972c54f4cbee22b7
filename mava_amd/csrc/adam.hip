// Fused per-network global-norm clip + Adam, in place, one launch (K11 / SURVEY §8 row A10),
// and the deterministic slab reducer that produces the flat gradient it consumes.
//
// Reference wiring: mava/systems/ppo/ff_mappo.py:359-366 builds, per network,
//   optax.chain(optax.clip_by_global_norm(max_grad_norm), optax.adam(lr, eps=1e-5))
// and ff_mappo.py:241-250 applies it; the learning rate is constant or the linear schedule of
// mava/utils/training.py:20-64 evaluated at the optimiser's pre-increment step count.
// optax is not vendored in the reference; its published semantics are restated here
// (parity unpinned, see oracle/ppo_oracle.py):
//   n = sqrt(sum g^2) over the whole network;  g <- g if n < c else (g / n) * c
//   m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; t = count + 1
//   p <- p - lr(count) * (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + eps) ; count <- t
//
// The incoming gradient is the SUM over (update-batch replicas x ranks); grad_scale = 1/(U*D)
// turns it into the pmean of ff_mappo.py:224-238.
//
// MI355X mapping: 77 K parameters = 2.1 MB of traffic, i.e. launch/latency bound.  One launch:
// every block first reduces the whole (L2-resident) gradient of each network - or the slab reducer's
// partial sums of it - in the same fixed order, so all blocks hold a bit-identical norm with no grid
// barrier and no atomics, then updates its own slice of p/m/v; everything a thread reads is requested
// in one round at the top.
#include "h2_core.h"
#include "ctx.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int MAX_SEG = 8;

struct AdamSegs {
  int off[MAX_SEG + 1];
  float lr[MAX_SEG];
};

__device__ inline double block_sum(double x, double* sh) {
  // wave reduce (64 lanes) then across the 4 waves, fixed order
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = x;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < ADAM_THREADS / 64; ++i) t += sh[i];
  return t;
}

// block_sum of two values at once: the same additions per value, one pair of barriers for both
__device__ inline void block_sum2(double& x, double& y, double (*sh2)[ADAM_THREADS / 64]) {
  for (int o = 32; o > 0; o >>= 1) {
    x += __shfl_down(x, o, 64);
    y += __shfl_down(y, o, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { sh2[0][w] = x; sh2[1][w] = y; }
  __syncthreads();
  double t = 0.0, u = 0.0;
  for (int i = 0; i < ADAM_THREADS / 64; ++i) { t += sh2[0][i]; u += sh2[1][i]; }
  x = t;
  y = u;
}

// Fused tail (mava_ppo_finish_f32): `norm_partials` != null - the squared norms come from the per-block partial sums the slab
// reducer left behind (n_partial x 2 doubles: segment 0, segment 1) instead of a pass over g; `ticket` != null - the block
// that finishes LAST (arrival ticket, no grid barrier: a barrier costs more than the kernel boundary it would replace,
// MI355X_MICROARCH.md price list) increments the step counts.  For PACK > 0 (the wide critic's 16-input steps) the launch
// also re-splits that network's W1 into `w1_split` for the next gradient launch: the W1 range of the parameters belongs to
// PACK_BLOCKS extra blocks (below), which split what they have just computed - no block waits for another.
struct AdamTail {
  const double* norm_partials;
  int n_partial;
  unsigned int* ticket;
  int pack_offset;  // start of the network whose W1 is re-split, as an offset into p
  int pack_din;
  uint4* w1_split;
};

// One parameter's clip + Adam step, the ONE place it is written: the flat lanes and the pack blocks must give the same bits
// (a weight belongs to either depending on the launch), and with contraction on the same expression can fuse differently
// in two contexts.  The roundings are those of the kernel as it always compiled: every product and sum of m and v rounded
// on its own, one fused multiply-add for the parameter.  (The library is built with -ffp-contract=fast, which fuses whatever
// it meets and honours no pragma: a product that must be rounded passes through an empty asm statement.  Without them the
// pack blocks and the flat lanes did differ in p, tests/test_gpu_tail.py.)  `nrm` < 0: no clipping.
__device__ __forceinline__ float rounded(float x) {
  asm("" : "+v"(x));
  return x;
}
__device__ __forceinline__ void adam_element(float g_sum, float& pi, float& mi, float& vi, float grad_scale, float nrm,
                                             float max_norm, float b1, float b2, float bc1, float bc2, float lr, float eps) {
  float gi = g_sum * grad_scale;
  if (nrm >= 0.0f) gi = (gi / nrm) * max_norm;
  const float g1 = rounded((1.0f - b1) * gi);
  const float g2 = rounded(((1.0f - b2) * gi) * gi);
  mi = rounded(b1 * mi) + g1;
  vi = rounded(b2 * vi) + g2;
  const float mhat = mi / bc1;
  const float vhat = vi / bc2;
  const float q = mhat / (sqrtf(vhat) + eps);
  pi = __builtin_fmaf(-lr, q, pi);
}

// A thread's batch of N parameters: loaded in one go (addresses of dead entries clamped to a live one), updated, stored.
template <int N>
struct AdamBatch {
  int idx[N];
  bool live[N];
  float g[N], p[N], m[N], v[N];
  __device__ __forceinline__ void load(const float* __restrict__ gp, const float* pp, const float* mp, const float* vp) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
      g[u] = gp[idx[u]];
      m[u] = mp[idx[u]];
      v[u] = vp[idx[u]];
      p[u] = pp[idx[u]];
    }
  }
};

// The W1 re-split inside the Adam launch.  pack_w1_body's 256 lanes (wave w, r, h) each run a carry chain over their
// own 8 * PACK inputs k = 16 s + 8 h + e of feature f = 32 w + r; the chain is serial, the Adam step of those inputs is
// not (~70 instructions each with four divisions and a root: 144 of them on the chain's own lane would cost more than
// the whole launch did).  So a pack block owns PACK_CHAINS chains (same w and h, consecutive f): its 256 threads update
// the chains' PACK_CHAINS x 8 PACK weights (one round of loads), leave the new values in LDS, and its first PACK_CHAINS
// lanes split them from there.
constexpr int PACK_CHAINS = 8;
constexpr int PACK_BLOCKS = 256 / PACK_CHAINS;

template <int PACK>
__global__ __launch_bounds__(ADAM_THREADS) void clip_adam_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, int32_t* __restrict__ count, AdamSegs segs, int n_seg,
    float grad_scale, float max_norm, int decay, int steps_per_update, int num_updates, float b1,
    float b2, float eps, const float* __restrict__ loss_sums, float vf_coef, float ent_coef,
    float* __restrict__ metrics_out, AdamTail tail) {
  constexpr int FLAT_N = 4;                           // parameters per flat thread and batch
  // a chain's 8 PACK inputs dealt to the block's 256 / PACK_CHAINS threads per chain
  constexpr int PACK_N = PACK > 0 ? (8 * PACK * PACK_CHAINS + ADAM_THREADS - 1) / ADAM_THREADS : 1;
  __shared__ double sh[ADAM_THREADS / 64];
  __shared__ double sh2[2][ADAM_THREADS / 64];
  __shared__ float s_clip[MAX_SEG];
  __shared__ float s_bc1[MAX_SEG], s_bc2[MAX_SEG];  // 1 - b^t, evaluated in f64 (no f32 cancellation)
  __shared__ float s_lr[MAX_SEG];
  __shared__ float s_w[PACK > 0 ? 8 * PACK : 1][PACK_CHAINS];  // a pack block's new weights, [input j][chain]

  // The W1 range [w1_lo, w1_lo + w1_n) belongs to the last PACK_BLOCKS blocks of the grid, everything else to the flat lanes
  const int total = segs.off[n_seg];
  const int w1_lo = PACK > 0 ? tail.pack_offset : 0;
  const int w1_n = PACK > 0 ? (tail.pack_din + 1) * MLP_H : 0;
  const int n_flat = total - w1_n;
  const int flat_blocks = (int)gridDim.x - (PACK > 0 ? PACK_BLOCKS : 0);
  const bool pack_block = PACK > 0 && (int)blockIdx.x >= flat_blocks;
  const int flat_stride = flat_blocks * ADAM_THREADS;
  auto flat_index = [&](int i) { return (PACK > 0 && i >= w1_lo) ? i + w1_n : i; };

  // ---- one round of loads: everything below that depends on nothing but the launch arguments is requested here, before the
  // first of it is used - this thread's parameters with their gradient and moments, the counts, and (fused tail) its share
  // of the norm partials.  The launch is a chain of round trips to memory other XCDs wrote; this makes it one.
  AdamBatch<FLAT_N> fb;
  AdamBatch<PACK_N> pb;
  const int chain = (PACK > 0 && pack_block) ? ((int)blockIdx.x - flat_blocks) * PACK_CHAINS + (threadIdx.x & (PACK_CHAINS - 1)) : 0;
  int flat_base = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (pack_block) {
    const int f = 32 * (chain >> 6) + (chain & 31), h = (chain & 63) >> 5;
#pragma unroll
    for (int u = 0; u < PACK_N; ++u) {
      const int j = (threadIdx.x / PACK_CHAINS) + (ADAM_THREADS / PACK_CHAINS) * u;  // input j of the chain, see pack_w1_chain
      const int k = 16 * (j >> 3) + 8 * h + (j & 7);
      pb.live[u] = j < 8 * PACK && k <= tail.pack_din;
      pb.idx[u] = w1_lo + min(k, tail.pack_din) * MLP_H + f;
    }
    pb.load(g, p, m, v);
  } else {
#pragma unroll
    for (int u = 0; u < FLAT_N; ++u) {
      const int i = flat_base + u * flat_stride;
      fb.live[u] = i < n_flat;
      fb.idx[u] = flat_index(min(i, n_flat - 1));
    }
    fb.load(g, p, m, v);
  }
  // the step counts: lanes 0 .. 2 n_seg - 1 of the block each raise one b to one t (f64 pow, ~1 us each; thread 0 used to
  // evaluate all of them in turn), lanes < n_seg also form the learning rate
  // (the counts through uniform addresses: scalar loads, which do not queue behind the vector loads around them)
  const bool coef_lane = (int)threadIdx.x < 2 * n_seg;
  int coef_cnt = 0;
#pragma unroll
  for (int k = 0; k < MAX_SEG; ++k) {
    const int c = k < n_seg ? count[k] : 0;
    if ((int)(threadIdx.x >> 1) == k) coef_cnt = c;
  }
  constexpr int NP = 8;  // norm partial pairs in flight per thread
  typedef double dbl2 __attribute__((ext_vector_type(2), aligned(8)));
  dbl2 q[NP];
  if (tail.norm_partials != nullptr) {
    const dbl2* np2 = reinterpret_cast<const dbl2*>(tail.norm_partials);
#pragma unroll
    for (int u = 0; u < NP; ++u) q[u] = np2[min((int)threadIdx.x + u * ADAM_THREADS, tail.n_partial - 1)];
  }
  if (coef_lane) {
    const int sgi = threadIdx.x >> 1;
    const double t = (double)(coef_cnt + 1);
    if (threadIdx.x & 1) s_bc2[sgi] = (float)(1.0 - pow((double)b2, t));
    else s_bc1[sgi] = (float)(1.0 - pow((double)b1, t));
    if ((threadIdx.x & 1) == 0) {
      float lr = segs.lr[sgi];
      if (decay) {
        // mava/utils/training.py:36-42: frac = 1 - (count // (epochs*minibatches)) / num_updates
        const float frac = 1.0f - (float)(coef_cnt / steps_per_update) / (float)num_updates;
        lr = lr * frac;
      }
      s_lr[sgi] = lr;
    }
  }

  // ---- phase 1: every block computes every segment's norm identically
  if (tail.norm_partials != nullptr) {
    // (two segments: mava_ppo_finish_f32.)  Fixed order: thread t adds partials t, t + 256, ...; then the block sum -
    // bit-identical in every block
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int u = 0; u < NP; ++u)
      if ((int)threadIdx.x + u * ADAM_THREADS < tail.n_partial) { a0 += q[u].x; a1 += q[u].y; }
    for (int b = threadIdx.x + NP * ADAM_THREADS; b < tail.n_partial; b += ADAM_THREADS) {
      a0 += tail.norm_partials[2 * b];
      a1 += tail.norm_partials[2 * b + 1];
    }
    block_sum2(a0, a1, sh2);
    if (threadIdx.x < 2) {
      const float nrm = (float)sqrt(threadIdx.x == 0 ? a0 : a1);
      s_clip[threadIdx.x] = (nrm < max_norm) ? -1.0f : nrm;
    }
  }
  for (int sgi = 0; tail.norm_partials == nullptr && sgi < n_seg; ++sgi) {
    const int lo = segs.off[sgi], hi = segs.off[sgi + 1];
    // 16-byte loads, 8 of them in flight per thread: this phase is a chain of L2 round trips (every block reads the
    // whole gradient), ~10 of them at 77 K parameters instead of the ~40 of one float per load
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int al = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? min(hi, (lo + 3) & ~3) : hi;  // first aligned index
    if (lo + (int)threadIdx.x < al) {
      const float gi = g[lo + threadIdx.x] * grad_scale;  // (al - lo <= 3 unless g itself is unaligned)
      a0 += (double)gi * (double)gi;
    }
    for (int i = lo + ADAM_THREADS + threadIdx.x; i < al; i += ADAM_THREADS) {
      const float gi = g[i] * grad_scale;
      a0 += (double)gi * (double)gi;
    }
    const int n4 = (hi - al) >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g + al);
    int i = threadIdx.x;
    for (; i + 7 * ADAM_THREADS < n4; i += 8 * ADAM_THREADS) {
      float4 q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = g4[i + u * ADAM_THREADS];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float x = q[u].x * grad_scale, y = q[u].y * grad_scale, z = q[u].z * grad_scale, w = q[u].w * grad_scale;
        a0 += (double)x * x;
        a1 += (double)y * y;
        a2 += (double)z * z;
        a3 += (double)w * w;
      }
    }
    for (; i < n4; i += ADAM_THREADS) {
      const float4 q = g4[i];
      const float x = q.x * grad_scale, y = q.y * grad_scale, z = q.z * grad_scale, w = q.w * grad_scale;
      a0 += (double)x * x;
      a1 += (double)y * y;
      a2 += (double)z * z;
      a3 += (double)w * w;
    }
    if (al + 4 * n4 + (int)threadIdx.x < hi) {
      const float gi = g[al + 4 * n4 + threadIdx.x] * grad_scale;
      a0 += (double)gi * (double)gi;
    }
    const double tot = block_sum((a0 + a1) + (a2 + a3), sh);
    if (threadIdx.x == 0) {
      const float nrm = (float)sqrt(tot);
      // optax.clip_by_global_norm: trigger = n < c ; else (g / n) * c
      s_clip[sgi] = (nrm < max_norm) ? -1.0f : nrm;
    }
  }
  __syncthreads();

  // ---- arrival ticket, taken as soon as this block has read the counts (the coefficient lanes consumed them before the
  // barrier above): whoever arrives last increments them at its end.  No other block waits on the ticket, and only this
  // wave for its round trip (the compiler broadcasts the returned number at once); at the end of the block, behind a fence
  // over all its stores, it cost 1 us more.
  unsigned int ticket_no = 0;
  if (tail.ticket != nullptr && threadIdx.x == 0)
    ticket_no = __hip_atomic_fetch_add(tail.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);

  // ---- phase 2: slice update
  // (dead entries of a batch are computed on the live element their address was clamped to and not stored: without a branch
  // per entry the compiler interleaves the entries' division chains)
  auto update = [&](bool live, int i, float gi, float& pi, float& mi, float& vi) {
    int sgi = 0;
#pragma unroll
    for (int k = 1; k < MAX_SEG; ++k)
      if (k < n_seg && i >= segs.off[k]) sgi = k;
    adam_element(gi, pi, mi, vi, grad_scale, s_clip[sgi], max_norm, b1, b2, s_bc1[sgi], s_bc2[sgi], s_lr[sgi], eps);
    if (live) {
      m[i] = mi;
      v[i] = vi;
      p[i] = pi;
    }
  };
  if (pack_block) {
    if constexpr (PACK > 0) {
#pragma unroll
      for (int u = 0; u < PACK_N; ++u) {
        update(pb.live[u], pb.idx[u], pb.g[u], pb.p[u], pb.m[u], pb.v[u]);
        const int j = (threadIdx.x / PACK_CHAINS) + (ADAM_THREADS / PACK_CHAINS) * u;
        if (j < 8 * PACK) s_w[j][threadIdx.x & (PACK_CHAINS - 1)] = pb.live[u] ? pb.p[u] : 0.0f;
      }
      __syncthreads();
      if (threadIdx.x < PACK_CHAINS)
        h2::pack_w1_chain<PACK>([&](int j) { return s_w[j][threadIdx.x]; }, tail.pack_din, tail.w1_split, chain,
                                h2::W_SCALE_CRITIC);
    }
  } else {
    for (;;) {
#pragma unroll
      for (int u = 0; u < FLAT_N; ++u)
        update(fb.live[u], fb.idx[u], fb.g[u], fb.p[u], fb.m[u], fb.v[u]);
      flat_base += FLAT_N * flat_stride;  // (a second batch only when the grid was capped: > 256 K parameters)
      if (flat_base >= n_flat) break;
#pragma unroll
      for (int u = 0; u < FLAT_N; ++u) {
        const int i = flat_base + u * flat_stride;
        fb.live[u] = i < n_flat;
        fb.idx[u] = flat_index(min(i, n_flat - 1));
      }
      fb.load(g, p, m, v);
    }
  }

  // ---- metrics (ff_mappo.py:255-265): loss_sums = [actor_loss, entropy, value_loss] summed
  // over replicas/ranks of per-replica means.
  if (metrics_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    const float actor_loss = loss_sums[0] * grad_scale;
    const float entropy = loss_sums[1] * grad_scale;
    const float value_loss = loss_sums[2] * grad_scale;
    metrics_out[0] = __builtin_fmaf(vf_coef, value_loss, __builtin_fmaf(-ent_coef, entropy, actor_loss));  // total_loss
    metrics_out[1] = value_loss;
    metrics_out[2] = actor_loss;
    metrics_out[3] = entropy;
  }

  // ---- last arriver: count increment (every block had read the counts when it took its ticket)
  if (tail.ticket != nullptr && threadIdx.x == 0 && ticket_no == gridDim.x - 1) {
    __hip_atomic_store(tail.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    for (int k = 0; k < n_seg; ++k) count[k] += 1;
  }
}

// Without a ticket the counter increment cannot race with readers because counts are bumped by
// a separate 1-thread kernel on the same stream after the update kernel.
__global__ void bump_counts_kernel(int32_t* count, int n_seg) {
  if (threadIdx.x < n_seg) count[threadIdx.x] += 1;
}

// Column sum over the slabs, shared by both reducers.  A block owns 64 columns; its 4 waves each sum a quarter of
// the slabs (ascending, 8 loads in flight), and the four partial sums are added in a fixed order through LDS - the
// result is a fixed function of the inputs (bitwise reproducible run to run), with 4x the waves and twice the loads
// in flight of one thread per column, which spent its time waiting on 64 dependent groups of loads.
__device__ __forceinline__ float slab_column_sum(const float* __restrict__ slab, int n_slab, long slab_stride,
                                                 int col, bool live, float (&part)[4][64]) {
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int per = (n_slab + 3) >> 2;
  const int b0 = g * per, b1 = min(n_slab, b0 + per);
  float acc = 0.0f;
  if (live) {
    const float* p = slab + (long)b0 * slab_stride + col;
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      float a[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] = p[(long)q * slab_stride];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc += a[q];
      p += 8 * slab_stride;
    }
    for (; b < b1; ++b) { acc += *p; p += slab_stride; }
  }
  part[g][c] = acc;
  __syncthreads();
  return ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// out[i] = sum_b slab[b][i] for i < n (fixed order).  Optionally accumulates onto the existing out (used when
// several update-batch replicas add into one flat gradient).
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab,
                                                          int n_slab, long slab_stride, int n,
                                                          int accumulate,
                                                          float* __restrict__ out) {
  __shared__ float part[4][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const float acc = slab_column_sum(slab, n_slab, slab_stride, i, i < n, part);
  if (threadIdx.x < 64 && i < n) out[i] = accumulate ? (out[i] + acc) : acc;
}

}  // namespace

extern "C" int mava_clip_adam(float* p, const float* g, float* m, float* v, int32_t* count,
                              const int* seg_off, const float* seg_lr, int n_seg,
                              float grad_scale, float max_norm, int decay, int steps_per_update,
                              int num_updates, float b1, float b2, float eps,
                              const float* loss_sums, float vf_coef, float ent_coef,
                              float* metrics_out, hipStream_t s) {
  MAVA_ARG_CHECK(n_seg >= 1 && n_seg <= MAX_SEG, 0, "mava_clip_adam: n_seg=%d out of [1,%d]",
                 n_seg, MAX_SEG);
  MAVA_ARG_CHECK(p && g && m && v && count && seg_off && seg_lr, 1,
                 "mava_clip_adam: null pointer argument");
  MAVA_ARG_CHECK(metrics_out == nullptr || loss_sums != nullptr, 2,
                 "mava_clip_adam: metrics_out needs loss_sums");
  MAVA_ARG_CHECK(!decay || (steps_per_update > 0 && num_updates > 0), 3,
                 "mava_clip_adam: decay needs steps_per_update>0 and num_updates>0");
  AdamSegs segs;
  for (int i = 0; i <= n_seg; ++i) {
    segs.off[i] = seg_off[i];
    MAVA_ARG_CHECK(i == 0 || seg_off[i] >= seg_off[i - 1], 4,
                   "mava_clip_adam: seg_off must be non-decreasing");
  }
  MAVA_ARG_CHECK(seg_off[0] == 0, 5, "mava_clip_adam: seg_off[0] must be 0");
  for (int i = 0; i < n_seg; ++i) segs.lr[i] = seg_lr[i];
  const int total = seg_off[n_seg];
  if (total == 0) return MAVA_OK;
  int blocks = mava_cdiv(total, ADAM_THREADS * 4);
  if (blocks > 256) blocks = 256;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(clip_adam_kernel<0>, dim3(blocks), dim3(ADAM_THREADS), 0, s, p, g, m, v, count,
                     segs, n_seg, grad_scale, max_norm, decay, steps_per_update, num_updates, b1,
                     b2, eps, loss_sums, vf_coef, ent_coef, metrics_out, AdamTail{});
  MAVA_LAUNCH_CHECK();
  hipLaunchKernelGGL(bump_counts_kernel, dim3(1), dim3(64), 0, s, count, n_seg);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

namespace {
// Same reduction with the slab row split in two destinations: columns [0, n_main) go to out_main
// and columns [n_main, n_main + n_tail) to out_tail (the loss sums that follow the gradient).
__global__ __launch_bounds__(256) void slab_reduce2_kernel(const float* __restrict__ slab, int n_slab,
                                                           long slab_stride, int n_main, int n_tail,
                                                           int accumulate, float* __restrict__ out_main,
                                                           float* __restrict__ out_tail) {
  __shared__ float part[4][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = i < n_main + n_tail;
  const float acc = slab_column_sum(slab, n_slab, slab_stride, i, live, part);
  if (threadIdx.x < 64 && live) {
    float* dst = (i < n_main) ? (out_main + i) : (out_tail + (i - n_main));
    *dst = accumulate ? (*dst + acc) : acc;
  }
}

}  // namespace

extern "C" int mava_slab_reduce2_f32(const float* slab, int n_slab, long slab_stride, int n_main,
                                     float* out_main, int n_tail, float* out_tail, int accumulate,
                                     hipStream_t s) {
  MAVA_ARG_CHECK(n_main >= 0 && n_tail >= 0 && n_slab >= 0 && slab_stride >= n_main + n_tail, 0,
                 "mava_slab_reduce2_f32: bad shape");
  if (n_main + n_tail == 0) return MAVA_OK;
  // (no slab: nothing is read - the sum is zero - so an empty slab array may come without a pointer)
  MAVA_ARG_CHECK((slab || n_slab == 0) && (n_main == 0 || out_main) && (n_tail == 0 || out_tail), 1,
                 "mava_slab_reduce2_f32: null pointer argument");
  hipLaunchKernelGGL(slab_reduce2_kernel, dim3(mava_cdiv(n_main + n_tail, 64)), dim3(256), 0, s, slab,
                     n_slab, slab_stride, n_main, n_tail, accumulate, out_main, out_tail);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

extern "C" int mava_slab_reduce_f32(const float* slab, int n_slab, long slab_stride, int n,
                                    int accumulate, float* out, hipStream_t s) {
  MAVA_ARG_CHECK(n >= 0 && n_slab >= 0 && slab_stride >= n, 0,
                 "mava_slab_reduce_f32: bad shape n=%d n_slab=%d stride=%ld", n, n_slab,
                 slab_stride);
  if (n == 0) return MAVA_OK;
  MAVA_ARG_CHECK((slab || n_slab == 0) && out, 1, "mava_slab_reduce_f32: null pointer argument");
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(mava_cdiv(n, 64)), dim3(256), 0, s, slab, n_slab,
                     slab_stride, n, accumulate, out);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

namespace {
// Both networks' slabs in ONE launch (fused tail): virtual column c of [actor slab (Pa + 2 columns) | critic slab (Pc + 1)]
// goes to g laid out [actor grad Pa | critic grad Pc | actor_loss, entropy, value_loss]; the column sums are the ones
// slab_reduce2_kernel forms (same partition of the slabs, same order: bit-identical), and every block also leaves the
// squared norm of its 64 columns per network - (sum * grad_scale)^2 in double, fixed order - for the Adam launch.
__global__ __launch_bounds__(256) void slab_reduce_pair_kernel(const float* __restrict__ slab_a, long stride_a,
                                                               const float* __restrict__ slab_c, long stride_c, int n_slab, int Pa,
                                                               int Pc, float grad_scale, float* __restrict__ g,
                                                               double* __restrict__ norm_partials) {
  __shared__ float part[4][64];
  __shared__ double sq[2][64];
  const int na = Pa + 2;                  // actor columns (gradient + 2 loss sums)
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = c < na + Pc + 1;
  const bool actor = c < na;
  const float* slab = actor ? slab_a : slab_c;
  const long stride = actor ? stride_a : stride_c;
  const int col = actor ? c : c - na;
  const float acc = slab_column_sum(slab, n_slab, stride, col, live, part);
  if (threadIdx.x < 64) {
    int dst = -1, seg = -1;
    if (live) {
      if (actor) { dst = (col < Pa) ? col : (Pa + Pc + (col - Pa)); seg = (col < Pa) ? 0 : -1; }
      else { dst = (col < Pc) ? (Pa + col) : (Pa + Pc + 2); seg = (col < Pc) ? 1 : -1; }
      g[dst] = acc;
    }
    const float gi = acc * grad_scale;
    const double q = (double)gi * (double)gi;
    sq[0][threadIdx.x] = (seg == 0) ? q : 0.0;
    sq[1][threadIdx.x] = (seg == 1) ? q : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int k = 0; k < 64; ++k) t += sq[threadIdx.x][k];  // fixed order
    norm_partials[2 * blockIdx.x + threadIdx.x] = t;
  }
}

inline int finish_blocks(int Pa, int Pc) { return mava_cdiv(Pa + 2 + Pc + 1, 64); }
}  // namespace

extern "C" size_t mava_ppo_finish_workspace_bytes(int Pa, int Pc) {
  return (size_t)finish_blocks(Pa, Pc) * 2 * sizeof(double) + 64;  // norm partials | arrival ticket
}

extern "C" int mava_ppo_finish_f32(mava_ctx* ctx, const float* slab_a, long stride_a, const float* slab_c, long stride_c,
                                   int n_slab, int Pa, int Pc, float* g, float* p, float* m, float* v, int32_t* count,
                                   float lr_a, float lr_c, float grad_scale, float max_norm, int decay, int steps_per_update,
                                   int num_updates, float b1, float b2, float eps, float vf_coef, float ent_coef,
                                   float* metrics_out, int critic_din, void* workspace, size_t workspace_bytes,
                                   hipStream_t s) {
  // n_slab == 0: `g` already holds [actor grad | critic grad | 3 loss sums] (summed over slabs, replicas and ranks by the
  // caller - the multi-rank path, whose all-reduce sits between the slab sums and Adam): only the Adam launch runs, with the
  // norms taken from g, and still carries the count increment and the W1 re-split (one launch instead of three)
  const bool reduced = n_slab == 0;
  MAVA_ARG_CHECK(Pa >= 1 && Pc >= 1 && n_slab >= 0 && (reduced || (stride_a >= Pa + 2 && stride_c >= Pc + 1)), 0,
                 "mava_ppo_finish_f32: Pa=%d Pc=%d n_slab=%d strides %ld %ld", Pa, Pc, n_slab, stride_a, stride_c);
  MAVA_ARG_CHECK((reduced || (slab_a && slab_c)) && g && p && m && v && count && workspace, 1,
                 "mava_ppo_finish_f32: null pointer argument");
  MAVA_ARG_CHECK(workspace_bytes >= mava_ppo_finish_workspace_bytes(Pa, Pc) && ((uintptr_t)workspace & 7) == 0, 2,
                 "mava_ppo_finish_f32: workspace of %zu bytes (8-byte aligned, zeroed once) required",
                 mava_ppo_finish_workspace_bytes(Pa, Pc));
  MAVA_ARG_CHECK(!decay || (steps_per_update > 0 && num_updates > 0), 3,
                 "mava_ppo_finish_f32: decay needs steps_per_update>0 and num_updates>0");
  const int nblk = finish_blocks(Pa, Pc);
  double* partials = static_cast<double*>(workspace);
  unsigned int* ticket = reinterpret_cast<unsigned int*>(partials + 2 * nblk);
  if (!reduced) {
    hipLaunchKernelGGL(slab_reduce_pair_kernel, dim3(nblk), dim3(256), 0, s, slab_a, stride_a, slab_c, stride_c, n_slab, Pa, Pc,
                       grad_scale, g, partials);
    MAVA_LAUNCH_CHECK();
  }
  AdamSegs segs = {};
  segs.off[0] = 0; segs.off[1] = Pa; segs.off[2] = Pa + Pc;
  segs.lr[0] = lr_a; segs.lr[1] = lr_c;
  AdamTail tail = {reduced ? nullptr : partials, nblk, ticket, 0, 0, nullptr};
  // the wide f16x2 critic (96 .. 287 inputs) reads W1 through a pre-split copy: re-split it here, from the parameters this
  // launch writes, and mark the handle's copy fresh - the next critic launch of the handle then skips its own pack launch
  const int steps = (critic_din + 1 + 15) / 16;
  const bool pack = ctx != nullptr && ctx->matmul_mode == 1 && critic_din > 0 && steps >= 7 && steps <= 18 &&
                    mlp_param_count(critic_din, 1) == Pc;
  if (pack) {
    void*& slot = ctx->w1_split[1];
    if (slot == nullptr) MAVA_HIP_CHECK(hipMalloc(&slot, h2::W1_SPLIT_BYTES));
    tail.pack_offset = Pa;
    tail.pack_din = critic_din;
    tail.w1_split = static_cast<uint4*>(slot);
  }
  // flat blocks for everything but the W1 range of a packing launch, which PACK_BLOCKS further blocks update and split
  int blocks = mava_cdiv(Pa + Pc - (pack ? (critic_din + 1) * MLP_H : 0), ADAM_THREADS * 4);
  if (blocks > 256) blocks = 256;
  if (pack) blocks += PACK_BLOCKS;
#define FINISH_ADAM(PK)                                                                                              \
  hipLaunchKernelGGL(clip_adam_kernel<PK>, dim3(blocks), dim3(ADAM_THREADS), 0, s, p, g, m, v, count, segs, 2, grad_scale, \
                     max_norm, decay, steps_per_update, num_updates, b1, b2, eps, g + Pa + Pc, vf_coef, ent_coef,      \
                     metrics_out, tail)
  if (pack && steps <= 12) FINISH_ADAM(12);
  else if (pack) FINISH_ADAM(18);
  else FINISH_ADAM(0);
#undef FINISH_ADAM
  MAVA_LAUNCH_CHECK();
  if (pack) {  // the key of the copy (ctx.h): the critic's parameters, width and the steps of the instantiation that packed it
    ctx->w1_fresh[1] = 1;
    ctx->w1_key_params[1] = p + Pa;
    ctx->w1_key_din[1] = critic_din;
    ctx->w1_key_steps[1] = steps <= 12 ? 12 : 18;
  }
  return MAVA_OK;
}
