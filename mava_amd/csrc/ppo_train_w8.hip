// Fused PPO actor minibatch kernel, f16x2 arithmetic, EIGHT waves per workgroup (two per SIMD).
//
// Reference: mava/systems/ppo/ff_mappo.py:150-180 (_actor_loss_fn), :204-214 (value_and_grad), :268-285 (shuffle as an
// index vector) - the same math and the same split-f16 products as ppo_train_h2.hip, phase by phase.
//
// Why a second mapping.  ppo_train_h2.hip runs four waves (one per SIMD, 492 registers each) on 32x32x16 MFMAs, wave w
// owning 32 features of every layer.  Its phase stamps (profiles/r02_v5_train_phase_stamps.txt) put a 32-row tile at
// ~12.2 K cycles for 3.8 K cycles of MFMAs: between the matrix phases sit ~1300 vector instructions per wave (splits,
// ReLU masks, image stores, the loss, the gather's address arithmetic), and ONE wave on a SIMD issues a vector
// instruction every 4 cycles where the SIMD could take one every 2 (MI355X_MICROARCH.md, cycle constants) - the kernel
// is bound by vector ISSUE with nothing to overlap it.  Here the same tile is worked by eight waves, wave v owning 16
// features of every layer on v_mfma_f32_16x16x32_f16 (M = 16 features, N = 16 batch rows, two N-tiles per 32-row tile):
// the per-wave register set halves (weights, accumulators: <= 256 registers, so two waves fit a SIMD), each SIMD
// interleaves the vector work of one wave with the matrix work of the other, and the barrier count per tile drops from
// five to four because the weight-gradient products read only the wave's OWN columns of the dz images.
//
// Operand maps (pinned on the hardware by tools/microbench/w8_probe.hip): lane (i = l & 15, kg = l >> 4) holds
// A[i][8 kg + j], B[8 kg + j][i] (j = 0..7) of the 16x16x32 product and C[4 kg + r][i] (r = 0..3); for 16x16x16:
// A[i][4 kg + j], B[4 kg + j][i] - so an accumulator tile IS the B operand of a 16-deep product (the head).
//
// LDS images: [rows][128 features] f16, hi and lo plane, 256-byte rows, 16-byte chunk c of row r at chunk c ^ sw(r),
// sw(r) = ((r & 3) << 1) | (9 * ((r >> 3) & 1)): conflict-free for the row reads of the 16x16x32 B operand
// (ds_read_b128, lanes (n, kg): row n, chunk 4 s + kg) AND for its hardware-transposed reads (ds_read_b64_tr_b16, two
// 4-row blocks 8 rows apart per 32-lane half) - the swizzle (b) of cdna_hip_programming.md T10 is 2-way on the former -
// and 2-way (8 LDS-array cycles for a 6-cycle instruction) on the 8-byte image stores of an accumulator tile (16 lanes =
// 16 rows of one 8-byte column; banks are mod 32 dwords for stores), where sw without the bit 0 term is 4-way (16 cycles:
// with eight waves storing at once that was ~1.3 K LDS-array cycles per tile; tools/lds_swizzle_search.py has the bank
// model and the search over the linear maps).
#include "h2_core.h"
#include "ppo_train_task.h"
#include "ctx.h"

namespace {

using namespace h2;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int STATS_BLOCKS = 128;  // == ppo_train.hip (mava_adv_stats_blocks)
#ifndef MAVA_W8_GWD
#define MAVA_W8_GWD 1
#endif
constexpr int GWD = MAVA_W8_GWD;  // operand prefetch depth of the weight-gradient products
// Deferred-dW1 form of the role-split tile loop on the f16 record (w8_body, DF): 2 = both wave groups run a tile's dW1 product
// inside the next tile's loss phase; 1 = only the staging waves 4-7 do, waves 0-3 keep theirs at the tile's end, alone on their
// SIMDs; 0 = neither (the schedule with dW1 as the last phase of its own tile, which MAVA_CTX_TRAIN_VARIANT bit 2 selects at run
// time).  Measured once each (profiles/defer_*): a 32-row tile of the headline instance takes 9092 cycles at 0, 8748
// at 2 and 8488 at 1 - on waves 0-3 the product does not hide under the loss, it lengthens P3 by ~540 cycles (the wave stalls at
// each MFMA's issue, its SIMD partner running the same product at the same time), where at the tile's end, with the partner gone
// ahead into the next tile's P1 and to barrier A, it takes ~480 instead of ~920.
#ifndef MAVA_W8_DEFER
#define MAVA_W8_DEFER 1
#endif
constexpr int W8_DEFER = MAVA_W8_DEFER;
static_assert(W8_DEFER >= 0 && W8_DEFER <= 2, "MAVA_W8_DEFER is 0, 1 or 2");
// Gathers-ahead form of the deferred-dW1 tile loop (w8_body, AH).  MAVA_W8_AHEAD_ROLES, bit 0: the staging role takes it, bit 1:
// the loss role does; MAVA_W8_AHEAD_POS: where the staging waves' block of row gathers and cursor updates sits in P3 - 0: behind
// the commit, in front of the deferred dW1 product; 1: behind the product.  Measured (profiles/ahead_bench.json,
// headline ms per update against the parent in the same calls): roles 1 / pos 0 -0.05, roles 1 / pos 1 -0.04, roles 3 / pos 1 -0.03
// and -0.04, roles 3 / pos 0 -0.02, roles 2 +0.03 - the loss role's block costs more in front of barrier C than it frees in front
// of barrier A, where waves 0-3 wait anyway.  Default: the staging role alone, behind the commit.
#ifndef MAVA_W8_AHEAD_ROLES
#define MAVA_W8_AHEAD_ROLES 1
#endif
#ifndef MAVA_W8_AHEAD_POS
#define MAVA_W8_AHEAD_POS 0
#endif
constexpr int W8_AHEAD_ROLES = MAVA_W8_AHEAD_ROLES, W8_AHEAD_POS = MAVA_W8_AHEAD_POS;
static_assert(W8_AHEAD_ROLES >= 0 && W8_AHEAD_ROLES <= 3 && (W8_AHEAD_POS == 0 || W8_AHEAD_POS == 1), "MAVA_W8_AHEAD_ROLES is 0 .. 3, MAVA_W8_AHEAD_POS 0 or 1");

#ifdef MAVA_STAMPS
// Cycle sums per phase: accumulator i is lane i of ONE vector register, 32 bits each (a launch is ~1.2 M cycles) - sixteen 64-bit
// sums in scalar registers cost the kernel, which is at its scalar register limit, spills and kernel-argument reloads inside the
// stamped blocks, and the stamps then measured those
#define WSTAMP_DECL unsigned ws_prev = (unsigned)__builtin_readcyclecounter(), ws_v = 0u;
#define WSTAMP(i)                                                                                        \
  do {                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    const unsigned ws_now = (unsigned)__builtin_readcyclecounter();                                      \
    ws_v += ((threadIdx.x & 63u) == (unsigned)(i)) ? (ws_now - ws_prev) : 0u;                            \
    ws_prev = ws_now;                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
  } while (0)
#else
#define WSTAMP_DECL
#define WSTAMP(i)
#endif

struct Frag4 {  // split operand of the 16-deep product: 4 k-values per lane as hi + lo
  half4 hi, lo;
};
__device__ __forceinline__ f32x4 mfma3w(const Frag& a, const Frag& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, b.hi, c, 0, 0, 0);  // small terms first
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.hi, c, 0, 0, 0);
}
// the same sum when one operand's low term is known to be zero (its product would add exactly 0: same bits, one MFMA less)
__device__ __forceinline__ f32x4 mfma2w_blo0(const Frag& a, const half8& bhi, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, bhi, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, bhi, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma2w_alo0(const half8& ahi, const Frag& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, b.hi, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma3k16(const Frag4& a, const Frag4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x16f16(a.lo, b.hi, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.hi, c, 0, 0, 0);
}
__device__ __forceinline__ Frag4 split4(const f32x4& v) {
  Frag4 f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    _Float16 a, b;
    split1(v[r], a, b);
    f.hi[r] = a;
    f.lo[r] = b;
  }
  return f;
}

// ---- image addressing (bytes) -------------------------------------------------------------------------------------------
constexpr int WROW = 256;              // bytes per image row
constexpr int WPLANE32 = 32 * WROW;    // one plane of a 32-row image
constexpr int WIMG = 2 * WPLANE32;     // hi + lo
constexpr int W2PLANE = 128 * WROW;
constexpr int DYROW = 48;              // [32 rows][16 outputs] f16 + 16 bytes: conflict-free 8-byte row reads
constexpr int DYPLANE = 32 * DYROW;
__host__ __device__ inline int w8_sw(int row) { return ((row & 3) << 1) | (((row >> 3) & 1) * 9); }
__host__ __device__ inline int w8_off(int row, int chunk) { return WROW * row + 16 * (chunk ^ w8_sw(row)); }

struct W8Layout {
  int h1, dz2, dz1, w2, xs, dy, small, h2hi, h2lo, end;
};
// One layout for every form of the tile loop.  The deferred-dW1 form (w8_body, DF != 0) reads the four planes of the x region
// differently - three hi planes of x, a ring, and the hi plane of an h2 image of its own - and is the only one that touches h2lo.
inline W8Layout make_w8_layout() {
  W8Layout L;
  L.h1 = 0;
  L.dz2 = L.h1 + WIMG;   // also the partial logits (f32), idle between barriers A and B2
  L.dz1 = L.dz2 + WIMG;  // also the h2 image (DF == 0): every wave reads back only its OWN 16 columns of either
  L.w2 = L.dz1 + WIMG;   // W2 [128 k][128 n]: row reads for dh1 = W2 . dz2 (the forward operand lives in registers)
  L.xs = L.w2 + 2 * W2PLANE;
  L.dy = L.xs + 2 * WIMG;  // two x buffers (hi, lo | hi, lo); DF != 0: x ring slots 0, 1, 2 | h2 hi plane
  L.small = L.dy + 2 * DYPLANE;
  L.h2hi = L.xs + 3 * WPLANE32;                         // DF != 0: the fourth plane of the x region
  L.h2lo = (L.small + (32 + 16 + 16) * 4 + 15) & ~15;  // f32: b3[32] | misc[16] | dummy, then DF != 0: the h2 image's lo plane
  L.end = L.h2lo + WPLANE32;
  return L;
}

// NO: padded action count of the loss lanes (8 or 16); S1: 32-input steps of layer 1 (din + 1 <= 32 S1 <= 128);
// XV: floats per staged piece (2 when the rows are 8-byte aligned and din is even).
// W2R: steps (of four) of the layer-2 forward operand - this wave's 16 columns of W2, 8 registers a step - that stay in
// registers; the others are read from the W2 image with hardware-transposed reads (4 per step, tile and wave).  All four
// resident need 271 registers and spill inside the tile loop; w8_w2r() below picks two where they fit.
// ROLE: with 8 action lanes per row the loss occupies 256 threads, so the per-row duties are divided between the two wave
// groups (separate functions: separate register sets): ROLE 1 = waves 0-3, the loss of the tile's 32 rows; ROLE 2 = waves 4-7,
// the x staging (gather of the next tile's rows, split + commit into the other x buffer) - in the first version, where
// every wave staged and waves 0-3 also ran the loss, waves 4-7 waited ~900 of a tile's 10.7 K cycles at barrier B2
// (phase stamps).  ROLE 0 (16 action lanes: every thread is a loss lane) does both.  All roles run the same barrier sequence
// and the same matrix work on their own 16 features.  (A static priority raise for waves 4-7, the younger half that loses
// issue arbitration against its SIMD partners - s_setprio 1 - was measured: 65.5 M env-steps/s either way.)
// X16 (staging roles): the x tiles come from the task's f16 record of x (TrainTask::x16, rows x16_ld halves apart, laid out
// like an x image row) - 16-byte loads and 16-byte LDS stores of the halves as they are into the hi plane: no split, no low
// plane, no flag; every tile takes the two-product paths of P1 and dW1 (the loss role reads a flag that stays 0).
// DF (roles 1 and 2 of a block whose staging role is the X16 twin; both roles read the same device word and agree): the
// deferred-dW1 form of the tile loop.  The dW1 product of a tile has no place in the tile's dependency chain - it reads the
// tile's x image and the wave's own columns of the dz1 image and adds into gW1[], which nobody reads before the epilogue - and
// since the record the staging waves commit the next x tile in ~220 cycles and then wait ~860 at barrier B2 while waves 0-3 run
// the loss, one dependent chain of vector instructions that leaves the matrix pipe and the LDS idle
// (profiles/view16_after_phase_stamps.txt).  With DF == 2 the product of tile n runs inside P3 of tile n + 1 (once more behind
// the loop for the block's last tile); DF == 1 has this form's storage and keeps the product at the tile's end.  Storage:
//  - x lives in a ring of three hi planes of the x region (the record path never touches a lo plane): tile n of the block in
//    slot n mod 3; P1 of tile n reads it, P3 of tile n commits tile n + 1 into slot (n + 1) mod 3, the deferred product in P3
//    of tile n reads slot (n - 1) mod 3 (the argument for each slot stands at the commit);
//  - h2 has an image of its own (L.h2hi: the fourth plane of the x region, L.h2lo), because the wave's dz1 columns of tile n
//    must survive P2 of tile n + 1; DZ1I then holds dz1 only, and every wave still reads back only columns it wrote itself:
//    program order is all the ordering either image needs;
//  - no x_lo flag is read: both products of layer 1 are the two-product ones.
// Same accumulators, same products, same tile order as DF == 0: the same bits.  Same __syncthreads sequence in every role.
// AH (either role of a block in the deferred form; the roles need not agree: MAVA_W8_AHEAD_ROLES, default the staging role alone):
// the row gathers, the index loads and the cursor updates leave the stretch in front of barrier A, which every wave is on the path
// to, for places where the role waits:
//  - staging role: P3, behind the commit.  The staging registers are free the moment the commit has stored them, so P3 of tile n
//    commits the x of tile n + 1 and at once issues the gathers of tile n + 2 into the same registers, from the index that P3 of
//    tile n - 1 loaded, and loads the index of tile n + 3.  The gathers are in flight for a whole tile; the role issues no other
//    global load but that index load BEHIND them (loads retire in order: the commit waits for all but the last one);
//  - loss role (measured, not the default): in front of barrier C, behind gW2.  The row of tile n + 1 is loaded straight into r_*, which P3 of tile n is done
//    with - one tile later than without AH, still two barriers and two matrix phases ahead of its use - and the index of tile n + 2
//    is loaded behind it.
// The rule above cursor_gather holds: an index is consumed one tile after the block that loads it.  Same rows, same order: the
// same bits.
template <int NO, int S1, int XV, int W2R, bool ACTOR, int ROLE, bool X16 = false, int DF = 0, bool AH = false>
__device__ __forceinline__ void w8_body(const TrainTask& tk, const W8Layout& L, u8* lds) {
  constexpr bool DO_LOSS = ROLE != 2, DO_STAGE = ROLE != 1;
  static_assert(!AH || DF != 0, "the gathers-ahead form is a form of the deferred-dW1 tile loop");
  static_assert(!X16 || (DO_STAGE && XV == 2), "the f16 record is read by a staging role of an XV = 2 instance");
  static_assert(DF == 0 || (NO == 8 && XV == 2 && (ROLE == 1 || (ROLE == 2 && X16 && DF == 2))),
                "the deferred-dW1 form belongs to the role-split instances on the f16 record; its staging role always defers");
  // ACTOR = false: the value network on narrow inputs (ff_ippo's critic, ff_mappo.py:183-213): one output, the clipped value
  // loss on lane 0 of a row's NO loss lanes; its weights are split as WS * w and the layer accumulators unscaled by WU
  // (h2_core.h W_SCALE_CRITIC: the low terms of the weights leave f16's subnormal range)
  constexpr float WS = ACTOR ? 1.0f : W_SCALE_CRITIC, WU = 1.0f / WS;
  constexpr int KT1 = 2 * S1;  // 16-input tiles of the layer-1 weight gradient
  u8* const H1I = lds + L.h1;
  u8* const DZ2I = lds + L.dz2;
  u8* const DZ1I = lds + L.dz1;
  u8* const W2I = lds + L.w2;
  u8* const DYI = lds + L.dy;
  u8* const H2HI = lds + (DF != 0 ? L.h2hi : L.dz1);            // the h2 image's planes
  u8* const H2LO = lds + (DF != 0 ? L.h2lo : L.dz1 + WPLANE32);
  float* const YP = reinterpret_cast<float*>(lds + L.dz2);
  constexpr int YSTR = (NO == 8) ? 9 : NO;  // floats per (wave, row) of partial logits: 8 x 32 x YSTR x 4 bytes <= one image
  float* const B3s = reinterpret_cast<float*>(lds + L.small);
  float* const misc = B3s + 32;
  // xflag[b] != 0: some staged value of x buffer b has a non-zero low f16 term.  Observations that are exact in f16 - flags,
  // one-hot ids, small integer coordinates: RobotWarehouse's and the synthetic env's whole agents_view - leave it 0, and the
  // layer-1 product and its weight gradient then skip the x_lo . W product (it would add exactly 0) and the reads of that plane.
  unsigned* const xflag = reinterpret_cast<unsigned*>(misc + 2);

  const int tid = threadIdx.x;
  const int l = tid & 63, v = tid >> 6, i = l & 15, kg = l >> 4;
  const int din = tk.din, no = tk.no;
  const long R = (long)tk.Rb * tk.A;
  const float invR = 1.0f / (float)R;
  const float* const P = tk.params;
  const int oW2 = mlp_off_w2(din), oW3 = mlp_off_w3(din);

  // ---------------------------------------------------------------- prologue: LDS images, small vectors
  for (int o = tid * 16; o < L.end; o += 512 * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (tid < no) B3s[tid] = P[mlp_off_b3(din, no) + tid];
  if (tid < (DF != 0 ? 96 : 64)) {  // the ones column of both x buffers: "row din" of W1 in the flat parameter vector is b1
    const int b = tid >> 5, row = tid & 31;  // (DF != 0: of the three ring slots - threads of the loss role, which knows the form)
    *reinterpret_cast<_Float16*>(lds + L.xs + b * (DF != 0 ? WPLANE32 : WIMG) + w8_off(row, din >> 3) + 2 * (din & 7)) = (_Float16)1.0f;
  }
  {
    // W2 image: thread = (output feature n, quarter of the k range), sequential over k with the error-diffusion carry of
    // split1_carry (h2_core.h); coalesced over n
    const int n = tid & 127, k0 = 32 * (tid >> 7);
    float carry = 0.0f;
#pragma unroll 8
    for (int k = k0; k < k0 + 32; ++k) {
      _Float16 x0, x1;
      split1_carry(P[oW2 + k * MLP_H + n] * WS, carry, x0, x1);
      const int o = w8_off(k, n >> 3) + 2 * (n & 7);
      *reinterpret_cast<_Float16*>(W2I + o) = x0;
      *reinterpret_cast<_Float16*>(W2I + W2PLANE + o) = x1;
    }
  }
  if (ACTOR && tid == 0) {
    // ff_mappo.py:164  gae = (gae - gae.mean()) / (gae.std() + 1e-8)   (population std)
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < STATS_BLOCKS; ++b) { s1 += tk.stats[2 * b]; s2 += tk.stats[2 * b + 1]; }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    misc[0] = (float)mean;
    misc[1] = 1.0f / ((float)sqrt(var) + 1e-8f);
  }
  // ---------------------------------------------------------------- weight fragments kept in registers
  // layer 1 (A operand): W1[k = 32 s + 8 kg + e][f = 16 v + i]; k == din is b1, k > din zero
  Frag W1f[S1], W2f[W2R > 0 ? W2R : 1];
  {
    float c1 = 0.0f, c2 = 0.0f;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      float w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 32 * s + 8 * kg + e;
        w[e] = (k <= din) ? P[k * MLP_H + 16 * v + i] * WS : 0.0f;
      }
      W1f[s] = split8_carry(w, c1);
    }
#pragma unroll
    for (int s = 0; s < W2R; ++s) {  // layer 2 (A operand), the first W2R steps: W2[k = 32 s + 8 kg + e][n = 16 v + i]
      float w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = P[oW2 + (32 * s + 8 * kg + e) * MLP_H + 16 * v + i] * WS;
      W2f[s] = split8_carry(w, c2);
    }
  }
  Frag4 W3h, W3d;  // head forward A[m = o = i][k = 4 kg + j] = W3[16 v + 4 kg + j][o]; backward A[m = f = i][k = o = 4 kg + j]
  {
    f32x4 a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = (i < no) ? P[oW3 + (16 * v + 4 * kg + j) * no + i] * W3_SCALE : 0.0f;
      b[j] = (4 * kg + j < no) ? P[oW3 + (16 * v + i) * no + 4 * kg + j] * W3_SCALE : 0.0f;
    }
    W3h = split4(a);
    W3d = split4(b);
  }
  float b2r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b2r[r] = P[mlp_off_b2(din) + 16 * v + 4 * kg + r] * WS;  // (unscaled with the products)
  __syncthreads();
  const float adv_mean = ACTOR ? misc[0] : 0.0f, adv_rstd = ACTOR ? misc[1] : 0.0f;

  // persistent accumulators (R x gradient units): wave v owns output columns [16 v, 16 v + 16) of dW1 and dW2
  f32x4 gW1[KT1], gW2[8], gW3;
#pragma unroll
  for (int t = 0; t < KT1; ++t) gW1[t] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 8; ++t) gW2[t] = f32x4{0, 0, 0, 0};
  gW3 = f32x4{0, 0, 0, 0};
  float ab2[4] = {0, 0, 0, 0}, ab3 = 0.0f, loss_a = 0.0f, loss_b = 0.0f;

  // ---------------------------------------------------------------- rows: cursors, staging, loss inputs
  constexpr int LOSS_THREADS = 32 * NO;   // one lane per (row, action slot): threads [0, 32 NO)
  static_assert(ROLE == 0 ? LOSS_THREADS == 512 : LOSS_THREADS == 256, "role split belongs to 8 action lanes");
  const int lrow = tid / NO, lo = tid & (NO - 1);
  constexpr int TPR = (ROLE == 2) ? 8 : 16;        // staging threads per row
  const int st = (ROLE == 2) ? (tid - 256) : tid;
  const int srow = st / TPR, l16 = st % TPR;
  const int nv = din / XV;                        // pieces per row
  constexpr int NPC = (32 * S1 / XV + TPR - 1) / TPR;   // pieces per thread
  constexpr int NR = DO_STAGE ? NPC * XV : 1;
  const uint32_t Au = (uint32_t)tk.A;
  const uint32_t q_step = 32u * gridDim.x, b_step = q_step / Au, a_step = q_step % Au;
  const uint32_t b_last = (uint32_t)(R - 1) / Au, a_last = (uint32_t)(R - 1) % Au;
  struct Cursor { uint32_t q, b, a; };
  auto cursor_at = [&](int rr) {
    Cursor c;
    c.q = 32u * blockIdx.x + (uint32_t)rr;
    c.b = c.q / Au;
    c.a = c.q - c.b * Au;
    return c;
  };
  auto cursor_advance = [&](Cursor& c) {
    c.q += q_step; c.b += b_step; c.a += a_step;
    if (c.a >= Au) { c.a -= Au; c.b += 1u; }
  };
  // The (t,e) index of a cursor's row is LOADED here and only USED a tile later (row = p_raw * A + a): an index load whose
  // value is consumed in the same block makes the compiler wait for it - and, loads retiring in order, for the x gathers
  // issued just before it: 1.9 K of a tile's 11.7 K cycles in the first version of this kernel (phase stamps).
  auto cursor_gather = [&](const Cursor& c, int32_t& p_raw, uint32_t& a_out) {
    const bool in = c.q < (uint32_t)R;
    const uint32_t b = in ? c.b : b_last;
    a_out = in ? c.a : a_last;
    p_raw = tk.idx ? tk.idx[b] : (int32_t)(tk.idx_base + (long)b);
  };
  // input row of agent row (index p, agent a): the critic's inputs may be shared by groups of xshare agent rows
  auto stage_row = [&](int32_t p_raw, uint32_t a) -> uint32_t {
    const uint32_t fr = (uint32_t)p_raw * Au + a;
    if constexpr (ACTOR) return fr;
    else return (tk.xshare == 1) ? fr : ((uint32_t)tk.xshare == Au ? (uint32_t)p_raw : fr / (uint32_t)tk.xshare);
  };
  auto stage_issue = [&](uint32_t fr, float (&xr)[NR]) {
    const float* xrow = tk.x + (long)fr * din;
#pragma unroll
    for (int k = 0; k < NPC; ++k) {
      const int c = l16 + TPR * k;
      const int cc = (c < nv) ? c : 0;  // a piece past the row end is loaded from the row start and stored to a dummy slot
      if (XV == 2) {
        const float2 t = reinterpret_cast<const float2*>(xrow)[cc];
        xr[2 * k] = t.x; xr[2 * k + 1] = t.y;
      } else {
        xr[k] = xrow[cc];
      }
    }
  };
  u8* const xs_dummy = reinterpret_cast<u8*>(misc + 8);
  const int xsw = 16 * w8_sw(srow);
  // X16: thread l16 of a row takes the 16-byte chunks l16, l16 + TPR, ... of the record's row; same rule for a chunk past the
  // row's last one.  (Pieces are native 4 x 32-bit vectors read through a global-address-space pointer: an array of them stays
  // in registers and the loads are global_load.)
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) u32x4* x16_gptr;
  constexpr int NPC16 = (4 * S1 + TPR - 1) / TPR;  // chunks per thread: an image row holds 4 S1 of them
  // chunks staged per row: up to and including the one with the ones column when the record carries it (x16_ld > din)
  const int rp16 = 8 * ((din + 8) >> 3);
  const int nv16 = (tk.x16_ld < rp16 ? tk.x16_ld : rp16) >> 3;
  auto stage_issue16 = [&](uint32_t fr, u32x4 (&xq)[NPC16]) {
    const x16_gptr xrow = (x16_gptr)(tk.x16 + (long)fr * tk.x16_ld);
#pragma unroll
    for (int k = 0; k < NPC16; ++k) {
      const int c = l16 + TPR * k;
      xq[k] = xrow[(c < nv16) ? c : 0];
    }
  };
  auto stage_commit16 = [&](int xo, const u32x4 (&xq)[NPC16]) {  // xo: byte offset of the hi plane in the x region
    u8* base = lds + L.xs + xo + WROW * srow;
#pragma unroll
    for (int k = 0; k < NPC16; ++k) {
      const int c = l16 + TPR * k;
      *reinterpret_cast<u32x4*>((c < nv16) ? (base + ((16 * c) ^ xsw)) : xs_dummy) = xq[k];
    }
  };
  auto stage_commit = [&](int buf, const float (&xr)[NR]) {
    u8* base = lds + L.xs + buf * WIMG + WROW * srow;
    uint32_t lo_any = 0;
#pragma unroll
    for (int k = 0; k < NPC; ++k) {
      const int c = l16 + TPR * k;
      const bool ok = c < nv;
      const int col = XV * c;  // first feature of the piece
      u8* qa = ok ? (base + ((16 * (col >> 3)) ^ xsw) + 2 * (col & 7)) : xs_dummy;
      u8* qb = ok ? (qa + WPLANE32) : xs_dummy;
      if (XV == 2) {
        typedef _Float16 half2v __attribute__((ext_vector_type(2)));
        half2v a, b;
#pragma unroll
        for (int e = 0; e < 2; ++e) { _Float16 x0, x1; split1(xr[2 * k + e], x0, x1); a[e] = x0; b[e] = x1; }
        *reinterpret_cast<half2v*>(qa) = a;
        *reinterpret_cast<half2v*>(qb) = b;
        lo_any |= __builtin_bit_cast(uint32_t, b) & 0x7FFF7FFFu;
      } else {
        _Float16 x0, x1;
        split1(xr[k], x0, x1);
        *reinterpret_cast<_Float16*>(qa) = x0;
        *reinterpret_cast<_Float16*>(qb) = x1;
        lo_any |= (uint32_t)__builtin_bit_cast(uint16_t, x1) & 0x7FFFu;
      }
    }
    if (lo_any != 0) xflag[buf] = 1u;  // (every writer stores the same value)
  };
  auto load_row = [&](uint32_t fr, int& act, float& f0, float& f1, uint32_t& m) {
    if constexpr (ACTOR) {
      act = tk.action[fr];
      f0 = tk.old_logp[fr];
      f1 = tk.adv[fr];
      const uint8_t* mk = (tk.mask != nullptr && lo < no) ? (tk.mask + (long)fr * no + lo) : nullptr;
      m = 1u;
      if (mk != nullptr) m = *mk;
    } else {
      act = 0;
      f0 = tk.old_value[fr];
      f1 = tk.targets[fr];
      m = 0u;
    }
  };

  const long ntiles = (R + 31) / 32;
  long it = blockIdx.x;
  float xr[X16 ? 1 : NR];
  u32x4 xq[X16 ? NPC16 : 1];
  // the two staging forms behind one pair of names
  auto issue = [&](uint32_t fr) __attribute__((always_inline)) {
    if constexpr (X16) stage_issue16(fr, xq); else stage_issue(fr, xr);
  };
  auto commit = [&](int b) __attribute__((always_inline)) {  // b: x buffer; DF != 0: byte offset of the ring slot
    if constexpr (X16) stage_commit16(DF != 0 ? b : b * WIMG, xq); else stage_commit(b, xr);
  };
  int r_act = 0, n_act = 0;
  float r_f0 = 0.0f, r_f1 = 0.0f, n_f0 = 0.0f, n_f1 = 0.0f;
  uint32_t r_m = 1u, n_m = 1u;
  Cursor cs = cursor_at(DO_STAGE ? srow : 0), cl = cursor_at(DO_LOSS ? lrow : 0);
  int32_t ps_next = 0, pl_next = 0;
  uint32_t as_next = 0, al_next = 0;
  // AH: the loads of this role stay in flight across the loop's back edge.  Everything the prologue loaded is waited for here,
  // once (vmcnt(0); expcnt and lgkmcnt left alone): a prologue load the compiler still counts as pending at the loop's head -
  // b2r, which the actor never touches before P2 - would put a wait for ALL loads, the gathers among them, in front of its first
  // use in every tile
  if constexpr (AH) __builtin_amdgcn_s_waitcnt(0x0F70);
  if (it < ntiles) {
    if constexpr (DO_STAGE) {
      cursor_gather(cs, ps_next, as_next);
      issue(stage_row(ps_next, as_next));
    }
    if constexpr (DO_LOSS) {
      cursor_gather(cl, pl_next, al_next);
      load_row((uint32_t)pl_next * Au + al_next, r_act, r_f0, r_f1, r_m);
    }
    if constexpr (DO_STAGE) {
      commit(0);
      cursor_advance(cs);
    }
    if constexpr (DO_LOSS) cursor_advance(cl);
    if (it + gridDim.x < ntiles) {
      if constexpr (DO_STAGE) { cursor_gather(cs, ps_next, as_next); cursor_advance(cs); }
      if constexpr (DO_LOSS) { cursor_gather(cl, pl_next, al_next); cursor_advance(cl); }
      if constexpr (DO_STAGE && AH) {
        // one stage more: the block's second tile in flight, the index of its third one loaded
        issue(stage_row(ps_next, as_next));
        if (it + 2 * (long)gridDim.x < ntiles) { cursor_gather(cs, ps_next, as_next); cursor_advance(cs); }
      }
    }
  }
  __syncthreads();

  // per-lane LDS byte offsets
  const int swi = w8_sw(i);
  int rdA[4];  // row read of image row (16 nt + i), chunk 4 s + kg: + 4096 nt (+ image base, + plane) as immediates
#pragma unroll
  for (int s = 0; s < 4; ++s) rdA[s] = WROW * i + 16 * ((4 * s + kg) ^ swi);
  const int wrA = WROW * i + 16 * ((2 * v + (kg >> 1)) ^ swi) + 8 * (kg & 1);  // image write: features 16 v + 4 kg .. + 3 of row i
  const int tq = i >> 2, tp = i & 3;
  const int trow = 8 * kg + tq;                       // transposed reads: block row of the first 4-row block
  const int trb = WROW * trow + 8 * (tp & 1);         // (second block: 4 rows = 1024 bytes on; same swizzle)
  const int thx = 16 * ((tp >> 1) ^ w8_sw(trow));     // chunk 2 t + (tp >> 1) of column tile t: ((32 t) ^ thx)
  int trA[8];  // tile-invariant: kept in registers (an xor + add per use otherwise: ~30 vector instructions per tile)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    trA[t] = trb + ((32 * t) ^ thx);
    asm volatile("" : "+v"(trA[t]));
  }
  auto tr_addr = [&](int t) -> int { return trA[t]; };
  const int trOwn = tr_addr(v);                       // this wave's own 16 columns
  auto read_tr = [&](const u8* img, int plane, int a0) -> Frag {
    Frag f;
    f.hi = read_tr8(img + a0, WROW);
    f.lo = read_tr8(img + plane + a0, WROW);
    return f;
  };
  auto read_row = [&](const u8* img, int plane, int a0) -> Frag { return read_row_frag(img, plane, a0); };
  // dy image: row reads (lane (n, kg): outputs 4 kg .. + 3 of row 16 nt + n) and transposed reads (outputs x rows)
  const int dyRd = DYROW * i + 8 * kg;
  const int dyTr = DYROW * trow + 8 * tp;
  int buf = 0;
  // DF != 0: byte offsets in the x region of the ring slots of this tile, the next and the previous one (rotated at the loop's end)
  int xo_cur = 0, xo_nxt = WPLANE32, xo_prv = 2 * WPLANE32;
  // DF != 0: gW1[k][n = 16 v + i] += sum_rows x[row][k] dz1[row][n] for the tile whose x sits at `xsi` and whose dz1 columns this
  // wave wrote last.  All operand reads first, then one product per accumulator and pass: the twelve MFMAs are independent of
  // their neighbours and of the loss chain that follows them on waves 0-3 (each accumulator still takes a_hi . b_lo, then
  // a_hi . b_hi, as mfma2w_alo0 does).
  auto dw1_exact = [&](const u8* xsi) __attribute__((always_inline)) {
    const Frag b = read_tr(DZ1I, WPLANE32, trOwn);
    half8 a[KT1];
#pragma unroll
    for (int t = 0; t < KT1; ++t) a[t] = read_tr8(xsi + tr_addr(t), WROW);
#pragma unroll
    for (int t = 0; t < KT1; ++t) gW1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t], b.lo, gW1[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < KT1; ++t) gW1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t], b.hi, gW1[t], 0, 0, 0);
  };

  WSTAMP_DECL
  for (; it < ntiles; it += gridDim.x, buf ^= 1) {
    WSTAMP(14);
    const long itn = it + gridDim.x;
    const bool have_next = itn < ntiles;
    // (wave-uniform) DF == 2: no product is pending yet.  The guard saves the work, the bits do not depend on it: until the block's
    // first P4 the dz1 image holds the prologue's zeros, and the product would add +0 to accumulators that are +0.
    const bool first_tile = it == (long)blockIdx.x;
    const u8* const XSI = lds + L.xs + (DF != 0 ? xo_cur : buf * WIMG);
    // rows of the next tile from the indices loaded a tile ago
    // (AH: formed where the role issues its loads)
    uint32_t xrow_next = (DO_STAGE && !AH) ? stage_row(ps_next, as_next) : 0u, lrow_next = (DO_LOSS && !AH) ? ((uint32_t)pl_next * Au + al_next) : 0u;
    if constexpr (DO_STAGE && !AH) asm volatile("" : "+v"(xrow_next));
    if constexpr (DO_LOSS && !AH) asm volatile("" : "+v"(lrow_next));
    // AH, staging role, tile n of the block: gathers of tile n + 2 into the registers that the commit of tile n + 1 has just
    // emptied, then the index of tile n + 3
    auto stage_ahead = [&]() __attribute__((always_inline)) {
      if constexpr (DO_STAGE && AH) {
        if (itn + gridDim.x < ntiles) {
          issue(stage_row(ps_next, as_next));
          if (itn + 2 * (long)gridDim.x < ntiles) { cursor_gather(cs, ps_next, as_next); cursor_advance(cs); }
        }
      }
    };

    // ---------------------------------------------------------------- P1: z1 = W1^T x^T (+ b1 through the ones column)
    f32x4 acc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
    // (wave-uniform: one branch per phase; DF != 0: the record is exact in f16 and the launch does not force the low products)
    const bool x_lo = DF == 0 && (__builtin_amdgcn_readfirstlane((int)xflag[buf]) != 0 || tk.force_xlo != 0);
    if (x_lo) {
      Frag xb[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) xb[nt] = read_row(XSI + 4096 * nt, WPLANE32, rdA[0]);
#pragma unroll
      for (int s = 0; s < S1; ++s) {
        Frag b[2] = {xb[0], xb[1]};
        if (s + 1 < S1) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) xb[nt] = read_row(XSI + 4096 * nt, WPLANE32, rdA[(s + 1) & 3]);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] = mfma3w(W1f[s], b[nt], acc[nt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {  // x is exact in f16: hi plane only, two products
      half8 xb[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) xb[nt] = *reinterpret_cast<const half8*>(XSI + 4096 * nt + rdA[0]);
#pragma unroll
      for (int s = 0; s < S1; ++s) {
        const half8 b[2] = {xb[0], xb[1]};
        if (s + 1 < S1) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) xb[nt] = *reinterpret_cast<const half8*>(XSI + 4096 * nt + rdA[(s + 1) & 3]);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] = mfma2w_blo0(W1f[s], b[nt], acc[nt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WSTAMP(0);
    uint32_t relu1 = 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[nt][r] = fmaxf(ACTOR ? acc[nt][r] : acc[nt][r] * WU, 0.0f);
        relu1 |= (acc[nt][r] > 0.0f) ? (1u << (4 * nt + r)) : 0u;
      }
      const Frag4 f = split4(acc[nt]);
      *reinterpret_cast<half4*>(H1I + 4096 * nt + wrA) = f.hi;
      *reinterpret_cast<half4*>(H1I + 4096 * nt + WPLANE32 + wrA) = f.lo;
    }
    WSTAMP(1);
    // next tile's gathers: their latency hides under P2 .. P3
    if (!AH && have_next) {
      if constexpr (DO_STAGE) issue(xrow_next);
      if constexpr (DO_LOSS) load_row(lrow_next, n_act, n_f0, n_f1, n_m);
      if (itn + gridDim.x < ntiles) {
        if constexpr (DO_STAGE) { cursor_gather(cs, ps_next, as_next); cursor_advance(cs); }
        if constexpr (DO_LOSS) { cursor_gather(cl, pl_next, al_next); cursor_advance(cl); }
      }
    }
    WSTAMP(2);
    __syncthreads();  // A: h1 image complete
    WSTAMP(3);
    // the other x buffer's flag: its last readers (the previous tile's dW1) are behind this barrier, its next writers (this
    // tile's commit) behind barrier B
    if constexpr (DO_STAGE && !X16) {
      if (tid == (ROLE == 2 ? 256 : 0)) xflag[buf ^ 1] = 0u;
    }

    // ---------------------------------------------------------------- P2: z2 = b2 + W2^T h1^T ; head partial logits
    f32x4 h2[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) h2[nt] = f32x4{b2r[0], b2r[1], b2r[2], b2r[3]};
    {
      Frag hb[2], wn;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) hb[nt] = read_row(H1I + 4096 * nt, WPLANE32, rdA[0]);
      // (not resident: W2[k = 32 s + 8 kg + e][n = 16 v + i] = rows 32 s + 8 kg .. of this wave's column tile of the W2 image)
      if constexpr (W2R < 1) wn = read_tr(W2I, W2PLANE, trOwn);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        Frag b[2] = {hb[0], hb[1]};
        const Frag a = (s < W2R) ? W2f[s < W2R ? s : 0] : wn;
        if (s + 1 < 4) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) hb[nt] = read_row(H1I + 4096 * nt, WPLANE32, rdA[s + 1]);
          if (s + 1 >= W2R) wn = read_tr(W2I + 32 * (s + 1) * WROW, W2PLANE, trOwn);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) h2[nt] = mfma3w(a, b[nt], h2[nt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WSTAMP(4);
    uint32_t relu2 = 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h2[nt][r] = fmaxf(ACTOR ? h2[nt][r] : h2[nt][r] * WU, 0.0f);
        relu2 |= (h2[nt][r] > 0.0f) ? (1u << (4 * nt + r)) : 0u;
      }
      const Frag4 f = split4(h2[nt]);
      // h2 image: only this wave's own columns are ever read back (dy^T . h2 below)
      *reinterpret_cast<half4*>(H2HI + 4096 * nt + wrA) = f.hi;
      *reinterpret_cast<half4*>(H2LO + 4096 * nt + wrA) = f.lo;
      // partial logits of this wave's 16 features: the accumulator tile is the B operand of the 16-deep product
      const f32x4 y = mfma3k16(W3h, f, f32x4{0, 0, 0, 0});
      // register r of lane (row i, kg) is output 4 kg + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * kg + r < NO) YP[(v * 32 + 16 * nt + i) * YSTR + 4 * kg + r] = y[r] * W3_UNSCALE;
      }
    }
    WSTAMP(5);
    __syncthreads();  // B: partial logits complete
    WSTAMP(6);

    // ---------------------------------------------------------------- P3: loss, d loss / d logits (x R) -> dy image
    if constexpr (DO_LOSS && DF == 2) {
      // the previous tile's dW1: its reads ahead of the partial-logit reads, its MFMAs ahead of the loss chain and executing under it
      if (!first_tile) dw1_exact(lds + L.xs + xo_prv);
      WSTAMP(15);
    }
    if constexpr (DO_LOSS) {
      const float lo_c = 1.0f - tk.clip_eps, hi_c = 1.0f + tk.clip_eps;
      const bool rvalid = (it * 32 + lrow) < R;
      const float* yp = YP + lrow * YSTR + lo;
      float y = B3s[lo];
#pragma unroll
      for (int u = 0; u < 8; ++u) y += yp[u * 32 * YSTR];
      float dyo = 0.0f, pg_row = 0.0f, ent_row = 0.0f;
      if constexpr (ACTOR) {
        // masked Categorical over the NO lanes of the row (networks.py:116-124, distributions.py:146-165)
        const bool legal = (lo < no) && (r_m != 0u);
        const float z = legal ? y : -FLT_MAX;
        auto fmax_op = [](float a, float b) { return fmaxf(a, b); };
        auto add_op = [](float a, float b) { return a + b; };
        const float mx = group_allreduce<NO>(z, fmax_op);
        const float se = group_allreduce<NO>(expf(z - mx), add_op);
        // a row without a legal action (mx stayed at finfo.min) is uniform over its `no` real outputs (mlp_core.h Categorical)
        const float logp = (mx == -FLT_MAX) ? ((lo < no) ? -logf((float)no) : -FLT_MAX) : z - (mx + logf(se));
        const float pr = expf(logp);
        const float ent = group_allreduce<NO>((pr > 0.0f) ? -(pr * logp) : 0.0f, add_op);
        const int act = r_act;
        const float lp = group_allreduce<NO>((lo == act) ? logp : 0.0f, add_op);
        const float gae = (r_f1 - adv_mean) * adv_rstd;
        const float ratio = expf(lp - r_f0);
        const float rc = fminf(fmaxf(ratio, lo_c), hi_c);
        const float l1 = ratio * gae, l2 = rc * gae;
        const float pg = -fminf(l1, l2);
        const bool inside = (ratio >= lo_c) && (ratio <= hi_c);
        const float g1 = (l1 < l2) ? 1.0f : ((l1 == l2) ? 0.5f : 0.0f);
        const float g2 = inside ? (1.0f - g1) : 0.0f;
        const float dlp = rvalid ? (-(g1 + g2) * gae * ratio) : 0.0f;  // x R: the 1/R of .mean() is applied at the end
        const float ec = rvalid ? tk.ent_coef : 0.0f;
        const float oh = (lo == act) ? 1.0f : 0.0f;
        const float pl2 = (pr > 0.0f) ? logp : 0.0f;
        dyo = dlp * (oh - pr) + ec * pr * (pl2 + ent);
        if (z == -FLT_MAX) dyo = 0.0f;
        pg_row = pg;
        ent_row = ent;
      } else {
        // clipped value loss (ff_mappo.py:198-213) on lane 0 of the row: y is the value
        const float ov = r_f0, tg = r_f1;
        const float diff = y - ov;
        const float vclip = ov + fminf(fmaxf(diff, -tk.clip_eps), tk.clip_eps);
        const float e1 = y - tg, e2 = vclip - tg;
        const float l1 = e1 * e1, l2 = e2 * e2;
        const bool inside = (diff >= -tk.clip_eps) && (diff <= tk.clip_eps);
        const float g1 = (l1 > l2) ? 1.0f : ((l1 == l2) ? 0.5f : 0.0f);
        const float g2 = inside ? (1.0f - g1) : 0.0f;
        dyo = (rvalid && lo == 0) ? (tk.vf_coef * (g1 * e1 + g2 * e2)) : 0.0f;  // x R
        pg_row = 0.5f * fmaxf(l1, l2);
      }
      _Float16 da, db;
      split1(dyo, da, db);
      *reinterpret_cast<_Float16*>(DYI + lrow * DYROW + 2 * lo) = da;
      *reinterpret_cast<_Float16*>(DYI + DYPLANE + lrow * DYROW + 2 * lo) = db;
      ab3 += dyo;
      if (rvalid && lo == 0) {
        loss_a += pg_row * invR;
        loss_b += ent_row * invR;
      }
      if constexpr (!AH) { r_act = n_act; r_f0 = n_f0; r_f1 = n_f1; r_m = n_m; }
    }
    // the next tile's x rows have arrived: split + store them into the other buffer (its last readers, the dW1 product of
    // the previous tile, finished before barrier A; it is read again from the next tile's P1 on, three barriers away)
    // DF != 0, tile n of the block: the commit writes ring slot (n + 1) mod 3.  Its last readers were the deferred dW1 product of
    // tile n - 2 (slot (n - 2) mod 3 is the same slot), run by every wave in P3 of tile n - 1, hence finished before barrier B2 of
    // tile n - 1 (with DF == 1 waves 0-3 read it last at the end of tile n - 2, before barrier A of tile n - 1); its next readers are
    // P1 of tile n + 1, behind barriers B2 and C of this tile.  Slot n mod 3 is only read in this phase's neighbourhood (P1 of this
    // tile; the product of this tile in P3 of tile n + 1 or at this tile's end); slot (n - 1) mod 3 is read by the deferred
    // product below and on waves 0-3 above, and written next by the commit of tile n + 1, behind barrier B2 of this tile.
    if constexpr (DO_STAGE) {
      if (have_next) commit(DF != 0 ? xo_nxt : (buf ^ 1));
    }
    WSTAMP(7);
    if constexpr (DO_STAGE && AH && W8_AHEAD_POS == 0) {
      stage_ahead();
      WSTAMP(16);
    }
    if constexpr (DO_STAGE && DF == 2) {
      if (!first_tile) dw1_exact(lds + L.xs + xo_prv);  // the previous tile's dW1, in time this role spent waiting at B2
      WSTAMP(15);
    }
    if constexpr (DO_STAGE && AH && W8_AHEAD_POS != 0) {
      stage_ahead();
      WSTAMP(16);
    }
    __syncthreads();  // B2: dy of all 32 rows visible; every reader of the partial logits is done
    WSTAMP(8);

    // ---------------------------------------------------------------- P3b: dW3, dz2 = W3 dy, dW2
    {
      // gW3^T[o][f = 16 v + i] += sum_rows dy[row][o] h2[row][f]   (outputs >= no of the dy image are zero)
      Frag a, b;
      a.hi = read_tr8(DYI + dyTr, DYROW);
      a.lo = read_tr8(DYI + DYPLANE + dyTr, DYROW);
      b.hi = read_tr8(H2HI + trOwn, WROW);
      b.lo = read_tr8(H2LO + trOwn, WROW);
      gW3 = mfma3w(a, b, gW3);
    }
    f32x4 dz[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      Frag4 b;
      b.hi = *reinterpret_cast<const half4*>(DYI + 16 * nt * DYROW + dyRd);
      b.lo = *reinterpret_cast<const half4*>(DYI + DYPLANE + 16 * nt * DYROW + dyRd);
      dz[nt] = mfma3k16(W3d, b, f32x4{0, 0, 0, 0});
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dz[nt][r] = ((relu2 >> (4 * nt + r)) & 1u) ? dz[nt][r] * W3_UNSCALE : 0.0f;
        ab2[r] += dz[nt][r];
      }
      const Frag4 f = split4(dz[nt]);
      *reinterpret_cast<half4*>(DZ2I + 4096 * nt + wrA) = f.hi;
      *reinterpret_cast<half4*>(DZ2I + 4096 * nt + WPLANE32 + wrA) = f.lo;
    }
    WSTAMP(9);
    {
      // gW2[k][n = 16 v + i] += sum_rows h1[row][k] dz2[row][n]: B = this wave's own columns of the dz2 image (written
      // above by this very wave: no barrier), A = column tile t of the h1 image
      // (operand reads run GWD products ahead of their MFMAs; measured on one box, headline env-steps/s: depth 1 68.6 M,
      // 2 68.2 M, 3 67.9 M - the phase is not waiting on its reads; MAVA_W8_GWD, default 1)
      const Frag b = read_tr(DZ2I, WPLANE32, trOwn);
      Frag an[GWD];
#pragma unroll
      for (int t = 0; t < GWD; ++t) an[t] = read_tr(H1I, WPLANE32, tr_addr(t));
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const Frag a = an[t % GWD];
        if (t + GWD < 8) an[t % GWD] = read_tr(H1I, WPLANE32, tr_addr(t + GWD));
        gW2[t] = mfma3w(a, b, gW2[t]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WSTAMP(10);
    if constexpr (DO_LOSS && AH) {
      // the next tile's row straight into r_* (P3 of this tile is done with it), then the index of the tile after next
      if (have_next) {
        load_row((uint32_t)pl_next * Au + al_next, r_act, r_f0, r_f1, r_m);
        if (itn + gridDim.x < ntiles) { cursor_gather(cl, pl_next, al_next); cursor_advance(cl); }
      }
      WSTAMP(17);
    }
    __syncthreads();  // C: dz2 image complete
    WSTAMP(11);

    // ---------------------------------------------------------------- P4: dh1 = W2 dz2^T -> dz1 ; dW1
    {
      acc[0] = f32x4{0, 0, 0, 0};
      acc[1] = f32x4{0, 0, 0, 0};
      Frag an = read_row(W2I + 4096 * v, W2PLANE, rdA[0]);  // W2[16 v + i][32 s + 8 kg .. + 7]
      Frag bn[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bn[nt] = read_row(DZ2I + 4096 * nt, WPLANE32, rdA[0]);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Frag a = an;
        Frag b[2] = {bn[0], bn[1]};
        if (s + 1 < 4) {
          an = read_row(W2I + 4096 * v, W2PLANE, rdA[s + 1]);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) bn[nt] = read_row(DZ2I + 4096 * nt, WPLANE32, rdA[s + 1]);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] = mfma3w(a, b[nt], acc[nt]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][r] = ((relu1 >> (4 * nt + r)) & 1u) ? (ACTOR ? acc[nt][r] : acc[nt][r] * WU) : 0.0f;
        const Frag4 f = split4(acc[nt]);
        *reinterpret_cast<half4*>(DZ1I + 4096 * nt + wrA) = f.hi;
        *reinterpret_cast<half4*>(DZ1I + 4096 * nt + WPLANE32 + wrA) = f.lo;
      }
    }
    WSTAMP(12);
    if constexpr (DF == 2) {
      // this tile's dW1 runs in P3 of the block's next tile, or behind the loop
    } else if constexpr (DF == 1) {
      dw1_exact(XSI);
    } else {
      // gW1[k][n = 16 v + i] += sum_rows x[row][k] dz1[row][n]   (row din of gW1 = db1 through the ones column)
      const Frag b = read_tr(DZ1I, WPLANE32, trOwn);
      constexpr int D1 = GWD < KT1 ? GWD : KT1;
      if (x_lo) {
        Frag an[D1];
#pragma unroll
        for (int t = 0; t < D1; ++t) an[t] = read_tr(XSI, WPLANE32, tr_addr(t));
#pragma unroll
        for (int t = 0; t < KT1; ++t) {
          const Frag a = an[t % D1];
          if (t + D1 < KT1) an[t % D1] = read_tr(XSI, WPLANE32, tr_addr(t + D1));
          gW1[t] = mfma3w(a, b, gW1[t]);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        half8 an[D1];
#pragma unroll
        for (int t = 0; t < D1; ++t) an[t] = read_tr8(XSI + tr_addr(t), WROW);
#pragma unroll
        for (int t = 0; t < KT1; ++t) {
          const half8 a = an[t % D1];
          if (t + D1 < KT1) an[t % D1] = read_tr8(XSI + tr_addr(t + D1), WROW);
          gW1[t] = mfma2w_alo0(a, b, gW1[t]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    WSTAMP(13);
    // no barrier here: the next tile's P1 reads the other x buffer (complete since B2) and writes the h1 image, whose
    // last readers (dW2) sit before barrier C; every other image is rewritten only behind barriers A .. B2
    if constexpr (DF != 0) {
      const int t = xo_prv;
      xo_prv = xo_cur; xo_cur = xo_nxt; xo_nxt = t;
    }
  }
  if constexpr (DF == 2) {
    // the dW1 product of the block's last tile (a block without a tile has none pending)
    if ((long)blockIdx.x < ntiles) dw1_exact(lds + L.xs + xo_prv);
    WSTAMP(15);
  }
#ifdef MAVA_STAMPS
  // (phases 16 and 17 behind the 8 x 16 words of every kernel: the buffer holds 144)
  if (tk.stamps != nullptr && blockIdx.x == 0 && l < 18) tk.stamps[l < 16 ? v * 16 + l : 128 + 2 * v + (l - 16)] = ws_v;
#endif

  // ------------------------------------------------------------------ epilogue: one slab per block (x 1/R)
  __syncthreads();
  if constexpr (X16) {  // proof that this launch read the f16 record
    if (st == 0 && blockIdx.x == 0 && tk.x16_launches != nullptr) atomicAdd(tk.x16_launches, 1ull);
    if constexpr (DF == 2) {  // ... in the deferred-dW1 form
      if (st == 0 && blockIdx.x == 0 && tk.defer_launches != nullptr) atomicAdd(tk.defer_launches, 1ull);
    }
    if constexpr (AH) {  // ... with the gathers a tile ahead
      if (st == 0 && blockIdx.x == 0 && tk.ahead_launches != nullptr) atomicAdd(tk.ahead_launches, 1ull);
    }
  }
  float* slab = tk.slab + (long)blockIdx.x * tk.slab_stride;
  const int oB2 = mlp_off_b2(din), oB3 = mlp_off_b3(din, no);
  const int Pn = mlp_param_count(din, no);
#pragma unroll
  for (int t = 0; t < KT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * t + 4 * kg + r;
      if (k <= din) slab[k * MLP_H + 16 * v + i] = gW1[t][r] * invR;  // row din = db1
    }
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[oW2 + (16 * t + 4 * kg + r) * MLP_H + 16 * v + i] = gW2[t][r] * invR;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float x = ab2[r];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) x += __shfl_xor(x, m, 64);
    if (i == 0) slab[oB2 + 16 * v + 4 * kg + r] = x * invR;
    const int o = 4 * kg + r;
    if (o < no) slab[oW3 + (16 * v + i) * no + o] = gW3[r] * invR;
  }
  float* red = reinterpret_cast<float*>(lds + L.h1);  // epilogue scratch (the tile loop is over)
  if constexpr (DO_LOSS) {
    float x = ab3;
#pragma unroll
    for (int m = NO; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    if (l < NO) red[v * NO + l] = x;
    for (int o = 32; o > 0; o >>= 1) {
      loss_a += __shfl_down(loss_a, o, 64);
      loss_b += __shfl_down(loss_b, o, 64);
    }
    if (l == 0) { red[8 * NO + 2 * v] = loss_a; red[8 * NO + 2 * v + 1] = loss_b; }
  }
  __syncthreads();
  constexpr int LW = LOSS_THREADS / 64;  // waves that ran the loss
  if (tid < no) {
    float x = 0.0f;
#pragma unroll
    for (int u = 0; u < LW; ++u) x += red[u * NO + tid];
    slab[oB3 + tid] = x * invR;
  }
  if (tid == 0) {
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int u = 0; u < LW; ++u) { a += red[8 * NO + 2 * u]; b += red[8 * NO + 2 * u + 1]; }
    slab[Pn] = a;
    slab[Pn + 1] = b;
  }
}

// Steps of the layer-2 forward operand kept in registers, per instantiation: two of the four where the register file has room
// (kernel-resource remarks: 254 of 256 registers at <8, 3, 2>, no spills), none in the wide instantiations
constexpr int w8_w2r(int no, int s1, int xv) {
#ifdef MAVA_W8_W2R
  return MAVA_W8_W2R;
#else
  return (no == 8) ? ((s1 <= 2) ? 2 : ((s1 == 3 && xv == 2) ? 2 : 0)) : ((s1 <= 2) ? 2 : 0);
#endif
}
template <int NO, int S1, int XV, int W2R, bool ACTOR>
__global__ __launch_bounds__(512, 2) void ppo_train_w8_kernel(TrainTask tk, W8Layout L) {
  extern __shared__ __attribute__((aligned(16))) u8 lds[];
  // Instances that stage pairs of floats carry both staging forms: the launch passes x16_valid only when everything the host
  // can see allows the f16 record (launch_w8), and the word itself - written by the kernel that wrote the record - is read here,
  // once per block, with a wave-uniform load.  The two forms are separate bodies: neither holds the other's registers.
  constexpr bool X16_CAPABLE = XV == 2;
  if constexpr (NO == 8) {
    // The deferred-dW1 form of the tile loop (w8_body, DF) is chosen for the whole block, ahead of the role split: every wave reads
    // the word (nothing writes it during the launch: the roles agree), the loss role to take the twin that shares the form's
    // storage with the X16 staging twin.  The other branch is the role split as it stands without the form.
    constexpr bool DEFER_CAPABLE = X16_CAPABLE && W8_DEFER != 0;
    bool defer = false;
    if constexpr (DEFER_CAPABLE) {
      if (tk.x16_valid != nullptr && tk.no_defer == 0) defer = __builtin_amdgcn_readfirstlane((int)*tk.x16_valid) == 1;
    }
    // ... and so is its gathers-ahead form (AH), on the actor's instances.  None of them has a scratch access in a tile loop with
    // the staged rows held across a tile (kernel resources and ISA).  The value network keeps the gathers in front of
    // barrier A: its loss is a dozen instructions, so its staging waves - commit, deferred dW1 - are the last at barrier B2 already
    // and the block lengthens the tile there (ff_ippo 8.01 -> 8.08 - 8.13 ms per update with the form on both networks)
    constexpr bool AHEAD_CAPABLE = DEFER_CAPABLE && ACTOR && W8_AHEAD_ROLES != 0;
    if (DEFER_CAPABLE && defer && AHEAD_CAPABLE && tk.no_ahead == 0) {
      if constexpr (AHEAD_CAPABLE) {
        if (threadIdx.x < 256) w8_body<NO, S1, XV, W2R, ACTOR, 1, false, W8_DEFER, (W8_AHEAD_ROLES & 2) != 0>(tk, L, lds);
        else w8_body<NO, S1, XV, W2R, ACTOR, 2, true, 2, (W8_AHEAD_ROLES & 1) != 0>(tk, L, lds);
      }
    } else if (DEFER_CAPABLE && defer) {
      if constexpr (DEFER_CAPABLE) {
        if (threadIdx.x < 256) w8_body<NO, S1, XV, W2R, ACTOR, 1, false, W8_DEFER>(tk, L, lds);
        else w8_body<NO, S1, XV, W2R, ACTOR, 2, true, 2>(tk, L, lds);
      }
    } else if (threadIdx.x < 256) {
      w8_body<NO, S1, XV, W2R, ACTOR, 1>(tk, L, lds);
    } else {
      bool x16 = false;
      if constexpr (X16_CAPABLE) {
        if (tk.x16_valid != nullptr) x16 = __builtin_amdgcn_readfirstlane((int)*tk.x16_valid) == 1;
      }
      if (X16_CAPABLE && x16) {
        if constexpr (X16_CAPABLE) w8_body<NO, S1, XV, W2R, ACTOR, 2, true>(tk, L, lds);
      } else {
        w8_body<NO, S1, XV, W2R, ACTOR, 2>(tk, L, lds);
      }
    }
  } else {
    bool x16 = false;
    if constexpr (X16_CAPABLE) {
      if (tk.x16_valid != nullptr) x16 = __builtin_amdgcn_readfirstlane((int)*tk.x16_valid) == 1;
    }
    if (X16_CAPABLE && x16) {
      if constexpr (X16_CAPABLE) w8_body<NO, S1, XV, W2R, ACTOR, 0, true>(tk, L, lds);
    } else {
      w8_body<NO, S1, XV, W2R, ACTOR, 0>(tk, L, lds);
    }
  }
}

template <int NO, int S1, int XV, bool ACTOR>
int launch_w8(const TrainTask& tk, int n_slab, hipStream_t s) {
  // the f16 record of x: handed to the kernel only where it has the second staging form and the record fits it (rows of whole
  // 16-byte chunks on a 16-byte aligned base that hold at least the din values, one input row per agent row, no forced x_lo
  // products); whether the record is VALID is the kernel's own look at the device word
  const int ld16 = tk.x16_ld != 0 ? tk.x16_ld : tk.din;
  const bool x16_ok = XV == 2 && tk.x16 != nullptr && tk.x16_valid != nullptr && ld16 % 8 == 0 && ld16 >= tk.din &&
                      (uintptr_t)tk.x16 % 16 == 0 && tk.force_xlo == 0 && tk.xshare == 1 && tk.agg <= 1;
  if (g_x16_query != nullptr) {  // (the rule asked, not a launch: ppo_train_task.h)
    *g_x16_query = x16_ok ? 1 : 0;
    return MAVA_OK;
  }
  const W8Layout L = make_w8_layout();
  MAVA_ARG_CHECK(L.end <= 163840, 8, "ppo_train_w8: %d bytes of LDS exceed the 160 KiB of a CU", L.end);
  static bool attr_set = false;
  if (!attr_set) {
    MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)ppo_train_w8_kernel<NO, S1, XV, w8_w2r(NO, S1, XV), ACTOR>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       L.end));
    attr_set = true;
  }
  TrainTask tkl = tk;
  tkl.x16_ld = ld16;
  if (!x16_ok) { tkl.x16 = nullptr; tkl.x16_valid = nullptr; tkl.x16_launches = nullptr; tkl.defer_launches = nullptr; tkl.ahead_launches = nullptr; }
  g_train_last_instance = train_instance_id(3, ACTOR, false, false, NO, S1, XV);
  hipLaunchKernelGGL((ppo_train_w8_kernel<NO, S1, XV, w8_w2r(NO, S1, XV), ACTOR>), dim3(n_slab), dim3(512), L.end, s, tkl, L);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

template <int NO, int S1, bool ACTOR>
int dispatch_w8_xv(const TrainTask& tk, int n_slab, hipStream_t s) {
  if (tk.din % 2 == 0 && ((uintptr_t)tk.x) % 8 == 0) return launch_w8<NO, S1, 2, ACTOR>(tk, n_slab, s);
  // (97 .. 127 inputs staged one float at a time need more staging registers than the eight-wave kernel has: hundreds of
  // spilled registers - the four-wave kernel takes that shape)
  if constexpr (S1 == 4) return 1;
  else return launch_w8<NO, S1, 1, ACTOR>(tk, n_slab, s);
}

template <int NO, bool ACTOR>
int dispatch_w8(const TrainTask& tk, int n_slab, hipStream_t s) {
  const int s1 = (tk.din + 1 + 31) / 32;  // 32-input steps of layer 1, including the ones (bias) column
  switch (s1) {
#ifndef MAVA_FAST_BUILD
    case 1: return dispatch_w8_xv<NO, 1, ACTOR>(tk, n_slab, s);
    case 2: return dispatch_w8_xv<NO, 2, ACTOR>(tk, n_slab, s);
    case 4: return dispatch_w8_xv<NO, 4, ACTOR>(tk, n_slab, s);
#endif
    case 3: return dispatch_w8_xv<NO, 3, ACTOR>(tk, n_slab, s);
    default: return 1;
  }
}

}  // namespace

// Discrete actor (<= 16 actions) or the value network without input aggregation, input width <= 127.  Returns MAVA_OK, 1 when
// the shape is not instantiated here (the caller then runs ppo_train_h2.hip's four-wave kernels), or a negative error code.
int mava_train_w8_launch(const TrainTask& tk, int n_slab, bool actor, hipStream_t s) {
  if (tk.action_f != nullptr || tk.din + 1 > 128) return 1;
  if (!actor) {
    if (tk.agg > 1 || tk.no != 1) return 1;
    return dispatch_w8<8, false>(tk, n_slab, s);
  }
  if (tk.no <= 8) return dispatch_w8<8, true>(tk, n_slab, s);
#ifndef MAVA_FAST_BUILD
  if (tk.no <= 16) return dispatch_w8<16, true>(tk, n_slab, s);
#endif
  return 1;
}
