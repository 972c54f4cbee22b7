// Direct convolution kernels of the CNN torso (mava/networks.py:61-85: nn.Conv 'SAME'): the patch matrix of the implicit
// product is formed in LDS, tile by tile, and never in memory (generic_layers.hip's im2col / col2im write and read it:
// k*k times the activation image per layer and direction).  Three kernels, wave64, eight waves per block:
//
//  * forward       z = patch(src) W + b, y = act(z);
//  * input grad    dsrc = gather form of dz W^T (no atomics): the same kernel with dz as the staged matrix;
//  * weight grad   one slab [dW | db] per block, dW = patch(src)^T dz, for mava_slab_reduce_f32.
//
// All matrices are T32 (element (row, f) of a (rows x N) matrix at ((row / 32) * N + f) * 32 + row % 32), conv rows are
// sample * Hout*Wout + pixel, the geometry is mava_t32_im2col_f32's.
//
// A block takes 32-row output tiles in a persistent loop.  For a tile it stages the BAND of the staged matrix that the
// tile's 32 rows read: a run of image rows (sample * H + y, consecutive over the images a tile straddles; halo included)
// as [pixel][channel] 32-bit words with an odd pixel stride (the staging writes and the gathers below walk pixels: no
// bank conflicts).  A word is the f32 value (exact mode) or its two f16 terms hi | lo << 16 (f16x2 mode): the split is paid
// once per staged element, not once per use, and one ds_read_b32 fetches both terms.
//
// Forward / input gradient: the summation index (k*k*Cin resp. k*k*Cout, in 16-deep steps) is dealt round-robin to the eight
// waves; a wave keeps the weight fragments of ITS steps in registers for all the block's tiles (split once per launch,
// error diffusion along the summation index), gathers the patch fragment of a step from the band - forward: through an
// LDS table that decodes the index into (ky, kx, word offset), in the weight's own row order; input gradient: a step lies
// inside one tap because Cout is a multiple of 16, so the tap's validity ((iy + pad - ky) % stride == 0 and the quotient
// inside the output image) is worked out once per step - and multiplies.  The eight partial tiles are summed in a fixed
// order through LDS (over the band, which is dead by then) and written with coalesced T32 stores.
// Weight gradient: the K x Cout accumulators are dealt to the waves by 32-row tile of K; both operands sum over the tile's
// 32 rows: patch^T is gathered from the band through the table and a per-row record (word offset of tap (0, 0), validity
// bits), dz comes from a staged copy of its tile.  The bias gradient is summed by the staging threads in tile order.
// Out-of-image taps and the padding of the summation index are predicated to zero words.
#include "ctx.h"
#include "h2_core.h"

namespace {

using h2::Frag;
typedef unsigned int u32;

constexpr int NTHREADS = 512, NWAVES = 8;
constexpr int LDS_LIMIT = 163840;
constexpr int DZ_LD = 36;  // words per feature of the staged dz tile (32 rows + 4)
// device code without packed f32 arithmetic (the host pass does not know the feature and would warn)
#ifdef __HIP_DEVICE_COMPILE__
#define NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PACKED_F32
#endif

struct ConvTask {
  const float* src;  // the staged matrix: the layer's source (forward, weight gradient) or dz (input gradient)
  const float* w;
  const float* bias;
  const float* dz;   // weight gradient: T32 (rows x Cout)
  float* z;          // forward: pre-activations; input gradient: dsrc
  float* y;
  float* slab;
  long slab_stride, ntiles;
  float out_scale;
  int src_flat, act;
  int Hin, Win, C, k, st, Hout, Wout, pad_h, pad_w, Cout;
  int K, nsteps;     // summation length of the kernel's product and its 16-deep steps
};

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ int floordiv(int a, int b) {  // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
// BWD = the input gradient: tile rows are SOURCE pixels and the band holds rows of dz; otherwise tile rows are output
// pixels and the band holds rows of the source image.  First / last band row (inside its image) that tile row y reads:
template <bool BWD>
__host__ __device__ __forceinline__ int band_lo(const ConvTask& t, int y) {
  if (!BWD) return clampi(y * t.st - t.pad_h, 0, t.Hin - 1);
  return clampi(-floordiv(-(y + t.pad_h - t.k + 1), t.st), 0, t.Hout - 1);
}
template <bool BWD>
__host__ __device__ __forceinline__ int band_hi(const ConvTask& t, int y) {
  if (!BWD) return clampi(y * t.st - t.pad_h + t.k - 1, 0, t.Hin - 1);
  return clampi(floordiv(y + t.pad_h, t.st), 0, t.Hout - 1);
}
// rows of the band of the tile whose first row is pixel p_a of its image; g_lo = band_lo of that row
template <bool BWD>
__host__ __device__ __forceinline__ int band_rows(const ConvTask& t, int p_a, int& g_lo) {
  const int P = BWD ? t.Hin * t.Win : t.Hout * t.Wout, WT = BWD ? t.Win : t.Wout, HB = BWD ? t.Hout : t.Hin;
  const int pb = p_a + 31, ds = pb / P, yb = (pb - ds * P) / WT;
  g_lo = band_lo<BWD>(t, p_a / WT);
  const int nb = ds * HB + band_hi<BWD>(t, yb) - g_lo + 1;
  return nb > 0 ? nb : 0;
}

// ---- operands: eight values of the summation index per lane and 16-deep step; slot e of lane half h is index
// 8 h + e of the step (f16 MFMA 32x32x16) or 2 e + h (eight f32 MFMAs 32x32x2)
template <int MODE>
__device__ __forceinline__ int kofs(int h, int e) {
  return MODE ? 8 * h + e : 2 * e + h;
}
template <int MODE>
struct Opnd;
template <>
struct Opnd<1> {
  Frag f;
};
template <>
struct Opnd<0> {
  float v[8];
};
template <int MODE>
__device__ __forceinline__ u32 pack_word(float v) {
  if constexpr (MODE == 0) {
    return __float_as_uint(v);
  } else {
    _Float16 hi, lo;
    h2::split1(v, hi, lo);
    return (u32)__builtin_bit_cast(unsigned short, hi) | ((u32)__builtin_bit_cast(unsigned short, lo) << 16);
  }
}
template <int MODE>
__device__ __forceinline__ Opnd<MODE> from_words(const u32 (&w)[8]) {
  Opnd<MODE> o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if constexpr (MODE == 0) {
      o.v[e] = __uint_as_float(w[e]);
    } else {
      o.f.hi[e] = __builtin_bit_cast(_Float16, (unsigned short)(w[e] & 0xffffu));
      o.f.lo[e] = __builtin_bit_cast(_Float16, (unsigned short)(w[e] >> 16));
    }
  }
  return o;
}
template <int MODE>
__device__ __forceinline__ Opnd<MODE> weight_opnd(const float (&v)[8], float& carry) {
  Opnd<MODE> o;
  if constexpr (MODE == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = v[e];
  } else {
    o.f = h2::split8_carry(v, carry);
  }
  return o;
}
template <int MODE>
__device__ __forceinline__ f32x16 mma(const Opnd<MODE>& a, const Opnd<MODE>& b, f32x16 c) {
  if constexpr (MODE == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) c = MFMA32(a.v[e], b.v[e], c);
    return c;
  } else {
    return h2::mfma3(a.f, b.f, c);
  }
}

// ---- band staging: rows g_lo .. g_lo + nb - 1 (counted from image s_a's first row) of a matrix of (HB, WB, CB) images,
// T32 (samples*HB*WB x CB) or, flat, T32 (samples x HB*WB*CB) with feature (y*WB + x)*CB + c
template <int MODE>
__device__ __forceinline__ void stage_band(const float* __restrict__ src, int flat, long s_a, int g_lo, int nb, int HB, int WB, int CB,
                                           u32* band) {
  const int CP = CB | 1, tid = threadIdx.x, npix = nb * WB;
  if (!flat) {
    // the aligned 32-row groups that cover the band are one contiguous run of memory: every load is coalesced
    const long R0 = (s_a * HB + g_lo) * WB, A0 = R0 & ~31L;
    const int lead = (int)(R0 - A0), nt32 = (lead + npix + 31) >> 5;
    const float* p = src + A0 * CB;
    for (int t32 = 0; t32 < nt32; ++t32)
      for (int i = tid; i < 32 * CB; i += NTHREADS) {
        const int q = t32 * 32 + (i & 31) - lead;
        if (q >= 0 && q < npix) band[q * CP + (i >> 5)] = pack_word<MODE>(p[(long)t32 * 32 * CB + i]);
      }
  } else {
    const int HW = HB * WB, poff = g_lo * WB;
    const long N = (long)HW * CB;
    for (int i = tid; i < npix * CB; i += NTHREADS) {
      const int q = i / CB, c = i - q * CB;
      const int ds = (poff + q) / HW;
      const long s = s_a + ds;
      const long f = (long)(poff + q - ds * HW) * CB + c;
      band[q * CP + c] = pack_word<MODE>(src[((s >> 5) * N + f) * 32 + (s & 31)]);
    }
  }
}

// Table entry of summation index kk = (ky*k + kx)*C + c of the forward product: word offset of the tap's channel from the
// row's tap (0, 0) | ky << 16 | kx << 20; past K: ky = 7, which no validity mask has.
__device__ __forceinline__ u32 tab_entry(const ConvTask& t, int kk) {
  if (kk >= t.K) return 7u << 16;
  const int tap = kk / t.C, c = kk - tap * t.C, ky = tap / t.k, kx = tap - ky * t.k;
  return (u32)((ky * t.Win + kx) * (t.C | 1) + c) | ((u32)ky << 16) | ((u32)kx << 20);
}
// Output pixel p_a + j of the tile: word offset of its tap (0, 0), channel 0 in the band (negative inside the padding:
// only valid taps are read) and the validity bits, ky at bit ky, kx at bit 8 + kx.
__device__ __forceinline__ void row_info(const ConvTask& t, int p_a, int g_lo, int j, int& base, u32& vm) {
  const int P = t.Hout * t.Wout, pj = p_a + j, ds = pj / P, p = pj - ds * P;
  const int oy = p / t.Wout, ox = p - oy * t.Wout;
  const int iy0 = oy * t.st - t.pad_h, ix0 = ox * t.st - t.pad_w;
  base = ((ds * t.Hin + iy0 - g_lo) * t.Win + ix0) * (t.C | 1);
  vm = 0;
  for (int q = 0; q < t.k; ++q) {
    if (iy0 + q >= 0 && iy0 + q < t.Hin) vm |= 1u << q;
    if (ix0 + q >= 0 && ix0 + q < t.Win) vm |= 1u << (8 + q);
  }
}
__device__ __forceinline__ bool tap_valid(u32 ent, u32 vm) { return ((vm >> ((ent >> 16) & 7)) & (vm >> (8 + ((ent >> 20) & 7))) & 1u) != 0; }
__device__ __forceinline__ u32 gather(const u32* band, int base, u32 ent, u32 vm) {
  const bool ok = tap_valid(ent, vm);
  const u32 v = band[ok ? base + (int)(ent & 0xffffu) : 0];
  return ok ? v : 0u;
}
__device__ __forceinline__ int div_stride(int v, int st) {  // 0 <= v < 4096, st in 1..3
  return st == 1 ? v : (st == 2 ? (v >> 1) : ((v * 43691) >> 17));
}
__device__ __forceinline__ float act_fwd(float v, int act) {
  if (act == 1) return fmaxf(v, 0.0f);
  if (act == 2) return tanhf(v);
  return v;
}

// Forward (BWD = false) and input gradient (BWD = true).  NS = 16-deep steps per wave (step s belongs to wave s % 8),
// NT = 32-feature output tiles (Cout resp. Cin).
template <int MODE, bool BWD, int NS, int NT>
__global__ __launch_bounds__(NTHREADS) NO_PACKED_F32 void conv_direct_kernel(ConvTask t) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  constexpr int TABW = BWD ? 0 : 16 * NWAVES * NS;
  u32* const tab = lds;
  u32* const band = lds + TABW;
  float* const red = reinterpret_cast<float*>(band);  // the partial tiles, once the band is dead
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NF = BWD ? t.C : t.Cout;                  // output features
  const int nw = t.nsteps < NWAVES ? t.nsteps : NWAVES;

  if constexpr (!BWD) {
    for (int p = tid; p < TABW; p += NTHREADS) tab[p] = tab_entry(t, (p & ~15) + kofs<MODE>((p >> 3) & 1, p & 7));
  }
  // ---- this wave's weight fragments: lane (j, h) holds the weights of output feature 32 tn + j
  Opnd<MODE> wf[NS][NT];
#pragma unroll
  for (int tn = 0; tn < NT; ++tn) {
    float carry = 0.0f;
    const int f = 32 * tn + j;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = w + NWAVES * i;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kk = 16 * s + kofs<MODE>(h, e);
        long at;
        bool ok;
        if constexpr (BWD) {  // W^T: index kk = tap * Cout + co, row tap * Cin + f of the kernel
          const int tap = kk / t.Cout, co = kk - tap * t.Cout;
          ok = kk < t.K && f < NF;
          at = ((long)tap * t.C + f) * t.Cout + co;
        } else {
          ok = kk < t.K && f < NF;
          at = (long)kk * t.Cout + f;
        }
        v[e] = ok ? t.w[ok ? at : 0] : 0.0f;
      }
      wf[i][tn] = weight_opnd<MODE>(v, carry);
    }
  }

  const int PT = BWD ? t.Hin * t.Win : t.Hout * t.Wout;  // tile-side pixels per image
  for (long tile = blockIdx.x; tile < t.ntiles; tile += gridDim.x) {
    const long s_a = (tile * 32) / PT;
    const int p_a = (int)(tile * 32 - s_a * PT);
    int g_lo;
    const int nb = band_rows<BWD>(t, p_a, g_lo);
    __syncthreads();  // the previous tile's partial sums have been read (and the table is written)
    if constexpr (BWD) {
      stage_band<MODE>(t.src, 0, s_a, g_lo, nb, t.Hout, t.Wout, t.Cout, band);
    } else {
      stage_band<MODE>(t.src, t.src_flat, s_a, g_lo, nb, t.Hin, t.Win, t.C, band);
    }
    __syncthreads();
    f32x16 acc[NT];
#pragma unroll
    for (int tn = 0; tn < NT; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tn][r] = 0.0f;
    if (w < nw) {
      int base = 0, iy = 0, ix = 0, ds = 0;
      u32 vm = 0;
      if constexpr (BWD) {
        const int pj = p_a + j;
        ds = pj / PT;
        const int p = pj - ds * PT;
        iy = p / t.Win;
        ix = p - iy * t.Win;
      } else {
        row_info(t, p_a, g_lo, j, base, vm);
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int s = w + NWAVES * i;
        if (s < t.nsteps) {
          u32 wd[8];
          if constexpr (BWD) {
            const int tap = (16 * s) / t.Cout, co0 = 16 * s - tap * t.Cout, ky = tap / t.k, kx = tap - ky * t.k;
            const int ty = iy + t.pad_h - ky, tx = ix + t.pad_w - kx;
            const int oy = div_stride(ty < 0 ? 0 : ty, t.st), ox = div_stride(tx < 0 ? 0 : tx, t.st);
            const bool ok = ty >= 0 && tx >= 0 && oy * t.st == ty && ox * t.st == tx && oy < t.Hout && ox < t.Wout;
            const int a0 = ok ? ((ds * t.Hout + oy - g_lo) * t.Wout + ox) * (t.Cout | 1) + co0 : 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const u32 v = band[ok ? a0 + kofs<MODE>(h, e) : 0];
              wd[e] = ok ? v : 0u;
            }
          } else {
            const uint4* tp = reinterpret_cast<const uint4*>(tab + 16 * s + 8 * h);
            const uint4 e0 = tp[0], e1 = tp[1];
            const u32 ent[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) wd[e] = gather(band, base, ent[e], vm);
          }
          const Opnd<MODE> xb = from_words<MODE>(wd);
#pragma unroll
          for (int tn = 0; tn < NT; ++tn) acc[tn] = mma<MODE>(wf[i][tn], xb, acc[tn]);
        }
      }
    }
    __syncthreads();  // every gather of the band is done: the partial tiles go over it
    if (w < nw) {
#pragma unroll
      for (int tn = 0; tn < NT; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          red[((w * NT + tn) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + j] = acc[tn][r];
    }
    __syncthreads();
    float* const zo = t.z + tile * NF * 32;
    float* const yo = t.y ? t.y + tile * NF * 32 : nullptr;
    for (int o = tid; o < NF * 32; o += NTHREADS) {
      float v = (!BWD && t.bias) ? t.bias[o >> 5] : 0.0f;
      for (int q = 0; q < nw; ++q) v += red[q * NT * 1024 + o];
      zo[o] = v;
      if (!BWD && yo) yo[o] = act_fwd(v, t.act);
    }
  }
}

// Weight and bias gradient.  KTW = 32-row tiles of K per wave (tile kt belongs to wave kt % 8), NT = Cout / 32.
template <int MODE, int KTW, int NT>
__global__ __launch_bounds__(NTHREADS) NO_PACKED_F32 void conv_direct_wgrad_kernel(ConvTask t) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  int* const rinfo = reinterpret_cast<int*>(lds);  // [32 rows][base, validity]
  u32* const dzt = lds + 64;                       // [Cout][DZ_LD]
  u32* const band = dzt + 32 * NT * DZ_LD;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ktiles = (t.K + 31) / 32;

  u32 ent[KTW];  // table entry of this lane's patch column 32 kt + j
#pragma unroll
  for (int i = 0; i < KTW; ++i) ent[i] = tab_entry(t, 32 * (w + NWAVES * i) + j);
  f32x16 acc[KTW][NT];
#pragma unroll
  for (int i = 0; i < KTW; ++i)
#pragma unroll
    for (int tn = 0; tn < NT; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][tn][r] = 0.0f;
  float bacc[2 * NT];  // this thread's share of the column sums of dz: element tid + 512 q of a tile, feature (tid + 512 q) / 32
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) bacc[q] = 0.0f;

  const int PT = t.Hout * t.Wout;
  for (long tile = blockIdx.x; tile < t.ntiles; tile += gridDim.x) {
    const long s_a = (tile * 32) / PT;
    const int p_a = (int)(tile * 32 - s_a * PT);
    int g_lo;
    const int nb = band_rows<false>(t, p_a, g_lo);
    __syncthreads();  // the previous tile's operands have been read
    stage_band<MODE>(t.src, t.src_flat, s_a, g_lo, nb, t.Hin, t.Win, t.C, band);
    if (tid < 32) {
      int base;
      u32 vm;
      row_info(t, p_a, g_lo, tid, base, vm);
      rinfo[2 * tid] = base;
      rinfo[2 * tid + 1] = (int)vm;
    }
    const float* dzg = t.dz + tile * t.Cout * 32;
#pragma unroll
    for (int q = 0; q < 2 * NT; ++q) {
      const int idx = tid + NTHREADS * q;
      const float v = dzg[idx];
      bacc[q] += v;
      dzt[(idx >> 5) * DZ_LD + (idx & 31)] = pack_word<MODE>(v);
    }
    __syncthreads();
#pragma unroll
    for (int stp = 0; stp < 2; ++stp) {
      int rb[8];
      u32 rv[8];
      Opnd<MODE> zb[NT];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int row = 16 * stp + kofs<MODE>(h, e);
        rb[e] = rinfo[2 * row];
        rv[e] = (u32)rinfo[2 * row + 1];
      }
#pragma unroll
      for (int tn = 0; tn < NT; ++tn) {
        u32 wd[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wd[e] = dzt[(32 * tn + j) * DZ_LD + 16 * stp + kofs<MODE>(h, e)];
        zb[tn] = from_words<MODE>(wd);
      }
#pragma unroll
      for (int i = 0; i < KTW; ++i) {
        if (w + NWAVES * i < ktiles) {
          u32 wd[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) wd[e] = gather(band, rb[e], ent[i], rv[e]);
          const Opnd<MODE> xa = from_words<MODE>(wd);
#pragma unroll
          for (int tn = 0; tn < NT; ++tn) acc[i][tn] = mma<MODE>(xa, zb[tn], acc[i][tn]);
        }
      }
    }
  }
  // ---- the block's slab: [dW (K x Cout) | db (Cout)]; a block without tiles writes zeros
  float* const slab = t.slab + (long)blockIdx.x * t.slab_stride;
  const float sc = t.out_scale;
#pragma unroll
  for (int i = 0; i < KTW; ++i)
#pragma unroll
    for (int tn = 0; tn < NT; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * (w + NWAVES * i) + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (kk < t.K) slab[(long)kk * t.Cout + 32 * tn + j] = acc[i][tn][r] * sc;
      }
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) {
    float b = bacc[q];
    b += __shfl_xor(b, 1, 64);
    b += __shfl_xor(b, 2, 64);
    b += __shfl_xor(b, 4, 64);
    b += __shfl_xor(b, 8, 64);
    b += __shfl_xor(b, 16, 64);
    if (j == 0) slab[(long)t.K * t.Cout + ((tid + NTHREADS * q) >> 5)] = b * sc;
  }
}

// ---- host side
// Fills the geometry; returns 1 outside the envelope (nothing is launched), an argument error code for nonsense.
int conv_task(ConvTask& t, const char* who, long samples, int Hin, int Win, int C, int k, int stride, int Cout, int src_flat) {
  MAVA_ARG_CHECK(samples >= 0 && Hin >= 1 && Win >= 1 && C >= 1 && k >= 1 && stride >= 1 && Cout >= 1, 0,
                 "%s: bad geometry samples=%ld Hin=%d Win=%d C=%d k=%d stride=%d Cout=%d", who, samples, Hin, Win, C, k, stride, Cout);
  if (k > 4 || stride > 3 || C > 64 || (Cout != 32 && Cout != 64) || Hin > 32 || Win > 32 || samples % 32 != 0) return 1;
  t = ConvTask{};
  t.Hin = Hin; t.Win = Win; t.C = C; t.k = k; t.st = stride; t.Cout = Cout; t.src_flat = src_flat;
  // flax nn.Conv padding='SAME' (as generic_layers.hip conv_geo)
  t.Hout = (Hin + stride - 1) / stride;
  t.Wout = (Win + stride - 1) / stride;
  const int ph = (t.Hout - 1) * stride + k - Hin, pw = (t.Wout - 1) * stride + k - Win;
  t.pad_h = (ph > 0 ? ph : 0) / 2;
  t.pad_w = (pw > 0 ? pw : 0) / 2;
  return MAVA_OK;
}

template <bool BWD>
int band_words(const ConvTask& t) {  // the largest band over every alignment of a tile in its image
  const int P = BWD ? t.Hin * t.Win : t.Hout * t.Wout;
  int nbmax = 0, g_lo;
  for (int p = 0; p < P; ++p) {
    const int nb = band_rows<BWD>(t, p, g_lo);
    nbmax = nb > nbmax ? nb : nbmax;
  }
  return nbmax * (BWD ? t.Wout * (t.Cout | 1) : t.Win * (t.C | 1)) + 1;
}

template <typename Kern>
int launch(Kern kern, const ConvTask& t, int blocks, int lds_bytes, hipStream_t s) {
  if (lds_bytes > LDS_LIMIT) return 1;
  MAVA_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(NTHREADS), lds_bytes, s, t);
  MAVA_LAUNCH_CHECK();
  return MAVA_OK;
}

template <int MODE, bool BWD>
int launch_direct(const ConvTask& t, hipStream_t s) {
  const int ns = (t.nsteps + NWAVES - 1) / NWAVES, nt = ((BWD ? t.C : t.Cout) + 31) / 32;
  const int nw = t.nsteps < NWAVES ? t.nsteps : NWAVES;
  const int bw = band_words<BWD>(t), rw = nw * nt * 1024;
  const int blocks = (int)(t.ntiles < 512 ? t.ntiles : 512);
#define DIRECT_CASE(NSv, NTv)                                                                          \
  if (ns <= NSv && nt == NTv)                                                                          \
  return launch(conv_direct_kernel<MODE, BWD, NSv, NTv>, t, blocks, 4 * ((BWD ? 0 : 16 * NWAVES * NSv) + (bw > rw ? bw : rw)), s)
  DIRECT_CASE(1, 1); DIRECT_CASE(3, 1); DIRECT_CASE(8, 1); DIRECT_CASE(1, 2); DIRECT_CASE(3, 2); DIRECT_CASE(8, 2);
#undef DIRECT_CASE
  return 1;
}

template <int MODE>
int launch_wgrad(const ConvTask& t, int n_slab, hipStream_t s) {
  const int ktw = ((t.K + 31) / 32 + NWAVES - 1) / NWAVES, nt = t.Cout / 32;
  const int words = 64 + 32 * nt * DZ_LD + band_words<false>(t);
#define WGRAD_CASE(KTWv, NTv) \
  if (ktw <= KTWv && nt == NTv) return launch(conv_direct_wgrad_kernel<MODE, KTWv, NTv>, t, n_slab, 4 * words, s)
  WGRAD_CASE(1, 1); WGRAD_CASE(2, 1); WGRAD_CASE(4, 1); WGRAD_CASE(1, 2); WGRAD_CASE(2, 2); WGRAD_CASE(4, 2);
#undef WGRAD_CASE
  return 1;
}

}  // namespace

extern "C" int mava_conv_fwd_f32(const mava_ctx* ctx, const float* src, int src_flat, long samples, int Hin, int Win, int C, int k,
                                 int stride, int Cout, const float* w, const float* bias, int act, float* z, float* y,
                                 hipStream_t s) {
  ConvTask t;
  const int rc = conv_task(t, "mava_conv_fwd_f32", samples, Hin, Win, C, k, stride, Cout, src_flat);
  if (rc != MAVA_OK) return rc;
  MAVA_ARG_CHECK(act >= 0 && act <= 2, 1, "mava_conv_fwd_f32: act=%d", act);
  if (samples == 0) return MAVA_OK;
  MAVA_ARG_CHECK(src && w && z, 2, "mava_conv_fwd_f32: null pointer argument");
  t.src = src; t.w = w; t.bias = bias; t.act = act; t.z = z; t.y = y;
  t.ntiles = samples * t.Hout * t.Wout / 32;
  t.K = k * k * C;
  t.nsteps = (t.K + 15) / 16;
  return mava_ctx_matmul_mode(ctx) == 1 ? launch_direct<1, false>(t, s) : launch_direct<0, false>(t, s);
}

extern "C" int mava_conv_bwd_data_f32(const mava_ctx* ctx, const float* dz, long samples, int Hin, int Win, int C, int k, int stride,
                                      int Cout, const float* w, float* dsrc, hipStream_t s) {
  ConvTask t;
  const int rc = conv_task(t, "mava_conv_bwd_data_f32", samples, Hin, Win, C, k, stride, Cout, 0);
  if (rc != MAVA_OK) return rc;
  if (samples == 0) return MAVA_OK;
  MAVA_ARG_CHECK(dz && w && dsrc, 2, "mava_conv_bwd_data_f32: null pointer argument");
  t.src = dz; t.w = w; t.z = dsrc;
  t.ntiles = samples * Hin * Win / 32;
  t.K = k * k * Cout;
  t.nsteps = t.K / 16;
  return mava_ctx_matmul_mode(ctx) == 1 ? launch_direct<1, true>(t, s) : launch_direct<0, true>(t, s);
}

extern "C" int mava_conv_bwd_weight_f32(const mava_ctx* ctx, const float* src, int src_flat, long samples, int Hin, int Win, int C,
                                        int k, int stride, int Cout, const float* dz, float grad_scale, float* slab,
                                        long slab_stride, int n_slab, hipStream_t s) {
  ConvTask t;
  const int rc = conv_task(t, "mava_conv_bwd_weight_f32", samples, Hin, Win, C, k, stride, Cout, src_flat);
  if (rc != MAVA_OK) return rc;
  t.K = k * k * C;
  MAVA_ARG_CHECK(n_slab >= 1 && n_slab <= 1024 && grad_scale > 0.0f && slab_stride >= (long)t.K * Cout + Cout, 1,
                 "mava_conv_bwd_weight_f32: n_slab=%d grad_scale=%g slab_stride=%ld (needs %ld)", n_slab, (double)grad_scale,
                 slab_stride, (long)t.K * Cout + Cout);
  MAVA_ARG_CHECK(src && dz && slab, 2, "mava_conv_bwd_weight_f32: null pointer argument");
  t.src = src; t.dz = dz; t.slab = slab; t.slab_stride = slab_stride; t.out_scale = 1.0f / grad_scale;
  t.ntiles = samples * t.Hout * t.Wout / 32;
  return mava_ctx_matmul_mode(ctx) == 1 ? launch_wgrad<1>(t, n_slab, s) : launch_wgrad<0>(t, n_slab, s);
}
