// Thin-channel NHWC convolutions (gfx950): one channel count t is 1 .. 8, the other a multiple of 16 -- the stem of a
// network (RGB or grey image -> 64 channels) and its head (64 channels -> 1 .. 8 maps), with their gradients.  The
// four data-path roles collapse onto two kernels: few -> many (stem forward, head data gradient through the flipped /
// transposed weight pack) and many -> few (head forward, stem data gradient).  All kernels work on the 8 x 32 pixel
// tile of conv_small.hip (4 waves, a wave owns 2 rows = four 16-pixel MFMA fragments) and take the activations as
// they are: t real channels per pixel, no padding to 4 or 16 in memory.
//
// thin_in_kernel<DT, KS, VEC>: few -> many, bound by its stores (128 B written per pixel at Co = 64 against 2 t read)
// ------------------------------------------------------------------------------------------------------
// GEMM: M = pixels, N = Co, K = KS^2 t <= 72, k = tap * t + c.  K is covered by v_mfma_f32_16x16x32 steps and, for a
// rest of 1 .. 16, one last v_mfma_f32_16x16x16 step; the host pads the weight rows with zeros to that length, so a
// lane's A fragment of (16-channel block, step) is one 16-B (8-B) global load.  The fragments of a pass of up to four
// 16-channel blocks (<= 48 VGPRs) are loaded ONCE per block when Co <= 64 and per pass otherwise (they stay in L2).
// A block walks over tiles (grid = a few blocks per CU).  In NHWC with t channels a halo row is ONE contiguous run of
// (32 + 2 d) t elements: it is staged flat, row by row, in units of VEC elements ALIGNED IN GLOBAL MEMORY.  VEC is the
// largest power of two <= 8 that divides the row length W t and the pointer's alignment (RGB with an odd W: rows start
// on 2-byte boundaries only, VEC = 1), so an aligned unit never straddles an image row: it is loaded whole or staged
// as zeros, and the run sits in its LDS row at the phase ph = (-d t) mod VEC it has in memory.  A lane gathers its B
// fragment with 16-bit LDS reads through a k -> (tap, c) offset table built once per block (k >= K: zero).
// Per 16-pixel fragment: gather, <= 3 x 4 MFMAs into 16 accumulator VGPRs, epilogue.  Two 16-channel blocks are
// interleaved (c16_row_channel) so that a lane owns 8 consecutive channels of its pixel: bias, ReLU, one RNE, one 16-B
// store; the 4 lanes of a pixel write 64 contiguous bytes.  The next tile's halo loads are issued into registers right
// after the staging barrier, i.e. before the gathers, MFMAs and stores of the current tile.
//
// thin_out_kernel<DT, KS, F32OUT>: many -> few, bound by its reads
// ------------------------------------------------------------------------------------------------------
// conv_c16_kernel's main loop with ONE 16-row weight block of which t rows are real (the others are zeros made at
// staging time; the MFMA waste is free in a read-bound kernel): 32-channel chunks of the halo tile at the odd pitch of
// 80 B (conv_small.hip "Halo bank argument" holds unchanged), register prefetch of the next chunk before the MFMAs.
// Epilogue: the t real rows (bias, optional ReLU, 16-bit RNE or fp32) are written into an LDS image of the output
// tile -- a tile row's outputs are ONE contiguous run of 32 t elements -- and stored flat in units of the widest
// power of two (<= 16 B) that divides W t and the pointer's alignment.  The 16 - t padding rows are never stored.
//
// wgrad_thin_kernel<DT, KS, STEM> + thin_reduce_kernel: dW [Co][Ci][k][k] and db [Co] in fp32
// ------------------------------------------------------------------------------------------------------
// The GEMM reduces over pixels; the tap shift applies to x.  STEM: x is thin, dz wide; otherwise x is wide, dz thin.
// A block owns 32 channels of the wide side and a slice of the pixel tiles.  Per tile it stages the dz tile and the
// x halo once, as they sit in memory ([pixel][channel]): the wide operand as in wgrad_c16_kernel (pitch 96 B), the
// thin one at 32 B per pixel = 16 channels of which t are real (channels 8 .. 15 are zeroed once per block, 0 .. 7
// come from the pixel's register).  Both are read with the transposing ds_read_b64_tr_b16 (a 16-lane group of the
// thin read covers 4 pixels x 32 B = 128 contiguous bytes: every bank once).  Wave (sw, kh): 16-channel sub-block sw
// of the wide side, tile rows 4 kh .. 4 kh + 3 as its K steps; A = dz, B = x shifted by the tap, KS^2 accumulators.
// db is one MFMA against ones per K step.  The two row halves write separate partials, so a slice contributes two;
// thin_reduce_kernel (c16_reduce_kernel's contract: out = scale * sum + beta * out) sums them 16 ways in parallel:
// partial group g adds partials g, g + 16, ... in order, then the 16 group sums are added in order.  The order is
// fixed by the partial count alone.  No atomics: bitwise repeatable.
#include "api.h"
#include "common.h"
#include "conv_epilogue.h"
#include "conv_thin_plan.h"
#include "conv_small_dev.h"

namespace can {
namespace {

enum { THIN_ERR_ALIGN = -44 };

template <int VEC> struct ThinVec;
template <> struct ThinVec<8> { typedef uint4 type; static __device__ type zero() { return make_uint4(0u, 0u, 0u, 0u); } };
template <> struct ThinVec<4> { typedef uint2 type; static __device__ type zero() { return make_uint2(0u, 0u); } };
template <> struct ThinVec<2> { typedef unsigned type; static __device__ type zero() { return 0u; } };
template <> struct ThinVec<1> { typedef unsigned short type; static __device__ type zero() { return 0; } };

__device__ __forceinline__ uint4 pack8u16(const unsigned short (&v)[8]) {
  return make_uint4((unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16),
                    (unsigned)v[4] | ((unsigned)v[5] << 16), (unsigned)v[6] | ((unsigned)v[7] << 16));
}

// ---------------------------------------------------------------------------------------------------------------
// few -> many
// ---------------------------------------------------------------------------------------------------------------
struct ThinInArgs {
  const bf16_t* x;       // [N][H][W][t]
  const bf16_t* w;       // [Co][KP], k = tap * t + c, zeros from K on
  const float* bias;     // [Co] (EPI_BIAS_RELU / EPI_BIAS)
  bf16_t* y;             // [N][H][W][Co]
  int N, H, W, t, Co, dil, epi;
  int tx, ty, total;     // tiles along the width / height, in all
  int K, KP, nk, tail16; // real K, padded K, MFMA steps, whether the last one is 16 deep
  int ph, upr, rpb;      // phase of the run in its LDS row, units per row, LDS bytes per row
};

template <int DT, int KS, int VEC>
__global__ void __launch_bounds__(256) thin_in_kernel(ThinInArgs a) {
  constexpr int MAXS = KS == 3 ? 3 : 1;
  constexpr int NU = thin_in_nu(VEC, KS);
  constexpr int NJ = C16_NJ;
  typedef typename ThinVec<VEC>::type vec_t;
  __shared__ __attribute__((aligned(16))) unsigned char hal[KS == 3 ? THIN_IN_LDS : C16_TR * THIN_IN_ROW_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int d = a.dil * (KS / 2), HR = C16_TR + 2 * d;
  const int rowel = a.W * a.t;

  // unit tid + 256 i of a halo: (row << 16) | unit of the row; -1 past the halo.  The same for every tile.
  int ucode[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = tid + 256 * i, hr = u / a.upr;
    ucode[i] = hr < HR ? ((hr << 16) | (u - hr * a.upr)) : -1;
  }
  // LDS byte offset of the lane's k values from its pixel's first element; kmask: which of them are below K
  int koff[MAXS][8];
  unsigned kmask = 0u;
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const bool w16 = a.tail16 && s == a.nk - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 32 * s + (w16 ? 4 * fq : 8 * fq) + e;
      const bool ok = s < a.nk && k < a.K && (!w16 || e < 4);
      const int tap = ok ? k / a.t : 0, c = ok ? k - tap * a.t : 0;
      const int kh = tap / KS, kw = tap - kh * KS;
      koff[s][e] = kh * a.dil * a.rpb + 2 * (kw * a.dil * a.t + c);
      kmask |= (ok ? 1u : 0u) << (s * 8 + e);
    }
  }

  const int co16 = a.Co >> 4, npass = (co16 + NJ - 1) / NJ;
  uint4 wf[NJ][MAXS];
  float bv[NJ / 2][8];
  auto load_w = [&](int pass) {
    const int njl = min(NJ, co16 - pass * NJ);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int s = 0; s < MAXS; ++s) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j < njl && s < a.nk) {
          const bf16_t* src = a.w + (size_t)(pass * NJ * 16 + c16_row_channel(j, fr, njl)) * a.KP + 32 * s;
          if (a.tail16 && s == a.nk - 1) { const uint2 h = *reinterpret_cast<const uint2*>(src + fq * 4); v.x = h.x; v.y = h.y; }
          else v = *reinterpret_cast<const uint4*>(src + fq * 8);
        }
        wf[j][s] = v;
      }
#pragma unroll
    for (int jp = 0; jp < NJ; jp += 2) {
#pragma unroll
      for (int c = 0; c < 8; ++c) bv[jp / 2][c] = 0.f;
      if (jp < njl && a.epi != EPI_NONE) {
        const bool paired = jp + 1 < njl;
        const int cbase = pass * NJ * 16 + jp * 16 + (paired ? fq * 8 : fq * 4);
        load_bias<4>(bv[jp / 2], a.bias + cbase);
        if (paired) load_bias<4>(bv[jp / 2] + 4, a.bias + cbase + 4);
      }
    }
  };

  vec_t hreg[NU];
  auto prefetch = [&](int tile) {
    int b = tile;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    const int e0 = (tc * C16_TC - d) * a.t - a.ph;       // row-relative element of unit 0: a multiple of VEC
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      vec_t v = ThinVec<VEC>::zero();
      if (ucode[i] >= 0) {
        const int ih = tr * C16_TR - d + (ucode[i] >> 16), e = e0 + (ucode[i] & 0xffff) * VEC;
        if (ih >= 0 && ih < a.H && e >= 0 && e < rowel)
          v = *reinterpret_cast<const vec_t*>(a.x + (size_t)(n * a.H + ih) * rowel + e);
      }
      hreg[i] = v;
    }
  };

  int tile = blockIdx.x;
  if (tile < a.total) prefetch(tile);
  if (npass == 1) load_w(0);
  for (; tile < a.total; tile += gridDim.x) {
    int b = tile;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    const int r0 = tr * C16_TR, c0 = tc * C16_TC;
    __syncthreads();                                     // the previous tile's gathers are done
#pragma unroll
    for (int i = 0; i < NU; ++i)
      if (ucode[i] >= 0)
        *reinterpret_cast<vec_t*>(hal + (ucode[i] >> 16) * a.rpb + (ucode[i] & 0xffff) * (VEC * 2)) = hreg[i];
    __syncthreads();
    if (tile + (int)gridDim.x < a.total) prefetch(tile + gridDim.x);   // in flight during the MFMAs and stores below

    for (int pass = 0; pass < npass; ++pass) {
      if (npass > 1) load_w(pass);
      const int njl = min(NJ, co16 - pass * NJ);
      const int cop = pass * NJ * 16;
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {                      // a real loop: one fragment's gathers and accumulators live
        // fragment i = pixel (r0 + 2 wave + i / 2, c0 + 16 (i & 1) + fr)
        const unsigned char* pb = hal + (wave * 2 + (i >> 1)) * a.rpb + 2 * (a.ph + ((i & 1) * 16 + fr) * a.t);
        uint4 bf[MAXS];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
          unsigned short v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const unsigned short g = *reinterpret_cast<const unsigned short*>(pb + koff[s][e]);
            v[e] = ((kmask >> (s * 8 + e)) & 1u) ? g : (unsigned short)0;
          }
          bf[s] = pack8u16(v);
        }
        f32x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
          if (s < a.nk) {
            if (a.tail16 && s == a.nk - 1) {
#pragma unroll
              for (int j = 0; j < NJ; ++j)
                if (j < njl)
                  acc[j] = mfma16k16<DT>(make_uint2(wf[j][s].x, wf[j][s].y), make_uint2(bf[s].x, bf[s].y), acc[j]);
            } else {
#pragma unroll
              for (int j = 0; j < NJ; ++j)
                if (j < njl)
                  acc[j] = mfma16<DT>(__builtin_bit_cast(frag8_t, wf[j][s]), __builtin_bit_cast(frag8_t, bf[s]), acc[j]);
            }
          }
        }
        const int oh = r0 + wave * 2 + (i >> 1), ow = c0 + (i & 1) * 16 + fr;
#pragma unroll
        for (int jp = 0; jp < NJ; jp += 2) {
          if (jp < njl) {
            const bool paired = jp + 1 < njl;
            const int cbase = cop + jp * 16 + (paired ? fq * 8 : fq * 4);
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = acc[jp][r]; v[4 + r] = acc[jp + 1][r]; }
            if (a.epi == EPI_BIAS_RELU) bias_act<EPI_BIAS_RELU, 8>(v, bv[jp / 2], true);
            else if (a.epi == EPI_BIAS) bias_act<EPI_BIAS, 8>(v, bv[jp / 2], true);
            if (oh < a.H && ow < a.W) {
              bf16_t* dst = a.y + ((size_t)(n * a.H + oh) * a.W + ow) * a.Co + cbase;
              if (paired) *reinterpret_cast<uint4*>(dst) = pack8h<DT>(v);
              else *reinterpret_cast<uint2*>(dst) = make_uint2(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]));
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// many -> few
// ---------------------------------------------------------------------------------------------------------------
struct ThinOutArgs {
  const bf16_t* x;       // [N][H][W][Ci]
  const bf16_t* w;       // [t][KS^2 * Ci], k = tap * Ci + ci
  const float* bias;     // [t] (EPI_BIAS_RELU / EPI_BIAS)
  void* y;               // [N][H][W][t], 16 bit or fp32
  int N, H, W, Ci, t, dil, epi;
  int tx, ty;
  int vec;               // elements per flat store
};

template <int DT, int KS, bool F32OUT>
__global__ void __launch_bounds__(256) thin_out_kernel(ThinOutArgs a) {
  constexpr int T = KS * KS;
  constexpr int NU = (KS == 3) ? (c16_halo_pixels(C16_MAX_DIL) * 4 + 255) / 256 : (C16_TR * C16_TC * 4) / 256;
  constexpr int WU = (T + 3) / 4;                        // weight units per thread: T fragments of 64 units
  constexpr int P = C16_FWD_PITCH;
  constexpr int ES = F32OUT ? 4 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int d = a.dil * (KS / 2), HC = C16_TC + 2 * d, npix = (C16_TR + 2 * d) * HC;
  unsigned char* hal = smem;
  unsigned char* wl = smem + ((npix * P + 15) & ~15);

  int b = blockIdx.x;
  const int tc = b % a.tx; b /= a.tx;
  const int tr = b % a.ty;
  const int n = b / a.ty;
  const int r0 = tr * C16_TR, c0 = tc * C16_TC;

  int pix[NU];
  halo_pixels<NU>(pix, tid, n, r0, c0, d, HC, npix, a.H, a.W);

  const int K = T * a.Ci;
  const int nch = (a.Ci + 31) >> 5;                      // chunks: Ci / 32 full ones + the 16-channel tail

  uint4 hreg[NU], wreg[WU];
  auto prefetch = [&](int ch) {
    const int cb = ch * 32, cw = min(32, a.Ci - cb);
    halo_load<NU>(hreg, pix, a.x, a.Ci, cb, cw >> 3, tid);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int tap = wave + 4 * i;                      // fragment of unit tid + 256 i; rows >= t are zeros
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (tap < T && fr < a.t) {
        const bf16_t* src = a.w + (size_t)fr * K + tap * a.Ci + cb;
        if (cw == 32) v = *reinterpret_cast<const uint4*>(src + fq * 8);
        else { const uint2 h = *reinterpret_cast<const uint2*>(src + fq * 4); v.x = h.x; v.y = h.y; }
      }
      wreg[i] = v;
    }
  };
  auto stage = [&](int ch) {
    const bool tail = (a.Ci - ch * 32) < 32;
    halo_store<NU, P>(hal, hreg, pix, tid);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int u = tid + 256 * i;
      if (u < T * 64) {
        if (!tail) *reinterpret_cast<uint4*>(wl + u * 16) = wreg[i];
        else *reinterpret_cast<uint2*>(wl + u * 8) = make_uint2(wreg[i].x, wreg[i].y);
      }
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned char* hb0 = hal + ((wave * 2) * HC + fr) * P;

  prefetch(0);
  for (int ch = 0; ch < nch; ++ch) {
    const bool tail = (a.Ci - ch * 32) < 32;
    __syncthreads();                                     // the previous chunk's fragment reads are done
    stage(ch);
    __syncthreads();
    if (ch + 1 < nch) prefetch(ch + 1);                  // in flight during the MFMAs below
#pragma unroll
    for (int tap = 0; tap < T; ++tap) {
      const int kh = tap / KS, kw = tap - kh * KS;
      const unsigned char* hb = hb0 + ((kh * a.dil) * HC + kw * a.dil) * P;
      if (!tail) {
        const frag8_t af = *reinterpret_cast<const frag8_t*>(wl + (tap * 64 + lane) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i] = mfma16<DT>(af, *reinterpret_cast<const frag8_t*>(hb + fq * 16 + ((i >> 1) * HC + (i & 1) * 16) * P),
                              acc[i]);
      } else {
        const uint2 af = *reinterpret_cast<const uint2*>(wl + (tap * 64 + lane) * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i] = mfma16k16<DT>(af, *reinterpret_cast<const uint2*>(hb + fq * 8 + ((i >> 1) * HC + (i & 1) * 16) * P),
                                 acc[i]);
      }
    }
  }

  // ---- epilogue: the lane holds channels 4 fq + r of pixel (2 wave + i / 2, 16 (i & 1) + fr) of the tile; the real
  // ones go into the LDS image of the output tile, [8 rows][32 t] elements, over the halo that is no longer read
  __syncthreads();
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.epi != EPI_NONE) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (fq * 4 + r < a.t) bv[r] = a.bias[fq * 4 + r];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int base = ((wave * 2 + (i >> 1)) * C16_TC + (i & 1) * 16 + fr) * a.t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = fq * 4 + r;
      if (c < a.t) {
        float v = acc[i][r];
        if (a.epi != EPI_NONE) v += bv[r];
        if (a.epi == EPI_BIAS_RELU) v = fmaxf(v, 0.f);
        if constexpr (F32OUT) reinterpret_cast<float*>(smem)[base + c] = v;
        else reinterpret_cast<bf16_t*>(smem)[base + c] = f2h<DT>(v);
      }
    }
  }
  __syncthreads();
  // flat stores: unit uu of tile row rr = elements [uu vec, uu vec + vec) of the row's run; W t and the pointer are
  // multiples of vec, so a unit lies inside the image row or past its end as a whole
  const int upr = (C16_TC * a.t) / a.vec;
  const int nvalid = min(C16_TC, a.W - c0) * a.t;
  const int bytes = a.vec * ES;
  for (int u = tid; u < C16_TR * upr; u += 256) {
    const int rr = u / upr, el = (u - rr * upr) * a.vec;
    if (r0 + rr >= a.H || el >= nvalid) continue;
    const unsigned char* src = smem + (size_t)(rr * C16_TC * a.t + el) * ES;
    unsigned char* dst = reinterpret_cast<unsigned char*>(a.y) + (((size_t)(n * a.H + r0 + rr) * a.W + c0) * a.t + el) * ES;
    if (bytes == 16) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else if (bytes == 8) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
    else if (bytes == 4) *reinterpret_cast<unsigned*>(dst) = *reinterpret_cast<const unsigned*>(src);
    else *reinterpret_cast<unsigned short*>(dst) = *reinterpret_cast<const unsigned short*>(src);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// weight + bias gradient
// ---------------------------------------------------------------------------------------------------------------
struct ThinWgArgs {
  const bf16_t* dy;      // [N][H][W][Co]
  const bf16_t* x;       // [N][H][W][Ci]
  float* ws;             // [2 S][Co * Ci * KS^2 + Co]
  int N, H, W, Ci, Co, dil;
  int tx, ty, total, tps;   // tiles along the width / height, tiles in all, tiles per slice
  int want_db;
  int fast;                 // the thin operand's pixels (2 t bytes, t = 2, 4 or 8) are aligned: one load per pixel
};

// the t channels of the thin operand's pixels -> the low halves of 16-B registers (zeros beyond t, outside the image)
template <int NU>
__device__ __forceinline__ void thin_load(uint4 (&reg)[NU], const int (&pix)[NU], const bf16_t* __restrict__ x, int t,
                                          int fast) {
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (pix[i] >= 0) {
      const bf16_t* p = x + (size_t)pix[i] * t;
      if (fast && t == 8) v = *reinterpret_cast<const uint4*>(p);
      else if (fast && t == 4) { const uint2 h = *reinterpret_cast<const uint2*>(p); v.x = h.x; v.y = h.y; }
      else if (fast && t == 2) v.x = *reinterpret_cast<const unsigned*>(p);
      else {
        unsigned short e[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) e[c] = c < t ? p[c] : (unsigned short)0;
        v = pack8u16(e);
      }
    }
    reg[i] = v;
  }
}
template <int NU>
__device__ __forceinline__ void thin_store(unsigned char* lds, const uint4 (&reg)[NU], const int (&pix)[NU], int tid) {
#pragma unroll
  for (int i = 0; i < NU; ++i)
    if (pix[i] != -2) *reinterpret_cast<uint4*>(lds + (tid + 256 * i) * THIN_WG_PITCH) = reg[i];
}

template <int DT, int KS, bool STEM>
__global__ void __launch_bounds__(256) wgrad_thin_kernel(ThinWgArgs a) {
  constexpr int T = KS * KS;
  constexpr int HP = (KS == 3) ? c16_halo_pixels(C16_MAX_DIL) : C16_TR * C16_TC;
  constexpr int NXU = STEM ? (HP + 255) / 256 : (HP * 4 + 255) / 256;   // x units per thread (thin: 1 / pixel)
  constexpr int NDU = STEM ? (C16_TR * C16_TC * 4) / 256 : 1;           // dz units per thread
  constexpr int PX = STEM ? THIN_WG_PITCH : C16_WG_PITCH;
  constexpr int PD = STEM ? C16_WG_PITCH : THIN_WG_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.dil * (KS / 2), HC = C16_TC + 2 * d, npix = (C16_TR + 2 * d) * HC;
  unsigned char* xh = smem;
  unsigned char* dyl = smem + npix * PX;

  const int t = STEM ? a.Ci : a.Co, wide = STEM ? a.Co : a.Ci;
  const int slice = blockIdx.y, w0 = blockIdx.x * C16_WG_CB;
  const int sw = wave & 1, kh2 = wave >> 1;
  const bool active = w0 + 16 * sw < wide;
  const bool do_bias = a.want_db && active && (STEM || (blockIdx.x == 0 && sw == 0));
  const int nuw = min(4, (wide - w0) >> 3);              // valid 16-B channel units of the wide block

  const int t0 = slice * a.tps, t1 = min(a.total, t0 + a.tps);

  // channels 8 .. 15 of the thin operand's pixels: zeros, written once
  {
    unsigned char* th = STEM ? xh : dyl;
    const int np = STEM ? npix : C16_TR * C16_TC;
    for (int hp = tid; hp < np; hp += 256)
      *reinterpret_cast<uint4*>(th + hp * THIN_WG_PITCH + 16) = make_uint4(0u, 0u, 0u, 0u);
  }

  int pix[NXU], dpix[NDU];
  uint4 hreg[NXU], dreg[NDU];
  auto prefetch = [&](int tl) {
    int b = tl;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    if constexpr (STEM) {
      halo_pixels<NXU, 0>(pix, tid, n, tr * C16_TR, tc * C16_TC, d, HC, npix, a.H, a.W);
      halo_pixels<NDU, 2>(dpix, tid, n, tr * C16_TR, tc * C16_TC, 0, C16_TC, C16_TR * C16_TC, a.H, a.W);
      thin_load<NXU>(hreg, pix, a.x, t, a.fast);
      halo_load<NDU>(dreg, dpix, a.dy, a.Co, w0, nuw, tid);
    } else {
      halo_pixels<NXU, 2>(pix, tid, n, tr * C16_TR, tc * C16_TC, d, HC, npix, a.H, a.W);
      halo_pixels<NDU, 0>(dpix, tid, n, tr * C16_TR, tc * C16_TC, 0, C16_TC, C16_TR * C16_TC, a.H, a.W);
      halo_load<NXU>(hreg, pix, a.x, a.Ci, w0, nuw, tid);
      thin_load<NDU>(dreg, dpix, a.dy, t, a.fast);
    }
  };

  f32x4 acc[T], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tp = 0; tp < T; ++tp) acc[tp] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag8_t ones = ones_frag<DT>();

  // transposed reads (conv_small.hip): lane (g, q, p) addresses the 8-B run of channels 4 p .. 4 p + 3 of pixel
  // 4 g + q (low half of the lane's k values) and of pixel 16 + 4 g + q (high half)
  const int g = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
  const int plo = 4 * g + q;
  const unsigned char* dlo = dyl + plo * PD + (STEM ? sw * 32 : 0) + p4 * 8;
  const unsigned char* xlo = xh + plo * PX + (STEM ? 0 : sw * 32) + p4 * 8;

  if (t0 < t1) prefetch(t0);
  for (int tl = t0; tl < t1; ++tl) {
    __syncthreads();
    if constexpr (STEM) { thin_store<NXU>(xh, hreg, pix, tid); halo_store<NDU, PD>(dyl, dreg, dpix, tid); }
    else { halo_store<NXU, PX>(xh, hreg, pix, tid); thin_store<NDU>(dyl, dreg, dpix, tid); }
    __syncthreads();
    if (tl + 1 < t1) prefetch(tl + 1);
    if (active) {
#pragma unroll 2
      for (int rr = 0; rr < C16_TR / 2; ++rr) {
        const int r = kh2 * (C16_TR / 2) + rr;
        const unsigned char* da = dlo + r * C16_TC * PD;
        const frag8_t af = c16_tr_read(da, da + 16 * PD);
        if (do_bias) accb = mfma16<DT>(af, ones, accb);
#pragma unroll
        for (int tap = 0; tap < T; ++tap) {
          const int kh = tap / KS, kw = tap - kh * KS;
          const unsigned char* xa = xlo + ((r + kh * a.dil) * HC + kw * a.dil) * PX;
          const frag8_t bf = c16_tr_read(xa, xa + 16 * PX);
          acc[tap] = mfma16<DT>(af, bf, acc[tap]);
        }
      }
    }
  }

  // D layout: column lane & 15 = input channel, rows 4 (lane >> 4) + r = output channels
  if (active) {
    const int fr = lane & 15, fq = lane >> 4;
    const size_t plane = (size_t)a.Co * a.Ci * T;
    float* part = a.ws + (size_t)(slice * 2 + kh2) * (plane + a.Co);
    const int ci = STEM ? fr : w0 + 16 * sw + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = STEM ? w0 + 16 * sw + fq * 4 + r : fq * 4 + r;
      if (ci < a.Ci && co < a.Co) {
#pragma unroll
        for (int tap = 0; tap < T; ++tap) part[((size_t)co * a.Ci + ci) * T + tap] = acc[tap][r];
        if (do_bias && fr == 0) part[plane + co] = accb[r];
      }
    }
  }
}

// out[i] = scale * sum of the S partials (+ beta * out[i]); i < plane -> dw, else db.  A block owns 16 outputs x 16
// partial groups (see the file header for the order of the sum)
__global__ void __launch_bounds__(256) thin_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                          float* __restrict__ db, int S, int plane, int Co, float beta,
                                                          float scale) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  const int n = plane + (db != nullptr ? Co : 0);
  const size_t stride = (size_t)plane + Co;
  float s = 0.f;
  if (i < n)
    for (int sl = g; sl < S; sl += 16) s += ws[(size_t)sl * stride + i];
  red[g][o] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    float tot = red[0][o];
#pragma unroll
    for (int q = 1; q < 16; ++q) tot += red[q][o];
    float* out = i < plane ? dw + i : db + (i - plane);
    *out = (beta != 0.f) ? scale * tot + beta * *out : scale * tot;
  }
}

size_t thin_wg_lds(int ksize, int dil, bool stem) {
  const int d = dil * (ksize / 2);
  return (size_t)c16_halo_pixels(d) * (stem ? THIN_WG_PITCH : C16_WG_PITCH) +
         (size_t)C16_TR * C16_TC * (stem ? C16_WG_PITCH : THIN_WG_PITCH);
}
size_t thin_out_lds(int ksize, int dil) {
  const int d = dil * (ksize / 2);
  return (size_t)((c16_halo_pixels(d) * C16_FWD_PITCH + 15) & ~15) + (size_t)ksize * ksize * 1024;
}

template <int DT, int KS, int VEC>
int launch_in(const ThinInArgs& a, hipStream_t s) {
  const int grid = a.total < 4 * can_device_cus() ? a.total : 4 * can_device_cus();
  hipLaunchKernelGGL((thin_in_kernel<DT, KS, VEC>), dim3(grid), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
template <int DT, int KS>
int launch_in_vec(const ThinInArgs& a, int vec, hipStream_t s) {
  switch (vec) {
    case 8: return launch_in<DT, KS, 8>(a, s);
    case 4: return launch_in<DT, KS, 4>(a, s);
    case 2: return launch_in<DT, KS, 2>(a, s);
    default: return launch_in<DT, KS, 1>(a, s);
  }
}
template <int DT>
int launch_in_ks(const ThinInArgs& a, int ksize, int vec, hipStream_t s) {
  return ksize == 3 ? launch_in_vec<DT, 3>(a, vec, s) : launch_in_vec<DT, 1>(a, vec, s);
}

template <int DT, int KS, bool F32OUT>
int launch_out(const ThinOutArgs& a, hipStream_t s) {
  auto kfn = thin_out_kernel<DT, KS, F32OUT>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)thin_out_lds(KS, C16_MAX_DIL)));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3(a.N * a.ty * a.tx), dim3(256), thin_out_lds(KS, a.dil), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_out_ks(const ThinOutArgs& a, int ksize, bool f32, hipStream_t s) {
  if (ksize == 3) return f32 ? launch_out<DT, 3, true>(a, s) : launch_out<DT, 3, false>(a, s);
  return f32 ? launch_out<DT, 1, true>(a, s) : launch_out<DT, 1, false>(a, s);
}

template <int DT, int KS, bool STEM>
int launch_wg(const ThinWgArgs& a, int S, hipStream_t s) {
  auto kfn = wgrad_thin_kernel<DT, KS, STEM>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)thin_wg_lds(KS, C16_MAX_DIL, STEM)));
    attr = true;
  }
  const int wide = STEM ? a.Co : a.Ci;
  hipLaunchKernelGGL(kfn, dim3(c16_cdiv(wide, C16_WG_CB), S), dim3(256), thin_wg_lds(KS, a.dil, STEM), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_wg_ks(const ThinWgArgs& a, int ksize, bool stem, int S, hipStream_t s) {
  if (ksize == 3) return stem ? launch_wg<DT, 3, true>(a, S, s) : launch_wg<DT, 3, false>(a, S, s);
  return stem ? launch_wg<DT, 1, true>(a, S, s) : launch_wg<DT, 1, false>(a, S, s);
}

bool thin_pair(int Ci, int Co) {
  const bool in = Ci >= 1 && Ci <= THIN_MAX && Co >= 16 && (Co & 15) == 0;
  const bool out = Co >= 1 && Co <= THIN_MAX && Ci >= 16 && (Ci & 15) == 0;
  return in || out;
}
// what the entry points refuse before any launch
int thin_check(int N, int H, int W, int Ci, int Co, int ksize, int dil) {
  if (N < 1 || H < 1 || W < 1 || !thin_pair(Ci, Co) || (ksize != 1 && ksize != 3)) return C16_ERR_SHAPE;
  if (dil < 1 || dil > C16_MAX_DIL) return C16_ERR_DIL;
  if ((long long)N * H * W * (Ci > Co ? Ci : Co) >= (1LL << 30)) return C16_ERR_ELEMS;   // 32-bit pixel offsets
  return 0;
}
bool aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

}  // namespace
}  // namespace can

extern "C" int can_conv_thin(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Ci,
                             int Co, int ksize, int dil, int epi, int f32out, int dt, void* stream) {
  using namespace can;
  const int rc = thin_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  if (epi != EPI_BIAS_RELU && epi != EPI_BIAS && epi != EPI_NONE) return C16_ERR_SHAPE;
  if (epi != EPI_NONE && bias == nullptr) return C16_ERR_SHAPE;
  if (!aligned16(w) || (epi != EPI_NONE && !aligned16(bias))) return THIN_ERR_ALIGN;
  const int tx = c16_cdiv(W, C16_TC), ty = c16_cdiv(H, C16_TR);
  if (Ci <= THIN_MAX) {
    if (f32out || !aligned16(y)) return f32out ? C16_ERR_SHAPE : THIN_ERR_ALIGN;
    ThinInArgs a;
    a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = (bf16_t*)y;
    a.N = N; a.H = H; a.W = W; a.t = Ci; a.Co = Co; a.dil = dil; a.epi = epi;
    a.tx = tx; a.ty = ty; a.total = N * tx * ty;
    a.K = ksize * ksize * Ci; a.KP = thin_k_pad(a.K); a.nk = thin_k_steps(a.K); a.tail16 = thin_k_tail16(a.K);
    const int d = dil * (ksize / 2), vec = thin_vec(x, (long long)W * Ci, 2, 8);
    a.ph = thin_in_phase(Ci, d, vec); a.upr = thin_in_upr(Ci, d, vec); a.rpb = (a.upr * vec * 2 + 15) & ~15;
    if (a.rpb > THIN_IN_ROW_BYTES || (C16_TR + 2 * d) * a.upr > 256 * thin_in_nu(vec, ksize)) return C16_ERR_SHAPE;
    CAN_DT_DISPATCH(dt, launch_in_ks<DT>(a, ksize, vec, (hipStream_t)stream));
  }
  if (!aligned16(x)) return THIN_ERR_ALIGN;
  ThinOutArgs a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = y;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.t = Co; a.dil = dil; a.epi = epi; a.tx = tx; a.ty = ty;
  a.vec = f32out ? thin_vec(y, (long long)W * Co, 4, 4) : thin_vec(y, (long long)W * Co, 2, 8);
  CAN_DT_DISPATCH(dt, launch_out_ks<DT>(a, ksize, f32out != 0, (hipStream_t)stream));
}

extern "C" int can_conv_thin_partials(long long M, int Ci, int Co) {
  return can::thin_wgrad_partials(M, Ci, Co, can_device_cus());
}

extern "C" int can_conv_thin_wgrad(const void* dy, const void* x, float* ws, long long ws_floats, float* dw, float* db,
                                   int N, int H, int W, int Ci, int Co, int ksize, int dil, float beta, float scale,
                                   int dt, void* stream) {
  using namespace can;
  const int rc = thin_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  const bool stem = Ci <= THIN_MAX;
  const int P = thin_wgrad_partials((long long)N * H * W, Ci, Co, can_device_cus()), S = P / 2;
  if (c16_wgrad_ws_floats(P, Ci, Co, ksize) > ws_floats) return C16_ERR_WS;
  if (!aligned16(stem ? dy : x)) return THIN_ERR_ALIGN;
  ThinWgArgs a;
  a.dy = (const bf16_t*)dy; a.x = (const bf16_t*)x; a.ws = ws;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.dil = dil;
  a.tx = c16_cdiv(W, C16_TC); a.ty = c16_cdiv(H, C16_TR); a.total = N * a.tx * a.ty;
  a.tps = c16_cdiv(a.total, S);
  a.want_db = db != nullptr;
  const int t = stem ? Ci : Co;
  a.fast = (t == 2 || t == 4 || t == 8) && (((size_t)(stem ? x : dy)) % (size_t)(2 * t)) == 0;
  hipStream_t s = (hipStream_t)stream;
  int lrc = -20;
  if (dt == DT_F16) lrc = launch_wg_ks<DT_F16>(a, ksize, stem, S, s);
  else if (dt == DT_BF16) lrc = launch_wg_ks<DT_BF16>(a, ksize, stem, S, s);
  if (lrc) return lrc;
  const int plane = Co * Ci * ksize * ksize;
  const int n = plane + (db != nullptr ? Co : 0);
  hipLaunchKernelGGL(thin_reduce_kernel, dim3(c16_cdiv(n, 16)), dim3(256), 0, s, ws, dw, db, P, plane, Co, beta, scale);
  return (int)hipGetLastError();
}
