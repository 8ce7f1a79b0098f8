// Small-channel NHWC convolutions (gfx950): Ci and Co multiples of 16 of which at least one is no multiple of 64.
// The 64-channel-chunk kernels of conv_igemm.hip / conv_wgrad.hip refuse these layers; this family serves them
// without padding the activations or the weights to 64 channels.
//
// conv_c16_kernel<DT, KS, NJ>: forward, and the data gradient through the flipped / transposed weight pack
// ------------------------------------------------------------------------------------------------------
// A block of 4 waves owns an 8-row x 32-column pixel tile; a wave owns 2 rows = four 16-pixel MFMA fragments.  K is
// small, so the block keeps NO ring over K: the input channels go by in 32-channel chunks (plus one 16-channel tail
// when Ci % 32 == 16), and per chunk
//   * the tile's halo, (8 + 2 d) x (32 + 2 d) pixels with d = dil (KS / 2), is staged in LDS ONCE; the KS^2 taps read
//     shifted windows of it.  Pixels outside the image are written as zeros at staging time: the MFMA loop has no
//     branch and no zero page;
//   * the chunk's weights, KS^2 x chunk x (16 NJ) output channels, are staged in the order the MFMA reads them:
//     fragment (tap, j) is 64 consecutive 16-B units, unit `lane` = what that lane feeds the MFMA, so the fragment
//     read is one linear 1-KiB ds_read_b128 (conflict free by construction).
// v_mfma_f32_16x16x32 on a 32-channel chunk, v_mfma_f32_16x16x16 on the 16-channel tail; A = weights (rows = output
// channels), B = pixels, so a lane of the D layout holds 4 channels of one pixel per 16-channel block.
//
// Halo bank argument.  A pixel occupies C16_FWD_PITCH = 80 B of LDS (64 B of channels + 16 B of padding): 5 16-B
// units, an odd count.  A B-fragment read is a ds_read_b128 in which the 16 lanes fr = 0 .. 15 of one k group fq read
// unit fq of 16 CONSECUTIVE halo pixels: 16-B unit numbers 5 (p0 + fr) + fq.  5 is odd, so over any 16 (or 8)
// consecutive lanes these are distinct modulo 16 (modulo 8): each lane group of the read covers every bank exactly
// once.  A tap shift moves p0 by (kh dil) (32 + 2 d) + kw dil pixels, i.e. adds one constant to all 16 unit numbers,
// which rotates the banks and keeps them distinct: the argument holds at every tap and every dilation because it
// rests on the pitch, not on an XOR of low address bits that a shift would break.  The tail's 8-B reads (units fq of
// 8 B at the same pitch) fall in distinct 8-B slots the same way.
//
// Output channels: at most NJ = 4 blocks of 16 are accumulated per pass (16 f32x4 = 64 VGPRs: no scratch); wider Co
// loops passes inside the block.  With a single chunk (Ci <= 32) later passes re-read the halo from LDS; otherwise
// they re-stage it from L2.  The next (pass, chunk)'s global loads are issued into registers before the MFMAs of the
// current one and written to LDS after them (register prefetch, one LDS buffer, two barriers per chunk).
// Two neighbouring 16-channel blocks are interleaved at staging time (row rho of block j <-> channel
// 8 (rho / 4) + 4 (j & 1) + rho % 4 of the pair) so that a lane owns 8 consecutive channels and stores 16 B; a last
// odd block keeps the identity order and stores 8 B.  Epilogue: fp32 + bias, optional ReLU, one RNE to 16 bits;
// ragged tiles are masked at the store.
//
// wgrad_c16_kernel<DT, KS> + c16_reduce_kernel (conv_small_reduce.h): dW [Co][Ci][k][k] and db [Co] in fp32
// ------------------------------------------------------------------------------------------------------
// The GEMM reduces over pixels.  A block owns all KS^2 taps of a 32 x 32 (co x ci) block of dW and a slice of the
// pixel tiles: grid = (channel blocks, slices).  Wave (sco, sci) owns the 16 x 16 sub-block and all taps (9 f32x4).
// Per 8 x 32 pixel tile the block stages the dY tile and the x halo tile once, as they sit in memory
// ([pixel][channel], zeros outside the image and past the channel count); every tap reuses them.  A K step is one
// tile row of 32 pixels; both operands are read with the transposing ds_read_b64_tr_b16 (2 per fragment).
// Bank argument: the pitch is C16_WG_PITCH = 96 B = 3 x 32 B, and lane group g of a transposed read takes the 32-B
// channel runs of pixels 4 g .. 4 g + 3 (low half) and 16 + 4 g .. (high half; the k index of an MFMA step may name
// any 32 pixels as long as both operands agree).  Pixels p .. p + 7 start at 32-B units 3 p, ..., 3 p + 21, distinct
// modulo 8 (and any 4 consecutive ones modulo 4), so a half-wave (or quarter-wave) of the read covers every bank
// once; a tap shift adds a multiple of 96 B, a whole number of 32-B units, and keeps that.
// db is the column sum of the staged dY (one MFMA against ones per K step) in the blocks of input-channel block 0.
// Each slice writes one fp32 partial in the PyTorch layout; c16_reduce_kernel sums the slices in slice order
// (out = scale * sum + beta * out, beta = 0: overwrite).  No atomics: both kernels are bitwise repeatable.
#include "api.h"
#include "common.h"
#include "conv_epilogue.h"
#include "conv_small_plan.h"
#include "conv_small_dev.h"
#include "conv_small_reduce.h"

namespace can {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// forward / data gradient
// ---------------------------------------------------------------------------------------------------------------
struct C16Args {
  const bf16_t* x;       // [N][H][W][Ci]
  const bf16_t* w;       // [Co][KS^2 * Ci], k = tap * Ci + ci
  const float* bias;     // [Co] (EPI_BIAS_RELU / EPI_BIAS)
  bf16_t* y;             // [N][H][W][Co]
  int N, H, W, Ci, Co, dil, epi;
  int tx, ty;            // tiles along the width / height
};

template <int DT, int KS, int NJ>
__global__ void __launch_bounds__(256) conv_c16_kernel(C16Args a) {
  constexpr int T = KS * KS;
  constexpr int NU = (KS == 3) ? (c16_halo_pixels(C16_MAX_DIL) * 4 + 255) / 256 : (C16_TR * C16_TC * 4) / 256;
  constexpr int WU = (T * NJ + 3) / 4;                   // weight units per thread: T * NJ fragments of 64 units
  constexpr int P = C16_FWD_PITCH;
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
  const int co16 = a.Co >> 4, npass = (co16 + NJ - 1) / NJ;
  const int total = npass * nch;

  uint4 hreg[NU], wreg[WU];
  // global loads of iteration it = pass * nch + chunk (the halo only where it has to be staged)
  auto prefetch = [&](int it) {
    const int pass = it / nch, ch = it - pass * nch;
    const int cb = ch * 32, cw = min(32, a.Ci - cb);
    if (nch > 1 || pass == 0) halo_load<NU>(hreg, pix, a.x, a.Ci, cb, cw >> 3, tid);
    const int njl = min(NJ, co16 - pass * NJ);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int t = wave + 4 * i;                        // fragment (tap, j) of unit tid + 256 i
      const int tap = t / NJ, j = t - tap * NJ;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (t < T * NJ && j < njl) {
        const bf16_t* src = a.w + (size_t)(pass * NJ * 16 + c16_row_channel(j, fr, njl)) * K + tap * a.Ci + cb;
        if (cw == 32) v = *reinterpret_cast<const uint4*>(src + fq * 8);
        else { const uint2 h = *reinterpret_cast<const uint2*>(src + fq * 4); v.x = h.x; v.y = h.y; }
      }
      wreg[i] = v;
    }
  };
  auto stage = [&](int it) {
    const int pass = it / nch, ch = it - pass * nch;
    const bool tail = (a.Ci - ch * 32) < 32;
    if (nch > 1 || pass == 0) halo_store<NU, P>(hal, hreg, pix, tid);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int u = tid + 256 * i;
      if (u < T * NJ * 64) {
        if (!tail) *reinterpret_cast<uint4*>(wl + u * 16) = wreg[i];
        else *reinterpret_cast<uint2*>(wl + u * 8) = make_uint2(wreg[i].x, wreg[i].y);
      }
    }
  };

  f32x4 acc[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's B operand of fragment i at tap (kh, kw): halo pixel (2 wave + i / 2 + kh dil, 16 (i & 1) + fr + kw dil)
  const unsigned char* hb0 = hal + ((wave * 2) * HC + fr) * P;

  prefetch(0);
  for (int it = 0; it < total; ++it) {
    const int pass = it / nch, ch = it - pass * nch;
    const int njl = min(NJ, co16 - pass * NJ);
    const bool tail = (a.Ci - ch * 32) < 32;
    __syncthreads();                                     // the previous iteration's fragment reads are done
    stage(it);
    __syncthreads();
    if (it + 1 < total) prefetch(it + 1);                // in flight during the MFMAs below

    if (!tail) {
#pragma unroll
      for (int tap = 0; tap < T; ++tap) {
        const int kh = tap / KS, kw = tap - kh * KS;
        const unsigned char* hb = hb0 + ((kh * a.dil) * HC + kw * a.dil) * P + fq * 16;
        frag8_t bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          bf[i] = *reinterpret_cast<const frag8_t*>(hb + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const frag8_t af = *reinterpret_cast<const frag8_t*>(wl + ((tap * NJ + j) * 64 + lane) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = mfma16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    } else {
#pragma unroll
      for (int tap = 0; tap < T; ++tap) {
        const int kh = tap / KS, kw = tap - kh * KS;
        const unsigned char* hb = hb0 + ((kh * a.dil) * HC + kw * a.dil) * P + fq * 8;
        uint2 bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = *reinterpret_cast<const uint2*>(hb + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const uint2 af = *reinterpret_cast<const uint2*>(wl + ((tap * NJ + j) * 64 + lane) * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = mfma16k16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    }

    if (ch + 1 < nch) continue;
    // ---- epilogue of the pass: fragment i = pixel (r0 + 2 wave + i / 2, c0 + 16 (i & 1) + fr)
    const int cop = pass * NJ * 16;
#pragma unroll
    for (int jp = 0; jp < NJ; jp += 2) {
      const int j1 = (jp + 1 < NJ) ? jp + 1 : jp;        // static index of the pair's second block
      const bool paired = jp + 1 < njl;
      if (jp < njl) {
        const int cbase = cop + jp * 16 + (paired ? fq * 8 : fq * 4);
        float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.epi != EPI_NONE) {
          load_bias<4>(bv, a.bias + cbase);
          if (paired) load_bias<4>(bv + 4, a.bias + cbase + 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int oh = r0 + wave * 2 + (i >> 1), ow = c0 + (i & 1) * 16 + fr;
          float v[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) { v[r] = acc[jp][i][r]; v[4 + r] = acc[j1][i][r]; }
          if (a.epi == EPI_BIAS_RELU) bias_act<EPI_BIAS_RELU, 8>(v, bv, true);
          else if (a.epi == EPI_BIAS) bias_act<EPI_BIAS, 8>(v, bv, true);
          if (oh < a.H && ow < a.W) {
            bf16_t* dst = a.y + ((size_t)(n * a.H + oh) * a.W + ow) * a.Co + cbase;
            if (paired) *reinterpret_cast<uint4*>(dst) = pack8h<DT>(v);
            else *reinterpret_cast<uint2*>(dst) = make_uint2(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]));
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ---------------------------------------------------------------------------------------------------------------
// weight + bias gradient
// ---------------------------------------------------------------------------------------------------------------
struct C16WgArgs {
  const bf16_t* dy;      // [N][H][W][Co]
  const bf16_t* x;       // [N][H][W][Ci]
  float* ws;             // [S][Co * Ci * KS^2 + Co]
  int N, H, W, Ci, Co, dil;
  int tx, ty, total, tps;   // tiles along the width / height, tiles in all, tiles per slice
  int ncob;                 // 32-channel blocks of Co
  int want_db;
};

template <int DT, int KS>
__global__ void __launch_bounds__(256) wgrad_c16_kernel(C16WgArgs a) {
  constexpr int T = KS * KS;
  constexpr int NU = (KS == 3) ? (c16_halo_pixels(C16_MAX_DIL) * 4 + 255) / 256 : (C16_TR * C16_TC * 4) / 256;
  constexpr int ND = (C16_TR * C16_TC * 4) / 256;        // dY units per thread
  constexpr int P = C16_WG_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.dil * (KS / 2), HC = C16_TC + 2 * d, npix = (C16_TR + 2 * d) * HC;
  unsigned char* xh = smem;
  unsigned char* dyl = smem + npix * P;                  // 256 pixels x 96 B

  const int cob = blockIdx.x % a.ncob, cib = blockIdx.x / a.ncob, slice = blockIdx.y;
  const int co0 = cob * C16_WG_CB, ci0 = cib * C16_WG_CB;
  const int sco = wave & 1, sci = wave >> 1;
  const bool active = (co0 + 16 * sco < a.Co) && (ci0 + 16 * sci < a.Ci);
  const bool do_bias = a.want_db && cib == 0 && sci == 0 && active;
  const int nux = min(4, (a.Ci - ci0) >> 3), nud = min(4, (a.Co - co0) >> 3);   // valid 16-B channel units

  const int t0 = slice * a.tps, t1 = min(a.total, t0 + a.tps);

  int pix[NU], dpix[ND];
  uint4 hreg[NU], dreg[ND];
  auto prefetch = [&](int t) {
    int b = t;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    halo_pixels<NU>(pix, tid, n, tr * C16_TR, tc * C16_TC, d, HC, npix, a.H, a.W);
    halo_pixels<ND>(dpix, tid, n, tr * C16_TR, tc * C16_TC, 0, C16_TC, C16_TR * C16_TC, a.H, a.W);
    halo_load<NU>(hreg, pix, a.x, a.Ci, ci0, nux, tid);
    halo_load<ND>(dreg, dpix, a.dy, a.Co, co0, nud, tid);
  };

  f32x4 acc[T], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag8_t ones = ones_frag<DT>();

  // transposed reads: lane (g, q, p) addresses the 8-B run of channels 4 p .. 4 p + 3 of pixel 4 g + q (low half of
  // the lane's k values) and of pixel 16 + 4 g + q (high half)
  const int g = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
  const int plo = 4 * g + q;
  const unsigned char* dlo = dyl + plo * P + sco * 32 + p4 * 8;
  const unsigned char* xlo = xh + plo * P + sci * 32 + p4 * 8;

  if (t0 < t1) prefetch(t0);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    halo_store<NU, P>(xh, hreg, pix, tid);
    halo_store<ND, P>(dyl, dreg, dpix, tid);
    __syncthreads();
    if (t + 1 < t1) prefetch(t + 1);
    if (active) {
#pragma unroll 2
      for (int r = 0; r < C16_TR; ++r) {
        const unsigned char* da = dlo + r * C16_TC * P;
        const frag8_t af = c16_tr_read(da, da + 16 * P);
        if (do_bias) accb = mfma16<DT>(af, ones, accb);
#pragma unroll
        for (int tap = 0; tap < T; ++tap) {
          const int kh = tap / KS, kw = tap - kh * KS;
          const unsigned char* xa = xlo + ((r + kh * a.dil) * HC + kw * a.dil) * P;
          const frag8_t bf = c16_tr_read(xa, xa + 16 * P);
          acc[tap] = mfma16<DT>(af, bf, acc[tap]);
        }
      }
    }
  }

  // D layout: column lane & 15 = input channel, rows 4 (lane >> 4) + r = output channels
  if (active) {
    const int fr = lane & 15, fq = lane >> 4;
    const size_t plane = (size_t)a.Co * a.Ci * T;
    float* part = a.ws + (size_t)slice * (plane + a.Co);
    const int ci = ci0 + 16 * sci + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * sco + fq * 4 + r;
#pragma unroll
      for (int tap = 0; tap < T; ++tap) part[((size_t)co * a.Ci + ci) * T + tap] = acc[tap][r];
      if (do_bias && fr == 0) part[plane + co] = accb[r];
    }
  }
}

size_t c16_fwd_lds(int ksize, int dil, int nj) {
  const int d = dil * (ksize / 2);
  return (size_t)((c16_halo_pixels(d) * C16_FWD_PITCH + 15) & ~15) + (size_t)ksize * ksize * nj * 1024;
}
size_t c16_wg_lds(int ksize, int dil) {
  const int d = dil * (ksize / 2);
  return (size_t)(c16_halo_pixels(d) + C16_TR * C16_TC) * C16_WG_PITCH;
}

template <int DT, int KS, int NJ>
int launch_fwd(const C16Args& a, hipStream_t s) {
  auto kfn = conv_c16_kernel<DT, KS, NJ>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)c16_fwd_lds(KS, C16_MAX_DIL, NJ)));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3(a.N * a.ty * a.tx), dim3(256), c16_fwd_lds(KS, a.dil, NJ), s, a);
  return (int)hipGetLastError();
}
template <int DT, int KS>
int launch_fwd_nj(const C16Args& a, hipStream_t s) {
  switch (a.Co >> 4) {
    case 1: return launch_fwd<DT, KS, 1>(a, s);
    case 2: return launch_fwd<DT, KS, 2>(a, s);
    case 3: return launch_fwd<DT, KS, 3>(a, s);
    default: return launch_fwd<DT, KS, C16_NJ>(a, s);
  }
}
template <int DT>
int launch_fwd_ks(const C16Args& a, int ksize, hipStream_t s) {
  return ksize == 3 ? launch_fwd_nj<DT, 3>(a, s) : launch_fwd_nj<DT, 1>(a, s);
}

template <int DT, int KS>
int launch_wg(const C16WgArgs& a, int S, hipStream_t s) {
  auto kfn = wgrad_c16_kernel<DT, KS>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)c16_wg_lds(KS, C16_MAX_DIL)));
    attr = true;
  }
  const int ncb = a.ncob * c16_cdiv(a.Ci, C16_WG_CB);
  hipLaunchKernelGGL(kfn, dim3(ncb, S), dim3(256), c16_wg_lds(KS, a.dil), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_wg_ks(const C16WgArgs& a, int ksize, int S, hipStream_t s) {
  return ksize == 3 ? launch_wg<DT, 3>(a, S, s) : launch_wg<DT, 1>(a, S, s);
}

// what both entry points refuse before any launch
int c16_check(int N, int H, int W, int Ci, int Co, int ksize, int dil) {
  if (N < 1 || H < 1 || W < 1 || Ci < 16 || Co < 16 || (Ci & 15) || (Co & 15) || (ksize != 1 && ksize != 3))
    return C16_ERR_SHAPE;
  if (dil < 1 || dil > C16_MAX_DIL) return C16_ERR_DIL;
  if ((long long)N * H * W * (Ci > Co ? Ci : Co) >= (1LL << 30)) return C16_ERR_ELEMS;   // 32-bit pixel offsets
  return 0;
}

}  // namespace
}  // namespace can

extern "C" int can_conv_small(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Ci,
                              int Co, int ksize, int dil, int epi, int dt, void* stream) {
  using namespace can;
  if (ksize > 3) return can_conv_large(x, w, bias, y, N, H, W, Ci, Co, ksize, dil, epi, dt, stream);   // conv_large.hip
  const int rc = c16_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  if (epi != EPI_BIAS_RELU && epi != EPI_BIAS && epi != EPI_NONE) return C16_ERR_SHAPE;
  if (epi != EPI_NONE && bias == nullptr) return C16_ERR_SHAPE;
  C16Args a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = (bf16_t*)y;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.dil = dil; a.epi = epi;
  a.tx = c16_cdiv(W, C16_TC); a.ty = c16_cdiv(H, C16_TR);
  CAN_DT_DISPATCH(dt, launch_fwd_ks<DT>(a, ksize, (hipStream_t)stream));
}

extern "C" int can_conv_small_slices(long long M, int Ci, int Co) {
  return can::c16_wgrad_slices(M, Ci, Co, can_device_cus());
}

extern "C" int can_conv_small_wgrad(const void* dy, const void* x, float* ws, long long ws_floats, float* dw, float* db,
                                    int N, int H, int W, int Ci, int Co, int ksize, int dil, float beta, float scale,
                                    int dt, void* stream) {
  using namespace can;
  if (ksize > 3)
    return can_conv_large_wgrad(dy, x, ws, ws_floats, dw, db, N, H, W, Ci, Co, ksize, dil, beta, scale, dt, stream);
  const int rc = c16_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  const int S = c16_wgrad_slices((long long)N * H * W, Ci, Co, can_device_cus());
  if (c16_wgrad_ws_floats(S, Ci, Co, ksize) > ws_floats) return C16_ERR_WS;
  C16WgArgs a;
  a.dy = (const bf16_t*)dy; a.x = (const bf16_t*)x; a.ws = ws;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.dil = dil;
  a.tx = c16_cdiv(W, C16_TC); a.ty = c16_cdiv(H, C16_TR); a.total = N * a.tx * a.ty;
  a.tps = c16_cdiv(a.total, S);
  a.ncob = c16_cdiv(Co, C16_WG_CB);
  a.want_db = db != nullptr;
  hipStream_t s = (hipStream_t)stream;
  int lrc = -20;
  if (dt == DT_F16) lrc = launch_wg_ks<DT_F16>(a, ksize, S, s);
  else if (dt == DT_BF16) lrc = launch_wg_ks<DT_BF16>(a, ksize, S, s);
  if (lrc) return lrc;
  return c16_reduce(ws, dw, db, S, Co * Ci * ksize * ksize, Co, beta, scale, s);
}
