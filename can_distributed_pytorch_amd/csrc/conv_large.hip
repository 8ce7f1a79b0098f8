// Large-kernel NHWC convolutions (gfx950): 5x5 (dilation 1 - 2) and 7x7 (dilation 1) layers on Ci, Co multiples of 16,
// the layers of multi-column and scale-aggregation counting networks.  The pixel tile, the halo staging and the LDS
// pitches are those of conv_small.hip; its kernels cannot be instantiated at these sizes (all KS^2 NJ weight fragments
// of a chunk in LDS: 196 KiB at 7x7; all KS^2 weight-gradient accumulators in registers: 196 VGPRs), so here the weights
// and the taps move one TAP ROW at a time.
//
// conv_l16_kernel<DT, KS, NJ>: forward, and the data gradient through the flipped / transposed weight pack
// ------------------------------------------------------------------------------------------------------
// As conv_c16_kernel: a block of 4 waves owns an 8 x 32 pixel tile, a wave 2 rows = four 16-pixel fragments; the input
// channels go by in 32-channel chunks (v_mfma_f32_16x16x32) plus a 16-channel tail (16x16x16); at most NJ = 4 output
// blocks of 16 channels per pass (64 accumulator VGPRs); the chunk's halo, (8 + 2 d) x (32 + 2 d) pixels with
// d = dil (KS / 2) <= 4, is staged ONCE per chunk at the 80-byte pitch, pixels outside the image as zeros.
// New: the unit of the pipeline is a step = (pass, chunk, tap row kh).  The weights of a step are KS NJ ready-made
// 1-KiB MFMA fragments (fragment (kw, j): unit `lane` = what that lane feeds the MFMA, one linear ds_read_b128) in one
// of TWO row buffers, step g in buffer g & 1.  The global loads of step g + 1 (row kh + 1, or row 0 of the next chunk
// or pass together with that chunk's halo) are issued into registers before the MFMAs of step g and written to LDS
// at the top of step g + 1, into the buffer that step g - 1 read: every wave has passed step g's barrier after its
// last read of it, so ONE barrier per step orders the weights.  The single halo buffer takes a second barrier, only
// at the first row of a chunk that re-stages it (with one chunk, Ci <= 32, later passes re-read the halo in LDS).
// The kh loop is a run-time loop (the step loop itself); the KS taps of a row are unrolled.
// Worst case, 7x7, NJ = 4, d = 3: halo 14 x 38 x 80 B = 41.6 KiB, weights 2 x 28 KiB, 7 uint4 of weight prefetch and
// 9 of halo prefetch per thread.
//
// Halo bank argument (conv_small.hip) at the larger shifts.  A pixel is 5 16-B units, an odd count, so the 16 lanes
// of one k group, which read unit fq of 16 consecutive halo pixels, hit unit numbers 5 (p0 + fr) + fq: distinct
// modulo 16 and modulo 8 whatever p0 is.  Tap (kh, kw) moves p0 by (kh dil) (32 + 2 d) + kw dil pixels, up to
// 6 x 38 + 6 at 7x7 and 8 x 40 + 8 at 5x5 dilation 2: a constant added to all 16 unit numbers, a rotation of the
// banks.  Nothing in the argument depends on the size of the shift; the tail's 8-B reads follow the same way.
//
// Epilogue: conv_c16_kernel's (pairs of blocks interleaved at staging time so that a lane stores 16 B, a last odd block
// 8 B; fp32 + bias, optional ReLU, one RNE; ragged tiles masked at the store).
//
// wgrad_l16_kernel<DT, KS> + c16_reduce_kernel (conv_small_reduce.h): dW [Co][Ci][k][k] and db [Co] in fp32
// ------------------------------------------------------------------------------------------------------
// grid = (32 x 32 channel blocks, tap rows, pixel slices).  Wave (sco, sci) owns a 16 x 16 sub-block and the KS taps of
// the block's row kh: KS f32x4 accumulators.  Per 8 x 32 pixel tile the block stages the dY tile and only the
// 8 x (32 + 2 d) strip of x its row reads, rows r0 + (kh - KS / 2) dil ..., both at the 96-byte pitch as they sit in
// memory, and reads them with ds_read_b64_tr_b16 (bank argument of conv_small.hip: a tap shift adds kw dil pixels of
// 96 B, whole 32-B units).  db comes from the blocks of input-channel block 0 and tap row 0.  Each slice writes its
// fp32 partial in the PyTorch layout; the tap rows multiply the grid, not the partials, so the slice count and the
// workspace are conv_small's.  No atomics: bitwise repeatable.
#include "api.h"
#include "common.h"
#include "conv_epilogue.h"
#include "conv_large_plan.h"
#include "conv_small_dev.h"
#include "conv_small_reduce.h"

namespace can {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// forward / data gradient
// ---------------------------------------------------------------------------------------------------------------
struct L16Args {
  const bf16_t* x;       // [N][H][W][Ci]
  const bf16_t* w;       // [Co][KS^2 * Ci], k = tap * Ci + ci
  const float* bias;     // [Co] (EPI_BIAS_RELU / EPI_BIAS)
  bf16_t* y;             // [N][H][W][Co]
  int N, H, W, Ci, Co, dil, epi;
  int tx, ty;            // tiles along the width / height
};

template <int DT, int KS, int NJ>
__global__ void __launch_bounds__(256) conv_l16_kernel(L16Args a) {
  constexpr int NU = (c16_halo_pixels(l16_max_reach(KS)) * 4 + 255) / 256;
  constexpr int RF = KS * NJ;                            // fragments of a tap row
  constexpr int WU = (RF + 3) / 4;                       // weight units per thread and row
  constexpr int P = C16_FWD_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int d = a.dil * (KS / 2), HC = C16_TC + 2 * d, npix = (C16_TR + 2 * d) * HC;
  unsigned char* hal = smem;
  unsigned char* wl0 = smem + ((npix * P + 15) & ~15);   // two row buffers of RF KiB

  int b = blockIdx.x;
  const int tc = b % a.tx; b /= a.tx;
  const int tr = b % a.ty;
  const int n = b / a.ty;
  const int r0 = tr * C16_TR, c0 = tc * C16_TC;

  int pix[NU];
  halo_pixels<NU>(pix, tid, n, r0, c0, d, HC, npix, a.H, a.W);

  const int K = KS * KS * a.Ci;
  const int nch = (a.Ci + 31) >> 5;                      // chunks: Ci / 32 full ones + the 16-channel tail
  const int co16 = a.Co >> 4, npass = (co16 + NJ - 1) / NJ;
  const int steps = npass * nch * KS;

  uint4 hreg[NU], wreg[WU];
  // global loads of step (pass, ch, kh): tap row kh of the chunk's weights, and the halo where a chunk begins
  auto prefetch = [&](int pass, int ch, int kh) {
    const int cb = ch * 32, cw = min(32, a.Ci - cb);
    if (kh == 0 && (nch > 1 || pass == 0)) halo_load<NU>(hreg, pix, a.x, a.Ci, cb, cw >> 3, tid);
    const int njl = min(NJ, co16 - pass * NJ);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int t = wave + 4 * i;                        // fragment (kw, j) of unit tid + 256 i
      const int kw = t / NJ, j = t - kw * NJ;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (t < RF && j < njl) {
        const bf16_t* src =
            a.w + (size_t)(pass * NJ * 16 + c16_row_channel(j, fr, njl)) * K + (kh * KS + kw) * a.Ci + cb;
        if (cw == 32) v = *reinterpret_cast<const uint4*>(src + fq * 8);
        else { const uint2 h = *reinterpret_cast<const uint2*>(src + fq * 4); v.x = h.x; v.y = h.y; }
      }
      wreg[i] = v;
    }
  };

  f32x4 acc[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's B operand of fragment i at tap (kh, kw): halo pixel (2 wave + i / 2 + kh dil, 16 (i & 1) + fr + kw dil)
  const unsigned char* hb0 = hal + ((wave * 2) * HC + fr) * P;

  int pass = 0, ch = 0, kh = 0;
  prefetch(0, 0, 0);
  for (int g = 0; g < steps; ++g) {
    const int njl = min(NJ, co16 - pass * NJ);
    const bool tail = (a.Ci - ch * 32) < 32;
    unsigned char* wl = wl0 + (g & 1) * (RF * 1024);
    if (kh == 0 && (nch > 1 || pass == 0)) {
      __syncthreads();                                   // the previous chunk's halo reads are done
      halo_store<NU, P>(hal, hreg, pix, tid);
    }
#pragma unroll
    for (int i = 0; i < WU; ++i) {                       // this buffer was last read two steps ago
      const int u = tid + 256 * i;
      if (u < RF * 64) {
        if (!tail) *reinterpret_cast<uint4*>(wl + u * 16) = wreg[i];
        else *reinterpret_cast<uint2*>(wl + u * 8) = make_uint2(wreg[i].x, wreg[i].y);
      }
    }
    __syncthreads();
    int npass_ = pass, nchunk = ch, nkh = kh + 1;        // the next step
    if (nkh == KS) {
      nkh = 0;
      if (++nchunk == nch) { nchunk = 0; ++npass_; }
    }
    if (g + 1 < steps) prefetch(npass_, nchunk, nkh);    // in flight during the MFMAs below

    const unsigned char* hrow = hb0 + (kh * a.dil * HC) * P;
    if (!tail) {
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const unsigned char* hb = hrow + (kw * a.dil) * P + fq * 16;
        frag8_t bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          bf[i] = *reinterpret_cast<const frag8_t*>(hb + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const frag8_t af = *reinterpret_cast<const frag8_t*>(wl + ((kw * NJ + j) * 64 + lane) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = mfma16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    } else {
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const unsigned char* hb = hrow + (kw * a.dil) * P + fq * 8;
        uint2 bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = *reinterpret_cast<const uint2*>(hb + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const uint2 af = *reinterpret_cast<const uint2*>(wl + ((kw * NJ + j) * 64 + lane) * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = mfma16k16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    }

    if (kh == KS - 1 && ch + 1 == nch) {
      // ---- epilogue of the pass: fragment i = pixel (r0 + 2 wave + i / 2, c0 + 16 (i & 1) + fr)
      const int cop = pass * NJ * 16;
#pragma unroll
      for (int jp = 0; jp < NJ; jp += 2) {
        const int j1 = (jp + 1 < NJ) ? jp + 1 : jp;      // static index of the pair's second block
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
    pass = npass_; ch = nchunk; kh = nkh;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// weight + bias gradient
// ---------------------------------------------------------------------------------------------------------------
struct L16WgArgs {
  const bf16_t* dy;      // [N][H][W][Co]
  const bf16_t* x;       // [N][H][W][Ci]
  float* ws;             // [S][Co * Ci * KS^2 + Co]
  int N, H, W, Ci, Co, dil;
  int tx, ty, total, tps;   // tiles along the width / height, tiles in all, tiles per slice
  int ncob;                 // 32-channel blocks of Co
  int want_db;
};

template <int DT, int KS>
__global__ void __launch_bounds__(256) wgrad_l16_kernel(L16WgArgs a) {
  constexpr int NU = (l16_strip_pixels(l16_max_reach(KS)) * 4 + 255) / 256;   // x units per thread
  constexpr int ND = (C16_TR * C16_TC * 4) / 256;                             // dY units per thread
  constexpr int P = C16_WG_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.dil * (KS / 2), HC = C16_TC + 2 * d, npix = C16_TR * HC;
  unsigned char* xh = smem;                              // the strip: 8 rows x HC pixels x 96 B
  unsigned char* dyl = smem + npix * P;                  // 256 pixels x 96 B

  const int cob = blockIdx.x % a.ncob, cib = blockIdx.x / a.ncob, kh = blockIdx.y, slice = blockIdx.z;
  const int co0 = cob * C16_WG_CB, ci0 = cib * C16_WG_CB;
  const int sco = wave & 1, sci = wave >> 1;
  const bool active = (co0 + 16 * sco < a.Co) && (ci0 + 16 * sci < a.Ci);
  const bool do_bias = a.want_db && cib == 0 && kh == 0 && sci == 0 && active;
  const int nux = min(4, (a.Ci - ci0) >> 3), nud = min(4, (a.Co - co0) >> 3);   // valid 16-B channel units

  const int t0 = slice * a.tps, t1 = min(a.total, t0 + a.tps);

  int pix[NU], dpix[ND];
  uint4 hreg[NU], dreg[ND];
  auto prefetch = [&](int t) {
    int b = t;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    // strip row hr is image row r0 + (kh - KS / 2) dil + hr = (r0 + kh dil) - d + hr
    halo_pixels<NU>(pix, tid, n, tr * C16_TR + kh * a.dil, tc * C16_TC, d, HC, npix, a.H, a.W);
    halo_pixels<ND>(dpix, tid, n, tr * C16_TR, tc * C16_TC, 0, C16_TC, C16_TR * C16_TC, a.H, a.W);
    halo_load<NU>(hreg, pix, a.x, a.Ci, ci0, nux, tid);
    halo_load<ND>(dreg, dpix, a.dy, a.Co, co0, nud, tid);
  };

  f32x4 acc[KS], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) acc[kw] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag8_t ones = ones_frag<DT>();

  // transposed reads (conv_small.hip): lane (g, q, p) addresses the 8-B run of channels 4 p .. 4 p + 3 of pixel
  // 4 g + q (low half of the lane's k values) and of pixel 16 + 4 g + q (high half)
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
        for (int kw = 0; kw < KS; ++kw) {
          const unsigned char* xa = xlo + (r * HC + kw * a.dil) * P;
          const frag8_t bf = c16_tr_read(xa, xa + 16 * P);
          acc[kw] = mfma16<DT>(af, bf, acc[kw]);
        }
      }
    }
  }

  // D layout: column lane & 15 = input channel, rows 4 (lane >> 4) + r = output channels
  if (active) {
    const int fr = lane & 15, fq = lane >> 4;
    const size_t plane = (size_t)a.Co * a.Ci * (KS * KS);
    float* part = a.ws + (size_t)slice * (plane + a.Co);
    const int ci = ci0 + 16 * sci + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * sco + fq * 4 + r;
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) part[((size_t)co * a.Ci + ci) * (KS * KS) + kh * KS + kw] = acc[kw][r];
      if (do_bias && fr == 0) part[plane + co] = accb[r];
    }
  }
}

template <int DT, int KS, int NJ>
int launch_fwd(const L16Args& a, hipStream_t s) {
  auto kfn = conv_l16_kernel<DT, KS, NJ>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)l16_fwd_lds(KS, l16_max_dil(KS), NJ)));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3(a.N * a.ty * a.tx), dim3(256), l16_fwd_lds(KS, a.dil, NJ), s, a);
  return (int)hipGetLastError();
}
template <int DT, int KS>
int launch_fwd_nj(const L16Args& a, hipStream_t s) {
  switch (a.Co >> 4) {
    case 1: return launch_fwd<DT, KS, 1>(a, s);
    case 2: return launch_fwd<DT, KS, 2>(a, s);
    case 3: return launch_fwd<DT, KS, 3>(a, s);
    default: return launch_fwd<DT, KS, C16_NJ>(a, s);
  }
}
template <int DT>
int launch_fwd_ks(const L16Args& a, int ksize, hipStream_t s) {
  return ksize == 7 ? launch_fwd_nj<DT, 7>(a, s) : launch_fwd_nj<DT, 5>(a, s);
}

template <int DT, int KS>
int launch_wg(const L16WgArgs& a, int S, hipStream_t s) {
  auto kfn = wgrad_l16_kernel<DT, KS>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)l16_wg_lds(KS, l16_max_dil(KS))));
    attr = true;
  }
  const int ncb = a.ncob * c16_cdiv(a.Ci, C16_WG_CB);
  hipLaunchKernelGGL(kfn, dim3(ncb, KS, S), dim3(256), l16_wg_lds(KS, a.dil), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_wg_ks(const L16WgArgs& a, int ksize, int S, hipStream_t s) {
  return ksize == 7 ? launch_wg<DT, 7>(a, S, s) : launch_wg<DT, 5>(a, S, s);
}

}  // namespace
}  // namespace can

extern "C" int can_conv_large(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Ci,
                              int Co, int ksize, int dil, int epi, int dt, void* stream) {
  using namespace can;
  const int rc = l16_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  if (epi != EPI_BIAS_RELU && epi != EPI_BIAS && epi != EPI_NONE) return C16_ERR_SHAPE;
  if (epi != EPI_NONE && bias == nullptr) return C16_ERR_SHAPE;
  L16Args a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = (bf16_t*)y;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.dil = dil; a.epi = epi;
  a.tx = c16_cdiv(W, C16_TC); a.ty = c16_cdiv(H, C16_TR);
  CAN_DT_DISPATCH(dt, launch_fwd_ks<DT>(a, ksize, (hipStream_t)stream));
}

extern "C" int can_conv_large_wgrad(const void* dy, const void* x, float* ws, long long ws_floats, float* dw, float* db,
                                    int N, int H, int W, int Ci, int Co, int ksize, int dil, float beta, float scale,
                                    int dt, void* stream) {
  using namespace can;
  const int rc = l16_check(N, H, W, Ci, Co, ksize, dil);
  if (rc) return rc;
  const int S = c16_wgrad_slices((long long)N * H * W, Ci, Co, can_device_cus());
  if (c16_wgrad_ws_floats(S, Ci, Co, ksize) > ws_floats) return C16_ERR_WS;
  L16WgArgs a;
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
