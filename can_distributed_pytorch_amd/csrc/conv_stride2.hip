// Stride-2 NHWC convolutions (gfx950): the down-sampling conv y[o] = sum x[2 o - p + (kh, kw)] w[:, :, kh, kw] and its
// adjoint, the 2x transposed conv (input pixel i adds to output pixel 2 i - p + (kh, kw)), ksize 1 .. 4,
// p = (ksize - 1) / 2, Ci and Co any multiples of 16, a large map of even H x W and a small map of H/2 x W/2.  Each of
// the two data-path kernels is one layer's forward and the other's data gradient; one weight-gradient kernel serves
// both.  Channels go by in 32-channel chunks (v_mfma_f32_16x16x32) plus a 16-channel tail (16x16x16), A = weights
// (rows = output channels), B = pixels, at most NJ = 4 output blocks of 16 channels per pass, the epilogue of
// conv_small.hip (pairs of blocks interleaved at staging time: a lane stores 16 B; bias, optional ReLU, one RNE).
//
// conv_d2_kernel<DT, NJ>: the gather at stride 2 (down forward, up's data gradient)
// ------------------------------------------------------------------------------------------------------
// A block of 4 waves owns 4 rows x 32 columns of the SMALL map, a wave one row = two 16-pixel fragments.  The tile's
// window of the large map, (6 + k) rows x (62 + k) columns, is staged once per chunk at the 80-byte pitch, SPLIT BY
// COLUMN PARITY: window column wc = 2 c + kw lies in plane wc & 1 at column wc >> 1, layout [row][plane][32 or 33].
// Bank argument.  At pixel stride 2 in one array the 16 lanes of a k group would read 16-B units 10 lane + const: only
// 8 distinct values modulo 16, a two-way conflict.  In the split layout tap kw reads the 16 CONSECUTIVE pixels
// c + (kw >> 1) of plane kw & 1: units 5 (p0 + lane) + fq, 5 odd, distinct modulo 16 (and 8); a tap moves p0 by a
// constant, a rotation of the banks, so the pitch argument of conv_small.hip holds at every tap.  Rows need no split:
// a row only adds a constant.  ksize 1 reads even rows of the even plane only; the rest is not staged.
// The weights go by one tap row at a time in two row buffers, the step pipeline of conv_large.hip (step = (pass,
// chunk, kh); the loads of step g + 1 are in registers during the MFMAs of step g; one barrier per step, a second one
// where a chunk re-stages the window).  ksize is a run-time argument: the kw loop is a run-time loop over ready-made
// 1-KiB fragments, the accumulators are indexed statically.
// LDS: window 10 x 66 x 80 B = 52.8 KB at k = 4 (47.5 KB at k = 3, 41 KB at k <= 2) + 2 k NJ KiB of weights: 84.8 KB
// at k = 4, 71.5 KB at k = 3 (two blocks per CU), 57 KB at k = 2.
//
// conv_u2_kernel<DT, NJ>: the four parity classes (up forward, down's data gradient)
// ------------------------------------------------------------------------------------------------------
// No scatter and no inserted zeros: output pixel (2 i + a, 2 j + b) of class (a, b) is a stride-1 conv of the small
// map with the taps kh = (a + p) & 1, + 2, ... < k, each reading the small map at row offset (a + p - kh) / 2 in
// {-1, 0, 1} (columns alike): 1 tap at k = 2, 2 x 2 at k = 4, 1 / 2 / 2 / 4 at k = 3, and at k = 1 three classes
// without a tap (bias only).  A block owns an 8 x 32 tile of the small map (a wave 2 rows = four fragments, halo reach
// 1 pixel from k = 3 on, the 80-byte pitch and bank argument of conv_small.hip) and writes the 16 x 64 output tile.
// The classes are looped with the accumulators of ONE class live (64 VGPRs): iteration = (pass, class, chunk), the
// class's at most 4 NJ weight fragments staged per iteration, the halo once when Ci <= 32 and per iteration
// otherwise (L2 serves the re-reads).  Stores are strided by one pixel, each a contiguous 16 B (8 B for a last odd
// block) of a pixel's Co run; a block writes both column classes, so lines complete in L2.
// LDS: halo 10 x 34 x 80 B = 27.2 KB (20.5 KB at k <= 2) + 4 NJ KiB: 43.2 KB at most.
//
// s2_wgrad_kernel<DT, KS> + c16_reduce_kernel: dw[a][b][kh][kw] = sum small[n, i, j, a] big[n, 2 i - p + kh, 2 j - p + kw, b]
// ------------------------------------------------------------------------------------------------------
// down: small = dY, big = x -> [Co][Ci][k][k]; up: small = x, big = dY -> [Ci][Co][k][k], the transposed layout
// directly.  grid = (32 x 32 channel blocks, pixel slices); wave (sa, sb) owns a 16 x 16 sub-block and all KS^2 taps.
// Per 4 x 32 tile of the small map the block stages the tile and the parity-split window of the large map (as above)
// at the 96-byte pitch, as they sit in memory, and reads both with ds_read_b64_tr_b16; a K step is one tile row of 32
// small pixels, whose 32 large-map pixels of tap kw are consecutive in one plane (bank argument of conv_small.hip: a
// tap adds whole 96-byte pixels).  db is one extra MFMA against ones per K step: of the small tile (down: dY is the
// small map), or of the window at the taps kh - p, kw - p in {0, 1}, which visit every large-map pixel exactly once
// (up: dY is the large map; ksize 1 has no such taps and runs on the KS = 2 geometry, storing tap (0, 0) only).
// Slices, workspace and the slice-ordered reduce are conv_small's, counted over the small map's pixels.  No atomics.
// LDS: (10 x 66 + 128) x 96 B = 75.6 KB at k = 4, 69.3 KB at k = 3.
#include "api.h"
#include "common.h"
#include "conv_epilogue.h"
#include "conv_stride2_plan.h"
#include "conv_small_dev.h"
#include "conv_small_reduce.h"

namespace can {
namespace {

// Window staging, shared by the gather and the weight gradient: unit u = tid + 256 i is 16-B channel unit u & 3 of
// window pixel u >> 2 in the order [row][plane][column] (conv_stride2_plan.h); (r0, c0) the tile's origin in the small
// map, H x W the large map.  pix[] as halo_pixels': -1 outside the image (zeros), -2 not staged.
template <int NU>
__device__ __forceinline__ void s2_window_pixels(int (&pix)[NU], int tid, int n, int r0, int c0, int ksize, int H,
                                                 int W) {
  const int p = s2_pad(ksize), PW = s2_plane_cols(ksize), npix = s2_win_pixels(ksize);
  const unsigned inv = 65536u / (unsigned)(2 * PW) + 1u;   // hp / (2 PW) == (hp * inv) >> 16 for hp < 1024, 2 PW = 64, 66
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int hp = (tid + 256 * i) >> 2;
    const int wr = (int)(((unsigned)hp * inv) >> 16), rem = hp - wr * 2 * PW;
    const int plane = rem >= PW ? 1 : 0, pc = rem - plane * PW;
    const int ih = 2 * r0 - p + wr, iw = 2 * c0 - p + 2 * pc + plane;
    const bool in = ih >= 0 && ih < H && iw >= 0 && iw < W;
    const bool used = ksize > 1 || (!(wr & 1) && !plane);
    pix[i] = (hp >= npix || !used) ? -2 : (in ? (n * H + ih) * W + iw : -1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the gather: down forward / up data gradient
// ---------------------------------------------------------------------------------------------------------------
struct D2Args {
  const bf16_t* x;       // [N][H][W][Ci], the large map
  const bf16_t* w;       // [Co][ks^2 * Ci], k = tap * Ci + ci
  const float* bias;     // [Co] (EPI_BIAS_RELU / EPI_BIAS)
  bf16_t* y;             // [N][H/2][W/2][Co]
  int N, H, W, Ci, Co, ks, epi;
  int tx, ty;            // tiles along the small map's width / height
};

template <int DT, int NJ>
__global__ void __launch_bounds__(256) conv_d2_kernel(D2Args a) {
  constexpr int NU = (s2_win_pixels(S2_MAX_K) * 4 + 255) / 256;
  constexpr int WU = (S2_MAX_K * NJ + 3) / 4;            // weight units per thread and tap row
  constexpr int P = C16_FWD_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int ks = a.ks, PW = s2_plane_cols(ks), RF = ks * NJ;   // RF: fragments of a tap row
  const int Ho = a.H >> 1, Wo = a.W >> 1;
  unsigned char* hal = smem;
  unsigned char* wl0 = smem + ((s2_win_pixels(ks) * P + 15) & ~15);   // two row buffers of RF KiB

  int b = blockIdx.x;
  const int tc = b % a.tx; b /= a.tx;
  const int tr = b % a.ty;
  const int n = b / a.ty;
  const int r0 = tr * S2_TR, c0 = tc * S2_TC;

  int pix[NU];
  s2_window_pixels<NU>(pix, tid, n, r0, c0, ks, a.H, a.W);

  const int K = ks * ks * a.Ci;
  const int nch = (a.Ci + 31) >> 5;                      // chunks: Ci / 32 full ones + the 16-channel tail
  const int co16 = a.Co >> 4, npass = (co16 + NJ - 1) / NJ;
  const int steps = npass * nch * ks;

  uint4 hreg[NU], wreg[WU];
  // global loads of step (pass, ch, kh): tap row kh of the chunk's weights, and the window where a chunk begins
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
            a.w + (size_t)(pass * NJ * 16 + c16_row_channel(j, fr, njl)) * K + (kh * ks + kw) * a.Ci + cb;
        if (cw == 32) v = *reinterpret_cast<const uint4*>(src + fq * 8);
        else { const uint2 h = *reinterpret_cast<const uint2*>(src + fq * 4); v.x = h.x; v.y = h.y; }
      }
      wreg[i] = v;
    }
  };

  f32x4 acc[NJ][2];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's B operand of fragment i at tap (kh, kw): window row 2 wave + kh, plane kw & 1, column 16 i + fr + (kw >> 1)
  const unsigned char* hb0 = hal + ((wave * 4) * PW + fr) * P;

  int pass = 0, ch = 0, kh = 0;
  prefetch(0, 0, 0);
  for (int g = 0; g < steps; ++g) {
    const int njl = min(NJ, co16 - pass * NJ);
    const bool tail = (a.Ci - ch * 32) < 32;
    unsigned char* wl = wl0 + (g & 1) * (RF * 1024);
    if (kh == 0 && (nch > 1 || pass == 0)) {
      __syncthreads();                                   // the previous chunk's window reads are done
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
    if (nkh == ks) {
      nkh = 0;
      if (++nchunk == nch) { nchunk = 0; ++npass_; }
    }
    if (g + 1 < steps) prefetch(npass_, nchunk, nkh);    // in flight during the MFMAs below

    const unsigned char* hrow = hb0 + (kh * 2 * PW) * P;
    if (!tail) {
      for (int kw = 0; kw < ks; ++kw) {
        const unsigned char* hb = hrow + ((kw & 1) * PW + (kw >> 1)) * P + fq * 16;
        frag8_t bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) bf[i] = *reinterpret_cast<const frag8_t*>(hb + i * 16 * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const frag8_t af = *reinterpret_cast<const frag8_t*>(wl + ((kw * NJ + j) * 64 + lane) * 16);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = mfma16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    } else {
      for (int kw = 0; kw < ks; ++kw) {
        const unsigned char* hb = hrow + ((kw & 1) * PW + (kw >> 1)) * P + fq * 8;
        uint2 bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) bf[i] = *reinterpret_cast<const uint2*>(hb + i * 16 * P);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < njl) {
            const uint2 af = *reinterpret_cast<const uint2*>(wl + ((kw * NJ + j) * 64 + lane) * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = mfma16k16<DT>(af, bf[i], acc[j][i]);
          }
        }
      }
    }

    if (kh == ks - 1 && ch + 1 == nch) {
      // ---- epilogue of the pass: fragment i = small-map pixel (r0 + wave, c0 + 16 i + fr)
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
          for (int i = 0; i < 2; ++i) {
            const int oh = r0 + wave, ow = c0 + i * 16 + fr;
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = acc[jp][i][r]; v[4 + r] = acc[j1][i][r]; }
            if (a.epi == EPI_BIAS_RELU) bias_act<EPI_BIAS_RELU, 8>(v, bv, true);
            else if (a.epi == EPI_BIAS) bias_act<EPI_BIAS, 8>(v, bv, true);
            if (oh < Ho && ow < Wo) {
              bf16_t* dst = a.y + ((size_t)(n * Ho + oh) * Wo + ow) * a.Co + cbase;
              if (paired) *reinterpret_cast<uint4*>(dst) = pack8h<DT>(v);
              else *reinterpret_cast<uint2*>(dst) = make_uint2(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]));
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    pass = npass_; ch = nchunk; kh = nkh;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the parity classes: up forward / down data gradient
// ---------------------------------------------------------------------------------------------------------------
struct U2Args {
  const bf16_t* x;       // [N][H][W][Ci], the small map
  const bf16_t* w;       // [Co][ks^2 * Ci], k = tap * Ci + ci, not flipped
  const float* bias;     // [Co] (EPI_BIAS_RELU / EPI_BIAS)
  bf16_t* y;             // [N][2 H][2 W][Co]
  int N, H, W, Ci, Co, ks, epi;
  int tx, ty;            // tiles along the small map's width / height
};

template <int DT, int NJ>
__global__ void __launch_bounds__(256) conv_u2_kernel(U2Args a) {
  constexpr int NU = (c16_halo_pixels(1) * 4 + 255) / 256;
  constexpr int WU = NJ;                                 // 4 NJ fragments of a class over 4 waves
  constexpr int P = C16_FWD_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int ks = a.ks, pad = s2_pad(ks);
  const int d = s2_up_reach(ks), HC = C16_TC + 2 * d, npix = (C16_TR + 2 * d) * HC;
  unsigned char* hal = smem;
  unsigned char* wl = smem + ((npix * P + 15) & ~15);

  int b = blockIdx.x;
  const int tc = b % a.tx; b /= a.tx;
  const int tr = b % a.ty;
  const int n = b / a.ty;
  const int r0 = tr * C16_TR, c0 = tc * C16_TC;

  int pix[NU];
  halo_pixels<NU>(pix, tid, n, r0, c0, d, HC, npix, a.H, a.W);

  const int K = ks * ks * a.Ci;
  const int nch = (a.Ci + 31) >> 5;                      // chunks: Ci / 32 full ones + the 16-channel tail
  const int co16 = a.Co >> 4, npass = (co16 + NJ - 1) / NJ;
  const int total = npass * 4 * nch;                     // iteration it = (pass * 4 + class) * nch + chunk

  uint4 hreg[NU], wreg[WU];
  // the halo is staged once when one chunk holds all of Ci, else by every iteration that has taps
  auto stages_halo = [&](int it, int cls) {
    return s2_class_taps(cls >> 1, ks) * s2_class_taps(cls & 1, ks) > 0 && (nch > 1 || it == 0);
  };
  auto prefetch = [&](int it) {
    const int pc = it / nch, ch = it - pc * nch, pass = pc >> 2, cls = pc & 3;
    const int cb = ch * 32, cw = min(32, a.Ci - cb);
    if (stages_halo(it, cls)) halo_load<NU>(hreg, pix, a.x, a.Ci, cb, cw >> 3, tid);
    const int njl = min(NJ, co16 - pass * NJ);
    const int nh = s2_class_taps(cls >> 1, ks), nw = s2_class_taps(cls & 1, ks);
    const int kh0 = s2_class_k0(cls >> 1, ks), kw0 = s2_class_k0(cls & 1, ks);
#pragma unroll
    for (int i = 0; i < WU; ++i) {
      const int t = wave + 4 * i;                        // fragment (tap, j) of unit tid + 256 i, tap = 2 th + tw
      const int tap = t / NJ, j = t - tap * NJ, th = tap >> 1, tw = tap & 1;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (th < nh && tw < nw && j < njl) {
        const bf16_t* src = a.w + (size_t)(pass * NJ * 16 + c16_row_channel(j, fr, njl)) * K +
                            ((kh0 + 2 * th) * ks + kw0 + 2 * tw) * a.Ci + cb;
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

  // the lane's B operand of fragment i at small-map offset (di, dj): halo pixel (d + 2 wave + i / 2 + di,
  // d + 16 (i & 1) + fr + dj)
  const unsigned char* hb0 = hal + ((wave * 2 + d) * HC + fr + d) * P;

  prefetch(0);
  for (int it = 0; it < total; ++it) {
    const int pc = it / nch, ch = it - pc * nch, pass = pc >> 2, cls = pc & 3;
    const int ca = cls >> 1, cb_ = cls & 1;              // row / column parity of the class's output pixels
    const int njl = min(NJ, co16 - pass * NJ);
    const bool tail = (a.Ci - ch * 32) < 32;
    const int nh = s2_class_taps(ca, ks), nw = s2_class_taps(cb_, ks);
    const int kh0 = s2_class_k0(ca, ks), kw0 = s2_class_k0(cb_, ks);
    if (nh * nw > 0) {                                   // a class without taps (k = 1) touches no LDS: no barriers
      __syncthreads();                                   // the previous iteration's fragment reads are done
      if (stages_halo(it, cls)) halo_store<NU, P>(hal, hreg, pix, tid);
#pragma unroll
      for (int i = 0; i < WU; ++i) {
        const int u = tid + 256 * i;
        if (!tail) *reinterpret_cast<uint4*>(wl + u * 16) = wreg[i];
        else *reinterpret_cast<uint2*>(wl + u * 8) = make_uint2(wreg[i].x, wreg[i].y);
      }
      __syncthreads();
    }
    if (it + 1 < total) prefetch(it + 1);                // in flight during the MFMAs below

    for (int th = 0; th < nh; ++th) {
      const int di = (ca + pad - kh0 - 2 * th) >> 1;     // even numerator: -1, 0 or 1
      for (int tw = 0; tw < nw; ++tw) {
        const int dj = (cb_ + pad - kw0 - 2 * tw) >> 1;
        const unsigned char* hb = hb0 + (di * HC + dj) * P;
        const int f0 = (th * 2 + tw) * NJ;
        if (!tail) {
          frag8_t bf[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            bf[i] = *reinterpret_cast<const frag8_t*>(hb + fq * 16 + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (j < njl) {
              const frag8_t af = *reinterpret_cast<const frag8_t*>(wl + ((f0 + j) * 64 + lane) * 16);
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[j][i] = mfma16<DT>(af, bf[i], acc[j][i]);
            }
          }
        } else {
          uint2 bf[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            bf[i] = *reinterpret_cast<const uint2*>(hb + fq * 8 + ((i >> 1) * HC + (i & 1) * 16) * P);
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (j < njl) {
              const uint2 af = *reinterpret_cast<const uint2*>(wl + ((f0 + j) * 64 + lane) * 8);
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[j][i] = mfma16k16<DT>(af, bf[i], acc[j][i]);
            }
          }
        }
      }
    }

    if (ch + 1 < nch) continue;
    // ---- epilogue of (pass, class): fragment i = small pixel (r0 + 2 wave + i / 2, c0 + 16 (i & 1) + fr) -> output
    // pixel (2 row + ca, 2 column + cb_)
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
          const int sh = r0 + wave * 2 + (i >> 1), sw = c0 + (i & 1) * 16 + fr;
          float v[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) { v[r] = acc[jp][i][r]; v[4 + r] = acc[j1][i][r]; }
          if (a.epi == EPI_BIAS_RELU) bias_act<EPI_BIAS_RELU, 8>(v, bv, true);
          else if (a.epi == EPI_BIAS) bias_act<EPI_BIAS, 8>(v, bv, true);
          if (sh < a.H && sw < a.W) {
            bf16_t* dst = a.y + ((size_t)(n * 2 * a.H + 2 * sh + ca) * (2 * a.W) + 2 * sw + cb_) * a.Co + cbase;
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
// weight + bias gradient of both layers
// ---------------------------------------------------------------------------------------------------------------
enum { S2_BIAS_NONE = 0, S2_BIAS_SMALL = 1, S2_BIAS_BIG = 2 };

struct S2WgArgs {
  const bf16_t* sm;      // [N][h][w][Ca], the small map
  const bf16_t* bg;      // [N][2 h][2 w][Cb], the large map
  float* ws;             // [S][Ca * Cb * kreal^2 + Cdb]
  int N, h, w, Ca, Cb;
  int kreal;             // taps per axis that are stored (KS, or 1 on the KS = 2 geometry)
  int bias_of, Cdb;      // whose pixel sum db is, and its channel count
  int tx, ty, total, tps;   // tiles along the small map's width / height, tiles in all, tiles per slice
  int nab;                  // 32-channel blocks of Ca
};

template <int DT, int KS>
__global__ void __launch_bounds__(256) s2_wgrad_kernel(S2WgArgs a) {
  constexpr int T = KS * KS, PD = s2_pad(KS), PW = s2_plane_cols(KS);
  constexpr int NU = (s2_win_pixels(KS) * 4 + 255) / 256;   // window units per thread
  constexpr int ND = (S2_TR * S2_TC * 4) / 256;             // small-tile units per thread
  constexpr int P = C16_WG_PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  // the wave index as a scalar: the two db conditions below then branch on SCC.  As a per-lane value they became EXEC
  // masks, and an MFMA runs whatever EXEC says: with both db forms in one kernel the form not asked for was added too
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* xh = smem;                              // the window
  unsigned char* sml = smem + s2_win_pixels(KS) * P;     // 128 pixels x 96 B

  const int ab = blockIdx.x % a.nab, bb = blockIdx.x / a.nab, slice = blockIdx.y;
  const int a0 = ab * C16_WG_CB, b0 = bb * C16_WG_CB;
  const int sa = wave & 1, sb = wave >> 1;
  const bool active = (a0 + 16 * sa < a.Ca) && (b0 + 16 * sb < a.Cb);
  const bool bias_small = a.bias_of == S2_BIAS_SMALL && bb == 0 && sb == 0 && active;
  const bool bias_big = a.bias_of == S2_BIAS_BIG && ab == 0 && sa == 0 && active;
  const int nus = min(4, (a.Ca - a0) >> 3), nub = min(4, (a.Cb - b0) >> 3);   // valid 16-B channel units

  const int t0 = slice * a.tps, t1 = min(a.total, t0 + a.tps);

  int pix[NU], dpix[ND];
  uint4 hreg[NU], dreg[ND];
  auto prefetch = [&](int t) {
    int b = t;
    const int tc = b % a.tx; b /= a.tx;
    const int tr = b % a.ty;
    const int n = b / a.ty;
    s2_window_pixels<NU>(pix, tid, n, tr * S2_TR, tc * S2_TC, KS, 2 * a.h, 2 * a.w);
    halo_pixels<ND>(dpix, tid, n, tr * S2_TR, tc * S2_TC, 0, S2_TC, S2_TR * S2_TC, a.h, a.w);
    halo_load<NU>(hreg, pix, a.bg, a.Cb, b0, nub, tid);
    halo_load<ND>(dreg, dpix, a.sm, a.Ca, a0, nus, tid);
  };

  f32x4 acc[T], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag8_t ones = ones_frag<DT>();

  // transposed reads (conv_small.hip): lane (g, q, p) addresses the 8-B run of channels 4 p .. 4 p + 3 of pixel
  // 4 g + q (low half of the lane's k values) and of pixel 16 + 4 g + q (high half)
  const int g = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
  const int plo = 4 * g + q;
  const unsigned char* slo = sml + plo * P + sa * 32 + p4 * 8;
  const unsigned char* xlo = xh + plo * P + sb * 32 + p4 * 8;

  if (t0 < t1) prefetch(t0);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    halo_store<NU, P>(xh, hreg, pix, tid);
    halo_store<ND, P>(sml, dreg, dpix, tid);
    __syncthreads();
    if (t + 1 < t1) prefetch(t + 1);
    if (active) {
#pragma unroll 2
      for (int r = 0; r < S2_TR; ++r) {
        const unsigned char* da = slo + r * S2_TC * P;
        const frag8_t af = c16_tr_read(da, da + 16 * P);
        if (bias_small) accb = mfma16<DT>(af, ones, accb);
#pragma unroll
        for (int tap = 0; tap < T; ++tap) {
          const int kh = tap / KS, kw = tap - kh * KS;
          // the 32 large-map pixels 2 j - p + kw of the row 2 r - p + kh: plane kw & 1, columns (kw >> 1) + j
          const unsigned char* xa = xlo + (((2 * r + kh) * 2 + (kw & 1)) * PW + (kw >> 1)) * P;
          const frag8_t bf = c16_tr_read(xa, xa + 16 * P);
          acc[tap] = mfma16<DT>(af, bf, acc[tap]);
          if (KS > 1 && (kh == PD || kh == PD + 1) && (kw == PD || kw == PD + 1)) {
            if (bias_big) accb = mfma16<DT>(ones, bf, accb);      // every row: the column sums
          }
        }
      }
    }
  }

  // D layout: column lane & 15 = large-map channel b, rows 4 (lane >> 4) + r = small-map channels a
  if (active) {
    const int fr = lane & 15, fq = lane >> 4;
    const int kr = a.kreal, tr_ = kr * kr;
    const size_t plane = (size_t)a.Ca * a.Cb * tr_;
    float* part = a.ws + (size_t)slice * (plane + a.Cdb);
    const int cbg = b0 + 16 * sb + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int csm = a0 + 16 * sa + fq * 4 + r;
#pragma unroll
      for (int tap = 0; tap < T; ++tap) {
        const int kh = tap / KS, kw = tap - kh * KS;
        if (kh < kr && kw < kr) part[((size_t)csm * a.Cb + cbg) * tr_ + kh * kr + kw] = acc[tap][r];
      }
      if (bias_small && fr == 0) part[plane + csm] = accb[r];
    }
    if (bias_big && fq == 0) part[plane + cbg] = accb[0];
  }
}

template <int DT, int NJ>
int launch_down(const D2Args& a, hipStream_t s) {
  auto kfn = conv_d2_kernel<DT, NJ>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)s2_down_lds(S2_MAX_K, NJ)));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3(a.N * a.ty * a.tx), dim3(256), s2_down_lds(a.ks, NJ), s, a);
  return (int)hipGetLastError();
}
template <int DT, int NJ>
int launch_up(const U2Args& a, hipStream_t s) {
  hipLaunchKernelGGL((conv_u2_kernel<DT, NJ>), dim3(a.N * a.ty * a.tx), dim3(256), s2_up_lds(a.ks, NJ), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_down_nj(const D2Args& a, hipStream_t s) {
  switch (a.Co >> 4) {
    case 1: return launch_down<DT, 1>(a, s);
    case 2: return launch_down<DT, 2>(a, s);
    case 3: return launch_down<DT, 3>(a, s);
    default: return launch_down<DT, C16_NJ>(a, s);
  }
}
template <int DT>
int launch_up_nj(const U2Args& a, hipStream_t s) {
  switch (a.Co >> 4) {
    case 1: return launch_up<DT, 1>(a, s);
    case 2: return launch_up<DT, 2>(a, s);
    case 3: return launch_up<DT, 3>(a, s);
    default: return launch_up<DT, C16_NJ>(a, s);
  }
}

template <int DT, int KS>
int launch_wg(const S2WgArgs& a, int S, hipStream_t s) {
  auto kfn = s2_wgrad_kernel<DT, KS>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)s2_wg_lds(KS)));
    attr = true;
  }
  const int ncb = a.nab * c16_cdiv(a.Cb, C16_WG_CB);
  hipLaunchKernelGGL(kfn, dim3(ncb, S), dim3(256), s2_wg_lds(KS), s, a);
  return (int)hipGetLastError();
}
template <int DT>
int launch_wg_ks(const S2WgArgs& a, int geo, int S, hipStream_t s) {
  switch (geo) {
    case 1: return launch_wg<DT, 1>(a, S, s);
    case 2: return launch_wg<DT, 2>(a, S, s);
    case 3: return launch_wg<DT, 3>(a, S, s);
    default: return launch_wg<DT, 4>(a, S, s);
  }
}

bool s2_epi_ok(int epi, const float* bias) {
  if (epi != EPI_BIAS_RELU && epi != EPI_BIAS && epi != EPI_NONE) return false;
  return epi == EPI_NONE || bias != nullptr;
}

}  // namespace
}  // namespace can

extern "C" int can_conv_down2(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Ci,
                              int Co, int ksize, int epi, int dt, void* stream) {
  using namespace can;
  const int rc = s2_check(N, H, W, Ci, Co, ksize);
  if (rc) return rc;
  if (!s2_epi_ok(epi, bias)) return S2_ERR_SHAPE;
  D2Args a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = (bf16_t*)y;
  a.N = N; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.ks = ksize; a.epi = epi;
  a.tx = c16_cdiv(W / 2, S2_TC); a.ty = c16_cdiv(H / 2, S2_TR);
  CAN_DT_DISPATCH(dt, launch_down_nj<DT>(a, (hipStream_t)stream));
}

extern "C" int can_conv_up2(const void* x, const void* w, const float* bias, void* y, int N, int h, int w_, int Ci,
                            int Co, int ksize, int epi, int dt, void* stream) {
  using namespace can;
  if (h < 1 || w_ < 1 || h > (1 << 20) || w_ > (1 << 20)) return S2_ERR_SHAPE;
  const int rc = s2_check(N, 2 * h, 2 * w_, Ci, Co, ksize);
  if (rc) return rc;
  if (!s2_epi_ok(epi, bias)) return S2_ERR_SHAPE;
  U2Args a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = (bf16_t*)y;
  a.N = N; a.H = h; a.W = w_; a.Ci = Ci; a.Co = Co; a.ks = ksize; a.epi = epi;
  a.tx = c16_cdiv(w_, C16_TC); a.ty = c16_cdiv(h, C16_TR);
  CAN_DT_DISPATCH(dt, launch_up_nj<DT>(a, (hipStream_t)stream));
}

extern "C" int can_conv_s2_slices(long long M, int Ca, int Cb) {
  return can::c16_wgrad_slices(M, Cb, Ca, can_device_cus());
}

extern "C" int can_conv_s2_wgrad(const void* small, const void* big, float* ws, long long ws_floats, float* dw,
                                 float* db, int N, int h, int w_, int Ca, int Cb, int ksize, int bias_of, float beta,
                                 float scale, int dt, void* stream) {
  using namespace can;
  if (h < 1 || w_ < 1 || h > (1 << 20) || w_ > (1 << 20)) return S2_ERR_SHAPE;
  const int rc = s2_check(N, 2 * h, 2 * w_, Ca, Cb, ksize);
  if (rc) return rc;
  if (bias_of != S2_BIAS_SMALL && bias_of != S2_BIAS_BIG) return S2_ERR_SHAPE;
  if (db == nullptr) bias_of = S2_BIAS_NONE;
  const int Cdb = bias_of == S2_BIAS_BIG ? Cb : Ca;
  const int S = c16_wgrad_slices((long long)N * h * w_, Cb, Ca, can_device_cus());
  if ((long long)S * ((long long)Ca * Cb * ksize * ksize + Cdb) > ws_floats) return S2_ERR_WS;
  S2WgArgs a;
  a.sm = (const bf16_t*)small; a.bg = (const bf16_t*)big; a.ws = ws;
  a.N = N; a.h = h; a.w = w_; a.Ca = Ca; a.Cb = Cb; a.kreal = ksize; a.bias_of = bias_of; a.Cdb = Cdb;
  a.tx = c16_cdiv(w_, S2_TC); a.ty = c16_cdiv(h, S2_TR); a.total = N * a.tx * a.ty;
  a.tps = c16_cdiv(a.total, S);
  a.nab = c16_cdiv(Ca, C16_WG_CB);
  // ksize 1 with db over the large map: the pixels at odd rows / columns belong to no tap, so the KS = 2 window
  const int geo = (ksize == 1 && bias_of == S2_BIAS_BIG) ? 2 : ksize;
  hipStream_t s = (hipStream_t)stream;
  int lrc = -20;
  if (dt == DT_F16) lrc = launch_wg_ks<DT_F16>(a, geo, S, s);
  else if (dt == DT_BF16) lrc = launch_wg_ks<DT_BF16>(a, geo, S, s);
  if (lrc) return lrc;
  return c16_reduce(ws, dw, db, S, Ca * Cb * ksize * ksize, Cdb, beta, scale, s);
}
