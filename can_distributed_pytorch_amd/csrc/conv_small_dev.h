// Device helpers of the small-channel conv kernels (conv_small.hip), shared with the thin-channel family
// (conv_thin.hip) and the large-kernel family (conv_large.hip): the 16-deep MFMA, halo staging through registers, and the transposing LDS fragment read.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "common.h"
#include "conv_small_plan.h"

namespace can {
namespace {

typedef short c16_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) c16_s16x4 c16_lds_s16x4;
typedef __bf16 c16_bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 c16_f16x4 __attribute__((ext_vector_type(4)));

// the 16-deep MFMA of the 16-channel tail: operands are 4 x 16-bit per lane (raw bits in a uint2)
template <int DT>
__device__ __forceinline__ f32x4 mfma16k16(const uint2& a, const uint2& b, const f32x4& c) {
  if constexpr (DT == DT_F16)
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(c16_f16x4, a), __builtin_bit_cast(c16_f16x4, b), c,
                                                 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(c16_s16x4, a),
                                                     __builtin_bit_cast(c16_s16x4, b), c, 0, 0, 0);
}

// local output channel of MFMA row rho of block j, njl blocks in the pass (conv_small.hip: pairs are interleaved)
__device__ __forceinline__ int c16_row_channel(int j, int rho, int njl) {
  const int jp = j & ~1;
  return (jp + 1 < njl) ? jp * 16 + (rho >> 2) * 8 + (j & 1) * 4 + (rho & 3) : j * 16 + rho;
}

// ---------------------------------------------------------------------------------------------------------------
// Halo staging, shared by the forward and the weight-gradient kernel.  Unit u = tid + 256 i of the block is 16-B
// channel unit u & 3 of halo pixel u >> 2 (row-major over HR x HC pixels with origin (r0 - d, c0 - d)).
// pix[i]: the pixel's index in the [N][H][W] map, -1 outside the image (staged as zeros), -2 past the halo (no store).
// SH: log2 of the units per pixel (2: the four 16-B units of a 32-channel block; 0: one unit per pixel, conv_thin.hip).
// ---------------------------------------------------------------------------------------------------------------
template <int NU, int SH = 2>
__device__ __forceinline__ void halo_pixels(int (&pix)[NU], int tid, int n, int r0, int c0, int d, int HC, int npix,
                                            int H, int W) {
  const unsigned inv = 65536u / (unsigned)HC + 1u;      // hp / HC == (hp * inv) >> 16 for hp < 1024, HC <= 40
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int hp = (tid + 256 * i) >> SH;
    const int hr = (int)(((unsigned)hp * inv) >> 16), hc = hp - hr * HC;
    const int ih = r0 - d + hr, iw = c0 - d + hc;
    const bool in = ih >= 0 && ih < H && iw >= 0 && iw < W;
    pix[i] = hp >= npix ? -2 : (in ? (n * H + ih) * W + iw : -1);
  }
}
// channels [cb, cb + 8 nun) of the halo pixels -> registers (units past nun, and pixels outside the image: zeros)
template <int NU>
__device__ __forceinline__ void halo_load(uint4 (&reg)[NU], const int (&pix)[NU], const bf16_t* __restrict__ x, int C,
                                          int cb, int nun, int tid) {
  const int un = tid & 3;
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (pix[i] >= 0 && un < nun) v = *reinterpret_cast<const uint4*>(x + (size_t)pix[i] * C + cb + un * 8);
    reg[i] = v;
  }
}
template <int NU, int PITCH>
__device__ __forceinline__ void halo_store(unsigned char* lds, const uint4 (&reg)[NU], const int (&pix)[NU], int tid) {
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = tid + 256 * i;
    if (pix[i] != -2) *reinterpret_cast<uint4*>(lds + (u >> 2) * PITCH + (u & 3) * 16) = reg[i];
  }
}

__device__ __forceinline__ frag8_t c16_tr_read(const unsigned char* lo, const unsigned char* hi) {
  const c16_s16x4 l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((c16_lds_s16x4*)lo);
  const c16_s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((c16_lds_s16x4*)hi);
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
  return __builtin_bit_cast(frag8_t, v);
}

}  // namespace
}  // namespace can
