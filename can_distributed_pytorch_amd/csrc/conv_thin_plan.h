// Geometry and launch plan of the thin-channel conv kernels (conv_thin.hip): one channel count is 1 .. 8 (the thin
// side t), the other a multiple of 16.  Pure functions of the problem shape, host and device, no HIP calls.  The pixel
// tile (8 x 32), the dilation limit and the LDS pitches of the wide operand are those of conv_small_plan.h.
#pragma once
#include "conv_small_plan.h"

namespace can {

constexpr int THIN_MAX = 8;                   // largest thin channel count
constexpr int THIN_WG_PITCH = 32;             // LDS bytes per pixel of the thin operand of the weight gradient (16 ch)
constexpr int THIN_MAX_SLICES = 256;          // pixel slices of the weight gradient (each writes two partials)

// K = ksize^2 t of thin_in is covered by MFMA steps of 32 and, for a rest of 1 .. 16, one last step of 16
constexpr int thin_k_steps(int K) { return (K + 31) / 32; }
constexpr bool thin_k_tail16(int K) { return (K & 31) >= 1 && (K & 31) <= 16; }
constexpr int thin_k_pad(int K) { return thin_k_tail16(K) ? (K / 32) * 32 + 16 : thin_k_steps(K) * 32; }

// largest power of two <= vmax that divides the row length (elements) and to which the pointer is aligned: the
// width in elements of the flat row loads / stores (every row start is then a multiple of it)
inline int thin_vec(const void* p, long long row_elems, int esize, int vmax) {
  int v = vmax;
  while (v > 1 && ((row_elems % v) != 0 || (((unsigned long long)(size_t)p) % (unsigned)(v * esize)) != 0)) v >>= 1;
  return v;
}

// thin_in halo row: ph = elements between the aligned start of the first unit and the halo's first element,
// upr = units per halo row (the phase is the same for every tile: a tile starts at a multiple of 32 pixels)
constexpr int thin_in_phase(int t, int d, int vec) { return (((-d * t) % vec) + vec) % vec; }
constexpr int thin_in_upr(int t, int d, int vec) { return (thin_in_phase(t, d, vec) + (C16_TC + 2 * d) * t + vec - 1) / vec; }
// units a thread stages per tile, for the largest halo of a load width (t = 8, d = 4; ksize 1: no halo)
constexpr int thin_in_nu(int vec, int ks) {
  return ks == 3 ? ((C16_TR + 2 * C16_MAX_DIL) * thin_in_upr(THIN_MAX, C16_MAX_DIL, vec) + 255) / 256
                 : (C16_TR * (C16_TC * THIN_MAX / vec) + 255) / 256;
}
constexpr int THIN_IN_ROW_BYTES = ((7 + (C16_TC + 2 * C16_MAX_DIL) * THIN_MAX + 7) * 2 + 15) & ~15;   // 672
constexpr int THIN_IN_LDS = (C16_TR + 2 * C16_MAX_DIL) * THIN_IN_ROW_BYTES;

// Weight gradient: a block owns 32 channels of the wide side (two waves) and splits its tiles' rows between two wave
// pairs, so a pixel slice writes TWO partials.  Slices: two blocks per CU over the wide side's blocks, at most one
// slice per 256 pixels (a tile), at most THIN_MAX_SLICES.  Returns the number of partials (2 x slices).
constexpr int thin_wgrad_partials(long long M, int Ci, int Co, int cus) {
  const int wide = Ci > Co ? Ci : Co;
  const int cb = c16_cdiv(wide, C16_WG_CB);
  long long s = (2LL * (cus > 0 ? cus : 256) + cb - 1) / cb;
  const long long cap = (M + 255) / 256;
  if (s > cap) s = cap;
  if (s > THIN_MAX_SLICES) s = THIN_MAX_SLICES;
  return 2 * (s < 1 ? 1 : (int)s);
}

}  // namespace can
