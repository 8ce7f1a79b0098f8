// Geometry of the large-kernel conv kernels (conv_large.hip): 5x5 and 7x7 layers on channel counts that are multiples
// of 16.  The pixel tile, the pitches, the slice count and the workspace are those of conv_small_plan.h; what is new is
// the reach rule and the LDS of weights that go by one tap row at a time.  Pure functions, host and device.
#pragma once
#include "conv_small_plan.h"

namespace can {

// the halo reaches d = dil * (ksize / 2) pixels; the staging of conv_small_dev.h is sized for C16_MAX_DIL = 4 of them
constexpr int l16_max_dil(int ksize) { return C16_MAX_DIL / (ksize / 2); }        // 5x5: 2, 7x7: 1
constexpr int l16_max_reach(int ksize) { return l16_max_dil(ksize) * (ksize / 2); }   // 5x5: 4, 7x7: 3

// forward: the halo at the 80-byte pitch + two buffers of one tap row (ksize * nj fragments of 1 KiB)
constexpr size_t l16_fwd_lds(int ksize, int dil, int nj) {
  return (size_t)((c16_halo_pixels(dil * (ksize / 2)) * C16_FWD_PITCH + 15) & ~15) + 2 * (size_t)ksize * nj * 1024;
}
// weight gradient: the 8 x (32 + 2 d) strip of x a tap row reads + the dY tile, both at the 96-byte pitch
constexpr int l16_strip_pixels(int d) { return C16_TR * (C16_TC + 2 * d); }
constexpr size_t l16_wg_lds(int ksize, int dil) {
  return (size_t)(l16_strip_pixels(dil * (ksize / 2)) + C16_TR * C16_TC) * C16_WG_PITCH;
}

// what both entry points refuse before any launch
constexpr int l16_check(int N, int H, int W, int Ci, int Co, int ksize, int dil) {
  if (N < 1 || H < 1 || W < 1 || Ci < 16 || Co < 16 || (Ci & 15) || (Co & 15) || (ksize != 5 && ksize != 7))
    return C16_ERR_SHAPE;
  if (dil < 1 || dil > l16_max_dil(ksize)) return C16_ERR_DIL;
  if ((long long)N * H * W * (Ci > Co ? Ci : Co) >= (1LL << 30)) return C16_ERR_ELEMS;   // 32-bit pixel offsets
  return 0;
}

}  // namespace can
