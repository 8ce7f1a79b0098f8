// Geometry and launch plan of the small-channel conv kernels (conv_small.hip): channel counts that are multiples of 16
// but not both multiples of 64.  Pure functions of the problem shape, host and device, no HIP calls.
#pragma once
#include <stddef.h>

namespace can {

constexpr int C16_TR = 8, C16_TC = 32;        // pixel tile of a block: 8 rows x 32 columns (each wave 2 rows)
constexpr int C16_MAX_DIL = 4;                // halo of at most (8 + 8) x (32 + 8) pixels
constexpr int C16_NJ = 4;                     // 16-channel output blocks a forward pass keeps in registers
constexpr int C16_FWD_PITCH = 80;             // LDS bytes per halo pixel, forward (see conv_small.hip)
constexpr int C16_WG_PITCH = 96;              // ... weight gradient
constexpr int C16_WG_CB = 32;                 // channels of a weight-gradient block on either side (2 x 2 waves)
constexpr int C16_MAX_SLICES = 128;

// launcher refusals
enum { C16_ERR_SHAPE = -40, C16_ERR_DIL = -41, C16_ERR_ELEMS = -42, C16_ERR_WS = -43 };

constexpr int c16_cdiv(int a, int b) { return (a + b - 1) / b; }

// halo pixels of a tile at padding d = dil * (ksize / 2)
constexpr int c16_halo_pixels(int d) { return (C16_TR + 2 * d) * (C16_TC + 2 * d); }

// Pixel slices of the weight gradient: two blocks per CU over all channel blocks, at most one slice per 256 pixels
// (M pixels make at least ceil(M / 256) tiles whatever the map's shape, so every slice count this returns is at
// most the tile count) and at most C16_MAX_SLICES partials for the reduce to sum.
constexpr int c16_wgrad_slices(long long M, int Ci, int Co, int cus) {
  const int cb = c16_cdiv(Co, C16_WG_CB) * c16_cdiv(Ci, C16_WG_CB);
  long long s = (2LL * (cus > 0 ? cus : 256) + cb - 1) / cb;
  const long long cap = (M + 255) / 256;
  if (s > cap) s = cap;
  if (s > C16_MAX_SLICES) s = C16_MAX_SLICES;
  return s < 1 ? 1 : (int)s;
}

// fp32 workspace of the weight gradient: S partials of dW [Co][Ci][k][k] followed by S partials of db [Co]
constexpr long long c16_wgrad_ws_floats(int S, int Ci, int Co, int ksize) {
  return (long long)S * ((long long)Co * Ci * ksize * ksize + Co);
}

}  // namespace can
