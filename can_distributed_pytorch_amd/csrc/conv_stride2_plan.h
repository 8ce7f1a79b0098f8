// Geometry of the stride-2 conv kernels (conv_stride2.hip): a down-sampling conv and its adjoint, the 2x transposed
// conv, on Ci, Co multiples of 16; ksize 1 .. 4, padding p = (ksize - 1) / 2, a large map of even H x W and a small map
// of H/2 x W/2.  The pitches, the slice count and the workspace are those of conv_small_plan.h.  Pure functions, host
// and device, no HIP calls.
#pragma once
#include "conv_small_plan.h"

namespace can {

constexpr int S2_TR = 4, S2_TC = 32;          // small-map tile of the gathering kernels (down2, wgrad): a wave owns a row
constexpr int S2_MAX_K = 4;

// launcher refusals
enum { S2_ERR_SHAPE = -50, S2_ERR_KSIZE = -51, S2_ERR_ELEMS = -52, S2_ERR_WS = -53 };

constexpr int s2_pad(int ksize) { return (ksize - 1) / 2; }

// The large-map window of an S2_TR x S2_TC small-map tile, split by column parity: window row wr = 2 r + kh, window
// column wc = 2 c + kw sits in plane wc & 1 at column wc >> 1, so that a tap reads S2_TC consecutive pixels of one
// plane.  Layout [wr][plane][pw]; ksize 1 reads even rows and the even plane only (the rest is never staged).
constexpr int s2_win_rows(int ksize) { return 2 * (S2_TR - 1) + ksize; }
constexpr int s2_plane_cols(int ksize) { return S2_TC + (ksize > 2 ? 1 : 0); }
constexpr int s2_win_pixels(int ksize) { return s2_win_rows(ksize) * 2 * s2_plane_cols(ksize); }

// down2: the window at the 80-byte pitch + two buffers of one tap row (ksize * nj fragments of 1 KiB)
constexpr size_t s2_down_lds(int ksize, int nj) {
  return (size_t)((s2_win_pixels(ksize) * C16_FWD_PITCH + 15) & ~15) + 2 * (size_t)ksize * nj * 1024;
}
// up2: the halo of an 8 x 32 small-map tile (reach 1 pixel from ksize 3 on) at the 80-byte pitch + the at most 2 x 2
// taps of one parity class (4 nj fragments of 1 KiB)
constexpr int s2_up_reach(int ksize) { return ksize > 2 ? 1 : 0; }
constexpr size_t s2_up_lds(int ksize, int nj) {
  return (size_t)((c16_halo_pixels(s2_up_reach(ksize)) * C16_FWD_PITCH + 15) & ~15) + 4 * (size_t)nj * 1024;
}
// weight gradient: the window + the small-map tile, both at the 96-byte pitch
constexpr size_t s2_wg_lds(int ksize) { return (size_t)(s2_win_pixels(ksize) + S2_TR * S2_TC) * C16_WG_PITCH; }

// taps of one axis that reach output parity a of the transposed conv: kh = kh0 + 2 t < ksize with kh0 = (a + p) & 1;
// tap kh reads the small map at offset (a + p - kh) / 2 (-1, 0 or 1)
constexpr int s2_class_k0(int a, int ksize) { return (a + s2_pad(ksize)) & 1; }
constexpr int s2_class_taps(int a, int ksize) { return (ksize - s2_class_k0(a, ksize) + 1) / 2; }

// what every entry point refuses before any launch; H x W: the large map
constexpr int s2_check(int N, int H, int W, int Ci, int Co, int ksize) {
  if (N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || Ci < 16 || Co < 16 || (Ci & 15) || (Co & 15)) return S2_ERR_SHAPE;
  if (ksize < 1 || ksize > S2_MAX_K) return S2_ERR_KSIZE;
  if ((long long)N * H * W * (Ci > Co ? Ci : Co) >= (1LL << 30)) return S2_ERR_ELEMS;   // 32-bit pixel offsets
  return 0;
}

}  // namespace can
