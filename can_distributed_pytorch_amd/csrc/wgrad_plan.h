// Launch planning of the weight gradients (conv_wgrad.hip): the tile-config table, plan_wgrad() and
// plan_wgrad_1x1_batched(), the ONE place that decides which kernel, slice count, bias mode, slab reduction and
// workspace size a weight-gradient launch gets.  The launchers execute a plan; can_wgrad_plan and the
// wgrad_launch_plan / wgrad_1x1_batched_launch_plan bindings return fields of it.  Host-only, plain C++17: no HIP
// calls, no globals.
#pragma once
#include "dispatch.h"
#include <algorithm>

namespace can {

// bias partial rows of the column-sum kernel and the most the slab reductions' bias blocks read (the workspace's bias
// area holds max(S, kBiasParts) x Cout floats)
constexpr int kBiasParts = 512;

// Kernel families: register-staged first-layer conv_wgrad_kernel, LDS-DMA v1 wgrad_glds_kernel, pipelined v2
// wgrad_glds2_kernel (row-aligned stages; virtual pixels on a ragged width), tap ring (wgrad_tap.inc), row-ring halo
// kernel (wgrad_ring.inc)
enum WgradFamily { WG_FIRST, WG_GLDS, WG_GLDS2, WG_TAP, WG_HALO };
struct WgradTile {
  int cfg, fam;
  int TCo, TK, BKM;                 // output channels x k per tile, pixels per stage (slices are whole stages);
                                    // tap ring: TCo = wgrad_tap_tco(Cout); halo: 64 x (9 taps x 64 ci) per co tile
  int WC, WK, WM, NBUF, KW, KK;     // the template arguments of the family's kernel (0: it has no such argument)
  int v1;                           // v2 configs: the v1 config (same tiles and slicing) that runs the layers v2 cannot
};
constexpr WgradTile kWgradTiles[] = {
    {0, WG_FIRST, 64, 64, 128, 1, 1, 4, 0, 0, 0, 0},
    {1, WG_GLDS, 128, 128, 64, 2, 2, 1, 4, 1, 2, 0},       // 4 waves, 4 buffers
    {2, WG_GLDS, 256, 128, 64, 4, 2, 1, 3, 1, 2, 0},       // 8 waves, 3 buffers
    {3, WG_GLDS, 64, 128, 128, 1, 2, 2, 3, 1, 2, 0},       // 4 waves, pixel-split 2, 3 buffers
    {4, WG_GLDS, 64, 64, 128, 1, 1, 2, 4, 1, 2, 0},        // 2 waves, pixel-split 2, 4 buffers
    {6, WG_GLDS, 128, 256, 64, 2, 2, 1, 3, 2, 2, 0},
    {7, WG_GLDS, 256, 256, 64, 4, 2, 1, 2, 2, 2, 0},
    {8, WG_HALO, 64, 576, 128, 0, 0, 0, 0, 0, 0, 0},       // tiles of 2 x 64 pixels
    {9, WG_GLDS2, 256, 256, 64, 4, 2, 0, 0, 2, 0, 7},
    {10, WG_GLDS2, 256, 128, 64, 4, 2, 0, 0, 1, 0, 2},     // k tile = one tap of a Cin % 128 layer
    {11, WG_GLDS2, 128, 256, 64, 2, 4, 0, 0, 1, 0, 6},     // Cout = 128
    {12, WG_TAP, 0, 576, 64, 0, 0, 0, 0, 0, 0, 0},
};
constexpr const WgradTile* find_wgrad_tile(int cfg) {
  for (const WgradTile& t : kWgradTiles)
    if (t.cfg == cfg) return &t;
  return nullptr;
}
constexpr bool wgrad_tiles_consistent() {
  for (const WgradTile& t : kWgradTiles) {
    if (t.fam == WG_GLDS && (t.TCo != 64 * t.WC || t.TK != 64 * t.WK * t.KW || t.BKM != 32 * t.KK * t.WM)) return false;
    if (t.fam == WG_GLDS2 && (t.TCo != 64 * t.WC || t.TK != 64 * t.WK * t.KW || t.BKM != 64)) return false;
    if (t.fam == WG_FIRST && (t.TCo != 64 * t.WC || t.TK != 64 * t.WK || t.BKM != 32 * t.WM)) return false;
    if (t.fam == WG_GLDS2) {
      const WgradTile* f = find_wgrad_tile(t.v1);
      if (!f || f->fam != WG_GLDS || f->TCo != t.TCo || f->TK != t.TK || f->BKM != t.BKM) return false;
    }
  }
  return true;
}
static_assert(wgrad_tiles_consistent(), "kWgradTiles: tile sizes do not follow from the template arguments");

// the output-channel tile of the tap-ring kernel for a layer: 128 (Cout % 128 == 0), 64 (Cout == 64), else 0
constexpr int wgrad_tap_tco(int Cout) { return (Cout % 128 == 0) ? 128 : (Cout == 64) ? 64 : 0; }
// the tap-ring kernel applies: 3x3, dilation 1 / 2, Cin % 64 == 0, Cout % 128 == 0 or Cout == 64, W % 8 == 0,
// operands addressable by 32-bit buffer offsets
constexpr bool wgrad_tap_ok(int N, int H, int W, int Cin, int Cout, int ksize, int dil) {
  const long long M = (long long)N * H * W;
  return ksize == 3 && (dil == 1 || dil == 2) && Cin % 64 == 0 && wgrad_tap_tco(Cout) != 0 && W % 8 == 0 && W >= 8 &&
         H >= 1 && M * Cout * 2 < 0x7fffff00LL && M * Cin * 2 < 0x7fffff00LL;
}

// The slab reduction of S slabs [K][Cout]: the LDS-transposing tiled kernel (3x3 layers with few slabs and >= 256
// tiles of 64 co x RCI ci) or the grid-stride kernel with 1 / 4 / 64 / 16 slab groups per block.
constexpr int RCI = 8;
enum WgradReduce { RED_TILED = 0, RED_1 = 1, RED_4 = 4, RED_16 = 16, RED_64 = 64 };
constexpr int wgrad_reduce_kind(int S, int K, int Cout, int Cin, int taps, int first) {
  if (!first && taps == 9 && S <= 16 && Cout % 64 == 0 && Cin % RCI == 0 && (Cout / 64) * (Cin / RCI) >= 256)
    return RED_TILED;
  if (S <= 16) return RED_1;
  if (S <= 128) return RED_4;
  // a small plane over many slabs (conv1_1's 36 x 64 over the ~512 slabs of the fused w1g kernel): 64 slab groups
  // of 4 elements per block, 8 slabs per thread -- <16> gave 148 blocks of 32 dependent loads per thread, 37 us
  return ((long long)K * Cout < 4096) ? RED_64 : RED_16;
}

// Where db comes from.  WB_KERNEL: the GEMM kernel writes one partial row per slice (Sb = S).  WB_COLSUM: a column-sum
// launch before the GEMM writes kBiasParts rows (v2 and the tap ring do no bias work).  WB_EXT: the data-gradient
// epilogue that produced dY already summed it into bext_rows <= kBiasParts rows, read in place.  WB_EXT_FOLD: a longer
// list is first folded to Sb_ext <= kBiasParts rows of bias_rpb input rows each, into the workspace's bias area.
enum WgradBias { WB_NONE, WB_KERNEL, WB_COLSUM, WB_EXT, WB_EXT_FOLD };

struct WgradQuery {
  int N = 1, H = 0, W = 0;    // W = 0: the map's width is unknown (sizing callers): the tap ring is not chosen and the
                              // width-dependent fields (family of cfg 9-11, ragged, vM) are not set.  H = 0: only
                              // M and W are known (the can_wgrad_plan query): a map under 2 x 2 is not refused and
                              // the halo tile counts are not set
  int M = 0;                  // N * H * W (a multiple of W when W is given)
  int Cin = 0, Cout = 0, ksize = 3, dil = 1, first = 0;
  bool want_db = false;
  int bext_rows = 0;          // rows of external bias partials (0: none)
  int target_blocks = 1024;   // the first layer's blocks per launch (a parameter of the can_wgrad_plan query only)
};
struct WgradPlan {
  int err = 0;                // 0 or the launcher's negative return code for this input (the other fields unset)
  int cfg = 0;                // a kWgradTiles entry
  int fam = 0;                // the family that runs: WG_GLDS for a cfg 9-11 layer the v2 kernel cannot take
  bool ragged = false;        // v2 on a width that is no multiple of 64: the virtual-pixel instantiation
  int S = 1, mslice = 0;      // pixel slices (slabs); pixels per slice (0: the tap ring / halo kernel slice by tiles)
  int vM = 0, vmslice = 0;    // a v2 launch's pixel count and slice length (virtual pixels when ragged)
  int ntile = 0, blocks = 0;  // (co, k) tiles; grid blocks = ntile * S
  int tap_total = 0, tap_spb = 0;   // tap ring: 64-pixel stages, stages per slice
  int halo_tiles = 0, halo_tps = 0; // halo kernel: 4 x 64 tiles, tiles per slice
  int bias = WB_NONE;
  int Sb = 0;                 // partial rows in the bias area: kBiasParts (WB_COLSUM), else S (written by WB_KERNEL)
  int Sb_ext = 0, bias_rpb = 0;     // WB_EXT / WB_EXT_FOLD: rows they sum; input rows folded into each (WB_EXT_FOLD)
  int reduce = RED_1;         // the slab-reduction kernel
  long long bias_off = 0;     // workspace: S slabs [K][Cout], then at this offset the bias area
  long long ws_floats = 0;    // S * K * Cout + max(S, kBiasParts) * Cout
};
inline WgradPlan wgrad_plan_error(int err) { WgradPlan p; p.err = err; return p; }

// The launch can_conv_wgrad makes for this query under dispatch d on a device of ncu CUs (<= 0: no device, an MI355X's
// 256 are assumed).  -2: not a first layer's channels; -3: channels not multiples of 64, or a map under 2 x 2 off the
// tap ring; -9: the slab plane exceeds the reduction's 32-bit indexing; -15: external bias partials for Cout > 1024.
inline WgradPlan plan_wgrad(const WgradQuery& q, const DispatchConfig& d, int ncu) {
  const int M = q.M, W = q.W, Cin = q.Cin, Cout = q.Cout, ksize = q.ksize, dil = q.dil;
  const bool first = q.first != 0;
  if (ncu <= 0) ncu = 256;
  const int K = first ? 64 : ksize * ksize * Cin;
  if ((long long)K * Cout >= 0x7fffffffLL) return wgrad_plan_error(-9);   // 32-bit plane indexing in the reduction
  // external bias partials (the dgrad epilogue that produced dY summed it): no bias work in the GEMM /
  // column-sum kernels, only a rows pre-reduction into the workspace's bias area (<= kBiasParts rows)
  const bool ext = q.want_db && q.bext_rows > 0;
  if (ext && (Cout % 64 || Cout > 1024)) return wgrad_plan_error(-15);
  if (first && (Cin != 4 || Cout % 64 || Cout < 64)) return wgrad_plan_error(-2);
  if (!first && (Cin % 64 || Cout % 64 || Cin < 64 || Cout < 64)) return wgrad_plan_error(-3);
  if (M < 1) return wgrad_plan_error(-3);

  WgradPlan p;
  // the halo weight-gradient kernel is dilation-1 only (B5: 256 -> 128, dil 2, reaches M >= 262144 at batch 32)
  const bool halo_ok = !first && ksize == 3 && dil == 1 && (Cout == 64 || Cout == 128) && Cin % 64 == 0;
  if (first) p.cfg = 0;
  else if (halo_ok && M >= 262144) p.cfg = 8;
  else if (Cout % 256 == 0 && K >= 2048) p.cfg = (K % 256 == 0) ? 9 : 7;
  else if (Cout % 256 == 0 && ksize == 1 && K % 256 == 0 && K >= 512)
    p.cfg = 9;   // 1x1 with many output rows (the linearised context module's dW2cat: 2048 x 512)
  else if (Cout % 256 == 0 && K >= 1024)
    p.cfg = (Cin % 128 == 0) ? 10 : 2;
  else if (Cout == 128 && Cin % 256 == 0 && K >= 2048)
    p.cfg = 11;
  else if (Cout % 128 == 0 && K >= 2048) p.cfg = 6;
  else if (Cout % 128 == 0) p.cfg = 1;
  else if (K >= 128) p.cfg = 3;
  else p.cfg = 4;
  // the tap-ring kernel (wgrad_tap.inc) for the layers the v2 GEMM takes (dispatch wgrad_tap >= 1) and the Cout = 128
  // ones of the full-resolution ring kernel (>= 2); it needs the map width (W = 0: unknown, not chosen)
  const int tco = wgrad_tap_tco(Cout);
  if (!first && W > 0 && M % W == 0 && wgrad_tap_ok(1, M / W, W, Cin, Cout, ksize, dil) &&
      d.wgrad_tap >= (tco == 64 ? 3 : p.cfg == 8 ? 2 : 1)) {
    // one block per CU (TCO 128) or two (TCO 64)
    p.ntile = (Cin / 64) * (Cout / tco);
    const int stages = (M / W) * ((W + 63) / 64);
    const int slots_per_cu = (tco == 128) ? 1 : 2;
    int S = 0;
    // the smallest slice count that fills whole rounds of the block slots to >= 90 %
    for (int R = 1; R <= 8 && !S; ++R) {
      const int s = (ncu * slots_per_cu * R) / p.ntile;
      if (s >= 1 && (long long)p.ntile * s * 10 >= 9LL * ncu * slots_per_cu * R) S = s;
    }
    if (S < 1) S = std::max(1, ncu * slots_per_cu / p.ntile);
    if (S > stages) S = stages;
    p.cfg = 12;
    p.S = S;
    p.tap_total = stages;
    p.tap_spb = (stages + S - 1) / S;
  } else {
    if (!first && q.H > 0 && (q.H < 2 || W < 2)) return wgrad_plan_error(-3);
    const WgradTile& t = *find_wgrad_tile(p.cfg);
    if (p.cfg == 8) {
      // slices of whole 4 x 64-pixel tiles: ~2 blocks per CU worth of (ci tile, co tile, slice) triples.
      // Cout = 128 runs as two 64-channel co tiles: the row-ring kernel (4-row tiles walked down 64-column strips,
      // each input row fetched once per strip)
      p.ntile = (Cin / 64) * (Cout / 64);
      p.S = std::max(1, 512 / p.ntile);
      if (q.H > 0) {
        p.halo_tiles = q.N * ((q.H + 3) / 4) * ((W + 63) / 64);
        p.halo_tps = (p.halo_tiles + p.S - 1) / p.S;
      }
    } else {
      p.ntile = (Cout / t.TCo) * ((K + t.TK - 1) / t.TK);
      // whole rounds of co-resident blocks (no half-empty last round)
      int S = q.target_blocks / p.ntile;
      if (!first) {
        // the pipelined kernels run one block per CU (LDS ring >= 128 KB): as few pixel slices as fill
        // whole rounds of the CUs to >= 90 % (fewer fp32 partial slabs to write and
        // reduce, longer K loops per block)
        for (int R = 1; R <= 8; ++R) {
          const int s = (ncu * R) / p.ntile;
          if (s >= 1 && (long long)p.ntile * s * 10 >= 9LL * ncu * R) { S = s; break; }
        }
      }
      S = std::max(1, std::min(S, (M + t.BKM - 1) / t.BKM));
      p.mslice = ((M + S - 1) / S + t.BKM - 1) / t.BKM * t.BKM;
      p.S = (M + p.mslice - 1) / p.mslice;
    }
  }
  const WgradTile& t = *find_wgrad_tile(p.cfg);
  p.fam = t.fam;
  p.blocks = p.ntile * p.S;
  if (t.fam == WG_GLDS2) {
    // v2 takes row-aligned stages: W % 64 == 0, or a 3x3 layer on a ragged width as virtual pixels (every row padded
    // to whole 64-pixel stages, the same slice count; slices past the end run no stage and write zero slabs)
    const bool rw = (W % 64) != 0 && ksize == 3;
    const long long vM = rw ? (long long)(M / W) * ((W + 63) / 64) * 64 : M;
    const long long vms = rw ? ((vM + p.S - 1) / p.S + 63) / 64 * 64 : p.mslice;
    if (W > 0 && (W % 64 == 0 || rw) && Cin % t.TK == 0 && K % t.TK == 0 && vms % 64 == 0 &&
        (long long)M * Cout * 2 < 0x7fffffffLL && Cout <= 2048) {
      p.ragged = rw;
      p.vM = (int)vM;
      p.vmslice = (int)vms;
    } else {
      p.fam = WG_GLDS;   // the tiles and slicing of t.v1
    }
  }
  if (ext) {
    // long external lists are folded to <= kBiasParts rows by a short launch queued AFTER the GEMM on this (weight-
    // gradient) stream: it then takes the CUs the GEMM's last blocks release.  Queued on the data-gradient stream (the
    // producer) it waited 85-345 us for CUs behind this stream's one-block-per-CU GEMM, on the critical path
    // (profiles/r3/ab_bias_prereduce.txt)
    p.bias = q.bext_rows <= kBiasParts ? WB_EXT : WB_EXT_FOLD;
    p.bias_rpb = p.bias == WB_EXT ? 0 : (q.bext_rows + kBiasParts - 1) / kBiasParts;
    p.Sb_ext = p.bias == WB_EXT ? q.bext_rows : (q.bext_rows + p.bias_rpb - 1) / p.bias_rpb;
  } else if (q.want_db) {
    p.bias = (p.fam == WG_GLDS2 || p.fam == WG_TAP) ? WB_COLSUM : WB_KERNEL;
  }
  p.Sb = p.bias == WB_COLSUM ? kBiasParts : p.S;
  p.reduce = wgrad_reduce_kind(p.S, K, Cout, first ? 4 : Cin, ksize * ksize, first);
  p.bias_off = (long long)p.S * K * Cout;
  p.ws_floats = p.bias_off + (long long)std::max(p.S, kBiasParts) * Cout;
  return p;
}

// Batched 1x1 weight gradient without bias (nb problems of one shape in one v2 launch of cfg 9's tiles): one round of
// 256 x 256 tiles over ncu CUs.  err -3: the shapes the kernel does not take (channels % 256, W % 64 with W = 0 for
// unknown, M % 64, 32-bit operand addressing).  S, mslice and ws_floats (nb * S slabs) are set whenever the channels
// hold a tile, also beside err: the executor sizes its workspace before it knows which maps take the batched launch.
struct WgradBatchedPlan {
  int err = 0, S = 0, mslice = 0;
  long long ws_floats = 0;
};
inline WgradBatchedPlan plan_wgrad_1x1_batched(int M, int W, int Cin, int Cout, int nb, int ncu) {
  constexpr WgradTile t = *find_wgrad_tile(9);
  WgradBatchedPlan p;
  if (Cout % t.TCo || Cin % t.TK || W % 64 || M % 64 || (long long)M * std::max(Cin, Cout) * 2 >= 0x7fffffffLL)
    p.err = -3;
  if (M < 1 || nb < 1 || Cin < t.TK || Cout < t.TCo || W < 0 || ncu < 1) {
    p.err = -3;
    return p;
  }
  const int ntile = (Cout / t.TCo) * (Cin / t.TK) * nb;
  const int S = std::max(1, ncu / ntile);
  p.mslice = ((M + S - 1) / S + 63) / 64 * 64;
  p.S = (M + p.mslice - 1) / p.mslice;
  p.ws_floats = (long long)nb * p.S * Cin * Cout;
  return p;
}

}  // namespace can
