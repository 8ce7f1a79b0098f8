// Launch planning of the forward / data-gradient convs (conv_igemm.hip): the tile-config table and plan_conv(), the
// ONE place that decides which kernel family, tile config, split-K factor and bias-partial rows a conv launch gets.
// The launchers execute a plan; can_conv_plan, can_splitk_plan, can_conv_pool_tp and the conv_launch_plan binding
// return fields of it.  Host-only, plain C++17: no HIP calls, no globals.
#pragma once
#include "dispatch.h"
#include <algorithm>
#include <stddef.h>

namespace can {

// Epilogues (described at the top of conv_igemm.hip).
enum { EPI_BIAS_RELU = 0, EPI_MASK = 1, EPI_NONE = 2, EPI_BIAS = 3, EPI_SIGMOID = 4, EPI_POOLBWD = 5,
       EPI_POOLFWD = 6, EPI_F32 = 7, EPI_CTXF = 8, EPI_CTXB = 9,
       // EPI_MASK whose ReLU mask comes as SIGN BITS (internal: the host API passes EPI_MASK + a bit tensor).
       // Sign bits of a 16-bit activation map [M][C]: byte m * (C / 8) + c / 8, bit c % 8 = (value > 0) on the
       // stored 16-bit pattern (pos_bits).  Written by the producing conv's forward epilogue (1/16 of the map's
       // bytes), they replace the data gradient's 2-byte-per-element mask read: conv1_2's data gradient reads
       // 50 MB instead of conv1_1's 805 MB output at batch 8 x 768 x 1024, conv2_2's 25 instead of 403 MB
       EPI_MASKB = 10 };

// Tile configs: the numbers are the `tile=` / tile_cfg values of the API (0 = the planner chooses).  Families:
// generic conv_igemm_kernel (1-4), LDS-DMA v1 conv_glds_kernel (11-13), v2 conv_glds2_kernel (21-25; 24 is the 4-wave
// tile of the context GEMMs only, not a tile= value), conv_rring_kernel (27-29), conv_halo64_kernel (31),
// conv_first_halo_kernel (32), conv_ws64_kernel (33: the weight-stationary form of 31 for Cout = 64, dispatch ws64)
enum ConvFamily { FAM_GENERIC, FAM_GLDS, FAM_GLDS2, FAM_CTX, FAM_RRING, FAM_HALO, FAM_FIRST, FAM_WS64 };
enum : unsigned {
  CAP_MASKB_IN = 1,    // takes the ReLU mask as sign bits (EPI_MASKB)
  CAP_SIGN_OUT = 2,    // writes its output's sign bits
  CAP_POOLFWD = 4,     // 2x2 max-pool in the epilogue (conv_pool_fwd)
  CAP_POOLBWD = 8,     // max-pool backward in the epilogue (EPI_POOLBWD)
  CAP_BATCHED = 16,    // nb > 1 items in one launch (grid.y)
  CAP_SPLITK = 32,     // split-K on small grids
  CAP_PADW = 64,       // width-padded maps (wv < W)
  CAPS_V2 = CAP_MASKB_IN | CAP_POOLFWD | CAP_POOLBWD | CAP_BATCHED | CAP_SPLITK | CAP_PADW,
  CAPS_RING = CAP_POOLBWD | CAP_PADW
};
struct TileCfg {
  int cfg, fam;
  int TC;               // output channels per tile (0: all of Cout)
  int TR, TW;           // a tile is TR image rows x TW columns; TR = 0: TW consecutive pixels (running across rows);
                        // TW = 0 (cfg 31): 64 columns for Cout = 64 (two blocks per CU), else 128
  int WC, WP, PW;       // waves along channels / pixels, 64-pixel fragments per wave (template arguments)
  int bp_slots;         // bias-partial rows per pixel tile (the wave slots along the pixels; 0: writes none)
  unsigned caps;
};
constexpr TileCfg kTileCfgs[] = {
    {1, FAM_GENERIC, 128, 0, 128, 2, 2, 1, 0, 0},
    {2, FAM_GENERIC, 64, 0, 256, 1, 4, 1, 0, 0},
    {3, FAM_GENERIC, 128, 0, 256, 2, 4, 1, 0, 0},
    {4, FAM_GENERIC, 256, 0, 128, 4, 2, 1, 0, 0},
    {11, FAM_GLDS, 256, 0, 256, 4, 2, 2, 2, CAP_POOLBWD | CAP_PADW},
    {12, FAM_GLDS, 128, 0, 256, 2, 4, 1, 4, CAP_POOLBWD | CAP_PADW},
    {13, FAM_GLDS, 64, 0, 512, 1, 8, 1, 8, CAP_POOLBWD | CAP_PADW},
    {21, FAM_GLDS2, 256, 0, 256, 4, 2, 2, 2, CAPS_V2},
    {22, FAM_GLDS2, 128, 0, 256, 2, 4, 1, 4, CAPS_V2},
    {23, FAM_GLDS2, 64, 0, 512, 1, 8, 1, 8, CAPS_V2},
    {24, FAM_CTX, 128, 0, 128, 2, 2, 1, 0, CAP_PADW},
    {25, FAM_GLDS2, 128, 0, 512, 2, 4, 2, 4, CAPS_V2},     // 2 fragments per wave, 160 KB LDS
    // row ring: the wave tiles of 21 / 23 / 22 on TR x 128-pixel tiles (bitwise those configs' results)
    {27, FAM_RRING, 256, 2, 128, 4, 2, 2, 2, CAPS_RING | CAP_POOLFWD | CAP_SPLITK},
    {28, FAM_RRING, 64, 4, 128, 1, 8, 1, 8, CAPS_RING},
    {29, FAM_RRING, 128, 2, 128, 2, 4, 1, 4, CAPS_RING | CAP_POOLFWD | CAP_SPLITK},
    {31, FAM_HALO, 0, 4, 0, 0, 0, 0, 4, CAP_SIGN_OUT | CAP_POOLFWD | CAP_PADW},
    {32, FAM_FIRST, 64, 4, 128, 0, 0, 0, 0, CAP_SIGN_OUT | CAP_PADW},
    {33, FAM_WS64, 64, 4, 64, 0, 0, 0, 0, CAP_POOLFWD | CAP_PADW},
};
constexpr const TileCfg* find_tile_cfg(int cfg) {
  for (const TileCfg& t : kTileCfgs)
    if (t.cfg == cfg) return &t;
  return nullptr;
}
constexpr int tile_cols(const TileCfg& t, int Cout) { return t.TW ? t.TW : (Cout == 64 ? 64 : 128); }
// pixel tiles of a launch (a ragged last tile row / column block is masked)
constexpr int pixel_tiles(const TileCfg& t, int N, int H, int W, int Cout) {
  const int tw = tile_cols(t, Cout);
  return t.TR ? N * ((H + t.TR - 1) / t.TR) * ((W + tw - 1) / tw) : (N * H * W + tw - 1) / tw;
}
// pixels of the 2-row pooling tile of a config that pools in its epilogue: the fused pool needs H even and
// W % (pool_tile_px / 2) == 0
constexpr int pool_tile_px(const TileCfg& t, int Cout) { return t.TR ? 2 * tile_cols(t, Cout) : t.TW; }
// rows a data-gradient epilogue may write into the bias-partial buffer for an output of N x H x W pixels (pooled
// resolution for EPI_POOLBWD), whichever config runs it
constexpr int bias_part_capacity(int N, int H, int W) {
  int cap = 0;
  for (const TileCfg& t : kTileCfgs) cap = std::max(cap, pixel_tiles(t, N, H, W, 64) * t.bp_slots);
  return cap;
}

enum ConvEntry { ENTRY_IGEMM, ENTRY_POOL, ENTRY_BATCHED, ENTRY_CTX };   // conv_igemm, conv_pool_fwd, .._batched, conv_ctx
struct ConvQuery {
  int entry = ENTRY_IGEMM, N = 1, H = 0, W = 0, Cin = 0, Cout = 0, ksize = 3, dil = 1, epi = EPI_BIAS_RELU;
  int tile_cfg = 0;
  int wv = 0;                 // valid width of a width-padded map, W its row pitch (0 or >= W: no padding)
  int first = 0, nb = 1;      // first layer (NHWC4 input); items of a batched launch
  bool mbits_in = false;      // the EPI_MASK mask comes as sign bits
  bool mbits_out = false;     // the output's sign bits are wanted
  bool want_bpart = false;    // a bias-partial buffer of bpart_cap rows is given
  int bpart_cap = 0;
};
struct ConvPlan {
  int err = 0;                // 0 or the launcher's negative return code for this input (the other fields unset)
  int cfg = 0;                // tile config (a kTileCfgs entry)
  int npt = 0, tiles = 0;     // pixel tiles; channel tiles x pixel tiles
  int ks = 1;                 // split-K factor (after the scratch-size cap)
  int bpart_rows = 0;         // rows of the bias-partial buffer the launch writes (0: none)
  bool ragged = false;        // row ring: W % 128 != 0 or H % TR != 0 (the masked-tile instantiation)
};
inline ConvPlan plan_error(int err) { ConvPlan p; p.err = err; return p; }
constexpr int valid_width(const ConvQuery& q) { return (q.wv <= 0 || q.wv > q.W) ? q.W : q.wv; }

// default LDS-DMA tile config: v2 (pipelined); 128 x 512 tiles measured faster for K <= 1152
inline int glds_default_cfg(const ConvQuery& q) {
  const int ktot = q.ksize * q.ksize * q.Cin;
  return (q.Cout % 256 == 0) ? 21 : (q.Cout % 128 == 0) ? (ktot <= 1152 ? 25 : 22) : 23;
}

// column-block utilisation of the row ring on a ragged width: W / (ceil(W / 128) * 128) >= 0.6 (W = 240, 480,
// 960: 94 %; 80, 160: 62.5 %); below it (W = 72, 135: 53-56 %) the per-tap LDS-DMA kernel, whose pixel tiles run
// across rows, wastes less.  (Round 6 lowered it from 0.7: 480 x 640's 1/4- and 1/8-resolution maps, 160 and 80
// columns, ran the LDS-DMA kernel on 150-228-block grids at 10-20 % of the MFMA rate; on the row ring the batch-1
// step is 5.7 % faster, 345.9 / 346.1 -> 365.8 / 365.3 img/s, profiles/r6/ab_rring_width_480x640.jsonl.)
// A ragged width must be a multiple of 8: the row DMA's validity is then uniform per 8-pixel piece (see issue_rows)
inline bool rring_width_ok(int W) {
  if (W % 128 == 0) return true;
  const int tx = (W + 127) / 128;
  return W % 8 == 0 && W >= 64 && 10 * W >= 6 * 128 * tx;
}
// the row-ring kernel applies: 3x3, dilation 1 / 2, a width the column blocks cover well (rring_width_ok); Cout % 256
// == 0 (cfg 27, 2-row tiles), Cout % 128 (cfg 29) or Cout == 64 (cfg 28, 4-row tiles); 0 = not applicable
inline int rring_cfg(const ConvQuery& q, const DispatchConfig& d) {
  if (q.ksize != 3 || (q.dil != 1 && q.dil != 2) || !rring_width_ok(q.W) || q.Cin % 64 || q.epi == EPI_POOLFWD ||
      q.epi == EPI_SIGMOID || q.epi == EPI_CTXF || q.epi == EPI_CTXB)
    return 0;
  if (q.Cout % 256 == 0) return 27;
  // cfg 29 (128 x (2 x 128), the wave tile of cfg 22): dispatch rring128 = 1 (default) for the dilation-1 cfg-22
  // layers (K > 1152: conv3_1's data gradient 0.270 -> 0.253 ms), = 2 also for the cfg-25 ones (128 x 512 tiles,
  // K <= 1152: conv2_2 +2 %), = 3 also dilation 2 (backend.8 forward +10 %); 0 = off (profiles/r3/ab_rring128.txt)
  const int m128 = d.rring128;
  if (q.Cout % 128 == 0 && m128 >= ((9 * q.Cin > 1152) ? 1 : 2) && (q.dil == 1 || m128 >= 3)) return 29;
  // cfg 28: conv2_1's data gradient 0.435 -> 0.347 ms isolated, step 487.3 -> 489.9 img/s
  // (profiles/r3/ab_dma_order.txt)
  return q.Cout == 64 ? 28 : 0;
}

// Split-K on small grids: a row-ring (2-row tiles) or LDS-DMA v2 launch whose grid fills at most half the CUs (the
// 1/8-resolution 512-channel layers at batch 1: 48-96 tiles; a 480 x 640 image's LDS-DMA layers: 19-75 tiles for 256
// CUs) splits its 64-channel input chunks over KS = min(chunks, CUs / tiles) blocks per tile (<= one block per CU),
// joined by splitk_fixup.  Scratch: fp32 partials of <= CUs blocks (256 KB each for 256-channel tiles) and one
// arrival counter per tile, allocated once and zeroed (the last part resets its counter).  Dispatch splitk = 0: off.
constexpr size_t SK_PART_BYTES = (size_t)64 << 20;
constexpr int SK_COUNTERS = 4096;
inline int splitk_ks(const TileCfg& t, int tiles, const ConvQuery& q, const DispatchConfig& d, int ncu) {
  if (!d.splitk || !(t.caps & CAP_SPLITK) || tiles < 1 || 2 * tiles > ncu || tiles > SK_COUNTERS) return 1;
  const int ks = std::max(1, std::min(q.Cin / 64, ncu / tiles));
  // every (tile, part) publishes its fp32 accumulators: TC channels x the tile's pixels
  const size_t part = (size_t)t.TC * (t.TR ? t.TR * tile_cols(t, q.Cout) : t.TW) * 4;
  return ((size_t)tiles * ks * part > SK_PART_BYTES) ? 1 : ks;
}

// the launch of config cfg: tile counts, split-K (single launches of the configs that have it) and the bias-partial
// rows (when they fit the buffer)
inline ConvPlan plan_launch(const ConvQuery& q, const DispatchConfig& d, int ncu, int cfg, bool splitk, bool bpart) {
  const TileCfg& t = *find_tile_cfg(cfg);
  ConvPlan p;
  p.cfg = cfg;
  p.npt = pixel_tiles(t, q.N, q.H, q.W, q.Cout);
  p.tiles = (t.TC ? q.Cout / t.TC : 1) * p.npt;
  p.ragged = t.fam == FAM_RRING && (q.W % 128 != 0 || q.H % t.TR != 0);
  if (splitk) p.ks = splitk_ks(t, p.tiles, q, d, ncu);
  const long long rows = (long long)p.npt * t.bp_slots;
  if (bpart && rows > 0 && rows <= q.bpart_cap) p.bpart_rows = (int)rows;
  return p;
}
// an LDS-DMA / row-ring config (explicit or chosen): -9 not one, -8 its channel tile does not divide Cout or it takes
// no batched launch, -16 the row ring does not apply to this conv
inline ConvPlan plan_tile(const ConvQuery& q, const DispatchConfig& d, int ncu, int cfg) {
  const TileCfg* t = find_tile_cfg(cfg);
  if (!t || (t->fam != FAM_GLDS && t->fam != FAM_GLDS2 && t->fam != FAM_RRING)) return plan_error(-9);
  if (q.nb > 1 && !(t->caps & CAP_BATCHED)) return plan_error(-8);
  if (t->fam == FAM_RRING && rring_cfg(q, d) != cfg) return plan_error(-16);
  if (t->fam != FAM_RRING && q.Cout % t->TC) return plan_error(-8);
  return plan_launch(q, d, ncu, cfg, q.nb == 1, q.want_bpart);
}
// the generic kernel: tile_cfg 0 = auto, else one of its tiles 1-4
inline ConvPlan plan_generic(const ConvQuery& q, const DispatchConfig& d, int ncu) {
  int cfg = q.tile_cfg;
  if (cfg == 0) cfg = (q.Cout % 128 != 0) ? 2 : (q.Cout % 256 == 0 && q.N * q.H * q.W >= 65536) ? 4 : 1;
  return (cfg < 1 || cfg > 4) ? plan_error(-1) : plan_launch(q, d, ncu, cfg, false, false);
}
// the halo-tiled Cin = 64 kernels (31, 33) take 3x3 / dilation-1 convs to 64 or 128 channels; ws64 (weight-stationary)
// instead of the halo kernel for Cin = Cout = 64 (dispatch ws64 = 0: halo kernel): it writes no bias partials
inline bool halo_shape_ok(const ConvQuery& q) {
  return q.Cin == 64 && q.ksize == 3 && q.dil == 1 && (q.Cout == 64 || q.Cout == 128);
}
inline int halo_or_ws64(const ConvQuery& q, const DispatchConfig& d, bool bpart_fits) {
  return (q.Cout == 64 && !bpart_fits && d.ws64 != 0) ? 33 : 31;
}

// conv_igemm
inline ConvPlan plan_igemm(ConvQuery q, const DispatchConfig& d, int ncu) {
  const bool padded = q.wv < q.W && (q.epi == EPI_BIAS_RELU || q.epi == EPI_BIAS);
  if (q.epi != EPI_MASK && q.epi != EPI_POOLBWD) q.want_bpart = false;
  if (q.mbits_in && q.epi != EPI_MASK) return plan_error(-17);
  // sign-bit outputs: the first layer and the Cin = 64 -> 128 halo kernel (conv1_1, conv2_1), ReLU epilogue
  if (q.mbits_out &&
      !(q.epi == EPI_BIAS_RELU && q.Cout == (q.first ? 64 : 128) && (q.tile_cfg == 0 || q.tile_cfg == (q.first ? 32 : 31)) &&
        (q.first ? (q.Cin == 4 && q.ksize == 3 && q.dil == 1) : halo_shape_ok(q))))
    return plan_error(-18);
  if (q.Cout % 64 != 0) return plan_error(-2);
  if (!q.first && q.Cin % 64 != 0) return plan_error(-3);
  if (q.first && (q.Cin != 4 || q.ksize != 3)) return plan_error(-4);
  if (q.first) {
    if ((q.tile_cfg == 32 || q.tile_cfg == 0) && q.Cout == 64 && q.epi == EPI_BIAS_RELU)
      return plan_launch(q, d, ncu, 32, false, false);
    if (padded) return plan_error(-19);            // the generic first-layer kernel takes no padding
    return q.epi == EPI_BIAS_RELU ? plan_generic(q, d, ncu) : plan_error(-5);
  }
  int cfg = q.tile_cfg;
  if (cfg == 0 && halo_shape_ok(q) && q.epi != EPI_SIGMOID && q.epi != EPI_POOLBWD && q.epi != EPI_F32 && !q.mbits_in)
    cfg = 31;
  if (cfg == 31) {
    if (!halo_shape_ok(q)) return plan_error(-11);
    if (q.mbits_in) return plan_error(-17);
    if (q.epi != EPI_BIAS_RELU && q.epi != EPI_MASK && q.epi != EPI_NONE && q.epi != EPI_BIAS) return plan_error(-6);
    const bool bpart = q.want_bpart && q.epi == EPI_MASK;
    const ConvPlan p = plan_launch(q, d, ncu, 31, false, bpart);
    return plan_launch(q, d, ncu, halo_or_ws64(q, d, p.bpart_rows > 0), false, bpart);
  }
  if (cfg == 0 || cfg >= 10) {
    if (q.H < 2 || q.W < 2) return plan_error(-7);
    // dispatch rring: 0 = off, 1 = dilation-1 layers, 2 (default) = every dilation.  With the row DMAs placed after
    // their MFMA group (CANNET_DMA_ORDER_RR, a compile-time choice, common.h) the dilation-2 layers gain too: step
    // 497.0 -> 501.3 img/s (profiles/r3/ab_rring128.txt).  Before that placement, per layer at batch 8 x 768 x 1024
    // (profiles/r3/ab_rring.txt) -2..-6 % vs cfg 21 with the rows issued 3 stages ahead (issued 2 ahead with a full
    // DMA drain per stage: dilation 1 -1..-4 %, dilation 2 +1..+7 %); the step: off 482.6, dilation 1 485.4, every
    // dilation 484.9 img/s (medians of 4 interleaved rounds)
    if (cfg == 0 && d.rring >= q.dil) cfg = rring_cfg(q, d);
    if (cfg == 0) cfg = glds_default_cfg(q);
    // EPI_MASKB (the ReLU mask as sign bits) runs on the v2 LDS-DMA tiles only (the data-gradient configs of
    // conv2_2-like layers: 128 x 512 for K <= 1152 and the other v2 tiles)
    if (q.mbits_in && !(find_tile_cfg(cfg) && (find_tile_cfg(cfg)->caps & CAP_MASKB_IN))) return plan_error(-17);
    if (q.epi < EPI_BIAS_RELU || q.epi > EPI_F32 || q.epi == EPI_POOLFWD) return plan_error(-6);
    return plan_tile(q, d, ncu, cfg);
  }
  if (q.mbits_in) return plan_error(-17);
  if (padded) return plan_error(-19);              // the generic kernel takes no padding
  return (q.epi < EPI_BIAS_RELU || q.epi > EPI_SIGMOID) ? plan_error(-6) : plan_generic(q, d, ncu);
}

// conv_pool_fwd: conv + bias + ReLU with the 2x2/s2 max-pool in the epilogue
inline ConvPlan plan_pool(ConvQuery q, const DispatchConfig& d, int ncu) {
  q.epi = EPI_POOLFWD;
  q.want_bpart = false;
  if (q.Cout % 64 || q.Cin % 64 || q.H < 2 || q.W < 2) return plan_error(-3);
  if (q.wv % 2) return plan_error(-19);            // pool windows wholly inside or outside the valid columns
  // row ring with the max-pool in the epilogue: 256 x (2 x 128) tiles (Cout % 256 == 0) or 128 x (2 x 128).
  // Default (dispatch rring_pool) only the 256-channel form: conv3_3 + pool 0.429 -> 0.384 ms; the 128-channel
  // one loses to conv_glds2's 128 x 512 tile on conv2_2 (0.588 -> 0.639 ms), profiles/r4/ab_rring_pool.txt
  if (q.ksize == 3 && q.dil == 1 && q.H % 2 == 0 && q.W % 128 == 0) {
    if ((q.tile_cfg == 27 || (q.tile_cfg == 0 && d.rring_pool)) && q.Cout % 256 == 0)
      return plan_launch(q, d, ncu, 27, true, false);
    if (q.tile_cfg == 29 && q.Cout % 128 == 0) return plan_launch(q, d, ncu, 29, true, false);
  }
  if (halo_shape_ok(q) && q.Cout == 64 && q.tile_cfg == 0)   // conv1_2: halo-tiled kernel, 4 x 64 output tiles (full
    return (q.H % 4 || q.W % 64) ? plan_error(-13)           // tiles only: the pool epilogue has barriers)
                                 : plan_launch(q, d, ncu, halo_or_ws64(q, d, false), false, false);
  const int cfg = q.tile_cfg ? q.tile_cfg : glds_default_cfg(q);
  const TileCfg* t = find_tile_cfg(cfg);
  if (!t || t->fam != FAM_GLDS2 || (q.H & 1) || q.W % (pool_tile_px(*t, q.Cout) / 2)) return plan_error(-12);
  return plan_tile(q, d, ncu, cfg);
}

// The launch a conv entry point makes for this query under dispatch d on a device of ncu CUs.
inline ConvPlan plan_conv(ConvQuery q, const DispatchConfig& d, int ncu) {
  q.wv = valid_width(q);
  const bool small = q.Cin % 64 || q.Cout % 64 || q.H < 2 || q.W < 2;
  switch (q.entry) {
    case ENTRY_POOL: return plan_pool(q, d, ncu);
    case ENTRY_BATCHED:   // nb independent convs of one shape in ONE launch of a v2 config (grid.y = item)
      if (q.nb < 1 || q.nb > 65535 || small) return plan_error(-2);
      if (q.tile_cfg != 0 && q.tile_cfg < 20) return plan_error(-8);
      if (q.epi != EPI_NONE && q.epi != EPI_SIGMOID && q.epi != EPI_BIAS_RELU) return plan_error(-6);
      return plan_tile(q, d, ncu, q.tile_cfg ? q.tile_cfg : glds_default_cfg(q));
    case ENTRY_CTX:
      // EPI_CTXF: C -> 4C, EPI_CTXB: 4C -> C.  256 x 256 tiles (8 waves, one block per CU; <= 5 image rows per
      // 256-pixel tile) or 128 x 128 (4 waves, 64 KB ring: two blocks per CU, one block's epilogue beside the other's
      // main loop); dispatch ctx_tile_f / ctx_tile_b select
      if (std::min(q.Cin, q.Cout) % 256 || q.W < 64 || q.H < 1) return plan_error(-2);
      return plan_launch(q, d, ncu, (q.epi == EPI_CTXF ? d.ctx_tile_f : d.ctx_tile_b) == 128 ? 24 : 21, false, false);
  }
  return plan_igemm(q, d, ncu);
}

}  // namespace can
