// Geometry and launch plan of the NHWC resampling kernels (resample.hip): adaptive average pool and bilinear resize,
// forward and backward.  Pure functions of the problem shape and the CU count, host and device, no HIP calls.
//
// A thread's unit is one 16-byte channel octet, as in batchnorm.hip.  The resize kernels split the C / 8 octets into
// G = ceil(C / 256) channel groups of near-equal width TX <= 32; the pool kernels index (pixel, octet) flat.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace can {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_TX = 32;                 // octets of a channel group: 256 channels
constexpr int RS_FWD_UNITS = 1536;            // resize forward: 8-float units of the staged window (48 KiB of LDS: the
                                              // static limit is 64 KiB, and three such blocks still share a CU)
constexpr int RS_BWD_UNITS = 1024;            // resize backward: units of the vertical-adjoint row (32 KiB)
constexpr int RS_POOL_TABLE = 512;            // separable pool: column bins whose bounds fit the row pass's LDS table
constexpr int RS_MAX_SLICES = 64;             // resize backward: output-row slices (one fp32 partial each)
// the project's 32-bit indexing rule (ops/conv.py MAX_ELEMS_PER_LAUNCH): elements of one operand of a launch
constexpr long long RS_MAX_ELEMS = (1ll << 30) - (1ll << 24);

enum { POOL_AUTO = 0, POOL_DIRECT = 1, POOL_SEPARABLE = 2 };

// bin i of S over a length L: [floor(i L / S), ceil((i + 1) L / S)); 32-bit division where the product allows
RS_HD inline int rs_floor_div(int a, int L, int S) {
  const unsigned long long p = (unsigned long long)a * (unsigned)L;
  return (p >> 32) ? (int)(p / (unsigned)S) : (int)((unsigned)p / (unsigned)S);
}
RS_HD inline int rs_ceil_div(int a, int L, int S) {
  const unsigned long long p = (unsigned long long)a * (unsigned)L + (unsigned)(S - 1);
  return (p >> 32) ? (int)(p / (unsigned)S) : (int)((unsigned)p / (unsigned)S);
}
RS_HD inline int rs_bin_lo(int i, int L, int S) { return rs_floor_div(i, L, S); }
RS_HD inline int rs_bin_hi(int i, int L, int S) { return rs_ceil_div(i + 1, L, S); }

// channel group g of G over C8 octets: first octet and width (the geometry of batchnorm.hip's bn_group)
RS_HD inline void rs_group(int C8, int G, int g, int& o0, int& TX) {
  const int base = C8 / G, rem = C8 % G;
  o0 = g * base + (g < rem ? g : rem);
  TX = base + (g < rem ? 1 : 0);
}
inline int rs_groups(int C8) { return (C8 + RS_MAX_TX - 1) / RS_MAX_TX; }
inline int rs_txmax(int C8) { const int G = rs_groups(C8); return (C8 + G - 1) / G; }

// shape checks shared by the four entries: -2 channels, -3 a size below 1, -5 an operand beyond the indexing rule
inline int rs_check(long long N, long long H, long long W, long long C, long long oh, long long ow) {
  if (C <= 0 || (C & 7)) return -2;
  if (N < 1 || H < 1 || W < 1 || oh < 1 || ow < 1) return -3;
  if (H > RS_MAX_ELEMS || W > RS_MAX_ELEMS || oh > RS_MAX_ELEMS || ow > RS_MAX_ELEMS || N > RS_MAX_ELEMS) return -5;
  if (H * W > RS_MAX_ELEMS / C || N * H * W > RS_MAX_ELEMS / C) return -5;
  if (oh * ow > RS_MAX_ELEMS / C || N * oh * ow > RS_MAX_ELEMS / C) return -5;
  return 0;
}

// ---- adaptive average pool, forward
// Direct: a thread per (output cell, octet) walks its bin in row-major order.  Separable: a row pass (a block per image
// row; a thread per (column bin, octet) sums its columns in ascending order into fp32 rowacc [N][H][ow][C]) and a cell
// pass (a thread per (cell, octet) adds its bin's rows in ascending order).  The direct form has N oh ow C / 8 threads
// in all; the separable one is picked when that is under two 256-thread blocks per CU and a bin has at least four rows,
// i.e. when the direct form would leave the chip idle while each thread walks a long bin.
struct PoolPlan {
  int err, form;
  long long ws_floats;          // rowacc of the separable form
};
inline PoolPlan pool_plan(int N, int H, int W, int C, int oh, int ow, int form, int cus) {
  PoolPlan p{rs_check(N, H, W, C, oh, ow), POOL_DIRECT, 0};
  if (p.err) return p;
  if (form < POOL_AUTO || form > POOL_SEPARABLE) { p.err = -6; return p; }
  const long long sep_ws = (long long)N * H * ow * C;
  const bool sep_ok = ow <= RS_POOL_TABLE && sep_ws <= RS_MAX_ELEMS;
  if (form == POOL_SEPARABLE && !sep_ok) { p.err = -6; return p; }
  if (form == POOL_AUTO) {
    const long long threads = (long long)N * oh * ow * (C / 8);
    const int ncu = cus > 0 ? cus : 256;
    form = (sep_ok && threads < 2ll * RS_THREADS * ncu && (H + oh - 1) / oh >= 4) ? POOL_SEPARABLE : POOL_DIRECT;
  }
  p.form = form;
  p.ws_floats = form == POOL_SEPARABLE ? sep_ws : 0;
  return p;
}

// ---- bilinear resize, forward
// A block owns (sample, channel group, tr output rows, sw output columns).  Staged: the source rows the tile's taps
// reach (i0 of its first row .. i1 of its last, contiguous: the tap map is monotone) are blended horizontally to fp32
// once per source row into LDS [win][sw][TX][8], then every output row is a vertical blend of two LDS rows.  win = rows
// the LDS holds; a block whose window is taller reads global memory instead (same arithmetic, same bits).  Staging is
// planned where rows are reused, i.e. for a vertical upscale whose estimated window fits.
struct ResizeFwdPlan {
  int err, G, tr, sw, win, staged;
};
inline ResizeFwdPlan resize_fwd_plan(int N, int h, int w, int C, int oh, int ow, int staged /* -1: planned */) {
  ResizeFwdPlan p{rs_check(N, h, w, C, oh, ow), 0, 0, 0, 0, 0};
  if (p.err) return p;
  if (staged < -1 || staged > 1) { p.err = -6; return p; }
  const int C8 = C / 8, tx = rs_txmax(C8);
  p.G = rs_groups(C8);
  p.sw = RS_THREADS / tx;
  if (p.sw > 64) p.sw = 64;
  if (p.sw > ow) p.sw = ow;
  p.tr = oh < 8 ? oh : 8;
  p.win = RS_FWD_UNITS / (p.sw * tx);
  const long long need = ((long long)(p.tr - 1) * h) / oh + 3;        // rows a tile's taps span, at most
  p.staged = staged < 0 ? (oh > h && need <= p.win) : staged;
  if (p.win < 1) p.staged = 0;
  return p;
}

// ---- bilinear resize, backward
// A block owns (slice, sample, source row, channel group, TY = 256 / TX source columns), a thread one (source column,
// octet).  The output columns that touch the strip are walked in chunks of oc_cap: the block sums the vertical adjoint
// of a chunk over its output rows (ascending) into an fp32 LDS row, then each thread gathers its horizontal adjoint
// from that row (ascending).  S > 1: the output rows of every source row are cut into S slices, each block writes an
// fp32 partial, and a reduce launch adds the slices in order.  S is planned so that the blocks fill the CUs twice,
// bounded by the rows a source row can gather (about 2 oh / h).
struct ResizeBwdPlan {
  int err, G, ty, oc_cap, S;
  long long ws_floats;          // S > 1: partials [S][N][h][w][C]
};
inline ResizeBwdPlan resize_bwd_plan(int N, int h, int w, int C, int oh, int ow, int slices /* 0: planned */,
                                     int cus) {
  ResizeBwdPlan p{rs_check(N, h, w, C, oh, ow), 0, 0, 0, 1, 0};
  if (p.err) return p;
  if (slices < 0 || slices > RS_MAX_SLICES) { p.err = -6; return p; }
  const int C8 = C / 8, tx = rs_txmax(C8);
  p.G = rs_groups(C8);
  p.ty = RS_THREADS / tx;
  p.oc_cap = RS_BWD_UNITS / tx;
  long long S = slices;
  if (S == 0) {
    const long long blocks = (long long)N * h * ((w + p.ty - 1) / p.ty) * p.G;
    const long long want = 2ll * (cus > 0 ? cus : 256);
    const long long rows = 2ll * ((oh + h - 1) / h);
    S = (want + blocks - 1) / blocks;
    if (S > rows) S = rows;
    if (S > RS_MAX_SLICES) S = RS_MAX_SLICES;
    if (S < 1) S = 1;
  }
  const long long part = (long long)N * h * w * C;
  while (S > 1 && S * part > RS_MAX_ELEMS) --S;
  p.S = (int)S;
  p.ws_floats = S > 1 ? S * part : 0;
  return p;
}

}  // namespace can
