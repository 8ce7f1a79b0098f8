// Group / instance normalisation (+ ReLU) of an NHWC 16-bit map x[N][HW][C], forward and backward (gfx950):
// F.group_norm(x, G, gamma, beta, eps) with statistics per (sample, group of cg = C / G channels); cg = 1 is instance
// norm.  Bandwidth-bound.  No atomics, fixed summation order: bitwise repeatable.  Plans: groupnorm_plan.h.
//
// The one intermediate, in both directions and both forms, is a pair of double sums per (sample, channel): sum x and
// sum x^2 forward, S1 = sum dz and S2 = sum dz xhat backward.  Groups are folded from them afterwards (ascending
// channel), so the loops over pixels do not depend on cg: a thread's unit is one 16-byte channel octet whatever the
// group width, also for groups narrower than an octet (cg = 1, 2, 4), wider, or straddling octets (cg = 3).  Only the
// backward's per-channel coefficients (mean, rstd, c1, c2 of the channel's group) are looked up through c / cg, once
// per thread.
//
// Streamed form (any size), grid (channel span, pixel slice or row block, sample):
//   gn_stats_kernel / gn_bwd_stats_kernel   per-slice double partials part[N][S][2][C]; a 256-thread block is TX <= 32
//                        octets x TY = 256 / TX pixels, a thread keeps its octet and adds its pixels in ascending order
//   gn_finalize_kernel   block = (sample, whole groups of 16 channels or one wider group): sums the S slices of a channel in Q <= 16 chunks of
//                        consecutive slices, each in order, then the chunks in order; folds channels into groups;
//                        forward: stats[N][G][3], ab[N][2][C]; backward: c12[N][G][2], and the channel totals go back
//                        into slice 0 of part for gn_param_grad_kernel
//   gn_apply_kernel / gn_bwd_apply_kernel   coefficients per (sample, channel), loaded once per thread
// Resident form (a sample's [HW][bundle] tile fits the LDS), grid (bundle, sample), 512 threads:
//   gn_res_fwd_kernel    reads x from HBM once: stages the tile, reduces, folds, applies from LDS, writes y and stats
//   gn_res_bwd_kernel    stages x and dz (dy with the mask already applied), writes S1 / S2 per (n, c) to part[N][1][2][C]
//                        and produces dx in the same kernel
// gn_param_grad_kernel (both forms): dbeta_c = sum_n S1[n,c], dgamma_c = sum_n S2[n,c], ascending n, one fp32 rounding.
//
// Resident layout.  The bundle is the smallest multiple of lcm(cg, 8) channels that reaches 32 (a 64-byte run per
// pixel; at most 512, the last bundle of a map may be narrower), BX octets.  Thread t = py BX + ox stages pixels py,
// py + TY, ... of octet ox at tile[p BX + ox]: at every step the 512 threads write 512 consecutive 16-byte words, and
// the apply pass reads back exactly the words the same thread wrote -- consecutive ds_read_b128 per lane, free of bank
// conflicts, and the tile needs no barrier.  The statistics are NOT re-read from LDS: each thread adds its octets in
// double while it stages them.  The block then reduces over py in two rounds of 8 values (sums, then squares / S2)
// through red[8][512 + BX] doubles: the row pitch 512 + BX puts value k of octet ox at bank offset k BX + ox, so the
// 8 BX partial sums a wave reads side by side are consecutive doubles.  Rows are added in Q chunks of consecutive py
// in order, then the chunks in order (gn_block_reduce8, shared with the streamed statistics kernels).
//
// fp32 rounding steps (every other operation is exact or in double; the tests' bounds count these):
//   forward   mean, var, rstd: double, each rounded once.  (1) a = gamma * rstd, (2) b = fma(-mean, a, beta),
//             (3) fma(x, a, b), then the one 16-bit rounding (ReLU clamps before it).
//   backward  (1) x - mean, (2) (.) * rstd = xhat, (3) gamma * dz, (4) (.) - c1, (5) fma(-xhat, c2, .), (6) rstd * (.),
//             then the 16-bit rounding; c1, c2 (double sums of gamma_c S[n,c] over the group / (HW cg)) and dgamma,
//             dbeta are rounded once each.  The mask is read from the stored y (y > 0 on its 16-bit pattern).
#include "common.h"
#include "api.h"
#include "groupnorm_plan.h"
#include <algorithm>
#include <cmath>

namespace can {

constexpr int kGnFinTile = 1024;      // gn_finalize_kernel: channels summed per pass
constexpr int kGnFinGroups = 16;      // and groups per block (two threads each): whole groups that make up 16 channels

struct GnGeo {
  int o0, BX, TY, ox, py;             // first octet and width of the block's channels, rows per block, the thread's place
};
// streamed: span blockIdx.x of `spans` near-equal spans over C8 octets
__device__ __forceinline__ GnGeo gn_span(int C8, int spans) {
  const int g = blockIdx.x, base = C8 / spans, rem = C8 % spans;
  GnGeo r;
  r.o0 = g * base + min(g, rem);
  r.BX = base + (g < rem ? 1 : 0);
  r.TY = GN_THREADS / r.BX;
  r.ox = threadIdx.x % r.BX;
  r.py = threadIdx.x / r.BX;          // py >= TY: the block's idle tail
  return r;
}
// resident: bundle blockIdx.x of B8 octets (the last one may be narrower)
__device__ __forceinline__ GnGeo gn_bundle(int C8, int B8) {
  GnGeo r;
  r.o0 = blockIdx.x * B8;
  r.BX = min(B8, C8 - r.o0);
  r.TY = GN_RES_THREADS / r.BX;
  r.ox = threadIdx.x % r.BX;
  r.py = threadIdx.x / r.BX;
  return r;
}

// Block sum over py of acc[8] (one value per channel of the thread's octet) in index order, out[ox * 8 + k]; out may
// be LDS or global.  red: 8 (T + BX) doubles, red2: T doubles.  Ends with a barrier: red is free and out is visible.
template <int T>
__device__ __forceinline__ void gn_block_reduce8(const GnGeo& g, const double (&acc)[8], double* red, double* red2,
                                                 double* out) {
  const int t = threadIdx.x, RS = T + g.BX;
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k * RS + t] = acc[k];               // idle threads hold zeros and are never read
  __syncthreads();
  const int NO = 8 * g.BX;                                            // outputs o = k * BX + ox
  const int Q = NO >= T ? 1 : T / NO;                                 // row chunks summed side by side
  const int R = (g.TY + Q - 1) / Q;
  for (int i = t; i < NO * Q; i += T) {
    const int o = i % NO, q = i / NO, k = o / g.BX, ox = o - k * g.BX;
    const int r1 = min(g.TY, (q + 1) * R);
    double s = 0.0;
    for (int r = q * R; r < r1; ++r) s += red[k * RS + r * g.BX + ox];
    red2[q * NO + o] = s;
  }
  __syncthreads();
  for (int o = t; o < NO; o += T) {
    double s = 0.0;
    for (int q = 0; q < Q; ++q) s += red2[q * NO + o];
    const int k = o / g.BX, ox = o - k * g.BX;
    out[ox * 8 + k] = s;
  }
  __syncthreads();
}

template <int DT>
__device__ __forceinline__ void gn_acc_x(const uint4& v, double (&s1)[8], double (&s2)[8]) {
  float f[8];
  unpack8h<DT>(v, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double d = (double)f[k];                  // x and x^2 of a 16-bit value are exact in double
    s1[k] += d;
    s2[k] = fma(d, d, s2[k]);
  }
}

// mean / biased var / rstd of a group from its double sums: IEEE divide and sqrt in double, each rounded to fp32 once
__device__ __forceinline__ void gn_mean_rstd(double s0, double s1, double cnt, double eps, float& meanf, float& varf,
                                             float& rstdf) {
#pragma clang fp contract(off)
  const double mean = s0 / cnt;
  const double var = fmax(0.0, s1 / cnt - mean * mean);
  meanf = (float)mean;
  varf = (float)var;
  rstdf = (float)(1.0 / sqrt(var + eps));
}

__device__ __forceinline__ void gn_load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

template <int DT, bool RELU>
__device__ __forceinline__ uint4 gn_apply8(const uint4& v, const float (&a)[8], const float (&b)[8]) {
  float f[8];
  unpack8h<DT>(v, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = __fmaf_rn(f[k], a[k], b[k]);
    if constexpr (RELU) f[k] = f[k] < 0.f ? 0.f : f[k];
  }
  return pack8h<DT>(f);
}

// dy with the 16-bit halves cleared where the stored y is not > 0
__device__ __forceinline__ uint4 gn_mask8(const uint4& dyv, const uint4& yv) {
  const unsigned d[4] = {dyv.x, dyv.y, dyv.z, dyv.w}, w[4] = {yv.x, yv.y, yv.z, yv.w};
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = (pos_bits((unsigned short)(w[i] & 0xffffu)) ? (d[i] & 0xffffu) : 0u) |
           (pos_bits((unsigned short)(w[i] >> 16)) ? (d[i] & 0xffff0000u) : 0u);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// the backward's per-channel values of a thread's octet
struct GnBwdCoef {
  float mean[8], rstd[8], gam[8];
};
__device__ __forceinline__ void gn_bwd_coef(const float* __restrict__ gamma, const float* __restrict__ stats_n, int oct,
                                            int cg, GnBwdCoef& q) {
  gn_load8(gamma + oct * 8, q.gam);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int g = (oct * 8 + k) / cg;
    q.mean[k] = stats_n[3 * g];
    q.rstd[k] = stats_n[3 * g + 2];
  }
}

// dz[8] from the masked dy, xh[8] = (x - mean) * rstd in fp32 (two roundings)
template <int DT>
__device__ __forceinline__ void gn_dz_xhat(const uint4& dzv, const uint4& xv, const GnBwdCoef& q, float (&dz)[8],
                                           float (&xh)[8]) {
  float xf[8];
  unpack8h<DT>(dzv, dz);
  unpack8h<DT>(xv, xf);
#pragma unroll
  for (int k = 0; k < 8; ++k) xh[k] = __fmul_rn(__fsub_rn(xf[k], q.mean[k]), q.rstd[k]);
}

template <int DT>
__device__ __forceinline__ void gn_acc_dz(const uint4& dzv, const uint4& xv, const GnBwdCoef& q, double (&s1)[8],
                                          double (&s2)[8]) {
  float dz[8], xh[8];
  gn_dz_xhat<DT>(dzv, xv, q, dz, xh);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double d = (double)dz[k];
    s1[k] += d;
    s2[k] = fma(d, (double)xh[k], s2[k]);           // the product of two fp32 values is exact in double
  }
}

// dx = f2h(rstd * (gamma * dz - c1 - xhat * c2))
template <int DT>
__device__ __forceinline__ uint4 gn_dx8(const uint4& dzv, const uint4& xv, const GnBwdCoef& q, const float (&c1)[8],
                                        const float (&c2)[8]) {
  float dz[8], xh[8], o[8];
  gn_dz_xhat<DT>(dzv, xv, q, dz, xh);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    o[k] = __fmul_rn(q.rstd[k], __fmaf_rn(-xh[k], c2[k], __fsub_rn(__fmul_rn(q.gam[k], dz[k]), c1[k])));
  return pack8h<DT>(o);
}

// ---- streamed form
template <int DT>
__global__ void __launch_bounds__(GN_THREADS) gn_stats_kernel(const uint4* __restrict__ x, double* __restrict__ part,
                                                              long long HW, long long pslice, int C8, int spans) {
  __shared__ double red[8 * (GN_THREADS + GN_MAX_TX)];
  __shared__ double red2[GN_THREADS];
  const GnGeo g = gn_span(C8, spans);
  const int n = blockIdx.z;
  double s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.0;
  if (g.py < g.TY) {
    const long long p1 = min(HW, ((long long)blockIdx.y + 1) * pslice), st = g.TY;
    const uint4* xo = x + (size_t)n * HW * C8 + g.o0 + g.ox;
    long long p = (long long)blockIdx.y * pslice + g.py;
    // four loads in flight per thread; the adds keep pixel order
    for (; p + 3 * st < p1; p += 4 * st) {
      const uint4 v0 = xo[(size_t)p * C8], v1 = xo[(size_t)(p + st) * C8], v2 = xo[(size_t)(p + 2 * st) * C8],
                  v3 = xo[(size_t)(p + 3 * st) * C8];
      gn_acc_x<DT>(v0, s1, s2); gn_acc_x<DT>(v1, s1, s2); gn_acc_x<DT>(v2, s1, s2); gn_acc_x<DT>(v3, s1, s2);
    }
    for (; p < p1; p += st) gn_acc_x<DT>(xo[(size_t)p * C8], s1, s2);
  }
  const size_t C = (size_t)C8 * 8;
  double* out = part + (((size_t)n * gridDim.y + blockIdx.y) * 2) * C + (size_t)g.o0 * 8;
  gn_block_reduce8<GN_THREADS>(g, s1, red, red2, out);
  gn_block_reduce8<GN_THREADS>(g, s2, red, red2, out + C);
}

template <int DT, bool RELU>
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_stats_kernel(const uint4* __restrict__ dy,
                                                                  const uint4* __restrict__ x,
                                                                  const uint4* __restrict__ y,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ stats,
                                                                  double* __restrict__ part, long long HW,
                                                                  long long pslice, int C8, int spans, int cg) {
  __shared__ double red[8 * (GN_THREADS + GN_MAX_TX)];
  __shared__ double red2[GN_THREADS];
  const GnGeo g = gn_span(C8, spans);
  const int n = blockIdx.z;
  const size_t C = (size_t)C8 * 8;
  double s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.0;
  if (g.py < g.TY) {
    const int oct = g.o0 + g.ox;
    GnBwdCoef q;
    gn_bwd_coef(gamma, stats + (size_t)n * (C / cg) * 3, oct, cg, q);
    const long long p1 = min(HW, ((long long)blockIdx.y + 1) * pslice), st = g.TY;
    const size_t base = (size_t)n * HW * C8 + oct;
    long long p = (long long)blockIdx.y * pslice + g.py;
    for (; p + st < p1; p += 2 * st) {
      const size_t i0 = base + (size_t)p * C8, i1 = base + (size_t)(p + st) * C8;
      uint4 d0 = dy[i0], d1 = dy[i1];
      const uint4 x0 = x[i0], x1 = x[i1];
      if constexpr (RELU) { d0 = gn_mask8(d0, y[i0]); d1 = gn_mask8(d1, y[i1]); }
      gn_acc_dz<DT>(d0, x0, q, s1, s2);
      gn_acc_dz<DT>(d1, x1, q, s1, s2);
    }
    for (; p < p1; p += st) {
      const size_t i0 = base + (size_t)p * C8;
      uint4 d0 = dy[i0];
      if constexpr (RELU) d0 = gn_mask8(d0, y[i0]);
      gn_acc_dz<DT>(d0, x[i0], q, s1, s2);
    }
  }
  double* out = part + (((size_t)n * gridDim.y + blockIdx.y) * 2) * C + (size_t)g.o0 * 8;
  gn_block_reduce8<GN_THREADS>(g, s1, red, red2, out);
  gn_block_reduce8<GN_THREADS>(g, s2, red, red2, out + C);
}

// Block (blockIdx.x, n): groups [g0, g0 + ng) of sample n, ng <= gpb = max(1, 16 / cg), their channels in passes of 1024
// (16 channels x 16 slice chunks keep the 256 threads busy, and a map of few channels still gets C / 16 blocks a sample).
//   forward:  part = sums of x, x^2; stats[n][g] = (mean, biased var, rstd); coef = ab[N][2][C]: a = gamma * rstd,
//             b = fma(-mean, a, beta), both from the ROUNDED mean and rstd.
//   backward: part = S1, S2; the channel totals are written to slice 0 of the sample (every slice of these channels
//             has been read by then, and no other block touches them); coef = c12[N][G][2]:
//             c_i[n][g] = sum_{c in g} gamma_c S_i[n][c] / cnt, ascending c in double, rounded once.
template <bool BWD>
__global__ void __launch_bounds__(GN_THREADS) gn_finalize_kernel(double* __restrict__ part, int S, int C, int cg, int gpb,
                                                                 double cnt, double eps,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 float* __restrict__ stats, float* __restrict__ coef) {
#pragma clang fp contract(off)
  __shared__ double red[2][kGnFinTile];
  __shared__ double tot[2][kGnFinTile];
  const int t = threadIdx.x, n = blockIdx.y, G = C / cg;
  const int g0 = blockIdx.x * gpb, ng = min(gpb, G - g0), c0 = g0 * cg, nch = ng * cg;
  double* pn = part + (size_t)n * S * 2 * C;
  const int gl = t >> 1, k = t & 1;                 // the fold: thread (group gl, statistic k) keeps its sum across passes
  double acc = 0.0;
  for (int tile0 = 0; tile0 < nch; tile0 += kGnFinTile) {
    const int tw = min(kGnFinTile, nch - tile0);
    const int Q = max(1, min(min(kGnFinTile / tw, 16), S)), R = (S + Q - 1) / Q;
    for (int u = t; u < tw * Q; u += GN_THREADS) {
      const int c = u % tw, q = u / tw, e = min(S, (q + 1) * R);
      const double* pc = pn + c0 + tile0 + c;
      double s0 = 0.0, s1 = 0.0;
      for (int s = q * R; s < e; ++s) {
        s0 += pc[((size_t)s * 2) * C];
        s1 += pc[((size_t)s * 2 + 1) * C];
      }
      red[0][u] = s0;
      red[1][u] = s1;
    }
    __syncthreads();
    for (int c = t; c < tw; c += GN_THREADS) {
      double s0 = 0.0, s1 = 0.0;
      for (int q = 0; q < Q; ++q) { s0 += red[0][q * tw + c]; s1 += red[1][q * tw + c]; }
      tot[0][c] = s0;
      tot[1][c] = s1;
      if constexpr (BWD) {
        pn[c0 + tile0 + c] = s0;
        pn[(size_t)C + c0 + tile0 + c] = s1;
      }
    }
    __syncthreads();
    if (gl < ng) {
      const int lo = max(gl * cg, tile0), hi = min((gl + 1) * cg, tile0 + tw);
      for (int c = lo; c < hi; ++c) {
        double v = tot[k][c - tile0];
        if constexpr (BWD) v *= (double)gamma[c0 + c];
        acc += v;
      }
    }
    __syncthreads();
  }
  double* gs = &red[0][0];                          // [2][16] group sums
  if (gl < ng) gs[k * kGnFinGroups + gl] = acc;
  __syncthreads();
  if constexpr (BWD) {
    if (t < ng) {
      float* o = coef + ((size_t)n * G + g0 + t) * 2;
      o[0] = (float)(gs[t] / cnt);
      o[1] = (float)(gs[kGnFinGroups + t] / cnt);
    }
  } else {
    float* gm = reinterpret_cast<float*>(&tot[0][0]);
    float* gr = gm + kGnFinGroups;
    if (t < ng) {
      float meanf, varf, rstdf;
      gn_mean_rstd(gs[t], gs[kGnFinGroups + t], cnt, eps, meanf, varf, rstdf);
      float* o = stats + ((size_t)n * G + g0 + t) * 3;
      o[0] = meanf; o[1] = varf; o[2] = rstdf;
      gm[t] = meanf;
      gr[t] = rstdf;
    }
    __syncthreads();
    for (int c = t; c < nch; c += GN_THREADS) {
      const int j = c / cg;
      const float a = __fmul_rn(gamma[c0 + c], gr[j]);
      coef[((size_t)n * 2) * C + c0 + c] = a;
      coef[((size_t)n * 2 + 1) * C + c0 + c] = __fmaf_rn(-gm[j], a, beta[c0 + c]);
    }
  }
}

// y = f2h(fma(x, a, b)) [clamped at 0]; blockIdx.y strides over the sample's pixels
template <int DT, bool RELU>
__global__ void __launch_bounds__(GN_THREADS) gn_apply_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                              const float* __restrict__ ab, long long HW, int C8,
                                                              int spans) {
  const GnGeo g = gn_span(C8, spans);
  if (g.py >= g.TY) return;
  const int n = blockIdx.z, oct = g.o0 + g.ox;
  const size_t C = (size_t)C8 * 8;
  float a[8], b[8];
  gn_load8(ab + (size_t)n * 2 * C + oct * 8, a);
  gn_load8(ab + ((size_t)n * 2 + 1) * C + oct * 8, b);
  const long long st = (long long)gridDim.y * g.TY;
  const size_t base = (size_t)n * HW * C8 + oct;
  const uint4* xo = x + base;
  uint4* yo = y + base;
  long long p = (long long)blockIdx.y * g.TY + g.py;
  for (; p + 3 * st < HW; p += 4 * st) {
    const uint4 v0 = xo[(size_t)p * C8], v1 = xo[(size_t)(p + st) * C8], v2 = xo[(size_t)(p + 2 * st) * C8],
                v3 = xo[(size_t)(p + 3 * st) * C8];
    yo[(size_t)p * C8] = gn_apply8<DT, RELU>(v0, a, b);
    yo[(size_t)(p + st) * C8] = gn_apply8<DT, RELU>(v1, a, b);
    yo[(size_t)(p + 2 * st) * C8] = gn_apply8<DT, RELU>(v2, a, b);
    yo[(size_t)(p + 3 * st) * C8] = gn_apply8<DT, RELU>(v3, a, b);
  }
  for (; p < HW; p += st) yo[(size_t)p * C8] = gn_apply8<DT, RELU>(xo[(size_t)p * C8], a, b);
}

template <int DT, bool RELU>
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_apply_kernel(const uint4* __restrict__ dy,
                                                                  const uint4* __restrict__ x,
                                                                  const uint4* __restrict__ y,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ c12,
                                                                  uint4* __restrict__ dx, long long HW, int C8,
                                                                  int spans, int cg) {
  const GnGeo g = gn_span(C8, spans);
  if (g.py >= g.TY) return;
  const int n = blockIdx.z, oct = g.o0 + g.ox, G = C8 * 8 / cg;
  GnBwdCoef q;
  gn_bwd_coef(gamma, stats + (size_t)n * G * 3, oct, cg, q);
  float c1[8], c2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float* c = c12 + ((size_t)n * G + (oct * 8 + k) / cg) * 2;
    c1[k] = c[0];
    c2[k] = c[1];
  }
  const long long st = (long long)gridDim.y * g.TY;
  const size_t base = (size_t)n * HW * C8 + oct;
  long long p = (long long)blockIdx.y * g.TY + g.py;
  for (; p + st < HW; p += 2 * st) {
    const size_t i0 = base + (size_t)p * C8, i1 = base + (size_t)(p + st) * C8;
    uint4 d0 = dy[i0], d1 = dy[i1];
    const uint4 x0 = x[i0], x1 = x[i1];
    if constexpr (RELU) { d0 = gn_mask8(d0, y[i0]); d1 = gn_mask8(d1, y[i1]); }
    dx[i0] = gn_dx8<DT>(d0, x0, q, c1, c2);
    dx[i1] = gn_dx8<DT>(d1, x1, q, c1, c2);
  }
  for (; p < HW; p += st) {
    const size_t i0 = base + (size_t)p * C8;
    uint4 d0 = dy[i0];
    if constexpr (RELU) d0 = gn_mask8(d0, y[i0]);
    dx[i0] = gn_dx8<DT>(d0, x[i0], q, c1, c2);
  }
}

// dgb[2][C] = (dgamma, dbeta) from the per-sample channel totals part[n * nstride + (0: S1, 1: S2) * C + c]
__global__ void __launch_bounds__(GN_THREADS) gn_param_grad_kernel(const double* __restrict__ part, size_t nstride,
                                                                   int N, int C, float* __restrict__ dgb) {
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= 2 * C) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += part[(size_t)n * nstride + i];
  dgb[i < C ? C + i : i - C] = (float)s;
}

// ---- resident form
// dynamic LDS: tile(s) [HW][BX] uint4, then red [8][T + BX], red2 [T], cs [2][8 BX] doubles, fv [4][8 BX] floats
struct GnResLds {
  double *red, *red2, *cs;
  float* fv;
};
__device__ __forceinline__ GnResLds gn_res_lds(uint4* after_tiles, int BX) {
  GnResLds l;
  l.red = reinterpret_cast<double*>(after_tiles);
  l.red2 = l.red + 8 * (GN_RES_THREADS + BX);
  l.cs = l.red2 + GN_RES_THREADS;
  l.fv = reinterpret_cast<float*>(l.cs + 16 * BX);
  return l;
}

template <int DT, bool RELU>
__global__ void __launch_bounds__(GN_RES_THREADS) gn_res_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta,
                                                                    float* __restrict__ stats, int HW, int C8, int cg,
                                                                    int B8, double eps) {
  extern __shared__ uint4 gn_smem[];
  const GnGeo g = gn_bundle(C8, B8);
  const int t = threadIdx.x, n = blockIdx.y, nch = 8 * g.BX, ng = nch / cg, G = C8 * 8 / cg;
  uint4* tile = gn_smem;
  const GnResLds l = gn_res_lds(tile + (size_t)HW * g.BX, g.BX);
  const size_t base = (size_t)n * HW * C8 + g.o0 + g.ox;
  double s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.0;
  if (g.py < g.TY) {
    const int st = g.TY;
    const uint4* xo = x + base;
    uint4* to = tile + g.ox;
    int p = g.py;
    for (; p + 3 * st < HW; p += 4 * st) {
      const uint4 v0 = xo[(size_t)p * C8], v1 = xo[(size_t)(p + st) * C8], v2 = xo[(size_t)(p + 2 * st) * C8],
                  v3 = xo[(size_t)(p + 3 * st) * C8];
      to[p * g.BX] = v0; to[(p + st) * g.BX] = v1; to[(p + 2 * st) * g.BX] = v2; to[(p + 3 * st) * g.BX] = v3;
      gn_acc_x<DT>(v0, s1, s2); gn_acc_x<DT>(v1, s1, s2); gn_acc_x<DT>(v2, s1, s2); gn_acc_x<DT>(v3, s1, s2);
    }
    for (; p < HW; p += st) {
      const uint4 v0 = xo[(size_t)p * C8];
      to[p * g.BX] = v0;
      gn_acc_x<DT>(v0, s1, s2);
    }
  }
  gn_block_reduce8<GN_RES_THREADS>(g, s1, l.red, l.red2, l.cs);
  gn_block_reduce8<GN_RES_THREADS>(g, s2, l.red, l.red2, l.cs + nch);
  // fold: thread (group j, statistic k) adds its cg channel sums in ascending order (2 ng <= 112 threads)
  if (t < 2 * ng) {
    const int j = t >> 1, k = t & 1;
    const double* c = l.cs + k * nch + j * cg;
    double acc = 0.0;
    for (int i = 0; i < cg; ++i) acc += c[i];
    l.red2[k * 64 + j] = acc;
  }
  __syncthreads();
  float *gm = l.fv, *gr = l.fv + nch, *ca = l.fv + 2 * nch, *cb = l.fv + 3 * nch;
  if (t < ng) {
    float meanf, varf, rstdf;
    gn_mean_rstd(l.red2[t], l.red2[64 + t], (double)HW * cg, eps, meanf, varf, rstdf);
    float* o = stats + ((size_t)n * G + (g.o0 * 8) / cg + t) * 3;
    o[0] = meanf; o[1] = varf; o[2] = rstdf;
    gm[t] = meanf;
    gr[t] = rstdf;
  }
  __syncthreads();
  for (int c = t; c < nch; c += GN_RES_THREADS) {
    const int j = c / cg;
    const float a = __fmul_rn(gamma[g.o0 * 8 + c], gr[j]);
    ca[c] = a;
    cb[c] = __fmaf_rn(-gm[j], a, beta[g.o0 * 8 + c]);
  }
  __syncthreads();
  if (g.py >= g.TY) return;
  float a[8], b[8];
  gn_load8(ca + g.ox * 8, a);
  gn_load8(cb + g.ox * 8, b);
  uint4* yo = y + base;
  const uint4* to = tile + g.ox;
  for (int p = g.py; p < HW; p += g.TY) yo[(size_t)p * C8] = gn_apply8<DT, RELU>(to[p * g.BX], a, b);
}

template <int DT, bool RELU>
__global__ void __launch_bounds__(GN_RES_THREADS) gn_res_bwd_kernel(const uint4* __restrict__ dy,
                                                                    const uint4* __restrict__ x,
                                                                    const uint4* __restrict__ y,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ stats,
                                                                    double* __restrict__ part, uint4* __restrict__ dx,
                                                                    int HW, int C8, int cg, int B8) {
#pragma clang fp contract(off)
  extern __shared__ uint4 gn_smem[];
  const GnGeo g = gn_bundle(C8, B8);
  const int t = threadIdx.x, n = blockIdx.y, nch = 8 * g.BX, ng = nch / cg, C = C8 * 8, G = C / cg;
  uint4* tx = gn_smem;
  uint4* td = tx + (size_t)HW * g.BX;
  const GnResLds l = gn_res_lds(td + (size_t)HW * g.BX, g.BX);
  const size_t base = (size_t)n * HW * C8 + g.o0 + g.ox;
  GnBwdCoef q;
  double s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.0;
  if (g.py < g.TY) {
    gn_bwd_coef(gamma, stats + (size_t)n * G * 3, g.o0 + g.ox, cg, q);
    const int st = g.TY;
    int p = g.py;
    for (; p + st < HW; p += 2 * st) {
      const size_t i0 = base + (size_t)p * C8, i1 = base + (size_t)(p + st) * C8;
      uint4 d0 = dy[i0], d1 = dy[i1];
      const uint4 x0 = x[i0], x1 = x[i1];
      if constexpr (RELU) { d0 = gn_mask8(d0, y[i0]); d1 = gn_mask8(d1, y[i1]); }
      tx[p * g.BX + g.ox] = x0; td[p * g.BX + g.ox] = d0;
      tx[(p + st) * g.BX + g.ox] = x1; td[(p + st) * g.BX + g.ox] = d1;
      gn_acc_dz<DT>(d0, x0, q, s1, s2);
      gn_acc_dz<DT>(d1, x1, q, s1, s2);
    }
    for (; p < HW; p += st) {
      const size_t i0 = base + (size_t)p * C8;
      uint4 d0 = dy[i0];
      const uint4 x0 = x[i0];
      if constexpr (RELU) d0 = gn_mask8(d0, y[i0]);
      tx[p * g.BX + g.ox] = x0; td[p * g.BX + g.ox] = d0;
      gn_acc_dz<DT>(d0, x0, q, s1, s2);
    }
  }
  gn_block_reduce8<GN_RES_THREADS>(g, s1, l.red, l.red2, l.cs);
  gn_block_reduce8<GN_RES_THREADS>(g, s2, l.red, l.red2, l.cs + nch);
  // S1 / S2 per (n, c) for the parameter gradients, and the group terms c1 / c2 (ascending c)
  for (int i = t; i < 2 * nch; i += GN_RES_THREADS) {
    const int k = i / nch, c = i - k * nch;
    part[((size_t)n * 2 + k) * C + g.o0 * 8 + c] = l.cs[i];
  }
  float *c1s = l.fv, *c2s = l.fv + nch;
  if (t < 2 * ng) {
    const int j = t >> 1, k = t & 1;
    const double* c = l.cs + k * nch + j * cg;
    const float* gc = gamma + g.o0 * 8 + j * cg;
    double acc = 0.0;
    for (int i = 0; i < cg; ++i) acc += (double)gc[i] * c[i];
    (k ? c2s : c1s)[j] = (float)(acc / ((double)HW * cg));
  }
  __syncthreads();
  if (g.py >= g.TY) return;
  float c1[8], c2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int j = (g.ox * 8 + k) / cg;
    c1[k] = c1s[j];
    c2[k] = c2s[j];
  }
  for (int p = g.py; p < HW; p += g.TY)
    dx[base + (size_t)p * C8] = gn_dx8<DT>(td[p * g.BX + g.ox], tx[p * g.BX + g.ox], q, c1, c2);
}

// ---- host side
static int gn_cus() {
  const int n = can_device_cus();
  return n > 0 ? n : 256;
}

// -20 the element type; the shape and request checks are gn_plan's
static GnPlan gn_checked_plan(int N, int H, int W, int C, int G, int backward, int form, int slices, int dt) {
  GnPlan p = gn_plan(N, H, W, C, G, backward, form, slices, gn_cus());
  if (!p.err && dt != DT_BF16 && dt != DT_F16) p.err = -20;
  return p;
}

#define GN_DISPATCH(dt, relu, F, ...)                                                  \
  ((dt) == DT_F16 ? ((relu) ? F<DT_F16, true>(__VA_ARGS__) : F<DT_F16, false>(__VA_ARGS__)) \
                  : ((relu) ? F<DT_BF16, true>(__VA_ARGS__) : F<DT_BF16, false>(__VA_ARGS__)))

template <int DT, bool RELU>
static int gn_launch_res_fwd(const GnPlan& p, hipStream_t s, const void* x, void* y, const float* gamma,
                             const float* beta, float* stats, int N, int HW, int C, int G, double eps) {
  auto kfn = gn_res_fwd_kernel<DT, RELU>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GN_LDS_BYTES));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3((C + p.bundle - 1) / p.bundle, N), dim3(GN_RES_THREADS), (size_t)p.lds, s,
                     (const uint4*)x, (uint4*)y, gamma, beta, stats, HW, C / 8, C / G, p.bundle / 8, eps);
  return (int)hipGetLastError();
}

template <int DT, bool RELU>
static int gn_launch_res_bwd(const GnPlan& p, hipStream_t s, const void* dy, const void* x, const void* y,
                             const float* gamma, const float* stats, double* part, void* dx, int N, int HW, int C,
                             int G) {
  auto kfn = gn_res_bwd_kernel<DT, RELU>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GN_LDS_BYTES));
    attr = true;
  }
  hipLaunchKernelGGL(kfn, dim3((C + p.bundle - 1) / p.bundle, N), dim3(GN_RES_THREADS), (size_t)p.lds, s,
                     (const uint4*)dy, (const uint4*)x, (const uint4*)y, gamma, stats, part, (uint4*)dx, HW, C / 8,
                     C / G, p.bundle / 8);
  return (int)hipGetLastError();
}

template <int DT, bool RELU>
static int gn_launch_apply(dim3 grid, hipStream_t s, const void* x, void* y, const float* ab, long long HW, int C8,
                           int spans) {
  hipLaunchKernelGGL((gn_apply_kernel<DT, RELU>), grid, dim3(GN_THREADS), 0, s, (const uint4*)x, (uint4*)y, ab, HW, C8,
                     spans);
  return 0;
}

template <int DT, bool RELU>
static int gn_launch_bwd_streamed(const GnPlan& p, dim3 rows, hipStream_t s, const void* dy, const void* x,
                                  const void* y, const float* gamma, const float* stats, double* part, float* c12,
                                  void* dx, int N, long long HW, int C, int G) {
  const int cg = C / G, gpb = std::max(1, kGnFinGroups / cg);
  hipLaunchKernelGGL((gn_bwd_stats_kernel<DT, RELU>), dim3(p.spans, p.S, N), dim3(GN_THREADS), 0, s, (const uint4*)dy,
                     (const uint4*)x, (const uint4*)y, gamma, stats, part, HW, (HW + p.S - 1) / p.S, C / 8, p.spans,
                     cg);
  hipLaunchKernelGGL(gn_finalize_kernel<true>, dim3((G + gpb - 1) / gpb, N), dim3(GN_THREADS), 0, s, part, p.S, C, cg,
                     gpb, (double)HW * cg, 0.0, gamma, (const float*)nullptr, (float*)nullptr, c12);
  hipLaunchKernelGGL((gn_bwd_apply_kernel<DT, RELU>), rows, dim3(GN_THREADS), 0, s, (const uint4*)dy, (const uint4*)x,
                     (const uint4*)y, gamma, stats, (const float*)c12, (uint4*)dx, HW, C / 8, p.spans, cg);
  return 0;
}

}  // namespace can

using namespace can;

extern "C" int can_gn_plan(int N, int H, int W, int C, int G, int backward, int form, int slices, int* out4,
                           long long* lds) {
  const GnPlan p = gn_plan(N, H, W, C, G, backward, form, slices, gn_cus());
  if (p.err) return p.err;
  if (out4) { out4[0] = p.form; out4[1] = p.S; out4[2] = p.bundle; out4[3] = p.spans; }
  if (lds) *lds = p.lds;
  return 0;
}

extern "C" int can_gn_forward(const void* x, void* y, const float* gamma, const float* beta, double* part, float* ab,
                              float* stats, int N, int H, int W, int C, int G, double eps, int relu, int dt, int form,
                              int slices, void* stream) {
  const GnPlan p = gn_checked_plan(N, H, W, C, G, 0, form, slices, dt);
  if (p.err) return p.err;
  if (!(eps >= 0.0) || !std::isfinite(eps)) return -4;
  if (x == nullptr || y == nullptr || gamma == nullptr || beta == nullptr || stats == nullptr) return -7;
  hipStream_t s = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  if (p.form == GN_RESIDENT)
    return GN_DISPATCH(dt, relu, gn_launch_res_fwd, p, s, x, y, gamma, beta, stats, N, (int)HW, C, G, eps);
  if (part == nullptr || ab == nullptr) return -6;
  const int cg = C / G, gpb = std::max(1, kGnFinGroups / cg);
  CAN_LAUNCH_DT(dt, gn_stats_kernel, dim3(p.spans, p.S, N), dim3(GN_THREADS), 0, s, (const uint4*)x, part, HW,
                (HW + p.S - 1) / p.S, C / 8, p.spans);
  hipLaunchKernelGGL(gn_finalize_kernel<false>, dim3((G + gpb - 1) / gpb, N), dim3(GN_THREADS), 0, s, part, p.S, C, cg,
                     gpb, (double)HW * cg, eps, gamma, beta, stats, ab);
  GN_DISPATCH(dt, relu, gn_launch_apply, dim3(p.spans, gn_apply_rows(N, HW, p, gn_cus()), N), s, x, y, ab, HW, C / 8,
              p.spans);
  return (int)hipGetLastError();
}

extern "C" int can_gn_backward(const void* dy, const void* x, const void* y, const float* gamma, const float* stats,
                               double* part, float* c12, float* dgb, void* dx, int N, int H, int W, int C, int G,
                               int relu, int dt, int form, int slices, void* stream) {
  const GnPlan p = gn_checked_plan(N, H, W, C, G, 1, form, slices, dt);
  if (p.err) return p.err;
  if (dy == nullptr || x == nullptr || (relu && y == nullptr) || gamma == nullptr || stats == nullptr ||
      dgb == nullptr || dx == nullptr)
    return -7;
  if (part == nullptr || (p.form == GN_STREAMED && c12 == nullptr)) return -6;
  hipStream_t s = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  if (p.form == GN_RESIDENT) {
    const int rc = GN_DISPATCH(dt, relu, gn_launch_res_bwd, p, s, dy, x, y, gamma, stats, part, dx, N, (int)HW, C, G);
    if (rc) return rc;
  } else {
    GN_DISPATCH(dt, relu, gn_launch_bwd_streamed, p, dim3(p.spans, gn_apply_rows(N, HW, p, gn_cus()), N), s, dy, x, y,
                gamma, stats, part, c12, dx, N, HW, C, G);
  }
  hipLaunchKernelGGL(gn_param_grad_kernel, dim3((2 * C + GN_THREADS - 1) / GN_THREADS), dim3(GN_THREADS), 0, s,
                     (const double*)part, (size_t)p.S * 2 * C, N, C, dgb);
  return (int)hipGetLastError();
}
