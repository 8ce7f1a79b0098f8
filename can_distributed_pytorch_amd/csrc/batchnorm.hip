// Batch normalisation (+ ReLU) of an NHWC 16-bit map x[M][C], M = N*H*W, forward and backward (gfx950): the layer
// between a conv and the pool in every *-BN backbone (nn.BatchNorm2d + ReLU, make_layers(batch_norm=True)).
// Bandwidth-bound: the design target is the HBM rate.  No atomics, fixed summation order: bitwise repeatable.
//
//   bn_stats_kernel      training forward, pass 1: per-slice double partials of sum x, sum x^2 per channel
//   bn_finalize_kernel   partials (or the running statistics, eval) -> fp32 stats (mean, biased var, rstd) and the folded
//                        coefficients a = gamma * rstd, b = fma(-mean, a, beta); backward: dgamma, dbeta, c1, c2
//   bn_apply_kernel      y = f2h(fma(x, a, b)), clamped at 0 with ReLU
//   bn_bwd_stats_kernel  backward pass 1: partials of sum dz, sum dz * xhat (dz = dy where the stored y > 0)
//   bn_bwd_apply_kernel  dx = a * (dz - c1 - xhat * c2) (training), a * dz (eval)
//
// Geometry, shared by the four streaming kernels.  A thread's unit is one 16-byte channel octet.  The C / 8 octets are
// split into G = ceil(C / 256) channel groups of near-equal width TX <= 32 (blockIdx.x); a 256-thread block is TX
// octets (tx, fastest) x TY = 256 / TX pixels (ty), so thread t reads octet t of a contiguous run of TY pixels when the
// map has one group (C = 8: 256 adjacent pixels; C = 24: tx = 3, 85 pixels, one thread idle) and 16 * TX contiguous
// bytes per pixel otherwise.  A thread keeps its octet for the whole launch: per-channel coefficients are loaded once,
// and all sums of a channel octet stay in its registers.
//
// Reductions.  A thread adds its pixels (ty, ty + TY, ...) in double from the first add: x and x^2 of a 16-bit value
// are exact in double, fma(d, d, s) rounds once.  The block then reduces over ty through LDS in index order, in two
// steps that use all 256 threads (row chunks in order, then the chunks in order), and writes one double per (slice,
// statistic, channel): part[S][2][C].  blockIdx.y = pixel slice s of S, pixels [s * ceil(M / S), (s + 1) * ceil(M / S)).
// bn_finalize_kernel sums the S partials of a channel in 16 chunks of consecutive slices, each in index order, then
// the chunks in order.  The order depends on (M, C, S) only.
//
// The backward mask is read from the stored y (y > 0 on its 16-bit pattern), not recomputed from x: 2 more bytes per
// element in both backward passes, and the mask is then the forward's by construction, whatever wrote y.
#include "common.h"
#include "api.h"
#include <cmath>

namespace can {

constexpr int kBnThreads = 256;
constexpr int kBnMaxTx = 32;          // octets of a channel group: 256 channels
constexpr int kBnFinCh = 16;          // bn_finalize_kernel: channels per block, and slice chunks per channel

struct BnGroup {
  int o0, TX, TY, tx, ty;             // first octet and width of the block's group, rows per block, the thread's place
};
__device__ __forceinline__ BnGroup bn_group(int C8, int G) {
  const int g = blockIdx.x, base = C8 / G, rem = C8 % G;
  BnGroup r;
  r.o0 = g * base + min(g, rem);
  r.TX = base + (g < rem ? 1 : 0);
  r.TY = kBnThreads / r.TX;
  r.tx = threadIdx.x % r.TX;
  r.ty = threadIdx.x / r.TX;          // ty >= TY: the block's idle tail (256 % TX threads)
  return r;
}

// Block sum over ty of acc[16] (k = statistic * 8 + channel of the octet) in index order, written to
// part[(slice * 2 + statistic) * C + channel].  red: 16 * 256 doubles (k-major: consecutive threads, consecutive
// addresses); red2: max(256, 16 * TX) doubles.
__device__ __forceinline__ void bn_block_reduce(const BnGroup& g, const double (&acc)[16], double* red, double* red2,
                                                double* __restrict__ part, int C) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 16; ++k) red[k * kBnThreads + t] = acc[k];      // idle threads hold zeros and are never read
  __syncthreads();
  const int NO = 16 * g.TX;                                            // outputs o = k * TX + tx
  const int Q = NO >= kBnThreads ? 1 : kBnThreads / NO;                // row chunks summed side by side
  const int R = (g.TY + Q - 1) / Q;
  for (int i = t; i < NO * Q; i += kBnThreads) {
    const int o = i % NO, q = i / NO, k = o / g.TX, tx = o - k * g.TX;
    const int r1 = min(g.TY, (q + 1) * R);
    double s = 0.0;
    for (int r = q * R; r < r1; ++r) s += red[k * kBnThreads + r * g.TX + tx];
    red2[q * NO + o] = s;
  }
  __syncthreads();
  for (int o = t; o < NO; o += kBnThreads) {
    double s = 0.0;
    for (int q = 0; q < Q; ++q) s += red2[q * NO + o];
    const int k = o / g.TX, tx = o - k * g.TX;
    part[((size_t)blockIdx.y * 2 + (k >> 3)) * C + (size_t)(g.o0 + tx) * 8 + (k & 7)] = s;
  }
}

template <int DT>
__device__ __forceinline__ void bn_acc_x(const uint4& v, double (&acc)[16]) {
  float f[8];
  unpack8h<DT>(v, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double d = (double)f[k];
    acc[k] += d;
    acc[8 + k] = fma(d, d, acc[8 + k]);
  }
}

template <int DT>
__global__ void __launch_bounds__(kBnThreads) bn_stats_kernel(const uint4* __restrict__ x, double* __restrict__ part,
                                                              long long M, long long mslice, int C8, int G) {
  __shared__ double red[16 * kBnThreads];
  __shared__ double red2[16 * kBnMaxTx];
  const BnGroup g = bn_group(C8, G);
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  if (g.ty < g.TY) {
    const long long p1 = min(M, ((long long)blockIdx.y + 1) * mslice), st = g.TY;
    const uint4* xo = x + g.o0 + g.tx;
    long long p = (long long)blockIdx.y * mslice + g.ty;
    // four loads in flight per thread; the adds keep pixel order
    for (; p + 3 * st < p1; p += 4 * st) {
      const uint4 v0 = xo[(size_t)p * C8], v1 = xo[(size_t)(p + st) * C8], v2 = xo[(size_t)(p + 2 * st) * C8],
                  v3 = xo[(size_t)(p + 3 * st) * C8];
      bn_acc_x<DT>(v0, acc); bn_acc_x<DT>(v1, acc); bn_acc_x<DT>(v2, acc); bn_acc_x<DT>(v3, acc);
    }
    for (; p < p1; p += st) bn_acc_x<DT>(xo[(size_t)p * C8], acc);
  }
  bn_block_reduce(g, acc, red, red2, part, C8 * 8);
}

// mode 0: training forward (part = sums of x, x^2); 1: eval forward (running statistics, no partials);
// 2: backward (part = sums of dz, dz * xhat).  Block = 16 channels x 16 chunks of consecutive slices.
//   modes 0 / 1: stats[3][C] = (mean, biased var, rstd), ab[2][C] = (a, b); mean / var / rstd in double with IEEE
//   divide and sqrt, each rounded to fp32 once; a and b are formed from the ROUNDED mean and rstd, so the backward's
//   gamma * stats.rstd is this a bit for bit.
//   mode 2: ab[4][C] = (dgamma, dbeta, c1 = sum dz / M, c2 = sum dz xhat / M).
__global__ void __launch_bounds__(kBnThreads) bn_finalize_kernel(const double* __restrict__ part, int S, int C,
                                                                 double M, double eps, int mode,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ rmean,
                                                                 const float* __restrict__ rvar,
                                                                 float* __restrict__ stats, float* __restrict__ ab) {
#pragma clang fp contract(off)
  __shared__ double red[2][kBnFinCh][kBnFinCh];
  const int cl = threadIdx.x % kBnFinCh, q = threadIdx.x / kBnFinCh;
  const int c = blockIdx.x * kBnFinCh + cl;
  double s0 = 0.0, s1 = 0.0;
  if (mode != 1 && c < C) {
    const int R = (S + kBnFinCh - 1) / kBnFinCh, e = min(S, (q + 1) * R);
    for (int s = q * R; s < e; ++s) {
      s0 += part[((size_t)s * 2) * C + c];
      s1 += part[((size_t)s * 2 + 1) * C + c];
    }
  }
  red[0][q][cl] = s0;
  red[1][q][cl] = s1;
  __syncthreads();
  if (q != 0 || c >= C) return;
  s0 = 0.0; s1 = 0.0;
  for (int i = 0; i < kBnFinCh; ++i) { s0 += red[0][i][cl]; s1 += red[1][i][cl]; }
  if (mode == 2) {
    ab[c] = (float)s1;
    ab[C + c] = (float)s0;
    ab[2 * (size_t)C + c] = (float)(s0 / M);
    ab[3 * (size_t)C + c] = (float)(s1 / M);
    return;
  }
  double mean, var;
  if (mode == 0) {
    mean = s0 / M;
    var = fmax(0.0, s1 / M - mean * mean);
  } else {
    mean = (double)rmean[c];
    var = (double)rvar[c];
  }
  const float meanf = (float)mean, rstdf = (float)(1.0 / sqrt(var + eps));
  stats[c] = meanf;
  stats[C + c] = (float)var;
  stats[2 * (size_t)C + c] = rstdf;
  const float a = __fmul_rn(gamma[c], rstdf);
  ab[c] = a;
  ab[C + c] = __fmaf_rn(-meanf, a, beta[c]);
}

__device__ __forceinline__ void bn_load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

template <int DT, bool RELU>
__device__ __forceinline__ uint4 bn_apply8(const uint4& v, const float (&a)[8], const float (&b)[8]) {
  float f[8];
  unpack8h<DT>(v, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = __fmaf_rn(f[k], a[k], b[k]);       // explicit: no other expression can be contracted into it
    if constexpr (RELU) f[k] = f[k] < 0.f ? 0.f : f[k];
  }
  return pack8h<DT>(f);
}

// y = f2h(fma(x, a, b)) [clamped at 0]; blockIdx.y strides over the pixels
template <int DT, bool RELU>
__global__ void __launch_bounds__(kBnThreads) bn_apply_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                              const float* __restrict__ ab, long long M, int C8,
                                                              int G) {
  const BnGroup g = bn_group(C8, G);
  if (g.ty >= g.TY) return;
  const int oct = g.o0 + g.tx, C = C8 * 8;
  float a[8], b[8];
  bn_load8(ab + oct * 8, a);
  bn_load8(ab + C + oct * 8, b);
  const long long st = (long long)gridDim.y * g.TY;
  const uint4* xo = x + oct;
  uint4* yo = y + oct;
  long long p = (long long)blockIdx.y * g.TY + g.ty;
  for (; p + 3 * st < M; p += 4 * st) {
    const uint4 v0 = xo[(size_t)p * C8], v1 = xo[(size_t)(p + st) * C8], v2 = xo[(size_t)(p + 2 * st) * C8],
                v3 = xo[(size_t)(p + 3 * st) * C8];
    yo[(size_t)p * C8] = bn_apply8<DT, RELU>(v0, a, b);
    yo[(size_t)(p + st) * C8] = bn_apply8<DT, RELU>(v1, a, b);
    yo[(size_t)(p + 2 * st) * C8] = bn_apply8<DT, RELU>(v2, a, b);
    yo[(size_t)(p + 3 * st) * C8] = bn_apply8<DT, RELU>(v3, a, b);
  }
  for (; p < M; p += st) yo[(size_t)p * C8] = bn_apply8<DT, RELU>(xo[(size_t)p * C8], a, b);
}

// dz[8] = dy where the stored y > 0 (RELU), xh[8] = (x - mean) * rstd in fp32 (two roundings)
template <int DT, bool RELU>
__device__ __forceinline__ void bn_dz_xhat(const uint4& dyv, const uint4& xv, const uint4& yv, const float (&mean)[8],
                                           const float (&rstd)[8], float (&dz)[8], float (&xh)[8]) {
  float xf[8];
  unpack8h<DT>(dyv, dz);
  unpack8h<DT>(xv, xf);
  if constexpr (RELU) {
    const unsigned w[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!pos_bits((unsigned short)(w[i] & 0xffffu))) dz[2 * i] = 0.f;
      if (!pos_bits((unsigned short)(w[i] >> 16))) dz[2 * i + 1] = 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) xh[k] = __fmul_rn(__fsub_rn(xf[k], mean[k]), rstd[k]);
}

template <int DT, bool RELU>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_stats_kernel(const uint4* __restrict__ dy,
                                                                  const uint4* __restrict__ x,
                                                                  const uint4* __restrict__ y,
                                                                  const float* __restrict__ stats,
                                                                  double* __restrict__ part, long long M,
                                                                  long long mslice, int C8, int G) {
  __shared__ double red[16 * kBnThreads];
  __shared__ double red2[16 * kBnMaxTx];
  const BnGroup g = bn_group(C8, G);
  const int C = C8 * 8;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  if (g.ty < g.TY) {
    const int oct = g.o0 + g.tx;
    float mean[8], rstd[8];
    bn_load8(stats + oct * 8, mean);
    bn_load8(stats + 2 * (size_t)C + oct * 8, rstd);
    const long long p1 = min(M, ((long long)blockIdx.y + 1) * mslice), st = g.TY;
    auto add = [&](const uint4& dv, const uint4& xv, const uint4& yv) {
      float dz[8], xh[8];
      bn_dz_xhat<DT, RELU>(dv, xv, yv, mean, rstd, dz, xh);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double d = (double)dz[k];
        acc[k] += d;
        acc[8 + k] = fma(d, (double)xh[k], acc[8 + k]);      // the product of two fp32 values is exact in double
      }
    };
    long long p = (long long)blockIdx.y * mslice + g.ty;
    for (; p + st < p1; p += 2 * st) {
      const size_t i0 = (size_t)p * C8 + oct, i1 = (size_t)(p + st) * C8 + oct;
      const uint4 d0 = dy[i0], x0 = x[i0], d1 = dy[i1], x1 = x[i1];
      uint4 y0 = d0, y1 = d1;
      if constexpr (RELU) { y0 = y[i0]; y1 = y[i1]; }
      add(d0, x0, y0);
      add(d1, x1, y1);
    }
    for (; p < p1; p += st) {
      const size_t i0 = (size_t)p * C8 + oct;
      const uint4 d0 = dy[i0], x0 = x[i0];
      uint4 y0 = d0;
      if constexpr (RELU) y0 = y[i0];
      add(d0, x0, y0);
    }
  }
  bn_block_reduce(g, acc, red, red2, part, C);
}

// TRAIN: dx = f2h(a * (dz - c1 - xhat * c2)), a = gamma * rstd (the forward's a bit for bit); eval: f2h(a * dz).
// fin[4][C] = (dgamma, dbeta, c1, c2) of bn_finalize_kernel.
template <int DT, bool RELU, bool TRAIN>
__global__ void __launch_bounds__(kBnThreads) bn_bwd_apply_kernel(const uint4* __restrict__ dy,
                                                                  const uint4* __restrict__ x,
                                                                  const uint4* __restrict__ y,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ fin,
                                                                  uint4* __restrict__ dx, long long M, int C8, int G) {
  const BnGroup g = bn_group(C8, G);
  if (g.ty >= g.TY) return;
  const int oct = g.o0 + g.tx, C = C8 * 8;
  float mean[8], rstd[8], a[8], c1[8], c2[8];
  bn_load8(stats + oct * 8, mean);
  bn_load8(stats + 2 * (size_t)C + oct * 8, rstd);
  bn_load8(gamma + oct * 8, a);
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = __fmul_rn(a[k], rstd[k]);
  if constexpr (TRAIN) {
    bn_load8(fin + 2 * (size_t)C + oct * 8, c1);
    bn_load8(fin + 3 * (size_t)C + oct * 8, c2);
  }
  auto one = [&](const uint4& dv, const uint4& xv, const uint4& yv) -> uint4 {
    float dz[8], xh[8], o[8];
    bn_dz_xhat<DT, RELU>(dv, xv, yv, mean, rstd, dz, xh);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if constexpr (TRAIN) o[k] = __fmul_rn(a[k], __fmaf_rn(-xh[k], c2[k], __fsub_rn(dz[k], c1[k])));
      else o[k] = __fmul_rn(a[k], dz[k]);
    }
    return pack8h<DT>(o);
  };
  const long long st = (long long)gridDim.y * g.TY;
  long long p = (long long)blockIdx.y * g.TY + g.ty;
  for (; p + st < M; p += 2 * st) {
    const size_t i0 = (size_t)p * C8 + oct, i1 = (size_t)(p + st) * C8 + oct;
    const uint4 d0 = dy[i0], x0 = x[i0], d1 = dy[i1], x1 = x[i1];
    uint4 y0 = d0, y1 = d1;
    if constexpr (RELU) { y0 = y[i0]; y1 = y[i1]; }
    dx[i0] = one(d0, x0, y0);
    dx[i1] = one(d1, x1, y1);
  }
  for (; p < M; p += st) {
    const size_t i0 = (size_t)p * C8 + oct;
    const uint4 d0 = dy[i0], x0 = x[i0];
    uint4 y0 = d0;
    if constexpr (RELU) y0 = y[i0];
    dx[i0] = one(d0, x0, y0);
  }
}

// ---- host side
struct BnPlan {
  int C8, G, tymin;        // octets, channel groups, rows per block of the widest group
};
static BnPlan bn_plan(int C) {
  BnPlan p;
  p.C8 = C / 8;
  p.G = (p.C8 + kBnMaxTx - 1) / kBnMaxTx;
  p.tymin = kBnThreads / ((p.C8 + p.G - 1) / p.G);
  return p;
}
static int bn_cus() {
  const int n = can_device_cus();
  return n > 0 ? n : 256;
}
// Pixel slices of the statistics passes: groups x S fills the CUs four times (four 36-KiB blocks are resident per CU:
// one whole round), fewer where a slice would get under 16 rows per thread.
static int bn_slices(long long M, const BnPlan& p) {
  long long S = (4ll * bn_cus()) / p.G, cap = M / (16ll * p.tymin);
  if (S > cap) S = cap;
  if (S > 65535) S = 65535;
  return S < 1 ? 1 : (int)S;
}
// blockIdx.y of the apply passes: eight blocks per CU over all groups, no more than the rows need
static int bn_apply_rows(long long M, const BnPlan& p) {
  long long gy = (8ll * bn_cus()) / p.G, need = (M + p.tymin - 1) / p.tymin;
  if (gy > need) gy = need;
  if (gy > 65535) gy = 65535;
  return gy < 1 ? 1 : (int)gy;
}
// -2 channels, -3 a training batch of one value per channel, -5 a map beyond the indexing (pixel offsets are 64-bit;
// the count must stay exact in double and M * C * 2 bytes addressable), -20 the element type
static int bn_check(long long M, int C, int training, int dt) {
  if (C <= 0 || (C & 7)) return -2;
  if (M < 1 || M > (1ll << 48) / C) return -5;
  if (training && M < 2) return -3;
  if (dt != DT_BF16 && dt != DT_F16) return -20;
  return 0;
}

#define BN_LAUNCH(dt, relu, K, ...)                                                                   \
  do {                                                                                                \
    if ((dt) == DT_F16) {                                                                             \
      if (relu) hipLaunchKernelGGL((K<DT_F16, true>), __VA_ARGS__);                                   \
      else hipLaunchKernelGGL((K<DT_F16, false>), __VA_ARGS__);                                       \
    } else {                                                                                          \
      if (relu) hipLaunchKernelGGL((K<DT_BF16, true>), __VA_ARGS__);                                  \
      else hipLaunchKernelGGL((K<DT_BF16, false>), __VA_ARGS__);                                      \
    }                                                                                                 \
  } while (0)

}  // namespace can

using namespace can;

extern "C" int can_bn_slices(long long M, int C) {
  const int rc = bn_check(M, C, 0, DT_BF16);
  return rc ? rc : bn_slices(M, bn_plan(C));
}

// Forward.  training: part [S][2][C] doubles (S >= 1: the caller's slice count), stats from the batch; eval: stats from
// (rmean, rvar), part unused.  stats [3][C] and ab [2][C] fp32 are written either way; y = [relu](x * a + b).
extern "C" int can_bn_forward(const void* x, void* y, const float* gamma, const float* beta, const float* rmean,
                              const float* rvar, double* part, int S, float* stats, float* ab, long long M, int C,
                              double eps, int training, int relu, int dt, void* stream) {
  const int rc = bn_check(M, C, training, dt);
  if (rc) return rc;
  if (!(eps >= 0.0) || !std::isfinite(eps)) return -4;
  if (x == nullptr || y == nullptr || gamma == nullptr || beta == nullptr || stats == nullptr || ab == nullptr)
    return -7;
  if (training ? (part == nullptr || S < 1 || S > 65535) : (rmean == nullptr || rvar == nullptr)) return -6;
  const BnPlan p = bn_plan(C);
  hipStream_t s = (hipStream_t)stream;
  if (training) {
    const long long mslice = (M + S - 1) / S;
    CAN_LAUNCH_DT(dt, bn_stats_kernel, dim3(p.G, S), dim3(kBnThreads), 0, s, (const uint4*)x, part, M, mslice, p.C8,
                  p.G);
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kBnFinCh - 1) / kBnFinCh), dim3(kBnThreads), 0, s,
                     (const double*)part, S, C, (double)M, eps, training ? 0 : 1, gamma, beta, rmean, rvar, stats, ab);
  BN_LAUNCH(dt, relu, bn_apply_kernel, dim3(p.G, bn_apply_rows(M, p)), dim3(kBnThreads), 0, s, (const uint4*)x,
            (uint4*)y, (const float*)ab, M, p.C8, p.G);
  return (int)hipGetLastError();
}

// Backward.  stats: the forward's; y: the forward's output (read with relu only); fin [4][C] fp32 = (dgamma, dbeta,
// c1, c2); part [S][2][C] doubles.
extern "C" int can_bn_backward(const void* dy, const void* x, const void* y, const float* gamma, const float* stats,
                               double* part, int S, float* fin, void* dx, long long M, int C, int training, int relu,
                               int dt, void* stream) {
  const int rc = bn_check(M, C, training, dt);
  if (rc) return rc;
  if (dy == nullptr || x == nullptr || (relu && y == nullptr) || gamma == nullptr || stats == nullptr ||
      fin == nullptr || dx == nullptr)
    return -7;
  if (part == nullptr || S < 1 || S > 65535) return -6;
  const BnPlan p = bn_plan(C);
  hipStream_t s = (hipStream_t)stream;
  const long long mslice = (M + S - 1) / S;
  BN_LAUNCH(dt, relu, bn_bwd_stats_kernel, dim3(p.G, S), dim3(kBnThreads), 0, s, (const uint4*)dy, (const uint4*)x,
            (const uint4*)y, stats, part, M, mslice, p.C8, p.G);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kBnFinCh - 1) / kBnFinCh), dim3(kBnThreads), 0, s,
                     (const double*)part, S, C, (double)M, 0.0, 2, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr, fin);
  const dim3 grid(p.G, bn_apply_rows(M, p));
#define BN_BWD_APPLY(DTV, RL, TR)                                                                               \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<DTV, RL, TR>), grid, dim3(kBnThreads), 0, s, (const uint4*)dy,        \
                     (const uint4*)x, (const uint4*)y, gamma, stats, (const float*)fin, (uint4*)dx, M, p.C8, p.G)
  const int v = (dt == DT_F16 ? 4 : 0) | (relu ? 2 : 0) | (training ? 1 : 0);
  switch (v) {
    case 0: BN_BWD_APPLY(DT_BF16, false, false); break;
    case 1: BN_BWD_APPLY(DT_BF16, false, true); break;
    case 2: BN_BWD_APPLY(DT_BF16, true, false); break;
    case 3: BN_BWD_APPLY(DT_BF16, true, true); break;
    case 4: BN_BWD_APPLY(DT_F16, false, false); break;
    case 5: BN_BWD_APPLY(DT_F16, false, true); break;
    case 6: BN_BWD_APPLY(DT_F16, true, false); break;
    default: BN_BWD_APPLY(DT_F16, true, true); break;
  }
#undef BN_BWD_APPLY
  return (int)hipGetLastError();
}
