// Resampling of an NHWC 16-bit map x[N][H][W][C], C % 8 == 0, forward and backward (gfx950): adaptive average pool
// (F.adaptive_avg_pool2d) and bilinear resize (F.interpolate(mode="bilinear")), the two layers of CANNet's context
// branches and of the VGG-19 point-loss networks that the cannet:: library lacked.  Streaming kernels: a lane's unit is
// one 16-byte channel octet, all arithmetic fp32, one rounding to 16 bit at the store, no atomics, every sum in a
// fixed order: bitwise repeatable.  Nothing here is matrix-core work: the contractions have K <= 4 (the four taps of a
// bilinear sample) or are plain sums over a bin, so the MFMA units stay idle by design.  Plans: resample_plan.h.
//
//   pool_fwd_direct_kernel   y = f2h(sum(bin) / float(count)), a thread per (cell, octet), bin walked row-major
//   pool_rows_kernel         separable form, pass 1: rowacc[n][h][j][c] = sum of row h over column bin j (ascending);
//                            the column-bin bounds of the row are built once per block in LDS
//   pool_cells_kernel        pass 2: y = f2h(sum over the row bin of rowacc (ascending) / float(count))
//   pool_bwd_kernel          dx[p] = f2h(sum over the bins holding p of dy[bin] / float(count)), row-bin-major gather
//   resize_fwd_kernel        out = fma(lv, bot - top, top), top / bot = fma(lh, b - a, a) of two source rows; staged
//                            through LDS (horizontal blends once per source row of the tile's window) or from global
//   resize_bwd_kernel        exact adjoint as a gather: vertical adjoint of a chunk of output columns into an fp32 LDS
//                            row, then the horizontal adjoint per source column; optional output-row slices
//   resize_reduce_kernel     dx = f2h(sum of the slices' partials, in slice order)
//
// Tap tables (built on the host in double, ops/resample.py), one int32 array per axis of source length l and output
// length L: i0[L], i1[L], lambda[L] (fp32 bits), w0[L], w1[L] (the adjoint's weights: fp32(1 - lambda) and lambda, or
// 1 and 0 where i0 == i1), lo[l], hi[l] (the outputs touching source s are exactly [lo[s], hi[s])).
#include "common.h"
#include "api.h"
#include "resample_plan.h"

namespace can {

__device__ __forceinline__ void rs_zero8(float (&a)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = 0.f;
}
template <int DT>
__device__ __forceinline__ void rs_add8(const uint4& v, float (&acc)[8]) {
  float f[8];
  unpack8h<DT>(v, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = __fadd_rn(acc[k], f[k]);
}
__device__ __forceinline__ void rs_load8f(const float* __restrict__ p, float (&v)[8]) {
  const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
__device__ __forceinline__ void rs_store8f(float* __restrict__ p, const float (&v)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
// sum of n octets p[0], p[stride], ... in index order, four loads in flight
template <int DT>
__device__ __forceinline__ void rs_sum_run(const uint4* __restrict__ p, size_t stride, int n, float (&acc)[8]) {
  int i = 0;
  for (; i + 3 < n; i += 4) {
    const uint4 v0 = p[i * stride], v1 = p[(i + 1) * stride], v2 = p[(i + 2) * stride], v3 = p[(i + 3) * stride];
    rs_add8<DT>(v0, acc); rs_add8<DT>(v1, acc); rs_add8<DT>(v2, acc); rs_add8<DT>(v3, acc);
  }
  for (; i < n; ++i) rs_add8<DT>(p[i * stride], acc);
}
template <int DT>
__device__ __forceinline__ uint4 rs_mean8(const float (&acc)[8], float cnt) {
  float o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = __fdiv_rn(acc[k], cnt);
  return pack8h<DT>(o);
}

// ---- adaptive average pool
template <int DT>
__global__ void __launch_bounds__(RS_THREADS) pool_fwd_direct_kernel(const uint4* __restrict__ x,
                                                                     uint4* __restrict__ y, int H, int W, int C8,
                                                                     int oh, int ow, unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)RS_THREADS + threadIdx.x;
  if (idx >= total) return;
  const unsigned cell = idx / (unsigned)C8, oct = idx - cell * C8;
  const unsigned ni = cell / (unsigned)ow, j = cell - ni * ow, n = ni / (unsigned)oh, i = ni - n * oh;
  const int h0 = rs_bin_lo(i, H, oh), h1 = rs_bin_hi(i, H, oh), w0 = rs_bin_lo(j, W, ow), w1 = rs_bin_hi(j, W, ow);
  float acc[8];
  rs_zero8(acc);
  for (int h = h0; h < h1; ++h)
    rs_sum_run<DT>(x + ((size_t)n * H + h) * W * C8 + (size_t)w0 * C8 + oct, (size_t)C8, w1 - w0, acc);
  y[idx] = rs_mean8<DT>(acc, (float)((long long)(h1 - h0) * (w1 - w0)));
}

// a block per image row (n, h): bounds[j] = (w0, w1) of column bin j, then a thread per (j, octet)
template <int DT>
__global__ void __launch_bounds__(RS_THREADS) pool_rows_kernel(const uint4* __restrict__ x,
                                                               float* __restrict__ rowacc, int W, int C8, int ow) {
  __shared__ int2 bounds[RS_POOL_TABLE];
  for (int j = threadIdx.x; j < ow; j += RS_THREADS) bounds[j] = make_int2(rs_bin_lo(j, W, ow), rs_bin_hi(j, W, ow));
  __syncthreads();
  const uint4* row = x + (size_t)blockIdx.x * W * C8;
  float* out = rowacc + (size_t)blockIdx.x * ow * C8 * 8;
  for (int it = threadIdx.x; it < ow * C8; it += RS_THREADS) {
    const int j = it / C8, oct = it - j * C8;
    const int2 b = bounds[j];
    float acc[8];
    rs_zero8(acc);
    rs_sum_run<DT>(row + (size_t)b.x * C8 + oct, (size_t)C8, b.y - b.x, acc);
    rs_store8f(out + (size_t)it * 8, acc);
  }
}

template <int DT>
__global__ void __launch_bounds__(RS_THREADS) pool_cells_kernel(const float* __restrict__ rowacc,
                                                                uint4* __restrict__ y, int H, int W, int C8, int oh,
                                                                int ow, unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)RS_THREADS + threadIdx.x;
  if (idx >= total) return;
  const unsigned cell = idx / (unsigned)C8, oct = idx - cell * C8;
  const unsigned ni = cell / (unsigned)ow, j = cell - ni * ow, n = ni / (unsigned)oh, i = ni - n * oh;
  const int h0 = rs_bin_lo(i, H, oh), h1 = rs_bin_hi(i, H, oh), w0 = rs_bin_lo(j, W, ow), w1 = rs_bin_hi(j, W, ow);
  const size_t st = (size_t)ow * C8 * 8;
  const float* p = rowacc + ((size_t)n * H + h0) * st + ((size_t)j * C8 + oct) * 8;
  float acc[8];
  rs_zero8(acc);
  int h = h0;
  for (; h + 3 < h1; h += 4, p += 4 * st) {
    float a[8], b[8], c[8], d[8];
    rs_load8f(p, a); rs_load8f(p + st, b); rs_load8f(p + 2 * st, c); rs_load8f(p + 3 * st, d);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      acc[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc[k], a[k]), b[k]), c[k]), d[k]);
  }
  for (; h < h1; ++h, p += st) {
    float a[8];
    rs_load8f(p, a);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = __fadd_rn(acc[k], a[k]);
  }
  y[idx] = rs_mean8<DT>(acc, (float)((long long)(h1 - h0) * (w1 - w0)));
}

// a thread per (input pixel, octet): the row bins holding row h are floor(h oh / H) .. ceil((h + 1) oh / H) - 1
template <int DT>
__global__ void __launch_bounds__(RS_THREADS) pool_bwd_kernel(const uint4* __restrict__ dy, uint4* __restrict__ dx,
                                                              int H, int W, int C8, int oh, int ow, unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)RS_THREADS + threadIdx.x;
  if (idx >= total) return;
  const unsigned pix = idx / (unsigned)C8, oct = idx - pix * C8;
  const unsigned nh = pix / (unsigned)W, w = pix - nh * W, n = nh / (unsigned)H, h = nh - n * H;
  const int i0 = rs_floor_div(h, oh, H), i1 = rs_ceil_div(h + 1, oh, H);
  const int j0 = rs_floor_div(w, ow, W), j1 = rs_ceil_div(w + 1, ow, W);
  float acc[8];
  rs_zero8(acc);
  for (int i = i0; i < i1; ++i) {
    const int bh = rs_bin_hi(i, H, oh) - rs_bin_lo(i, H, oh);
    const uint4* row = dy + ((size_t)n * oh + i) * ow * C8 + oct;
    for (int j = j0; j < j1; ++j) {
      const float cnt = (float)((long long)bh * (rs_bin_hi(j, W, ow) - rs_bin_lo(j, W, ow)));
      float f[8];
      unpack8h<DT>(row[(size_t)j * C8], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = __fadd_rn(acc[k], __fdiv_rn(f[k], cnt));
    }
  }
  dx[idx] = pack8h<DT>(acc);
}

// ---- bilinear resize
struct RsAxis {
  const int *i0, *i1;
  const float *lam, *w0, *w1;
  const int *lo, *hi;
};
__device__ __forceinline__ RsAxis rs_axis(const int* __restrict__ t, int l, int L) {
  RsAxis a;
  a.i0 = t; a.i1 = t + L;
  a.lam = reinterpret_cast<const float*>(t + 2 * (size_t)L);
  a.w0 = reinterpret_cast<const float*>(t + 3 * (size_t)L);
  a.w1 = reinterpret_cast<const float*>(t + 4 * (size_t)L);
  a.lo = t + 5 * (size_t)L; a.hi = a.lo + l;
  return a;
}
// weight of output o on source s (s is i0[o] or i1[o]): exactly one term is non-zero, or w0 = 1, w1 = 0
__device__ __forceinline__ float rs_weight(const RsAxis& a, int o, int s) {
  return (a.i0[o] == s ? a.w0[o] : 0.f) + (a.i1[o] == s ? a.w1[o] : 0.f);
}
// fma(lam, b - a, a) per channel of two 16-bit octets
template <int DT>
__device__ __forceinline__ void rs_hblend(const uint4& va, const uint4& vb, float lam, float (&o)[8]) {
  float a[8], b[8];
  unpack8h<DT>(va, a);
  unpack8h<DT>(vb, b);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = __fmaf_rn(lam, __fsub_rn(b[k], a[k]), a[k]);
}

// grid.x = ((n * ntr + tile row) * nst + strip) * G + group
template <int DT>
__global__ void __launch_bounds__(RS_THREADS) resize_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                                const int* __restrict__ tv,
                                                                const int* __restrict__ th, int h, int w, int C8,
                                                                int G, int oh, int ow, int TR, int SW, int win,
                                                                int ntr, int nst) {
  __shared__ float4 hb[RS_FWD_UNITS * 2];
  unsigned b = blockIdx.x;
  const int g = b % G; b /= G;
  const int st = b % nst; b /= nst;
  const int tr = b % ntr, n = b / ntr;
  int o0, TX;
  rs_group(C8, G, g, o0, TX);
  const RsAxis av = rs_axis(tv, h, oh), ah = rs_axis(th, w, ow);
  const int r0 = tr * TR, r1 = min(oh, r0 + TR), c0 = st * SW, ncol = min(ow, c0 + SW) - c0;
  const int sr0 = av.i0[r0], nwin = av.i1[r1 - 1] - sr0 + 1;
  const bool staged = nwin <= win && nwin * ncol * TX <= RS_FWD_UNITS;      // block-uniform
  const uint4* xn = x + (size_t)n * h * w * C8 + o0;
  if (staged) {
    for (int it = threadIdx.x; it < nwin * ncol * TX; it += RS_THREADS) {
      const int q = it / TX, tx = it - q * TX, wr = q / ncol, c = q - wr * ncol;
      const uint4* row = xn + (size_t)(sr0 + wr) * w * C8 + tx;
      float o[8];
      rs_hblend<DT>(row[(size_t)ah.i0[c0 + c] * C8], row[(size_t)ah.i1[c0 + c] * C8], ah.lam[c0 + c], o);
      hb[2 * it] = make_float4(o[0], o[1], o[2], o[3]);
      hb[2 * it + 1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
  }
  for (int it = threadIdx.x; it < (r1 - r0) * ncol * TX; it += RS_THREADS) {
    const int q = it / TX, tx = it - q * TX, rr = q / ncol, c = q - rr * ncol, r = r0 + rr;
    const int s0 = av.i0[r], s1 = av.i1[r];
    float top[8], bot[8], o[8];
    if (staged) {
      const int u0 = ((s0 - sr0) * ncol + c) * TX + tx, u1 = ((s1 - sr0) * ncol + c) * TX + tx;
      const float4 a = hb[2 * u0], a2 = hb[2 * u0 + 1], d = hb[2 * u1], d2 = hb[2 * u1 + 1];
      top[0] = a.x; top[1] = a.y; top[2] = a.z; top[3] = a.w; top[4] = a2.x; top[5] = a2.y; top[6] = a2.z; top[7] = a2.w;
      bot[0] = d.x; bot[1] = d.y; bot[2] = d.z; bot[3] = d.w; bot[4] = d2.x; bot[5] = d2.y; bot[6] = d2.z; bot[7] = d2.w;
    } else {
      const size_t ja = (size_t)ah.i0[c0 + c] * C8 + tx, jb = (size_t)ah.i1[c0 + c] * C8 + tx;
      const uint4 *ra = xn + (size_t)s0 * w * C8, *rb = xn + (size_t)s1 * w * C8;
      const float lh = ah.lam[c0 + c];
      rs_hblend<DT>(ra[ja], ra[jb], lh, top);
      rs_hblend<DT>(rb[ja], rb[jb], lh, bot);
    }
    const float lv = av.lam[r];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = __fmaf_rn(lv, __fsub_rn(bot[k], top[k]), top[k]);
    y[(((size_t)n * oh + r) * ow + c0 + c) * C8 + o0 + tx] = pack8h<DT>(o);
  }
}

// grid.x = ((((slice * N + n) * h + s) * nst + strip) * G + group; thread = (source column ty, octet tx).
// PART: the block's sum goes to part [S][N][h][w][C] fp32, else to dx in 16 bit.
template <int DT, bool PART>
__global__ void __launch_bounds__(RS_THREADS) resize_bwd_kernel(const uint4* __restrict__ dy, void* __restrict__ out,
                                                                const int* __restrict__ tv,
                                                                const int* __restrict__ th, int N, int h, int w,
                                                                int C8, int G, int oh, int ow, int S, int oc_cap,
                                                                int TY, int nst) {
  __shared__ float4 vrow[RS_BWD_UNITS * 2];
  unsigned b = blockIdx.x;
  const int g = b % G; b /= G;
  const int st = b % nst; b /= nst;
  const int s = b % h; b /= h;
  const int n = b % N, k = b / N;
  int o0, TX;
  rs_group(C8, G, g, o0, TX);
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;      // TY = 256 / (widest group): the same strips for all
  const int sc = st * TY + ty;
  const bool active = ty < TY && sc < w;
  const RsAxis av = rs_axis(tv, h, oh), ah = rs_axis(th, w, ow);
  // the slice's output rows of source row s
  const int rlo = av.lo[s], len = max(0, av.hi[s] - rlo), chunk = (len + S - 1) / S;
  const int ra = rlo + k * chunk, rb = min(rlo + len, ra + chunk);
  // output columns touching the strip, and this thread's own
  const int olo = ah.lo[st * TY], ohi = ah.hi[min(w, st * TY + TY) - 1];
  const int mylo = active ? ah.lo[sc] : 0, myhi = active ? ah.hi[sc] : 0;
  const uint4* dyn = dy + (size_t)n * oh * ow * C8 + o0;
  float acc[8];
  rs_zero8(acc);
  for (int ocb = olo; ocb < ohi; ocb += oc_cap) {
    const int nc = min(oc_cap, ohi - ocb);
    for (int it = threadIdx.x; it < nc * TX; it += RS_THREADS) {
      const int c = it / TX, t = it - c * TX;
      float v[8];
      rs_zero8(v);
      const uint4* col = dyn + (size_t)(ocb + c) * C8 + t;
      for (int o = ra; o < rb; ++o) {
        const float wgt = rs_weight(av, o, s);
        float f[8];
        unpack8h<DT>(col[(size_t)o * ow * C8], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = __fmaf_rn(wgt, f[q], v[q]);
      }
      vrow[2 * it] = make_float4(v[0], v[1], v[2], v[3]);
      vrow[2 * it + 1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    const int e = min(ocb + nc, myhi);
    for (int oc = max(ocb, mylo); oc < e; ++oc) {
      const float wgt = rs_weight(ah, oc, sc);
      const int u = (oc - ocb) * TX + tx;
      const float4 a = vrow[2 * u], a2 = vrow[2 * u + 1];
      acc[0] = __fmaf_rn(wgt, a.x, acc[0]); acc[1] = __fmaf_rn(wgt, a.y, acc[1]);
      acc[2] = __fmaf_rn(wgt, a.z, acc[2]); acc[3] = __fmaf_rn(wgt, a.w, acc[3]);
      acc[4] = __fmaf_rn(wgt, a2.x, acc[4]); acc[5] = __fmaf_rn(wgt, a2.y, acc[5]);
      acc[6] = __fmaf_rn(wgt, a2.z, acc[6]); acc[7] = __fmaf_rn(wgt, a2.w, acc[7]);
    }
    __syncthreads();
  }
  if (!active) return;
  const size_t pix = ((size_t)n * h + s) * w + sc;
  if constexpr (PART)
    rs_store8f(reinterpret_cast<float*>(out) + (((size_t)k * N * h * w + pix) * C8 + o0 + tx) * 8, acc);
  else
    reinterpret_cast<uint4*>(out)[pix * C8 + o0 + tx] = pack8h<DT>(acc);
}

template <int DT>
__global__ void __launch_bounds__(RS_THREADS) resize_reduce_kernel(const float* __restrict__ part,
                                                                   uint4* __restrict__ dx, int S, unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)RS_THREADS + threadIdx.x;
  if (idx >= total) return;
  float acc[8];
  rs_load8f(part + (size_t)idx * 8, acc);
  for (int k = 1; k < S; ++k) {
    float a[8];
    rs_load8f(part + ((size_t)k * total + idx) * 8, a);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = __fadd_rn(acc[q], a[q]);
  }
  dx[idx] = pack8h<DT>(acc);
}

static int rs_dt_check(int dt) { return dt == DT_BF16 || dt == DT_F16 ? 0 : -20; }
static unsigned rs_blocks(long long items) { return (unsigned)((items + RS_THREADS - 1) / RS_THREADS); }

}  // namespace can

using namespace can;

extern "C" int can_pool_adaptive_plan(int N, int H, int W, int C, int oh, int ow, int form, long long* ws_floats) {
  const PoolPlan p = pool_plan(N, H, W, C, oh, ow, form, can_device_cus());
  if (p.err) return p.err;
  if (ws_floats) *ws_floats = p.ws_floats;
  return p.form;
}

extern "C" int can_pool_adaptive_fwd(const void* x, void* y, float* ws, long long ws_floats, int N, int H, int W, int C,
                                     int oh, int ow, int form, int dt, void* stream) {
  const PoolPlan p = pool_plan(N, H, W, C, oh, ow, form, can_device_cus());
  if (p.err) return p.err;
  if (rs_dt_check(dt)) return -20;
  if (x == nullptr || y == nullptr) return -7;
  if (p.ws_floats && (ws == nullptr || ws_floats < p.ws_floats)) return -6;
  hipStream_t s = (hipStream_t)stream;
  const int C8 = C / 8;
  const long long items = (long long)N * oh * ow * C8;
  if (p.form == POOL_SEPARABLE) {
    CAN_LAUNCH_DT(dt, pool_rows_kernel, dim3((unsigned)(N * H)), dim3(RS_THREADS), 0, s, (const uint4*)x, ws, W, C8, ow);
    CAN_LAUNCH_DT(dt, pool_cells_kernel, dim3(rs_blocks(items)), dim3(RS_THREADS), 0, s, (const float*)ws, (uint4*)y,
                  H, W, C8, oh, ow, (unsigned)items);
  } else {
    CAN_LAUNCH_DT(dt, pool_fwd_direct_kernel, dim3(rs_blocks(items)), dim3(RS_THREADS), 0, s, (const uint4*)x,
                  (uint4*)y, H, W, C8, oh, ow, (unsigned)items);
  }
  return (int)hipGetLastError();
}

extern "C" int can_pool_adaptive_bwd(const void* dy, void* dx, int N, int H, int W, int C, int oh, int ow, int dt,
                                     void* stream) {
  const int rc = rs_check(N, H, W, C, oh, ow);
  if (rc) return rc;
  if (rs_dt_check(dt)) return -20;
  if (dy == nullptr || dx == nullptr) return -7;
  const int C8 = C / 8;
  const long long items = (long long)N * H * W * C8;
  CAN_LAUNCH_DT(dt, pool_bwd_kernel, dim3(rs_blocks(items)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                (const uint4*)dy, (uint4*)dx, H, W, C8, oh, ow, (unsigned)items);
  return (int)hipGetLastError();
}

extern "C" int can_resize_bilinear_fwd_plan(int N, int h, int w, int C, int oh, int ow, int staged, int* out5) {
  const ResizeFwdPlan p = resize_fwd_plan(N, h, w, C, oh, ow, staged);
  if (p.err) return p.err;
  if (out5) { out5[0] = p.G; out5[1] = p.tr; out5[2] = p.sw; out5[3] = p.win; out5[4] = p.staged; }
  return 0;
}

extern "C" int can_resize_bilinear_bwd_plan(int N, int h, int w, int C, int oh, int ow, int slices, int* out4,
                                            long long* ws_floats) {
  const ResizeBwdPlan p = resize_bwd_plan(N, h, w, C, oh, ow, slices, can_device_cus());
  if (p.err) return p.err;
  if (out4) { out4[0] = p.G; out4[1] = p.ty; out4[2] = p.oc_cap; out4[3] = p.S; }
  if (ws_floats) *ws_floats = p.ws_floats;
  return 0;
}

extern "C" int can_resize_bilinear_fwd(const void* x, void* y, const int* tv, const int* th, int N, int h, int w, int C,
                                       int oh, int ow, int staged, int dt, void* stream) {
  const ResizeFwdPlan p = resize_fwd_plan(N, h, w, C, oh, ow, staged);
  if (p.err) return p.err;
  if (rs_dt_check(dt)) return -20;
  if (x == nullptr || y == nullptr || tv == nullptr || th == nullptr) return -7;
  const int ntr = (oh + p.tr - 1) / p.tr, nst = (ow + p.sw - 1) / p.sw;
  const long long blocks = (long long)N * ntr * nst * p.G;
  if (blocks > 0x7fffffffll) return -5;
  CAN_LAUNCH_DT(dt, resize_fwd_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, (hipStream_t)stream,
                (const uint4*)x, (uint4*)y, tv, th, h, w, C / 8, p.G, oh, ow, p.tr, p.sw, p.staged ? p.win : 0, ntr,
                nst);
  return (int)hipGetLastError();
}

// dy [N][oh][ow][C] -> dx [N][h][w][C]; ws: the plan's ws_floats fp32 partials when it cuts slices
extern "C" int can_resize_bilinear_bwd(const void* dy, void* dx, const int* tv, const int* th, float* ws,
                                       long long ws_floats, int N, int h, int w, int C, int oh, int ow, int slices,
                                       int dt, void* stream) {
  const ResizeBwdPlan p = resize_bwd_plan(N, h, w, C, oh, ow, slices, can_device_cus());
  if (p.err) return p.err;
  if (rs_dt_check(dt)) return -20;
  if (dy == nullptr || dx == nullptr || tv == nullptr || th == nullptr) return -7;
  if (p.ws_floats && (ws == nullptr || ws_floats < p.ws_floats)) return -6;
  const int C8 = C / 8, nst = (w + p.ty - 1) / p.ty;
  const long long blocks = (long long)p.S * N * h * nst * p.G;
  if (blocks > 0x7fffffffll) return -5;
  hipStream_t s = (hipStream_t)stream;
#define RS_BWD(DTV, PARTV, OUT)                                                                                   \
  hipLaunchKernelGGL((resize_bwd_kernel<DTV, PARTV>), dim3((unsigned)blocks), dim3(RS_THREADS), 0, s,              \
                     (const uint4*)dy, (void*)(OUT), tv, th, N, h, w, C8, p.G, oh, ow, p.S, p.oc_cap, p.ty, nst)
  if (p.S > 1) {
    if (dt == DT_F16) RS_BWD(DT_F16, true, ws); else RS_BWD(DT_BF16, true, ws);
    const long long items = (long long)N * h * w * C8;
    CAN_LAUNCH_DT(dt, resize_reduce_kernel, dim3(rs_blocks(items)), dim3(RS_THREADS), 0, s, (const float*)ws,
                  (uint4*)dx, p.S, (unsigned)items);
  } else {
    if (dt == DT_F16) RS_BWD(DT_F16, false, dx); else RS_BWD(DT_BF16, false, dx);
  }
#undef RS_BWD
  return (int)hipGetLastError();
}
