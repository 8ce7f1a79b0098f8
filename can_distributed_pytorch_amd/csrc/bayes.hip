// Bayesian point loss (Ma et al., ICCV 2019) on head records, gfx950 wave64 (README, "Bayesian loss").
//
// A sample has a crop (ch, cw), a downsample d and a map et [h][w], h = ch / d, w = cw / d; its heads z_n are points in
// crop pixels.  Pixel m = (i, j) sits at x_m = (d j + d / 2, d i + d / 2).  With k = -1 / (2 sigma^2):
//   l_nm = k |x_m - z_n|^2,  l_0m = k (D - dmin_m)^2 (the background class, D = rho min(ch, cw), only with rho > 0),
//   p(n|m) = exp(l_nm - lse_m),  E_n = sum_m p(n|m) et_m,  L = sum_{n>=1} |1 - E_n| + |E_0|,
//   g_m = sum_{n>=1} sgn(E_n - 1) p(n|m) + sgn(E_0) p(0|m).
// A sample without heads is the background class alone: p(0|m) = 1, E_0 = sum et, L = |E_0|, g = sgn(E_0), for any rho.
//
// The N x M posterior matrix is never stored: three passes recompute the logits from the points.
//   crop_points   head table + crop descriptors -> the points of every sample, in table order (ballot + prefix count)
//   bayes_norm    grid (16 x 16 pixel tile, sample), one pixel per thread, the points through LDS in chunks of 256:
//                 a first sweep keeps dmin^2 (so the largest logit is known: k dmin^2 or l_0), a second sums the
//                 exponentials -> lse_m, dmin_m
//   bayes_expect  one wave per four heads, sixteen heads per block; the pixels' (x, y, lse, et) go through LDS in chunks
//                 of 1024 and every lane sums its pixels (lane, lane + 64, ...) for its wave's four heads, then a
//                 butterfly over the wave -> E_n; bayes_e0: one block per sample -> E_0
//   bayes_grad    the normaliser's grid; (z, sgn(E_n - 1)) through LDS -> g_m, zero in the padding columns of a
//                 width-padded g;  bayes_loss: one block, per sample and then over samples in index order -> the loss
//                 and its non-finite flag (head_reduce_kernel's contract)
// No grid depends on the device-side counts (blocks loop to cnt[s]), nothing is read back, there are no atomics and
// every sum has a fixed order: all outputs are bitwise repeatable.  The work is N x M exponentials feeding two
// matrix-vector products, so there is nothing for the matrix cores to do.
//
// Every logit is formed by bl_logit / bl_bg with explicit roundings (no contraction), so the three passes agree on it.
#include "common.h"
#include "api.h"

namespace can {

constexpr int BL_T = 16;                         // pixel tile edge of the normaliser and gradient passes
constexpr int BL_CHUNK = 256;                    // points per LDS chunk
constexpr int BE_HPW = 4;                        // heads per wave of the expectation pass
constexpr int BE_HPB = 4 * BE_HPW;               // heads per block
constexpr int BE_PIX = 1024;                     // pixels per LDS chunk (16 KiB of float4)

__device__ __forceinline__ float bl_logit(float px, float py, float zx, float zy, float k) {
  const float dx = px - zx, dy = py - zy;
  return __fmul_rn(k, __fmaf_rn(dx, dx, __fmul_rn(dy, dy)));
}
__device__ __forceinline__ float bl_bg(float dmin, float D, float k) {
  const float q = D - dmin;
  return __fmul_rn(k, __fmul_rn(q, q));
}

// One block per output sample.  A record (c, r, ., .) is in the window iff x0 <= c < x0 + sw and y0 <= r < y0 + sh; an
// unscaled crop (slot 7 == 1) uses crop_window's valid extent as the window and maps onto it, as gt_from_heads_kernel
// reads the descriptor.  zx = float(double((2 (c - x0) + 1) tw) / double(2 sw)), mirrored about tw when flipped.
__global__ void __launch_bounds__(256) crop_points_kernel(const float4* __restrict__ heads,
                                                          const long long* __restrict__ ranges,
                                                          const long long* __restrict__ desc,
                                                          const long long* __restrict__ begins,
                                                          float2* __restrict__ pts, int* __restrict__ cnt, int CH,
                                                          int CW, int ds) {
  __shared__ int wcount[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const long long* d = desc + (size_t)s * 8;
  const int flip = (int)d[4], y0 = (int)d[5], x0 = (int)d[6];
  long long sh, sw, th = CH, tw = CW;
  if (d[7] == 1) {
    sh = min((long long)CH, d[1] / ds * ds), sw = min((long long)CW, d[2] / ds * ds);
    th = sh, tw = sw;
  } else {
    sh = d[7] >> 32, sw = d[7] & 0xffffffffll;
  }
  const long long first = ranges[2 * (size_t)s], count = ranges[2 * (size_t)s + 1];
  float2* out = pts + begins[s];
  int kept = 0;
  for (long long base = 0; base < count; base += 256) {
    const long long idx = base + tid;
    bool hit = false;
    float2 z = make_float2(0.f, 0.f);
    if (idx < count) {
      const float4 hr = heads[first + idx];
      const long long c = (long long)hr.x - x0, r = (long long)hr.y - y0;
      hit = c >= 0 && c < sw && r >= 0 && r < sh;
      if (hit) {
        z.x = (float)((double)((2 * c + 1) * tw) / (double)(2 * sw));
        z.y = (float)((double)((2 * r + 1) * th) / (double)(2 * sh));
        if (flip) z.x = (float)((double)tw - (double)z.x);
      }
    }
    const unsigned long long mask = __ballot(hit);
    __syncthreads();                             // (the previous chunk's wcount has been read)
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int slot = kept + __popcll(mask & ((1ull << lane) - 1ull));
    for (int q = 0; q < wave; ++q) slot += wcount[q];
    if (hit) out[slot] = z;
    kept += wcount[0] + wcount[1] + wcount[2] + wcount[3];
  }
  if (tid == 0) cnt[s] = kept;
}

__global__ void __launch_bounds__(256) bayes_norm_kernel(const float2* __restrict__ pts,
                                                         const long long* __restrict__ begins,
                                                         const int* __restrict__ cnt, float* __restrict__ lse,
                                                         float* __restrict__ dmin, int h, int w, int d, float k,
                                                         float D, int bg, int tiles_x) {
  __shared__ float2 zs[BL_CHUNK];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i = ti * BL_T + (tid >> 4), j = tj * BL_T + (tid & 15);
  const float px = (float)(d * j) + 0.5f * (float)d, py = (float)(d * i) + 0.5f * (float)d;
  const int N = cnt[s];
  const float2* z = pts + begins[s];
  float m2 = 3.0e38f;
  for (int c0 = 0; c0 < N; c0 += BL_CHUNK) {
    if (c0 + tid < N) zs[tid] = z[c0 + tid];
    __syncthreads();
    const int nn = min(BL_CHUNK, N - c0);
    for (int t = 0; t < nn; ++t) {
      const float dx = px - zs[t].x, dy = py - zs[t].y;
      m2 = fminf(m2, __fmaf_rn(dx, dx, __fmul_rn(dy, dy)));
    }
    __syncthreads();
  }
  // the largest logit: k < 0 and the rounding of k * v is monotone in v, so it is the logit of dmin^2 (or l_0)
  const float dm = sqrtf(m2);
  const float l0 = bl_bg(dm, D, k);
  float mx = __fmul_rn(k, m2);
  if (bg) mx = fmaxf(mx, l0);
  float sum = 0.f;
  for (int c0 = 0; c0 < N; c0 += BL_CHUNK) {
    if (c0 + tid < N) zs[tid] = z[c0 + tid];
    __syncthreads();
    const int nn = min(BL_CHUNK, N - c0);
    for (int t = 0; t < nn; ++t) sum += expf(bl_logit(px, py, zs[t].x, zs[t].y, k) - mx);
    __syncthreads();
  }
  if (bg) sum += expf(l0 - mx);
  if (i < h && j < w) {
    const size_t o = ((size_t)s * h + i) * w + j;
    lse[o] = N > 0 ? mx + logf(sum) : 0.f;       // (no head: the posterior of the background is 1, lse unused)
    dmin[o] = N > 0 ? dm : 0.f;
  }
}

__global__ void __launch_bounds__(256) bayes_expect_kernel(const float2* __restrict__ pts,
                                                           const long long* __restrict__ begins,
                                                           const int* __restrict__ cnt, const float* __restrict__ et,
                                                           const float* __restrict__ lse, float* __restrict__ E, int h,
                                                           int w, int d, float k) {
  __shared__ float4 px[BE_PIX];                  // (x_m, y_m, lse_m, et_m)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.y;
  const long long base = begins[s];
  const long long slots = begins[s + 1] - base;  // the sample's slots in pts / E: its first cnt[s] hold heads
  const int N = cnt[s];
  const int b0 = blockIdx.x * BE_HPB, h0 = b0 + wave * BE_HPW;
  if (b0 >= slots) return;
  if (b0 >= N) {                                 // slots without a head: E = 0
    if (tid < BE_HPB && b0 + tid < slots) E[base + b0 + tid] = 0.f;
    return;
  }
  float zx[BE_HPW], zy[BE_HPW], acc[BE_HPW];
#pragma unroll
  for (int q = 0; q < BE_HPW; ++q) {
    const float2 z = (h0 + q < N) ? pts[base + h0 + q] : make_float2(0.f, 0.f);
    zx[q] = z.x, zy[q] = z.y, acc[q] = 0.f;
  }
  const int M = h * w;
  const float* ets = et + (size_t)s * M;
  const float* lss = lse + (size_t)s * M;
  for (int m0 = 0; m0 < M; m0 += BE_PIX) {
    const int nn = min(BE_PIX, M - m0);
    for (int e = tid; e < nn; e += 256) {
      const int m = m0 + e, i = m / w, j = m - i * w;
      px[e] = make_float4((float)(d * j) + 0.5f * (float)d, (float)(d * i) + 0.5f * (float)d, lss[m], ets[m]);
    }
    __syncthreads();
    if (h0 < N) {
      for (int e = lane; e < nn; e += 64) {
        const float4 v = px[e];
#pragma unroll
        for (int q = 0; q < BE_HPW; ++q)
          acc[q] = __fmaf_rn(expf(bl_logit(v.x, v.y, zx[q], zy[q], k) - v.z), v.w, acc[q]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < BE_HPW; ++q) {
    const float r = wave_sum(acc[q]);
    if (lane == 0 && h0 + q < slots) E[base + h0 + q] = (h0 + q < N) ? r : 0.f;
  }
}

// E_0 of every sample, one block each: sum_m p(0|m) et_m (0 for a sample with heads when rho = 0)
__global__ void __launch_bounds__(256) bayes_e0_kernel(const int* __restrict__ cnt, const float* __restrict__ et,
                                                       const float* __restrict__ lse, const float* __restrict__ dmin,
                                                       float* __restrict__ E0, int M, float k, float D, int bg) {
  __shared__ float red[4];
  const int s = blockIdx.x, N = cnt[s];
  const size_t o = (size_t)s * M;
  float acc = 0.f;
  if (N == 0) {
    for (int m = threadIdx.x; m < M; m += 256) acc += et[o + m];
  } else if (bg) {
    for (int m = threadIdx.x; m < M; m += 256)
      acc = __fmaf_rn(expf(bl_bg(dmin[o + m], D, k) - lse[o + m]), et[o + m], acc);
  }
  const float r = bl_block_sum(acc, red);
  if (threadIdx.x == 0) E0[s] = r;
}

// g [n][h][gp]: the first w columns of a row hold the gradient, the rest (gp > w: a width-padded map) zeros
__global__ void __launch_bounds__(256) bayes_grad_kernel(const float2* __restrict__ pts,
                                                         const long long* __restrict__ begins,
                                                         const int* __restrict__ cnt, const float* __restrict__ E,
                                                         const float* __restrict__ E0, const float* __restrict__ lse,
                                                         const float* __restrict__ dmin, float* __restrict__ g, int h,
                                                         int w, int gp, int d, float k, float D, int bg,
                                                         int tiles_x) {
  __shared__ float4 zs[BL_CHUNK];                // (zx, zy, sgn(E_n - 1), 0)
  const int tid = threadIdx.x, s = blockIdx.y;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i = ti * BL_T + (tid >> 4), j = tj * BL_T + (tid & 15);
  const bool live = i < h && j < w;
  const float px = (float)(d * j) + 0.5f * (float)d, py = (float)(d * i) + 0.5f * (float)d;
  const int N = cnt[s];
  const long long base = begins[s];
  const size_t o = ((size_t)s * h + (live ? i : 0)) * w + (live ? j : 0);
  const float ls = lse[o], dm = dmin[o];
  float acc = 0.f;
  for (int c0 = 0; c0 < N; c0 += BL_CHUNK) {
    if (c0 + tid < N) {
      const float2 z = pts[base + c0 + tid];
      zs[tid] = make_float4(z.x, z.y, bl_sgn(E[base + c0 + tid] - 1.f), 0.f);
    }
    __syncthreads();
    const int nn = min(BL_CHUNK, N - c0);
    for (int t = 0; t < nn; ++t) {
      const float4 z = zs[t];
      acc = __fmaf_rn(z.z, expf(bl_logit(px, py, z.x, z.y, k) - ls), acc);
    }
    __syncthreads();
  }
  const float s0 = bl_sgn(E0[s]);
  if (N == 0) acc = s0;
  else if (bg) acc = __fmaf_rn(s0, expf(bl_bg(dm, D, k) - ls), acc);
  if (i < h && j < gp) g[((size_t)s * h + i) * gp + j] = live ? acc : 0.f;
}

// the loss, one block: per sample sum_n |1 - E_n| (+ |E_0|), then the samples in index order
__global__ void __launch_bounds__(256) bayes_loss_kernel(const long long* __restrict__ begins,
                                                         const int* __restrict__ cnt, const float* __restrict__ E,
                                                         const float* __restrict__ E0, int n, int bg,
                                                         float* __restrict__ loss, float* __restrict__ nonfinite) {
  __shared__ float red[4];
  float total = 0.f;
  for (int s = 0; s < n; ++s) {
    const int N = cnt[s];
    const float* e = E + begins[s];
    float acc = 0.f;
    for (int t = threadIdx.x; t < N; t += 256) acc += fabsf(1.f - e[t]);
    float r = bl_block_sum(acc, red);
    if (bg || N == 0) r += fabsf(E0[s]);
    total += r;
  }
  if (threadIdx.x == 0) {
    loss[0] = total;
    if (nonfinite != nullptr) nonfinite[0] = isfinite(total) ? 0.f : 1.f;
  }
}

// The head backward for a given g [P] fp32 (indexed and width-padded like head_train's gt): head_train_kernel's lane
// layout, grid and per-block partials with gs = g * gscale in the place of 2 (et - gt) gscale, the loss slot zero.
template <int DT>
__global__ void __launch_bounds__(256) head_bwd_kernel(const uint4* __restrict__ y, const float* __restrict__ w,
                                                       const float* __restrict__ gp, uint4* __restrict__ dy,
                                                       float* __restrict__ part, int P, float gscale,
                                                       const float* __restrict__ lscale) {
  __shared__ float red[256 / 8][66];
  const float dys = (lscale != nullptr) ? lscale[0] : 1.f;   // loss scale: applied to dy only
  const int lane8 = threadIdx.x & 7;
  const int pg = threadIdx.x >> 3;
  float wl[8], dwl[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { wl[k] = w[lane8 * 8 + k]; dwl[k] = 0.f; }
  float dbl = 0.f;
  for (size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 3; p < (size_t)P; p += ((size_t)gridDim.x * 256) >> 3) {
    float v[8];
    unpack8h<DT>(y[p * 8 + lane8], v);
    float g = gp[p] * gscale;
    asm volatile("" : "+v"(g));                  // (rounded here, as head_train_kernel's g: not fused into the db sum)
    if (lane8 == 0) dbl += g;
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      // the product lands in a register as fp32 before the 16-bit conversion, as in head_train_kernel: left alone, the
      // compiler fuses the multiply into the fp16 conversion (one rounding, and the sign of a zero product is lost)
      float t = g * dys * wl[k];
      asm volatile("" : "+v"(t));
      o[k] = (v[k] > 0.f) ? t : 0.f;
      dwl[k] += g * v[k];
    }
    dy[p * 8 + lane8] = pack8h<DT>(o);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[pg][lane8 * 8 + k] = dwl[k];
  if (lane8 == 0) { red[pg][64] = dbl; red[pg][65] = 0.f; }
  __syncthreads();
  if (threadIdx.x < 66) {
    float s = 0.f;
    for (int r = 0; r < 256 / 8; ++r) s += red[r][threadIdx.x];
    part[(size_t)blockIdx.x * 66 + threadIdx.x] = s;
  }
}

}  // namespace can

// pts [T][2] and cnt [n] of n crop windows from a heads pack's table: heads [.][4] fp32 (16-byte aligned), ranges [n][2]
// and desc [n][8] int64 as can_gt_from_heads takes them, begins [n] int64 the first slot of every sample in pts (the
// running sum of the ranges' counts).  Everything on the device; the pack has passed can_gt_from_heads_check.
extern "C" int can_crop_points(const float* heads, const long long* ranges, const long long* desc,
                               const long long* begins, int n, float* pts, int* cnt, int CH, int CW, int ds,
                               void* stream) {
  using namespace can;
  if (n <= 0 || n > 65535 || ds <= 0 || CH <= 0 || CW <= 0 || CH % ds || CW % ds) return -2;
  if (ranges == nullptr || desc == nullptr || begins == nullptr || cnt == nullptr || ((uintptr_t)heads & 15) ||
      ((uintptr_t)pts & 7))
    return -2;
  hipLaunchKernelGGL(crop_points_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const float4*)heads, ranges,
                     desc, begins, (float2*)pts, cnt, CH, CW, ds);
  return (int)hipGetLastError();
}

// The three passes.  et [n][h][w] fp32 dense; pts [T][2]; begins [n + 1] int64 (begins[n] = T); cnt [n] int32, cnt[s] <=
// begins[s + 1] - begins[s] <= max_count (host-known: it sizes the expectation grid); lse, dmin [n][h][w] scratch;
// E [T + n] (the heads' E_n in their slots, 0 in a slot without a head, then E_0 of every sample); g [n][h][gpitch],
// gpitch >= w; loss / nonfinite as head_reduce_kernel writes them (nonfinite may be null).  passes: bit 0 normaliser,
// bit 1 expectation, bit 2 gradient and loss (7: all; the others are for timing one pass over a finished run).
extern "C" int can_bayes_loss(const float* et, const float* pts, const long long* begins, const int* cnt, int n, int h,
                              int w, long long T, int max_count, float sigma, float rho, int ch, int cw, int d,
                              float* lse, float* dmin, float* E, float* g, int gpitch, float* loss, float* nonfinite,
                              int passes, void* stream) {
  using namespace can;
  hipStream_t st = (hipStream_t)stream;
  if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || d <= 0 || ch != h * d || cw != w * d || gpitch < w || T < 0 ||
      max_count < 0 || max_count > T)
    return -2;
  if (!(sigma > 0.f) || !(rho >= 0.f) || (long long)h * gpitch > 0x7fffffff || (long long)ch * cw > 0x7fffffff)
    return -2;
  if (et == nullptr || begins == nullptr || cnt == nullptr || lse == nullptr || dmin == nullptr || E == nullptr ||
      g == nullptr || loss == nullptr || (T > 0 && pts == nullptr) || ((uintptr_t)pts & 7))
    return -2;
  const float k = (float)(-0.5 / ((double)sigma * (double)sigma));
  const float D = (float)((double)rho * (double)(ch < cw ? ch : cw));
  const int bg = rho > 0.f;
  const int ty = (h + BL_T - 1) / BL_T;
  if (passes & 1) {
    const int tx = (w + BL_T - 1) / BL_T;
    hipLaunchKernelGGL(bayes_norm_kernel, dim3(tx * ty, n), dim3(256), 0, st, (const float2*)pts, begins, cnt, lse,
                       dmin, h, w, d, k, D, bg, tx);
  }
  if (passes & 2) {
    if (max_count > 0)
      hipLaunchKernelGGL(bayes_expect_kernel, dim3((max_count + BE_HPB - 1) / BE_HPB, n), dim3(256), 0, st,
                         (const float2*)pts, begins, cnt, et, lse, E, h, w, d, k);
    hipLaunchKernelGGL(bayes_e0_kernel, dim3(n), dim3(256), 0, st, cnt, et, lse, dmin, E + T, h * w, k, D, bg);
  }
  if (passes & 4) {
    const int tx = (gpitch + BL_T - 1) / BL_T;
    hipLaunchKernelGGL(bayes_grad_kernel, dim3(tx * ty, n), dim3(256), 0, st, (const float2*)pts, begins, cnt, E,
                       E + T, lse, dmin, g, h, w, gpitch, d, k, D, bg, tx);
    hipLaunchKernelGGL(bayes_loss_kernel, dim3(1), dim3(256), 0, st, begins, cnt, E, E + T, n, bg, loss, nonfinite);
  }
  return (int)hipGetLastError();
}

// dy, dw, db of the head for a given g [P]: head_bwd_kernel, then the head's own reduction (can_head_reduce) with a
// scratch loss slot and no non-finite flag, so the flags of the loss pass stand.  beta as can_head_train's.
extern "C" int can_head_bwd(const void* y, const float* w, const float* g, void* dy, float* part, int nblk, float* dw,
                            float* db, float* scratch, int P, float gscale, float beta, const float* lscale, int dt,
                            void* stream) {
  using namespace can;
  if (P <= 0 || nblk <= 0 || y == nullptr || w == nullptr || g == nullptr || dy == nullptr || part == nullptr ||
      dw == nullptr || db == nullptr || scratch == nullptr)
    return -2;
  CAN_LAUNCH_DT(dt, head_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint4*)y, w, g, (uint4*)dy,
                part, P, gscale, lscale);
  return can_head_reduce(part, nblk, dw, db, scratch, beta, nullptr, stream);
}
