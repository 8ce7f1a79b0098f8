// Geometry-adaptive Gaussian density-map generator on the GPU (gfx950).
//
// Reference: data_preparation/k_nearest_gaussian_kernel.py:14-54 — KD-tree
// 4-NN query, sigma = 0.1 * (d1 + d2 + d3) (avg(shape)/4 for a single
// head), a unit delta at (int(y), int(x)) filtered by scipy gaussian_filter
// (mode='constant', truncate=4.0), summed over heads: O(N*H*W) on the CPU,
// "one minute or more per thousand heads".
//
// Here: (1) knn: one thread per head, brute-force over all heads staged
// through LDS in 256-point tiles, keeping the 4 smallest squared distances
// (self included, like the tree query); (2) splat: one workgroup per head
// writes the clipped outer product of two normalised 1-D Gaussians of radius
// R = int(4*sigma + 0.5) — exactly what gaussian_filter does to a delta
// (SURVEY §2.7), for any radius (the sigma = (H+W)/8 single-head case at
// 768x1024 has R = 896) — with fp32 atomics (the sum order across heads is not fixed:
// bitwise run-to-run reproducibility is NOT guaranteed, equality to ~1e-7 is).
#include "common.h"

namespace can {

__global__ void __launch_bounds__(256) density_knn_kernel(const float2* __restrict__ pts, int n,
                                                          float* __restrict__ sigma, float single_sigma) {
  __shared__ float2 tile[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float2 me = (i < n) ? pts[i] : make_float2(0.f, 0.f);
  float d[4] = {3.4e38f, 3.4e38f, 3.4e38f, 3.4e38f};
  for (int base = 0; base < n; base += 256) {
    const int j = base + threadIdx.x;
    tile[threadIdx.x] = (j < n) ? pts[j] : make_float2(3.0e18f, 3.0e18f);
    __syncthreads();
    const int cnt = min(256, n - base);
    for (int t = 0; t < cnt; ++t) {
      const float dx = tile[t].x - me.x, dy = tile[t].y - me.y;
      float v = dx * dx + dy * dy;
      // insertion into the sorted 4-list
      if (v < d[3]) {
        if (v < d[2]) {
          d[3] = d[2];
          if (v < d[1]) {
            d[2] = d[1];
            if (v < d[0]) { d[1] = d[0]; d[0] = v; }
            else d[1] = v;
          } else d[2] = v;
        } else d[3] = v;
      }
    }
    __syncthreads();
  }
  if (i < n) {
    if (n == 1) sigma[i] = single_sigma;
    else {
      // k=4 with fewer than 4 points: scipy returns inf distances -> sigma inf;
      // the reference then filters with an infinite sigma (degenerate).  Use the
      // available neighbours only.
      float s = 0.f;
      for (int k = 1; k < 4 && k < n; ++k) s += sqrtf(d[k]);
      sigma[i] = 0.1f * s;
    }
  }
}

// one block per head; threads cover the clipped (2R+1)^2 footprint.  Any radius: the normaliser
// sum_{t=-R..R} exp(-t^2 / 2 s^2) is a block reduction over the WHOLE kernel (mass outside the image is
// dropped after normalising, like gaussian_filter on a delta), the 1-D weights are tabulated in dynamic
// LDS only over the clipped window (<= H rows + W columns).  max_r > 0 optionally caps R.
__global__ void __launch_bounds__(256) density_splat_kernel(const float2* __restrict__ pts,
                                                            const float* __restrict__ sigma, int n, int H, int W,
                                                            float* __restrict__ out, int max_r) {
  extern __shared__ float tab[];                 // [H] row weights, then [W] column weights
  __shared__ float red[4];
  const int i = blockIdx.x;
  if (i >= n) return;
  const float2 p = pts[i];
  const int px = (int)p.x, py = (int)p.y;      // python int() truncation
  if (p.x < 0.f || p.y < 0.f || px >= W || py >= H) return;   // reference skips out-of-image heads
  const float s = sigma[i];
  if (s <= 0.f) {   // degenerate: delta
    if (threadIdx.x == 0) atomicAdd(out + (size_t)py * W + px, 1.f);
    return;
  }
  const float rf = 4.0f * s + 0.5f;
  int R = (rf >= 2.0e9f) ? 2000000000 : (int)rf;
  if (max_r > 0 && R > max_r) R = max_r;
  const float k = -0.5f / (s * s);
  // normaliser over the full 2R+1 taps (fixed per-thread stride order + fixed tree: deterministic)
  float part = 0.f;
  for (long long t = (long long)threadIdx.x - R; t <= R; t += 256) {
    const float x = (float)t;
    part += __expf(k * x * x);
  }
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  const float inv_sum = 1.f / ((red[0] + red[1]) + (red[2] + red[3]));
  const int y0 = max(0, py - R), y1 = min(H - 1, py + R);
  const int x0 = max(0, px - R), x1 = min(W - 1, px + R);
  const int w = x1 - x0 + 1, h = y1 - y0 + 1;
  float* ky = tab;
  float* kx = tab + h;
  for (int t = threadIdx.x; t < h; t += 256) {
    const float d = (float)(y0 + t - py);
    ky[t] = __expf(k * d * d) * inv_sum;
  }
  for (int t = threadIdx.x; t < w; t += 256) {
    const float d = (float)(x0 + t - px);
    kx[t] = __expf(k * d * d) * inv_sum;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < w * h; t += 256) {
    const int yy = t / w, xx = t - yy * w;
    atomicAdd(out + (size_t)(y0 + yy) * W + x0 + xx, ky[yy] * kx[xx]);
  }
}

__global__ void density_fill_kernel(float* __restrict__ sigma, int n, float v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) sigma[i] = v;
}


// ---------------------------------------------------------------------------------------------------------------
// Ground truth of crop windows straight from head records (c, r, sigma, R): no density map is resampled.  Cell (i, j)
// of a sample is the exact area sum of the density over its source rectangle, which is separable per head:
// gt[i][j] = sum_h Py_h[i] * Px_h[j], Py_h[i] = sum_p overlap_i(p) * k_h[p - r_h], the overlaps integers over the
// number of cells (README, "Ground truth from heads").  Grid (16 x 16 cell tile, sample).  A block walks its sample's
// head range in chunks of GH_CHUNK: heads whose footprint misses the tile's source rectangle are dropped by an ORDERED
// compaction (they would add exactly +0), one wave per surviving head sums the normaliser over the whole 2R + 1 taps
// (1 + 2 * sum_{t=1..R}, the kernel is even), the block tabulates the 16 + 16 profile entries of every survivor in
// LDS (eight lanes per survivor, over the entries that have taps), and each thread runs one fma per survivor for its cell: table order, no atomics, bitwise repeatable.
constexpr int GH_CHUNK = 256;
constexpr int GH_T = 16;

// sum over the source pixels p (window-relative) of cell i's integer overlap with p times exp(k (p - q)^2), |p - q| <= R.
// In units of 1 / cells of a pixel, cell i is [i ext, (i + 1) ext) and pixel p is [p cells, (p + 1) cells).
__device__ __forceinline__ float gh_entry(int i, int ext, int cells, int q, int R, float k) {
  const int lo = i * ext, hi = lo + ext;
  const long long pa = max((long long)(lo / cells), (long long)q - R);
  const long long pb = min((long long)((hi - 1) / cells), (long long)q + R);
  float s = 0.f;
  for (long long pl = pa; pl <= pb; ++pl) {
    const int p = (int)pl;
    const int ov = min((p + 1) * cells, hi) - max(p * cells, lo);
    const float x = (float)(p - q);
    s = fmaf((float)ov, __expf(k * x * x), s);
  }
  return s;
}

__global__ void __launch_bounds__(256) gt_from_heads_kernel(const float4* __restrict__ heads,
                                                            const long long* __restrict__ ranges,
                                                            const long long* __restrict__ desc, float* __restrict__ gt,
                                                            int rows, int cols, int CH, int CW, int ds, int tiles_x) {
  __shared__ float prof[GH_CHUNK][2 * GH_T];     // [survivor][16 row entries | 16 column entries]
  __shared__ int4 hd[GH_CHUNK];                  // survivor: (c - x0, r - y0, R, bits of k)
  __shared__ float inv[GH_CHUNK];
  __shared__ int wcount[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.y;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int ty = tid >> 4, tx = tid & 15;
  const long long* d = desc + (size_t)s * 8;
  const int flip = (int)d[4], y0 = (int)d[5], x0 = (int)d[6];
  int sh, sw, vrows = rows, vcols = cols;
  if (d[7] == 1) {                               // unscaled: the valid extent of crop_window, the rest is padding
    sh = min((long long)CH, d[1] / ds * ds), sw = min((long long)CW, d[2] / ds * ds);
    vrows = sh / ds, vcols = sw / ds;
  } else {
    sh = (int)(d[7] >> 32), sw = (int)(d[7] & 0xffffffffll);
  }
  const long long begin = ranges[2 * (size_t)s], count = ranges[2 * (size_t)s + 1];
  const int i0 = ti * GH_T, j0 = tj * GH_T;
  const int i1 = min(i0 + GH_T, vrows), j1 = min(j0 + GH_T, vcols);
  const bool live = i0 < vrows && j0 < vcols;    // a tile of padding only writes zeros
  // the tile's source rectangle, window-relative, both ends included
  const int ya = live ? (int)((long long)i0 * sh / vrows) : 0, yb = live ? (int)(((long long)i1 * sh - 1) / vrows) : -1;
  const int xa = live ? (int)((long long)j0 * sw / vcols) : 0, xb = live ? (int)(((long long)j1 * sw - 1) / vcols) : -1;
  float acc = 0.f;
  for (long long base = 0; live && base < count; base += GH_CHUNK) {
    const long long idx = base + tid;
    bool hit = false;
    int qx = 0, qy = 0, R = 0;
    float k = 0.f;
    if (idx < count) {
      const float4 h = heads[begin + idx];
      qx = (int)h.x - x0, qy = (int)h.y - y0;
      if (h.z > 0.f) {                           // sigma <= 0: a unit delta (R = 0, exp(0 * 0) = 1, normaliser 1)
        R = (int)h.w;
        k = -0.5f / fmaxf(h.z * h.z, 1e-30f);
      }
      hit = (long long)qy + R >= ya && (long long)qy - R <= yb && (long long)qx + R >= xa && (long long)qx - R <= xb;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int slot = __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += wcount[w];
    const int m = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    if (hit) hd[slot] = make_int4(qx, qy, R, __float_as_int(k));
    __syncthreads();
    for (int e = tid; e < m * 2 * GH_T; e += 256) (&prof[0][0])[e] = 0.f;
    for (int t = wave; t < m; t += 4) {          // one wave per survivor: the normaliser over the whole kernel
      const int Rt = hd[t].z;
      const float kt = __int_as_float(hd[t].w);
      float part = 0.f;
      for (int u = 1 + lane; u <= Rt; u += 64) {
        const float x = (float)u;
        part += __expf(kt * x * x);
      }
      part = wave_sum(part);
      if (lane == 0) inv[t] = 1.f / (1.f + 2.f * part);
    }
    __syncthreads();
    // the entries that have taps: a survivor's footprint, cut to the tile's source rectangle, covers the pixels
    // [pa, pb] of an axis, which overlap the contiguous cells [pa cells / ext, ((pb + 1) cells - 1) / ext]; every
    // other entry stays the 0 written above.  Eight lanes per survivor walk its row cells, then its column cells (a
    // small head reaches two or three cells of an axis: one lane per entry left most of a wave idle).
    for (int e = tid; e < m * 8; e += 256) {
      const int t = e >> 3;
      const int4 h = hd[t];
      const float kt = __int_as_float(h.w), sc = inv[t];
      const int pya = (int)max((long long)ya, (long long)h.y - h.z), pyb = (int)min((long long)yb, (long long)h.y + h.z);
      const int pxa = (int)max((long long)xa, (long long)h.x - h.z), pxb = (int)min((long long)xb, (long long)h.x + h.z);
      const int ia = max(i0, pya * vrows / sh), ib = min(i1 - 1, ((pyb + 1) * vrows - 1) / sh);
      const int ja = max(j0, pxa * vcols / sw), jb = min(j1 - 1, ((pxb + 1) * vcols - 1) / sw);
      const int nr = max(0, ib - ia + 1), nc = max(0, jb - ja + 1);
      for (int u = e & 7; u < nr + nc; u += 8) {
        const bool row = u < nr;
        const int cell = row ? ia + u : ja + u - nr, cells = row ? vrows : vcols;
        const float v = gh_entry(cell, row ? sh : sw, cells, row ? h.y : h.x, h.z, kt) * sc / (float)cells;
        prof[t][row ? cell - i0 : GH_T + cell - j0] = v;
      }
    }
    __syncthreads();
    for (int t = 0; t < m; ++t) acc = fmaf(prof[t][ty], prof[t][GH_T + tx], acc);
    __syncthreads();
  }
  const int i = i0 + ty, j = j0 + tx;            // j: the column before the flip
  if (i < rows && j < cols) {
    const int jo = (flip && j < vcols) ? vcols - 1 - j : j;
    gt[(size_t)s * rows * cols + (size_t)i * cols + jo] = acc;
  }
}

}  // namespace can

// fixed_sigma > 0: every head gets that sigma (no kNN; the synthetic-data generator's fixed-width heads)
extern "C" int can_density_map(const float* pts, int n, int H, int W, float* sigma_ws, float* out, int max_r,
                               void* stream, float fixed_sigma) {
  using namespace can;
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return 0;
  const size_t lds = (size_t)(H + W) * sizeof(float);
  if (lds > 150 * 1024) return -2;                      // weight tables of one clipped footprint in LDS
  if (fixed_sigma > 0.f) {
    hipLaunchKernelGGL(density_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, sigma_ws, n, fixed_sigma);
  } else {
    const float single = 0.25f * 0.5f * (float)(H + W);   // avg(shape)/2/2 (reference intent, Q9)
    hipLaunchKernelGGL(density_knn_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float2*)pts, n, sigma_ws,
                       single);
  }
  if (lds > 64 * 1024)
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)density_splat_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
  hipLaunchKernelGGL(density_splat_kernel, dim3(n), dim3(256), lds, s, (const float2*)pts, sigma_ws, n, H, W, out,
                     max_r);
  return (int)hipGetLastError();
}

// The host copies of a gt_from_heads launch, checked before it: 0, or -2 arguments (a crop that is no multiple of ds
// among them), -3 a window that is empty or leaves its image, -4 a head range that leaves the table, -5 a radius that is
// negative, no integer or above 2^24, -6 a sigma that is not finite, -7 a head that is no integer pixel of its image.
extern "C" int can_gt_from_heads_check(const float* heads_host, long long n_heads, const long long* ranges_host,
                                       const long long* desc_host, int n, int CH, int CW, int ds) {
  if (n <= 0 || n > 65535 || ds <= 0 || CH <= 0 || CW <= 0 || CH % ds || CW % ds) return -2;
  if (n_heads < 0 || ranges_host == nullptr || desc_host == nullptr || (n_heads > 0 && heads_host == nullptr)) return -2;
  if ((long long)(CH / ds) * (CW / ds) > 0x7fffffff) return -2;
  long long seen_b = -1, seen_c = -1, seen_h = -1, seen_w = -1;
  for (int i = 0; i < n; ++i) {
    const long long* d = desc_host + (size_t)i * 8;
    const long long H0 = d[1], W0 = d[2], flip = d[4], y0 = d[5], x0 = d[6];
    if (H0 <= 0 || W0 <= 0 || H0 > 0x7fffffff || W0 > 0x7fffffff || (flip != 0 && flip != 1)) return -3;
    long long sh, sw, vr = CH / ds, vc = CW / ds;
    if (d[7] == 1) {
      sh = H0 / ds * ds < CH ? H0 / ds * ds : CH, sw = W0 / ds * ds < CW ? W0 / ds * ds : CW;
      vr = sh / ds, vc = sw / ds;
    } else {
      sh = d[7] >> 32, sw = d[7] & 0xffffffffll;
      if (d[7] <= 1 || sh < 1 || sw < 1) return -3;
    }
    if (y0 < 0 || x0 < 0 || y0 > H0 - sh || x0 > W0 - sw) return -3;
    if (sh * vr > 0x7fffffff || sw * vc > 0x7fffffff) return -3;       // the kernel's integer overlaps
    const long long b = ranges_host[2 * (size_t)i], c = ranges_host[2 * (size_t)i + 1];
    if (b < 0 || c < 0 || b > n_heads || c > n_heads - b) return -4;
    if (b == seen_b && c == seen_c && H0 == seen_h && W0 == seen_w) continue;   // the K crops of one image
    for (long long t = b; t < b + c; ++t) {
      const float* h = heads_host + 4 * (size_t)t;
      if (!(h[2] - h[2] == 0.f)) return -6;
      if (!(h[3] >= 0.f) || h[3] > 16777216.f || h[3] != (float)(long long)h[3]) return -5;
      if (!(h[0] >= 0.f && h[0] < (float)W0 && h[1] >= 0.f && h[1] < (float)H0) || h[0] != (float)(long long)h[0] ||
          h[1] != (float)(long long)h[1])
        return -7;
    }
    seen_b = b, seen_c = c, seen_h = H0, seen_w = W0;
  }
  return 0;
}

// gt [n][1][CH/ds][CW/ds] of n windows from the head table: heads [n_heads][4] fp32 (c, r, sigma, R), ranges [n][2]
// int64 (first head, head count) and the crop launch's descriptors [n][8], each on the device and on the host, where
// can_gt_from_heads_check runs first (its code is returned, nothing is launched).  Every cell is written.
extern "C" int can_gt_from_heads(const float* heads, const long long* ranges, const long long* desc,
                                 const float* heads_host, long long n_heads, const long long* ranges_host,
                                 const long long* desc_host, int n, float* gt, int CH, int CW, int ds, void* stream) {
  using namespace can;
  const int rc = can_gt_from_heads_check(heads_host, n_heads, ranges_host, desc_host, n, CH, CW, ds);
  if (rc != 0) return rc;
  if (ranges == nullptr || desc == nullptr || gt == nullptr || (n_heads > 0 && heads == nullptr) ||
      ((uintptr_t)heads & 15))
    return -2;
  const int rows = CH / ds, cols = CW / ds;
  const int tiles_x = (cols + GH_T - 1) / GH_T, tiles_y = (rows + GH_T - 1) / GH_T;
  if ((long long)tiles_x * tiles_y > 0x7fffffff) return -2;
  hipLaunchKernelGGL(gt_from_heads_kernel, dim3(tiles_x * tiles_y, n), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)heads, ranges, desc, gt, rows, cols, CH, CW, ds, tiles_x);
  return (int)hipGetLastError();
}
