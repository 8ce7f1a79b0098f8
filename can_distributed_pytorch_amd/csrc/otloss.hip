// DM-Count loss (Wang et al., NeurIPS 2020) on head records, gfx950 wave64, fp32 (README, "DM-Count loss").
//
// A sample has a crop (ch, cw), a downsample d, a map et [h][w] (M = h w cells, cell m = (i, j) at x_m = (d j + d / 2,
// d i + d / 2)) and N heads z_n.  p = |et|, P = sum p, a = p / (P + 1e-8), b_n = 1 / N.  Three terms:
//   count   L_c = |N - P|
//   OT      T Sinkhorn iterations on the Gibbs kernel K_nm = B_ni A_nj, A_nj = exp(-(s (x_j - zx_n))^2 / eps),
//           B_ni = exp(-(s (y_i - zy_n))^2 / eps), s = 2 / max(ch, cw):  u = 1 / M;  v = b / (K u), u = a / (K^T v);
//           beta = eps log(u + 1e-16), alpha = eps log(v + 1e-16), L_ot = <a, beta> + <b, alpha>,
//           G = P / (P^2 + 1e-8) beta - <p, beta> / (P^2 + 1e-8)
//   TV      q_m = heads in cell m, r = sgn(a - q / N), L_tv = N sum |a - q / N|, dL_tv/dp = N / (P + 1e-8) (r - <a, r>)
//   g = sgn(et) (sgn(P - N) + w_ot G + w_tv dL_tv/dp);  a sample with N = 0 or P = 0 has the count term alone.
//
// K is never formed: it is an outer product per head, so both products of an iteration are small dense GEMMs on
// v_mfma_f32_16x16x4_f32 whose operands are the N (h + w) exponentials the setup launch wrote once.
//   ot_setup    grid (cell blocks + head blocks, sample): P, a, q, u = 1 / M per cell (q by comparing the cell of every
//               head, staged through LDS, with the thread's own: no atomics); the rows of A [. x wp] and
//               B [. x hp] (hp, wp: h, w rounded up to 16, zeros in the padding) per 16 heads
//   ot_iter     grid (head tile, sample), TILE = 16 / 32 / 64 heads per block (host: from max_count).  The tile's A and B
//               rows and the whole u go to LDS with zeros in every padding row and column.  R^T = U A_tile^T
//               ([hp x wp] [wp x TILE]) on MFMA, one 16 x 16 block per wave at a time; each lane dots its four
//               accumulators with B (K u = rowdot(B, R)), a butterfly over the four lane groups and a fixed-order sum
//               over the row blocks finish K u, v = b / (K u).  B is scaled by v in place and the tile's partial
//               S = (B v)^T A_tile ([hp x TILE] [TILE x wp]) goes to part[sample][tile] through MFMA again.
//   ot_reduce   grid (cell blocks, sample): the tiles' partials in tile order, u = a / S; the last one writes beta
//   ot_tail     one block per sample: the sums, the three terms, g (zeros in a width-padded map's padding columns);
//               block 0 goes on over the other samples in index order -> the loss and its non-finite flag
//               (head_reduce_kernel's contract)
// 2 T + 2 launches, separated by stream order alone: no grid barrier, no spin wait, no atomics, no read-back, no grid
// that depends on a device-side count (blocks past cnt[s] leave at once, the reduce reads ceil(cnt[s] / TILE) tiles).
// Every sum has a fixed order, so all outputs are bitwise repeatable.
//
// LDS pitches are 4 mod 16 floats.  The first GEMM reads 16 rows x 4 consecutive floats per MFMA operand, which that
// pitch spreads over all banks; the second reads 4 rows x 16 consecutive floats, and takes rows 4 apart (the k index of
// an MFMA step may name any four heads, as long as both operands agree) for the same effect.
#include "common.h"
#include "api.h"

namespace can {

constexpr int OT_PAD = 4;                        // LDS row padding in floats
constexpr int OT_HB = 16;                        // heads per setup block
constexpr float OT_TINY = 1e-16f, OT_DEN = 1e-8f;

__device__ __forceinline__ float ot_gibbs(float x, float z, float sc, float eps) {
  const float t = (x - z) * sc;
  return expf(-(t * t) / eps);
}

// the cell of coordinate z among n cells of d pixels: floor(z / d), exact for any d, the outer cells open outwards
__device__ __forceinline__ int ot_cell(float z, int d, int n) {
  z = fminf(fmaxf(z, 0.f), (float)(d * n));
  int c = (int)(z / (float)d);
  if ((float)(d * c) > z) --c;
  if ((float)(d * c + d) <= z) ++c;
  return min(max(c, 0), n - 1);
}

__global__ void __launch_bounds__(256) ot_setup_kernel(const float* __restrict__ et, const float2* __restrict__ pts,
                                                       const long long* __restrict__ begins,
                                                       const int* __restrict__ cnt, float* __restrict__ Pb,
                                                       float* __restrict__ a, float* __restrict__ q,
                                                       float* __restrict__ u, float* __restrict__ Ar,
                                                       float* __restrict__ Br, int h, int w, int hp, int wp, int d,
                                                       float sc, float eps, int cell_blocks) {
  __shared__ float red[4];
  __shared__ int4 cs[64];                        // the cells of 256 heads (-1: no head)
  const int tid = threadIdx.x, s = blockIdx.y, M = h * w;
  const int N = cnt[s];
  const long long base = begins[s];
  if ((int)blockIdx.x < cell_blocks) {
    const float* e = et + (size_t)s * M;
    float acc = 0.f;                             // P: the same fixed order in every cell block of the sample
    for (int m = tid; m < M; m += 256) acc += fabsf(e[m]);
    const float P = bl_block_sum(acc, red);
    const int m = blockIdx.x * 256 + tid;
    int qc = 0;                                  // q: the heads of cell m, the heads' cells through LDS in chunks of 256
    for (int c0 = 0; c0 < N; c0 += 256) {
      int cell = -1;
      if (c0 + tid < N) {
        const float2 z = pts[base + c0 + tid];
        cell = ot_cell(z.y, d, h) * w + ot_cell(z.x, d, w);
      }
      ((int*)cs)[tid] = cell;
      __syncthreads();
#pragma unroll 8
      for (int t = 0; t < 64; ++t) {
        const int4 c = cs[t];
        qc += (c.x == m) + (c.y == m) + (c.z == m) + (c.w == m);
      }
      __syncthreads();
    }
    if (m < M) {
      const size_t o = (size_t)s * M + m;
      a[o] = fabsf(e[m]) / (P + OT_DEN);
      q[o] = (float)qc;
      u[o] = 1.f / (float)M;
    }
    if (blockIdx.x == 0 && tid == 0) Pb[s] = P;
    return;
  }
  const int n0 = ((int)blockIdx.x - cell_blocks) * OT_HB, row = wp + hp;
  if (n0 >= N) return;
  for (int e = tid; e < OT_HB * row; e += 256) {
    const int r = e / row, c = e - r * row, n = n0 + r;
    if (n >= N) continue;
    const float2 z = pts[base + n];
    const float half = 0.5f * (float)d;
    if (c < wp)
      Ar[(size_t)(base + n) * wp + c] = c < w ? ot_gibbs((float)(d * c) + half, z.x, sc, eps) : 0.f;
    else
      Br[(size_t)(base + n) * hp + (c - wp)] = c - wp < h ? ot_gibbs((float)(d * (c - wp)) + half, z.y, sc, eps) : 0.f;
  }
}

// a tile's rows of a [. x cols] matrix (cols a multiple of 4, rows 16-byte aligned) into LDS at pitch cols + OT_PAD,
// zeros in the rows from `live` on.  Loads go out four at a time before the first store waits for one: a loop of
// load-then-store pays one round trip to memory per element.
template <int TILE>
__device__ __forceinline__ void ot_stage(float* dst, const float* __restrict__ src, int cols, int live) {
  const int c4 = cols >> 2, pitch = cols + OT_PAD, total = TILE * c4;
  for (int e0 = threadIdx.x; e0 < total; e0 += 4 * 256) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + 256 * k, r = e / c4, c = e - r * c4;
      v[k] = (e < total && r < live) ? ((const float4*)(src + (size_t)r * cols))[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + 256 * k, r = e / c4, c = e - r * c4;
      if (e < total) *(float4*)(dst + r * pitch + 4 * c) = v[k];
    }
  }
}

template <int TILE>
__global__ void __launch_bounds__(256) ot_iter_kernel(const float* __restrict__ Ar, const float* __restrict__ Br,
                                                      const long long* __restrict__ begins,
                                                      const int* __restrict__ cnt, const float* __restrict__ Pb,
                                                      const float* __restrict__ u, float* __restrict__ v,
                                                      float* __restrict__ part, int h, int w, int hp, int wp,
                                                      int ntiles) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, gq = lane >> 4;
  const int s = blockIdx.y, tile = blockIdx.x, n0 = tile * TILE, M = h * w;
  const int N = cnt[s];
  if (n0 >= N || !(Pb[s] > 0.f)) return;         // (uniform over the block; P = 0: the count term alone)
  const int PU = wp + OT_PAD, PA = wp + OT_PAD, PB = hp + OT_PAD, NI = hp >> 4, NJ = wp >> 4, NH = TILE >> 4;
  float* Us = lds;                               // [hp][PU]
  float* As = Us + hp * PU;                      // [TILE][PA]
  float* Bs = As + TILE * PA;                    // [TILE][PB]
  float* sp = Bs + TILE * PB;                    // [NI][TILE]: K u per row block
  float* vs = sp + NI * TILE;                    // [TILE]
  const long long base = begins[s] + n0;
  const int live = min(TILE, N - n0);
  const float* us = u + (size_t)s * M;
  for (int e0 = tid; e0 < hp * wp; e0 += 8 * 256) {          // (eight loads in flight, as in ot_stage)
    float uv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int e = e0 + 256 * k, i = e / wp, j = e - i * wp;
      uv[k] = (i < h && j < w) ? us[i * w + j] : 0.f;          // (e >= hp wp: i >= hp >= h)
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int e = e0 + 256 * k, i = e / wp, j = e - i * wp;
      if (e < hp * wp) Us[i * PU + j] = uv[k];
    }
  }
  ot_stage<TILE>(As, Ar + (size_t)base * wp, wp, live);
  ot_stage<TILE>(Bs, Br + (size_t)base * hp, hp, live);
  __syncthreads();

  // K u: block (is, hs) of R^T = U A^T is D[i = 16 is + 4 gq + r][n = 16 hs + c] in acc[r]
  for (int item = wave; item < NI * NH; item += 4) {
    const int is = item / NH, hs = item - is * NH;
    const float* ua = Us + (is * 16 + c) * PU + gq;
    const float* ab = As + (hs * 16 + c) * PA + gq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < wp; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[k0], ab[k0], acc, 0, 0, 0);
    const float4 bv = *(const float4*)(Bs + (hs * 16 + c) * PB + is * 16 + 4 * gq);
    float dot = acc[0] * bv.x;
    dot = __fmaf_rn(acc[1], bv.y, dot);
    dot = __fmaf_rn(acc[2], bv.z, dot);
    dot = __fmaf_rn(acc[3], bv.w, dot);
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    if (gq == 0) sp[is * TILE + hs * 16 + c] = dot;
  }
  __syncthreads();
  if (tid < TILE) {
    float ku = 0.f;
    for (int is = 0; is < NI; ++is) ku += sp[is * TILE + tid];
    const float vn = tid < live ? (1.f / (float)N) / ku : 0.f;
    vs[tid] = vn;
    if (tid < live) v[base + tid] = vn;
  }
  __syncthreads();
  for (int e = tid; e < TILE * hp; e += 256) {
    const int r = e / hp, i = e - r * hp;
    Bs[r * PB + i] *= vs[r];
  }
  __syncthreads();

  // the tile's K^T v: block (is, js) of (B v)^T A; step kk of the k loop names the heads 16 (kk / 4) + kk % 4 + 4 gq
  float* out = part + ((size_t)s * ntiles + tile) * M;
  for (int item = wave; item < NI * NJ; item += 4) {
    const int is = item / NJ, js = item - is * NJ;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < TILE / 4; ++kk) {
      const int n = ((kk >> 2) << 4) + (kk & 3) + 4 * gq;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Bs[n * PB + is * 16 + c], As[n * PA + js * 16 + c], acc, 0, 0, 0);
    }
    const int j = js * 16 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = is * 16 + 4 * gq + r;
      if (i < h && j < w) out[i * w + j] = acc[r];
    }
  }
}

__global__ void __launch_bounds__(256) ot_reduce_kernel(const float* __restrict__ part, const float* __restrict__ a,
                                                        const int* __restrict__ cnt, const float* __restrict__ Pb,
                                                        float* __restrict__ u, float* __restrict__ beta, int M,
                                                        int ntiles, int tile, float eps, int last) {
  const int s = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
  const int N = cnt[s];
  if (m >= M || N <= 0 || !(Pb[s] > 0.f)) return;
  const int nt = (N + tile - 1) / tile;
  const float* p = part + (size_t)s * ntiles * M + m;
  float S = 0.f;
#pragma unroll 8
  for (int t = 0; t < nt; ++t) S += p[(size_t)t * M];
  const size_t o = (size_t)s * M + m;
  const float un = a[o] / S;
  u[o] = un;
  if (last) beta[o] = eps * logf(un + OT_TINY);
}

struct OtSample {
  float Lc, Lot, Ltv, sc, ot0, ot1, tv0, tv1;    // G = ot0 beta - ot1, dL_tv/dp = tv0 (r - tv1)
  float invN;
  bool active;
};

// the sums of sample s over the whole block (every thread calls, every thread gets the result)
__device__ OtSample ot_sample(int s, const float* __restrict__ et, const float* __restrict__ a,
                              const float* __restrict__ q, const float* __restrict__ beta,
                              const float* __restrict__ v, const long long* __restrict__ begins,
                              const int* __restrict__ cnt, const float* __restrict__ Pb, int M, float eps,
                              float* red) {
  OtSample r;
  const int N = cnt[s];
  const float P = Pb[s], Nf = (float)N;
  r.Lc = fabsf(Nf - P);
  r.sc = bl_sgn(P - Nf);
  r.Lot = r.Ltv = r.ot0 = r.ot1 = r.tv0 = r.tv1 = r.invN = 0.f;
  r.active = N > 0 && P > 0.f;
  if (!r.active) return r;
  const size_t o = (size_t)s * M;
  const float invN = 1.f / Nf;
  float ab = 0.f, pb = 0.f, ar = 0.f, tv = 0.f, ba = 0.f;
  for (int m = threadIdx.x; m < M; m += 256) {
    const float am = a[o + m], bm = beta[o + m], df = am - q[o + m] * invN;
    ab = __fmaf_rn(am, bm, ab);
    pb = __fmaf_rn(fabsf(et[o + m]), bm, pb);
    ar = __fmaf_rn(am, bl_sgn(df), ar);
    tv += fabsf(df);
  }
  const float* vn = v + begins[s];
  for (int n = threadIdx.x; n < N; n += 256) ba = __fmaf_rn(invN, eps * logf(vn[n] + OT_TINY), ba);
  ab = bl_block_sum(ab, red);
  pb = bl_block_sum(pb, red);
  ar = bl_block_sum(ar, red);
  tv = bl_block_sum(tv, red);
  ba = bl_block_sum(ba, red);
  const float den = __fmaf_rn(P, P, OT_DEN);
  r.Lot = ab + ba;
  r.Ltv = Nf * tv;
  r.ot0 = P / den, r.ot1 = pb / den;
  r.tv0 = Nf / (P + OT_DEN), r.tv1 = ar;
  r.invN = invN;
  return r;
}

__device__ __forceinline__ float ot_total(const OtSample& r, float w_ot, float w_tv) {
  return (r.Lc + w_ot * r.Lot) + w_tv * r.Ltv;
}

// g [n][h][gp]: the first w columns of a row hold the gradient, the rest (gp > w: a width-padded map) zeros
__global__ void __launch_bounds__(256) ot_tail_kernel(const float* __restrict__ et, const float* __restrict__ a,
                                                      const float* __restrict__ q, const float* __restrict__ beta,
                                                      const float* __restrict__ v,
                                                      const long long* __restrict__ begins,
                                                      const int* __restrict__ cnt, const float* __restrict__ Pb,
                                                      float* __restrict__ g, float* __restrict__ terms, int n, int h,
                                                      int w, int gp, float eps, float w_ot, float w_tv,
                                                      float* __restrict__ loss, float* __restrict__ nonfinite) {
  __shared__ float red[4];
  const int s = blockIdx.x, M = h * w;
  const OtSample r = ot_sample(s, et, a, q, beta, v, begins, cnt, Pb, M, eps, red);
  const size_t o = (size_t)s * M;
  for (int e = threadIdx.x; e < h * gp; e += 256) {
    const int i = e / gp, j = e - i * gp;
    float gm = 0.f;
    if (j < w) {
      const int m = i * w + j;
      float t = r.sc;
      if (r.active) {
        const float G = r.ot0 * beta[o + m] - r.ot1;
        const float dtv = r.tv0 * (bl_sgn(a[o + m] - q[o + m] * r.invN) - r.tv1);
        t = (t + w_ot * G) + w_tv * dtv;
      }
      gm = bl_sgn(et[o + m]) * t;
    }
    g[(size_t)s * h * gp + e] = gm;
  }
  if (threadIdx.x == 0) {
    terms[3 * s] = r.Lc;
    terms[3 * s + 1] = r.Lot;
    terms[3 * s + 2] = r.Ltv;
  }
  if (s != 0) return;
  float total = ot_total(r, w_ot, w_tv);         // block 0: the samples in index order
  for (int s2 = 1; s2 < n; ++s2)
    total += ot_total(ot_sample(s2, et, a, q, beta, v, begins, cnt, Pb, M, eps, red), w_ot, w_tv);
  if (threadIdx.x == 0) {
    loss[0] = total;
    if (nonfinite != nullptr) nonfinite[0] = isfinite(total) ? 0.f : 1.f;
  }
}

static size_t ot_iter_lds(int tile, int hp, int wp) {
  return sizeof(float) * ((size_t)hp * (wp + OT_PAD) + (size_t)tile * (wp + OT_PAD) + (size_t)tile * (hp + OT_PAD) +
                          (size_t)(hp / 16) * tile + tile);
}

template <int TILE>
static void ot_launch_iter(dim3 grid, size_t lds, hipStream_t st, const float* Ar, const float* Br,
                           const long long* begins, const int* cnt, const float* Pb, const float* u, float* v,
                           float* part, int h, int w, int hp, int wp, int ntiles) {
  hipLaunchKernelGGL(ot_iter_kernel<TILE>, grid, dim3(256), lds, st, Ar, Br, begins, cnt, Pb, u, v, part, h, w, hp, wp,
                     ntiles);
}

}  // namespace can

// The DM-Count loss of et [n][h][w] fp32 (dense) against the points of a PointTarget (pts, begins [n + 1], cnt [n],
// T = begins[n], max_count the largest begins[s + 1] - begins[s]).  tile: 16, 32 or 64 heads per iteration block.
// Scratch, all fp32, hp / wp = h / w rounded up to 16: Ar [T][wp] and Br [T][hp] (16-byte aligned), u, a, q, beta
// [n][h][w], v [T], Pb [n], part [n][ceil(max_count / tile)][h][w].  g [n][h][gpitch], gpitch >= w; terms [n][3]
// (L_c, L_ot, L_tv, unweighted); loss / nonfinite as head_reduce_kernel writes them (nonfinite may be null).
// Everything is checked before the first launch: -2 for an argument out of range, -41 when u and a tile's rows do not
// fit the 64 KiB of LDS a block may have.
extern "C" int can_dmcount_loss(const float* et, const float* pts, const long long* begins, const int* cnt, int n, int h,
                                int w, long long T, int max_count, int tile, float eps, int iters, float w_ot,
                                float w_tv, int ch, int cw, int d, float* Ar, float* Br, float* u, float* v, float* a,
                                float* q, float* beta, float* Pb, float* part, float* g, int gpitch, float* terms,
                                float* loss, float* nonfinite, void* stream) {
  using namespace can;
  hipStream_t st = (hipStream_t)stream;
  if (n < 1 || n > 65535 || h < 1 || w < 1 || d < 1 || ch != h * d || cw != w * d || gpitch < w || T < 0 ||
      max_count < 0 || max_count > T || (tile != 16 && tile != 32 && tile != 64))
    return -2;
  if (!(eps >= 1.f && eps <= 100.f) || iters < 1 || iters > 1000 || !(w_ot >= 0.f && w_ot < INFINITY) ||
      !(w_tv >= 0.f && w_tv < INFINITY) || (long long)h * gpitch > 0x7fffffff || (long long)ch * cw > 0x7fffffff)
    return -2;
  if (et == nullptr || begins == nullptr || cnt == nullptr || u == nullptr || a == nullptr || q == nullptr ||
      beta == nullptr || Pb == nullptr || g == nullptr || terms == nullptr || loss == nullptr)
    return -2;
  if (T > 0 && (pts == nullptr || ((uintptr_t)pts & 7) || Ar == nullptr || ((uintptr_t)Ar & 15) || Br == nullptr ||
                ((uintptr_t)Br & 15) || v == nullptr || (max_count > 0 && part == nullptr)))
    return -2;
  const int hp = (h + 15) / 16 * 16, wp = (w + 15) / 16 * 16, M = h * w;
  const size_t lds = ot_iter_lds(tile, hp, wp);
  if (lds > 65536) return -41;
  const int cell_blocks = (M + 255) / 256, ntiles = (max_count + tile - 1) / tile;
  const float sc = (float)(2.0 / (double)(ch > cw ? ch : cw));
  hipLaunchKernelGGL(ot_setup_kernel, dim3(cell_blocks + (max_count + OT_HB - 1) / OT_HB, n), dim3(256), 0, st, et,
                     (const float2*)pts, begins, cnt, Pb, a, q, u, Ar, Br, h, w, hp, wp, d, sc, eps, cell_blocks);
  if (ntiles > 0) {
    const dim3 grid(ntiles, n);
    for (int t = 0; t < iters; ++t) {
      if (tile == 16) ot_launch_iter<16>(grid, lds, st, Ar, Br, begins, cnt, Pb, u, v, part, h, w, hp, wp, ntiles);
      else if (tile == 32) ot_launch_iter<32>(grid, lds, st, Ar, Br, begins, cnt, Pb, u, v, part, h, w, hp, wp, ntiles);
      else ot_launch_iter<64>(grid, lds, st, Ar, Br, begins, cnt, Pb, u, v, part, h, w, hp, wp, ntiles);
      hipLaunchKernelGGL(ot_reduce_kernel, dim3(cell_blocks, n), dim3(256), 0, st, part, a, cnt, Pb, u, beta, M, ntiles,
                         tile, eps, t == iters - 1);
    }
  }
  hipLaunchKernelGGL(ot_tail_kernel, dim3(n), dim3(256), 0, st, et, a, q, beta, v, begins, cnt, Pb, g, terms, n, h, w,
                     gpitch, eps, w_ot, w_tv, loss, nonfinite);
  return (int)hipGetLastError();
}
