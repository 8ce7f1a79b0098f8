// Memory-bound kernels of the CANNet step (gfx950): all NHWC bf16, 16-B
// vectorised per lane (8 channels), grid-stride, no atomics on hot paths.
//
//   maxpool2x2_fwd      nn.MaxPool2d(2,2)                  model/CANNet.py:112
//                       (+ optional max-pool codes: first-max one-hots, see conv_igemm.hip)
//   maxpool2x2_bwd_codes max-pool backward + ReLU mask from the codes alone
//   maxpool2x2_bwd_relu max_pool2d_with_indices_backward + threshold_backward
//                       (gather form: first-max-in-window wins, as ATen; the
//                       ReLU mask of the pooled layer is folded in)
//   head_fwd            output_layer 1x1 64->1 + bias       model/CANNet.py:17,90
//   head_train          head fwd + MSELoss(sum) + its backward + ReLU mask of
//                       the last backend layer, one pass      utils/train_eval_utils.py:20,37-38
//   sgd_momentum        torch.optim.SGD(momentum=0.95) step over the flat fp32
//                       arena, gradient averaging folded in, skipped on a
//                       device-side non-finite flag             train.py:126
//   img_to_nhwc4        [N,3,H,W] fp32 -> [N,H,W,4] bf16 (first-layer input)
#include "common.h"
#include "conv_epilogue.h"

namespace can {

// ---------------------------------------------------------------- maxpool
// codes (optional): per pooled pixel and 8-channel chunk, one uint32 of 4-bit one-hot first-max positions
// (ATen order, 0 when the max is not > 0) — the layout of the conv pool epilogues (conv_igemm.hip)
template <int DT>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                          uint32_t* __restrict__ codes, int N, int H, int W, int C8) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t total = (size_t)N * Ho * Wo * C8;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = i % C8;
    size_t p = i / C8;
    const int ox = p % Wo; p /= Wo;
    const int oy = p % Ho; const int n = p / Ho;
    const size_t base = (((size_t)n * H + 2 * oy) * W + 2 * ox) * C8 + c;
    float t[4][8], m[8];
    unpack8h<DT>(x[base], t[0]);
    unpack8h<DT>(x[base + C8], t[1]);
    unpack8h<DT>(x[base + (size_t)W * C8], t[2]);
    unpack8h<DT>(x[base + (size_t)W * C8 + C8], t[3]);
    pool_max(t, m);
    y[i] = pack8h<DT>(m);  // exact: max of bf16 values is a bf16 value
    if (codes != nullptr) codes[i] = pool_codes(t, m);
  }
}

// dx[full] = dy[pooled] at the window position the code marks, 0 elsewhere (max-pool backward + the ReLU
// mask of the pool input, from the codes alone: the pool input is not read)
template <int DT>
__global__ void __launch_bounds__(256) maxpool_bwd_codes_kernel(const uint32_t* __restrict__ codes,
                                                                const uint4* __restrict__ dy, uint4* __restrict__ dx,
                                                                int N, int H, int W, int C8) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t total = (size_t)N * Ho * Wo * C8;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = i % C8;
    size_t p = i / C8;
    const int ox = p % Wo; p /= Wo;
    const int oy = p % Ho; const int n = p / Ho;
    const size_t b0 = (((size_t)n * H + 2 * oy) * W + 2 * ox) * C8 + c;
    const size_t off[4] = {b0, b0 + C8, b0 + (size_t)W * C8, b0 + (size_t)W * C8 + C8};
    float g[8], o[4][8];
    unpack8h<DT>(dy[i], g);
    const uint32_t cw = codes[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t nib = (cw >> (4 * k)) & 0xFu;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q][k] = ((nib >> q) & 1u) ? g[k] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dx[off[q]] = pack8h<DT>(o[q]);
  }
}

// dx[full] = (x is the first max of its window) * (x > 0) * dy[pooled]
template <int DT>
__global__ void __launch_bounds__(256) maxpool_bwd_relu_kernel(const uint4* __restrict__ x, const uint4* __restrict__ dy,
                                                               uint4* __restrict__ dx, int N, int H, int W, int C8) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t total = (size_t)N * Ho * Wo * C8;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = i % C8;
    size_t p = i / C8;
    const int ox = p % Wo; p /= Wo;
    const int oy = p % Ho; const int n = p / Ho;
    const size_t b0 = (((size_t)n * H + 2 * oy) * W + 2 * ox) * C8 + c;
    const size_t off[4] = {b0, b0 + C8, b0 + (size_t)W * C8, b0 + (size_t)W * C8 + C8};
    float v[4][8], g[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) unpack8h<DT>(x[off[q]], v[q]);
    unpack8h<DT>(dy[i], g);
    float o[4][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      // ATen scan order: (0,0),(0,1),(1,0),(1,1); strict '>' keeps the first max
      int arg = 0;
      float mv = v[0][k];
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (v[q][k] > mv) { mv = v[q][k]; arg = q; }
      const float gg = (mv > 0.f) ? g[k] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q][k] = (q == arg) ? gg : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dx[off[q]] = pack8h<DT>(o[q]);
  }
}

// ---------------------------------------------------------------- head
// et[p] = sum_c y[p][c] * w[c] + b      (y: [P][64] bf16 post-ReLU)
// Width-padded map (rows of `pitch` pixels, the first wv valid; ops/executor.py "Ragged widths"): et = 0 at the
// padding columns (pitch <= wv: none)
__device__ __forceinline__ bool head_valid(size_t p, int pitch, int wv) {
  return pitch <= wv || (int)(p % (size_t)pitch) < wv;
}
template <int DT>
__global__ void __launch_bounds__(256) head_fwd_kernel(const uint4* __restrict__ y, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* __restrict__ et, int P,
                                                       int pitch, int wv) {
  // 8 lanes per pixel (8 channels each)
  const int lane8 = threadIdx.x & 7;
  float wl[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wl[k] = w[lane8 * 8 + k];
  const float bias = b[0];
  for (size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 3; p < (size_t)P; p += ((size_t)gridDim.x * 256) >> 3) {
    float v[8];
    unpack8h<DT>(y[p * 8 + lane8], v);
    float s = 0.f;   // explicit fma chain: head_fwd and head_train produce bitwise-identical et
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf(v[k], wl[k], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (lane8 == 0) et[p] = head_valid(p, pitch, wv) ? s + bias : 0.f;
  }
}

// Training head: et = y.w + b; loss = sum (et-gt)^2; det = 2(et-gt)*gscale;
// dy[p][c] = det * S * w[c] * (y > 0) (S = device loss scale, 1 if null); partial dw[c] = sum_p det*y[p][c], db = sum det.
// Per-block partials -> part[block][66] (64 dw, db, loss); reduced by head_reduce.  Padding columns of a
// width-padded map (head_valid) add nothing to the loss or the gradients (et = 0, dy = 0 there).
// WT (can_head_train with a weight plane): one more pointer, wt, P floats indexed and padded like gt, the per-pixel
// loss weight m: dm = m * d (one fp32 product), loss += dm * d, det = (2 * dm) * gscale; et stays unweighted.  With
// m = 1.0 dm is d itself, so every output is the WT = false kernel's bit for bit.
__device__ __forceinline__ const float* head_wt(const float* wt) { return wt; }
template <int DT, bool WT = false, typename... Wt>
__global__ void __launch_bounds__(256) head_train_kernel(const uint4* __restrict__ y, const float* __restrict__ w,
                                                         const float* __restrict__ b, const float* __restrict__ gt,
                                                         float* __restrict__ et, uint4* __restrict__ dy,
                                                         float* __restrict__ part, int P, float gscale,
                                                         const float* __restrict__ lscale, int pitch, int wv,
                                                         Wt... wt) {
  static_assert(sizeof...(Wt) == (WT ? 1 : 0), "the weight plane is the one extra argument of a WT kernel");
  __shared__ float red[256 / 8][66];
  const float dys = (lscale != nullptr) ? lscale[0] : 1.f;   // loss scale: applied to dy only
  const int lane8 = threadIdx.x & 7;
  const int pg = threadIdx.x >> 3;
  float wl[8], dwl[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { wl[k] = w[lane8 * 8 + k]; dwl[k] = 0.f; }
  const float bias = b[0];
  float dbl = 0.f, lossl = 0.f;
  for (size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 3; p < (size_t)P; p += ((size_t)gridDim.x * 256) >> 3) {
    float v[8];
    unpack8h<DT>(y[p * 8 + lane8], v);
    float s = 0.f;   // explicit fma chain: head_fwd and head_train produce bitwise-identical et
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf(v[k], wl[k], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    const bool valid = head_valid(p, pitch, wv);
    const float e = valid ? s + bias : 0.f;
    const float d = valid ? e - gt[p] : 0.f;
    float g;
    if constexpr (WT) {
      const float dm = head_wt(wt...)[p] * d;
      g = 2.f * dm * gscale;
      if (lane8 == 0) { et[p] = e; lossl += dm * d; dbl += g; }
    } else {
      g = 2.f * d * gscale;
      if (lane8 == 0) { et[p] = e; lossl += d * d; dbl += g; }
    }
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o[k] = (v[k] > 0.f) ? g * dys * wl[k] : 0.f;
      dwl[k] += g * v[k];
    }
    dy[p * 8 + lane8] = pack8h<DT>(o);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[pg][lane8 * 8 + k] = dwl[k];
  if (lane8 == 0) { red[pg][64] = dbl; red[pg][65] = lossl; }
  __syncthreads();
  if (threadIdx.x < 66) {
    float s = 0.f;
    for (int r = 0; r < 256 / 8; ++r) s += red[r][threadIdx.x];
    part[(size_t)blockIdx.x * 66 + threadIdx.x] = s;
  }
}

// out[0..63] = dw, out[64] = db, loss_out[0] = loss  (fixed-order, deterministic):
// 15 groups x 66 outputs, group g sums blocks g, g+15, ... then the 15 group
// sums are added in order (a single thread per output serialised ~1k loads).
// nonfinite (optional): 1.0 if the loss is inf/NaN, else 0.0 -- the
// reference's `if not isfinite(loss)` guard (utils/train_eval_utils.py:48)
// computed where the loss is produced, no extra launch.
__global__ void __launch_bounds__(1024) head_reduce_kernel(const float* __restrict__ part, int nblk,
                                                           float* __restrict__ dw, float* __restrict__ db,
                                                           float* __restrict__ loss, float beta,
                                                           float* __restrict__ nonfinite) {
  constexpr int G = 15;
  __shared__ float red[G][66];
  const int t = threadIdx.x;
  const int o = t % 66, g = t / 66;
  if (g < G) {
    float s0 = 0.f, s1 = 0.f;
    int i = g;
    for (; i + G < nblk; i += 2 * G) {
      s0 += part[(size_t)i * 66 + o];
      s1 += part[(size_t)(i + G) * 66 + o];
    }
    if (i < nblk) s0 += part[(size_t)i * 66 + o];
    red[g][o] = s0 + s1;
  }
  __syncthreads();
  if (t < 66) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < G; ++q) s += red[q][t];
    if (t < 64) dw[t] = (beta != 0.f) ? dw[t] * beta + s : s;
    else if (t == 64) db[0] = (beta != 0.f) ? db[0] * beta + s : s;
    else {
      loss[0] = s;
      if (nonfinite != nullptr) nonfinite[0] = isfinite(s) ? 0.f : 1.f;
    }
  }
}

// ---------------------------------------------------------------- SGD
// torch.optim.SGD semantics (dampening 0, nesterov False, wd 0):
//   buf = g (first step) | momentum*buf + g ;  p -= lr*buf,  g = grad*gscale.
// flags = {non-finite loss (all-reduced: any rank), loss, non-finite gradient
// (fp16 step), sticky "a non-finite loss happened since the last reset"}.
// flags[0] != 0 or flags[2] != 0 -> the whole update is skipped (graph-safe,
// no host sync); flags[0] != 0 also latches flags[3], which the host polls at
// its logging cadence (a NaN on a step it does not read is never lost).
// lr_dev (optional): the learning rate read from device memory, so a captured
// step follows an lr schedule (the host updates the scalar between replays).
// Vectorised float4 over a 16-B aligned arena.
//
// The prologue of every kernel that steps under the flags (sgd_momentum, pack_multi, adam, ema): true = skip.  latch:
// this is the one thread of the launch that writes flags[3].
__device__ __forceinline__ bool opt_skip(float* flags, bool latch) {
  if (flags == nullptr) return false;
  if (flags[0] != 0.f) {
    if (latch) flags[3] = 1.f;
    return true;
  }
  return flags[2] != 0.f;
}
// One element of the step past the first, for the stand-alone and the fused kernel alike (as adam1 below is for Adam).
// WD: torch.optim.SGD's coupled weight decay, g += wd * p ahead of the momentum.  Explicit multiply / fma in this
// order: the same rounding steps in every caller whatever the compiler would contract.
template <bool WD>
__device__ __forceinline__ void sgd1(float& p, float& b, float g, float lr, float momentum, float gscale, float wd) {
  g = __fmul_rn(g, gscale);
  if constexpr (WD) g = fmaf(wd, p, g);
  b = fmaf(momentum, b, g);
  p = fmaf(-lr, b, p);
}
__global__ void __launch_bounds__(256) sgd_momentum_kernel(float4* __restrict__ p, float4* __restrict__ buf,
                                                           const float4* __restrict__ g, size_t n4, float lr,
                                                           float momentum, float gscale, int first,
                                                           float* __restrict__ flags, const float* __restrict__ lr_dev,
                                                           const float* __restrict__ gmul) {
  if (opt_skip(flags, blockIdx.x == 0 && threadIdx.x == 0)) return;
  if (lr_dev != nullptr) lr = lr_dev[0];
  // gmul (optional): a device-side gradient multiplier (the clip coefficient of grad_norm_final_kernel), folded into
  // gscale by ONE fp32 product per thread, so the step equals passing float(gscale) * float(gmul[0]) from the host
  if (gmul != nullptr) gscale = __fmul_rn(gscale, gmul[0]);
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 gv = g[i];
    float4 pv = p[i], b;
    if (first) {
      b = make_float4(__fmul_rn(gv.x, gscale), __fmul_rn(gv.y, gscale), __fmul_rn(gv.z, gscale),
                      __fmul_rn(gv.w, gscale));
      pv.x = fmaf(-lr, b.x, pv.x); pv.y = fmaf(-lr, b.y, pv.y); pv.z = fmaf(-lr, b.z, pv.z); pv.w = fmaf(-lr, b.w, pv.w);
    } else {
      b = buf[i];
      sgd1<false>(pv.x, b.x, gv.x, lr, momentum, gscale, 0.f); sgd1<false>(pv.y, b.y, gv.y, lr, momentum, gscale, 0.f);
      sgd1<false>(pv.z, b.z, gv.z, lr, momentum, gscale, 0.f); sgd1<false>(pv.w, b.w, gv.w, lr, momentum, gscale, 0.f);
    }
    buf[i] = b;
    p[i] = pv;
  }
}

// ---------------------------------------------------------------- loss scaling
// Dynamic loss scaling for the fp16 step, entirely device-side (graph-safe):
// grad_nonfinite ORs "some gradient is inf/NaN" into *flag (the step's
// flags[2], which the fused SGD skips on); scale_update then backs the scale
// off on overflow or grows it after `interval` clean steps.
// scaler = {S, 1/S, clean steps, 0}.
__global__ void __launch_bounds__(256) grad_nonfinite_kernel(const float4* __restrict__ g, size_t n4,
                                                             float* __restrict__ flag) {
  bool bad = false;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = g[i];
    bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int*>(flag), 0x3f800000);   // 1.0f
}

// ---------------------------------------------------------------- split-bf16 (fp32 path)
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi): the fp32 path (ops/fp32.py) computes every conv GEMM as
// hi*hi + hi*lo + lo*hi on the bf16 MFMA kernels with fp32 accumulation.  src fp32 [M][C]; three blocks,
// block b = lo if bit b of `pattern` is set, else hi:
//   mode 0 (K-concatenated operand): dst [M][stride], block b at channels [b*C, (b+1)*C), zero from 3*C on;
//   mode 1 (M-stacked operand):      dst [3][M][stride], block b = rows [b*M, (b+1)*M), zero from C on.
// General form (small or padded C, e.g. the 3-channel image into 64-channel rows): one thread per output row
// chunk of 8 values (one 16-byte store; stride % 8 == 0).
__global__ void __launch_bounds__(256) split_x3_kernel(const float* __restrict__ src, uint4* __restrict__ dst,
                                                       int M, int C, int stride, int mode, int pattern) {
  const int rows = (mode == 0 ? 1 : 3) * M, s8 = stride >> 3;
  const long long total = (long long)rows * s8;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int row = (int)(t / s8), col0 = (int)(t - (long long)row * s8) * 8;
    const int b0 = (mode == 0) ? 0 : row / M;
    const int m = (mode == 0) ? row : row - b0 * M;
    unsigned short v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int col = col0 + k;
      const int b = (mode == 0) ? col / C : b0;
      const int c = (mode == 0) ? col - b * C : col;
      unsigned short o = 0;
      if (b < 3 && c < C) {
        const float x = src[(size_t)m * C + c];
        const unsigned short hi = f2bf(x);
        o = ((pattern >> b) & 1) ? f2bf(x - bf2f(hi)) : hi;
      }
      v[k] = o;
    }
    dst[t] = make_uint4(v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16), v[4] | ((unsigned)v[5] << 16),
                        v[6] | ((unsigned)v[7] << 16));
  }
}

// Fast path (C % 4 == 0, no padding columns): one thread per 4 source values; one float4 read, three 8-byte
// stores, 32-bit index math (the generic kernel's 64-bit divisions made it 30 % of the fp32 step).
__global__ void __launch_bounds__(256) split_x3_vec_kernel(const float4* __restrict__ src, uint2* __restrict__ dst,
                                                           int M, int C4, int mode, int pattern) {
  const int total = M * C4;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
    const float4 x = src[t];
    const float xv[4] = {x.x, x.y, x.z, x.w};
    unsigned short hi[4], lo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hi[k] = f2bf(xv[k]);
      lo[k] = f2bf(xv[k] - bf2f(hi[k]));
    }
    const uint2 h = make_uint2(hi[0] | ((unsigned)hi[1] << 16), hi[2] | ((unsigned)hi[3] << 16));
    const uint2 l = make_uint2(lo[0] | ((unsigned)lo[1] << 16), lo[2] | ((unsigned)lo[3] << 16));
    const int m = t / C4, c4 = t - m * C4;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const uint2 v = ((pattern >> b) & 1) ? l : h;
      if (mode == 0) dst[(size_t)m * 3 * C4 + b * C4 + c4] = v;      // [M][3C]
      else dst[(size_t)b * total + t] = v;                           // [3][M][C]
    }
  }
}

__global__ void scale_update_kernel(const float* __restrict__ flag, float* __restrict__ scaler, int interval,
                                    float growth, float backoff, float max_scale) {
  if (threadIdx.x != 0) return;
  float S = scaler[0], n = scaler[2];
  if (flag[0] != 0.f) {
    S = fmaxf(S * backoff, 1.f);
    n = 0.f;
  } else if (n + 1.f >= (float)interval) {
    S = fminf(S * growth, max_scale);
    n = 0.f;
  } else {
    n += 1.f;
  }
  scaler[0] = S;
  scaler[1] = 1.f / S;
  scaler[2] = n;
}

// ---------------------------------------------------------------- packing
// All layers' packs in one launch: blockIdx.y = descriptor row, rows of kPackRow int64
//   {w, fwd, dgr, Co, Ci, taps, first, mode, fwd2, dgr2, si, n}
// mode 0: a conv weight [Co][Ci][taps] -> fwd [Co][tap][Ci] and dgr [Ci][taps-1-tap][Co] (first: fwd [Co][64],
// k = tap*4 + c); when fwd2 != 0 the same (1x1 conv{S}_2) weight also goes into the interleaved context packs at
// scale si (see below).  mode -1 (optimizer launches only): a parameter without a pack (bias, head, conv{S}_1), n elements.
// blockIdx.x = a 32(co) x 32(ci) x taps tile transposed through LDS, so the fp32 reads (ci, tap contiguous per co),
// the fwd-pack writes (ci contiguous per co, tap) and the dgrad-pack writes (co contiguous per ci, tap) are all
// coalesced; mode -1: a 4096-element chunk.
//
// OPT != OPT_NONE: the optimizer step fused in front of the packing (one launch per step instead of sgd_momentum +
// pack_multi: the packs no longer re-read the 83 MB of fp32 masters).  Every arena parameter is exactly one row;
// grad / momentum live at the same offsets of their own arenas (goff / boff floats from w).  Per element the same
// fp32 operations as sgd_momentum_kernel (torch.optim.SGD semantics), so the result is bit for bit that of the
// two-launch step; a skipped step (non-finite loss or gradient) leaves weights, momentum AND packs untouched.
constexpr int kPackRow = 12;
// OPT: which optimizer runs in front of the packing.  OPT_SGD is the step above (weight decay 0); OPT_SGD_WD adds
// torch.optim.SGD's coupled weight decay (g += wd * p ahead of the momentum); OPT_ADAM is torch.optim.Adam / AdamW
// (adam1 below), its second moment in a third arena voff floats from the masters.
// OPT_SWAP is no optimizer: it exchanges every master with its EMA copy (eoff floats away) and packs what lands in the
// master slot (evaluation under the averaged weights, see ema below).
enum { OPT_NONE = 0, OPT_SGD = 1, OPT_SGD_WD = 2, OPT_ADAM = 3, OPT_SWAP = 4 };
struct OptArgs {
  long long goff, boff, voff;  // gradient / momentum (Adam: first moment) / second-moment arena offsets, in floats
  float lr, momentum, gscale;
  float wd, eps;
  int decoupled;               // Adam: 1 = AdamW (p *= 1 - lr*wd), 0 = coupled (g += wd*p)
  double beta1, beta2;         // double: 1 - float(0.999)^t is 3e-5 off 1 - 0.999^t at t = 1
  float* flags;
  const float* lr_dev;
  const int* t;                // Adam: applied steps so far, on the device (advanced by opt_tick_kernel); null:
  int step;                    //   this call's 1-based step from the host instead
  const float* gmul;           // device gradient multiplier (clip coefficient): gscale *= gmul[0], once per thread; null: none
  long long eoff;              // EMA arena's offset from the masters, in floats (EMA instantiations and OPT_SWAP)
  double ema_decay;            // double: 1 - float(0.9999) is 3e-4 off 1 - 0.9999 relatively
  int ema_warmup;              // 1: d_n = min(decay, (1 + n) / (10 + n))
  const int* ema_t;            // EMA updates applied so far, on the device (advanced by opt_tick_kernel); null (stand-alone
};                             //   kernel only): step - 1

// ---- Adam (torch.optim.Adam / AdamW, no amsgrad, no maximize), fp32 per element:
//   g' = gscale*g (+ wd*p coupled);  p *= 1 - lr*wd (decoupled);  m += (1-b1)(g' - m);  v = b2*v + (1-b2) g'^2;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc = 1 - beta^t, t the 1-based step.
// The per-launch scalars are computed once per thread in double (beta^t by repeated squaring: <= 2*32 multiplies,
// relative error ~1e-15, so bc1 / bc2 are the float64 values to rounding for any t), as torch computes them on the
// host.  One function for the fused and the stand-alone kernel: both run the same rounding steps.
struct AdamCoef { float gscale, cwd, decay, w1, w2, b2, step_size, bc2s, eps; };
__device__ __forceinline__ double powi(double b, unsigned n) {
  double r = 1.0;
  for (; n != 0u; n >>= 1, b *= b)
    if (n & 1u) r *= b;
  return r;
}
__device__ __forceinline__ AdamCoef adam_coef(const OptArgs& a, float lr) {
  const int t = (a.t != nullptr) ? a.t[0] + 1 : a.step;
  const double bc1 = 1.0 - powi(a.beta1, (unsigned)t), bc2 = 1.0 - powi(a.beta2, (unsigned)t);
  AdamCoef c;
  c.gscale = (a.gmul != nullptr) ? __fmul_rn(a.gscale, a.gmul[0]) : a.gscale;
  c.cwd = a.decoupled ? 0.f : a.wd;
  c.decay = a.decoupled ? (float)(1.0 - (double)lr * (double)a.wd) : 1.f;
  c.w1 = (float)(1.0 - a.beta1);
  c.w2 = (float)(1.0 - a.beta2);
  c.b2 = (float)a.beta2;
  c.step_size = (float)((double)lr / bc1);
  c.bc2s = (float)sqrt(bc2);
  c.eps = a.eps;
  return c;
}
// (wd = 0: fmaf(0, p, g) = g and p * 1 = p exactly, so one branch-free form serves all three variants; IEEE divide and
// sqrt: the kernels are bandwidth-bound)
__device__ __forceinline__ void adam1(const AdamCoef& c, float& p, float& m, float& v, float g) {
#pragma clang fp contract(off)
  g = g * c.gscale;
  g = fmaf(c.cwd, p, g);
  p = p * c.decay;
  m = fmaf(c.w1, g - m, m);
  v = fmaf(c.w2 * g, g, c.b2 * v);
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  p = fmaf(-c.step_size, m / denom, p);
}

// ---- EMA of the parameters: e += w * (p - e), w = float(1 - d_n), d_n = min(decay, (1 + n) / (10 + n)) with warm-up,
// decay without; n = updates applied so far.  d_n and 1 - d_n are formed in double once per thread (as adam_coef), the
// update is one fp32 subtraction and one fma.  One pair of functions for the fused and the stand-alone kernel.
__device__ __forceinline__ float ema_coef(const OptArgs& a) {
  const int n = (a.ema_t != nullptr) ? a.ema_t[0] : a.step - 1;
  double d = a.ema_decay;
  if (a.ema_warmup) d = fmin(d, (1.0 + (double)n) / (10.0 + (double)n));
  return (float)(1.0 - d);
}
__device__ __forceinline__ float ema1(float w, float p, float e) {
#pragma clang fp contract(off)
  const float diff = p - e;
  return fmaf(w, diff, e);
}
__device__ __forceinline__ float4 ema4(float w, float4 p, float4 e) {
  return make_float4(ema1(w, p.x, e.x), ema1(w, p.y, e.y), ema1(w, p.z, e.z), ema1(w, p.w, e.w));
}

// Every optimizer's packs are the 16-bit rounding of the fp32 master as stored, on every store path: resume,
// swap_weights and refresh_packs re-pack from the stored masters and must reproduce them.  Without the barrier the
// compiler folds the update's last fma into the conversion (v_fma_mixlo_f16: the exact fma result rounded once, to
// fp16), which differs from a re-pack of the stored master in rare double-rounding cases (the master lands on an fp16
// midpoint after an update below half an fp32 ulp; 5.5e-5 of N(0, 0.3) weights per SGD step at lr = 3e-3).
// tests/test_gpu_optpack_exact.py pins it with directed cases.  (OPT_NONE packs a loaded value: nothing to fold.)
template <int OPT>
__device__ __forceinline__ float as_stored(float x) {
  if constexpr (OPT != OPT_NONE) asm volatile("" : "+v"(x));
  return x;
}

// EMA (optimizer instantiations only): every path that stores an updated master also updates its EMA copy at
// pw[eoff] from the master as stored -- one more fp32 read and write per element, no re-read of the masters.
template <int DT, int OPT, bool EMA = false>
__global__ void __launch_bounds__(256) pack_multi_kernel(const long long* __restrict__ desc, OptArgs sa) {
  static_assert(!EMA || (OPT >= OPT_SGD && OPT <= OPT_ADAM), "EMA rides on an optimizer step");
  __shared__ unsigned short t[32][32 * 9 + 2];       // [co][ci*taps + tap] bf16 bits
  const long long* d = desc + (size_t)blockIdx.y * kPackRow;
  float* w = reinterpret_cast<float*>(d[0]);
  bf16_t* fwd = reinterpret_cast<bf16_t*>(d[1]);
  bf16_t* dgr = reinterpret_cast<bf16_t*>(d[2]);
  const int Co = (int)d[3], Ci = (int)d[4], taps = (int)d[5], first = (int)d[6];
  const int mode = (int)d[7];
  float lr = sa.lr;
  if constexpr (OPT != OPT_NONE && OPT != OPT_SWAP) {
    if (opt_skip(sa.flags, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)) return;
    if (sa.lr_dev != nullptr) lr = sa.lr_dev[0];
    if constexpr (OPT != OPT_ADAM) {              // (Adam: adam_coef folds gmul in)
      if (sa.gmul != nullptr) sa.gscale = __fmul_rn(sa.gscale, sa.gmul[0]);
    }
  }
  AdamCoef ac{};                // Adam: filled in below, past the exits of the blocks that have no work
  float ew = 0.f;               // EMA: likewise
  auto sgd = [&](float& p, float& b, float g) {
    sgd1<OPT == OPT_SGD_WD>(p, b, g, lr, sa.momentum, sa.gscale, sa.wd);
  };
  // one element of the optimizer step (sgd1 / adam1: the stand-alone kernels' operations, in their order)
  auto step1 = [&](float* pw, float pv, float gv, float bv) -> float {
    float ev = 0.f;
    if constexpr (EMA) ev = pw[sa.eoff];
    if constexpr (OPT == OPT_ADAM) {
      float vv = pw[sa.voff];
      adam1(ac, pv, bv, vv, gv);
      pw[sa.boff] = bv;
      pw[sa.voff] = vv;
    } else {
      sgd(pv, bv, gv);
      pw[sa.boff] = bv;
    }
    pw[0] = pv;
    if constexpr (EMA) pw[sa.eoff] = ema1(ew, as_stored<OPT>(pv), ev);
    return pv;
  };
  // one element of the swap: the EMA copy lands in the master slot (and is what the packs are made from)
  auto swap1 = [&](float* pw) -> float {
    const float pv = pw[0], ev = pw[sa.eoff];
    pw[sa.eoff] = pv;
    pw[0] = ev;
    return ev;
  };
  if (mode < 0) {
    if constexpr (OPT != OPT_NONE) {
      const long long n = d[11];
      if constexpr (OPT == OPT_ADAM || EMA) {
        if ((long long)blockIdx.x * 4096 >= n) return;
        if constexpr (OPT == OPT_ADAM) ac = adam_coef(sa, lr);
        if constexpr (EMA) ew = ema_coef(sa);
      }
      const long long e1 = min(n, (long long)(blockIdx.x + 1) * 4096);
      for (long long i = (long long)blockIdx.x * 4096 + threadIdx.x; i < e1; i += 256) {
        if constexpr (OPT == OPT_SWAP) swap1(w + i);
        else step1(w + i, w[i], w[i + sa.goff], w[i + sa.boff]);
      }
    }
    return;
  }
  const int nci = (Ci + 31) / 32, nco = (Co + 31) / 32;
  if ((int)blockIdx.x >= nci * nco) return;
  if constexpr (OPT == OPT_ADAM) ac = adam_coef(sa, lr);
  if constexpr (EMA) ew = ema_coef(sa);
  const int co0 = (blockIdx.x / nci) * 32, ci0 = (blockIdx.x % nci) * 32;
  const int cis = min(32, Ci - ci0), cos_ = min(32, Co - co0);
  const int row = cis * taps;                          // contiguous floats per co in the tile
  // whole 32 x 32 tiles of 8-aligned channel counts (every non-first layer): 16-B loads and stores, 8 channels
  // per thread (the 2-byte-store form took 81 us per step for the 41 M weights); ragged tiles: element-wise
  // (v4n: the guard of the step without EMA)
  const bool v4n = !first && cis == 32 && cos_ == 32 && Ci % 8 == 0 && Co % 8 == 0 && (row & 3) == 0 &&
                   ((((size_t)co0 * Ci + ci0) * taps) & 3) == 0 && (((size_t)Ci * taps) & 3) == 0 &&
                   ((uintptr_t)w & 15) == 0 &&
                   (OPT == OPT_NONE || ((sa.goff | sa.boff | sa.voff) & 3) == 0);   // every arena 16-B aligned
  const bool v4 = v4n && (!(EMA || OPT == OPT_SWAP) || (sa.eoff & 3) == 0);
  if (v4 && OPT == OPT_ADAM) {
    // Adam: the next iteration's four loads are issued ahead of this one's arithmetic and stores.  The iterations
    // touch distinct addresses, which the compiler cannot prove (the stores through pw + boff / voff may alias the
    // loads), so without this each iteration is load - wait - long ALU chain - store with nothing in flight meanwhile.
    const int r4 = row >> 2, total = 32 * r4;
    auto at = [&](int i, int& c, int& r) -> float* {
      c = i / r4;
      r = (i - c * r4) * 4;
      return w + ((size_t)(co0 + c) * Ci + ci0) * taps + r;
    };
    int i = threadIdx.x, c = 0, r = 0;
    float* pw = w;
    float4 v{}, gv{}, m{}, s{}, e{};
    if (i < total) {
      pw = at(i, c, r);
      v = *reinterpret_cast<const float4*>(pw);
      gv = *reinterpret_cast<const float4*>(pw + sa.goff);
      m = *reinterpret_cast<const float4*>(pw + sa.boff);
      s = *reinterpret_cast<const float4*>(pw + sa.voff);
      if constexpr (EMA) e = *reinterpret_cast<const float4*>(pw + sa.eoff);
    }
    while (i < total) {
      const int in = i + 256;
      int cn = 0, rn = 0;
      float* pwn = pw;
      float4 vn{}, gvn{}, mn{}, sn{}, en{};
      if (in < total) {
        pwn = at(in, cn, rn);
        vn = *reinterpret_cast<const float4*>(pwn);
        gvn = *reinterpret_cast<const float4*>(pwn + sa.goff);
        mn = *reinterpret_cast<const float4*>(pwn + sa.boff);
        sn = *reinterpret_cast<const float4*>(pwn + sa.voff);
        if constexpr (EMA) en = *reinterpret_cast<const float4*>(pwn + sa.eoff);
      }
      adam1(ac, v.x, m.x, s.x, gv.x); adam1(ac, v.y, m.y, s.y, gv.y);
      adam1(ac, v.z, m.z, s.z, gv.z); adam1(ac, v.w, m.w, s.w, gv.w);
      *reinterpret_cast<float4*>(pw + sa.boff) = m;
      *reinterpret_cast<float4*>(pw + sa.voff) = s;
      *reinterpret_cast<float4*>(pw) = v;
      v.x = as_stored<OPT>(v.x); v.y = as_stored<OPT>(v.y); v.z = as_stored<OPT>(v.z); v.w = as_stored<OPT>(v.w);
      if constexpr (EMA) *reinterpret_cast<float4*>(pw + sa.eoff) = ema4(ew, v, e);
      t[c][r] = f2h<DT>(v.x); t[c][r + 1] = f2h<DT>(v.y); t[c][r + 2] = f2h<DT>(v.z); t[c][r + 3] = f2h<DT>(v.w);
      i = in; pw = pwn; c = cn; r = rn; v = vn; gv = gvn; m = mn; s = sn;
      if constexpr (EMA) e = en;
    }
  } else if (v4) {
    const int r4 = row >> 2;
    for (int i = threadIdx.x; i < 32 * r4; i += 256) {
      const int c = i / r4, r = (i - c * r4) * 4;
      float* pw = w + ((size_t)(co0 + c) * Ci + ci0) * taps + r;
      float4 v = *reinterpret_cast<const float4*>(pw);
      if constexpr (OPT == OPT_SWAP) {
        const float4 e = *reinterpret_cast<const float4*>(pw + sa.eoff);
        *reinterpret_cast<float4*>(pw + sa.eoff) = v;
        *reinterpret_cast<float4*>(pw) = e;
        v = e;
      } else if constexpr (OPT != OPT_NONE && OPT != OPT_ADAM) {
        float4 gv = *reinterpret_cast<const float4*>(pw + sa.goff);
        float4 b = *reinterpret_cast<const float4*>(pw + sa.boff);
        float4 e{};
        if constexpr (EMA) e = *reinterpret_cast<const float4*>(pw + sa.eoff);
        sgd(v.x, b.x, gv.x); sgd(v.y, b.y, gv.y); sgd(v.z, b.z, gv.z); sgd(v.w, b.w, gv.w);
        *reinterpret_cast<float4*>(pw + sa.boff) = b;
        *reinterpret_cast<float4*>(pw) = v;
        if constexpr (EMA)
          *reinterpret_cast<float4*>(pw + sa.eoff) =
              ema4(ew, make_float4(as_stored<OPT>(v.x), as_stored<OPT>(v.y), as_stored<OPT>(v.z), as_stored<OPT>(v.w)), e);
      }
      v.x = as_stored<OPT>(v.x); v.y = as_stored<OPT>(v.y); v.z = as_stored<OPT>(v.z); v.w = as_stored<OPT>(v.w);
      t[c][r] = f2h<DT>(v.x); t[c][r + 1] = f2h<DT>(v.y); t[c][r + 2] = f2h<DT>(v.z); t[c][r + 3] = f2h<DT>(v.w);
    }
  } else {
    // ragged tiles, and whole tiles of a misaligned slot or arena: element-wise, packed from the master as stored like
    // every other path (as_stored), so the packs depend neither on the tile shape nor on where an arena lies
    for (int i = threadIdx.x; i < cos_ * row; i += 256) {
      const int c = i / row, r = i - c * row;
      float* pw = w + ((size_t)(co0 + c) * Ci + ci0) * taps + r;
      float v = pw[0];
      if constexpr (OPT == OPT_SWAP) v = swap1(pw);
      else if constexpr (OPT != OPT_NONE) v = step1(pw, v, pw[sa.goff], pw[sa.boff]);
      t[c][r] = f2h<DT>(as_stored<OPT>(v));
    }
  }
  __syncthreads();
  if (first) {
    for (int i = threadIdx.x; i < cos_ * row; i += 256) {
      const int c = i / row, r = i - c * row, ci = r / taps, tap = r - ci * taps;
      fwd[(size_t)(co0 + c) * 64 + tap * 4 + ci0 + ci] = t[c][r];
    }
    return;
  }
  if (d[8] != 0) {
    // linearised context module (conv_igemm.hip): W2cat[4co + si][ci] = W2_S[co][ci] (fwd2, rows interleaved over
    // the four scales) and its transpose W2cat^T[ci][4co + si] (dgr2); 1x1 only, si = d[10]
    bf16_t* fwd2 = reinterpret_cast<bf16_t*>(d[8]);
    bf16_t* dgr2 = reinterpret_cast<bf16_t*>(d[9]);
    const int si = (int)d[10];
    for (int i = threadIdx.x; i < cos_ * cis; i += 256) {
      const int ci = i % cis, c = i / cis;
      fwd2[((size_t)4 * (co0 + c) + si) * Ci + ci0 + ci] = t[c][ci];
    }
    for (int i = threadIdx.x; i < cis * cos_; i += 256) {
      const int c = i % cos_, ci = i / cos_;
      dgr2[(size_t)(ci0 + ci) * 4 * Co + 4 * (co0 + c) + si] = t[c][ci];
    }
  }
  if (cis == 32 && cos_ == 32 && Ci % 8 == 0 && Co % 8 == 0 && ((uintptr_t)fwd & 15) == 0 &&
      ((uintptr_t)dgr & 15) == 0) {
    // fwd[co][tap][ci]: 8 consecutive ci per 16-B store
    for (int i = threadIdx.x; i < 32 * taps * 4; i += 256) {
      const int g = i & 3, rest = i >> 2, tap = rest % taps, c = rest / taps;
      unsigned short e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = t[c][(g * 8 + j) * taps + tap];
      *reinterpret_cast<uint4*>(fwd + ((size_t)(co0 + c) * taps + tap) * Ci + ci0 + g * 8) =
          make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
                     e[6] | ((unsigned)e[7] << 16));
    }
    if (dgr) {
      // dgr[ci][taps-1-tap][co]: 8 consecutive co per 16-B store
      for (int i = threadIdx.x; i < 32 * taps * 4; i += 256) {
        const int g = i & 3, rest = i >> 2, tap = rest % taps, ci = rest / taps;
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = t[g * 8 + j][ci * taps + tap];
        *reinterpret_cast<uint4*>(dgr + ((size_t)(ci0 + ci) * taps + (taps - 1 - tap)) * Co + co0 + g * 8) =
            make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
                       e[6] | ((unsigned)e[7] << 16));
      }
    }
    return;
  }
  // fwd[co][tap][ci]: ci fastest
  for (int i = threadIdx.x; i < cos_ * taps * cis; i += 256) {
    const int ci = i % cis, rest = i / cis, tap = rest % taps, c = rest / taps;
    fwd[((size_t)(co0 + c) * taps + tap) * Ci + ci0 + ci] = t[c][ci * taps + tap];
  }
  if (dgr) {
    // dgr[ci][taps-1-tap][co]: co fastest
    for (int i = threadIdx.x; i < cis * taps * cos_; i += 256) {
      const int c = i % cos_, rest = i / cos_, tap = rest % taps, ci = rest / taps;
      dgr[((size_t)(ci0 + ci) * taps + (taps - 1 - tap)) * Co + co0 + c] = t[c][ci * taps + tap];
    }
  }
}

// [N,3,H,W] fp32 -> [N,H,W,4] bf16 (4th channel zero)
template <int DT>
__global__ void __launch_bounds__(256) img_to_nhwc4_kernel(const float* __restrict__ img, uint2* __restrict__ out,
                                                           int N, int H, int W) {
  const size_t HW = (size_t)H * W;
  const size_t total = (size_t)N * HW;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t n = i / HW, p = i % HW;
    const float* b = img + n * 3 * HW + p;
    out[i] = make_uint2(pack2<DT>(b[0], b[HW]), pack2<DT>(b[2 * HW], 0.f));
  }
}

// ---------------------------------------------------------------- Adam (stand-alone) + step count
// The Adam step over flat buffers, per element exactly the fused kernel's adam1 (so "fused == adam + pack_multi" holds
// bit for bit); flags / lr_dev as sgd_momentum_kernel.  vec: every pointer 16-B aligned -> float4 groups, the n % 4
// tail (or, unaligned, everything) element-wise.
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ g, size_t n, int vec, OptArgs a) {
  if (opt_skip(a.flags, blockIdx.x == 0 && threadIdx.x == 0)) return;
  const AdamCoef c = adam_coef(a, (a.lr_dev != nullptr) ? a.lr_dev[0] : a.lr);
  const size_t n4 = vec ? n / 4 : 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i],
           vv = reinterpret_cast<float4*>(v)[i];
    adam1(c, pv.x, mv.x, vv.x, gv.x); adam1(c, pv.y, mv.y, vv.y, gv.y);
    adam1(c, pv.z, mv.z, vv.z, gv.z); adam1(c, pv.w, mv.w, vv.w, gv.w);
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  for (size_t i = 4 * n4 + blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float pv = p[i], mv = m[i], vv = v[i];
    adam1(c, pv, mv, vv, g[i]);
    m[i] = mv; v[i] = vv; p[i] = pv;
  }
}

// The device step count t advances by one per APPLIED Adam step: a one-thread launch right after the step kernel,
// which skips on the same flags.  Every block of the step kernel read t before this launch starts (stream order), so
// all of them saw the same value; a captured step replays both nodes and its bias correction advances.
// t2 (optional): a second count advanced under the same flags -- the EMA's update count beside Adam's step count.
__global__ void opt_tick_kernel(const float* __restrict__ flags, int* __restrict__ t, int* __restrict__ t2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (flags != nullptr && (flags[0] != 0.f || flags[2] != 0.f)) return;
  if (t != nullptr) t[0] += 1;
  if (t2 != nullptr) t2[0] += 1;
}

// ---------------------------------------------------------------- EMA (stand-alone)
// e += w * (p - e) over flat buffers, per element exactly the fused kernel's ema_coef / ema1 (so "fused == optimizer
// without EMA, then ema" holds bit for bit); flags as adam_kernel.  vec: both pointers 16-B aligned -> float4 groups,
// the n % 4 tail (or, unaligned, everything) element-wise.
__global__ void __launch_bounds__(256) ema_kernel(float* __restrict__ e, const float* __restrict__ p, size_t n, int vec,
                                                  OptArgs a) {
  if (opt_skip(a.flags, blockIdx.x == 0 && threadIdx.x == 0)) return;
  const float w = ema_coef(a);
  const size_t n4 = vec ? n / 4 : 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
    reinterpret_cast<float4*>(e)[i] = ema4(w, reinterpret_cast<const float4*>(p)[i], reinterpret_cast<float4*>(e)[i]);
  for (size_t i = 4 * n4 + blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    e[i] = ema1(w, p[i], e[i]);
}

// ---------------------------------------------------------------- gradient norm (global-norm clipping)
// Segmented sum of squares over the fp32 gradient arena in two launches, no atomics, fixed order (bitwise repeatable).
// tab: {arena offset, element count} per parameter, in arena order (int64 pairs).
// Stage 1, grid (chunk, parameter): block (c, p) sums the squares of elements [c*kNormChunk, (c+1)*kNormChunk) of
// parameter p in double from the first add (the kernel reads the arena once and is bandwidth-bound) -- 16-byte loads
// where the parameter starts 16-byte aligned (chunks keep the alignment), element-wise otherwise -- then reduces over
// the wave by shuffles and over the four waves through LDS in wave order, and writes part[p * max_chunks + c].
constexpr int kNormChunk = 4096;
__global__ void __launch_bounds__(256) grad_norm_partial_kernel(const float* __restrict__ g,
                                                                const long long* __restrict__ tab,
                                                                double* __restrict__ part, int max_chunks) {
  __shared__ double red[4];
  const int p = blockIdx.y;
  const long long off = tab[2 * p], n = tab[2 * p + 1];
  const long long s0 = (long long)blockIdx.x * kNormChunk;
  if (s0 >= n) return;
  const int cnt = (int)min((long long)kNormChunk, n - s0);
  const float* x = g + off + s0;
  double s = 0.0;
  if ((reinterpret_cast<uintptr_t>(g + off) & 15) == 0) {
    const int n4 = cnt >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      s = fma((double)v.x, (double)v.x, s); s = fma((double)v.y, (double)v.y, s);
      s = fma((double)v.z, (double)v.z, s); s = fma((double)v.w, (double)v.w, s);
    }
    for (int i = 4 * n4 + threadIdx.x; i < cnt; i += 256) s = fma((double)x[i], (double)x[i], s);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) s = fma((double)x[i], (double)x[i], s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)p * max_chunks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Stage 2, one block: thread p sums parameter p's partials in index order (its sum replaces the row's first partial),
// then thread 0 sums the parameters in arena order and writes the fp32 vector gn:
//   gn[0] = gscale * sqrt(total), the norm of the gradient the optimizer sees (gscale = 1 / world);
//   gn[1] = the clip coefficient min(1, max_norm / (gn[0] + 1e-6)) (torch.nn.utils.clip_grad_norm_'s rule, in fp32;
//           max_norm = inf: exactly 1);  gn[2 + p] = gscale * sqrt(parameter p's sum).
// A double sum of squares of finite fp32 values cannot overflow, so a non-finite total means a non-finite element:
// then gn[1] = 0 and flag[0] (the step's flags[2], which the optimizer kernels skip on) is set.
__global__ void __launch_bounds__(256) grad_norm_final_kernel(const long long* __restrict__ tab, int np,
                                                              double* __restrict__ part, int max_chunks,
                                                              float* __restrict__ gn, float gscale, float max_norm,
                                                              float* __restrict__ flag) {
  for (int p = threadIdx.x; p < np; p += 256) {
    const long long n = tab[2 * p + 1];
    const int nc = (int)min((long long)max_chunks, (n + kNormChunk - 1) / kNormChunk);
    double* row = part + (size_t)p * max_chunks;
    double s = 0.0;
    for (int c = 0; c < nc; ++c) s += row[c];
    row[0] = s;
    gn[2 + p] = (float)((double)gscale * sqrt(s));
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int p = 0; p < np; ++p) total += part[(size_t)p * max_chunks];
  if (!isfinite(total)) {
    gn[0] = (float)total;
    gn[1] = 0.f;
    if (flag != nullptr) flag[0] = 1.f;
    return;
  }
  const float norm = (float)((double)gscale * sqrt(total));
  gn[0] = norm;
  gn[1] = fminf(1.f, max_norm / (norm + 1e-6f));
}

// Gradient accumulation: folds the micro-batch loss the fused head just wrote to flags[1] into a device accumulator
// (one thread, like opt_tick_kernel).  fold: 1 = the window's first micro-step (set), 2 = a later one (add), 0 = none
// (a window closed by flush(), whose micro-steps are all folded already); close: the window's total goes back to
// flags[1] and its non-finite flag to flags[0], ahead of the loss all-reduce.
__global__ void accum_tick_kernel(float* __restrict__ flags, float* __restrict__ acc, int fold, int close) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float a = (fold == 1) ? flags[1] : (fold == 2) ? acc[0] + flags[1] : acc[0];
  acc[0] = a;
  if (close) {
    flags[1] = a;
    flags[0] = isfinite(a) ? 0.f : 1.f;
  }
}

// ---------------------------------------------------------------- count metrics (masked counts, GAME 0..3)
// Per sample of et / gt [h][w] fp32 and an optional weight plane m (null: 1): level-l cell (a, b) covers rows
// [(a h) >> l, ((a+1) h) >> l) and the columns likewise with w; every level's cells are unions of level-3 cells.
// Stage 1, grid (64 level-3 cells, sample): block (c, s) sums double(m) * double(et) and double(m) * double(gt) (exact
// products) over its cell, pixel k of the cell by thread k % 256, then reduces like grad_norm_partial_kernel: over the
// wave by shuffles, over the four waves through LDS in wave order.  No atomics, fixed order: bitwise repeatable.  An
// empty cell (a map smaller than 8) writes 0.  part: [n][64][2] doubles (E_cell, G_cell).
__global__ void __launch_bounds__(256) count_metrics_kernel(const float* __restrict__ et, const float* __restrict__ gt,
                                                            long long gt_stride, const float* __restrict__ m,
                                                            long long m_stride, int h, int w,
                                                            double* __restrict__ part) {
  __shared__ double red[2][4];
  const int a = blockIdx.x >> 3, b = blockIdx.x & 7;
  const int r0 = (a * h) >> 3, r1 = ((a + 1) * h) >> 3, c0 = (b * w) >> 3, c1 = ((b + 1) * w) >> 3;
  const int cw = c1 - c0, cnt = (r1 - r0) * cw;
  const size_t s = blockIdx.y;
  const float* e = et + s * (size_t)h * w;
  const float* g = gt + s * (size_t)gt_stride;
  const float* mm = (m != nullptr) ? m + s * (size_t)m_stride : nullptr;
  double se = 0.0, sg = 0.0;
  for (int k = threadIdx.x; k < cnt; k += 256) {
    const size_t i = (size_t)(r0 + k / cw) * w + (c0 + k % cw);
    const double wm = (mm != nullptr) ? (double)mm[i] : 1.0;
    se = fma(wm, (double)e[i], se);
    sg = fma(wm, (double)g[i], sg);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    se += __shfl_down(se, o, 64);
    sg += __shfl_down(sg, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = se; red[1][threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* r = red[threadIdx.x];
    part[(s * 64 + blockIdx.x) * 2 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// Stage 2, one block per sample: thread q < 85 owns cell q of the 1 + 4 + 16 + 64 cells of levels 0..3 and sums the
// level-3 cells it is the union of in index order (rows, then columns), E and G apart; thread l < 4 then sums level l's
// |E_cell - G_cell| in cell order.  out: [n][6] doubles = (E, G, GAME_0 .. GAME_3), E and G the level-0 sums.
__global__ void __launch_bounds__(128) count_metrics_final_kernel(const double* __restrict__ part,
                                                                  double* __restrict__ out) {
  __shared__ double diff[85];
  const double* p = part + (size_t)blockIdx.x * 128;
  double* o = out + (size_t)blockIdx.x * 6;
  const int q = threadIdx.x;
  if (q < 85) {
    const int l = (q >= 21) ? 3 : (q >= 5) ? 2 : (q >= 1) ? 1 : 0;
    const int c = q - ((l == 3) ? 21 : (l == 2) ? 5 : (l == 1) ? 1 : 0);
    const int side = 1 << l, span = 8 >> l;
    const int a = c / side, b = c % side;
    double se = 0.0, sg = 0.0;
    for (int i = a * span; i < (a + 1) * span; ++i)
      for (int j = b * span; j < (b + 1) * span; ++j) {
        se += p[(i * 8 + j) * 2];
        sg += p[(i * 8 + j) * 2 + 1];
      }
    diff[q] = fabs(se - sg);
    if (q == 0) { o[0] = se; o[1] = sg; }
  }
  __syncthreads();
  if (q < 4) {
    const int first = (q == 3) ? 21 : (q == 2) ? 5 : (q == 1) ? 1 : 0, cells = 1 << (2 * q);
    double sd = 0.0;
    for (int c = 0; c < cells; ++c) sd += diff[first + c];
    o[2 + q] = sd;
  }
}

static inline int grid_for(size_t n, int per = 256, int cap = 4096) {
  size_t g = (n + per - 1) / per;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace can

using namespace can;

extern "C" int can_maxpool_fwd(const void* x, void* y, void* codes, int N, int H, int W, int C, int dt,
                               void* stream) {
  if ((C & 7) || (H & 1) || (W & 1)) return -2;
  const size_t tot = (size_t)N * (H / 2) * (W / 2) * (C / 8);
  CAN_LAUNCH_DT(dt, maxpool_fwd_kernel, dim3(grid_for(tot, 256, 8192)), dim3(256), 0,
                (hipStream_t)stream, (const uint4*)x, (uint4*)y, (uint32_t*)codes, N, H, W, C / 8);
  return (int)hipGetLastError();
}

extern "C" int can_maxpool_bwd_codes(const void* codes, const void* dy, void* dx, int N, int H, int W, int C, int dt,
                                     void* stream) {
  if ((C & 7) || (H & 1) || (W & 1)) return -2;
  const size_t tot = (size_t)N * (H / 2) * (W / 2) * (C / 8);
  CAN_LAUNCH_DT(dt, maxpool_bwd_codes_kernel, dim3(grid_for(tot, 256, 8192)), dim3(256), 0,
                (hipStream_t)stream, (const uint32_t*)codes, (const uint4*)dy, (uint4*)dx, N, H, W, C / 8);
  return (int)hipGetLastError();
}

extern "C" int can_maxpool_bwd_relu(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int dt,
                                    void* stream) {
  if ((C & 7) || (H & 1) || (W & 1)) return -2;
  const size_t tot = (size_t)N * (H / 2) * (W / 2) * (C / 8);
  CAN_LAUNCH_DT(dt, maxpool_bwd_relu_kernel, dim3(grid_for(tot, 256, 8192)), dim3(256), 0,
                (hipStream_t)stream, (const uint4*)x, (const uint4*)dy, (uint4*)dx, N, H, W,
                C / 8);
  return (int)hipGetLastError();
}

// pitch / wv: row pitch and valid width of a width-padded map (pitch <= wv: no padding)
extern "C" int can_head_fwd(const void* y, const float* w, const float* b, float* et, int P, int dt, void* stream,
                            int pitch, int wv) {
  CAN_LAUNCH_DT(dt, head_fwd_kernel, dim3(grid_for((size_t)P * 8, 256, 2048)), dim3(256),
                0, (hipStream_t)stream, (const uint4*)y, w, b, et, P, pitch, wv);
  return (int)hipGetLastError();
}

extern "C" int can_head_train(const void* y, const float* w, const float* b, const float* gt, float* et, void* dy,
                              float* part, int nblk, float* dw, float* db, float* loss, int P, float gscale,
                              float beta, const float* lscale, float* nonfinite, int dt, void* stream, int pitch,
                              int wv, const float* wt) {
  hipStream_t s = (hipStream_t)stream;
  if (wt != nullptr && dt == DT_F16)
    hipLaunchKernelGGL((head_train_kernel<DT_F16, true>), dim3(nblk), dim3(256), 0, s, (const uint4*)y, w, b, gt, et,
                       (uint4*)dy, part, P, gscale, lscale, pitch, wv, wt);
  else if (wt != nullptr && dt == DT_BF16)
    hipLaunchKernelGGL((head_train_kernel<DT_BF16, true>), dim3(nblk), dim3(256), 0, s, (const uint4*)y, w, b, gt, et,
                       (uint4*)dy, part, P, gscale, lscale, pitch, wv, wt);
  else if (dt == DT_F16)
    hipLaunchKernelGGL(head_train_kernel<DT_F16>, dim3(nblk), dim3(256), 0, s, (const uint4*)y, w, b, gt, et,
                       (uint4*)dy, part, P, gscale, lscale, pitch, wv);
  else if (dt == DT_BF16)
    hipLaunchKernelGGL(head_train_kernel<DT_BF16>, dim3(nblk), dim3(256), 0, s, (const uint4*)y, w, b, gt, et,
                       (uint4*)dy, part, P, gscale, lscale, pitch, wv);
  else
    return -20;
  hipLaunchKernelGGL(head_reduce_kernel, dim3(1), dim3(1024), 0, s, part, nblk, dw, db, loss, beta, nonfinite);
  return (int)hipGetLastError();
}

extern "C" int can_sgd_momentum(float* p, float* buf, const float* g, size_t n, float lr, float momentum,
                                float gscale, int first, float* flags, const float* lr_dev, void* stream,
                                const float* gmul) {
  if (n & 3) return -2;
  hipLaunchKernelGGL(sgd_momentum_kernel, dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                     (float4*)p, (float4*)buf, (const float4*)g, n / 4, lr, momentum, gscale, first, flags, lr_dev,
                     gmul);
  return (int)hipGetLastError();
}

__global__ void __launch_bounds__(256) scale_inplace_kernel(float* __restrict__ x, size_t n, float s) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] *= s;
}

extern "C" int can_scale_inplace(float* x, size_t n, float s, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scale_inplace_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, n, s);
  return (int)hipGetLastError();
}

extern "C" int can_grad_nonfinite(const float* g, size_t n, float* flag, void* stream) {
  if (n & 3) return -2;
  hipLaunchKernelGGL(grad_nonfinite_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)g, n / 4, flag);
  return (int)hipGetLastError();
}

extern "C" int can_split_x3(const float* src, void* dst, long long M, int C, int stride, int mode, int pattern,
                            void* stream) {
  if (M < 1 || C < 1 || (mode == 0 && stride < 3 * C) || (mode == 1 && stride < C) || mode < 0 || mode > 1) return -2;
  const size_t total = (size_t)(mode == 0 ? 1 : 3) * (size_t)M * (size_t)stride;
  const bool dense = (mode == 0) ? stride == 3 * C : stride == C;
  if (dense && C % 4 == 0 && (size_t)M * C < (1u << 31) && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0) {
    const size_t n4 = (size_t)M * (C / 4);
    hipLaunchKernelGGL(split_x3_vec_kernel, dim3(grid_for(n4, 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)src, (uint2*)dst, (int)M, C / 4, mode, pattern);
    return (int)hipGetLastError();
  }
  if (stride % 8 || (size_t)M * 3 >= (1u << 31) || ((uintptr_t)dst & 15)) return -3;
  hipLaunchKernelGGL(split_x3_kernel, dim3(grid_for(total / 8, 256, 16384)), dim3(256), 0, (hipStream_t)stream, src,
                     (uint4*)dst, (int)M, C, stride, mode, pattern);
  return (int)hipGetLastError();
}

extern "C" int can_scale_update(const float* flag, float* scaler, int interval, float growth, float backoff,
                                float max_scale, void* stream) {
  hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flag, scaler, interval, growth,
                     backoff, max_scale);
  return (int)hipGetLastError();
}

extern "C" int can_img_to_nhwc4(const float* img, void* out, int N, int H, int W, int dt, void* stream) {
  CAN_LAUNCH_DT(dt, img_to_nhwc4_kernel, dim3(grid_for((size_t)N * H * W, 256, 8192)),
                dim3(256), 0, (hipStream_t)stream, img, (uint2*)out, N, H, W);
  return (int)hipGetLastError();
}

// The one place that maps (dt, OPT, EMA) to an instantiation of pack_multi_kernel (all 16 of them).  grid.x covers the
// largest row's 32x32 tiles (B1: 512 -> 1024 channels = 512 tiles) or 4096-element chunks.  -20: not a 16-bit dt.
// t1 / t2 (optimizer steps): the device counts that advance in one one-thread launch right after the step, under the
// step's flags (nothing comes between the two launches on the host).
static int pack_multi_launch(const long long* desc, int rows, int max_tiles, int dt, int opt, bool ema,
                             const OptArgs& sa, hipStream_t s, int* t1 = nullptr, int* t2 = nullptr) {
  if (dt != DT_F16 && dt != DT_BF16) return -20;
  const dim3 grid(max_tiles, rows), blk(256);
#define CAN_PACK_CASE(O, E)                                                                                        \
  case 2 * O + E:                                                                                                  \
    if (dt == DT_F16) hipLaunchKernelGGL((pack_multi_kernel<DT_F16, O, E>), grid, blk, 0, s, desc, sa);             \
    else hipLaunchKernelGGL((pack_multi_kernel<DT_BF16, O, E>), grid, blk, 0, s, desc, sa);                         \
    break
  switch (2 * opt + (ema ? 1 : 0)) {
    CAN_PACK_CASE(OPT_NONE, false);
    CAN_PACK_CASE(OPT_SGD, false);
    CAN_PACK_CASE(OPT_SGD, true);
    CAN_PACK_CASE(OPT_SGD_WD, false);
    CAN_PACK_CASE(OPT_SGD_WD, true);
    CAN_PACK_CASE(OPT_ADAM, false);
    CAN_PACK_CASE(OPT_ADAM, true);
    CAN_PACK_CASE(OPT_SWAP, false);
    default: return -2;
  }
#undef CAN_PACK_CASE
  if (t1 != nullptr || t2 != nullptr)
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, s, (const float*)sa.flags, t1, t2);
  return (int)hipGetLastError();
}

extern "C" int can_pack_multi(const long long* desc, int layers, int max_tiles, int dt, void* stream) {
  if (layers <= 0) return 0;
  return pack_multi_launch(desc, layers, max_tiles, dt, OPT_NONE, false, OptArgs{}, (hipStream_t)stream);
}

// Stand-alone Adam / AdamW over flat fp32 buffers (any n, any alignment).  t_dev: the device step count (applied steps
// so far; advanced by one here unless the step is skipped through flags); null: `step` is this call's 1-based step.
extern "C" int can_adam(float* p, float* m, float* v, const float* g, size_t n, float lr, double beta1, double beta2,
                        float eps, float wd, int decoupled, float gscale, int step, int* t_dev, float* flags,
                        const float* lr_dev, void* stream, const float* gmul) {
  if (n == 0) return 0;
  if (t_dev == nullptr && step < 1) return -2;
  OptArgs a{};
  a.lr = lr; a.gscale = gscale; a.wd = wd; a.eps = eps; a.decoupled = decoupled; a.beta1 = beta1; a.beta2 = beta2;
  a.flags = flags; a.lr_dev = lr_dev; a.t = t_dev; a.step = step; a.gmul = gmul;
  const int vec = (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256, 4096)), dim3(256), 0, s, p, m, v, g, n, vec,
                     a);
  if (t_dev != nullptr)
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, s, (const float*)flags, t_dev, (int*)nullptr);
  return (int)hipGetLastError();
}

// Stand-alone EMA update over flat fp32 buffers (any n, any alignment).  t_dev: the device count of applied updates
// (advanced by one here unless the update is skipped through flags); null: `step` is this call's 1-based update.
extern "C" int can_ema(float* e, const float* p, size_t n, double decay, int warmup, int step, int* t_dev, float* flags,
                       void* stream) {
  if (!(decay >= 0.0 && decay < 1.0)) return -2;
  if (t_dev == nullptr && step < 1) return -2;
  if (n == 0) return 0;
  OptArgs a{};
  a.ema_decay = decay; a.ema_warmup = warmup ? 1 : 0; a.ema_t = t_dev; a.step = step; a.flags = flags;
  const int vec = (((uintptr_t)e | (uintptr_t)p) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256, 4096)), dim3(256), 0, s, e, p, n, vec, a);
  if (t_dev != nullptr)
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, s, (const float*)flags, t_dev, (int*)nullptr);
  return (int)hipGetLastError();
}

// The fused optimizer step for every optimizer: rows cover every parameter of the arena once; the gradient and momentum
// arenas are at goff / boff floats from the masters.  opt 1 = SGD-momentum, 2 = SGD with coupled weight decay, 3 = Adam
// / AdamW (mom = first moment, second moment at voff; t_dev required, advanced when applied).  eoff != 0: the EMA of
// the parameters is updated in the same launch, its arena eoff floats from the masters, ema_t the device count of
// applied updates (required; advanced with the step, for every optimizer); refuses a decay outside [0, 1).
extern "C" int can_opt_pack(const long long* desc, int rows, int max_tiles, int opt, long long goff, long long boff,
                            long long voff, float lr, float momentum, double beta1, double beta2, float eps, float wd,
                            int decoupled, float gscale, int* t_dev, float* flags, const float* lr_dev, int dt,
                            void* stream, const float* gmul, long long eoff, double ema_decay, int ema_warmup,
                            int* ema_t) {
  const bool ema = eoff != 0;
  if (rows <= 0) return 0;
  if (opt < OPT_SGD || opt > OPT_ADAM || (opt == OPT_ADAM && t_dev == nullptr)) return -2;
  if (ema && (ema_t == nullptr || !(ema_decay >= 0.0 && ema_decay < 1.0))) return -2;
  OptArgs sa{};
  sa.goff = goff; sa.boff = boff; sa.voff = (opt == OPT_ADAM) ? voff : 0;
  sa.lr = lr; sa.momentum = momentum; sa.gscale = gscale; sa.wd = wd; sa.eps = eps; sa.decoupled = decoupled;
  sa.beta1 = beta1; sa.beta2 = beta2; sa.flags = flags; sa.lr_dev = lr_dev; sa.t = t_dev; sa.gmul = gmul;
  sa.eoff = eoff; sa.ema_decay = ema_decay; sa.ema_warmup = ema_warmup ? 1 : 0; sa.ema_t = ema_t;
  return pack_multi_launch(desc, rows, max_tiles, dt, opt, ema, sa, (hipStream_t)stream,
                           (opt == OPT_ADAM) ? t_dev : nullptr, ema ? ema_t : nullptr);
}

// The swap launch (pack_multi_kernel<DT, OPT_SWAP>): every master exchanged with its EMA copy eoff floats away, over
// the optimizer's descriptor rows, and every pack written from what lands in the master slot.  No flags: it always runs.
extern "C" int can_swap_pack(const long long* desc, int rows, int max_tiles, long long eoff, int dt, void* stream) {
  if (rows <= 0) return 0;
  if (eoff == 0) return -2;
  OptArgs sa{};
  sa.eoff = eoff;
  return pack_multi_launch(desc, rows, max_tiles, dt, OPT_SWAP, false, sa, (hipStream_t)stream);
}

// The gradient-norm pass (grad_norm_partial_kernel + grad_norm_final_kernel).  tab: np {offset, count} int64 pairs on
// the device; max_count: the largest count (host copy); part: np * ceil(max_count / 4096) doubles of scratch;
// gn: 2 + np floats; flag: the step's flags + 2 (optional).
extern "C" int can_grad_norm_chunk() { return kNormChunk; }
extern "C" int can_grad_norm(const float* g, const long long* tab, int np, long long max_count, double* part, float* gn,
                             float gscale, float max_norm, float* flag, void* stream) {
  if (np <= 0 || max_count < 0 || !(max_norm >= 0.f)) return -2;
  const long long mc = (max_count + kNormChunk - 1) / kNormChunk;
  if (mc > 0x7fffffffll || np > 65535) return -3;
  const int max_chunks = mc < 1 ? 1 : (int)mc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(max_chunks, np), dim3(256), 0, s, g, tab, part, max_chunks);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, tab, np, part, max_chunks, gn, gscale, max_norm,
                     flag);
  return (int)hipGetLastError();
}

// Count metrics of n samples (count_metrics_kernel + count_metrics_final_kernel): et [n][h][w] contiguous, gt and the
// optional weight plane m (null: 1) [h][w] planes gt_stride / m_stride floats apart from sample to sample (so the two
// channels of a [n,2,h,w] tensor are read in place), part: n * 128 doubles of scratch, out: [n][6] doubles.
extern "C" int can_count_metrics(const float* et, const float* gt, long long gt_stride, const float* m,
                                 long long m_stride, int n, int h, int w, double* part, double* out, void* stream) {
  if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || (long long)h * w > 0x0fffffff) return -2;
  if (et == nullptr || gt == nullptr || part == nullptr || out == nullptr) return -2;
  if (gt_stride < (long long)h * w || (m != nullptr && m_stride < (long long)h * w)) return -2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(count_metrics_kernel, dim3(64, n), dim3(256), 0, s, et, gt, gt_stride, m, m_stride, h, w, part);
  hipLaunchKernelGGL(count_metrics_final_kernel, dim3(n), dim3(128), 0, s, (const double*)part, out);
  return (int)hipGetLastError();
}

extern "C" int can_accum_tick(float* flags, float* acc, int fold, int close, void* stream) {
  if (fold < 0 || fold > 2) return -2;
  hipLaunchKernelGGL(accum_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flags, acc, fold, close);
  return (int)hipGetLastError();
}
