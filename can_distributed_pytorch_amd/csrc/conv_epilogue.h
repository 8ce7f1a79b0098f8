// Epilogue pieces shared by the forward / data-gradient conv kernels (conv_igemm.hip) and the stand-alone max-pool
// (elementwise.hip): what happens to one pixel's N consecutive output channels between the fp32 accumulators and the
// 16-bit store.  Every piece works on values already in registers, except load_bias (global reads) and
// pool_staged_store (LDS reads, global stores); the kernels keep their own mask / code loads, barriers and stores,
// whose placement is tuned per kernel.  Device-only, all inlined.
#pragma once
#include "common.h"
#include "conv_plan.h"

namespace can {

// two 16-bit lanes per VGPR (the max-pool epilogue works on the stored bf16 / fp16 bit patterns: after the ReLU they
// are non-negative, where the unsigned order of the bits is the order of the values)
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ unsigned pk_sub_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_sub_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ unsigned pk_lshl_b16(unsigned v, unsigned sh) {
  unsigned r;
  asm("v_pk_lshlrev_b16 %0, %1, %2" : "=v"(r) : "v"(sh), "v"(v));
  return r;
}
__device__ __forceinline__ unsigned pk_mul_lo_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// per 16-bit half: v >> sh (arithmetic), shift amounts from the halves of sh
__device__ __forceinline__ unsigned pk_ashr_i16(unsigned v, unsigned sh) {
  unsigned r;
  asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(r) : "v"(sh), "v"(v));
  return r;
}

// sign bits of 8 consecutive 16-bit values (two per 32-bit word, low half first): bit k = value k > 0
__device__ __forceinline__ unsigned sign_bits8(unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
  const unsigned w[4] = {w0, w1, w2, w3};
  unsigned b = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    b |= (pos_bits((unsigned short)(w[k] & 0xFFFFu)) ? 1u : 0u) << (2 * k);
    b |= (pos_bits((unsigned short)(w[k] >> 16)) ? 1u : 0u) << (2 * k + 1);
  }
  return b;
}
// of the 16 channels stored as o0 | o1 (EPI_MASKB layout: two bytes)
__device__ __forceinline__ unsigned sign_bits16(const uint4& o0, const uint4& o1) {
  return sign_bits8(o0.x, o0.y, o0.z, o0.w) | (sign_bits8(o1.x, o1.y, o1.z, o1.w) << 8);
}

// b[0 .. N) = p[0 .. N), 16-B loads
template <int N>
__device__ __forceinline__ void load_bias(float* b, const float* p) {
#pragma unroll
  for (int c = 0; c < N; c += 4) {
    const float4 b4 = *reinterpret_cast<const float4*>(p + c);
    b[c] = b4.x; b[c + 1] = b4.y; b[c + 2] = b4.z; b[c + 3] = b4.w;
  }
}

// the lane's 4 NJ channels of pixel fragment i (MFMA D layout: row block j holds channels 4j .. 4j + 3 of the lane);
// the second form for a kernel that keeps one fragment's accumulators at a time
template <int NJ, int NI>
__device__ __forceinline__ void frag_values(float* v, const f32x4 (&acc)[NJ][NI], int i) {
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[j * 4 + r] = acc[j][i][r];
}
template <int NJ>
__device__ __forceinline__ void frag_values(float* v, const f32x4 (&acc)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[j * 4 + r] = acc[j][r];
}

// EPI_BIAS_RELU / EPI_BIAS / EPI_POOLFWD: bias, ReLU (not EPI_BIAS), and zero where the pixel is not valid (cv: a
// padding column of a width-padded map)
template <int EPI, int N>
__device__ __forceinline__ void bias_act(float* v, const float* bias, bool cv) {
#pragma unroll
  for (int c = 0; c < N; ++c) {
    v[c] += bias[c];
    if (EPI != EPI_BIAS) v[c] = fmaxf(v[c], 0.f);
    v[c] = cv ? v[c] : 0.f;
  }
}

template <int N>
__device__ __forceinline__ void sigmoid(float* v) {
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = 1.f / (1.f + __expf(-v[c]));
}

// ReLU mask of a data gradient: v[c] kept where the masking activation is > 0, from its 16-bit map (N / 2 words,
// channel c in half c & 1 of word c / 2) or from its sign bits (bit c); SUM: the masked values also go into the
// bias-gradient sums bs[]
template <int N, bool SUM>
__device__ __forceinline__ void relu_mask16(float* v, const unsigned* words, float* bs) {
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const unsigned short bits = (unsigned short)(words[c >> 1] >> ((c & 1) * 16));
    const bool pos = pos_bits(bits);
    v[c] = pos ? v[c] : 0.f;
    if (SUM) bs[c] += v[c];
  }
}
template <int N, bool SUM>
__device__ __forceinline__ void relu_mask_bits(float* v, unsigned bits, float* bs) {
#pragma unroll
  for (int c = 0; c < N; ++c) {
    v[c] = ((bits >> c) & 1u) ? v[c] : 0.f;
    if (SUM) bs[c] += v[c];
  }
}

// 2x2 max-pool of 8 channels: t[q] = the window's values at position q in ATen scan order (row * 2 + column),
// m = their max.  pool_codes: the max-pool code word (conv_igemm.hip "Max-pool codes": nibble k = one-hot of the
// FIRST max of channel k, 0 when that max is not > 0).  The conv pool epilogues and maxpool_fwd_kernel must agree bit
// for bit, which is why there is one copy; two steps, because every caller stores the max before it builds the codes
__device__ __forceinline__ void pool_max(const float (&t)[4][8], float (&m)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = fmaxf(fmaxf(t[0][k], t[1][k]), fmaxf(t[2][k], t[3][k]));
}
__device__ __forceinline__ uint32_t pool_codes(const float (&t)[4][8], const float (&m)[8]) {
  uint32_t cw = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t first = (t[0][k] == m[k]) ? 1u : (t[1][k] == m[k]) ? 2u : (t[2][k] == m[k]) ? 4u : 8u;
    cw |= ((m[k] > 0.f) ? first : 0u) << (4 * k);
  }
  return cw;
}

// Pool tail of the kernels that stage their 4 x 64-pixel, 64-channel output tile in LDS ([4 rows][64 cols] x 128 B,
// 16-B chunk c of column col at slot c ^ (col & 7)): pooled pixel (pr, pc) of the tile, channels 8c .. 8c + 7; max of
// the stored (rounded) values, exactly what maxpool_fwd_kernel computes from the stored map.  pp = the pooled
// pixel's index in yp [..][64] / codes [..][8] (codes optional)
template <int DT>
__device__ __forceinline__ void pool_staged_store(const unsigned char* stage, int pr, int pc, int c, size_t pp,
                                                  bf16_t* yp, uint32_t* codes) {
  float m[8], t[4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int rr = 2 * pr + (q >> 1), cc = 2 * pc + (q & 1);
    unpack8h<DT>(reinterpret_cast<const uint4*>(stage + (rr * 64 + cc) * 128)[c ^ (cc & 7)], t[q]);
  }
  pool_max(t, m);
  *reinterpret_cast<uint4*>(yp + pp * 64 + c * 8) = pack8h<DT>(m);
  if (codes != nullptr) codes[pp * 8 + c] = pool_codes(t, m);
}

}  // namespace can
