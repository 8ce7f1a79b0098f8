// The slice-ordered reduce of the small-channel and large-kernel weight gradients (conv_small.hip, conv_large.hip).
// Each translation unit that includes this gets its own copy of the kernel (anonymous namespace).
#pragma once
#include "common.h"
#include "conv_small_plan.h"

namespace can {
namespace {

// out[i] = scale * (part_0[i] + part_1[i] + ...) (+ beta * out[i]): slices in slice order; i < plane -> dw, else db
__global__ void __launch_bounds__(256) c16_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                         float* __restrict__ db, int S, int plane, int Co, float beta,
                                                         float scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = plane + (db != nullptr ? Co : 0);
  if (i >= n) return;
  const size_t stride = (size_t)plane + Co;
  float s = 0.f;
  for (int sl = 0; sl < S; ++sl) s += ws[(size_t)sl * stride + i];
  float* out = i < plane ? dw + i : db + (i - plane);
  *out = (beta != 0.f) ? scale * s + beta * *out : scale * s;
}

// S partials of plane + Co floats in ws -> dw (+ db when not null)
inline int c16_reduce(const float* ws, float* dw, float* db, int S, int plane, int Co, float beta, float scale,
                      hipStream_t s) {
  const int n = plane + (db != nullptr ? Co : 0);
  hipLaunchKernelGGL(c16_reduce_kernel, dim3(c16_cdiv(n, 256)), dim3(256), 0, s, ws, dw, db, S, plane, Co, beta, scale);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace can
