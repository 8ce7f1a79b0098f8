// GPU input pipeline for CrowdDataset samples (gfx950).
//
// Reference semantics (model/CrowdDataset.py:38-67): image/255 -> optional
// horizontal flip -> cv2.resize(INTER_LINEAR) to (W//8*8, H//8*8) ->
// ImageNet normalisation; density -> same flip -> cv2.resize to (W//8, H//8)
// -> x64.  cv2's INTER_LINEAR = half-pixel-centre bilinear, source
// coordinate clamped at 0 (left/top) and taps clamped at the last pixel,
// no anti-aliasing.  Here both run on the GPU straight from the decoded uint8
// image and write the first conv layer's NHWC4 bf16 layout (channel 3 = 0),
// so the host only decodes JPEGs.
//
// Every kernel below is built from one set of helpers: lin_tap (the tap rule), blend4 (the four-tap blend),
// imagenet / normalise / pack_px (ImageNet constants, x 1/255, NHWC4 words), resample_px (a whole pixel) and load_desc; the
// PHOTO instantiations of the crop kernels (photometric jitter) add load_photo and lut_tap (a source pixel's three values
// through the sample's tone table).
#include "common.h"

namespace can {

__device__ __forceinline__ void lin_tap(int o, float scale, int in, int& i0, int& i1, float& f) {
  float src = ((float)o + 0.5f) * scale - 0.5f;
  if (src < 0.f) src = 0.f;
  int x0 = (int)src;
  f = src - (float)x0;
  if (x0 >= in - 1) { x0 = in - 1; f = 0.f; }
  i0 = x0;
  i1 = min(x0 + 1, in - 1);
}

// taps a b (top row) / d e (bottom row), left to right
__device__ __forceinline__ float blend4(float a, float b, float d, float e, float fx, float fy) {
  const float top = a + (b - a) * fx, bot = d + (e - d) * fx;
  return top + (bot - top) * fy;
}

// channel c of a pixel in [0, 1] -> ImageNet-normalised (the one copy of the constants)
__device__ __forceinline__ float imagenet(float v, int c) {
  const float m[3] = {0.485f, 0.456f, 0.406f}, is[3] = {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f};
  return (v - m[c]) * is[c];
}

// the same of a pixel on the uint8 scale [0, 255]
__device__ __forceinline__ float normalise(float v, int c) { return imagenet(v * (1.f / 255.f), c); }

// one NHWC4 pixel (channel 3 = 0) as two 16-bit pairs
template <int DT>
__device__ __forceinline__ uint2 pack_px(const float (&v)[3]) {
  return make_uint2(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], 0.f));
}

// The row of floats per output sample of a photo pack: 256 tone-table entries on the 0..255 scale, the gray flag, 3 zeros.
constexpr int PHOTO_ROW = 260;

// PHOTO: the three channel values of one source pixel on the 0..255 scale.  Every byte goes through the sample's tone
// table lut (LDS) instead of the int-to-float conversion; gray (C == 1) feeds all three channels; with mix a colour
// pixel becomes its luma in all three (a 1-channel pixel is left alone).
__device__ __forceinline__ void lut_tap(const unsigned char* px, int C, const float* lut, bool mix, float (&t)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = lut[px[(C == 1) ? 0 : c]];
  if (mix && C != 1) t[0] = t[1] = t[2] = __fmaf_rn(0.114f, t[2], __fmaf_rn(0.587f, t[1], 0.299f * t[0]));
}

// One output pixel of a uint8 image: tap rows ra / rb, tap pixels at byte offsets oa / ob of a row; gray (C == 1)
// feeds all three channels.  PHOTO: the four tap pixels are lut_tap's values.
template <int DT, bool PHOTO = false>
__device__ __forceinline__ uint2 resample_px(const unsigned char* ra, const unsigned char* rb, size_t oa, size_t ob,
                                             int C, float fx, float fy, const float* lut = nullptr, bool mix = false) {
  float v[3];
  if constexpr (PHOTO) {
    float a[3], b[3], d[3], e[3];
    lut_tap(ra + oa, C, lut, mix, a);
    lut_tap(ra + ob, C, lut, mix, b);
    lut_tap(rb + oa, C, lut, mix, d);
    lut_tap(rb + ob, C, lut, mix, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = normalise(blend4(a[c], b[c], d[c], e[c], fx, fy), c);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cc = (C == 1) ? 0 : c;
      v[c] = normalise(blend4(ra[oa + cc], ra[ob + cc], rb[oa + cc], rb[ob + cc], fx, fy), c);
    }
  }
  return pack_px<DT>(v);
}

// A block's 256 threads bring their sample's (blockIdx.y's) tone table into lut, one entry each, and return the
// sample's gray flag, a block-uniform value; the barrier stands ahead of the pixel loop.
__device__ __forceinline__ bool load_photo(const float* __restrict__ photo, float* lut) {
  const float* row = photo + (size_t)blockIdx.y * PHOTO_ROW;
  lut[threadIdx.x] = row[threadIdx.x];
  const bool mix = row[256] != 0.f;
  __syncthreads();
  return mix;
}

// Sample blockIdx.y's descriptor {image byte offset, H0, W0, C, flip, y0, x0, ext}: slots 5..7 are 0 for a whole
// image, ext == 1 for an unscaled crop at (y0, x0), ext == (sh << 32) | sw for a window of that extent.
struct Desc {
  long long off;
  int H0, W0, C, flip, y0, x0;
  long long ext;
};

__device__ __forceinline__ Desc load_desc(const long long* desc) {
  const long long* d = desc + (size_t)blockIdx.y * 8;
  return {d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], (int)d[6], d[7]};
}

// img: uint8 [H0][W0][C] (C = 1, 3 or 4) -> out NHWC4 bf16 [Ho][Wo][4] (sample n of a batch)
template <int DT>
__global__ void __launch_bounds__(256) preprocess_image_kernel(const unsigned char* __restrict__ img, int H0, int W0,
                                                               int C, int flip, uint2* __restrict__ out, int Ho,
                                                               int Wo) {
  const float sy = (float)H0 / (float)Ho, sx = (float)W0 / (float)Wo;
  const int total = Ho * Wo;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int oy = i / Wo, ox = i % Wo;
    int y0, y1, x0, x1;
    float fy, fx;
    lin_tap(oy, sy, H0, y0, y1, fy);
    lin_tap(ox, sx, W0, x0, x1, fx);
    if (flip) {   // flip happens BEFORE the resize in the reference: mirror the source columns
      x0 = W0 - 1 - x0;
      x1 = W0 - 1 - x1;
    }
    out[i] = resample_px<DT>(img + (size_t)y0 * W0 * C, img + (size_t)y1 * W0 * C, (size_t)x0 * C, (size_t)x1 * C, C,
                             fx, fy);
  }
}

// density fp32 [H0][W0] -> [Ho][Wo] x mult (after optional flip)
__global__ void __launch_bounds__(256) preprocess_density_kernel(const float* __restrict__ d, int H0, int W0, int flip,
                                                                 float* __restrict__ out, int Ho, int Wo, float mult) {
  const float sy = (float)H0 / (float)Ho, sx = (float)W0 / (float)Wo;
  const int total = Ho * Wo;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int oy = i / Wo, ox = i % Wo;
    int y0, y1, x0, x1;
    float fy, fx;
    lin_tap(oy, sy, H0, y0, y1, fy);
    lin_tap(ox, sx, W0, x0, x1, fx);
    if (flip) { x0 = W0 - 1 - x0; x1 = W0 - 1 - x1; }
    const float* ra = d + (size_t)y0 * W0;
    const float* rb = d + (size_t)y1 * W0;
    out[i] = blend4(ra[x0], ra[x1], rb[x0], rb[x1], fx, fy) * mult;
  }
}

// Random-crop batch in ONE launch (no resize): desc[n] = {image byte offset, H0, W0, C, flip, y0, x0, 1}; several
// descriptors may share one image.  Output sample n = the window [y0, y0+vh) x [x0, x0+vw) of its image, vh =
// min(CH, H0/ds*ds), vw = min(CW, W0/ds*ds), mirrored within the window when flipped, normalised, zero outside the
// window (bottom / right padding of an image smaller than the crop).  A thread writes two adjacent NHWC4 pixels as
// one 16-byte store (CW is even); it reads only bytes of the window.  PHOTO (can_preprocess_crop_photo): every source
// byte goes through the sample's tone table and gray mix (lut_tap); the padding stays zero.
template <int DT, bool PHOTO = false, typename... Photo>
__global__ void __launch_bounds__(256) preprocess_crop_kernel(const unsigned char* __restrict__ imgs,
                                                              const long long* __restrict__ desc,
                                                              uint4* __restrict__ x4, int CH, int CW, int ds,
                                                              Photo... photo) {
  static_assert(sizeof...(Photo) == (PHOTO ? 1 : 0), "the photo region is the one extra argument of a PHOTO kernel");
  __shared__ float lut[PHOTO ? 256 : 1];
  bool mix = false;
  if constexpr (PHOTO) mix = load_photo(photo..., lut);
  const Desc s = load_desc(desc);
  const int vh = min(CH, s.H0 / ds * ds), vw = min(CW, s.W0 / ds * ds);
  const unsigned char* img = imgs + s.off;
  const int half = CW / 2;
  uint4* out = x4 + (size_t)blockIdx.y * CH * half;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < CH * half; i += gridDim.x * 256) {
    const int oy = i / half, ox = (i % half) * 2;
    uint2 w[2] = {make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (oy < vh) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int x = ox + p;
        if (x < vw) {
          const int sx = s.x0 + (s.flip ? vw - 1 - x : x);
          const unsigned char* px = img + ((size_t)(s.y0 + oy) * s.W0 + sx) * s.C;
          float v[3];
          if constexpr (PHOTO) {
            lut_tap(px, s.C, lut, mix, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = normalise(v[c], c);
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = normalise((float)px[(s.C == 1) ? 0 : c], c);
          }
          w[p] = pack_px<DT>(v);
        }
      }
    }
    out[i] = make_uint4(w[0].x, w[0].y, w[1].x, w[1].y);
  }
}

// Resize batch and random-scale crop batch, ONE launch either way.  Output sample n = a window of its image resampled
// to CH x CW by the cv2 INTER_LINEAR rule (lin_tap relative to the window, taps clamped inside it; column taps
// mirrored within the window when flipped: the flip comes BEFORE the resize), normalised.  The window is the whole
// image where slot 7 of the descriptor is 0 (an uncropped pack, can_preprocess_batch) and [y0, y0+sh) x [x0, x0+sw)
// where it is (sh << 32) | sw (can_preprocess_crop_scaled); several descriptors may share one image.  No padding:
// the whole sample is valid.  It reads only bytes of the window.  For sh == CH, sw == CW every fraction is exactly 0
// and the blend returns the pixel itself, so the output is bitwise preprocess_crop_kernel's.  A thread writes two
// adjacent NHWC4 pixels as one 16-byte store (CW is even).  PHOTO (can_preprocess_crop_photo): every tap pixel goes
// through the sample's tone table and gray mix (lut_tap) BEFORE the blend.
template <int DT, bool PHOTO = false, typename... Photo>
__global__ void __launch_bounds__(256) preprocess_resample_kernel(const unsigned char* __restrict__ imgs,
                                                                  const long long* __restrict__ desc,
                                                                  uint4* __restrict__ x4, int CH, int CW,
                                                                  Photo... photo) {
  static_assert(sizeof...(Photo) == (PHOTO ? 1 : 0), "the photo region is the one extra argument of a PHOTO kernel");
  __shared__ float lut[PHOTO ? 256 : 1];
  bool mix = false;
  if constexpr (PHOTO) mix = load_photo(photo..., lut);
  const Desc s = load_desc(desc);
  const int sh = s.ext ? (int)(s.ext >> 32) : s.H0, sw = s.ext ? (int)(s.ext & 0xffffffffll) : s.W0;
  const int y0 = s.ext ? s.y0 : 0, x0 = s.ext ? s.x0 : 0;
  const unsigned char* win = imgs + s.off + ((size_t)y0 * s.W0 + x0) * s.C;      // the window's first pixel
  const size_t pitch = (size_t)s.W0 * s.C;
  const float sy = (float)sh / (float)CH, sx = (float)sw / (float)CW;
  const int half = CW / 2;
  uint4* out = x4 + (size_t)blockIdx.y * CH * half;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < CH * half; i += gridDim.x * 256) {
    const int oy = i / half, ox = (i % half) * 2;
    int ya, yb;
    float fy;
    lin_tap(oy, sy, sh, ya, yb, fy);
    const unsigned char* ra = win + (size_t)ya * pitch;
    const unsigned char* rb = win + (size_t)yb * pitch;
    uint2 w[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int xa, xb;
      float fx;
      lin_tap(ox + p, sx, sw, xa, xb, fx);
      if (s.flip) { xa = sw - 1 - xa; xb = sw - 1 - xb; }
      w[p] = resample_px<DT, PHOTO>(ra, rb, (size_t)xa * s.C, (size_t)xb * s.C, s.C, fx, fy, lut, mix);
    }
    out[i] = make_uint4(w[0].x, w[0].y, w[1].x, w[1].y);
  }
}

// ROI weight plane of a pack whose images are 4-channel, the mask in the alpha byte (README, "ROI masks").  Grid
// (16 x 16 cell tile, sample), one cell per thread.  The window is read from the descriptor as the image kernels and
// gt_from_heads_kernel read it: the whole image for slot 7 == 0, the valid (vh, vw) of the crop at (y0, x0) for 1 (its
// cells exact ds x ds boxes, the padding cells 0), [y0, y0+sh) x [x0, x0+sw) otherwise.  Cell (i, j) of a window cut
// into R x Q cells covers rows [i sh / R, (i+1) sh / R) and the columns of j' = Q-1-j when flipped; with the integer
// overlap numerators oy_i(t) = min((t+1) R, (i+1) sh) - max(t R, i sh) and ox likewise,
//   S = sum_t sum_u oy_i(t) ox_j'(u) alpha[y0+t][x0+u]   (int64),   m = float(double(S) / double(255 sh sw)):
// integers up to one division, so the host rule (data/transforms.py:roi_weights) gives the same bits.  It reads no
// byte outside the window.  out [n][2][rows][cols]: plane 0 = gt (the pack's ground truth region), plane 1 = m.
__global__ void __launch_bounds__(256) roi_weights_kernel(const unsigned char* __restrict__ imgs,
                                                          const long long* __restrict__ desc,
                                                          const float* __restrict__ gt, float* __restrict__ out,
                                                          int rows, int cols, int ds) {
  const Desc s = load_desc(desc);
  const int tiles_x = (cols + 15) / 16;
  const int i = (blockIdx.x / tiles_x) * 16 + (threadIdx.x >> 4), j = (blockIdx.x % tiles_x) * 16 + (threadIdx.x & 15);
  if (i >= rows || j >= cols) return;
  long long y0 = s.y0, x0 = s.x0, sh, sw;
  int R = rows, Q = cols;
  if (s.ext == 0) {
    y0 = 0; x0 = 0; sh = s.H0; sw = s.W0;
  } else if (s.ext == 1) {
    R = min(rows, s.H0 / ds); Q = min(cols, s.W0 / ds);
    sh = (long long)R * ds; sw = (long long)Q * ds;
  } else {
    sh = s.ext >> 32; sw = s.ext & 0xffffffffll;
  }
  const size_t plane = (size_t)rows * cols;
  const size_t o = (size_t)blockIdx.y * 2 * plane + (size_t)i * cols + j;
  out[o] = gt[(size_t)blockIdx.y * plane + (size_t)i * cols + j];
  float m = 0.f;
  if (i < R && j < Q) {
    const long long jj = s.flip ? Q - 1 - j : j;
    const long long ta = (i * sh) / R, tb = ((i + 1) * sh + R - 1) / R;
    const long long ua = (jj * sw) / Q, ub = ((jj + 1) * sw + Q - 1) / Q;
    const unsigned char* alpha = imgs + s.off + 3;
    long long S = 0;
    for (long long t = ta; t < tb; ++t) {
      const long long oy = min((t + 1) * R, (i + 1) * sh) - max(t * R, i * sh);
      const unsigned char* row = alpha + ((size_t)(y0 + t) * s.W0 + x0) * 4;
      long long rs = 0;
      for (long long u = ua; u < ub; ++u) {
        const long long ox = min((u + 1) * Q, (jj + 1) * sw) - max(u * Q, jj * sw);
        rs += ox * row[(size_t)u * 4];
      }
      S += oy * rs;
    }
    m = (float)((double)S / (double)(255ll * sh * sw));
  }
  out[o + plane] = m;
}

// ---------------------------------------------------------------------------
// Synthetic crowd batch on the GPU (train.py --synthetic / bench data; data/synthetic.py is the CPU
// reference of the same recipe): per image, head points (host RNG, tiny) -> fixed-sigma Gaussian
// density (density_splat, density.hip) -> 8x8 sum-pool to the 1/8 ground truth (count preserving);
// image = bilinear upsample of a coarse noise grid + 0.3 * density / max(density), ImageNet-normalised,
// written as NHWC4 16-bit.
// dens: [N][H][W] fp32 full-res density, noise: [N][3][H/16][W/16] fp32, dmax: [N] per-image max.
__global__ void __launch_bounds__(256) synth_gt_kernel(const float* __restrict__ dens, float* __restrict__ gt,
                                                       float* __restrict__ dmax, int H, int W) {
  // blockIdx.y = image: 8x8 sum pool + per-image max (block-level max -> atomicMax on the float bits,
  // valid for the non-negative densities)
  const float* d = dens + (size_t)blockIdx.y * H * W;
  const int Hd = H / 8, Wd = W / 8;
  float mx = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < Hd * Wd; i += gridDim.x * 256) {
    const int oy = i / Wd, ox = i % Wd;
    float s = 0.f;
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float v = d[(size_t)(oy * 8 + r) * W + ox * 8 + c];
        s += v;
        mx = fmaxf(mx, v);
      }
    gt[(size_t)blockIdx.y * Hd * Wd + i] = s;
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int*>(dmax + blockIdx.y), __float_as_int(mx));
}

template <int DT>
__global__ void __launch_bounds__(256) synth_image_kernel(const float* __restrict__ dens,
                                                          const float* __restrict__ noise,
                                                          const float* __restrict__ dmax, uint2* __restrict__ x4,
                                                          int H, int W) {
  const int n = blockIdx.y, Hn = H / 16, Wn = W / 16;
  const float* d = dens + (size_t)n * H * W;
  const float* nz = noise + (size_t)n * 3 * Hn * Wn;
  const float inv = 1.f / (dmax[n] + 1e-6f);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
    const int oy = i / W, ox = i % W;
    int y0, y1, x0, x1;
    float fy, fx;
    lin_tap(oy, (float)Hn / (float)H, Hn, y0, y1, fy);
    lin_tap(ox, (float)Wn / (float)W, Wn, x0, x1, fx);
    const float blob = 0.3f * d[i] * inv;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = nz + (size_t)c * Hn * Wn;
      const float up = blend4(p[y0 * Wn + x0], p[y0 * Wn + x1], p[y1 * Wn + x0], p[y1 * Wn + x1], fx, fy);
      v[c] = imagenet(fminf(fmaxf(0.7f * up + blob, 0.f), 1.f), c);
    }
    x4[(size_t)n * H * W + i] = pack_px<DT>(v);
  }
}

}  // namespace can

namespace {

// blocks of 256 threads for `work` items, capped: the kernels stride over what is left
int capped_grid(long long work, int cap) {
  const long long b = (work + 255) / 256;
  return (int)(b < cap ? b : cap);
}

// the arguments of a crop launch, apart from the descriptors
bool crop_args_ok(const void* imgs, const long long* desc, const long long* desc_host, int n, const void* x4, int CH,
                  int CW, int ds) {
  if (n <= 0 || n > 65535 || ds <= 0 || CH <= 0 || CW <= 0 || CH % ds || CW % ds || CW % 2) return false;
  if ((long long)CH * CW > 0x7fffffff) return false;
  return imgs != nullptr && desc != nullptr && desc_host != nullptr && x4 != nullptr && !((uintptr_t)x4 & 15);
}

// one host descriptor: a 1-, 3- or 4-channel image inside the img_bytes of packed images, and a window of extent
// eh x ew at (y0, x0) inside that image
bool crop_desc_ok(const long long* d, long long img_bytes, long long eh, long long ew) {
  const long long off = d[0], H0 = d[1], W0 = d[2], C = d[3], flip = d[4], y0 = d[5], x0 = d[6];
  if ((C != 1 && C != 3 && C != 4) || (flip != 0 && flip != 1)) return false;
  if (H0 <= 0 || W0 <= 0 || H0 > 0x7fffffff || W0 > 0x7fffffff) return false;
  if (off < 0 || off > img_bytes || H0 * W0 > (img_bytes - off) / C) return false;
  return y0 >= 0 && x0 >= 0 && y0 <= H0 - eh && x0 <= W0 - ew;
}

// the host descriptors of an unscaled crop launch: slot 7 == 1, the valid extent of the crop inside its image
bool crop_descs_ok(const long long* desc_host, int n, long long img_bytes, int CH, int CW, int ds) {
  for (int i = 0; i < n; ++i) {
    const long long* d = desc_host + (size_t)i * 8;
    const long long vh = d[1] / ds * ds < CH ? d[1] / ds * ds : CH, vw = d[2] / ds * ds < CW ? d[2] / ds * ds : CW;
    if (d[7] != 1 || !crop_desc_ok(d, img_bytes, vh, vw)) return false;
  }
  return true;
}

// the host descriptors of a scaled crop launch: slot 7 == (sh << 32) | sw, a window inside its image and within a
// factor 4 of the crop either way
bool scaled_descs_ok(const long long* desc_host, int n, long long img_bytes, int CH, int CW) {
  for (int i = 0; i < n; ++i) {
    const long long* d = desc_host + (size_t)i * 8;
    const long long sh = d[7] >> 32, sw = d[7] & 0xffffffffll;
    if (d[7] <= 1 || sh < 1 || sw < 1 || sh > d[1] || sw > d[2] || !crop_desc_ok(d, img_bytes, sh, sw)) return false;
    if (sh > 4ll * CH || sw > 4ll * CW || CH > 4 * sh || CW > 4 * sw) return false;
  }
  return true;
}

// the host copy of a photo region: every table entry finite and in [0, 255] (a NaN fails both comparisons), every
// gray flag 0 or 1
bool photo_rows_ok(const float* photo_host, int n) {
  for (int i = 0; i < n; ++i) {
    const float* row = photo_host + (size_t)i * can::PHOTO_ROW;
    for (int u = 0; u < 256; ++u)
      if (!(row[u] >= 0.f && row[u] <= 255.f)) return false;
    if (row[256] != 0.f && row[256] != 1.f) return false;
  }
  return true;
}

}  // namespace

// Images only: the ground truth of a pack arrives at 1/ds resolution already, so dens and gt must be null.
extern "C" int can_preprocess_batch(const void* imgs, const float* dens, const long long* desc, int n, void* x4,
                                    float* gt, int Ho, int Wo, int ds, int dt, void* stream) {
  using namespace can;
  if (n <= 0 || Ho % ds || Wo % ds || Wo % 2 || ((uintptr_t)x4 & 15)) return -2;
  if (dens != nullptr || gt != nullptr) return -2;
  CAN_LAUNCH_DT(dt, preprocess_resample_kernel, dim3(capped_grid((long long)Ho * (Wo / 2), 512), n), dim3(256), 0,
                (hipStream_t)stream, (const unsigned char*)imgs, desc, (uint4*)x4, Ho, Wo);
  return (int)hipGetLastError();
}

// desc: the device copy the kernel reads; desc_host: the same [n][8] table on the host, checked here before the
// launch (a window that leaves its image, or an image that leaves the img_bytes of packed images, is refused).
extern "C" int can_preprocess_crop(const void* imgs, long long img_bytes, const long long* desc,
                                   const long long* desc_host, int n, void* x4, int CH, int CW, int ds, int dt,
                                   void* stream) {
  using namespace can;
  if (!crop_args_ok(imgs, desc, desc_host, n, x4, CH, CW, ds)) return -2;
  if (!crop_descs_ok(desc_host, n, img_bytes, CH, CW, ds)) return -2;
  CAN_LAUNCH_DT(dt, preprocess_crop_kernel, dim3(capped_grid((long long)CH * (CW / 2), 512), n), dim3(256), 0,
                (hipStream_t)stream, (const unsigned char*)imgs, desc, (uint4*)x4, CH, CW, ds);
  return (int)hipGetLastError();
}

// can_preprocess_crop's checks on the window extents of slot 7, which must also be inside the image and within a
// factor 4 of the crop either way (the range of --crop-scale, with the rounding of the extents).
extern "C" int can_preprocess_crop_scaled(const void* imgs, long long img_bytes, const long long* desc,
                                          const long long* desc_host, int n, void* x4, int CH, int CW, int ds, int dt,
                                          void* stream) {
  using namespace can;
  if (!crop_args_ok(imgs, desc, desc_host, n, x4, CH, CW, ds)) return -2;
  if (!scaled_descs_ok(desc_host, n, img_bytes, CH, CW)) return -2;
  CAN_LAUNCH_DT(dt, preprocess_resample_kernel, dim3(capped_grid((long long)CH * (CW / 2), 512), n), dim3(256), 0,
                (hipStream_t)stream, (const unsigned char*)imgs, desc, (uint4*)x4, CH, CW);
  return (int)hipGetLastError();
}

namespace {

template <int DT>
void launch_photo(int scaled, dim3 grid, hipStream_t stream, const unsigned char* imgs, const long long* desc,
                  uint4* x4, int CH, int CW, int ds, const float* photo) {
  using namespace can;
  if (scaled)
    hipLaunchKernelGGL((preprocess_resample_kernel<DT, true>), grid, dim3(256), 0, stream, imgs, desc, x4, CH, CW,
                       photo);
  else
    hipLaunchKernelGGL((preprocess_crop_kernel<DT, true>), grid, dim3(256), 0, stream, imgs, desc, x4, CH, CW, ds,
                       photo);
}

}  // namespace

// can_preprocess_crop (scaled == 0) or can_preprocess_crop_scaled (scaled != 0) with photometric jitter: photo, float
// [n][260] on the device (16-byte aligned), is one row per output sample of 256 tone-table entries on the 0..255 scale,
// the gray flag and three zeros; photo_host is the same region on the host.  Everything the plain entry refuses is
// refused, and so are a table entry that is not finite or leaves [0, 255] and a gray flag other than 0 or 1: all of it
// on the host copies, before the launch.
extern "C" int can_preprocess_crop_photo(const void* imgs, long long img_bytes, const long long* desc,
                                         const long long* desc_host, int n, void* x4, int CH, int CW, int ds, int dt,
                                         void* stream, const float* photo, const float* photo_host, int scaled) {
  using namespace can;
  if (!crop_args_ok(imgs, desc, desc_host, n, x4, CH, CW, ds)) return -2;
  if (photo == nullptr || photo_host == nullptr || ((uintptr_t)photo & 15)) return -2;
  if (!(scaled ? scaled_descs_ok(desc_host, n, img_bytes, CH, CW) : crop_descs_ok(desc_host, n, img_bytes, CH, CW, ds)))
    return -2;
  if (!photo_rows_ok(photo_host, n)) return -2;
  const dim3 grid(capped_grid((long long)CH * (CW / 2), 512), n);
  if (dt == DT_F16)
    launch_photo<DT_F16>(scaled, grid, (hipStream_t)stream, (const unsigned char*)imgs, desc, (uint4*)x4, CH, CW, ds,
                         photo);
  else if (dt == DT_BF16)
    launch_photo<DT_BF16>(scaled, grid, (hipStream_t)stream, (const unsigned char*)imgs, desc, (uint4*)x4, CH, CW, ds,
                          photo);
  else
    return -20;
  return (int)hipGetLastError();
}

// The host descriptors of a roi launch, each refusal with its own code (api.h): every image 4-channel (-31), the sample
// a multiple of ds (-32), every window non-empty and inside its image, the image inside img_bytes (-33).
extern "C" int can_roi_weights_check(const long long* desc_host, int n, long long img_bytes, int CH, int CW, int ds) {
  if (desc_host == nullptr || n <= 0 || n > 65535 || ds <= 0 || CH <= 0 || CW <= 0 || img_bytes < 0) return -2;
  if ((long long)CH * CW > 0x7fffffff) return -2;
  for (int i = 0; i < n; ++i)
    if (desc_host[(size_t)i * 8 + 3] != 4) return -31;
  if (CH % ds || CW % ds) return -32;
  for (int i = 0; i < n; ++i) {
    const long long* d = desc_host + (size_t)i * 8;
    const long long H0 = d[1], W0 = d[2];
    long long eh, ew;
    if (d[7] == 0) {                       // whole image: the sample is its largest multiple of ds
      if (d[5] != 0 || d[6] != 0 || H0 / ds * ds != CH || W0 / ds * ds != CW) return -33;
      eh = H0;
      ew = W0;
    } else if (d[7] == 1) {
      eh = H0 / ds * ds < CH ? H0 / ds * ds : CH;
      ew = W0 / ds * ds < CW ? W0 / ds * ds : CW;
    } else {
      eh = d[7] >> 32;
      ew = d[7] & 0xffffffffll;
      if (d[7] < 0 || eh < 1 || ew < 1) return -33;
    }
    if (!crop_desc_ok(d, img_bytes, eh, ew)) return -33;
  }
  return 0;
}

extern "C" int can_roi_weights(const void* imgs, long long img_bytes, const long long* desc,
                               const long long* desc_host, int n, const float* gt, float* out, int CH, int CW, int ds,
                               void* stream) {
  using namespace can;
  if (imgs == nullptr || desc == nullptr || gt == nullptr || out == nullptr) return -2;
  const int rc = can_roi_weights_check(desc_host, n, img_bytes, CH, CW, ds);
  if (rc) return rc;
  const int rows = CH / ds, cols = CW / ds;
  hipLaunchKernelGGL(roi_weights_kernel, dim3(((rows + 15) / 16) * ((cols + 15) / 16), n), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned char*)imgs, desc, gt, out, rows, cols, ds);
  return (int)hipGetLastError();
}

extern "C" int can_synth_render(const float* dens, const float* noise, float* dmax, void* x4, float* gt, int n, int H,
                                int W, int dt, void* stream) {
  using namespace can;
  if (n <= 0 || H % 16 || W % 16) return -2;
  hipStream_t s = (hipStream_t)stream;
  CAN_HIP_CHECK(hipMemsetAsync(dmax, 0, sizeof(float) * n, s));
  hipLaunchKernelGGL(synth_gt_kernel, dim3(capped_grid((long long)(H / 8) * (W / 8), 256), n), dim3(256), 0, s, dens,
                     gt, dmax, H, W);
  CAN_LAUNCH_DT(dt, synth_image_kernel, dim3(capped_grid((long long)H * W, 1024), n), dim3(256), 0, s, dens, noise,
                dmax, (uint2*)x4, H, W);
  return (int)hipGetLastError();
}

extern "C" int can_preprocess_image(const void* img, int H0, int W0, int C, int flip, void* out, int Ho, int Wo, int dt,
                                    void* stream) {
  using namespace can;
  if (C != 1 && C != 3 && C != 4) return -2;
  CAN_LAUNCH_DT(dt, preprocess_image_kernel, dim3(capped_grid((long long)Ho * Wo, 4096)), dim3(256), 0,
                (hipStream_t)stream, (const unsigned char*)img, H0, W0, C, flip, (uint2*)out, Ho, Wo);
  return (int)hipGetLastError();
}

extern "C" int can_preprocess_density(const float* d, int H0, int W0, int flip, float* out, int Ho, int Wo,
                                      float mult, void* stream) {
  using namespace can;
  hipLaunchKernelGGL(preprocess_density_kernel, dim3(capped_grid((long long)Ho * Wo, 4096)), dim3(256), 0,
                     (hipStream_t)stream, d, H0, W0, flip, out, Ho, Wo, mult);
  return (int)hipGetLastError();
}
