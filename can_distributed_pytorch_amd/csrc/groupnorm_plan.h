// Launch plan of the NHWC group / instance normalisation kernels (groupnorm.hip).  Pure functions of the problem shape
// and the CU count, host only, no HIP calls.
//
// Two forms.  Streamed (any size): statistics -> finalize -> apply over a grid of (channel span, pixel slice, sample),
// double partials part [N][S][2][C].  Resident (small per-sample maps): one kernel per direction; a block owns one sample
// and a channel bundle and keeps its [H W][bundle] tile (two tiles in backward: x and the masked dy) in LDS.
#pragma once

namespace can {

enum { GN_AUTO = 0, GN_STREAMED = 1, GN_RESIDENT = 2 };

constexpr int GN_THREADS = 256;               // streamed kernels and the finalize
constexpr int GN_MAX_TX = 32;                 // octets of a channel span: 256 channels
constexpr int GN_RES_THREADS = 512;           // resident kernels: a block is alone on its CU when its tile is large
constexpr int GN_RES_MAX_BX = 64;             // octets of a bundle: 512 channels
constexpr int GN_RES_MIN_RUN = 32;            // channels: a pixel of a bundle is a run of at least 64 bytes where C allows
constexpr long long GN_LDS_BYTES = 160 * 1024;
constexpr int GN_MAX_DIM = 65535;             // samples and slices are grid dimensions

// LDS of a resident block beside its tile(s), in bytes: the reduction's rows red [8][T + BX] and chunk sums red2 [T]
// (doubles), the channel sums cs [2][8 BX] (doubles) and four fp32 vectors of 8 BX (per-channel or per-group values)
inline long long gn_res_scratch(int BX) {
  return 8ll * (8 * (GN_RES_THREADS + BX) + GN_RES_THREADS + 16 * BX) + 4ll * 32 * BX;
}

struct GnPlan {
  int err, form, S;
  int spans, tymin;             // streamed: channel spans of <= 32 octets, pixel rows per block of the widest span
  int bundle;                   // resident: channels of a bundle (0: the resident form cannot serve the shape)
  long long lds;                // resident: dynamic LDS of a block (tiles + scratch)
};

inline long long gn_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// -2 C or G, -3 a group of fewer than two values, -5 a map beyond the indexing (64-bit pixel offsets; the sample and
// slice counts are grid dimensions), -6 a form or slice count out of range, -8 a forced resident form that does not fit.
// backward: two tiles per block.  form: GN_AUTO plans (resident when the tiles fit the LDS), slices: 0 plans.
inline GnPlan gn_plan(long long N, long long H, long long W, long long C, long long G, int backward, int form,
                      int slices, int cus) {
  GnPlan p{0, GN_STREAMED, 1, 0, 0, 0, 0};
  if (C <= 0 || (C & 7) || C > (1 << 24) || G <= 0 || C % G) { p.err = -2; return p; }
  if (N < 1 || H < 1 || W < 1 || N > GN_MAX_DIM || H > (1ll << 31) || W > (1ll << 31)) { p.err = -5; return p; }
  const long long HW = H * W, cg = C / G;
  if (HW > (1ll << 48) / C || N * HW > (1ll << 48) / C) { p.err = -5; return p; }
  if (HW * cg < 2) { p.err = -3; return p; }
  if (form < GN_AUTO || form > GN_RESIDENT || slices < 0 || slices > GN_MAX_DIM) { p.err = -6; return p; }
  const int C8 = (int)(C / 8), ncu = cus > 0 ? cus : 256;
  // resident: the bundle is the smallest whole number of groups and of octets that is a 64-byte run
  const long long L = cg / gn_gcd(cg, 8) * 8;
  if (L <= 8 * GN_RES_MAX_BX) {
    long long B = (GN_RES_MIN_RUN + L - 1) / L * L;
    if (B > C) B = C;
    const long long lds = HW * B * 2 * (backward ? 2 : 1) + gn_res_scratch((int)(B / 8));
    if (HW <= (1 << 20) && lds <= GN_LDS_BYTES) { p.bundle = (int)B; p.lds = lds; }
  }
  if (form == GN_RESIDENT && !p.bundle) { p.err = -8; return p; }
  if (form == GN_RESIDENT || (form == GN_AUTO && p.bundle)) { p.form = GN_RESIDENT; return p; }
  // streamed: N x spans x S blocks fill the CUs four times, fewer where a slice would get under 16 rows per thread
  p.spans = (C8 + GN_MAX_TX - 1) / GN_MAX_TX;
  p.tymin = GN_THREADS / ((C8 + p.spans - 1) / p.spans);
  long long S = slices;
  if (S == 0) {
    S = (4ll * ncu) / (N * p.spans);
    const long long cap = HW / (16ll * p.tymin);
    if (S > cap) S = cap;
    if (S > GN_MAX_DIM) S = GN_MAX_DIM;
    if (S < 1) S = 1;
  }
  p.S = (int)S;
  return p;
}

// blockIdx.y of the streamed apply passes: eight blocks per CU over all samples and spans, no more than the rows need
inline int gn_apply_rows(long long N, long long HW, const GnPlan& p, int cus) {
  long long gy = (8ll * (cus > 0 ? cus : 256)) / (N * p.spans), need = (HW + p.tymin - 1) / p.tymin;
  if (gy > need) gy = need;
  if (gy > GN_MAX_DIM) gy = GN_MAX_DIM;
  return gy < 1 ? 1 : (int)gy;
}

}  // namespace can
