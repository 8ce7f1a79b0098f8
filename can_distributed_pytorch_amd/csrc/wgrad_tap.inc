// Included by conv_wgrad.hip (inside namespace can, after the v2 kernel).
//
// Tap-ring weight gradient (cfg 12) for 3x3 layers with Cin % 64 == 0 and Cout % 128 == 0, dilation 1 or 2.
//
// The v2 kernel (wgrad_glds2) computes a 256 x 256 tile of dW[co][k] (k = tap * Cin + ci) and stages, per
// 64-pixel K step, 32 KB of dY plus 32 KB of im2col'd X: every X row is fetched once per tap.  Its LDS-DMA issue
// is what bounds it (profiles/r2/wgrad_mainloop_probe.txt: 0.95 PF/s, 1.6-1.8 PF/s with the DMA removed).
// Here a block owns 128 output channels x ALL 9 taps of a 64-channel input slice (a 128 x 576 tile: the same
// FLOPs per pixel as 256 x 288), and walks its pixels as 64-pixel stages DOWN a column: stage (n, oh, ow0..+63)
// needs input rows oh - d, oh, oh + d, which it shares with the stages above and below, so the input rows sit in
// a 6-slot LDS ring and a stage fetches ONE new row (80 pixels: 8-pixel guards both sides) beside its 16 KB of
// dY.  Per 64-pixel stage: 26 one-KiB DMA pieces for 9.4 MFLOP, against 64 pieces for 8.4 MFLOP in the v2 kernel.
//
// Chains: a column (image n, 64-column block cb) is walked as d chains (row phase p: oh = p + d t), so that the
// row ring works for dilation 2 as well (rows oh - 2, oh, oh + 2 of chain row t are chain rows t - 1, t, t + 1).
// A slice is a contiguous run of stages in (n, cb, p, t) order; it is processed as segments of one chain each,
// every segment with its own pipeline prologue (2 leading rows) and drain.
//
// Pipeline: dY stages in 4 buffers, rows in 6 ring slots, a stage's DMA issued 3 stages ahead (its pieces
// between the MFMA groups of the second K half), a counted vmcnt that leaves the stage two ahead in flight, one
// s_barrier per stage.  8 waves = 2 (64 output channels) x 4 (16 input channels x 9 taps): 36 MFMA 16x16x32 per
// wave per 32-pixel K step on 4 dY + 9 X fragments (transposed LDS reads, ds_read_b64_tr_b16).  The X fragments
// and dY fragments of the next K step are read into the registers their MFMA group just consumed (a rolling
// schedule: 144 accumulators + 4 + 9 fragments, 208 VGPRs of operands and results).
//
// TCO = 64 (Cout = 64 layers, e.g. conv1_2): 4 waves of 64 channels x (16 input channels x 9 taps), a 74 KiB
// ring (3 dY buffers, 5 row slots, DMA 2 stages ahead with a full drain) so that two blocks share a CU.
//
// Zero padding / ragged widths: all DMA goes through buffer descriptors whose range is the operand; a piece
// outside the image gets an offset beyond the range and reads zeros.  W % 8 == 0 keeps every piece wholly
// inside or outside (piece-uniform validity).

struct TapArgs {
  const bf16_t* dy;
  const bf16_t* x;
  float* ws;                 // [S][9 * Cin][Cout] fp32 partial slabs
  int N, H, W, Cin, Cout;
  int tx64;                  // 64-pixel column blocks per row
  int total;                 // stages = N * tx64 * H
  int spb;                   // stages per slice
  int S;
  unsigned dy_bytes, x_bytes;
};

// geometry of the TCO-channel tile: waves, dY buffers, row slots, DMA lead (stages), LDS bytes
// (8-wave forms of the 64-channel tile measured negative at the step: pixel-split -0.3 %, profiles/r4/ab_confirm.txt;
// 8 waves of 32 output channels, one block per CU, -0.3 % (conv1_2's weight gradient 0.669 -> 0.725 ms: 11 LDS
// fragment reads per 18 MFMAs instead of 13 per 36), profiles/r4/ab_wgrad_tap_w8.txt)
template <int TCO>
struct TapGeo {
  static constexpr int NW = (TCO == 128) ? 8 : 4;
  static constexpr bool BIG = (NW == 8);               // one block per CU, 3-stage lead
  static constexpr int JA = 4;                         // dY fragments (16 output channels each) per wave
  static constexpr int NDB = BIG ? 4 : 3;
  static constexpr int RING = BIG ? 6 : 5;
  static constexpr int LEAD = BIG ? 3 : 2;
  static constexpr int RBA = TCO * 2;                  // dY row bytes
  static constexpr int DYB = 64 * RBA;                 // one 64-pixel dY stage
  static constexpr int SLOT = 80 * 128;                // (8 | 64 | 8) pixels x 64 channels
  static constexpr int LDS = NDB * DYB + RING * SLOT;  // 124 KiB / 74 KiB
  static constexpr int XP = (10 + NW - 1) / NW;        // X row pieces per wave (at most)
  static constexpr int DPW = 64 * RBA / 1024 / NW;     // dY pieces per wave (2)
  static_assert(RING >= LEAD + 3 && NDB >= LEAD + 1, "ring / buffers too small for the lead");
};

template <int RB>
__device__ __forceinline__ unsigned tap_tr_off(int row, int c8) {   // byte offset of an 8-byte unit (swizzled)
  return (unsigned)(row * RB + swz8b<RB>(row, c8) * 8);
}

__device__ __forceinline__ frag8_t tap_tr_read(const unsigned char* base, unsigned lo, unsigned hi) {
  const s16x4 l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + lo));
  const s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + hi));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
  return __builtin_bit_cast(frag8_t, v);
}

// a wave-uniform value the optimizer cannot see through (keeps it a scalar base instead of folded into VGPRs)
__device__ __forceinline__ unsigned opaque_u32(unsigned v) {
  unsigned r;
  asm("s_mov_b32 %0, %1" : "=s"(r) : "s"(__builtin_amdgcn_readfirstlane(v)));
  return r;
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n
__device__ __forceinline__ void tap_wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

template <int DT, int D, int TCO, bool ADB>
__global__ void __launch_bounds__((TapGeo<TCO>::NW * 64), (TapGeo<TCO>::BIG ? 1 : 2)) wgrad_tap_kernel(TapArgs a) {
  using G = TapGeo<TCO>;
  constexpr int NW = G::NW, RBA = G::RBA, JA = G::JA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ring = smem + G::NDB * G::DYB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = (NW == 8) ? (wave & 1) : 0;          // half of the co tile (16 JA channels)
  const int wk = (NW == 8) ? (wave >> 1) : wave;      // 16-channel quarter of the ci tile
  const int nci = a.Cin >> 6, nco = a.Cout / TCO;
  const int ntile = nci * nco;
  const int bid = xcd_remap(blockIdx.x, ntile * a.S);
  const int tile = bid % ntile, slice = bid / ntile;       // consecutive blocks: the ci tiles of one dY tile
  const int ci0 = (tile % nci) * 64, co0 = (tile / nci) * TCO;

  const __amdgpu_buffer_rsrc_t dy_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, (short)0, a.dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);

  // DMA: dY pieces wave, wave + NW (1 KiB = 1024 / RBA pixel rows of the stage); X row pieces wave + NW * part
  // (slot pixels 8 * piece + lane / 8, 128-B rows), 10 per row.  A piece NW further keeps the swizzle (a multiple
  // of 16 rows away), so one per-lane offset serves all of a wave's pieces.
  unsigned dofs, xofs;
  {
    constexpr int RPP = 1024 / RBA, LPR = RBA / 16;   // rows per piece, lanes per row
    const int row = RPP * wave + lane / LPR;
    const int lc = swz8b<RBA>(row, (lane % LPR) * 2) >> 1;
    dofs = (unsigned)((row * a.Cout + co0 + lc * 8) * 2);
    const int xr = 8 * wave + (lane >> 3);
    const int xl = swz8b<128>(xr, (lane & 7) * 2) >> 1;
    xofs = (unsigned)((xr * a.Cin + ci0 + xl * 8) * 2);
  }
  const unsigned dstep = (unsigned)((1024 / RBA) * NW * a.Cout * 2), xstep = (unsigned)(8 * NW * a.Cin * 2);
  const int nxp = (10 - wave + NW - 1) / NW;             // X pieces this wave issues per row
  const int nst = G::DPW + nxp;                          // pieces per stage

  // fragment read offsets (kk = 0; kk = 1 is 32 rows further: +32 RBA B in a dY buffer, +4096 B in a row slot)
  const int g = lane >> 4, qd = (lane & 15) >> 2, p = lane & 3;
  // A fragment jj: c8 = 4 JA wc + 4 jj + p on disjoint bits, so its swizzled offset is fragment 0's XOR 32 jj
  const unsigned offA0 = tap_tr_off<RBA>(8 * g + qd, wc * 4 * JA + p);
  const unsigned offA1 = tap_tr_off<RBA>(8 * g + qd + 4, wc * 4 * JA + p);
  unsigned offB[3][2];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int r = 8 + (kw - 1) * D + 8 * g + qd;
    offB[kw][0] = tap_tr_off<128>(r, wk * 4 + p);
    offB[kw][1] = tap_tr_off<128>(r + 4, wk * 4 + p);
  }

  f32x4 acc[JA][9];
#pragma unroll
  for (int j = 0; j < JA; ++j)
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int per_img = a.tx64 * a.H;
  const int T0 = (a.H + D - 1) / D;                    // rows of chain phase 0
  int g0 = slice * a.spb;
  const int gend = min(a.total, g0 + a.spb);

  while (g0 < gend) {
    // the segment: stages g0 .. g0 + T - 1 of one chain (image n, column block cb, phase ph), chain rows t0 ..
    const int n = g0 / per_img;
    const int r = g0 - n * per_img;
    const int cb = r / a.H;
    const int q = r - cb * a.H;
    const int ph = (D == 2 && q >= T0) ? 1 : 0;
    const int t0 = q - ph * T0;
    const int tlen = ph ? (a.H / 2) : T0;
    const int T = min(gend - g0, tlen - t0);
    const int ow0 = cb * 64;
    const int img_row0 = n * a.H;

    auto issue_row = [&](int u, int slot, int part) {     // chain row u into ring slot, this wave's piece `part`
      if (part >= nxp) return;
      const int ih = ph + D * u;
      const int pc = wave + NW * part;                      // piece: slot pixels 8 pc .. 8 pc + 7
      const int iw0 = ow0 - 8 + 8 * pc;
      const bool ok = (unsigned)ih < (unsigned)a.H && iw0 >= 0 && iw0 < a.W;      // piece-uniform (W % 8 == 0)
      // byte offset of slot pixel 0 (wraps below 0 only when !ok: unsigned arithmetic)
      const unsigned base = (unsigned)((img_row0 + ih) * a.W + ow0 - 8) * (unsigned)(a.Cin * 2);
      const unsigned off = ok ? base + xofs + (unsigned)part * xstep : 0xFFFFFFF0u;
      blds16(x_rsrc, off, 0u, lds_addr(ring + slot * G::SLOT + pc * 1024));
    };
    auto issue_dy = [&](int j, int part) {                  // dY of stage j, piece wave + NW * part
      const int oh = ph + D * (t0 + j);
      const int ow = ow0 + (1024 / RBA) * (wave + NW * part);
      const int m0 = (img_row0 + oh) * a.W + ow0;
      const unsigned off = (ow < a.W) ? (unsigned)(m0 * a.Cout * 2) + dofs + (unsigned)part * dstep : 0xFFFFFFF0u;
      blds16(dy_rsrc, off, 0u, lds_addr(smem + (j % G::NDB) * G::DYB + (wave + NW * part) * 1024));
    };
    // stage j's pieces: dY DPW, the chain row t0 + j + 1 (its first reader is stage j) 1 .. XP
    auto issue_part = [&](int j, int k) {
      if (k < G::DPW) issue_dy(j, k);
      else issue_row(t0 + j + 1, (j + 2) % G::RING, k - G::DPW);
    };
    auto rdA = [&](int j, int kk, frag8_t (&dst)[JA]) {
      const unsigned char* b = smem + (j % G::NDB) * G::DYB + kk * 32 * RBA;
#pragma unroll
      for (int jj = 0; jj < JA; ++jj) dst[jj] = tap_tr_read(b, offA0 ^ (jj * 32), offA1 ^ (jj * 32));
    };
    // the ring slots of stage j's rows kh = 0, 1, 2 as opaque scalars: folded into the per-lane offsets, the nine
    // (kh, kw) combinations each took their own VGPR (18 offsets instead of 6, and spills)
    auto slots = [&](int j, unsigned (&sb)[3]) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) sb[kh] = opaque_u32((unsigned)(((j + kh) % G::RING) * G::SLOT));
    };
    auto rdB = [&](const unsigned (&sb)[3], int kk, int i) -> frag8_t {     // tap i = 3 kh + kw
      const int kh = i / 3, kw = i - 3 * kh;
      const unsigned char* b = ring + sb[kh] + kk * 4096;
      return tap_tr_read(b, offB[kw][0], offB[kw][1]);
    };

    // prologue: chain rows t0 - 1, t0 (slots 0, 1), stages 0 .. LEAD - 1, then stage 0 (and the rows) landed
#pragma unroll
    for (int k = 0; k < G::XP; ++k) {
      issue_row(t0 - 1, 0, k);
      issue_row(t0, 1, k);
    }
    for (int s = 0; s < G::LEAD && s < T; ++s)
#pragma unroll
      for (int k = 0; k < G::DPW + G::XP; ++k) issue_part(s, k);
    tap_wait_vm(nst * max(0, min(T, G::LEAD) - 1));
    asm volatile("s_barrier" ::: "memory");

    // one K step (32 pixels): the 36 MFMAs of (A, B) with the next step's fragments (stage rs, half rkk) read into
    // the registers each MFMA group has just consumed (B[i] after group i) and, when dma, the DMA pieces of stage
    // rs - 1 + LEAD after groups 0 ..
    frag8_t A0[JA], A1[JA], B[9];
    // ADB = 0: one dY fragment set, the next step's read after its last use (after the MFMA with B[8]); ADB = 1:
    // two sets, the next step's read at the start of this one (its latency hidden behind 36 MFMAs; +16 VGPRs)
    auto kstep = [&](frag8_t (&A)[JA], frag8_t (&An)[JA], bool next, int rs, int rkk, bool dma) {
      unsigned sb[3];
      slots(rs, sb);
      const unsigned char* ab = smem + (rs % G::NDB) * G::DYB + rkk * 32 * RBA;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int jj = 0; jj < JA; ++jj) acc[jj][i] = mfma16<DT>(A[jj], B[i], acc[jj][i]);
        __builtin_amdgcn_sched_barrier(0);
        if (next) B[i] = rdB(sb, rkk, i);
        if constexpr (ADB) {
          if (next && i < JA) An[i] = tap_tr_read(ab, offA0 ^ (i * 32), offA1 ^ (i * 32));
        }
        // TCO 128 (4 parts): after groups 1, 3, 5, 7; TCO 64 (up to 5): after groups 0, 2, 4, 6, 7
        if constexpr (G::BIG) {
          if (dma && (i & 1)) issue_part(rs - 1 + G::LEAD, i >> 1);
        } else {
          if (dma && ((i & 1) == 0 || i == 7)) issue_part(rs - 1 + G::LEAD, (i == 7) ? 4 : (i >> 1));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int jj = 0; jj < JA; ++jj) {
        acc[jj][8] = mfma16<DT>(A[jj], B[8], acc[jj][8]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!ADB) {
          if (next) A[jj] = tap_tr_read(ab, offA0 ^ (jj * 32), offA1 ^ (jj * 32));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (next) B[8] = rdB(sb, rkk, 8);
      __builtin_amdgcn_sched_barrier(0);
    };

    rdA(0, 0, A0);
    {
      unsigned sb[3];
      slots(0, sb);
#pragma unroll
      for (int i = 0; i < 9; ++i) B[i] = rdB(sb, 0, i);
    }

    for (int j = 0; j < T; ++j) {
      // first K half of stage j; reads its second half
      if constexpr (ADB) kstep(A0, A1, true, j, 1, false);
      else kstep(A0, A0, true, j, 1, false);
      const bool more = j + 1 < T;
      if (more) {
        // this wave's reads of stage j are done, its DMA of stage j + 1 retired (LEAD 3: stage j + 2 may stay in
        // flight); after the barrier every wave's is, and no wave still reads the buffers stage j + LEAD overwrites
        tap_wait_vm((G::LEAD == 3 && j + 2 < T) ? nst : 0);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      // second K half of stage j; reads stage j + 1's first half, issues stage j + LEAD
      if constexpr (ADB) kstep(A1, A0, more, j + 1, 0, j + G::LEAD < T);
      else kstep(A0, A0, more, j + 1, 0, j + G::LEAD < T);
    }
    // every wave done with the buffers before the next segment's prologue refills them
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("s_barrier" ::: "memory");
    g0 += T;
  }

  // dW partial slab of this slice: acc[j][i] = rows co0 + 64 wc + 16 j + 4 fq .. + 3, column k = tap i of input
  // channel ci0 + 16 wk + fr
  const int fr = lane & 15, fq = lane >> 4;
  const int Ktot = 9 * a.Cin;
  float* slab = a.ws + (size_t)slice * Ktot * a.Cout;
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = 0; j < JA; ++j) {
      const int k = i * a.Cin + ci0 + wk * 16 + fr;
      const int co = co0 + wc * 16 * JA + j * 16 + fq * 4;
      *reinterpret_cast<f32x4*>(slab + (size_t)k * a.Cout + co) = acc[j][i];
    }
}

template <int DT, int D, int TCO, bool ADB>
static int launch_wgrad_tap(const TapArgs& a, hipStream_t s) {
  using G = TapGeo<TCO>;
  auto kfn = wgrad_tap_kernel<DT, D, TCO, ADB>;
  static bool attr = false;
  if (!attr) {
    CAN_HIP_CHECK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS));
    attr = true;
  }
  const int ntile = (a.Cin / 64) * (a.Cout / TCO);
  hipLaunchKernelGGL(kfn, dim3(ntile * a.S), dim3(G::NW * 64), G::LDS, s, a);
  return (int)hipGetLastError();
}
// (the shapes the kernel takes: wgrad_tap_ok / wgrad_tap_tco in wgrad_plan.h)
