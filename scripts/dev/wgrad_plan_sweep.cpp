// Sweeps the weight-gradient planner (csrc/wgrad_plan.h: host-only C++) under the sanitizers.  Reads layer shapes
// "N H W Cin Cout ksize dil first" from stdin (the fixture's grid), plans each under dispatch wgrad_tap 0-3, the width
// given / unknown, every bias mode and several CU counts, adds degenerate inputs (one pixel, W = 8, slice-count clamps,
// refused shapes, extreme target_blocks) and checks the plan's invariants.  Prints the number of plans made.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ican_distributed_pytorch_amd/csrc scripts/dev/wgrad_plan_sweep.cpp -o /tmp/wgrad_plan_sweep
//   python -c "import json; [print(*r[:8]) for r in json.load(open('tests/golden/wgrad_plan_parent.json'))['rows']]" \
//       | /tmp/wgrad_plan_sweep
#include "wgrad_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace can;

#define CHECK(c)                                                                                     \
  do {                                                                                               \
    if (!(c)) {                                                                                      \
      std::fprintf(stderr, "%s:%d: %s failed (N %d H %d W %d M %d Cin %d Cout %d k %d dil %d first %d)\n", __FILE__, \
                   __LINE__, #c, q.N, q.H, q.W, q.M, q.Cin, q.Cout, q.ksize, q.dil, q.first);        \
      std::exit(1);                                                                                  \
    }                                                                                                \
  } while (0)

static long g_plans = 0;

static void check(const WgradQuery& q, const DispatchConfig& d, int ncu) {
  const WgradPlan p = plan_wgrad(q, d, ncu);
  ++g_plans;
  if (p.err) {
    CHECK(p.err == -2 || p.err == -3 || p.err == -9 || p.err == -15);
    return;
  }
  const WgradTile* t = find_wgrad_tile(p.cfg);
  const long long K = q.first ? 64 : (long long)q.ksize * q.ksize * q.Cin;
  CHECK(t && p.S >= 1 && p.ntile >= 1 && p.blocks == p.ntile * p.S);
  if (p.fam == WG_FIRST || p.fam == WG_GLDS || p.fam == WG_GLDS2) {
    CHECK((long long)p.S * p.mslice >= q.M && p.mslice % t->BKM == 0);
    CHECK(p.fam != WG_GLDS2 || ((long long)p.S * p.vmslice >= p.vM && p.vM >= q.M && p.vmslice % 64 == 0));
  }
  CHECK(p.fam != WG_TAP || (p.S <= p.tap_total && (long long)p.S * p.tap_spb >= p.tap_total));
  CHECK(p.fam != WG_HALO || q.W == 0 || (long long)p.S * p.halo_tps >= p.halo_tiles);
  CHECK(p.Sb_ext <= kBiasParts && p.Sb <= std::max(p.S, kBiasParts));
  CHECK(p.bias_off == p.S * K * q.Cout && p.ws_floats == p.bias_off + (long long)std::max(p.S, kBiasParts) * q.Cout);
  CHECK(p.reduce == wgrad_reduce_kind(p.S, (int)K, q.Cout, q.first ? 4 : q.Cin, q.ksize * q.ksize, q.first));
}

static void sweep(WgradQuery q) {
  const int W = q.W;
  for (int tap = 0; tap <= 3; ++tap)
    for (int ncu : {0, 1, 64, 256, 304})
      for (int wq : {W, 0})
        for (int rows : {-1, 0, 1, 512, 513, 100000}) {
          DispatchConfig d;
          d.wgrad_tap = tap;
          q.W = wq;
          q.want_db = rows >= 0;
          q.bext_rows = std::max(rows, 0);
          check(q, d, ncu);
        }
}

int main() {
  std::vector<WgradQuery> qs;
  WgradQuery q;
  while (std::scanf("%d %d %d %d %d %d %d %d", &q.N, &q.H, &q.W, &q.Cin, &q.Cout, &q.ksize, &q.dil, &q.first) == 8) {
    q.M = q.N * q.H * q.W;
    qs.push_back(q);
  }
  for (const WgradQuery& r : qs) sweep(r);
  // degenerate inputs: tiny and empty maps, W = 8, odd channels, huge layers, extreme target_blocks
  for (int first : {0, 1})
    for (int ksize : {1, 3})
      for (int dil : {1, 2})
        for (int H : {0, 1, 2, 3})
          for (int W : {0, 1, 2, 8, 63, 64, 65})
            for (int Cin : {0, 3, 4, 64, 96, 128, 256, 36864})
              for (int Cout : {0, 32, 64, 128, 256, 2048, 4096, 8192})
                for (int tb : {0, 1, 1024, 1 << 30}) {
                  WgradQuery r;
                  r.N = 1; r.H = H; r.W = W; r.M = H * W; r.Cin = Cin; r.Cout = Cout; r.ksize = ksize; r.dil = dil;
                  r.first = first; r.target_blocks = tb;
                  sweep(r);
                }
  // the largest maps one launch takes (32-bit operand addressing: the front end chunks above it)
  for (int Cout : {64, 128, 256, 512}) {
    WgradQuery r;
    r.N = 16; r.H = 1024; r.W = (1 << 30) / (16 * 1024) / Cout; r.M = r.N * r.H * r.W; r.Cin = 64; r.Cout = Cout;
    sweep(r);
  }
  long batched = 0;
  for (int M : {0, 1, 64, 3072, 3040, 98304, 1 << 21})
    for (int W : {0, 64, 96, 128})
      for (int C : {0, 128, 256, 512, 1024})
        for (int nb : {0, 1, 4, 65535})
          for (int ncu : {0, 1, 224, 256}) {
            const WgradBatchedPlan p = plan_wgrad_1x1_batched(M, W, C, 512, nb, ncu);
            ++batched;
            if (p.S == 0) {
              if (p.err != -3) return 2;
              continue;
            }
            if ((long long)p.S * p.mslice < M || p.mslice % 64 || p.ws_floats != (long long)nb * p.S * C * 512) return 3;
          }
  std::printf("%ld plans, %ld batched plans: ok\n", g_plans, batched);
  return 0;
}
