// Stand-alone host check of csrc/awq_linear_route.hpp (tests/test_linear_route_host.py builds it with the host compiler and
// -fsanitize=address,undefined): walks the six entries x the row counts and shapes of tests/linear_route_cases.py (and the rows around them) x every
// combination of the flags, at the default knobs and at every knob block the suite sets, for 256, 304 and 64 CUs, and asserts what the entries rely on
// when they switch on a route without falling through: every call in range gets exactly one leaf, that leaf's own predicate -- the guard of its
// launcher -- accepts the call as the entry will make it, and the workspace, the bias and the scale format are handed on where the leaf takes them.
#include <stdio.h>

#include <initializer_list>

#include "awq_decode_plan.hpp"
#include "awq_linear_route.hpp"

using namespace awq;

static long long g_points = 0, g_bad = 0;

static void fail(const char* what, int entry, int m, int n, int k, int flags, int cus, const LinearRoute& r) {
  if (g_bad++ < 20) printf("FAIL %s: entry %d m %d n %d k %d flags %d cus %d -> leaf %d row %d\n", what, entry, m, n, k, flags, cus, r.leaf, r.row);
}

static void walk(const LinearKnobs& kn, int cus) {
  const int rows[] = {1, 2, 4, 5, 8, 9, 12, 16, 17, 32, 33, 48, 49, 64, 65, 71, 72, 100, 128, 129, 150, 192, 193, 200, 255, 256, 300, 1024, 2048, 4096};
  const int slabs[] = {1, 2, 3, 48, 192, 256, 384, 511, 512, 513, 639, 640, 768, 1023, 1024, 1025, 1376, 1792, 1793, 3584};
  const int nits[] = {1, 2, 6, 24, 31, 32, 64, 86, 96, 112, 191, 192, 224};
  for (int entry = kEntryForward; entry <= kEntryPartial; ++entry)
    for (int m : rows)
      for (int sl : slabs)
        for (int nit : nits)
          for (int flags = 0; flags < 32; ++flags) {
            const int n = 16 * sl, k = 128 * nit;
            const bool szp = flags & kHasSzPacked, szh = flags & kHasSzHalf, bias = flags & kHasBias, ws = flags & kHasWs;
            if ((entry == kEntryGemv && m > 16) || ((entry == kEntryGateUp || entry == kEntryPartial) && !szp)) continue;   // the entry refuses these itself
            const LinearRoute r = linear_route(entry, m, n, k, flags, cus, kn);
            ++g_points;
            if (r.leaf < kLeafDecode || r.leaf > kLeafGeneric || r.row < 1) {
              fail("exactly one leaf", entry, m, n, k, flags, cus, r);
              continue;
            }
            const LinearRoute again = linear_route(entry, m, n, k, flags, cus, kn);
            if (again.leaf != r.leaf || again.row != r.row) fail("the route is a function of its arguments", entry, m, n, k, flags, cus, r);
            // the call the entry makes
            const bool fwd = entry == kEntryForward || entry == kEntryForwardSzh, fused = r.bias == kBiasFused, f32 = r.epilogue == kEpiPartial;
            const int epi = r.epilogue == kEpiPair ? 2 : 0;
            if (r.epilogue != (entry == kEntryGateUp ? kEpiPair : (entry == kEntryPartial ? kEpiPartial : kEpiPlain))) fail("the entry's epilogue", entry, m, n, k, flags, cus, r);
            if ((fwd && bias) != (r.bias != kBiasNone)) fail("a bias is added exactly when the call has one", entry, m, n, k, flags, cus, r);
            if (r.bias == kBiasAdd && r.leaf != kLeafGeneric && r.leaf != kLeafSkinny && r.leaf != kLeafDecode && r.leaf != kLeafGemvRing) fail("bias-add behind a leaf of the plain GEMM rows", entry, m, n, k, flags, cus, r);
            if (fused && (r.leaf == kLeafGeneric || r.leaf == kLeafSkinnyGateUp)) fail("a fused bias on a leaf that takes none", entry, m, n, k, flags, cus, r);
            if (r.bias_align16 && !(r.leaf == kLeafMidm || r.leaf == kLeafTiles || r.leaf == kLeafSkinny16)) fail("bias_align16 on a leaf that reads bias by elements", entry, m, n, k, flags, cus, r);
            if (r.szfmt != 0 && !(szh && entry != kEntryForward && entry != kEntryGemm && entry != kEntryGemv)) fail("sz_half only where the call has it", entry, m, n, k, flags, cus, r);
            if (r.szfmt != 0 && !(r.leaf == kLeafDecode || r.leaf == kLeafMidm || r.leaf == kLeafSkinny16 || r.leaf == kLeafTiles)) fail("sz_half on a leaf with that dequant form", entry, m, n, k, flags, cus, r);
            if (r.leaf != kLeafGeneric && !szp) fail("a cdna4 kernel without sz_packed", entry, m, n, k, flags, cus, r);
            // the leaf's predicate = the guard of its launcher
            bool ok = false;
            switch (r.leaf) {
              case kLeafDecode: ok = decode_serves(m, n, k, epi, true, fused, f32, cus, kn) && (entry >= kEntryGateUp || kn.gemv_dma); break;
              case kLeafGemvRing: ok = gemv_ring_serves(m, n, k, 0) && !(kn.gemv_dma && decode_serves(m, n, k, 0, true, fused, false, cus, kn)); break;
              case kLeafMidm: ok = midm_serves(m, n, k, epi, fused, f32, 4, cus, kn); break;
              case kLeafSkinny16: ok = skinny16_serves(m, n, k, epi, fused, f32); break;
              case kLeafSkinny: ok = skinny_serves(m, n, k, fused, f32); break;
              case kLeafSkinnyGateUp: ok = skinny_gate_up_serves(m, n, k); break;
              case kLeafTiles: ok = tiles_serve(m, n, k, 4, r.epilogue == kEpiPair ? 2 : (f32 ? 3 : 0), true, kn); break;
              case kLeafGeneric: ok = entry <= kEntryGemv; break;   // launch_gemm / launch_gemv serve every shape check_common lets through
            }
            if (!ok) fail("the leaf's predicate accepts the call", entry, m, n, k, flags, cus, r);
            // the workspace: handed on to every leaf that can use one, as the caller gave it; the gate/up entry's tile row only with one that passed its test
            const bool takes_ws = (r.leaf == kLeafMidm || r.leaf == kLeafSkinny || r.leaf == kLeafTiles || r.leaf == kLeafGeneric) && entry != kEntryGemv && entry != kEntryPartial;
            const bool want_ws = ws && takes_ws && !(entry == kEntryGateUp && r.leaf == kLeafTiles && !(flags & kWsTiles));
            if (r.ws != want_ws) fail("the workspace is handed on where the leaf asks for it", entry, m, n, k, flags, cus, r);
          }
}

int main() {
  for (int cus : {256, 304, 64}) {
    LinearKnobs kn;
    walk(kn, cus);
    kn.midm = 0;
    walk(kn, cus);
    kn.mlp_skinny_max = 8;
    walk(kn, cus);
    kn = LinearKnobs{};
    kn.midm_min = 9, kn.midm_max = 255;
    walk(kn, cus);
    kn = LinearKnobs{};
    kn.midm_max = 192;
    walk(kn, cus);
    for (int small_m : {0, 2}) {
      kn = LinearKnobs{};
      kn.gemm_small_m = small_m;
      walk(kn, cus);
    }
    for (int v = 1; v <= 5; ++v) {
      kn = LinearKnobs{};
      kn.gemm_variant = v;
      walk(kn, cus);
    }
    kn = LinearKnobs{};
    kn.skinny16_szh = 0;
    walk(kn, cus);
    kn = LinearKnobs{};
    kn.gemv_dma = 0;
    walk(kn, cus);
    kn = LinearKnobs{};
    kn.gemm_v4 = 0;
    walk(kn, cus);
  }
  printf("%lld points, %lld failures\n", g_points, g_bad);
  return g_bad != 0;
}
