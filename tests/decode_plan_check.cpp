// Stand-alone host check of csrc/awq_decode_plan.hpp (tests/test_decode_plan_host.py builds it with the host compiler and
// -fsanitize=address,undefined): walks epilogue 0 - 2 x 1 - 8 rows x 1 - 4200 slabs x k-steps 1 - 129, 224, 256, 448 at the default knobs
// and with every forced setting the suite uses, and asserts what launch_gemv_dma relies on when it walks a plan.  An argument S > 1 thins the
// slab counts to the multiples of S, the first sixteen and the three around every multiple of 128 (where the classes of 256 CUs change).
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "awq_decode_plan.hpp"

using namespace awq;

static long long g_points = 0, g_chunks = 0, g_bad = 0;
static int g_stride = 1;

static void fail(const char* what, int epi, int m, int slabs, int nit, int chunk) {
  if (g_bad++ < 20) printf("FAIL %s: epilogue %d m %d slabs %d k-steps %d chunk %d\n", what, epi, m, slabs, nit, chunk);
}

static bool compiled_pair(int waves, int d) {
  if (waves == 8) return d == 1 || d == 2 || d == 4 || d == 8;
  if (waves == 16) return d == 1 || d == 2 || d == 4 || d == 7;
  if (waves == 4) return d == 1 || d == 2 || d == 4 || d == 7 || d == 8;
  return false;
}

static void walk(const DecodeKnobs& kn, int cus) {
  for (int epi = 0; epi <= 2; ++epi)
    for (int m = 1; m <= 8; ++m)
      for (int slabs = 1; slabs <= 4200; ++slabs) {
        if (slabs % g_stride != 0 && slabs > 16 && (slabs + 1) % 128 > 2) continue;
        for (int i = 1; i <= 132; ++i) {
          const int nit = i <= 129 ? i : (i == 130 ? 224 : (i == 131 ? 256 : 448));
          const DecodePlan p = decode_plan(m, (epi == 1 ? 32 : 16) * slabs, nit * 128, epi, cus, kn);
          ++g_points;
          if (!p.in_range) fail("in range", epi, m, slabs, nit, -1);
          if (!p.served) {
            if (p.nchunks != 0) fail("unserved plan has chunks", epi, m, slabs, nit, -1);
            continue;
          }
          int rows = 0;
          bool any_skinny = false;
          for (int c = 0; c < p.nchunks; ++c) {
            const DecodeChunk& ch = p.chunk[c];
            ++g_chunks;
            rows += ch.rows;
            if (ch.rows < 1) fail("rows >= 1", epi, m, slabs, nit, c);
            if (ch.kernel == kDecodeSkinny) {
              any_skinny = true;
              if (epi == 1) fail("no skinny chunk for the stacked epilogue", epi, m, slabs, nit, c);
              if (ch.shape < 0 || ch.shape > 3 || ch.x_pieces != (ch.rows <= 4 ? 1 : 2)) fail("skinny shape / pieces", epi, m, slabs, nit, c);
              continue;
            }
            if (ch.kernel != kDecodeStreaming) fail("kernel", epi, m, slabs, nit, c);
            if (ch.tx < ch.d || ch.d < 1) fail("tx >= d >= 1", epi, m, slabs, nit, c);
            if (ch.waves * ch.tx < nit) fail("the waves cover K", epi, m, slabs, nit, c);
            if (ch.smem_bytes <= 0 || ch.smem_bytes > 160 * 1024) fail("smem <= 160 KiB", epi, m, slabs, nit, c);
            if (ch.smem_bytes != streaming_smem(ch.waves, ch.d, epi == 1 ? 2 : 1, ch.tx, ch.rows)) fail("smem is the configuration's", epi, m, slabs, nit, c);
            if (!compiled_pair(ch.waves, ch.d)) fail("(waves, d) is compiled", epi, m, slabs, nit, c);
            if (ch.one_row_form && !(ch.rows == 1 && nit == ch.waves * ch.tx && one_row_tx(epi, ch.waves, ch.d) == ch.tx)) fail("one-row form", epi, m, slabs, nit, c);
          }
          if (rows != m) fail("chunk rows sum to m", epi, m, slabs, nit, -1);
          if (p.nchunks > 1 && any_skinny) fail("a chunked call stays on the streaming kernel (what the one-kernel query answers)", epi, m, slabs, nit, -1);
        }
      }
}

int main(int argc, char** argv) {
  const int cus = 256;
  if (argc > 1 && atoi(argv[1]) > 1) g_stride = atoi(argv[1]);
  DecodeKnobs kn;
  walk(kn, cus);
  for (int from : {1, 9}) {
    kn = DecodeKnobs{};
    kn.skinny_from = from;
    walk(kn, cus);
  }
  for (int il : {0, 1}) {
    kn = DecodeKnobs{};
    kn.il = il;
    walk(kn, cus);
  }
  const int wd[8][2] = {{4, 4}, {8, 1}, {8, 2}, {8, 4}, {8, 8}, {16, 1}, {16, 2}, {16, 4}};
  for (const auto& p : wd) {
    kn = DecodeKnobs{};
    kn.skinny_from = 9;
    kn.waves = p[0];
    kn.d = p[1];
    walk(kn, cus);
  }
  // out of range: no plan, nothing served
  const int bad[][4] = {{0, 4096, 4096, 0}, {9, 4096, 4096, 0}, {4, 4100, 4096, 0}, {4, 4096, 4000, 0}, {4, 4096, 0, 0}, {4, 0, 4096, 0}, {4, 4112, 4096, 1}, {4, 4096, 4096, 3}, {4, 4096, 4096, -1}};
  for (const auto& b : bad) {
    const DecodePlan p = decode_plan(b[0], b[1], b[2], b[3], cus, DecodeKnobs{});
    if (p.in_range || p.served || p.nchunks != 0) fail("out of range", b[3], b[0], b[1], b[2], -1);
  }
  // the largest arguments an int holds: no overflow on the way to "not served"
  (void)decode_plan(8, 2147483632, 2147483520, 0, cus, DecodeKnobs{});
  (void)decode_plan(8, 2147483616, 2147483520, 1, cus, DecodeKnobs{});
  printf("%lld points, %lld chunks, %lld failures\n", g_points, g_chunks, g_bad);
  return g_bad != 0;
}
