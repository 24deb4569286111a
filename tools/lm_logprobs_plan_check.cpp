// Host-side check of the launcher arithmetic of awq_lm_logprobs_cdna4.hip: the plan and the workspace size over the shapes the tests and the benchmark
// use, and over the edges of the accepted range, re-derived here in 64-bit integers.  A stand-alone program for a sanitizer build on the CPU (no GPU
// call is made: only awq::lm_logprobs_plan and awq::lm_logprobs_workspace_bytes run):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I llm_awq_amd/csrc -I include tools/lm_logprobs_plan_check.cpp llm_awq_amd/csrc/awq_lm_logprobs_cdna4.hip -o build/lm_logprobs_plan_check
//   ASAN_OPTIONS=detect_leaks=0 build/lm_logprobs_plan_check          (build/ is git-ignored)
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

namespace awq {
int lm_logprobs_plan(int t, int v, int k, int out[4]);
size_t lm_logprobs_workspace_bytes(int t, int v, int k, int with_gamma);
// the norm launch lives in another translation unit; this program never launches
int launch_rmsnorm(const void*, const void*, float, void*, int, int, int, hipStream_t) { return -1; }
}  // namespace awq

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

int main() {
  int probe[4] = {0, 0, 0, 0};
  CHECK(awq::lm_logprobs_plan(1, 1, 8, probe) == 0);
  const int64_t rt = probe[0], vt = probe[1];
  CHECK(rt > 0 && vt > 0 && probe[2] == 1 && probe[3] == 64);
  const int ts[] = {1, 2, (int)rt - 1, (int)rt, (int)rt + 1, 2 * (int)rt + 5, 130, 300, 2047, 1 << 20, 2147483647};
  const int vs[] = {1, 17, (int)vt - 1, (int)vt, (int)vt + 1, 2 * (int)vt + 17, 513, 2000, 32000, 128256, 132000, 1 << 20, 1 << 30};
  const int ks[] = {8, 40, 72, 136, 1032, 4096, 8192, 8200, 1 << 20};
  long long accepted = 0, refused = 0;
  for (int t : ts)
    for (int v : vs)
      for (int k : ks) {
        int plan[4] = {-1, -1, -1, -1};
        const int64_t ntr = ((int64_t)t + rt - 1) / rt, ntv = ((int64_t)v + vt - 1) / vt;
        const bool fits = ntr * ntv <= 2147483647LL;
        const int rc = awq::lm_logprobs_plan(t, v, k, plan);
        CHECK((rc == 0) == fits);
        for (int g = 0; g < 2; ++g) {
          const uint64_t got = awq::lm_logprobs_workspace_bytes(t, v, k, g);
          if (!fits) {
            CHECK(got == 0);
            continue;
          }
          const uint64_t want = (g ? up256((uint64_t)t * (uint64_t)k * 2) : 0) + 3 * up256((uint64_t)(ntr * ntv) * (uint64_t)rt * 4) + up256((uint64_t)ntr * (uint64_t)rt * 4);
          CHECK(got == want);
        }
        if (fits) {
          CHECK(plan[0] == rt && plan[1] == vt && plan[2] == (int)(ntr * ntv) && plan[3] == 64);
          ++accepted;
        } else {
          ++refused;
        }
      }
  const int bad[][3] = {{0, 10, 8}, {-1, 10, 8}, {1, 0, 8}, {1, -5, 8}, {1, (1 << 30) + 1, 8}, {1, 10, 0}, {1, 10, 4}, {1, 10, 12}, {1, 10, -8}};
  for (const auto& b : bad) {
    int plan[4];
    CHECK(awq::lm_logprobs_plan(b[0], b[1], b[2], plan) != 0);
    CHECK(awq::lm_logprobs_workspace_bytes(b[0], b[1], b[2], 1) == 0);
  }
  std::printf("lm_logprobs_plan_check: %lld shapes accepted, %lld refused, %d failures\n", accepted, refused, fails);
  return fails ? 1 : 0;
}
