// Next-token sampling on the device (gfx950, wave64): logits [B, V] -> tokens [B] in ONE launch, every parameter a per-row device tensor, no
// host read (DESIGN.md "Sampling" states the contract by values; tests/sample_oracle.py restates it in numpy).
//
// One block of 1024 threads per row.  The row routine -- the max, select, sum and find passes over a row that does not fit LDS, with
// fixed-point masses that make the launch bit-stable -- is awq_sample_row.hpp, which the packed verifier of a speculative step
// (awq_spec_cdna4.hip) runs as well; this file is the per-slot frame around it: the slot's parameters, the history's bitmap and step 9.
// No global atomics, no workspace; the only global stores are thread 0's results of the row.
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_sample_row.hpp"

namespace awq {
namespace {

using namespace sample_row;

struct SampleArgs {
  const void* logits;
  const float* u;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const float* penalty;
  int* history;
  int* hist_len;
  int* seqlens;
  const int* stop_ids;
  int* finished;
  int* tokens;
  int vocab, max_history, num_stop, max_len, flags;
};

template <int LT>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // the history's presence bitmap: V bits (only launches with a history have it)

  const int b = blockIdx.x, tid = threadIdx.x, V = a.vocab;
  const int seq = a.seqlens ? a.seqlens[b] : 0;
  if (seq < 0) {  // inactive slot: nothing else is read or written
    if (tid == 0) a.tokens[b] = -1;
    return;
  }
  const float t = a.temperature ? a.temperature[b] : 1.0f, p = a.top_p ? a.top_p[b] : 1.0f, r = a.penalty ? a.penalty[b] : 1.0f;
  const int k = a.top_k ? a.top_k[b] : 0;
  int hl = (a.history && a.hist_len) ? a.hist_len[b] : 0;
  const int hl_raw = hl;
  hl = hl < 0 ? 0 : (hl > a.max_history ? a.max_history : hl);

  const RowView<LT> row = make_row_view<LT>(a.logits, (size_t)b, V, t, r, r > 1.0f && hl > 0, reinterpret_cast<const u32*>(smem));
  if (row.pen)  // (block-uniform)
    build_bitmap(reinterpret_cast<u32*>(smem), V, a.history + (size_t)b * a.max_history, hl, nullptr, 0);

  const int tok = sample_row_token<LT>(row, p, k, a.u + b);

  if (tid == 0) {  // the row's results, and the step that makes a slot finished
    a.tokens[b] = tok;
    const bool append = (a.flags & 1) && a.history && a.hist_len;
    sample_finish_token(tok, append ? a.history + (size_t)b * a.max_history : nullptr, a.max_history, append ? a.hist_len + b : nullptr, hl_raw,
                        a.stop_ids, a.num_stop, a.finished ? a.finished + b : nullptr, ((a.flags & 2) && a.seqlens) ? a.seqlens + b : nullptr, seq,
                        a.max_len);
  }
}

}  // namespace

int launch_sample_logits(const void* logits, int logits_dtype, int batch, int vocab, const void* u, const void* temperature, const void* top_k,
                         const void* top_p, const void* penalty, void* history, void* hist_len, int max_history, void* seqlens, const void* stop_ids,
                         int num_stop, void* finished, int max_len, int flags, void* tokens, hipStream_t st) {
  if (batch < 1 || vocab < 1 || vocab > (1 << 20) || logits_dtype < 0 || logits_dtype > 2) return -1;
  SampleArgs a;
  a.logits = logits;
  a.u = (const float*)u;
  a.temperature = (const float*)temperature;
  a.top_k = (const int*)top_k;
  a.top_p = (const float*)top_p;
  a.penalty = (const float*)penalty;
  a.history = (int*)history;
  a.hist_len = (int*)hist_len;
  a.seqlens = (int*)seqlens;
  a.stop_ids = (const int*)stop_ids;
  a.finished = (int*)finished;
  a.tokens = (int*)tokens;
  a.vocab = vocab;
  a.max_history = history ? max_history : 0;
  a.num_stop = stop_ids ? num_stop : 0;
  a.max_len = max_len;
  a.flags = flags;
  // the bitmap exists only where a penalty can apply: V bits, at most 128 KiB beside the 25 KiB of static LDS (160 KiB per workgroup)
  const size_t lds = (history && hist_len && penalty) ? (size_t)((vocab + 31) / 32) * 4 : 0;
  auto go = [&](void (*kernel)(SampleArgs)) {
    static bool raised[3] = {false, false, false};  // dynamic LDS above 64 KiB is opted into once per kernel; not a stream operation
    if (lds > 48 * 1024 && !raised[logits_dtype]) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      raised[logits_dtype] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(kSampleThreads), lds, st, a);
  };
  if (logits_dtype == 0) go(sample_kernel<0>);
  else if (logits_dtype == 1) go(sample_kernel<1>);
  else go(sample_kernel<2>);
  return 0;
}

}  // namespace awq
