// Prompt-lookup speculative decoding on the device (gfx950, wave64): the token-level machinery around a packed step of the KV-cache path.
// DESIGN.md "Speculative decoding" states the four contracts by values; tests/spec_oracle.py restates them in numpy.
//
//   spec_draft_kernel   one block per slot: the longest (then most recent) earlier occurrence of the history's last n-gram, its continuation
//   spec_pack_kernel    one block: grants the step's token budget in slot order -> cu_seqlens_q and the packed input ids
//   spec_verify_kernel  one block of 1024 per packed row: the sampler's row routine (awq_sample_row.hpp, the text sample_kernel runs) with the
//                       owner's parameters; the penalty set is the history plus the burst's earlier inputs
//   spec_accept_kernel  one thread per slot: the leading run of drafts that equal their samples, and step 9 of the sampling contract per token
//
// Nothing is read on the host, no workspace, no global atomics; every grid comes from host arguments, so the four launches sit in the step's
// captured graph.  Every index formed from a device array is clamped or guarded before it forms an address: corrupt arrays give unspecified
// results, never an access outside the tensors.
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_sample_row.hpp"
#include "awq_varq.hpp"

namespace awq {
namespace {

using namespace sample_row;

// ---- the drafter ----
constexpr int kDraftThreads = 256, kDraftWaves = kDraftThreads / 64;
constexpr int kMaxNgram = 8, kMaxDraft = 15;

struct DraftArgs {
  const int* history;
  const int* hist_len;
  const int* seqlens;
  const int* max_draft;
  int* drafts;
  int* draft_len;
  int max_history, vocab, kmax, ngram_min, ngram_max, max_len;
};

__global__ __launch_bounds__(kDraftThreads) void spec_draft_kernel(DraftArgs a) {
  __shared__ int s_suffix[kMaxNgram];  // s_suffix[t] = history[L - 1 - t]
  __shared__ u64 s_red[kDraftWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = a.hist_len[b], seq = a.seqlens[b];
  const int* h = a.history + (size_t)b * a.max_history;
  const bool can = seq >= 0 && L <= a.max_history && L >= a.ngram_min + 1;  // (block-uniform)
  u64 best = 0ull;  // max over (m_i << 32 | i) of the candidates with m_i >= ngram_min; m_i >= 1, so 0 = none
  if (can) {
    if (tid < a.ngram_max) s_suffix[tid] = L - 1 - tid >= 0 ? h[L - 1 - tid] : 0;  // (t <= i <= L - 2: such an entry is never compared)
    __syncthreads();
    int suf[kMaxNgram];
#pragma unroll
    for (int t = 0; t < kMaxNgram; ++t) suf[t] = t < a.ngram_max ? s_suffix[t] : 0;
    for (int i = tid; i <= L - 2; i += kDraftThreads) {  // the row is read once: only an end that matches the last token looks further back
      int m = 0;
#pragma unroll
      for (int t = 0; t < kMaxNgram; ++t) {
        const bool go = m == t && t < a.ngram_max && i - t >= 0;
        if (go && h[i - t] == suf[t]) m = t + 1;
      }
      const u64 key = ((u64)(u32)m << 32) | (u64)(u32)i;
      if (m >= a.ngram_min && key > best) best = key;
    }
  }
  best = wave_max(best);
  if (lane == 0) s_red[wave] = best;
  __syncthreads();
  if (wave != 0) return;
  best = s_red[0];
#pragma unroll
  for (int w = 1; w < kDraftWaves; ++w) best = s_red[w] > best ? s_red[w] : best;
  int c = 0, start = 0;
  if (best != 0ull) {
    const int i = (int)(u32)best;
    const int md = a.max_draft ? a.max_draft[b] : a.kmax;
    long long cap = a.kmax;
    cap = cap < (long long)md ? cap : (long long)md;
    cap = cap < (long long)(L - 1 - i) ? cap : (long long)(L - 1 - i);  // it may run into the suffix itself: a periodic text drafts its period
    const long long room = (long long)a.max_len - (long long)seq - 1;  // the store of the step stays inside the cache
    cap = cap < room ? cap : room;
    c = cap > 0 ? (int)cap : 0;
    start = i + 1;  // start + c - 1 <= L - 1 < max_history
  }
  const int id = lane < c ? h[start + lane] : 0;
  const u64 bad = __ballot(lane < c && (id < 0 || id >= a.vocab));
  if (bad) c = __ffsll((long long)bad) - 1;
  if (lane < a.kmax) a.drafts[(size_t)b * a.kmax + lane] = lane < c ? id : -1;
  if (lane == 0) a.draft_len[b] = c;
}

// ---- the packer ----
constexpr int kPackThreads = 1024, kPackWaves = kPackThreads / 64;

struct PackArgs {
  const int* last_tokens;
  int* drafts;
  int* draft_len;
  const int* seqlens;
  int* cu;
  int* input_ids;
  int batch, kmax, total_q;
};

// exclusive prefix sum of v over the block's threads; total: the block's sum (two barriers, s_w is free again on return)
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int off = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kPackWaves; ++w) {
    const int x = s_w[w];
    off += w < wave ? x : 0;
    sum += x;
  }
  __syncthreads();
  total = sum;
  return off + incl - v;
}

__global__ __launch_bounds__(kPackThreads) void spec_pack_kernel(PackArgs a) {
  __shared__ int s_w[kPackWaves];
  const int tid = threadIdx.x, B = a.batch, K = a.kmax;
  int cnt = 0;
  for (int b = tid; b < B; b += kPackThreads) cnt += a.seqlens[b] >= 0 ? 1 : 0;
  int A;
  (void)block_scan_excl(cnt, s_w, A);
  const int R = a.total_q - A;  // >= 0: total_q >= batch >= A
  int carry_e = 0, carry_n = 0;  // drafts asked for / rows granted by the slots before this round's (block-uniform)
  for (int base = 0; base < B; base += kPackThreads) {
    const int b = base + tid;
    const bool in = b < B, act = in && a.seqlens[b] >= 0;
    int d = act ? a.draft_len[b] : 0;
    d = d < 0 ? 0 : (d > K ? K : d);
    int sum_d, sum_n;
    const int e = carry_e + block_scan_excl(d, s_w, sum_d);
    int c = R - e;
    c = c < 0 ? 0 : (c > d ? d : c);
    const int n = act ? 1 + c : 0;
    const int off = carry_n + block_scan_excl(n, s_w, sum_n);  // off + n <= A + min(R, sum of d) <= total_q
    if (in) {
      a.draft_len[b] = c;
      a.cu[b] = off;
      if (act && off + n <= a.total_q) {
        a.input_ids[off] = a.last_tokens[b];
        for (int j = 0; j < c; ++j) a.input_ids[off + 1 + j] = a.drafts[(size_t)b * K + j];
      }
      for (int j = c; j < K; ++j) a.drafts[(size_t)b * K + j] = -1;  // what the budget cut is no draft any more
    }
    carry_e += sum_d;
    carry_n += sum_n;
  }
  if (tid == 0) a.cu[B] = carry_n;
  for (int r = carry_n + tid; r < a.total_q; r += kPackThreads) a.input_ids[r] = -1;  // padding: zeros from embed_tokens, skipped by the packed kernels
}

// ---- the verifier ----
struct VerifyArgs {
  const void* logits;
  const float* u;
  const int* cu;
  const int* input_ids;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const float* penalty;
  const int* history;
  const int* hist_len;
  int* row_tokens;
  int batch, vocab, max_history, total_q;
};

template <int LT>
__global__ __launch_bounds__(kSampleThreads) void spec_verify_kernel(VerifyArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // the penalty set's presence bitmap: V bits (only launches with a history have it)
  const int r = blockIdx.x, tid = threadIdx.x, V = a.vocab;
  int b = 0;
  long long s = 0, sq = 0;
  if (!varq_owner(as_const_i32(a.cu), a.batch, r, b, s, sq)) {  // padding of the token budget: nothing else is read
    if (tid == 0) a.row_tokens[r] = -1;
    return;
  }
  const float t = a.temperature ? a.temperature[b] : 1.0f, p = a.top_p ? a.top_p[b] : 1.0f, pr = a.penalty ? a.penalty[b] : 1.0f;
  const int k = a.top_k ? a.top_k[b] : 0;
  const bool hist = a.history && a.hist_len;
  const int Lh = hist ? a.max_history : 0;
  const int hl_raw = hist ? a.hist_len[b] : 0;
  const int hl = hl_raw < 0 ? 0 : (hl_raw > Lh ? Lh : hl_raw);
  // the burst's earlier inputs i = 1 .. j that the serial loop would have appended before this position: 0 <= hl_raw + i - 1 < Lh.
  // 0 <= s <= r, so the burst's rows r - s .. r lie inside [0, total_q).
  const long long i0 = hl_raw < 0 ? 1ll - (long long)hl_raw : 1ll, i1 = s < (long long)Lh - hl_raw ? s : (long long)Lh - hl_raw;
  const int n_extra = i1 >= i0 ? (int)(i1 - i0 + 1) : 0;
  const int* extra = a.input_ids + ((long long)r - s + (n_extra ? i0 : 0));

  const RowView<LT> row = make_row_view<LT>(a.logits, (size_t)r, V, t, pr, pr > 1.0f && (hl > 0 || n_extra > 0), reinterpret_cast<const u32*>(smem));
  if (row.pen)  // (block-uniform)
    build_bitmap(reinterpret_cast<u32*>(smem), V, a.history + (size_t)b * Lh, hl, extra, n_extra);

  const int tok = sample_row_token<LT>(row, p, k, a.u + r);
  if (tid == 0) a.row_tokens[r] = tok;
}

// ---- the accept chain ----
constexpr int kAcceptThreads = 64;

struct AcceptArgs {
  const int* row_tokens;
  const int* input_ids;
  const int* cu;
  int* history;
  int* hist_len;
  int* seqlens;
  const int* stop_ids;
  int* finished;
  int* out_tokens;
  int* num_emitted;
  int* last_tokens;
  int batch, total_q, kmax, max_history, num_stop, max_len, flags;
};

__global__ __launch_bounds__(kAcceptThreads) void spec_accept_kernel(AcceptArgs a) {
  const int b = blockIdx.x * kAcceptThreads + threadIdx.x;
  if (b >= a.batch) return;
  int* out = a.out_tokens + (size_t)b * (a.kmax + 1);
  for (int j = 0; j <= a.kmax; ++j) out[j] = -1;
  const long long c0 = a.cu[b], c1 = a.cu[b + 1];
  long long n = c1 - c0;
  int seq = a.seqlens ? a.seqlens[b] : 0;
  if (n <= 0 || seq < 0 || c0 < 0 || c0 >= a.total_q) {  // inactive, or no rows this step: nothing else is touched
    a.num_emitted[b] = 0;
    a.last_tokens[b] = -1;
    return;
  }
  n = n > a.kmax + 1 ? a.kmax + 1 : n;
  n = c0 + n > a.total_q ? a.total_q - c0 : n;
  const int* rt = a.row_tokens + c0;
  const int* in = a.input_ids + c0;
  int acc = 0;  // the leading drafts that equal the sample of the row before them
  while (acc <= (int)n - 2 && rt[acc] == in[acc + 1]) ++acc;
  const bool append = (a.flags & 1) && a.history && a.hist_len;
  int hl_raw = append ? a.hist_len[b] : 0;
  int emitted = 0, tok = -1;
  for (int j = 0; j <= acc; ++j) {
    tok = rt[j];
    out[j] = tok;
    ++emitted;
    seq = sample_finish_token(tok, append ? a.history + (size_t)b * a.max_history : nullptr, a.max_history, append ? a.hist_len + b : nullptr, hl_raw,
                              a.stop_ids, a.num_stop, a.finished ? a.finished + b : nullptr, ((a.flags & 2) && a.seqlens) ? a.seqlens + b : nullptr,
                              seq, a.max_len);
    ++hl_raw;
    if (seq < 0) break;  // the slot has finished: what the serial loop would not have sampled is not emitted
  }
  a.num_emitted[b] = emitted;
  a.last_tokens[b] = tok;
}

}  // namespace

int launch_spec_draft_ngram(const void* history, const void* hist_len, const void* seqlens, const void* max_draft, void* drafts, void* draft_len,
                            int batch, int max_history, int vocab, int kmax, int ngram_min, int ngram_max, int max_len, hipStream_t st) {
  if (batch < 1 || max_history < 1 || vocab < 1 || kmax < 0 || kmax > kMaxDraft || ngram_min < 1 || ngram_min > ngram_max || ngram_max > kMaxNgram)
    return -1;
  DraftArgs a;
  a.history = (const int*)history;
  a.hist_len = (const int*)hist_len;
  a.seqlens = (const int*)seqlens;
  a.max_draft = (const int*)max_draft;
  a.drafts = (int*)drafts;
  a.draft_len = (int*)draft_len;
  a.max_history = max_history;
  a.vocab = vocab;
  a.kmax = kmax;
  a.ngram_min = ngram_min;
  a.ngram_max = ngram_max;
  a.max_len = max_len;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(batch), dim3(kDraftThreads), 0, st, a);
  return 0;
}

int launch_spec_pack(const void* last_tokens, void* drafts, void* draft_len, const void* seqlens, void* cu_seqlens_q, void* input_ids, int batch,
                     int kmax, int total_q, hipStream_t st) {
  if (batch < 1 || batch > 65535 || kmax < 0 || kmax > kMaxDraft || total_q < batch) return -1;
  PackArgs a;
  a.last_tokens = (const int*)last_tokens;
  a.drafts = (int*)drafts;
  a.draft_len = (int*)draft_len;
  a.seqlens = (const int*)seqlens;
  a.cu = (int*)cu_seqlens_q;
  a.input_ids = (int*)input_ids;
  a.batch = batch;
  a.kmax = kmax;
  a.total_q = total_q;
  hipLaunchKernelGGL(spec_pack_kernel, dim3(1), dim3(kPackThreads), 0, st, a);
  return 0;
}

int launch_spec_verify(const void* logits, int logits_dtype, int total_q, int vocab, const void* u, const void* cu_seqlens_q, const void* input_ids,
                       int batch, const void* temperature, const void* top_k, const void* top_p, const void* penalty, const void* history,
                       const void* hist_len, int max_history, void* row_tokens, hipStream_t st) {
  if (total_q < 1 || batch < 1 || batch > 65535 || vocab < 1 || vocab > (1 << 20) || logits_dtype < 0 || logits_dtype > 2) return -1;
  VerifyArgs a;
  a.logits = logits;
  a.u = (const float*)u;
  a.cu = (const int*)cu_seqlens_q;
  a.input_ids = (const int*)input_ids;
  a.temperature = (const float*)temperature;
  a.top_k = (const int*)top_k;
  a.top_p = (const float*)top_p;
  a.penalty = (const float*)penalty;
  a.history = (const int*)history;
  a.hist_len = (const int*)hist_len;
  a.row_tokens = (int*)row_tokens;
  a.batch = batch;
  a.vocab = vocab;
  a.max_history = history ? max_history : 0;
  a.total_q = total_q;
  // as in launch_sample_logits: the bitmap exists only where a penalty can apply
  const size_t lds = (history && hist_len && penalty) ? (size_t)((vocab + 31) / 32) * 4 : 0;
  auto go = [&](void (*kernel)(VerifyArgs)) {
    static bool raised[3] = {false, false, false};  // dynamic LDS above 64 KiB is opted into once per kernel; not a stream operation
    if (lds > 48 * 1024 && !raised[logits_dtype]) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      raised[logits_dtype] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(total_q), dim3(kSampleThreads), lds, st, a);
  };
  if (logits_dtype == 0) go(spec_verify_kernel<0>);
  else if (logits_dtype == 1) go(spec_verify_kernel<1>);
  else go(spec_verify_kernel<2>);
  return 0;
}

int launch_spec_accept(const void* row_tokens, const void* input_ids, const void* cu_seqlens_q, int batch, int total_q, int kmax, void* history,
                       void* hist_len, int max_history, void* seqlens, const void* stop_ids, int num_stop, void* finished, int max_len, int flags,
                       void* out_tokens, void* num_emitted, void* last_tokens, hipStream_t st) {
  if (batch < 1 || batch > 65535 || total_q < 1 || kmax < 0 || kmax > kMaxDraft) return -1;
  AcceptArgs a;
  a.row_tokens = (const int*)row_tokens;
  a.input_ids = (const int*)input_ids;
  a.cu = (const int*)cu_seqlens_q;
  a.history = (int*)history;
  a.hist_len = (int*)hist_len;
  a.seqlens = (int*)seqlens;
  a.stop_ids = (const int*)stop_ids;
  a.finished = (int*)finished;
  a.out_tokens = (int*)out_tokens;
  a.num_emitted = (int*)num_emitted;
  a.last_tokens = (int*)last_tokens;
  a.batch = batch;
  a.total_q = total_q;
  a.kmax = kmax;
  a.max_history = history ? max_history : 0;
  a.num_stop = stop_ids ? num_stop : 0;
  a.max_len = max_len;
  a.flags = flags;
  hipLaunchKernelGGL(spec_accept_kernel, dim3((batch + kAcceptThreads - 1) / kAcceptThreads), dim3(kAcceptThreads), 0, st, a);
  return 0;
}

}  // namespace awq
