// Internal launcher declarations (host side).  The public surface is include/awq_cdna4.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "awq_linear_route.hpp"

namespace awq {
// every knob the routes of the dense W4 cdna4 entries read (awq_linear_route.hpp); awq_tune_set writes it, the launchers and the entries read it (awq_capi.hip)
extern LinearKnobs g_linear;
// Kernels that use more than 64 KiB of dynamic LDS must be opted in with hipFuncSetAttribute, and the attribute belongs to the
// (kernel, DEVICE) pair: a single-process multi-GPU caller (the reference's accelerate layer placement, awq/entry.py:167-186)
// launches the same kernel on several devices.  One LdsOptIn per kernel instantiation remembers, per device ordinal, that the
// opt-in has been made; racing threads may both make the (idempotent) call.
struct LdsOptIn {
  std::atomic<uint64_t> done[4] = {};  // device ordinals 0..255
  void ensure(const void* kern, int bytes = 160 * 1024) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    std::atomic<uint64_t>& w = done[(dev >> 6) & 3];
    if (w.load(std::memory_order_acquire) & bit) return;
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    w.fetch_or(bit, std::memory_order_release);
  }
};
// Compute units of the current device (cached per ordinal).  The plans that assume ONE residency round on the whole MI355X (the block-pair
// K split: 256 blocks, pair partners on one XCD) ask it: a partitioned (CPX / NPS), CU-masked or other part falls back to plans that do
// not depend on co-residency.  Without a device (host-side plan queries in CPU tests) the answer is the MI355X's 256.
inline int device_cu_count() {
  static std::atomic<int> cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::atomic<int>& c = cached[dev & 63];
  int v = c.load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    c.store(v, std::memory_order_relaxed);
  }
  return v;
}
// layout: 0 = reference v2 interleave, 1 = cdna4 interleave (bf16 only)
// szp: optional packed {scale | scaled_zero << 16} u32 [N/16][K/128][16] (cdna4 layout only), else nullptr
int launch_gemv(const void* x, const void* qw, const void* s, const void* z, const void* szp, void* out, int m, int n,
                int k, int dtype, int layout, hipStream_t st);
// fast decode path on cdna4 buffers (1 <= m <= 8, bf16 / fp16 (W3: bf16), packed sz required).  epi 0: out[m,n] (+bias);
// epi 1: qw = [gate; up] stacked (n = 2*ffn rows), out[m, n/2] = silu(gate) * up.  Returns -1 if unsupported.
int launch_gemv_cdna4(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                      int epi, int bits, int dtype, hipStream_t st);
// RMSNorm fused in front of the decode GEMV (awq_gemv_cdna4.hip, NORM = 1): 1 <= m <= 4.  Returns -1 if unsupported.
int launch_gemv_cdna4_norm(const void* x, const void* gamma, float eps, const void* qw, const void* szp, const void* bias, void* out,
                           int m, int n, int k, int epi, int dtype, hipStream_t st);
// reference (v2) layout fast decode path (awq_gemv_v2fast.hip): 1 <= m <= 8, n % 16 == 0, fp16 / bf16, bias fused.
// gpad = rows of scales / zeros that may be read (>= k / 128).  Returns -1 if unsupported.
bool gemv_v2fast_enabled();  // false while a knob of the older kernel (awq_tune_set gemv_*) is active
int launch_gemv_v2fast(const void* x, const void* qw, const void* s, const void* z, const void* bias, void* out, int m, int n, int k,
                       int gpad, int dtype, hipStream_t st);
// reference (v2) layout skinny GEMM (awq_skinny_v2.hip): 9 <= m <= 255, n % 16 == 0, fp16 / bf16, bias fused.  -1 if unsupported.
int launch_skinny_v2(const void* x, const void* qw, const void* s, const void* z, const void* bias, void* out, int m, int n, int k,
                     int gpad, int dtype, hipStream_t st);
// W3 ("w3c") format helpers (awq_w3.hip)
int launch_pack_w3(const void* q_u8, void* qw3, int n, int k, hipStream_t st);
int launch_unpack_w3(const void* qw3, void* out_u8, int n, int k, hipStream_t st);
int launch_dequant_w3(const void* qw3, const void* s, const void* z, void* out, int n, int k, int dtype, hipStream_t st);
int launch_expand_w3_to_cdna4(const void* qw3, void* qw4, int n, int k, hipStream_t st);
int gemv_cdna4_tune_set(const char* key, int value);
// LDS-DMA streaming decode GEMV (awq_gemv_dma.hip): 1 <= m <= 8, cdna4 layout + packed sz.  epi 0: out[m,n] (+bias); epi 1: stacked
// [gate; up]; epi 2: gate / up rows interleaved 8 + 8 per slab; both out[m, n/2] = silu(gate) * up.  -1 if the shape is not served.
// szfmt 0: szp = sz_packed {s | sz << 16} in T;  szfmt 1: szp = sz_half (f16-mantissa dequant, awq_pack_szh_cdna4)
// f32out (epi 0, no bias): out is float [m, n], the fp32 sums unrounded -- the K-shard partial of a tensor-parallel row split
int launch_gemv_dma(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int epi,
                    int dtype, int szfmt, hipStream_t st, int f32out = 0);
int gemv_dma_tune_set(const char* key, int value);
int launch_moe_gemv_cdna4(const void* x, const void* qw, const void* szp, const void* offsets, void* out, int total_rows,
                          int experts, int n, int k, int dtype, hipStream_t st);
// tail pass of the grouped prefill GEMM (awq_skinny_cdna4.hip): the rows of every expert's last partial 256-row tile when there are fewer than `tail` of them
int launch_moe_skinny_tail_cdna4(const void* x, const void* qw, const void* szp, const void* offsets, void* out, int experts, int n, int k,
                                 int dtype, hipStream_t st, int epi, int tail);
void moe_v6_set_tail(int v);  // knob moe_tail (0 .. 64; default 64)
// grouped skinny kernel for 9..255 sorted rows (awq_skinny_cdna4.hip)
int launch_moe_skinny_cdna4(const void* x, const void* qw, const void* szp, const void* offsets, void* out, int total_rows,
                            int experts, int n, int k, int dtype, hipStream_t st);
int launch_pack_sz_cdna4(const void* s, const void* z, void* szp, int n, int k, hipStream_t st);
// "sz_half" form for the decode kernels: {f16(s') | f16(sz) << 16}; *inexact (device int, caller-zeroed) is set if a value is not exact
int launch_pack_szh_cdna4(const void* s, const void* z, void* szh, int* inexact, int n, int k, int dtype, hipStream_t st);
int launch_gemm(const void* x, const void* qw, const void* s, const void* z, const void* szp, void* out, int m, int n,
                int k, int dtype, int layout, void* ws, size_t ws_bytes, hipStream_t st);
int launch_repack_v2_cdna4(const void* src, void* dst, int n, int k, int to_cdna4, hipStream_t st);
int launch_unpack_cdna4(const void* qw, void* out_u8, int n, int k, hipStream_t st);
int launch_dequant_cdna4(const void* qw, const void* s, const void* z, void* out, int n, int k, int dtype, hipStream_t st);
size_t gemm_workspace_bytes(int m, int n, int k);
// bias may be nullptr; when given it is added in the epilogue (`out + bias` in T)
// bits 4: cdna4 W4 tiles; bits 3: w3c tiles (read natively by the v4 / v4n weight producers)
int launch_gemm_cdna4_v3(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                         int tile_n, int dtype, void* ws, size_t ws_bytes, hipStream_t st, int bits = 4, int epi = 0, const void* szh = nullptr);
// epi 2: qw holds QuantLlamaMLP's 8 + 8 row-interleaved gate / up pair, out[m, n/2] = silu(gate) * up fused into the tile epilogue
// epi 3: out is float [m, n]: the fp32 accumulators unrounded, no bias (K-shard partial of a tensor-parallel row split)
// skinny GEMM, 9 <= m <= 255 (row chunks of <= 64), cdna4 layout + packed sz (awq_skinny_cdna4.hip); bias may be nullptr; -1 if unsupported
int launch_skinny_cdna4(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                        int dtype, hipStream_t st, int f32out = 0, void* ws = nullptr, size_t ws_bytes = 0);
// the skinny launch's K split across blocks (awq_skinny_cdna4.hip): K parts for a pass of m rows (1 = unsplit), its optional fp32 scratch, knob
int launch_skinny_w3(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int epi, int dtype, hipStream_t st,
                     int f32out = 0);
int launch_skinny_gate_up(const void* x, const void* qw, const void* szp, void* out, int m, int n2, int k, int dtype, hipStream_t st);
int skinny_splitk_parts(int m, int n, int k);
size_t skinny_splitk_workspace_bytes(int m, int n, int k);
int skinny_tune_set(const char* key, int value);
// mid-M GEMM (awq_midm_cdna4.hip): 9 <= m <= 255, x tile shared by the block through LDS-DMA, waves split N, K split across blocks (ticket + fp32 parts);
// szfmt 0: szp = sz_packed, 1: sz_half; epi 0 / 2; f32out: float [m, n] unrounded; ws: the optional scratch of the K split.  -1 if the shape is not served
int launch_midm_cdna4(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int epi, int dtype, int szfmt,
                      int bits, int f32out, void* ws, size_t ws_bytes, hipStream_t st);
bool midm_takes(int m, int n, int k);
size_t midm_workspace_bytes(int m, int n, int k);
int midm_parts(int m, int n, int k);
int midm_tune_set(const char* key, int value);
int midm_init();
// ticket words of an in-launch K split (zero outside a launch that uses them): `groups` words that belong to ONE launch at a time -- the lane of the stream for
// eager launches, words of their own for launches recorded during a capture; nullptr = none available (the caller runs unsplit).  awq_midm_cdna4.hip
unsigned* splitk_ticket_words(hipStream_t st, int groups);
// batched decode on the same kernel (m <= 16; szfmt 1: szp = sz_half; epi 0 / 2 as launch_gemv_dma); -1 if unsupported
int launch_skinny_decode(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int epi,
                         int dtype, int szfmt, hipStream_t st, int f32out = 0);
int launch_moe_gemm(const void* x, const void* qw, const void* s, const void* z, const void* offsets, void* out, int total_m,
                    int experts, int n, int k, int gpad, int dtype, int layout, hipStream_t st);
int gemv_tune_set(const char* key, int value);
int gemm_v3_tune_set(const char* key, int value);  // tile-plan / dispatch knobs (awq_gemm_plan.hip)
// 256 x 128 tiles with the same hand-scheduled K loop (awq_gemm_v4n.hip)
void launch_gemm_cdna4_v4n(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                           int n_begin, int n_end, int dtype, void* ws, size_t ws_bytes, hipStream_t st, int bits = 4, int epi = 0);
size_t gemm_v4n_workspace_bytes(int m, int n_cols, int k);
extern int g_v4n_ksplit_force;  // knob gemm_splitk > 1
extern int g_v4n_ksplit_cap;    // knob gemm_splitk_cap
bool gemm_cdna4_v3_takes(int m, int k);  // m >= 256, or a shorter prompt the 256-row tile still beats the skinny kernel on
size_t gemm_cdna4_v3_workspace_bytes(int m, int n, int k);
int gemm_cdna4_v3_plan(int m, int n, int bits, int* mode, int* cols_main);
int gemm_cdna4_v3_narrow_kernel(int m, int n_cols, int k, int bits, int has_workspace, int epi);  // 1 v6 (NS = 2), 0 v4n unsplit, >= 2 v4n split-K ranges
int gemv_dma_plan(int m, int n, int k, int epi, int* kernel);  // weight passes of the decode entry (0: not served); *kernel 0 streaming, 1 skinny
int gemv_dma_plan_detail(int m, int n, int k, int epi, int chunk, int out[8]);  // chunk count; out = the words of chunk `chunk` (awq_decode_plan.hpp)
size_t gemm_cdna4_v3_workspace_bytes_w3(int m, int n, int k);  // same rule for w3c tiles (every m > 8 takes the tile kernels)
bool moe_v4_enabled();  // knob moe_v4 (default on): the grouped skinny / tile kernels; 0 = the 128 x 128 grouped kernel for every batch above 8 rows
// the same grouped GEMM on the v6 tile (awq_gemm_v6.hip: one pipelined wave per SIMD, weights in registers); total >= 256
// epi 2: per-expert w1 / w3 pair interleaved 8 + 8 per slab (n = 2 x ffn), out [total, n / 2] = silu(w1 x) * (w3 x) fused into the tile epilogue
// szh: the experts' stacked sz_half side buffers (optional): the tile launch then dequantises in the f16-mantissa form; the tail pass keeps sz_packed
int launch_moe_gemm_cdna4_v6(const void* x, const void* qw, const void* szp, const void* offsets, void* out, int total, int experts,
                             int n, int k, int dtype, hipStream_t st, int epi = 0, const void* szh = nullptr);
// out[t, 8 j + c] = T(T(silu(in[t, 16 j + c])) * in[t, 16 j + 8 + c]): the SiLU * mul tail on an [m, n2] result of the 8 + 8 interleaved pair
int launch_silu_mul_interleaved(const void* in, void* out, int m, int n2, int dtype, hipStream_t st);
int launch_silu_mul(const void* gate, const void* up, void* out, size_t count, int dtype, hipStream_t st);  // out = T(T(silu(gate)) * up), count % 8 == 0
bool moe_v6_enabled();  // knob moe_v6 (default on)
// MoE routing on the device (awq_moe_route_cdna4.hip); -1 if the sizes are outside the documented limits, pointers validated by the caller
// logits [tokens, experts] (logits_dtype 0 fp16, 1 bf16, 2 fp32) -> topk_ids int32 / topk_w fp32 [tokens, top_k], order / inv int32 [tokens top_k], offsets int32 [experts + 1]
int launch_moe_route(const void* logits, int logits_dtype, int tokens, int experts, int top_k, int renormalize, void* topk_ids, void* topk_w,
                     void* order, void* inv, void* offsets, hipStream_t st);
int launch_moe_gather(const void* x, const void* order, void* xs, int tokens, int top_k, int hidden, hipStream_t st);  // xs[r] = x[order[r] / top_k]
int launch_moe_combine(const void* ys, const void* inv, const void* topk_w, void* out, int tokens, int top_k, int hidden, int dtype, hipStream_t st);
// next-token sampling on the device (awq_sample_cdna4.hip): one block per row of logits [batch, vocab]; -1 if the sizes are outside the documented
// limits, pointers validated by the caller (every pointer but logits / u / tokens may be null = that step is off); flags: 1 append, 2 advance
int launch_sample_logits(const void* logits, int logits_dtype, int batch, int vocab, const void* u, const void* temperature, const void* top_k,
                         const void* top_p, const void* penalty, void* history, void* hist_len, int max_history, void* seqlens, const void* stop_ids,
                         int num_stop, void* finished, int max_len, int flags, void* tokens, hipStream_t st);
// prompt-lookup speculative decoding on the device (awq_spec_cdna4.hip): the n-gram drafter (one block per slot), the packer of the step's
// cu_seqlens_q / input ids (one block), the sampler's row routine on every packed row, and the accept chain (step 9 per emitted token); -1 if the
// sizes are outside the documented limits, pointers validated by the caller
int launch_spec_draft_ngram(const void* history, const void* hist_len, const void* seqlens, const void* max_draft, void* drafts, void* draft_len,
                            int batch, int max_history, int vocab, int kmax, int ngram_min, int ngram_max, int max_len, hipStream_t st);
int launch_spec_pack(const void* last_tokens, void* drafts, void* draft_len, const void* seqlens, void* cu_seqlens_q, void* input_ids, int batch,
                     int kmax, int total_q, hipStream_t st);
int launch_spec_verify(const void* logits, int logits_dtype, int total_q, int vocab, const void* u, const void* cu_seqlens_q, const void* input_ids,
                       int batch, const void* temperature, const void* top_k, const void* top_p, const void* penalty, const void* history,
                       const void* hist_len, int max_history, void* row_tokens, hipStream_t st);
int launch_spec_accept(const void* row_tokens, const void* input_ids, const void* cu_seqlens_q, int batch, int total_q, int kmax, void* history,
                       void* hist_len, int max_history, void* seqlens, const void* stop_ids, int num_stop, void* finished, int max_len, int flags,
                       void* out_tokens, void* num_emitted, void* last_tokens, hipStream_t st);
// LM head for decode (awq_lm_head_cdna4.hip): out[m, v] = rmsnorm(x)[m, k] W[v, k]^T (+ bias) in one launch, rows with seqlens[b] < 0 left untouched;
// the plan is {blocks, vocabulary rows per tile, waves, k split}; -1 if the sizes are outside the documented limits, pointers validated by the caller
int lm_head_plan(int m, int v, int k, int out[4]);
int launch_lm_head(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                   int out_f32, int m, int v, int k, int dtype, int max_blocks, hipStream_t st);
// the same launch with the logits capped behind the bias (awq_softcap.hpp): y <- softcap * tanh(y / softcap) in fp32; softcap = 0: launch_lm_head
int launch_lm_head_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                           int out_f32, int m, int v, int k, int dtype, float softcap, int max_blocks, hipStream_t st);
int launch_embed_tokens(const int* tokens, const void* table, void* out, int n, int v, int k, hipStream_t st);  // zeros for an id outside [0, v)
// Token log-probabilities (awq_lm_logprobs_cdna4.hip): the LM head fused with log-sum-exp (tile launch + combine launch; with gamma the rmsnorm launch
// runs first into the head of the workspace), and the companion for logits that already exist.  The plan is {row tile, vocabulary tile, blocks, k step};
// -1 if the sizes are outside the documented limits, pointers / alignment / workspace size validated by the caller
int lm_logprobs_plan(int t, int v, int k, int out[4]);
size_t lm_logprobs_workspace_bytes(int t, int v, int k, int with_gamma);
int launch_lm_logprobs(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets, float* logprob,
                       float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits, void* workspace, int max_blocks,
                       hipStream_t st);
int launch_token_logprobs(const void* logits, int logits_dtype, long ld, const int* targets, float* logprob, float* lse, int* argmax, int b, int v,
                          hipStream_t st);
// every logit capped in the tile epilogue before the max / sum-exp, the target pick and the argmax (awq_softcap.hpp); softcap = 0: launch_lm_logprobs
int launch_lm_logprobs_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                               float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                               float softcap, void* workspace, int max_blocks, hipStream_t st);
// logits that already exist, capped in place (awq_util.hip): z <- softcap * tanh(z / softcap) in fp32, one elementwise launch; rows with
// seqlens[b] < 0 untouched (seqlens may be null); logits_dtype 0 fp16, 1 bf16, 2 fp32
int launch_logit_softcap(void* logits, int logits_dtype, long ld, const int* seqlens, int b, int v, float softcap, hipStream_t st);
// Multi-LoRA on packed steps (awq_lora_cdna4.hip): shrink (x A_a^T into the fp32 K-split workspace) and expand (scale, round, B_a^T, add into y in
// place), the adapter of a row read on the device; the plan is {KS, k per split, expand column tile, waves}; -1 if the sizes are outside the documented
// limits, pointers / alignment / workspace size validated by the caller
int lora_plan(int k, int r, int n_slices, int out[4]);
size_t lora_workspace_bytes(int total_q, int k, int r, int n_slices);
int launch_lora_shrink(const void* x, long ldx, const void* a_pool, const int* adapter_ids, const int* cu_seqlens_q, void* ws, int batch,
                       int max_seqlen_q, int total_q, int slots, int k, int r, int n_slices, int dtype, hipStream_t st);
int launch_lora_expand(const void* ws, const void* b_pool, const float* scaling, const int* adapter_ids, const int* cu_seqlens_q, void* y, int batch,
                       int max_seqlen_q, int total_q, int slots, int n, int k, int r, const int* slice_end, int n_slices, int dtype, hipStream_t st);
// expand on QuantLlamaMLP's gate / up pair: y2 [total_q, n2] is the unfused output of the 8 + 8 interleaved stream (read only), b_pool [slots, n2, r]
// holds B_gate rows then B_up rows, h [total_q, n2 / 2] = T(T(silu(gate')) up') with the two deltas added first; rows of an active sequence without
// an adapter get the plain tail; two slices in the workspace (lora_plan(k, r, 2))
int launch_lora_expand_gate_up(const void* ws, const void* b_pool, const float* scaling, const int* adapter_ids, const int* cu_seqlens_q,
                               const void* y2, void* h, int batch, int max_seqlen_q, int total_q, int slots, int n2, int k, int r, int dtype,
                               hipStream_t st);
// AWQ quantisation (awq_quant_cdna4.hip): the group quantiser + packer (layout 0 = v2, 1 = cdna4; every output optional) and the clip search;
// -1 if the sizes are outside the documented limits, pointers / alignment validated by the caller
int launch_quantize_group(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                          void* zeros, void* qweight, int layout, int n, int k, int n_bit, int dtype, hipStream_t st);
// host twin of launch_quantize_group for host memory (the same awq_quant_grid.hpp text compiled for the CPU); intweight: uint8 [n, k], the recovered
// integers' low four bits, instead of a packed qweight
void quantize_group_host(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                         void* zeros, void* intweight, int n, int k, int n_bit, int dtype);
int launch_clip_search(const void* w, long ldw, const void* x, long ldx, void* best_max_val, int* best_idx, float* err, int n, int k, int s,
                       int n_bit, int n_grid, int n_steps, int dtype, hipStream_t st);
// awq_gemm_v6.hip: 256 x 256 blocks of four software-pipelined waves (256 x 64 per wave, weights in registers, x through ds_write)
void launch_gemm_cdna4_v6(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int n_begin,
                          int n_end, int dtype, hipStream_t st, int bits = 4, int epi = 0, int szfmt = 0, int tile_n = 256);
void gemm_v6_set_probe(int v);
// K split over pairs of 256 x 256 blocks inside one launch (tiles that fill at most half the chip, long K: down_proj at 2048 rows); -1 = not served
bool gemm_v6_pair_takes(int m, int n, int k);
int gemm_v6_pair_lost(unsigned* count);  // awq_gemm_v6.hip: pair blocks of the current device that gave up waiting for their partner (outputs NaN) since load
int gemm_cdna4_v3_pair_plan(int m, int n, int k);  // awq_gemm_plan.hip: 1 = the prefill call (with its workspace) takes the block-pair K split
size_t gemm_v6_pair_workspace_bytes(int m, int n, int k);
int launch_gemm_cdna4_v6_pair(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int n_begin, int n_end,
                              int dtype, void* ws, size_t ws_bytes, hipStream_t st, int bits = 4, int epi = 0, int szfmt = 0);
void gemm_v6_set_pair_lead(int v);
void gemm_v6_set_pair_min_nit(int v);
int launch_bias_add(void* out, const void* bias, int m, int n, int dtype, hipStream_t st);
// out[m, n] = T(in_f32) (+ bias in T); n % 8 == 0 (awq_util.hip)
int launch_round_bias_f32(const void* in_f32, const void* bias, void* out, int m, int n, int dtype, hipStream_t st);
// RMSNorm of m rows of k (awq_util.hip; layernorm.cu:39-61's arithmetic); -1 if k % 8 != 0
int launch_rmsnorm(const void* x, const void* gamma, float eps, void* out, int m, int k, int dtype, hipStream_t st);
// decode attention over the FT KV cache (awq_attn_cdna4.hip); arguments validated by the caller
int attn_decode_plan(int batch, int nheads_kv, int head_dim, int timestep, int lmax, int* splits, int* chunk);
size_t attn_decode_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int timestep, int lmax);
int launch_attn_decode(const void* q, const void* k, const void* v, void* k_cache, void* v_cache, const int* lens, const float* alibi,
                       void* out, int B, int H, int Hkv, int Dh, int Lmax, long long q_bs, long long k_bs, long long v_bs, int timestep,
                       int rot, float rot_base, float rot_scale, int neox, int dtype, void* workspace, hipStream_t st);
// prefill attention and the prompt-side rotary embeddings (awq_attn_prefill_cdna4.hip); arguments validated by the caller
int attn_prefill_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* q_tile_rows,
                      int* blocks);
// the q tile and the grid of a packed-query launch (awq_varq.hpp): 64 or 128 rows, a provisional rule
int attn_varq_plan(int batch, int nheads, int nheads_kv, int head_dim, int max_seqlen_q, int* q_tile_rows, int* blocks);
int attn_prefill_tune_set(const char* key, int value);  // "attn_prefill_rows": force the q tile (0 = plan)
int launch_attn_prefill(const void* q, const void* k, const void* v, void* out, int B, int Sq, int Sk, int H, int Hkv, int Dh, long long q_bs,
                        long long q_rs, long long k_bs, long long k_rs, long long v_bs, long long v_rs, float scale, int causal, int dtype,
                        hipStream_t st);
// the same attention with K / V staged from the FT caches (k_cache [Bc, Hkv, Dh/8, Lmax, 8], v_cache [Bc, Hkv, Lmax, Dh]): key j = cache position kv_start + j
int launch_attn_prefill_ftcache(const void* q, const void* k_cache, const void* v_cache, void* out, int B, int Sq, int kv_start, int Sk, int H,
                                int Hkv, int Dh, int Lmax, long long q_bs, long long q_rs, float scale, int causal, int dtype, hipStream_t st);
// prompt-side chunk preparation (awq_attn_chunk_cdna4.hip): rope of q and k, K / V stored into the FT caches, one launch
int launch_rope_kv_store(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int B, int S, int H, int Hkv, int Dh,
                         int rot, int lmax, int start_pos, long long bs, long long rs, int dtype, hipStream_t st);
// split-KV attention for few query rows over a long natural-layout history (awq_attn_splitkv_cdna4.hip); arguments validated by the caller
int attn_splitkv_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* splits, int* chunk);
size_t attn_splitkv_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal);
int attn_splitkv_tune_set(const char* key, int value);  // "attn_splitkv_chunk": force the chunk, a multiple of 64 (0 = plan)
// (the natural-layout store and the split pair themselves: launch_kv_store / launch_kv_attn over the descriptors of awq_kvcache.hpp)
// FP8 KV cache (awq_kv8.hpp): k / v are e4m3 codes [B, Sk, Hkv, Dh] with strides in bytes, k_scale / v_scale fp32 [B, Sk, Hkv] with strides in
// floats.  The one-pass form (awq_attn_prefill_cdna4.hip):
int launch_attn_prefill_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int B, int Sq,
                            int Sk, int H, int Hkv, int Dh, long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs,
                            long long v_rs, long long ks_bs, long long ks_rs, long long vs_bs, long long vs_rs, float scale, int causal, int dtype,
                            hipStream_t st);
// the plan of the device-length form (awq_devlen.hpp): made from the host bound max_seqlen_k alone
int attn_kvcache_plan(int batch, int nheads_kv, int max_seqlen_k, int* splits, int* chunk);
size_t attn_kvcache_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k);
// the plan of a windowed mixed step (awq_window.hpp): attn_kvcache_plan for the bound min(max_seqlen_k, window_left + split_seqlen_q + 63)
int attn_varq_window_plan(int batch, int nheads_kv, int split_seqlen_q, int max_seqlen_k, int window_left, int* splits, int* chunk);
size_t attn_varq_window_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int window_left);
// the plan of a shared-prefix decode (awq_shared.hpp): attn_kvcache_plan for the bound max_prefix, and again for max_seqlen_k
int attn_kvcache_shared_plan(int batch, int nheads_kv, int max_prefix, int max_seqlen_k, int* splits_p, int* chunk_p, int* splits_s, int* chunk_s);
size_t attn_kvcache_shared_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix, int max_seqlen_k);
int launch_rope_with_pos(const void* in, const float* freqs, void* out, int n0, int n1, int h, int d, int d2, long long s0, long long s1,
                         long long sh, long long o0, long long o1, long long oh, int dtype, hipStream_t st);
int launch_rope_neox(const long long* positions, void* query, void* key, const void* cache, int tokens, int heads, int head_size, int rot_dim,
                     int max_pos, int dtype, hipStream_t st);
// encoder-tower attention (awq_attn_tower_cdna4.hip): non-causal, head dims 64 and 72, sequences described on the device by cu_seqlens
// (varlen) or cu_seqlens == NULL (dense: nseq x Sq x Sk with batch strides); arguments validated by the caller
int attn_varlen_plan(int nseq, int nheads, int head_dim, int max_seqlen, int* q_tile_rows, int* blocks);
int attn_tower_tune_set(const char* key, int value);  // "tower_rows": force the q tile (0 = plan)
int launch_attn_tower(const void* q, const void* k, const void* v, void* out, const int* cu_seqlens, int nseq, int Sq, int Sk,
                      long long total_rows, int H, int Hkv, int Dh, long long q_bs, long long q_rs, long long k_bs, long long k_rs,
                      long long v_bs, long long v_rs, float scale, int dtype, hipStream_t st);
// W8A8 linear (awq_w8a8_cdna4.hip); arguments validated by the caller.  w8a8_gemm_plan: blocks of the launch (0 = shape not served) and its tile
int w8a8_gemm_plan(int m, int n, int k, int* tile_m, int* tile_n);
int w8a8_tune_set(const char* key, int value);  // "w8a8_tile": force the 64 x 64 or the 128 x 128 tile (0 = plan)
int launch_w8a8_gemm(const void* x, const void* w, const void* wscales, const void* ascales, const void* bias, void* out, int m, int n, int k,
                     hipStream_t st);
int launch_quant_per_token(const void* x, void* out_i8, void* scale, int m, int k, int dtype, hipStream_t st);
int launch_gelu_quant_per_token(const void* x, void* out_i8, void* scale, void* tmp, int m, int k, hipStream_t st);
int launch_layernorm_quant(const void* x, const void* gamma, const void* beta, float eps, void* out_i8, void* scale, int m, int k,
                           int per_token, int dtype, hipStream_t st);
int launch_unpack_v2(const void* qw, void* out_u8, int n, int k, hipStream_t st);
int launch_dequant_v2(const void* qw, const void* s, const void* z, void* out, int n, int k, int dtype, hipStream_t st);
int launch_pack_v2(const void* q_u8, void* qw, int n, int k, hipStream_t st);
int launch_repack_v1_to_v2(const void* qw1, const void* s1, const void* qz1, void* qw2, void* s2, void* sz2, int n, int k,
                           int gpad, int dtype, hipStream_t st);
}  // namespace awq
