// The natural-layout KV cache family, described once (host side only; no device code reads this header's structs).
//
// A call of the family is a KvView -- where K / V live: dense caches or a pool of pages, T or FP8 codes with scales -- inside a
// KvStoreCall (rope + store of a qkv chunk) or a KvAttnCall (split-KV attention of few query rows).  The C entries of awq_capi.hip
// build one from their positional arguments, check it once per phase and hand it to one of the two launchers below; the launchers pick
// the kernel traits (HostLen / DevLen / Paged<DevLen>, TCache / Kv8) from what the descriptor holds and fill the kernels' own argument
// structs.  A new cache variant adds its fields here, its terms to the phase checks and its traits to the two launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace awq {

struct KvView {
  const void* k = nullptr;  // caches [outer, rows, Hkv, Dh] or pools [num_pages, page_size, Hkv, Dh]: T, or e4m3 codes when k_scale is set
  const void* v = nullptr;
  const float* k_scale = nullptr;  // [outer, rows, Hkv] fp32 (awq_kv8.hpp); nullptr: the T cache
  const float* v_scale = nullptr;
  // outer (batch or page) and row strides: elements of T, bytes of codes, floats of scales.  The dense STORE entries take contiguous
  // caches and give no strides: theirs stay 0 and the store kernels address [outer, rows, Hkv, Dh] themselves.
  long long k_os = 0, k_rs = 0, v_os = 0, v_rs = 0, ks_os = 0, ks_rs = 0, vs_os = 0, vs_rs = 0;
  int outer = 0;                     // cache_batch or num_pages
  int rows = 0;                      // lmax or page_size
  const int* block_table = nullptr;  // device int32 [batch, pages_per_seq] (awq_paged.hpp); nullptr: dense caches
  long long bt_rs = 0;               // its row stride, entries
  int pages_per_seq = 0;
  // keys one sequence can hold, as an int (positions and lengths are int32)
  int capacity() const {
    const long long cap = block_table ? (long long)pages_per_seq * rows : rows;
    return cap < 0x7FFFFFFFll ? (int)cap : 0x7FFFFFFF;
  }
};

struct KvStoreCall {
  const void* qkv;     // [B, S, (H + 2 Hkv) Dh], strides bs / rs
  const float* freqs;  // the call's angles (host start_pos) or the model's whole table [table_rows, rot] (device cache_seqlens)
  void* q_out;
  KvView kv;
  int start_pos;             // host position, used when cache_seqlens == nullptr
  const int* cache_seqlens;  // device int32 [B] (awq_devlen.hpp), with table_rows
  int table_rows;
  int B, S, H, Hkv, Dh, rot;
  long long bs, rs;
  int dtype;
  // packed tokens (awq_varq.hpp): qkv [total_q, (H + 2 Hkv) Dh] with row stride rs, sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1;
  // S is then the host's bound max_seqlen_q and bs unused.  nullptr: the rectangle [B, S]
  const int* cu_seqlens_q = nullptr;
  int max_seqlen_q = 0, total_q = 0;
  // per-head RMSNorm of q and k over Dh before the rotation (awq_rope.hpp, the *_qknorm entries): gammas fp32 [Dh], both or neither.
  // nullptr: no norm, the kernels above
  const float* q_gamma = nullptr;
  const float* k_gamma = nullptr;
  float norm_eps = 0;
};

struct KvAttnCall {
  const void* q;  // [B, Sq, H, Dh], strides q_bs / q_rs
  void* out;
  KvView kv;
  int Sk;                // host length, used when seqlens_k == nullptr
  const int* seqlens_k;  // device int32 [B] (awq_devlen.hpp): length of b = seqlens_k[b] + seqlen_offset <= max_seqlen_k
  int seqlen_offset, max_seqlen_k;
  int B, Sq, H, Hkv, Dh;
  long long q_bs, q_rs;
  float scale;
  int causal, dtype;
  // packed queries (awq_varq.hpp): q / out [total_q, H, Dh], row stride q_rs; Sq is then the host's bound max_seqlen_q, q_bs unused and
  // seqlen_offset the flag lens_before_step (length of b = seqlens_k[b] + Sq_b when set, seqlens_k[b] when clear).  nullptr: the rectangle
  const int* cu_seqlens_q = nullptr;
  int max_seqlen_q = 0, total_q = 0;
  // a mixed step (awq_varq.hpp, awq_attn_varq and its siblings): the split pair takes a sequence with Sq_b <= split_seqlen_q and
  // Sk_b >= split_min_keys, the one-pass kernel leaves it alone.  split_seqlen_q = 0: the plain packed launch
  int split_seqlen_q = 0, split_min_keys = 0;
  // a sliding window on a packed step (awq_window.hpp, awq_attn_varq_window and its siblings): a row attends its own key and the
  // window_left keys before it, clamped by the entry to max_seqlen_k - 1.  -1: no window, the kernels above
  int window_left = -1;
  // a cap on the logits of a windowed step (awq_softcap.hpp, awq_attn_varq_softcap and its siblings): cap * tanh(scale * q.k / cap) in
  // front of the mask.  Finite and > 0; 0: no cap, the kernels above
  float softcap = 0.f;
};

// what awq_attn_kvcache_paged_shared[_kv8] takes beside attn_kvcache_paged's KvAttnCall (awq_shared.hpp)
struct KvSharedCall {
  const int* group_members = nullptr;  // device int32 [num_groups, group_cap], -1 padding
  const int* group_prefix = nullptr;   // device int32 [num_groups]
  const int* seq_prefix = nullptr;     // device int32 [B]
  long long members_row_stride = 0;
  int num_groups = 0, group_cap = 0, max_prefix = 0;
};

// awq_kv_page_copy[_fp8]: n (src, dst) page pairs of the pools in v (awq_paged.hpp), rows of Hkv * Dh elements or codes
struct KvPageCopyCall {
  KvView kv;  // the pools; k / v are written
  const int* src_pages;
  const int* dst_pages;
  int n, Hkv, Dh;
};

// Arguments validated by the caller.  awq_attn_chunk_cdna4.hip serves the T cache and hands a view with scales to
// awq_attn_kv8_cdna4.hip: each file keeps its own kernel and argument struct; the form and the grid come from awq_kvstore.hpp.  With
// cu_seqlens_q set, the packed-token store (awq_varq.hpp): device positions, dense or paged.
int launch_kv_store(const KvStoreCall& c, hipStream_t st);
int launch_kv_store_fp8(const KvStoreCall& c, hipStream_t st);
// the split launch and its combine (awq_attn_splitkv_cdna4.hip); the caller holds the plan and a workspace of the plan's size.  With
// cu_seqlens_q set and split_seqlen_q > 0, the packed forms of the pair: only the sequences the rule hands to them are touched, and the
// workspace has split_seqlen_q rows per (sequence, query head)
int launch_kv_attn(const KvAttnCall& c, int splits, int chunk, void* workspace, hipStream_t st);
// the three launches of a shared-prefix decode (awq_shared.hpp): prefix blocks, suffix blocks, combine; the plan is
// attn_kvcache_shared_plan's and the workspace has its size
int launch_kv_attn_shared(const KvAttnCall& c, const KvSharedCall& s, void* workspace, hipStream_t st);
// one launch: the K and V rows (and the scales of an FP8 pool) of n pages, 16 bytes per move
int launch_kv_page_copy(const KvPageCopyCall& c, hipStream_t st);
// the one-pass prefill kernel under device lengths, dense or paged (awq_attn_prefill_cdna4.hip): any seqlen_q, no workspace; with
// cu_seqlens_q set, its packed-query form; with split_seqlen_q > 0 the form that leaves the split pair's sequences alone
int launch_kv_prefill(const KvAttnCall& c, hipStream_t st);

// f(element traits, std::integral_constant<int, DH>) for dtype 0 / 1 (F16 / BF16 of awq_device.hpp) and Dh 128 / 64
template <typename F16T, typename BF16T, typename F>
void for_dtype_dh(int dtype, int Dh, F&& f) {
  if (dtype == 0) {
    if (Dh == 128) f(F16T{}, std::integral_constant<int, 128>{});
    else f(F16T{}, std::integral_constant<int, 64>{});
  } else {
    if (Dh == 128) f(BF16T{}, std::integral_constant<int, 128>{});
    else f(BF16T{}, std::integral_constant<int, 64>{});
  }
}

}  // namespace awq
