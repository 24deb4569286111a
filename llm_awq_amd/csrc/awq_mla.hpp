// The LATENT KV cache of multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2): one row of 576 T per token -- columns 0..511 the
// normalised latent c_kv, 512..575 the rotated shared key k_pe -- whatever the head count.  In the absorbed (decode) form every query head
// attends that one row with a 576-wide query (q_nope W_uk | rotated q_pe).  awq_attn_mla_cdna4.hip holds the store of a packed step; the C
// entry is awq_mla_kv_store (awq_capi.hip).  The attention over this cache is not in the tree yet.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace awq {

constexpr int kMlaLatent = 512;                 // kv_lora_rank of every published MLA model
constexpr int kMlaRope = 64;                    // qk_rope_head_dim
constexpr int kMlaRow = kMlaLatent + kMlaRope;  // a cache row, and a row of q_abs
constexpr int kMlaMaxHeads = 128;

// the latent cache of one call: dense [Bc, Lmax, 576] (block_table == nullptr) or a pool [num_pages, page_size, 576] behind a table
struct MlaCache {
  const void* c;           // T
  long long c_os, c_rs;    // outer (batch or page) and row strides, elements; c_rs >= 576
  int outer, rows;         // Bc, Lmax -- or num_pages, page_size
  const int* block_table;  // device int32 [>= B, pages_per_seq]
  long long bt_rs;
  int pages_per_seq;
};

struct MlaStoreCall {
  const void* kv_a;  // T [total_q, 576], row stride kv_rs
  const void* q_pe;  // T [total_q, H, 64], token stride q_ts, head stride q_hs
  void* q_abs;       // T [total_q, H, 576] contiguous: columns 512..575 are written
  MlaCache cache;
  const int* cu_seqlens_q;   // device int32 [B + 1]
  const int* cache_seqlens;  // device int32 [B]
  const float* freqs_table;  // fp32 [table_rows, 64]
  const float* gamma;        // fp32 [512]
  float eps;
  long long kv_rs, q_ts, q_hs;
  int B, H, total_q, max_seqlen_q, table_rows, rope_interleaved, dtype;
};

void launch_mla_kv_store(const MlaStoreCall& c, hipStream_t st);

}  // namespace awq
