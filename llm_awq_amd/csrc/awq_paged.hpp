// Paged KV cache: the natural-layout decode path (rope_kv_store_natural_pos[_fp8], attn_splitkv under device lengths) reading and writing a
// POOL of fixed-size pages through a per-sequence block table in the place of a dense [B, L, Hkv, Dh] rectangle
// (awq_rope_kv_store_paged_pos[_fp8], awq_attn_kvcache_paged[_kv8]).
//
//   k_pool / v_pool [num_pages, page_size, Hkv, Dh] of T or of e4m3 codes, a page stride and a row stride of their own, heads contiguous
//   scale pools     [num_pages, page_size, Hkv] fp32 (FP8 only), a page stride and a row stride of their own
//   block_table     device int32 [batch, pages_per_seq], a row stride of its own
//   logical key p of sequence b  =  row p % page_size of page block_table[b, p / page_size]
//
// page_size % 64 == 0: the split kernel walks keys in 64-key tiles that begin at multiples of 64 (every chunk is one), so a tile never
// straddles a page and its page id is ONE value for the whole block -- one scalar load per tile, looked up a tile ahead of the K / V loads
// that need it.  A page id is clamped into [0, num_pages) before it forms an address, and no table entry at or behind
// ceil(Sk_b / page_size) is read.
//
// The kernels select the form by the element traits -- Paged<DevLen<F16>>, Paged<DevLen<Kv8<BF16>>>, the same traits under another name,
// as DevLen<DT>, Kv8<DT> and FtCache<DT> are -- so the dense kernels keep their names and their code.
#pragma once
#include "awq_devlen.hpp"

namespace awq {

template <typename DT>
struct Paged : DT {};
template <typename DT>
using PagedDevLen = Paged<DevLen<DT>>;
template <typename DT>
struct IsPaged {
  static constexpr bool value = false;
};
template <typename DT>
struct IsPaged<Paged<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsDevLen<Paged<DT>> {
  static constexpr bool value = IsDevLen<DT>::value;
};
template <typename DT>
struct IsKv8<Paged<DT>> {
  static constexpr bool value = IsKv8<DT>::value;
};

// the launch arguments of a pool and its table that every paged kernel takes
struct PageArgs {
  const int* block_table;  // device int32 [batch, pages_per_seq]
  long long bt_rs;         // its row stride, entries
  int page_size, num_pages;
};

// entry idx of a sequence's table row, clamped into the pool.  idx is uniform over the block in the attention kernel (a scalar load).
__device__ __forceinline__ int page_id(const int* table_row, int idx, int num_pages) { return min(max(table_row[idx], 0), num_pages - 1); }
// the same clamp for an entry that was loaded earlier (the one-pass prefill kernel requests an entry a tile ahead and clamps it at its use)
__device__ __forceinline__ int page_id(int entry, int num_pages) { return min(max(entry, 0), num_pages - 1); }

}  // namespace awq
