// Packed queries ("varq"): the tokens of a call are one flat run of rows and sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1,
// so the sequences of ONE launch may bring different numbers of new tokens (awq_rope_kv_store_natural_varq[_fp8],
// awq_rope_kv_store_paged_varq[_fp8], awq_attn_prefill_kvcache_varq[_kv8], awq_attn_prefill_paged_varq[_kv8]).
//
//   cu_seqlens_q  device int32 [B + 1], non-decreasing, cu[0] = 0; never read by the host
//   Sq_b          cu[b + 1] - cu[b]; 0 is legal (a slot with nothing to do), a sequence with Sq_b > max_seqlen_q is inactive
//   total_q       rows of the packed tensors (host); rows >= cu[B] are the padding of a fixed token budget: neither read nor written
//   max_seqlen_q  the host's bound of every Sq_b; it sizes the attention grid
//
// A row index formed from cu_seqlens_q is clamped into [0, total_q - 1] before it forms an address and a write is guarded by
// row < min(cu[b + 1], total_q): a corrupt array gives unspecified results, never an address outside the tensors (the tower kernel's rule,
// awq_attn_tower_cdna4.hip).
//
// The kernels select the form by the element traits -- VarQ<DevLen<F16>>, VarQ<Paged<DevLen<Kv8<BF16>>>>, the same traits under another
// name, as Paged<DT>, DevLen<DT>, Kv8<DT> and FtCache<DT> are -- so the rectangular kernels keep their names and their code.
//
// A MIXED step (awq_attn_varq[_kv8], awq_attn_paged_varq[_kv8]) serves every sequence by exactly one of two kernels: the split-KV pair
// (VarQ<..> forms of awq_attn_splitkv_cdna4.hip) takes the short sequences over a long history, the one-pass kernel (VarQMix<..> forms of
// awq_attn_prefill_cdna4.hip) everything else.  Who serves a sequence is varq_split_takes below, evaluated by all three launches on what
// cu_seqlens_q and the lengths hold: the launch set never depends on the step.
#pragma once
#include "awq_paged.hpp"

namespace awq {

template <typename DT>
struct VarQ : DT {};
template <typename DT>
using VarQDevLen = VarQ<DevLen<DT>>;
template <typename DT>
using VarQPagedDevLen = VarQ<Paged<DevLen<DT>>>;
template <typename DT>
struct IsVarQ {
  static constexpr bool value = false;
};
template <typename DT>
struct IsVarQ<VarQ<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsPaged<VarQ<DT>> {
  static constexpr bool value = IsPaged<DT>::value;
};
template <typename DT>
struct IsDevLen<VarQ<DT>> {
  static constexpr bool value = IsDevLen<DT>::value;
};
template <typename DT>
struct IsKv8<VarQ<DT>> {
  static constexpr bool value = IsKv8<DT>::value;
};

// the one-pass kernel of a mixed step: VarQ in every respect, and a sequence the split pair takes is left alone
template <typename DT>
struct VarQMix : DT {};
template <typename DT>
using VarQMixDevLen = VarQMix<DevLen<DT>>;
template <typename DT>
using VarQMixPagedDevLen = VarQMix<Paged<DevLen<DT>>>;
template <typename DT>
struct IsVarQMix {
  static constexpr bool value = false;
};
template <typename DT>
struct IsVarQMix<VarQMix<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsVarQ<VarQMix<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsPaged<VarQMix<DT>> {
  static constexpr bool value = IsPaged<DT>::value;
};
template <typename DT>
struct IsDevLen<VarQMix<DT>> {
  static constexpr bool value = IsDevLen<DT>::value;
};
template <typename DT>
struct IsKv8<VarQMix<DT>> {
  static constexpr bool value = IsKv8<DT>::value;
};

// the launch arguments of a packed step that every varq kernel takes
struct VarQArgs {
  const int* cu_seqlens_q;  // device int32 [B + 1]
  int total_q, max_seqlen_q;
  int lens_before_step;  // attention only: Sk_b = seqlens_k[b] + Sq_b (the lengths the store launch took) instead of seqlens_k[b]
};

// the two host thresholds of a mixed step; a struct of its own behind VarQArgs, so that the argument blocks of the plain varq kernels stay
// what they were
struct VarQSplitArgs {
  int split_seqlen_q;  // the split pair takes at most this many new tokens; split_seqlen_q * (H / Hkv) <= 128
  int split_min_keys;  // .. over at least this many keys, >= 1
};

// Who serves sequence b of a mixed step.  sq_b = cu[b + 1] - cu[b] and sk_b = the length as the varq kernels form it (64 bits, with
// lens_before_step), both block-uniform.  true: the split pair; false: the one-pass kernel, exactly as in a plain varq launch -- inactive
// sequences (zero rows), Sq_b = 0 and prompt chunks among them.
__device__ __forceinline__ bool varq_split_takes(long long sq_b, long long sk_b, int max_seqlen_q, int max_seqlen_k, const VarQSplitArgs& sp) {
  const bool active = sq_b >= 1 && sq_b <= max_seqlen_q && sk_b >= 1 && sk_b <= max_seqlen_k;
  return active && sq_b <= sp.split_seqlen_q && sk_b >= sp.split_min_keys;
}

// cu_seqlens_q is read through the constant address space, as the block table is: nothing writes it while a kernel runs, and the loads
// of a block-uniform index stay scalar loads
typedef const int __attribute__((address_space(4))) * const_i32_t;
__device__ __forceinline__ const_i32_t as_const_i32(const int* p) { return reinterpret_cast<const_i32_t>(reinterpret_cast<uintptr_t>(p)); }

// The store kernels' lookup: the owner of packed token t >= 0, the sequence b with cu[b] <= t < cu[b + 1].  A binary search per thread that
// keeps cu[lo] <= t < cu[hi]: one load of cu[B] and at most 16 more for B <= 65535, every one an index inside [0, B] and a hit in the cache
// (the threads of a launch read the same few lines).  The LAST b with cu[b] <= t wins, so a token behind a run of zero-length sequences
// goes to its owner and not to one of them.  cu[0] = 0 is taken for granted, never loaded.  false: t >= cu[B], a padding row.  s and sq
// are 64 bits: whatever the array holds, 0 <= s < sq.
__device__ __forceinline__ bool varq_owner(const_i32_t cu, int B, int t, int& b, long long& s, long long& sq) {
  int lo = 0, hi = B, c_lo = 0, c_hi = cu[B];
  if (t >= c_hi) return false;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1, c = cu[mid];
    if (c <= t) lo = mid, c_lo = c;
    else hi = mid, c_hi = c;
  }
  b = lo;
  s = (long long)t - c_lo;
  sq = (long long)c_hi - c_lo;
  return true;
}

}  // namespace awq
