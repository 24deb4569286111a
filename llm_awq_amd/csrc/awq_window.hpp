// Sliding-window attention on packed steps (awq_attn_varq_window[_kv8], awq_attn_paged_varq_window[_kv8]): flash-attn's
// window_size = (left, 0) under the bottom-right aligned causal mask of the packed kernels.
//
//   row s of sequence b stands at position p = s + Sk_b - Sq_b and attends keys j with max(0, p - left) <= j <= p
//   Sk_b as the varq kernels form it (64 bits, with lens_before_step); p < 0: zeros, as without a window.  Every other row attends at
//   least its own key: a window makes no new empty rows.  left >= max_seqlen_k - 1 is no window at all (the host clamps left to that).
//
// The kernels select the form by the element traits -- Window<VarQMix<..>> of the one-pass kernel, Window<VarQ<..>> of the split pair, the
// same traits under another name, as VarQ<DT>, Paged<DT>, DevLen<DT> and Kv8<DT> are -- so the unwindowed kernels keep their names, their
// argument blocks and their code.  No rectangular, host-length, FT or tower form takes a window.
//
// The one-pass kernel starts its tile walk at the tile of the block's first key, a_blk = max(0, q0 + Sk_b - Sq_b - left); the split pair
// anchors its splits there instead of at key 0 (window_anchor below).  Neither reads a key, a scale or a table entry below that tile:
// pages wholly below it are dead to every later step and may go back to the pool (PageTable.release_before).
#pragma once
#include "awq_varq.hpp"

namespace awq {

template <typename DT>
struct Window : DT {};
template <typename DT>
using WindowVarQDevLen = Window<VarQ<DevLen<DT>>>;
template <typename DT>
using WindowVarQPagedDevLen = Window<VarQ<Paged<DevLen<DT>>>>;
template <typename DT>
using WindowVarQMixDevLen = Window<VarQMix<DevLen<DT>>>;
template <typename DT>
using WindowVarQMixPagedDevLen = Window<VarQMix<Paged<DevLen<DT>>>>;
template <typename DT>
struct IsWindow {
  static constexpr bool value = false;
};
template <typename DT>
struct IsWindow<Window<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsVarQ<Window<DT>> {
  static constexpr bool value = IsVarQ<DT>::value;
};
template <typename DT>
struct IsVarQMix<Window<DT>> {
  static constexpr bool value = IsVarQMix<DT>::value;
};
template <typename DT>
struct IsPaged<Window<DT>> {
  static constexpr bool value = IsPaged<DT>::value;
};
template <typename DT>
struct IsDevLen<Window<DT>> {
  static constexpr bool value = IsDevLen<DT>::value;
};
template <typename DT>
struct IsKv8<Window<DT>> {
  static constexpr bool value = IsKv8<DT>::value;
};

// the one launch argument of a window; a struct of its own behind the argument structs of the unwindowed kernels, never inside them
struct WindowArgs {
  int left;  // 0 <= left <= max_seqlen_k - 1 (clamped by the host)
};

// keys_b: how many keys sequence b attends at all, rows [Sk_b - Sq_b - left, Sk_b) clipped at key 0.  64 bits.
__host__ __device__ __forceinline__ long long window_keys(long long sq_b, long long sk_b, int left) {
  const long long w = (long long)left + sq_b;
  return sk_b < w ? sk_b : w;
}

// Who serves sequence b of a windowed mixed step: varq_split_takes with keys_b in the place of Sk_b -- a decode over a long history with a
// short window is no longer "long".  Evaluated by all three launches; block-uniform.  true: the split pair.
__device__ __forceinline__ bool varq_window_split_takes(long long sq_b, long long sk_b, int max_seqlen_q, int max_seqlen_k, const VarQSplitArgs& sp,
                                                        const WindowArgs& w) {
  const bool active = sq_b >= 1 && sq_b <= max_seqlen_q && sk_b >= 1 && sk_b <= max_seqlen_k;
  return active && sq_b <= sp.split_seqlen_q && window_keys(sq_b, sk_b, w.left) >= sp.split_min_keys;
}

// The split pair's anchor: the 64-key tile that holds the window start of the sequence's FIRST row.  Split s owns keys
// [anchor + s * chunk, min(Sk_b, .. + chunk)); Sk_b - anchor <= left + Sq_b + 63, the bound awq_attn_varq_window_plan plans for.
__device__ __forceinline__ int window_anchor(int sq_b, int sk_b, int left) {
  const long long a = (long long)sk_b - sq_b - left;
  return a > 0 ? (int)a & ~63 : 0;
}

// the plan's bound: the most keys an anchored walk can cover
inline int window_plan_bound(int split_seqlen_q, int max_seqlen_k, int left) {
  const long long w = (long long)left + split_seqlen_q + 63;
  return w < max_seqlen_k ? (int)w : max_seqlen_k;
}

}  // namespace awq
