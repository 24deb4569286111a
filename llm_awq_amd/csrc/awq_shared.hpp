// Shared-prefix decode on the paged KV cache (awq_attn_kvcache_paged_shared[_kv8]): the sequences of a GROUP hold the same keys below a
// common prefix -- one system prompt or document, the n samples of one request, beams -- and the prefix is fetched from HBM once for the
// whole group in the place of once per sequence.
//
//   group_members  device int32 [num_groups, group_cap], a row stride of its own, -1 padding: the slots of group g in list order
//   group_prefix   device int32 [num_groups]: the tokens group g shares
//   seq_prefix     device int32 [batch]: the tokens sequence b shares with its group (0: ungrouped)
//   pfx(P, Sk) = min(P, max_prefix, max(0, Sk - Sq)) & ~63, 0 for P < 64: the effective prefix, a whole number of 64-key tiles that lies
//   below the causal limit of every query row of a sequence of Sk keys
//
// Three launches over one workspace of splits_p + splits_s entries per (sequence, query head, query position):
//   prefix   SharedPrefix<Paged<DevLen<..>>> of the split kernel, num_groups * Hkv * splits_p blocks.  The lead of group g is its first
//            member in list order that is a valid slot and active; P_g = pfx(group_prefix[g], Sk_lead).  Split s walks keys
//            [s * chunk_p, min(P_g, (s + 1) * chunk_p)) through the LEAD's table row with the query rows of all members in the MFMA tile,
//            packed row = (j * Sq + i) * G + gh, and no mask.  The partial of a row of member m lands in entry s of m's workspace rows.
//   suffix   SharedSuffix<Paged<DevLen<..>>>, batch * Hkv * splits_s blocks: attn_kvcache_paged's block with its splits anchored at
//            P_b = pfx(seq_prefix[b], Sk_b), the way awq_window.hpp anchors them at the window; entry splits_p + s.
//   combine  SharedCombine<DevLen<..>>: the dense rule over the first ceil(P_b / chunk_p) prefix entries, then every suffix entry.
//
// A row's partial depends only on its q row, its keys and the split boundaries -- not on the other rows of the MFMA tile, and not on
// the table the keys came through.  With chunk_p == chunk_s == c and P_b % c == 0 the entries a sequence combines are therefore the
// entries awq_attn_kvcache_paged[_kv8] combines under chunk c, in the same order: the same bits.
//
// The kernels select the form by the element traits, as Window<>, VarQ<>, Paged<> and DevLen<> do: the unshared kernels keep their names,
// their argument blocks and their code.
#pragma once
#include "awq_paged.hpp"

namespace awq {

template <typename DT>
struct SharedPrefix : DT {};
template <typename DT>
struct SharedSuffix : DT {};
template <typename DT>
struct SharedCombine : DT {};
template <typename DT>
using SharedPrefixPagedDevLen = SharedPrefix<Paged<DevLen<DT>>>;
template <typename DT>
using SharedSuffixPagedDevLen = SharedSuffix<Paged<DevLen<DT>>>;
template <typename DT>
using SharedCombineDevLen = SharedCombine<DevLen<DT>>;
template <typename DT>
struct IsSharedPrefix {
  static constexpr bool value = false;
};
template <typename DT>
struct IsSharedPrefix<SharedPrefix<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsSharedSuffix {
  static constexpr bool value = false;
};
template <typename DT>
struct IsSharedSuffix<SharedSuffix<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsSharedCombine {
  static constexpr bool value = false;
};
template <typename DT>
struct IsSharedCombine<SharedCombine<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsShared {
  static constexpr bool value = IsSharedPrefix<DT>::value || IsSharedSuffix<DT>::value || IsSharedCombine<DT>::value;
};
#define AWQ_SHARED_FORWARD(Trait)                   \
  template <typename DT>                            \
  struct Trait<SharedPrefix<DT>> {                  \
    static constexpr bool value = Trait<DT>::value; \
  };                                                \
  template <typename DT>                            \
  struct Trait<SharedSuffix<DT>> {                  \
    static constexpr bool value = Trait<DT>::value; \
  };                                                \
  template <typename DT>                            \
  struct Trait<SharedCombine<DT>> {                 \
    static constexpr bool value = Trait<DT>::value; \
  };
AWQ_SHARED_FORWARD(IsPaged)
AWQ_SHARED_FORWARD(IsDevLen)
AWQ_SHARED_FORWARD(IsKv8)
#undef AWQ_SHARED_FORWARD

// the launch arguments of the group arrays; a struct of its own behind the argument structs of the unshared kernels, never inside them
struct SharedArgs {
  const int* group_members;  // device int32 [num_groups, group_cap]
  long long gm_rs;           // its row stride, entries
  const int* group_prefix;   // device int32 [num_groups]
  const int* seq_prefix;     // device int32 [batch]
  int num_groups, group_cap, max_prefix;
  int splits_p, chunk_p;     // the prefix plan (the combine skips prefix entries at and behind ceil(P_b / chunk_p))
  int ws_splits, ws_first;   // workspace entries per row (splits_p + splits_s) and the launch's first entry (prefix 0, suffix splits_p)
};

// the effective prefix of a sequence of sk keys (1 <= sk) that brings sq query rows
__host__ __device__ __forceinline__ int shared_pfx(int p, int max_prefix, int sk, int sq) {
  const int room = sk > sq ? sk - sq : 0;
  int e = p < max_prefix ? p : max_prefix;
  e = e < room ? e : room;
  return e > 0 ? e & ~63 : 0;
}

}  // namespace awq
