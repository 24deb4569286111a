// The natural-layout rope + store launch, the part both launchers share (host side): launch_kv_store (awq_attn_chunk_cdna4.hip, the T
// cache) and launch_kv_store_fp8 (awq_attn_kv8_cdna4.hip, codes and scales) serve the same forms of a KvStoreCall -- the rectangle [B, S]
// or a packed step (cu_seqlens_q set), host or device positions, dense caches or pools -- over the same grid.
#pragma once
#include "awq_kvcache.hpp"
#include "awq_varq.hpp"

namespace awq {

// blocks of 256 threads, one thread per 8 columns of a token, over the call's tokens -- the rectangle, or the total_q packed rows -- from
// host arguments only
inline unsigned kv_store_blocks(const KvStoreCall& c) {
  const long long tokens = c.cu_seqlens_q ? (long long)c.total_q : (long long)c.B * c.S;
  return (unsigned)((tokens * (c.Dh / 8) + 255) / 256);
}

// f(form) for the length traits the descriptor asks for; form.of<DT> is HostLen<DT>, DevLen<DT>, .., VarQPagedDevLen<DT>
template <template <typename> class L>
struct KvStoreForm {
  template <typename DT>
  using of = L<DT>;
};
template <typename F>
void for_kv_store_form(const KvStoreCall& c, F&& f) {
  if (c.cu_seqlens_q) {
    if (c.kv.block_table) f(KvStoreForm<VarQPagedDevLen>{});
    else f(KvStoreForm<VarQDevLen>{});
  } else if (c.kv.block_table) {
    f(KvStoreForm<PagedDevLen>{});
  } else if (c.cache_seqlens) {
    f(KvStoreForm<DevLen>{});
  } else {
    f(KvStoreForm<HostLen>{});
  }
}

}  // namespace awq
