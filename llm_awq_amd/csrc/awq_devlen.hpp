// Lengths on the device: the kernels of the natural-layout decode path (rope_kv_store_natural[_fp8], attn_splitkv and its combine) read
// each sequence's length from a device int32 array instead of taking one length for the whole batch as a launch argument
// (awq_rope_kv_store_natural_pos[_fp8], awq_attn_kvcache[_kv8]).  They select the form by the element traits -- DevLen<F16>,
// DevLen<Kv8<BF16>>, the same traits under another name, as Kv8<DT> and FtCache<DT> are -- so the host-length kernels keep their names and
// their code.
#pragma once
#include "awq_kv8.hpp"

namespace awq {

template <typename DT>
struct DevLen : DT {};
template <typename DT>
using HostLen = DT;  // lengths / positions from the host: the element traits themselves
template <typename DT>
struct IsDevLen {
  static constexpr bool value = false;
};
template <typename DT>
struct IsDevLen<DevLen<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsKv8<DevLen<Kv8<DT>>> {
  static constexpr bool value = true;
};

}  // namespace awq
