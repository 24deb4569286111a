// The latent KV cache of multi-head latent attention (awq_mla.hpp): the store of a packed step.
//
//   cache row p of a sequence: [ rmsnorm(kv_a[0:512]) * gamma | rope(kv_a[512:576]) ]        576 T per token, whatever the head count
//   q_abs[t, h, 512:576]     : rope(q_pe[t, h])                                              the rope columns of the absorbed query
//
// mla_kv_store_kernel, one launch: one WAVE per packed token.  The 64 lanes hold the 64 16-byte chunks of the raw latent, so the sum of
// squares is rmsnorm_kernel's on a row of K = 512, bit for bit: each lane folds its 8 columns in ascending order with fmaf from 0, the
// lanes combine with ss += __shfl_xor(ss, d), d = 1 .. 32 (that kernel's other three waves hold 0), rstd = rsqrtf(ss / 512 + eps),
// y = T((x * rstd) * gamma), one rounding.  The same wave then rotates k_pe and the H q_pe heads, a lane per (head, 8 columns), with
// awq_rope.hpp's expression.  rope_interleaved: the pairs of the INPUT are (2 i, 2 i + 1) (DeepSeek's checkpoint order); the lane of
// output columns c0 .. c0 + 7 reads the 16 input columns 2 (c0 & 31) .. + 15 and takes the even ones as x and the odd ones as partner
// (first half) or the other way round (second half): the non-interleaved rotation of the input permuted to [0, 2, .., 62, 1, 3, .., 63],
// so q and k come out in half-split order alike.  The token's owner is varq_owner's; an inactive sequence (cache_seqlens[b] < 0,
// Sq_b > max_seqlen_q, or the chunk does not fit the cache / the table of angles) stores nothing and gets zero q_pe columns; rows
// >= cu[B] are neither read nor written.  16-byte loads and stores throughout; no atomics, no host read of a device array.
#include "awq_mla.hpp"

#include "awq_device.hpp"
#include "awq_rope.hpp"
#include "awq_varq.hpp"

#include <math.h>

namespace awq {
namespace {

struct StoreArgs {
  const uint16_t* kv_a;
  const uint16_t* q_pe;
  uint16_t* q_abs;
  uint16_t* c;
  const int* cu;
  const int* lens;
  const int* table;
  const float* freqs;
  const float* gamma;
  long long kv_rs, q_ts, q_hs, c_os, c_rs, bt_rs;
  int B, H, total_q, max_q, table_rows, interleaved, rows, pages_per_seq, num_pages;
  float eps;
};

template <typename DT, bool PAGED>
__global__ __launch_bounds__(256) void mla_kv_store_kernel(StoreArgs a) {
  const int lane = threadIdx.x & 63;
  const long long tl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tl >= a.total_q) return;
  const int t = (int)tl;
  int b = 0;
  long long s = 0, sq = 0;
  if (!varq_owner(as_const_i32(a.cu), a.B, t, b, s, sq)) return;  // padding behind cu[B]
  const long long cs = a.lens[b];
  const long long cap = PAGED ? (long long)a.pages_per_seq * a.rows : (long long)a.rows;
  const bool active = cs >= 0 && sq <= a.max_q && cs + sq <= min(cap, (long long)a.table_rows);
  uint16_t* qa = a.q_abs + (long long)t * a.H * kMlaRow;
  const int c0 = (lane & 7) * 8;  // the lane's rope columns, the same in every round of the head loop
  if (!active) {
    for (int j = lane; j < a.H * 8; j += 64) *reinterpret_cast<u32x4*>(qa + (long long)(j >> 3) * kMlaRow + kMlaLatent + c0) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const long long pos = cs + s;  // < cap, < table_rows
  uint16_t* crow;
  if constexpr (PAGED) {
    const int pi = (int)(pos / a.rows);
    const int page = page_id(a.table + (long long)b * a.bt_rs, pi, a.num_pages);
    crow = a.c + (long long)page * a.c_os + (pos - (long long)pi * a.rows) * a.c_rs;
  } else {
    crow = a.c + (long long)b * a.c_os + pos * a.c_rs;
  }
  const uint16_t* src = a.kv_a + (long long)t * a.kv_rs;

  // ---- the latent: rmsnorm_kernel's arithmetic on a row of 512 ----
  {
    float x[8];
    unpack8<DT>(*reinterpret_cast<const u32x4*>(src + 8 * lane), x);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) ss += __shfl_xor(ss, d, 64);
    const float rstd = rsqrtf(ss / (float)kMlaLatent + a.eps);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + 8 * lane), g1 = *reinterpret_cast<const f32x4*>(a.gamma + 8 * lane + 4);
    const float g[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
    u32 w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = (u32)qk_norm_round<DT>(x[2 * e], rstd, g[2 * e]) | ((u32)qk_norm_round<DT>(x[2 * e + 1], rstd, g[2 * e + 1]) << 16);
    *reinterpret_cast<u32x4*>(crow + 8 * lane) = u32x4{w[0], w[1], w[2], w[3]};
  }

  // ---- the rotations: task j = (head j >> 3, columns c0 .. c0 + 7); head 0 is k_pe, head 1 + h is q head h ----
  const RopeLane rl(a.freqs + pos * kMlaRope + c0, c0, kMlaRope);
  const int ib = 2 * (c0 & 31);  // interleaved: the first of the 16 input columns
  for (int j = lane; j < (a.H + 1) * 8; j += 64) {
    const int hd = j >> 3;
    const uint16_t* in = hd == 0 ? src + kMlaLatent : a.q_pe + (long long)t * a.q_ts + (long long)(hd - 1) * a.q_hs;
    uint16_t* dst = hd == 0 ? crow + kMlaLatent : qa + (long long)(hd - 1) * kMlaRow + kMlaLatent;
    u32x4 bits;
    if (a.interleaved) {
      float lo[8], hi[8], x[8], y[8], res[8];
      unpack8<DT>(*reinterpret_cast<const u32x4*>(in + ib), lo);
      unpack8<DT>(*reinterpret_cast<const u32x4*>(in + ib + 8), hi);
      const bool first = c0 < kMlaRope / 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ev = e < 4 ? lo[2 * e] : hi[2 * e - 8], od = e < 4 ? lo[2 * e + 1] : hi[2 * e - 7];
        x[e] = first ? ev : od;
        y[e] = first ? od : ev;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) res[e] = __builtin_fmaf(x[e], rl.cs[e], (rl.sign * y[e]) * rl.sn[e]);
      bits = pack8<DT>(res);
    } else {
      bits = rl.template rotate<DT>(in, c0);
    }
    *reinterpret_cast<u32x4*>(dst + c0) = bits;
  }
}

template <typename DT>
void launch_store_t(const MlaStoreCall& c, hipStream_t st) {
  const MlaCache& k = c.cache;
  const StoreArgs a{(const uint16_t*)c.kv_a, (const uint16_t*)c.q_pe, (uint16_t*)c.q_abs, (uint16_t*)const_cast<void*>(k.c), c.cu_seqlens_q, c.cache_seqlens,
                    k.block_table, c.freqs_table, c.gamma, c.kv_rs, c.q_ts, c.q_hs, k.c_os, k.c_rs, k.bt_rs, c.B, c.H, c.total_q, c.max_seqlen_q,
                    c.table_rows, c.rope_interleaved, k.rows, k.pages_per_seq, k.outer, c.eps};
  const unsigned blocks = (unsigned)(((long long)c.total_q + 3) / 4);
  if (k.block_table) hipLaunchKernelGGL((mla_kv_store_kernel<DT, true>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((mla_kv_store_kernel<DT, false>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

void launch_mla_kv_store(const MlaStoreCall& c, hipStream_t st) {
  if (c.dtype == 0) launch_store_t<F16>(c, st);
  else launch_store_t<BF16>(c, st);
}

}  // namespace awq
