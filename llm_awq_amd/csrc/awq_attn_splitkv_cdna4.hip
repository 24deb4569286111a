// Split-KV attention (flash-decoding) for flash_attn_func's natural layout: a few query rows over a long history.
//
//   O = softmax(scale * Q K^T + mask) V        q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh], out [B, Sq, H, Dh]
//   awq_attn_prefill's contract (bottom-right aligned causal mask, query head h reads KV head h / G, G = H / Hkv), restricted to
//   R = Sq * G <= 128 packed rows per KV head.  This is the whole decode phase of tinychat's long-context path (fused_attn.py:505-546):
//   at Sq = 1 the one-pass kernel runs B * H blocks, each walking all of K / V for one live MFMA row, the G heads of a group each
//   fetching the same keys again.
//
// Two launches, no atomics:
//   1. attn_splitkv_kernel, B * Hkv * splits blocks.  One block = one (batch, KV head, split): keys [split * chunk, min(Sk, .. + chunk)),
//      chunk % 64 == 0, walked in the prefill kernel's 64-key tiles (same LDS images and swizzles k_off / v_off, same double buffering
//      through registers, same MFMA operand layouts, restated here so that the prefill unit stays untouched).  The MFMA query rows
//      are the R rows of the KV head's group, packed row = i * G + g (query position i, head g of the group): K and V of the chunk are
//      fetched from HBM ONCE for the whole group.  Wave w owns packed rows 32 w .. 32 w + 31.  Rounding points are the prefill
//      kernel's: fp32 scores and accumulation on v_mfma_f32_32x32x16, every weight rounded to T once, that rounded value feeding both
//      P.V and the row sum.  The block writes, per (row, split), an UNNORMALISED fp32 partial: O [Dh], the running max m (of the
//      scaled base-2 logits) and the row sum l.  A row that attends nothing of the chunk (causal: the last chunk is shorter than
//      Sq - 1 - i keys) writes O = 0, l = 0, m = -inf.  Rows >= Sk of k / v are never read: address clamped to Sk - 1, score masked.
//   2. attn_splitkv_combine_kernel: one thread = 8 columns of one row.  M = max_s m_s; O = sum_s 2^(m_s - M) O_s and
//      L = sum_s 2^(m_s - M) l_s in ascending split order (fmaf, fp32); out = T(O * (1 / L)): one division, one rounding.  A partial
//      with m_s = -inf is skipped: it contributes exactly nothing and no Inf - Inf is ever formed.  Split 0 holds key 0, which every
//      row attends, so M is finite and L > 0.
//
// Workspace (fp32, 16-byte aligned), n = B * Hkv * R * splits = B * H * Sq * splits entries, entry e = ((b * Hkv + kvh) * R + row) * splits + s:
//      O [n][Dh] | m [n] | l [n]                                   = n * (Dh + 2) * 4 bytes
//
// Work split inside a block -- the form kept: row split, every wave staging.  All 4 waves of a block load and stage every K / V
// tile; only the ceil(R / 32) waves that own rows compute.  At R <= 32 three waves are then load helpers.  The alternative (the waves
// split the chunk's key tiles, partials merged in LDS in wave order) keeps four tiles per block in LDS at once -- four times the LDS
// per block, one resident block per CU at Dh = 128 -- for the same bytes in flight per CU, and the compute it would spread (32 MFMAs and
// one 64-key softmax per tile on one wave) is several times shorter than the HBM time of a tile at one or two blocks per CU.  This is
// reasoning from the code, not an A/B: the key-split form was not built.  tools/splitkv_attn_bench.py times the kernel as a whole
// (README.md: 0.46 of 8 TB/s at 131072 keys, 16x the one-pass kernel at 32768 keys, Llama-3-8B, one token).
//
// awq_attn_kvcache[_kv8] is the same pair with every sequence's length read on the device (DevLen<..> instantiations, awq_devlen.hpp): the
// grid and the chunk come from a host bound (attn_kvcache_plan), blocks beyond a sequence's length leave at once, and the pair runs for
// any number of splits.  tools/kvcache_attn_bench.py prices it (README.md "Device-side lengths").
//
// awq_attn_kvcache_paged[_kv8] is that pair again with K / V (and the scales) fetched from a pool of pages through a block table
// (Paged<DevLen<..>> instantiations of the split kernel, awq_paged.hpp; the combine launch is the dense form's).
//
// awq_attn_varq[_kv8] / awq_attn_paged_varq[_kv8] run the pair inside a PACKED step (VarQ<..> instantiations of both kernels, awq_varq.hpp):
// q / out are packed rows, sequence b brings Sq_b = cu[b + 1] - cu[b] of them, and the pair serves only the sequences varq_split_takes
// hands to it -- few new tokens over a long history.  Every other sequence belongs to the one-pass launch of the same call.
//
// awq_attn_kvcache_paged_shared[_kv8] is the paged pair for sequences that share a prefix (Shared..<..> instantiations, awq_shared.hpp):
// a prefix launch of the split kernel with the query rows of a whole GROUP in its tile, a suffix launch anchored behind each
// sequence's prefix, and the combine over both sets of partials.
#include "awq_device.hpp"
#include "awq_devlen.hpp"
#include "awq_kernels.hpp"
#include "awq_kv8.hpp"
#include "awq_kvcache.hpp"
#include "awq_paged.hpp"
#include "awq_shared.hpp"
#include "awq_varq.hpp"
#include "awq_softcap.hpp"
#include "awq_window.hpp"

#include <math.h>
#include <string.h>

#include <type_traits>

namespace awq {
namespace {

constexpr int kKV = 64;        // keys per tile
constexpr int kMfmaRows = 32;  // packed rows per wave
constexpr int kNW = 4;         // waves per block
constexpr int kMaxRows = kNW * kMfmaRows;
constexpr int kCUs = 256;      // the MI355X; a constant because the plan is a host-only function that CPU tests pin
constexpr int kMinKeys = 2048;   // below this the one-pass kernel serves (a walk of <= 32 tiles is not worth a second launch)
constexpr int kMinChunk = 1024;  // keys per split of the plan, at least
int g_force_chunk = 0;         // knob attn_splitkv_chunk (awq_tune_set): a multiple of 64 forces the chunk, 0 = the plan

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

struct SplitArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* out;
  float* ws_o;
  float* ws_m;
  float* ws_l;
  long long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;  // elements
  int B, Sq, Sk, H, Hkv, G, R, splits, chunk, causal;
  float scale_log2e;
  // Kv8 only (awq_kv8.hpp): the scales [B, Sk, Hkv] of the e4m3 codes k / v point at, batch / row strides in floats; k_bs .. v_rs are then
  // in codes (bytes)
  const float* k_scale;
  const float* v_scale;
  long long ks_bs, ks_rs, vs_bs, vs_rs;
  // DevLen only (awq_devlen.hpp): the length of sequence b is seqlens_k[b] + seqlen_offset, read by the kernel; Sk above is then the
  // host's bound max_seqlen_k, which sized the grid
  const int* seqlens_k;
  int seqlen_offset;
};
// Paged only (awq_paged.hpp): k / v are the pools, k_bs / v_bs (ks_bs / vs_bs) their PAGE strides.  A struct of its own, so that the
// argument block of the dense kernels -- and with it their register assignment and schedule -- stays what it was.
struct PagedSplitArgs : SplitArgs {
  PageArgs pg;
};
// VarQ only (awq_varq.hpp): q / out are the packed rows, Sq the host's split_seqlen_q and R = split_seqlen_q * G the workspace rows per
// (sequence, KV head); the dense form carries an unused pg.  A struct of its own again, for both kernels of the pair.
struct VarQSplitKArgs : PagedSplitArgs {
  VarQArgs vq;
  VarQSplitArgs sp;
};
// Window<VarQ<..>> only (awq_window.hpp): the window behind everything above, for both kernels of the pair
struct WindowSplitKArgs : VarQSplitKArgs {
  WindowArgs w;
};
// Softcap<Window<VarQ<..>>> only (awq_softcap.hpp): the cap behind the window, for the split kernel alone -- the combine is the windowed one
struct SoftcapSplitKArgs : WindowSplitKArgs {
  SoftcapArgs cap;
};
// Shared<..> only (awq_shared.hpp): the group arrays behind the paged arguments, for all three launches of the call
struct SharedSplitArgs : PagedSplitArgs {
  SharedArgs sh;
};
template <typename DT>
using SplitArgsOf = typename std::conditional<
    IsShared<DT>::value, SharedSplitArgs,
    typename std::conditional<
        IsSoftcap<DT>::value, SoftcapSplitKArgs,
        typename std::conditional<
            IsWindow<DT>::value, WindowSplitKArgs,
            typename std::conditional<IsVarQ<DT>::value, VarQSplitKArgs,
                                      typename std::conditional<IsPaged<DT>::value, PagedSplitArgs, SplitArgs>::type>::type>::type>::type>::type;
template <typename DT>
using CombineArgsOf = typename std::conditional<
    IsShared<DT>::value, SharedSplitArgs,
    typename std::conditional<IsWindow<DT>::value, WindowSplitKArgs,
                              typename std::conditional<IsVarQ<DT>::value, VarQSplitKArgs, SplitArgs>::type>::type>::type;
__device__ __forceinline__ SharedArgs shared_args(const SplitArgs&) { return SharedArgs{nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ SharedArgs shared_args(const SharedSplitArgs& a) { return a.sh; }
__device__ __forceinline__ VarQArgs varq_args(const SplitArgs&) { return VarQArgs{nullptr, 0, 0, 0}; }
__device__ __forceinline__ VarQArgs varq_args(const VarQSplitKArgs& a) { return a.vq; }
__device__ __forceinline__ VarQSplitArgs split_args(const SplitArgs&) { return VarQSplitArgs{0, 0}; }
__device__ __forceinline__ VarQSplitArgs split_args(const VarQSplitKArgs& a) { return a.sp; }
__device__ __forceinline__ WindowArgs window_args(const SplitArgs&) { return WindowArgs{0}; }
__device__ __forceinline__ WindowArgs window_args(const WindowSplitKArgs& a) { return a.w; }
__device__ __forceinline__ SoftcapArgs cap_args(const SplitArgs&) { return SoftcapArgs{0.f, 0.f}; }
__device__ __forceinline__ SoftcapArgs cap_args(const SoftcapSplitKArgs& a) { return a.cap; }
__device__ __forceinline__ PageArgs page_args(const SplitArgs&) { return PageArgs{nullptr, 0, 0, 0}; }
__device__ __forceinline__ PageArgs page_args(const PagedSplitArgs& a) { return a.pg; }

// LDS images of awq_attn_prefill_cdna4.hip, restated: rows of DH elements, the 16-byte chunks of a row permuted by an XOR of the row.
//   K (read by rows, ds_read_b128, 16 consecutive lanes = 16 consecutive rows, one chunk): the 16 rows land on 16 different 16-byte slots
//   V (transposed reads, a 32-lane half = 4 consecutive rows x 64 bytes): the 4 rows land on 4 different 64-byte quarters of the banks
template <int DH>
__device__ __forceinline__ int k_off(int row, int ch) {
  return row * DH + ((ch ^ (DH == 128 ? (row & 15) : ((row >> 1) & 7))) << 3);
}
template <int DH>
__device__ __forceinline__ int v_off(int row, int ch) {
  return row * DH + ((ch ^ (DH == 128 ? (((row & 3) << 2) | ((row >> 2) & 3)) : (((row >> 1) & 1) << 2))) << 3);
}

// Kv8<DT> (awq_kv8.hpp) is the FP8 cache: the staging loads the 8 code bytes of the thread's chunk and the row's scale (same
// c = tid + i * NT mapping, same clamp to Sk - 1), dequantises T(float(code) * s) and writes the same 16 bytes into the same LDS slot.
// The 8-byte form is the one kept in both attention kernels (the reason is the prefill kernel's: awq_attn_prefill_cdna4.hip).
//
// DevLen<..> (awq_devlen.hpp, awq_attn_kvcache): Sk_b = seqlens_k[b] + seqlen_offset stands wherever a.Sk stands in the host-length form.
// A block whose sequence is inactive (Sk_b < 1 or Sk_b > a.Sk, the bound) or whose first key lies at or beyond Sk_b is EMPTY: it writes
// m = -inf, l = 0 for its rows and leaves before its first load of q, K, V or a scale.  The test is uniform over the block (b comes from
// blockIdx, the length is one scalar load) and no barrier precedes it.  A ragged batch therefore costs what its lengths cost.
//
// Paged<DevLen<..>> (awq_paged.hpp, awq_attn_kvcache_paged): key g of the sequence is row g % page_size of page table[b][g / page_size].  A
// tile begins at a multiple of 64 and page_size % 64 == 0, so the 64 keys of a tile (and the clamp to Sk_b - 1, which stays inside the
// tile) share ONE page: its id is uniform over the block, one scalar load per tile.  The ids run a tile ahead of the loads that use them:
// tile t + 1's K / V loads of iteration t take an id that was loaded in iteration t - 1 (the first two in front of the loop), so no table
// load stands between a barrier and the K / V loads behind it.  (pg_i, pg_ro) = (table index, first row inside the page) of the tile last
// looked up; they advance by 64 rows, so the one division is the block's first.  Only tiles j < nt are looked up: their first key lies
// below Sk_b, so no entry at or behind ceil(Sk_b / page_size) is read.  Everything behind the staging loads is the dense kernel.
//
// VarQ<DevLen<..>> / VarQ<Paged<DevLen<..>>> (awq_varq.hpp, a mixed step): the head of the block loads cu[b] and cu[b + 1] through the
// constant address space, then the length, and evaluates varq_split_takes.  Not taken: the block returns before any vector load and writes
// nothing, not even to the workspace.  Taken with k_begin >= Sk_b: m = -inf, l = 0 for its R_b rows, as the DevLen form.  Otherwise the
// DevLen / Paged kernel with Sq = Sq_b and R = R_b = Sq_b * G (block-uniform) and the q row cu[b] + qi, clamped into [0, total_q - 1].
// Every early exit is uniform over the block and stands in front of the first barrier.  The workspace keeps a.R = split_seqlen_q * G rows
// per (sequence, KV head); rows >= R_b are neither written nor read.
//
// Window<VarQ<..>> (awq_window.hpp, a windowed mixed step): the rule is varq_window_split_takes, and the splits are anchored at the window and
// not at key 0 -- k_begin = anchor_b + split * chunk with anchor_b = max(0, Sk_b - Sq_b - left) & ~63, block-uniform, one scalar expression
// behind the length load.  A split with k_begin >= Sk_b is empty, as above; no key and no table entry below anchor_b is read (the page walk
// begins at k_begin already).  Row i attends keys max(0, lim - left) .. lim: a tile wholly below the wave's first window start is skipped by
// a wave-uniform test, the low mask runs only in tiles below the wave's last window start, and a row whose window starts behind the
// split's last key leaves m = -inf, l = 0 for that split, which the combine skips.  Every row attends its own key, so some split's m is finite.
//
// Softcap<Window<VarQ<..>>> (awq_softcap.hpp, a capped windowed step): the windowed block with the logit
// x = cap_log2e * softcap_tanh(s * scale_over_cap) in the place of x = s * scale_log2e; the mask selects behind it, as without a cap.
//
// SharedSuffix<Paged<DevLen<..>>> (awq_shared.hpp, awq_attn_kvcache_paged_shared): the Paged block with k_begin = P_b + split * chunk,
// P_b = pfx(seq_prefix[b], Sk_b) one scalar expression behind the length load, and its partial in entry ws_first + split of the
// workspace's ws_splits entries per row.  No key, scale or table entry below P_b is read (the page walk begins at k_begin).
// SharedPrefix<Paged<DevLen<..>>>: the block is (group, KV head, prefix split).  Its head loads group_prefix[g] (below 64: the block
// leaves), then the member list through the constant address space, lane j of EVERY wave member j (j + 64 in a second round): the first
// set bit of one ballot of "valid slot and active" names the lead, the same in every wave, and its slot and length are read from that
// lane.  No lead, or k_begin >= P_g = pfx(group_prefix[g], Sk_lead): the block leaves, writing nothing.  Otherwise the Paged block with
// Sk = P_g (a multiple of 64: the clamp and the mask are idle), no causal mask, the lead's table row, and R = group_cap * Sq * G rows:
// packed row (j * Sq + i) * G + gh reads q of member j's slot, clamped into [0, B - 1], and is stored -- into THAT slot's workspace rows
// -- only when member j is a valid, active slot.  Every exit is block-uniform and stands in front of the first barrier.
template <typename DT, int DH>
__global__ __launch_bounds__(kNW * 64) void attn_splitkv_kernel(SplitArgsOf<DT> a) {
  constexpr bool KV8 = IsKv8<DT>::value;
  constexpr bool DEVLEN = IsDevLen<DT>::value;
  constexpr bool PAGED = IsPaged<DT>::value;
  constexpr bool VARQ = IsVarQ<DT>::value;
  constexpr bool WINDOW = IsWindow<DT>::value;
  constexpr bool SOFTCAP = IsSoftcap<DT>::value;
  static_assert(!SOFTCAP || WINDOW, "a cap exists on the windowed form only");
  static_assert(!PAGED || DEVLEN, "the paged form reads its lengths on the device");
  static_assert(!VARQ || DEVLEN, "packed queries read their lengths on the device");
  static_assert(!WINDOW || VARQ, "a window exists on the packed form only");
  constexpr bool SH_PFX = IsSharedPrefix<DT>::value, SH_SFX = IsSharedSuffix<DT>::value;
  static_assert(!(SH_PFX || SH_SFX) || (PAGED && !VARQ), "a shared prefix exists on the rectangular paged form only");
  using vec8 = typename DT::vec8;
  using elem = typename DT::elem;
  constexpr int NT = kNW * 64;
  constexpr int CPR = DH / 8;            // 16-byte chunks per row
  constexpr int LOADS = kKV * CPR / NT;  // chunks of one K (or V) tile per thread
  constexpr int KS = DH / 16;            // k-steps of Q K^T
  constexpr int DB = DH / 32;            // 32-column blocks of O
  static_assert(LOADS >= 1 && LOADS * NT == kKV * CPR, "tile does not divide over the block");
  __shared__ __attribute__((aligned(16))) uint16_t k_s[2][kKV * DH];
  __shared__ __attribute__((aligned(16))) uint16_t v_s[2][kKV * DH];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bi = blockIdx.x;
  const int split = bi % a.splits;
  bi /= a.splits;
  const int kvh = bi % a.Hkv;
  const int b = bi / a.Hkv;                             // SharedPrefix: the group
  // Shared: the workspace holds ws_splits entries per row, this launch's from ws_first on.  (A macro, and the constexpr selects below:
  // every unshared form keeps the very expressions it had, and with them its instruction stream.)
#define WS_ENTRY(row) ((row) * ((SH_PFX || SH_SFX) ? shared_args(a).ws_splits : a.splits) + ((SH_PFX || SH_SFX) ? shared_args(a).ws_first + split : split))
  int k_begin = split * a.chunk;                        // < Sk: (splits - 1) * chunk < Sk (DevLen: or the block is empty)
  int Sk = a.Sk;
  int Sq = a.Sq, R = a.R;  // VarQ: Sq_b and R_b = Sq_b * G, block-uniform; a.R stays the workspace's row count
  long long row0 = 0;      // VarQ: the sequence's first packed row
  (void)row0;
  int tb = b;              // the sequence whose table row the block walks (SharedPrefix: the lead)
  const_i32_t members = nullptr;  // SharedPrefix: the group's member list
  (void)members;
  if constexpr (SH_PFX) {
    const SharedArgs sh = shared_args(a);
    const int gp = as_const_i32(sh.group_prefix)[b];
    if (gp < kKV) return;  // nothing shared
    members = as_const_i32(sh.group_members) + (long long)b * sh.gm_rs;
    int lead = -1, sk_lead = 0;
    for (int j0 = 0; j0 < sh.group_cap && lead < 0; j0 += 64) {  // group_cap <= 128: two rounds at most, uniform
      const int j = j0 + lane;
      const int m = j < sh.group_cap ? members[j] : -1;
      long long len = 0;
      if (m >= 0 && m < a.B) len = (long long)a.seqlens_k[m] + a.seqlen_offset;
      const bool ok = len >= 1 && len <= a.Sk;  // a valid slot, and active
      const unsigned long long live = __ballot(ok);
      if (live) {
        const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(live));
        lead = __builtin_amdgcn_readlane(m, src);
        sk_lead = __builtin_amdgcn_readlane((int)len, src);
      }
    }
    if (lead < 0) return;
    Sk = shared_pfx(gp, sh.max_prefix, sk_lead, a.Sq);  // P_g: a multiple of 64, <= Sk_lead - Sq
    if (k_begin >= Sk) return;                          // (P_g = 0 included) nothing is written: the combine does not read this entry
    tb = lead;
    R = sh.group_cap * a.R;                             // <= 128 (checked by the entry)
  } else if constexpr (VARQ) {
    const VarQArgs vq = varq_args(a);
    const const_i32_t cu = as_const_i32(vq.cu_seqlens_q);
    const int c0 = cu[b], c1 = cu[b + 1];
    const long long sq_b = (long long)c1 - c0;
    const long long len = (long long)a.seqlens_k[b] + (vq.lens_before_step ? sq_b : 0ll);  // 64 bits, as the one-pass kernel forms it
    if constexpr (WINDOW) {
      if (!varq_window_split_takes(sq_b, len, vq.max_seqlen_q, a.Sk, split_args(a), window_args(a))) return;
    } else {
      if (!varq_split_takes(sq_b, len, vq.max_seqlen_q, a.Sk, split_args(a))) return;  // the one-pass kernel's sequence
    }
    Sq = (int)sq_b;  // 1 .. split_seqlen_q
    R = Sq * a.G;    // <= a.R <= 128
    row0 = c0;
    Sk = (int)len;   // 1 .. a.Sk
    if constexpr (WINDOW) {  // the splits start at the window: a k_begin at or beyond Sk (or beyond int) is clamped to Sk, an empty split
      const long long kb = (long long)window_anchor(Sq, Sk, window_args(a).left) + k_begin;
      k_begin = (int)min(kb, (long long)Sk);
    }
    if (k_begin >= Sk) {  // empty
      if (tid < R) {
        const long long e = (((long long)b * a.Hkv + kvh) * a.R + tid) * a.splits + split;
        a.ws_m[e] = -INFINITY;
        a.ws_l[e] = 0.f;
      }
      return;
    }
  } else if constexpr (DEVLEN) {
    const long long len = (long long)a.seqlens_k[b] + a.seqlen_offset;  // 64 bits: no entry can wrap into an active length
    Sk = (int)len;
    if constexpr (SH_SFX) {  // the splits start behind the prefix; a k_begin at or beyond Sk (or beyond int) is clamped to Sk, an empty split
      if (len >= 1 && len <= a.Sk) {
        const SharedArgs sh = shared_args(a);
        const long long kb = (long long)shared_pfx(as_const_i32(sh.seq_prefix)[b], sh.max_prefix, Sk, a.Sq) + k_begin;
        k_begin = (int)min(kb, (long long)Sk);
      }
    }
    if (len < 1 || len > a.Sk || k_begin >= Sk) {  // empty
      if (tid < a.R) {
        const long long e = WS_ENTRY(((long long)b * a.Hkv + kvh) * a.R + tid);
        a.ws_m[e] = -INFINITY;
        a.ws_l[e] = 0.f;
      }
      return;
    }
  }
  const int shift = Sk - Sq;
  const int k_end = min(Sk, k_begin + a.chunk);         // keys [k_begin, k_end) are this block's
  const int nt = (k_end - k_begin + kKV - 1) / kKV;

#define CAUSAL (SH_PFX ? 0 : a.causal)  // SharedPrefix: the prefix lies below every row's causal limit
  const int wr0 = wave * kMfmaRows;                     // first packed row of the wave
  const bool wave_on = wr0 < R;                         // (a wave without rows still stages K / V and meets the barriers)
  const int pr = min(wr0 + r, R - 1);                   // rows >= R compute row R - 1 again and are not stored
  const int sr = SH_PFX ? pr % a.R : pr;                // SharedPrefix: packed row = (j * Sq + i) * G + g, sr = the member's own row
  const int qi = (SH_PFX ? sr : pr) / a.G, h = kvh * a.G + (SH_PFX ? sr : pr) % a.G;    // packed row = i * G + g
  const int lim = CAUSAL ? qi + shift : Sk - 1;                                       // last key this lane's row attends
  const int wave_max = CAUSAL ? min(wr0 + kMfmaRows - 1, R - 1) / a.G + shift : Sk - 1;    // .. any row of the wave
  const int wave_min = CAUSAL ? wr0 / a.G + shift : Sk - 1;                         // every row of the wave attends keys <= this
#undef CAUSAL
  long long qb = b;      // the sequence of this lane's row
  bool row_live = true;  // SharedPrefix: the row's member is a valid, active slot
  if constexpr (SH_PFX) {
    const int m = members[pr / a.R];  // pr / a.R < group_cap
    long long len = 0;
    if (m >= 0 && m < a.B) len = (long long)a.seqlens_k[m] + a.seqlen_offset;
    row_live = len >= 1 && len <= a.Sk;
    qb = min(max(m, 0), a.B - 1);  // clamped before it forms an address; a dead row is computed and not stored
  }
  // Window (causal only): this lane's first key, and the first / last window start of the wave's rows
  int lo = 0, wave_lo = 0, wave_lo_max = 0;
  unsigned span = 0;  // lim - lo, the width of this lane's window
  (void)lo, (void)span, (void)wave_lo, (void)wave_lo_max;
  if constexpr (WINDOW) {
    const long long left = window_args(a).left;
    // a row that attends nothing (lim < 0) gets a start no key reaches and an empty span
    lo = lim < 0 ? 0x40000000 : (int)max(0ll, (long long)lim - left);
    span = lim < 0 ? 0u : (unsigned)(lim - lo);
    wave_lo = (int)max(0ll, (long long)wave_min - left);
    wave_lo_max = (int)max(0ll, (long long)wave_max - left);
  }

  // Q: the B operand of S^T = K Q^T, lane (r, hh) holds Q[row r][16 ks + 8 hh + 0..7]
  vec8 qf[KS];
  {
    const uint16_t* qp = a.q + (SH_PFX ? qb : (long long)b) * a.q_bs + (long long)qi * a.q_rs + (long long)h * DH + 8 * hh;
    if constexpr (VARQ)  // the packed row of (b, qi), clamped into the tensor before it forms an address
      qp = a.q + min(max(row0 + qi, 0ll), (long long)varq_args(a).total_q - 1) * a.q_rs + (long long)h * DH + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(qp + 16 * ks));
  }

  const long long pool_b = PAGED ? 0 : b;  // Paged: the pools have no batch dimension, the page offset is added per tile
  const uint16_t* kb = a.k + pool_b * a.k_bs + (long long)kvh * DH;
  const uint16_t* vb = a.v + pool_b * a.v_bs + (long long)kvh * DH;
  using stage_t = typename std::conditional<KV8, u32x2, u32x4>::type;
  stage_t kr[LOADS], vr[LOADS];
  float ksc[KV8 ? LOADS : 1], vsc[KV8 ? LOADS : 1];  // Kv8: the scale of the chunk's row
  const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(a.k) + pool_b * a.k_bs + (long long)kvh * DH;
  const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(a.v) + pool_b * a.v_bs + (long long)kvh * DH;
  const float* ksb = KV8 ? a.k_scale + pool_b * a.ks_bs + kvh : nullptr;
  const float* vsb = KV8 ? a.v_scale + pool_b * a.vs_bs + kvh : nullptr;
  // Paged: page = the (clamped) id of the tile's page, ro = the tile's first row inside it; unused otherwise
  auto stage_load = [&](int t0, int page, int ro) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      const long long g = min(t0 + row, Sk - 1);    // no row >= Sk is read
      if constexpr (PAGED) {
        const long long prow = ro + (g - t0);        // row of the page: < page_size, the tile does not straddle
        if constexpr (KV8) {
          kr[i] = *reinterpret_cast<const u32x2*>(kb8 + page * a.k_bs + prow * a.k_rs + ch * 8);
          vr[i] = *reinterpret_cast<const u32x2*>(vb8 + page * a.v_bs + prow * a.v_rs + ch * 8);
          ksc[i] = ksb[page * a.ks_bs + prow * a.ks_rs];
          vsc[i] = vsb[page * a.vs_bs + prow * a.vs_rs];
        } else {
          kr[i] = *reinterpret_cast<const u32x4*>(kb + page * a.k_bs + prow * a.k_rs + ch * 8);
          vr[i] = *reinterpret_cast<const u32x4*>(vb + page * a.v_bs + prow * a.v_rs + ch * 8);
        }
      } else if constexpr (KV8) {
        kr[i] = *reinterpret_cast<const u32x2*>(kb8 + g * a.k_rs + ch * 8);
        vr[i] = *reinterpret_cast<const u32x2*>(vb8 + g * a.v_rs + ch * 8);
        ksc[i] = ksb[g * a.ks_rs];
        vsc[i] = vsb[g * a.vs_rs];
      } else {
        kr[i] = *reinterpret_cast<const u32x4*>(kb + g * a.k_rs + ch * 8);
        vr[i] = *reinterpret_cast<const u32x4*>(vb + g * a.v_rs + ch * 8);
      }
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      if constexpr (KV8) {
        *reinterpret_cast<u32x4*>(&k_s[buf][k_off<DH>(row, ch)]) = kv8_dequant8<DT>(kr[i], ksc[i]);
        *reinterpret_cast<u32x4*>(&v_s[buf][v_off<DH>(row, ch)]) = kv8_dequant8<DT>(vr[i], vsc[i]);
      } else {
        *reinterpret_cast<u32x4*>(&k_s[buf][k_off<DH>(row, ch)]) = kr[i];
        *reinterpret_cast<u32x4*>(&v_s[buf][v_off<DH>(row, ch)]) = vr[i];
      }
    }
  };

  f32x16 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // l: this lane's 32 keys of every tile; the two halves are added at the end

  // transposed-read addressing: lane 4 qq + p of a 16-lane group supplies row qq, columns 4 p .. 4 p + 3 of the group's 4 x 16 block
  const int tr_q = (lane & 15) >> 2, tr_p = lane & 3, tr_g = (lane >> 4) & 1;

  // Paged: the ids of tiles 0 and 1, both in flight before the first K / V load is issued
  const PageArgs pg = page_args(a);
  const int* table = PAGED ? pg.block_table + (long long)(SH_PFX ? tb : b) * pg.bt_rs : nullptr;
  int pg_i = 0, pg_ro = 0, pg_cur = 0, ro_cur = 0, pg_nxt = 0, ro_nxt = 0;
  auto next_page = [&]() {  // (pg_i, pg_ro) -> the tile 64 keys on; returns its page id
    pg_ro += kKV;
    if (pg_ro == pg.page_size) {
      pg_ro = 0;
      ++pg_i;
    }
    return page_id(table, pg_i, pg.num_pages);
  };
  if constexpr (PAGED) {
    pg_i = k_begin / pg.page_size;
    pg_ro = k_begin - pg_i * pg.page_size;
    pg_cur = page_id(table, pg_i, pg.num_pages);
    ro_cur = pg_ro;
    if (nt > 1) {
      pg_nxt = next_page();
      ro_nxt = pg_ro;
    }
  }

  stage_load(k_begin, pg_cur, ro_cur);
  stage_write(0);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));  // Q has arrived before the loop (no vmcnt(0) behind the loop's loads)
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1, t0 = k_begin + t * kKV;
    const bool more = t + 1 < nt;
    int pg_n2 = pg_nxt, ro_n2 = ro_nxt;
    if constexpr (PAGED) {
      if (t + 2 < nt) {  // the id tile t + 2 will load with in the next iteration: a whole tile ahead of its use
        pg_n2 = next_page();
        ro_n2 = pg_ro;
      }
    }
    if (more) stage_load(t0 + kKV, pg_nxt, ro_nxt);

    bool below = false;  // Window: the tile lies wholly below every window start of the wave
    if constexpr (WINDOW) below = t0 + kKV <= wave_lo;
    if (wave_on && t0 <= wave_max && !below) {  // wave-uniform: every lane of the wave takes part in the transposed reads
      // ---- S^T = K Q^T: s[kb2][e] = key t0 + 32 kb2 + (e & 3) + 8 (e >> 2) + 4 hh, packed row r ----
      f32x16 s[2];
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kb2][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const vec8 ka = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(&k_s[buf][k_off<DH>(32 * kb2 + r, 2 * ks + hh)]));
          s[kb2] = DT::mfma32(ka, qf[ks], s[kb2]);
        }
      }
      // ---- online softmax (base 2: the logits are scaled by scale * log2 e) ----
      const bool need_mask = t0 + kKV - 1 > wave_min;  // (wave_min <= Sk - 1: the end of K is covered too)
      const bool need_lo = WINDOW && t0 < wave_lo_max;  // some row of the wave starts inside or behind this tile
      float mx = -INFINITY;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[kb2][e] * a.scale_log2e;
          if constexpr (SOFTCAP) x = cap_args(a).cap_log2e * softcap_tanh(s[kb2][e] * cap_args(a).scale_over_cap);
          if constexpr (WINDOW) {
            if (need_mask || need_lo) {  // both ends in one unsigned compare: lo <= key <= lim  <=>  key - lo <= lim - lo
              const int key = t0 + 32 * kb2 + (e & 3) + 8 * (e >> 2) + 4 * hh;
              x = (unsigned)(key - lo) <= span ? x : -INFINITY;
            }
          } else if (need_mask) {
            const int key = t0 + 32 * kb2 + (e & 3) + 8 * (e >> 2) + 4 * hh;
            x = key <= lim ? x : -INFINITY;
          }
          s[kb2][e] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      // a row may attend nothing of the chunk so far (m_new = -inf): subtract 0 instead, every weight is then exp2(-inf) = 0 and
      // alpha = exp2(-inf) = 0 multiplies an O and an l that are still 0 -- no Inf - Inf.  With m_new finite this is the prefill kernel's code
      const float m_sub = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_sub);
      m_run = m_new;
      vec8 pf[4];
      float sum = 0.f;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const elem pt = (elem)__builtin_amdgcn_exp2f(s[kb2][e] - m_sub);  // the ONE rounding of a weight
          pf[2 * kb2 + (e >> 3)][e & 7] = pt;
          sum += (float)pt;
        }
      l_run = l_run * alpha + sum;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
      // ---- O^T += V^T P^T: k-step s2 = keys 16 s2 + 8 (j >> 2) + 4 hh + (j & 3), j = operand element ----
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const int row = 16 * s2 + 4 * hh + tr_q, ch = 4 * db + 2 * tr_g + (tr_p >> 1);
          const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) i16x4*)(&v_s[buf][v_off<DH>(row, ch) + 4 * (tr_p & 1)]));
          const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) i16x4*)(&v_s[buf][v_off<DH>(row + 8, ch) + 4 * (tr_p & 1)]));
          const i16x8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = DT::mfma32(__builtin_bit_cast(vec8, va), pf[s2], o[db]);
        }
      }
    }

    if (more) stage_write(buf ^ 1);  // the other buffer: its readers finished before the barrier that ended tile t - 1
    __syncthreads();
    pg_nxt = pg_n2;
    ro_nxt = ro_n2;
  }

  // ---- the unnormalised partial; lane (r, hh) holds O[row r][32 db + 8 g4 + 4 hh + 0..3] in o[db][4 g4 + 0..3] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (wr0 + r < R && (!SH_PFX || row_live)) {
    const long long e = WS_ENTRY(((SH_PFX ? qb : (long long)b) * a.Hkv + kvh) * a.R + (SH_PFX ? sr : pr));
#undef WS_ENTRY
    float* op = a.ws_o + e * DH + 4 * hh;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<f32x4*>(op + 32 * db + 8 * g4) = f32x4{o[db][4 * g4], o[db][4 * g4 + 1], o[db][4 * g4 + 2], o[db][4 * g4 + 3]};
    if (hh == 0) {
      a.ws_m[e] = m_run;
      a.ws_l[e] = l_tot;
    }
  }
}

// DevLen<..>: a row may have attended nothing at all (its sequence is inactive, or Sk_b < Sq and the row's causal limit is negative); then
// every m_s is -inf, M = -inf and L = 0, and the row is written as zeros without the division.
//
// VarQ<DevLen<..>> (a mixed step): one thread = 8 columns of one (b, kvh, row < a.R = split_seqlen_q * G).  It evaluates varq_split_takes
// on its sequence and leaves if the split kernel did not take it or row >= R_b: such a workspace row was never written.  The result goes
// to packed row cu[b] + row / G, guarded by row < min(cu[b + 1], total_q).  Window<VarQ<DevLen<..>>>: the same under the windowed rule; the
// partials do not know where their split began.
//
// SharedCombine<DevLen<..>> (awq_shared.hpp): a.splits = splits_p + splits_s entries per row.  The thread forms P_b as the suffix block
// did and runs the rule over entries 0 .. ceil(P_b / chunk_p) - 1 and splits_p .. a.splits - 1, ascending; the prefix entries between
// belong to no key of this sequence, were never written for it, and are not read.
template <typename DT, int DH>
__global__ __launch_bounds__(256) void attn_splitkv_combine_kernel(CombineArgsOf<DT> a) {
  constexpr int CPR = DH / 8;
  constexpr bool VARQ = IsVarQ<DT>::value;
  constexpr bool SHARED = IsSharedCombine<DT>::value;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)a.B * a.Hkv * a.R * CPR) return;
  const int ch = (int)(id % CPR);
  const long long row = id / CPR;  // (b * Hkv + kvh) * R + packed row
  const int pr = (int)(row % a.R);
  const long long bk = row / a.R;
  const int kvh = (int)(bk % a.Hkv);
  const long long b = bk / a.Hkv;
  long long out_row = b * a.Sq + pr / a.G;  // VarQ: the packed row
  if constexpr (VARQ) {
    const VarQArgs vq = varq_args(a);
    const const_i32_t cu = as_const_i32(vq.cu_seqlens_q);
    const int c0 = cu[b], c1 = cu[b + 1];
    const long long sq_b = (long long)c1 - c0;
    const long long len = (long long)a.seqlens_k[b] + (vq.lens_before_step ? sq_b : 0ll);
    bool takes;
    if constexpr (IsWindow<DT>::value) takes = varq_window_split_takes(sq_b, len, vq.max_seqlen_q, a.Sk, split_args(a), window_args(a));
    else takes = varq_split_takes(sq_b, len, vq.max_seqlen_q, a.Sk, split_args(a));
    if (!takes || pr >= sq_b * a.G) return;
    out_row = (long long)c0 + pr / a.G;
    if (out_row < 0 || out_row >= min((long long)c1, (long long)vq.total_q)) return;  // (a corrupt array: no address outside the tensor)
  }
  // SharedCombine: entries [own_p, skip_to) are prefix splits behind this sequence's prefix -- never written for it, never read.  The
  // loops below count the entries that ARE read, t -> s = t below own_p, t - own_p + skip_to behind it: no branch inside them, so the
  // loads of the first loop pipeline as the dense form's do
  int own_p = 0, skip_to = 0;
  (void)own_p, (void)skip_to;
  if constexpr (SHARED) {
    const SharedArgs sh = shared_args(a);
    const long long len = (long long)a.seqlens_k[b] + a.seqlen_offset;
    const int p = len >= 1 && len <= a.Sk ? shared_pfx(as_const_i32(sh.seq_prefix)[b], sh.max_prefix, (int)len, a.Sq) : 0;
    own_p = (p + sh.chunk_p - 1) / sh.chunk_p;  // <= splits_p: p <= max_prefix <= splits_p * chunk_p
    skip_to = sh.splits_p;
  }
  const float* pm = a.ws_m + row * a.splits;
  const float* pl = a.ws_l + row * a.splits;
  const float* po = a.ws_o + row * a.splits * DH + ch * 8;
  const int n_read = SHARED ? own_p + a.splits - skip_to : a.splits;
  float M = -INFINITY;
  for (int t = 0; t < n_read; ++t) M = fmaxf(M, pm[SHARED ? (t < own_p ? t : t - own_p + skip_to) : t]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int t = 0; t < n_read; ++t) {
    const int s = SHARED ? (t < own_p ? t : t - own_p + skip_to) : t;
    const float m = pm[s];
    if (m == -INFINITY) continue;  // nothing attended in this split: contributes exactly nothing
    const float w = __builtin_amdgcn_exp2f(m - M);
    const f32x4 o0 = *reinterpret_cast<const f32x4*>(po + (long long)s * DH), o1 = *reinterpret_cast<const f32x4*>(po + (long long)s * DH + 4);
    L = __builtin_fmaf(w, pl[s], L);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = __builtin_fmaf(w, o0[e], acc[e]);
      acc[4 + e] = __builtin_fmaf(w, o1[e], acc[4 + e]);
    }
  }
  if constexpr (IsDevLen<DT>::value) {
    if (M == -INFINITY) {  // nothing attended: zeros, never 0 / 0
      *reinterpret_cast<u32x4*>(a.out + (out_row * a.H + kvh * a.G + pr % a.G) * DH + ch * 8) = u32x4{0u, 0u, 0u, 0u};
      return;
    }
  }
  const float inv = 1.0f / L;
  u32 ws[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ws[e] = (u32)DT::from_float(acc[2 * e] * inv) | ((u32)DT::from_float(acc[2 * e + 1] * inv) << 16);
  const int h = kvh * a.G + pr % a.G;
  *reinterpret_cast<u32x4*>(a.out + (out_row * a.H + h) * DH + ch * 8) = u32x4{ws[0], ws[1], ws[2], ws[3]};
}

}  // namespace

// Host plan.  *splits == 1: not taken, the one-pass kernel serves (then *chunk = Sk rounded up to 64).  Taken only for Sk >= 2048,
// Sq * G <= 128, Dh 64 / 128 and a one-pass launch of fewer than kCUs blocks.  Beyond that: aim at two blocks per CU (the LDS of two
// Dh = 128 blocks fits a CU), B * Hkv * splits >= 2 kCUs, with chunks of at least 1024 keys; chunk is the largest multiple of 64 that still
// yields that many splits.  Measured on the MI355X for B * Hkv = 8 (tools/splitkv_attn_bench.py --sweep-chunk, Llama-3-8B, bf16, Sq = 1,
// profiles/splitkv_attn_sweep.json): among chunks >= 1024 the rule's choice is the fastest or within noise of it -- 1024 at 32768 keys
// (52.6 us; 2048: 71.2), 2048 at 131072 (142 us; 4096: 142, 1024: 205).  Below 32768 keys chunks of 256 / 512 are faster still; the
// 1024-key floor is a fixed condition of the plan.  Other B * Hkv are not swept.  Depends on host arguments only (and on the knob).
int attn_splitkv_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* splits, int* chunk) {
  *splits = 1;
  *chunk = (int)((((long long)seqlen_k + kKV - 1) / kKV) * kKV);
  const long long rows = (long long)seqlen_q * (nheads / nheads_kv);
  if (rows > kMaxRows || (head_dim != 64 && head_dim != 128)) return 0;
  int c = 0;
  if (g_force_chunk) {
    c = g_force_chunk;
  } else {
    if (seqlen_k < kMinKeys) return 0;
    int q_tile = 0, one_pass_blocks = 0;
    attn_prefill_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal, &q_tile, &one_pass_blocks);
    if (one_pass_blocks >= kCUs) return 0;
    const long long groups = (long long)batch * nheads_kv;  // < kCUs here
    const int want = (int)((2 * kCUs + groups - 1) / groups);
    c = seqlen_k / want / kKV * kKV;
    if (c < kMinChunk) c = kMinChunk;
  }
  const int n = (int)(((long long)seqlen_k + c - 1) / c);
  if (n <= 1) return 0;
  *splits = n;
  *chunk = c;
  return 0;
}

size_t attn_splitkv_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal) {
  int splits = 1, chunk = 0;
  attn_splitkv_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal, &splits, &chunk);
  if (splits <= 1) return 0;
  return (size_t)batch * nheads * seqlen_q * splits * (head_dim + 2) * sizeof(float);
}

int attn_splitkv_tune_set(const char* key, int value) {
  if (strcmp(key, "attn_splitkv_chunk") != 0 || value < 0 || (value % kKV) != 0) return -1;
  g_force_chunk = value;
  return 0;
}

// Host plan of the device-length form (awq_attn_kvcache): made from the bound max_seqlen_k alone, never from a length.  The chunk rule
// above (two blocks per CU, a multiple of 64, at least 1024 keys, or the knob) without the 2048-key floor and the one-pass test: the
// split pair always runs, splits >= 1 and splits * chunk >= max_seqlen_k.
// The rule counts the KV heads of ONE sequence, not batch * nheads_kv: the plan cannot know how many sequences of the batch are long, and
// a batch is as slow as its longest sequence.  Counting the batch (the first form of this plan) gave the 131072-key sequence of the
// ragged batch of tools/kvcache_attn_bench.py 8 splits of 16384 keys, 64 live blocks on 256 CUs: 444 us against 320 us for the seven
// per-sequence calls (profiles/kvcache_attn_bench.json keeps that row as "ragged_batch_rule").  Sized for one sequence, a full batch of
// long sequences gets batch times as many blocks of the same chunk as a single sequence does; the blocks beyond a sequence's length leave
// at once.  The 1024-key floor is carried over from the host-length plan; under a loose bound it is not the best choice (README.md).
int attn_kvcache_plan(int batch, int nheads_kv, int max_seqlen_k, int* splits, int* chunk) {
  (void)batch;
  int c = g_force_chunk;
  if (!c) {
    const long long groups = nheads_kv;
    const long long want = groups >= 2 * kCUs ? 1 : (2 * kCUs + groups - 1) / groups;
    c = (int)(max_seqlen_k / want / kKV * kKV);
    if (c < kMinChunk) c = kMinChunk;
  }
  *splits = (int)(((long long)max_seqlen_k + c - 1) / c);
  *chunk = c;
  return 0;
}

size_t attn_kvcache_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k) {
  int splits = 1, chunk = 0;
  attn_kvcache_plan(batch, nheads_kv, max_seqlen_k, &splits, &chunk);
  return (size_t)batch * nheads * seqlen_q * splits * (head_dim + 2) * sizeof(float);
}

// Host plan of a windowed mixed step (awq_window.hpp): attn_kvcache_plan for the most keys an anchored walk can cover,
// min(max_seqlen_k, left + split_seqlen_q + 63) -- Sk_b - anchor_b never exceeds it.  The knob attn_splitkv_chunk applies.  Host arguments only.
int attn_varq_window_plan(int batch, int nheads_kv, int split_seqlen_q, int max_seqlen_k, int window_left, int* splits, int* chunk) {
  return attn_kvcache_plan(batch, nheads_kv, window_plan_bound(split_seqlen_q, max_seqlen_k, window_left), splits, chunk);
}

size_t attn_varq_window_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int window_left) {
  return attn_kvcache_workspace_bytes(batch, nheads, nheads_kv, head_dim, split_seqlen_q, window_plan_bound(split_seqlen_q, max_seqlen_k, window_left));
}

// Host plan of a shared-prefix decode (awq_shared.hpp): attn_kvcache_plan's rule twice, for the bound max_prefix of the prefix walk and
// for max_seqlen_k of the suffix walk (a suffix is as long as max_seqlen_k when a sequence shares nothing).  The knob forces both chunks.
// Nothing here is tuned to a measurement of the shared call.  Host arguments only.
int attn_kvcache_shared_plan(int batch, int nheads_kv, int max_prefix, int max_seqlen_k, int* splits_p, int* chunk_p, int* splits_s, int* chunk_s) {
  attn_kvcache_plan(batch, nheads_kv, max_prefix, splits_p, chunk_p);
  return attn_kvcache_plan(batch, nheads_kv, max_seqlen_k, splits_s, chunk_s);
}

size_t attn_kvcache_shared_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix, int max_seqlen_k) {
  int sp = 1, cp = 0, ss = 1, cs = 0;
  attn_kvcache_shared_plan(batch, nheads_kv, max_prefix, max_seqlen_k, &sp, &cp, &ss, &cs);
  return (size_t)batch * nheads * seqlen_q * ((size_t)sp + ss) * (head_dim + 2) * sizeof(float);
}

namespace {

// Both launches of one call. K is the traits of the split kernel (DT, or Kv8<DT> for the FP8 cache); the combine launch reads fp32
// partials only, so it is the T cache's in either case.
// L is the identity for host lengths, DevLen for lengths on the device and PagedDevLen for those over a pool of pages; C is what L is to
// the combine launch (the paged form combines with the dense DevLen kernel: the partials do not know where K / V came from).
template <template <typename> class K, template <typename> class L, template <typename> class C, typename A>
void launch_pair(const A& a, int Dh, int dtype, hipStream_t st) {
  const dim3 grid((unsigned)((long long)a.B * a.Hkv * a.splits));
  const dim3 cgrid((unsigned)(((long long)a.B * a.Hkv * a.R * (Dh / 8) + 255) / 256));
  for_dtype_dh<F16, BF16>(dtype, Dh, [&](auto dt, auto dh) {
    using DT = decltype(dt);
    constexpr int DH = decltype(dh)::value;
    hipLaunchKernelGGL((attn_splitkv_kernel<L<K<DT>>, DH>), grid, dim3(kNW * 64), 0, st, a);
    hipLaunchKernelGGL((attn_splitkv_combine_kernel<C<DT>, DH>), cgrid, dim3(256), 0, st, (const CombineArgsOf<C<DT>>&)a);
  });
}
template <typename DT>
using TCache = DT;  // the T cache: the element traits themselves
template <template <typename> class L, template <typename> class C, typename A>
void launch_for_cache(const A& a, int Dh, int dtype, hipStream_t st) {
  if (a.k_scale) launch_pair<Kv8, L, C>(a, Dh, dtype, st);
  else launch_pair<TCache, L, C>(a, Dh, dtype, st);
}

}  // namespace

// The split pair over a view.  Host length: Sk keys of every sequence.  Device lengths (awq_attn_kvcache[_kv8]): the Sk of the kernel
// arguments is the bound max_seqlen_k (<= the capacity of the view, so the clamp to Sk_b - 1 <= max_seqlen_k - 1 stays inside the
// sequence's rows).  Paged (awq_attn_kvcache_paged[_kv8]): k / v are the pools and the outer strides their page strides; max_seqlen_k <=
// pages_per_seq * page_size, so every table index the kernel forms lies inside a table row.  Scales in the view select the FP8 cache
// (awq_kv8.hpp: codes with strides in bytes, scales with strides in floats).  The caller has validated the arguments and holds the plan
// (splits > 1 for a host length) and a workspace of its size.
int launch_kv_attn(const KvAttnCall& c, int splits, int chunk, void* workspace, hipStream_t st) {
  const KvView& kv = c.kv;
  const bool mixed = c.cu_seqlens_q && c.split_seqlen_q > 0;  // the packed pair: c.Sq is max_seqlen_q, c.seqlen_offset the flag
  SoftcapSplitKArgs a;
  a.q = (const uint16_t*)c.q;
  a.k = (const uint16_t*)kv.k;
  a.v = (const uint16_t*)kv.v;
  a.out = (uint16_t*)c.out;
  a.q_bs = c.q_bs, a.q_rs = c.q_rs;
  a.k_bs = kv.k_os, a.k_rs = kv.k_rs, a.v_bs = kv.v_os, a.v_rs = kv.v_rs;
  a.B = c.B;
  a.Sq = mixed ? c.split_seqlen_q : c.Sq;
  a.Sk = c.seqlens_k ? c.max_seqlen_k : c.Sk;
  a.H = c.H;
  a.Hkv = c.Hkv;
  a.G = c.H / c.Hkv;
  a.R = a.Sq * a.G;
  a.splits = splits;
  a.chunk = chunk;
  a.causal = c.causal ? 1 : 0;
  a.scale_log2e = c.scale * 1.4426950408889634f;
  const long long n = (long long)c.B * c.Hkv * a.R * splits;
  a.ws_o = (float*)workspace;
  a.ws_m = a.ws_o + n * c.Dh;
  a.ws_l = a.ws_m + n;
  a.k_scale = kv.k_scale;
  a.v_scale = kv.v_scale;
  a.ks_bs = kv.ks_os, a.ks_rs = kv.ks_rs, a.vs_bs = kv.vs_os, a.vs_rs = kv.vs_rs;
  a.seqlens_k = c.seqlens_k;
  a.seqlen_offset = c.seqlens_k && !mixed ? c.seqlen_offset : 0;
  a.pg = PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer};
  a.vq = VarQArgs{c.cu_seqlens_q, c.total_q, c.max_seqlen_q, c.seqlen_offset ? 1 : 0};
  a.sp = VarQSplitArgs{c.split_seqlen_q, c.split_min_keys};
  a.w = WindowArgs{c.window_left >= 0 ? c.window_left : 0};
  a.cap = softcap_args(c.scale, c.softcap > 0.f ? c.softcap : 1.f);
  const WindowSplitKArgs& win = a;
  const VarQSplitKArgs& varq = a;
  const PagedSplitArgs& paged = a;
  const SplitArgs& dense = a;
  if (mixed && c.window_left >= 0 && c.softcap > 0.f) {  // a capped windowed step (awq_softcap.hpp): the window's plan and combine
    if (kv.block_table) launch_for_cache<SoftcapWindowVarQPagedDevLen, WindowVarQDevLen>(a, c.Dh, c.dtype, st);
    else launch_for_cache<SoftcapWindowVarQDevLen, WindowVarQDevLen>(a, c.Dh, c.dtype, st);
  } else if (mixed && c.window_left >= 0) {  // a windowed step (awq_window.hpp): the caller's plan is awq_attn_varq_window_plan's
    if (kv.block_table) launch_for_cache<WindowVarQPagedDevLen, WindowVarQDevLen>(win, c.Dh, c.dtype, st);
    else launch_for_cache<WindowVarQDevLen, WindowVarQDevLen>(win, c.Dh, c.dtype, st);
  } else if (mixed) {
    if (kv.block_table) launch_for_cache<VarQPagedDevLen, VarQDevLen>(varq, c.Dh, c.dtype, st);
    else launch_for_cache<VarQDevLen, VarQDevLen>(varq, c.Dh, c.dtype, st);
  } else if (kv.block_table) launch_for_cache<PagedDevLen, DevLen>(paged, c.Dh, c.dtype, st);
  else if (c.seqlens_k) launch_for_cache<DevLen, DevLen>(dense, c.Dh, c.dtype, st);
  else launch_for_cache<HostLen, HostLen>(dense, c.Dh, c.dtype, st);
  return 0;
}

namespace {

template <template <typename> class K>
void launch_shared(const SharedSplitArgs& a, int splits_s, int chunk_s, int Dh, int dtype, hipStream_t st) {
  const SharedArgs& sh = a.sh;
  SharedSplitArgs pfx = a, sfx = a, cmb = a;
  pfx.splits = sh.splits_p, pfx.chunk = sh.chunk_p, pfx.sh.ws_first = 0;
  sfx.splits = splits_s, sfx.chunk = chunk_s, sfx.sh.ws_first = sh.splits_p;
  cmb.splits = sh.ws_splits;
  const dim3 pgrid((unsigned)((long long)sh.num_groups * a.Hkv * sh.splits_p));
  const dim3 sgrid((unsigned)((long long)a.B * a.Hkv * splits_s));
  const dim3 cgrid((unsigned)(((long long)a.B * a.Hkv * a.R * (Dh / 8) + 255) / 256));
  for_dtype_dh<F16, BF16>(dtype, Dh, [&](auto dt, auto dh) {
    using DT = decltype(dt);
    constexpr int DH = decltype(dh)::value;
    hipLaunchKernelGGL((attn_splitkv_kernel<SharedPrefixPagedDevLen<K<DT>>, DH>), pgrid, dim3(kNW * 64), 0, st, pfx);
    hipLaunchKernelGGL((attn_splitkv_kernel<SharedSuffixPagedDevLen<K<DT>>, DH>), sgrid, dim3(kNW * 64), 0, st, sfx);
    hipLaunchKernelGGL((attn_splitkv_combine_kernel<SharedCombineDevLen<DT>, DH>), cgrid, dim3(256), 0, st, cmb);
  });
}

}  // namespace

// The three launches of awq_attn_kvcache_paged_shared[_kv8] (awq_shared.hpp).  The set of launches and their grids come from host
// arguments only; which blocks do work is decided on the device, so a captured call follows the lengths, tables and group arrays in place.
int launch_kv_attn_shared(const KvAttnCall& c, const KvSharedCall& s, void* workspace, hipStream_t st) {
  const KvView& kv = c.kv;
  int splits_p = 1, chunk_p = 0, splits_s = 1, chunk_s = 0;
  attn_kvcache_shared_plan(c.B, c.Hkv, s.max_prefix, c.max_seqlen_k, &splits_p, &chunk_p, &splits_s, &chunk_s);
  SharedSplitArgs a;
  a.q = (const uint16_t*)c.q;
  a.k = (const uint16_t*)kv.k;
  a.v = (const uint16_t*)kv.v;
  a.out = (uint16_t*)c.out;
  a.q_bs = c.q_bs, a.q_rs = c.q_rs;
  a.k_bs = kv.k_os, a.k_rs = kv.k_rs, a.v_bs = kv.v_os, a.v_rs = kv.v_rs;
  a.B = c.B;
  a.Sq = c.Sq;
  a.Sk = c.max_seqlen_k;
  a.H = c.H;
  a.Hkv = c.Hkv;
  a.G = c.H / c.Hkv;
  a.R = a.Sq * a.G;
  a.splits = splits_p + splits_s;
  a.chunk = chunk_s;
  a.causal = c.causal ? 1 : 0;
  a.scale_log2e = c.scale * 1.4426950408889634f;
  const long long n = (long long)c.B * c.Hkv * a.R * a.splits;
  a.ws_o = (float*)workspace;
  a.ws_m = a.ws_o + n * c.Dh;
  a.ws_l = a.ws_m + n;
  a.k_scale = kv.k_scale;
  a.v_scale = kv.v_scale;
  a.ks_bs = kv.ks_os, a.ks_rs = kv.ks_rs, a.vs_bs = kv.vs_os, a.vs_rs = kv.vs_rs;
  a.seqlens_k = c.seqlens_k;
  a.seqlen_offset = c.seqlen_offset;
  a.pg = PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer};
  a.sh = SharedArgs{s.group_members, s.members_row_stride, s.group_prefix, s.seq_prefix, s.num_groups, s.group_cap, s.max_prefix,
                    splits_p, chunk_p, splits_p + splits_s, 0};
  if (kv.k_scale) launch_shared<Kv8>(a, splits_s, chunk_s, c.Dh, c.dtype, st);
  else launch_shared<TCache>(a, splits_s, chunk_s, c.Dh, c.dtype, st);
  return 0;
}

}  // namespace awq
