// Prefill attention (flash_attn_func's forward) and the two rotary-embedding exports tinychat calls on a prompt.
//
//   O = softmax(scale * Q K^T + mask) V        q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh], out [B, Sq, H, Dh]
//   causal: query row i attends keys j <= i + (Sk - Sq) (bottom-right aligned, flash-attn >= 2.1; tinychat's chunk prefill passes
//   Sq = seqlen, Sk = start_pos + seqlen, llama.py:218 / fused_attn.py:477,539); query head h reads KV head h / (H / Hkv).
//
// Structure (flash attention, one pass over K / V per q tile, online softmax; nothing of size Sq x Sk exists anywhere):
//   * One block = NW waves (NW = 4; 8 or 2 where attn_prefill_plan measured a gain; every NW exists for both head dims) = one q tile
//     of 32 NW rows of ONE (batch, query head); wave w owns rows 32 w .. 32 w + 31.  Blocks are numbered (tile rank, batch, head) with the head fastest, so the G query heads of a KV group run
//     next to each other and re-read their K / V from L2, and with causal masking rank 0 is the LAST q tile (the longest one): the
//     short tiles fill the tail of the launch.
//   * K / V are walked in tiles of 64 keys, double-buffered in LDS through registers: the global loads of tile t + 1 are issued before
//     the MFMAs of tile t and written to the other LDS buffer after them (one barrier per tile), so their latency hides under the
//     compute.  Rows >= Sk are never read: their address is clamped to row Sk - 1 and their score is masked.
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (A = K rows from LDS, ds_read_b128 on an XOR-swizzled image; B = Q, held in registers for the
//     whole block): a lane then holds, for ITS query row (lane % 32), the scores of 32 of the tile's 64 keys, the lane 32 away the other
//     32 -- the row max costs 31 v_max and one cross-half exchange, and the softmax is lane-local.
//   * P is rounded to T once; the row sum l is accumulated from those ROUNDED weights (numerator and denominator carry the same
//     rounding).  The rounded P registers are directly the B operand of O^T = V^T P^T (an accumulator tile's registers 8 s .. 8 s + 7
//     are the k-step s of the next product, in the permuted key order 16 s + 8 (j / 4) + 4 (lane / 32) + j % 4); the A operand V^T comes
//     from the row-major V image with ds_read_b64_tr_b16, two reads of 4 consecutive keys each -- exactly that permuted order.  O^T has
//     the query row on the lane again, so the rescale by exp(m_old - m_new) is lane-local too.
//   * Tiles wholly above the diagonal are skipped per block (loop bound) and per wave (wave-uniform test); -inf masking runs only in
//     the tiles the diagonal or the end of K crosses.
//   * No workspace, no atomics: bit-deterministic.  O is divided by l (IEEE division of 1 / l, once per row) and rounded to T once.
#include "awq_device.hpp"
#include "awq_devlen.hpp"
#include "awq_kernels.hpp"
#include "awq_kv8.hpp"
#include "awq_kvcache.hpp"
#include "awq_paged.hpp"
#include "awq_rope.hpp"
#include "awq_varq.hpp"
#include "awq_softcap.hpp"
#include "awq_window.hpp"

#include <math.h>
#include <string.h>

#include <type_traits>

namespace awq {
namespace {

constexpr int kKV = 64;       // keys per tile
constexpr int kMfmaRows = 32;  // q rows per wave
constexpr int kCUs = 256;      // the MI355X; a constant because the plan is a host-only function that CPU tests pin (as attn_decode_plan's)
int g_force_rows = 0;          // knob attn_prefill_rows (awq_tune_set): 64 / 128 / 256 forces the q tile, 0 = the plan's choice

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

struct PrefillArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* out;
  long long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;  // elements
  int B, Sq, Sk, H, G, ntiles, causal;
  float scale_log2e;
  // Kv8 only (awq_kv8.hpp): the scales [B, Sk, Hkv] of the e4m3 codes a.k / a.v point at, batch / row strides in floats; a.k_bs .. a.v_rs
  // are then in codes (bytes)
  const float* k_scale;
  const float* v_scale;
  long long ks_bs, ks_rs, vs_bs, vs_rs;
};
// DevLen / Paged only (awq_devlen.hpp, awq_paged.hpp): what awq_attn_prefill_kvcache / awq_attn_prefill_paged add to a launch.  A struct
// of its own, passed NEXT to PrefillArgs as a second kernel argument: the host-length kernels keep their PrefillArgs block, their
// register assignment and their code (DESIGN.md "Prompt chunks on the device-length caches").
struct PrefillLenArgs {
  const int* seqlens_k;  // device int32 [B]: the length of sequence b is seqlens_k[b] + seqlen_offset
  int seqlen_offset;
  int max_seqlen_k;      // the host's bound: a sequence beyond it is inactive
  PageArgs pg;           // Paged: a.k / a.v are then the pools and a.k_bs / a.v_bs (a.ks_bs / a.vs_bs) their PAGE strides
  VarQArgs vq;           // VarQ (awq_varq.hpp): a.q / a.out are then the packed rows, a.Sq the host's bound max_seqlen_q; no other form reads it
};

// VarQMix only (awq_varq.hpp, a mixed step): the two thresholds of the rule behind the length arguments.  A struct of its own, so that the
// plain VarQ kernels keep their PrefillLenArgs block
struct PrefillMixArgs : PrefillLenArgs {
  VarQSplitArgs sp;
};

// Window<VarQMix<..>> only (awq_window.hpp): the window behind the thresholds.  A struct of its own once more: the VarQMix kernels keep their
// PrefillMixArgs block
struct PrefillWinArgs : PrefillMixArgs {
  WindowArgs w;
};

// Softcap<Window<VarQMix<..>>> only (awq_softcap.hpp): the cap behind the window.  A struct of its own again: the windowed kernels keep their
// PrefillWinArgs block
struct PrefillCapArgs : PrefillWinArgs {
  SoftcapArgs cap;
};

struct NoLenArgs {};
template <typename DT>
using LenArgsOf = typename std::conditional<
    IsSoftcap<DT>::value, PrefillCapArgs,
    typename std::conditional<
        IsWindow<DT>::value, PrefillWinArgs,
        typename std::conditional<IsVarQMix<DT>::value, PrefillMixArgs,
                                  typename std::conditional<IsDevLen<DT>::value, PrefillLenArgs, NoLenArgs>::type>::type>::type>::type;
__device__ __forceinline__ PrefillLenArgs len_args(const NoLenArgs&) { return PrefillLenArgs{nullptr, 0, 0, PageArgs{nullptr, 0, 0, 0}, VarQArgs{nullptr, 0, 0, 0}}; }
__device__ __forceinline__ PrefillLenArgs len_args(const PrefillLenArgs& x) { return x; }
__device__ __forceinline__ VarQSplitArgs split_args(const NoLenArgs&) { return VarQSplitArgs{0, 0}; }
__device__ __forceinline__ VarQSplitArgs split_args(const PrefillLenArgs&) { return VarQSplitArgs{0, 0}; }
__device__ __forceinline__ VarQSplitArgs split_args(const PrefillMixArgs& x) { return x.sp; }
__device__ __forceinline__ WindowArgs window_args(const NoLenArgs&) { return WindowArgs{0}; }
__device__ __forceinline__ WindowArgs window_args(const PrefillLenArgs&) { return WindowArgs{0}; }
__device__ __forceinline__ WindowArgs window_args(const PrefillWinArgs& x) { return x.w; }
__device__ __forceinline__ SoftcapArgs cap_args(const NoLenArgs&) { return SoftcapArgs{0.f, 0.f}; }
__device__ __forceinline__ SoftcapArgs cap_args(const PrefillLenArgs&) { return SoftcapArgs{0.f, 0.f}; }
__device__ __forceinline__ SoftcapArgs cap_args(const PrefillCapArgs& x) { return x.cap; }

// LDS images: rows of DH elements, the 16-byte chunks of a row permuted by an XOR that depends on the row.
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

// FT = true: K / V are staged straight from the FasterTransformer caches the decode kernel reads and writes, k_cache [Bc, Hkv, DH/8, Lmax, 8]
// and v_cache [Bc, Hkv, Lmax, DH] (launch_attn_prefill_ftcache below).  a.k / a.v then point at cache position kv_start of row 0, head 0,
// a.k_rs is the stride between two 8-column chunks of K (Lmax * 8), a.k_bs = a.v_bs the row stride Hkv * Lmax * DH, and the head stride of
// both caches is a.k_rs * DH / 8.  Only the global addresses of the staging differ: the LDS images, the tile walk and every rounding
// are those of the natural-layout form, so the two give the same bits on the same keys and values.
//
// The FT form is selected by the element traits -- FtCache<F16> / FtCache<BF16>, the same traits under another name -- so it is a
// separate instantiation and the natural-layout kernels keep their names, their compile-time strides and their code.
//
// Kv8<DT> (awq_kv8.hpp) selects the FP8 cache the same way: K / V are e4m3 codes [B, Sk, Hkv, DH] with one fp32 scale per (key, KV head).
// A thread keeps the c = tid + i * NT mapping and loads the 8 bytes of its chunk and the row's scale; the dequantisation T(float(code) * s)
// sits between the global load and the LDS write, which stores the same 16 bytes into the same slot.  The 8-byte form is kept over 16 bytes
// per lane (two chunks): at DH = 64 with eight waves a tile has 256 sixteen-byte code chunks for 512 threads, which would idle half the
// loaders, and the mapping, the clamp and the LDS slots stay those of the T cache.
template <typename DT>
struct FtCache : DT {};
template <typename DT>
struct IsFtCache {
  static constexpr bool value = false;
};
template <typename DT>
struct IsFtCache<FtCache<DT>> {
  static constexpr bool value = true;
};

//
// DevLen<..> (awq_attn_prefill_kvcache[_kv8]): Sk_b = seqlens_k[b] + seqlen_offset stands wherever a.Sk stands in the host-length form.  The
// length is one scalar load at the head of the block, issued next to the Q loads, which do not depend on it.  A block whose sequence is
// inactive (Sk_b < 1 or Sk_b > max_seqlen_k) or whose q tile attends no key (causal, Sk_b < Sq: every row's limit is negative) writes zero
// rows and leaves before its first K / V load; the test is uniform over the block and no barrier precedes it.  A row of a live block may
// still attend nothing (its limit is negative while a later row's is not): its running max stays -inf, so 0 is subtracted in its place
// (every weight is exp2(-inf) = 0, alpha = 0 multiplies an O and an l that are still 0: no Inf - Inf), and it is written as zeros without
// the division by l = 0.  With a finite max both guards select the host-length kernel's expressions: same bits.
//
// Paged<DevLen<..>> (awq_attn_prefill_paged[_kv8]): key g of the sequence is row g % page_size of page table[b][g / page_size].  Tiles
// begin at multiples of 64 from key 0 and page_size % 64 == 0, so a tile (and the clamp to Sk_b - 1, which stays inside it) has ONE page,
// uniform over the block: a scalar load.  The ids run a tile ahead of the loads that use them, as in the split kernel
// (awq_attn_splitkv_cdna4.hip): tile t + 1's K / V loads of iteration t take an id requested in iteration t - 1, the first two at the head
// of the block behind the length.  (pg_i, pg_ro) advance by 64 rows: no division in the loop.  Only tiles j < nt are looked up; their
// first key lies below kv_end <= Sk_b, so no entry at or behind ceil(Sk_b / page_size) is read.
//
// VarQ<..> over the four forms above (awq_varq.hpp, awq_attn_prefill_kvcache_varq[_kv8], awq_attn_prefill_paged_varq[_kv8]): q / out are
// packed rows and Sq_b = cu[b + 1] - cu[b] stands wherever a.Sq stands -- shift, q_last, qi, wave_on and the store guard -- so an active
// sequence's rows carry the bits of the rectangular launch on that sequence alone.  cu[b] and cu[b + 1] are two scalar loads through the
// constant address space at the very head of the block, in front of the length: the q row (cu[b] + qi) depends on them, so unlike the
// rectangular forms the Q loads wait for one scalar round trip.  The grid is sized by the host's bound, ceil(max_seqlen_q / rows) ranks;
// a block whose rank is at or beyond ntiles_b = ceil(Sq_b / rows) returns before any vector load, and the tile reversal counts from
// ntiles_b, so rank 0 is every sequence's longest tile.  Sq_b outside [0, max_seqlen_q] makes the sequence inactive: rows
// s < min(Sq_b, max_seqlen_q) are written as zeros.  With lens_before_step the length is seqlens_k[b] + Sq_b, formed in 64 bits.
//
// VarQMix<..> (awq_attn_varq[_kv8], awq_attn_paged_varq[_kv8]): the VarQ form of a mixed step.  Behind the length load the block evaluates
// varq_split_takes (awq_varq.hpp) on its sequence; a sequence the split pair takes is not this kernel's: the block returns before any
// vector load and writes nothing.  The test is uniform over the block and no barrier precedes it.  Every other sequence runs the VarQ code.
//
// Window<VarQMix<..>> (awq_window.hpp, awq_attn_varq_window[_kv8], awq_attn_paged_varq_window[_kv8]): row s attends keys
// max(0, lim - left) .. lim, lim = s + shift.  The rule is varq_window_split_takes.  The block's first key is a_blk = max(0, q0 + shift - left)
// and its walk begins at tile t_lo = a_blk / 64 in the place of tile 0: staging, the page walk (one division at the head of the block, ids
// still requested a tile ahead) and the loop all start there, so no key and no table entry below t_lo * 64 is read.  t_lo < nt in every
// live block: a_blk <= q0 + shift < kv_end.  A tile wholly below the wave's first window start max(0, wq0 + shift - left) is skipped by a
// wave-uniform test, as a tile above the diagonal is; the low mask key >= max(0, lim - left) runs only in tiles below the wave's LAST window
// start.  A row may meet its first attended key tiles after its wave's first one: the running max is still -inf then, the DevLen guards'
// case.  With left >= Sk_b - 1 every one of these is the VarQMix expression: t_lo = 0, no tile skipped, no key masked -- same bits.
//
// Softcap<Window<VarQMix<..>>> (awq_softcap.hpp, awq_attn_varq_softcap[_kv8], awq_attn_paged_varq_softcap[_kv8]): the windowed form with the
// logit x = cap_log2e * softcap_tanh(s * scale_over_cap) in the place of x = s * scale_log2e.  The mask selects behind it, so a masked logit
// is -inf and a dead key's score, a NaN included, is never looked at; nothing else differs.
//
// The device-length forms take their PrefillLenArgs as a SECOND kernel argument.  For the host-length forms that argument is the empty
// NoLenArgs -- one padded byte behind PrefillArgs that no instruction reads: their PrefillArgs, their registers and their instruction
// stream are those of the one-argument kernel.
template <typename DT, int DH, int NW>
__global__ __launch_bounds__(NW * 64) void attn_prefill_kernel(PrefillArgs a, LenArgsOf<DT> xs) {
  const PrefillLenArgs x = len_args(xs);
  constexpr bool FT = IsFtCache<DT>::value;
  constexpr bool KV8 = IsKv8<DT>::value;
  constexpr bool DEVLEN = IsDevLen<DT>::value;
  constexpr bool PAGED = IsPaged<DT>::value;
  constexpr bool VARQ = IsVarQ<DT>::value;
  constexpr bool WINDOW = IsWindow<DT>::value;
  constexpr bool SOFTCAP = IsSoftcap<DT>::value;
  static_assert(!SOFTCAP || WINDOW, "a cap exists on the windowed form only");
  static_assert(!PAGED || DEVLEN, "the paged form reads its lengths on the device");
  static_assert(!FT || !DEVLEN, "the FT caches take a host length");
  static_assert(!VARQ || DEVLEN, "packed queries read their lengths on the device");
  static_assert(!WINDOW || IsVarQMix<DT>::value, "a window exists on the mixed packed form only");
  using vec8 = typename DT::vec8;
  using elem = typename DT::elem;
  constexpr int NT = NW * 64;
  constexpr int CPR = DH / 8;             // 16-byte chunks per row
  constexpr int LOADS = kKV * CPR / NT;   // chunks of one K (or V) tile per thread
  constexpr int KS = DH / 16;             // k-steps of Q K^T
  constexpr int DB = DH / 32;             // 32-column blocks of O
  static_assert(LOADS >= 1 && LOADS * NT == kKV * CPR, "tile does not divide over the block");
  __shared__ __attribute__((aligned(16))) uint16_t k_s[2][kKV * DH];
  __shared__ __attribute__((aligned(16))) uint16_t v_s[2][kKV * DH];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bi = blockIdx.x;
  const int h = bi % a.H;
  bi /= a.H;
  const int b = bi % a.B;
  const int rank = bi / a.B;
  int Sq = a.Sq, ntiles = a.ntiles;
  long long row0 = 0, row_end = 0, sq_b = 0;  // VarQ: the sequence's first packed row, the end of its rows, Sq_b before the clamp
  (void)row0, (void)row_end, (void)sq_b;
  if constexpr (VARQ) {  // two scalar loads; everything below depends on them
    const const_i32_t cu = as_const_i32(x.vq.cu_seqlens_q);
    const int c0 = cu[b], c1 = cu[b + 1];
    row0 = c0;
    row_end = min((long long)c1, (long long)x.vq.total_q);
    sq_b = (long long)c1 - c0;
    Sq = (int)min(max(sq_b, 0ll), (long long)x.vq.max_seqlen_q);
    ntiles = (Sq + NW * kMfmaRows - 1) / (NW * kMfmaRows);
    if (rank >= ntiles) return;  // a rank the host's bound paid for and this sequence does not need; Sq_b = 0: every block
  }
  const int tile = a.causal ? ntiles - 1 - rank : rank;
  const int kvh = h / a.G;
  const int q0 = tile * (NW * kMfmaRows);
  int Sk = a.Sk;
  bool live = true;
  (void)live;
  if constexpr (DEVLEN) {  // one scalar load; the Q loads below do not depend on it and are issued beside it
    // 64 bits: no entry can wrap into an active length
    const long long len = (long long)x.seqlens_k[b] + (VARQ ? (x.vq.lens_before_step ? sq_b : 0ll) : (long long)x.seqlen_offset);
    if constexpr (IsVarQMix<DT>::value) {  // the split pair's sequence: nothing of it is read or written here
      if constexpr (WINDOW) {
        if (varq_window_split_takes(sq_b, len, x.vq.max_seqlen_q, x.max_seqlen_k, split_args(xs), window_args(xs))) return;
      } else {
        if (varq_split_takes(sq_b, len, x.vq.max_seqlen_q, x.max_seqlen_k, split_args(xs))) return;
      }
    }
    Sk = (int)len;
    live = len >= 1 && len <= x.max_seqlen_k;
    if constexpr (VARQ) {
      live = live && sq_b == Sq;  // Sq_b < 0 never gets here (ntiles = 0); Sq_b > max_seqlen_q: inactive
      Sk = live ? Sk : 1;         // (an inactive sequence forms no address from its length; keep the arithmetic below inside int)
    }
  }
  const int shift = Sk - Sq;
  const int q_last = min(q0 + NW * kMfmaRows, Sq) - 1;
  const int kv_end = a.causal ? min(Sk, q_last + shift + 1) : Sk;  // keys [0, kv_end) matter to this block
  const int nt = (kv_end + kKV - 1) / kKV;

  const int wq0 = q0 + wave * kMfmaRows;
  const bool wave_on = wq0 < Sq;                   // (a wave past the last row still stages K / V and meets the barriers)
  const int qi = min(wq0 + r, Sq - 1);             // rows >= Sq compute row Sq - 1 again and are not stored
  const int lim = a.causal ? qi + shift : Sk - 1;                                 // last key this lane's row attends
  const int wave_max = a.causal ? min(wq0 + kMfmaRows - 1, Sq - 1) + shift : Sk - 1;  // .. any row of the wave
  const int wave_min = a.causal ? wq0 + shift : Sk - 1;                           // every row of the wave attends keys <= this
  // Window (causal only): the block's first tile, this lane's first key, and the first / last window start of the wave's rows
  int t_lo = 0, lo = 0, wave_lo = 0, wave_lo_max = 0;
  unsigned span = 0;  // lim - lo, the width of this lane's window
  (void)lo, (void)span, (void)wave_lo, (void)wave_lo_max;
  if constexpr (WINDOW) {
    const long long left = window_args(xs).left;
    t_lo = (int)(max(0ll, (long long)q0 + shift - left) / kKV);
    // a row that attends nothing (lim < 0) gets a start no key reaches and an empty span
    lo = lim < 0 ? 0x40000000 : (int)max(0ll, (long long)lim - left);
    span = lim < 0 ? 0u : (unsigned)(lim - lo);
    wave_lo = (int)max(0ll, (long long)wave_min - left);
    wave_lo_max = (int)max(0ll, (long long)wave_max - left);
  }

  // Q: the B operand of S^T = K Q^T, lane (r, hh) holds Q[row r][16 ks + 8 hh + 0..7]
  // VarQ: the packed row of (b, qi), clamped into the tensors before it forms an address; a store is guarded by row < min(cu[b + 1], total_q)
  const long long qrow = VARQ ? min(max(row0 + qi, 0ll), (long long)x.vq.total_q - 1) : 0ll;
  const bool row_ok = VARQ ? row0 + qi < row_end : true;
  (void)qrow, (void)row_ok;
  vec8 qf[KS];
  {
    const uint16_t* qp = a.q + (long long)b * a.q_bs + (long long)qi * a.q_rs + (long long)h * DH + 8 * hh;
    if constexpr (VARQ) qp = a.q + qrow * a.q_rs + (long long)h * DH + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(qp + 16 * ks));
  }

  if constexpr (DEVLEN) {
    if (!live || kv_end < 1) {  // inactive, or no row of the q tile attends a key: zero rows, no K / V load
      if (wq0 + r < Sq && row_ok) {
        uint16_t* op = a.out + (((long long)b * a.Sq + qi) * a.H + h) * DH + 4 * hh;
        if constexpr (VARQ) op = a.out + (qrow * a.H + h) * DH + 4 * hh;
#pragma unroll
        for (int c = 0; c < DH / 8; ++c) *reinterpret_cast<u32x2*>(op + 8 * c) = u32x2{0u, 0u};
      }
      return;
    }
  }

  const long long pool_b = PAGED ? 0 : b;  // Paged: the pools have no batch dimension, the page offset is added per tile
  const uint16_t* kb = a.k + pool_b * a.k_bs + (FT ? (long long)kvh * a.k_rs * CPR : (long long)kvh * DH);
  const uint16_t* vb = a.v + pool_b * a.v_bs + (FT ? (long long)kvh * a.k_rs * CPR : (long long)kvh * DH);
  using stage_t = typename std::conditional<KV8, u32x2, u32x4>::type;
  stage_t kr[LOADS], vr[LOADS];
  float ksc[KV8 ? LOADS : 1], vsc[KV8 ? LOADS : 1];  // Kv8: the scale of the chunk's row
  const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(a.k) + pool_b * a.k_bs + (long long)kvh * DH;
  const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(a.v) + pool_b * a.v_bs + (long long)kvh * DH;
  const float* ksb = KV8 ? a.k_scale + pool_b * a.ks_bs + kvh : nullptr;
  const float* vsb = KV8 ? a.v_scale + pool_b * a.vs_bs + kvh : nullptr;
  // FT: the K chunks of a tile go to the threads with the KEY fastest (NT is a multiple of 64, so a wave reads 64 consecutive positions
  // of one chunk index: 1 KiB contiguous in the cache) and land in the same LDS image; V rows are DH contiguous elements in the cache
  // too, so V keeps the chunk-fastest mapping.  Keys >= Sk are clamped to Sk - 1 like rows: no position outside the Sk keys is read.
  // Paged: page = the (clamped) id of the tile's page, ro = the tile's first row inside it; unused otherwise
  auto stage_load = [&](int t0, int page, int ro) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      const long long g = min(t0 + row, Sk - 1);
      if constexpr (FT) {
        const int krow = c % kKV, kch = c / kKV;
        const long long kg = min(t0 + krow, Sk - 1);
        kr[i] = *reinterpret_cast<const u32x4*>(kb + kch * a.k_rs + kg * 8);
        vr[i] = *reinterpret_cast<const u32x4*>(vb + g * DH + ch * 8);
      } else if constexpr (PAGED) {
        const long long prow = ro + (g - t0);  // row of the page: < page_size, the tile does not straddle
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
      if constexpr (FT) {
        *reinterpret_cast<u32x4*>(&k_s[buf][k_off<DH>(c % kKV, c / kKV)]) = kr[i];
        *reinterpret_cast<u32x4*>(&v_s[buf][v_off<DH>(row, ch)]) = vr[i];
      } else if constexpr (KV8) {
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

  // Paged: the ids of tiles 0 and 1, both requested before the first K / V load is issued.  The table is read through the constant
  // address space: nothing writes it while the kernel runs, and only so does the load inside the loop stay a SCALAR load -- behind a
  // barrier the compiler otherwise takes memory for clobbered and reads the entry with a vector load and a full wait at the head of
  // every tile.  An entry is REQUESTED at the head of an iteration and clamped (page_id) behind the barrier that ends it, where the
  // wait the barrier needs anyway has covered it.
  typedef const int __attribute__((address_space(4))) * const_table_t;
  const const_table_t table = PAGED ? reinterpret_cast<const_table_t>(reinterpret_cast<uintptr_t>(x.pg.block_table + (long long)b * x.pg.bt_rs)) : nullptr;
  int pg_i = 0, pg_ro = 0, pg_cur = 0, ro_cur = 0, pg_nxt = 0, ro_nxt = 0;
  auto next_entry = [&]() {  // (pg_i, pg_ro) -> the tile 64 keys on; returns its table entry, not yet clamped
    pg_ro += kKV;
    if (pg_ro == x.pg.page_size) {
      pg_ro = 0;
      ++pg_i;
    }
    return table[pg_i];
  };
  if constexpr (PAGED) {
    if constexpr (WINDOW) {  // the walk starts at tile t_lo: the block's one division
      pg_i = t_lo * kKV / x.pg.page_size;
      pg_ro = t_lo * kKV - pg_i * x.pg.page_size;
      ro_cur = pg_ro;
    }
    pg_cur = page_id(table[pg_i], x.pg.num_pages);
    if (t_lo + 1 < nt) {
      pg_nxt = page_id(next_entry(), x.pg.num_pages);
      ro_nxt = pg_ro;
    }
  }

  stage_load(t_lo * kKV, pg_cur, ro_cur);
  stage_write(t_lo & 1);
  // Q has arrived before the loop starts: a wait for it inside the loop would be a vmcnt(0) behind the loads the loop has just
  // issued (the counter retires in order), which is exactly the overlap the staging exists for
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  __syncthreads();

  for (int t = t_lo; t < nt; ++t) {
    const int buf = t & 1, t0 = t * kKV;
    const bool more = t + 1 < nt;
    int pg_n2 = pg_nxt, ro_n2 = ro_nxt;
    if constexpr (PAGED) {
      if (t + 2 < nt) {  // the entry tile t + 2 will load with in the next iteration: a whole tile ahead of its use
        pg_n2 = next_entry();
        ro_n2 = pg_ro;
      }
    }
    if (more) stage_load(t0 + kKV, pg_nxt, ro_nxt);

    bool below = false;  // Window: the tile lies wholly below every window start of the wave
    if constexpr (WINDOW) below = t0 + kKV <= wave_lo;
    if (wave_on && t0 <= wave_max && !below) {
      // ---- S^T = K Q^T: s[kb2][e] = key t0 + 32 kb2 + (e & 3) + 8 (e >> 2) + 4 hh, query row r ----
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
      const bool need_mask = t0 + kKV - 1 > wave_min;
      const bool need_lo = WINDOW && t0 < wave_lo_max;  // some row of the wave starts inside or behind this tile
      float mx = -INFINITY;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[kb2][e] * a.scale_log2e;
          if constexpr (SOFTCAP) x = cap_args(xs).cap_log2e * softcap_tanh(s[kb2][e] * cap_args(xs).scale_over_cap);
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
      const float m_new = fmaxf(m_run, mx);  // host length: finite from the first tile on, key 0 is attended by every row
      float m_sub = m_new;
      if constexpr (DEVLEN) m_sub = m_new == -INFINITY ? 0.f : m_new;  // a row that has attended nothing so far
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
    if constexpr (PAGED) {
      pg_nxt = page_id(pg_n2, x.pg.num_pages);  // (clamping an id twice changes nothing)
      ro_nxt = ro_n2;
    }
  }

  // ---- O / l, rounded to T once; lane (r, hh) holds O[row r][32 db + 8 g4 + 4 hh + 0..3] in o[db][4 g4 + 0..3] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (wq0 + r < Sq && row_ok) {
    float inv = 1.0f / l_tot;
    if constexpr (DEVLEN) inv = l_tot > 0.f ? inv : 0.f;  // a row that attended nothing: zeros (o is 0), never 0 * Inf
    uint16_t* op = a.out + (((long long)b * a.Sq + qi) * a.H + h) * DH + 4 * hh;
    if constexpr (VARQ) op = a.out + (qrow * a.H + h) * DH + 4 * hh;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const u32 w0 = (u32)DT::from_float(o[db][4 * g4] * inv) | ((u32)DT::from_float(o[db][4 * g4 + 1] * inv) << 16);
        const u32 w1 = (u32)DT::from_float(o[db][4 * g4 + 2] * inv) | ((u32)DT::from_float(o[db][4 * g4 + 3] * inv) << 16);
        *reinterpret_cast<u32x2*>(op + 32 * db + 8 * g4) = u32x2{w0, w1};
      }
  }
}

template <typename DT, int DH>
void launch_nw(const PrefillArgs& a, int nw, int blocks, hipStream_t st) {
  switch (nw) {
    case 8: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 8>), dim3(blocks), dim3(512), 0, st, a, NoLenArgs{}); break;
    case 4: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 4>), dim3(blocks), dim3(256), 0, st, a, NoLenArgs{}); break;
    default: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 2>), dim3(blocks), dim3(128), 0, st, a, NoLenArgs{}); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// fused_rope_with_pos_forward_func (awq/kernels/csrc/rope_new/fused_rope_with_pos.cu:33-72, 263-333).  input [n0, n1, h, d] with
// strides (s0, s1, sh, 1); the angle of (i0, i1, ., c), c < d2, is freqs[(i1 * n0 + i0) * d2 + c] (:45 with gridDim.x = n0 -- the
// reference's own index, meaningful when one of n0, n1 is 1); partner c + d2/2 negated for the first half, c - d2/2 for the second
// (:51-55); x cos + x_rot sin in fp32, rounded to T once; columns >= d2 copied (:60-70).  One thread = 8 consecutive columns of one
// (i0, i1) over all heads (the sincosf of a column is evaluated once, as in the reference), 16-byte loads and stores.
// ------------------------------------------------------------------------------------------------------------------------------
struct RopePosArgs {
  const uint16_t* in;
  const float* freqs;
  uint16_t* out;
  int n0, n1, h, d, d2;
  long long s0, s1, sh, o0, o1, oh;
};

template <typename DT>
__global__ __launch_bounds__(256) void rope_with_pos_kernel(RopePosArgs a) {
  const int cpr = a.d >> 3;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)a.n0 * a.n1 * cpr) return;
  const int ch = (int)(id % cpr);
  const long long pos = id / cpr;
  const int i1 = (int)(pos % a.n1), i0 = (int)(pos / a.n1);
  const int c0 = ch * 8;
  const uint16_t* src = a.in + i0 * a.s0 + i1 * a.s1;
  uint16_t* dst = a.out + i0 * a.o0 + i1 * a.o1;
  if (c0 >= a.d2) {
    for (int hd = 0; hd < a.h; ++hd)
      *reinterpret_cast<u32x4*>(dst + hd * a.oh + c0) = *reinterpret_cast<const u32x4*>(src + hd * a.sh + c0);
    return;
  }
  const RopeLane rope(a.freqs + ((long long)i1 * a.n0 + i0) * a.d2 + c0, c0, a.d2);  // awq_rope.hpp
  for (int hd = 0; hd < a.h; ++hd) *reinterpret_cast<u32x4*>(dst + hd * a.oh + c0) = rope.rotate<DT>(src + hd * a.sh, c0);
}

// rotary_embedding_neox (awq/kernels/csrc/position_embedding/pos_encoding_kernels.cu:12-87): in place on query and key
// [tokens, heads, head_size]; cos_sin_cache [max_pos, rot_dim] = cos | sin.  One thread = 8 consecutive rotation pairs of one
// (token, head).  The rotation is evaluated in fp32 and rounded once (the reference rounds every product and sum to T).
template <typename DT>
__global__ __launch_bounds__(256) void rope_neox_kernel(const long long* __restrict__ positions, uint16_t* __restrict__ query,
                                                        uint16_t* __restrict__ key, const uint16_t* __restrict__ cache, int tokens, int heads,
                                                        int head_size, int rot_dim, int max_pos) {
  const int embed = rot_dim >> 1, cpe = embed >> 3;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)tokens * heads * cpe) return;
  const int ch = (int)(id % cpe);
  const long long th = id / cpe;  // token * heads + head
  const long long token = th / heads;
  long long pos = positions[token];
  pos = pos < 0 ? 0 : (pos >= max_pos ? max_pos - 1 : pos);  // (the reference reads whatever lies there)
  const uint16_t* cp = cache + pos * rot_dim + ch * 8;
  float cs[8], sn[8];
  unpack8<DT>(*reinterpret_cast<const u32x4*>(cp), cs);
  unpack8<DT>(*reinterpret_cast<const u32x4*>(cp + embed), sn);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    uint16_t* p = (which ? key : query) + th * head_size + ch * 8;
    float x[8], y[8], rx[8], ry[8];
    unpack8<DT>(*reinterpret_cast<const u32x4*>(p), x);
    unpack8<DT>(*reinterpret_cast<const u32x4*>(p + embed), y);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      rx[e] = __builtin_fmaf(x[e], cs[e], -(y[e] * sn[e]));
      ry[e] = __builtin_fmaf(y[e], cs[e], x[e] * sn[e]);
    }
    *reinterpret_cast<u32x4*>(p) = pack8<DT>(rx);
    *reinterpret_cast<u32x4*>(p + embed) = pack8<DT>(ry);
  }
}

}  // namespace

// Host plan: the q tile (rows per block) of a launch, from what was measured on the MI355X (tools/attn_prefill_bench.py shapes, bf16, each
// tile size forced in turn; DESIGN.md "Prefill attention"): 128 rows (4 waves, two blocks per CU) is the fastest or within 1 % of it
// almost everywhere.  Dh = 128 gains 5 % from 256 rows once that still leaves two blocks per CU (Llama-3-8B at S = 4096); Dh = 64
// never does, and prefers 64 rows while 128-row tiles leave fewer than two blocks per CU (Falcon-like at S <= 512: 12 %).  Depends on
// host arguments only.
int attn_prefill_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* q_tile_rows,
                      int* blocks) {
  (void)nheads_kv;
  (void)seqlen_k;
  (void)causal;
  const long long bh = (long long)batch * nheads;
  auto nblocks = [&](int rows) { return bh * ((seqlen_q + rows - 1) / rows); };
  int rows = 128;
  if (head_dim == 128 && nblocks(256) >= 2 * kCUs) rows = 256;
  else if (head_dim == 64 && nblocks(128) < 2 * kCUs) rows = 64;
  if (g_force_rows) rows = g_force_rows;
  *q_tile_rows = rows;
  *blocks = (int)nblocks(rows);
  return 0;
}

// Host plan of a packed-query launch (awq_varq.hpp).  PROVISIONAL, not a measurement: 64 rows while no sequence can fill more
// (max_seqlen_q <= 64), otherwise what attn_prefill_plan gives for a rectangle of max_seqlen_q rows, capped at 128 -- only the 64- and
// 128-row kernels exist for packed queries.  The knob attn_prefill_rows forces 64 or 128; a forced 256 leaves this plan's own choice in
// place.  *blocks is the grid: ceil(max_seqlen_q / rows) ranks for every (sequence, head), whatever the sequences turn out to hold.
int attn_varq_plan(int batch, int nheads, int nheads_kv, int head_dim, int max_seqlen_q, int* q_tile_rows, int* blocks) {
  (void)nheads_kv;
  const long long bh = (long long)batch * nheads;
  auto nblocks = [&](int rows) { return bh * ((max_seqlen_q + rows - 1) / rows); };
  int rows = 128;
  if (max_seqlen_q <= 64 || (head_dim == 64 && nblocks(128) < 2 * kCUs)) rows = 64;
  if (g_force_rows == 64 || g_force_rows == 128) rows = g_force_rows;
  *q_tile_rows = rows;
  *blocks = (int)nblocks(rows);
  return 0;
}

int attn_prefill_tune_set(const char* key, int value) {
  if (strcmp(key, "attn_prefill_rows") != 0 || (value != 0 && value != 64 && value != 128 && value != 256)) return -1;
  g_force_rows = value;
  return 0;
}

int launch_attn_prefill(const void* q, const void* k, const void* v, void* out, int B, int Sq, int Sk, int H, int Hkv, int Dh, long long q_bs,
                        long long q_rs, long long k_bs, long long k_rs, long long v_bs, long long v_rs, float scale, int causal, int dtype,
                        hipStream_t st) {
  PrefillArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k;
  a.v = (const uint16_t*)v;
  a.out = (uint16_t*)out;
  a.q_bs = q_bs;
  a.q_rs = q_rs;
  a.k_bs = k_bs;
  a.k_rs = k_rs;
  a.v_bs = v_bs;
  a.v_rs = v_rs;
  a.B = B;
  a.Sq = Sq;
  a.Sk = Sk;
  a.H = H;
  a.G = H / Hkv;
  a.causal = causal ? 1 : 0;
  a.scale_log2e = scale * 1.4426950408889634f;
  a.k_scale = a.v_scale = nullptr;
  a.ks_bs = a.ks_rs = a.vs_bs = a.vs_rs = 0;
  int rows = 0, blocks = 0;
  attn_prefill_plan(B, H, Hkv, Dh, Sq, Sk, causal, &rows, &blocks);
  a.ntiles = (Sq + rows - 1) / rows;
  const int nw = rows / kMfmaRows;
  if (dtype == 0) {
    if (Dh == 128) launch_nw<F16, 128>(a, nw, blocks, st);
    else launch_nw<F16, 64>(a, nw, blocks, st);
  } else {
    if (Dh == 128) launch_nw<BF16, 128>(a, nw, blocks, st);
    else launch_nw<BF16, 64>(a, nw, blocks, st);
  }
  return 0;
}

// The same launch with K / V read from the FT caches: key j of the attention is cache position kv_start + j.  The plan is asked with the
// same arguments as the natural-layout launch of the same problem, so the q tile -- and with it every bit of the result -- is the same.
int launch_attn_prefill_ftcache(const void* q, const void* k_cache, const void* v_cache, void* out, int B, int Sq, int kv_start, int Sk, int H,
                                int Hkv, int Dh, int Lmax, long long q_bs, long long q_rs, float scale, int causal, int dtype, hipStream_t st) {
  PrefillArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k_cache + (long long)kv_start * 8;
  a.v = (const uint16_t*)v_cache + (long long)kv_start * Dh;
  a.out = (uint16_t*)out;
  a.q_bs = q_bs;
  a.q_rs = q_rs;
  a.k_bs = a.v_bs = (long long)Hkv * Lmax * Dh;
  a.k_rs = (long long)Lmax * 8;
  a.v_rs = Dh;
  a.B = B;
  a.Sq = Sq;
  a.Sk = Sk;
  a.H = H;
  a.G = H / Hkv;
  a.causal = causal ? 1 : 0;
  a.scale_log2e = scale * 1.4426950408889634f;
  a.k_scale = a.v_scale = nullptr;
  a.ks_bs = a.ks_rs = a.vs_bs = a.vs_rs = 0;
  int rows = 0, blocks = 0;
  attn_prefill_plan(B, H, Hkv, Dh, Sq, Sk, causal, &rows, &blocks);
  a.ntiles = (Sq + rows - 1) / rows;
  const int nw = rows / kMfmaRows;
  if (dtype == 0) {
    if (Dh == 128) launch_nw<FtCache<F16>, 128>(a, nw, blocks, st);
    else launch_nw<FtCache<F16>, 64>(a, nw, blocks, st);
  } else {
    if (Dh == 128) launch_nw<FtCache<BF16>, 128>(a, nw, blocks, st);
    else launch_nw<FtCache<BF16>, 64>(a, nw, blocks, st);
  }
  return 0;
}

// The same launch on the FP8 cache: k / v are e4m3 codes [B, Sk, Hkv, Dh] (strides in bytes), k_scale / v_scale their fp32 scales
// [B, Sk, Hkv] (strides in floats).  The plan is asked with the same arguments, so the q tile and every bit behind the staging are those of
// launch_attn_prefill on the dequantised tensors.
int launch_attn_prefill_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int B, int Sq,
                            int Sk, int H, int Hkv, int Dh, long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs,
                            long long v_rs, long long ks_bs, long long ks_rs, long long vs_bs, long long vs_rs, float scale, int causal, int dtype,
                            hipStream_t st) {
  PrefillArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k;
  a.v = (const uint16_t*)v;
  a.out = (uint16_t*)out;
  a.q_bs = q_bs;
  a.q_rs = q_rs;
  a.k_bs = k_bs;
  a.k_rs = k_rs;
  a.v_bs = v_bs;
  a.v_rs = v_rs;
  a.B = B;
  a.Sq = Sq;
  a.Sk = Sk;
  a.H = H;
  a.G = H / Hkv;
  a.causal = causal ? 1 : 0;
  a.scale_log2e = scale * 1.4426950408889634f;
  a.k_scale = k_scale;
  a.v_scale = v_scale;
  a.ks_bs = ks_bs;
  a.ks_rs = ks_rs;
  a.vs_bs = vs_bs;
  a.vs_rs = vs_rs;
  int rows = 0, blocks = 0;
  attn_prefill_plan(B, H, Hkv, Dh, Sq, Sk, causal, &rows, &blocks);
  a.ntiles = (Sq + rows - 1) / rows;
  const int nw = rows / kMfmaRows;
  if (dtype == 0) {
    if (Dh == 128) launch_nw<Kv8<F16>, 128>(a, nw, blocks, st);
    else launch_nw<Kv8<F16>, 64>(a, nw, blocks, st);
  } else {
    if (Dh == 128) launch_nw<Kv8<BF16>, 128>(a, nw, blocks, st);
    else launch_nw<Kv8<BF16>, 64>(a, nw, blocks, st);
  }
  return 0;
}

namespace {

// L<K<DT>>: K is the cache's traits (DT, or Kv8<DT> for codes with scales), L the lengths' (DevLen, or PagedDevLen over a pool)
template <template <typename> class K, template <typename> class L>
void launch_kv_prefill_as(const PrefillArgs& a, const PrefillLenArgs& x, int Dh, int dtype, int nw, int blocks, hipStream_t st) {
  for_dtype_dh<F16, BF16>(dtype, Dh, [&](auto dt, auto dh) {
    using DT = L<K<decltype(dt)>>;
    constexpr int DH = decltype(dh)::value;
    switch (nw) {
      case 8: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 8>), dim3(blocks), dim3(512), 0, st, a, x); break;
      case 4: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 4>), dim3(blocks), dim3(256), 0, st, a, x); break;
      default: hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 2>), dim3(blocks), dim3(128), 0, st, a, x); break;
    }
  });
}
// the packed-query forms: q tiles of 128 and 64 rows only (attn_varq_plan)
template <template <typename> class K, template <typename> class L, typename X>
void launch_kv_prefill_varq_as(const PrefillArgs& a, const X& x, int Dh, int dtype, int nw, int blocks, hipStream_t st) {
  for_dtype_dh<F16, BF16>(dtype, Dh, [&](auto dt, auto dh) {
    using DT = L<K<decltype(dt)>>;
    constexpr int DH = decltype(dh)::value;
    if (nw == 4) hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 4>), dim3(blocks), dim3(256), 0, st, a, x);
    else hipLaunchKernelGGL((attn_prefill_kernel<DT, DH, 2>), dim3(blocks), dim3(128), 0, st, a, x);
  });
}
template <typename DT>
using TCache = DT;  // the T cache: the element traits themselves

}  // namespace

// The one-pass kernel over a view with every sequence's length read on the device (awq_attn_prefill_kvcache[_kv8], awq_attn_prefill_paged
// [_kv8]): dense caches or a pool of pages, T or FP8, selected by what the descriptor holds.  The plan is asked with the bound in the place
// of seqlen_k -- it ignores both -- so the q tile and the block count are the host-length launch's for the same (B, H, Dh, Sq), and the
// knob attn_prefill_rows applies.  The caller has validated the arguments: max_seqlen_k <= the capacity of the view, so the clamp to
// Sk_b - 1 stays inside a sequence's rows and every table index inside a table row.
int launch_kv_prefill(const KvAttnCall& c, hipStream_t st) {
  const KvView& kv = c.kv;
  PrefillArgs a;
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
  a.G = c.H / c.Hkv;
  a.causal = c.causal ? 1 : 0;
  a.scale_log2e = c.scale * 1.4426950408889634f;
  a.k_scale = kv.k_scale;
  a.v_scale = kv.v_scale;
  a.ks_bs = kv.ks_os, a.ks_rs = kv.ks_rs, a.vs_bs = kv.vs_os, a.vs_rs = kv.vs_rs;
  int rows = 0, blocks = 0;
  if (c.cu_seqlens_q) {  // packed queries: c.Sq is max_seqlen_q, c.seqlen_offset the flag lens_before_step; the kernel forms a.ntiles per sequence
    const PrefillLenArgs x{c.seqlens_k, 0, c.max_seqlen_k, PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer},
                           VarQArgs{c.cu_seqlens_q, c.total_q, c.Sq, c.seqlen_offset ? 1 : 0}};
    attn_varq_plan(c.B, c.H, c.Hkv, c.Dh, c.Sq, &rows, &blocks);
    a.ntiles = (c.Sq + rows - 1) / rows;
    const int nw = rows / kMfmaRows;
    if (c.window_left >= 0) {  // a windowed step (awq_window.hpp): the mixed form for every split_seqlen_q, 0 hands nothing to the split pair
      PrefillCapArgs m;
      static_cast<PrefillLenArgs&>(m) = x;
      m.sp = VarQSplitArgs{c.split_seqlen_q, c.split_min_keys};
      m.w = WindowArgs{c.window_left};
      if (c.softcap > 0.f) {  // a capped step (awq_softcap.hpp): the windowed form with the cap behind it
        m.cap = softcap_args(c.scale, c.softcap);
        if (kv.block_table) {
          if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, SoftcapWindowVarQMixPagedDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
          else launch_kv_prefill_varq_as<TCache, SoftcapWindowVarQMixPagedDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
        } else {
          if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, SoftcapWindowVarQMixDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
          else launch_kv_prefill_varq_as<TCache, SoftcapWindowVarQMixDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
        }
        return 0;
      }
      const PrefillWinArgs& w = m;
      if (kv.block_table) {
        if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, WindowVarQMixPagedDevLen>(a, w, c.Dh, c.dtype, nw, blocks, st);
        else launch_kv_prefill_varq_as<TCache, WindowVarQMixPagedDevLen>(a, w, c.Dh, c.dtype, nw, blocks, st);
      } else {
        if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, WindowVarQMixDevLen>(a, w, c.Dh, c.dtype, nw, blocks, st);
        else launch_kv_prefill_varq_as<TCache, WindowVarQMixDevLen>(a, w, c.Dh, c.dtype, nw, blocks, st);
      }
      return 0;
    }
    if (c.split_seqlen_q > 0) {  // a mixed step: the same launch, with the sequences of the split pair left alone
      PrefillMixArgs m;
      static_cast<PrefillLenArgs&>(m) = x;
      m.sp = VarQSplitArgs{c.split_seqlen_q, c.split_min_keys};
      if (kv.block_table) {
        if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, VarQMixPagedDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
        else launch_kv_prefill_varq_as<TCache, VarQMixPagedDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
      } else {
        if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, VarQMixDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
        else launch_kv_prefill_varq_as<TCache, VarQMixDevLen>(a, m, c.Dh, c.dtype, nw, blocks, st);
      }
      return 0;
    }
    if (kv.block_table) {
      if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, VarQPagedDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
      else launch_kv_prefill_varq_as<TCache, VarQPagedDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
    } else {
      if (kv.k_scale) launch_kv_prefill_varq_as<Kv8, VarQDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
      else launch_kv_prefill_varq_as<TCache, VarQDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
    }
    return 0;
  }
  const PrefillLenArgs x{c.seqlens_k, c.seqlen_offset, c.max_seqlen_k, PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer},
                         VarQArgs{nullptr, 0, 0, 0}};
  attn_prefill_plan(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.max_seqlen_k, c.causal, &rows, &blocks);
  a.ntiles = (c.Sq + rows - 1) / rows;
  const int nw = rows / kMfmaRows;
  if (kv.block_table) {
    if (kv.k_scale) launch_kv_prefill_as<Kv8, PagedDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
    else launch_kv_prefill_as<TCache, PagedDevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
  } else {
    if (kv.k_scale) launch_kv_prefill_as<Kv8, DevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
    else launch_kv_prefill_as<TCache, DevLen>(a, x, c.Dh, c.dtype, nw, blocks, st);
  }
  return 0;
}

int launch_rope_with_pos(const void* in, const float* freqs, void* out, int n0, int n1, int h, int d, int d2, long long s0, long long s1,
                         long long sh, long long o0, long long o1, long long oh, int dtype, hipStream_t st) {
  RopePosArgs a{(const uint16_t*)in, freqs, (uint16_t*)out, n0, n1, h, d, d2, s0, s1, sh, o0, o1, oh};
  const long long n = (long long)n0 * n1 * (d / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL((rope_with_pos_kernel<F16>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((rope_with_pos_kernel<BF16>), grid, dim3(256), 0, st, a);
  return 0;
}

int launch_rope_neox(const long long* positions, void* query, void* key, const void* cache, int tokens, int heads, int head_size, int rot_dim,
                     int max_pos, int dtype, hipStream_t st) {
  const long long n = (long long)tokens * heads * (rot_dim / 16);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 0)
    hipLaunchKernelGGL((rope_neox_kernel<F16>), grid, dim3(256), 0, st, positions, (uint16_t*)query, (uint16_t*)key, (const uint16_t*)cache, tokens,
                       heads, head_size, rot_dim, max_pos);
  else
    hipLaunchKernelGGL((rope_neox_kernel<BF16>), grid, dim3(256), 0, st, positions, (uint16_t*)query, (uint16_t*)key, (const uint16_t*)cache, tokens,
                       heads, head_size, rot_dim, max_pos);
  return 0;
}

}  // namespace awq
