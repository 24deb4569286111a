// rope_kv_store_natural on the FP8 KV cache (awq_kv8.hpp): rotate q and k of a fused qkv chunk, quantise k and v per (token, KV head) and
// store codes and scales, one launch.
//
//   qkv [B, S, (H + 2 Hkv) Dh] (batch and row strides of its own)  ->  q_out   [B, S, H, Dh]                          rotated, T
//                                                                      k_cache [b, start_pos + s, kvh, :]  e4m3 codes of the rotated k
//                                                                      v_cache [b, start_pos + s, kvh, :]  e4m3 codes of v
//                                                                      k_scale / v_scale [b, start_pos + s, kvh]       fp32
//
// The rotation is rope_kv_store_natural_kernel's (awq_attn_chunk_cdna4.hip), expression for expression: the angle of (b, s, ., c), c < rot,
// is freqs[(s * B + b) * rot + c] (the reference's own flat index), sincosf once per column, fmaf(x, cos, (+-x_rot) * sin) rounded to T
// once, columns >= rot copied.  q_out therefore holds that kernel's bits, and the K row that is quantised is, after its rounding to T, the
// row that kernel would have stored.
//
// Mapping: that kernel's, one thread = 8 consecutive columns of one (b, s), the column chunk fastest, walking the H query heads, the Hkv
// key heads and the Hkv value heads -- so a column's sincosf is still evaluated once.  The Dh / 8 threads of a (b, s) are consecutive
// lanes of one wave (Dh / 8 = 8 or 16 divides 64 and the block size): for every K and V head they own the head row together, and its
// max |x| is a butterfly of __shfl_xor over those lanes -- no LDS, no barrier; every lane ends up with the row's scale.  A lane stores the
// 8 code bytes of its chunk (8 or 16 lanes write one contiguous 64- or 128-byte row); the lane of chunk 0 stores the scale, an ordinary
// 4-byte store.  Nothing outside positions [start_pos, start_pos + S) of cache rows b < B is written, in the caches or in the scales.
#include "awq_device.hpp"
#include "awq_devlen.hpp"
#include "awq_kernels.hpp"
#include "awq_kv8.hpp"
#include "awq_kvcache.hpp"
#include "awq_kvstore.hpp"
#include "awq_paged.hpp"
#include "awq_rope.hpp"
#include "awq_varq.hpp"

namespace awq {
namespace {

struct RopeStoreFp8Args {
  const uint16_t* qkv;
  const float* freqs;
  uint16_t* q_out;
  uint8_t* k_cache;
  uint8_t* v_cache;
  float* k_scale;
  float* v_scale;
  long long bs, rs;  // qkv batch / row strides, elements
  int B, S, H, Hkv, rot, lmax, start;
  const int* seqlens;  // DevLen only: device int32 [B], the tokens already in each sequence's cache
  // Paged only (awq_paged.hpp): the caches and the scales are pools, page and row strides in codes (bytes) / in floats; lmax =
  // min(pages_per_seq * page_size, INT_MAX)
  PageArgs pg;
  long long k_ps, k_rs, v_ps, v_rs, ks_ps, ks_rs, vs_ps, vs_rs;
  VarQArgs vq;  // VarQ only (awq_varq.hpp): qkv / q_out are packed rows, S the host's bound max_seqlen_q, bs unused
};
// what a NORM instantiation takes: the same arguments and the per-head q/k RMSNorm behind them (rope_kv_store_natural_kernel's)
struct RopeStoreFp8NormArgs : RopeStoreFp8Args {
  QkNormArgs nm;
};

// DevLen<..> (awq_devlen.hpp, awq_rope_kv_store_natural_pos_fp8): rope_kv_store_natural_kernel's device positions.  a.freqs is the whole
// angle table [a.start rows, rot], pos_b = a.seqlens[b]; an inactive sequence (pos_b < 0 or pos_b + S > min(lmax, table rows)) gets a zero
// q_out and nothing else.  The CPR lanes of a (b, s) share b, so they leave or stay together and the butterflies below never meet a lane
// that has left.
//
// Paged<DevLen<..>> (awq_paged.hpp, awq_rope_kv_store_paged_pos_fp8): rope_kv_store_natural_kernel's paged form -- the token's page is looked
// up in the table, codes and scales go to row p % page_size of that page in their pools.
//
// VarQ<..> over the two device forms (awq_varq.hpp, awq_rope_kv_store_natural_varq_fp8 / awq_rope_kv_store_paged_varq_fp8):
// rope_kv_store_natural_kernel's packed tokens -- the owner of packed row t is looked up in cu_seqlens_q, and the thread goes on as thread
// (b, t - cu[b]) of the rectangular form.  The CPR lanes of a token share t, so the lookup keeps them together.
//
// NORM (the *_fp8_qknorm entries; awq_rope.hpp): rope_kv_store_natural_kernel's per-head RMSNorm of q and k before the rotation.  The sum
// of squares of a head row travels over the CPR lanes of its token as max |x| does below, for the q heads as well as the k heads; the lanes
// of a token leave or stay together at every exit above, so that butterfly too never meets a lane that has left.  The quantiser then sees
// the normalised, rotated k row; V is untouched.  NORM = false is the kernel without any of this.
template <typename DT, int DH, bool NORM = false>
__global__ __launch_bounds__(256) void rope_kv_store_natural_fp8_kernel(std::conditional_t<NORM, RopeStoreFp8NormArgs, RopeStoreFp8Args> a) {
  constexpr bool DEVLEN = IsDevLen<DT>::value;
  constexpr bool PAGED = IsPaged<DT>::value;
  constexpr bool VARQ = IsVarQ<DT>::value;
  static_assert(!PAGED || DEVLEN, "the paged form reads its positions on the device");
  static_assert(!VARQ || DEVLEN, "packed tokens read their positions on the device");
  constexpr int CPR = DH / 8;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  int ch, s, b;
  long long S = a.S;      // the tokens the sequence brings: a.S, or Sq_b of a packed step
  long long tok_row = 0;  // VarQ: the token's packed row, < total_q by the grid guard and < cu[b + 1] by the lookup
  (void)tok_row;
  if constexpr (VARQ) {
    if (id >= (long long)a.vq.total_q * CPR) return;  // (the CPR lanes of a token share every test below: they leave or stay together)
    ch = (int)(id % CPR);
    tok_row = id / CPR;
    long long s64;
    if (!varq_owner(as_const_i32(a.vq.cu_seqlens_q), a.B, (int)tok_row, b, s64, S)) return;  // a padding row: nobody's
    s = (int)s64;  // (beyond int only under an inactive S, which leaves below before s is used)
  } else {
    if (id >= (long long)a.B * a.S * CPR) return;  // (the CPR lanes of a (b, s) leave or stay together)
    ch = (int)(id % CPR);
    s = (int)((id / CPR) % a.S);
    b = (int)(id / ((long long)a.S * CPR));
  }
  const int c0 = ch * 8, half = a.rot >> 1;
  const uint16_t* row = a.qkv + (VARQ ? tok_row * a.rs : b * a.bs + s * a.rs);
  const uint16_t* ks = row + (long long)a.H * DH;  // the K heads follow the H query heads
  const uint16_t* vs = row + (long long)(a.H + a.Hkv) * DH;
  uint16_t* qd = a.q_out + (VARQ ? tok_row : (long long)b * a.S + s) * a.H * DH + c0;
  int start = a.start;
  if constexpr (DEVLEN) {
    start = a.seqlens[b];
    if (start < 0 || (VARQ && S > a.vq.max_seqlen_q) || (long long)start + S > (long long)min(a.lmax, a.start)) {
      for (int hd = 0; hd < a.H; ++hd) *reinterpret_cast<u32x4*>(qd + hd * DH) = u32x4{0u, 0u, 0u, 0u};
      return;
    }
  }
  // (token, head 0) of the caches and of the scales; Paged: 0, the pointers below carry the token's row of each pool
  const long long tok = PAGED ? 0 : ((long long)b * a.lmax + start + s) * a.Hkv;
  uint8_t *kc = a.k_cache, *vc = a.v_cache;
  float *ksc = a.k_scale, *vsc = a.v_scale;
  if constexpr (PAGED) {
    const int p = start + s, pi = p / a.pg.page_size;
    const long long page = page_id(a.pg.block_table + (long long)b * a.pg.bt_rs, pi, a.pg.num_pages), pr = p - pi * a.pg.page_size;
    kc += page * a.k_ps + pr * a.k_rs;
    vc += page * a.v_ps + pr * a.v_rs;
    ksc += page * a.ks_ps + pr * a.ks_rs;
    vsc += page * a.vs_ps + pr * a.vs_rs;
  }

  // one head row of T (this lane's chunk w of it) -> codes and scale
  auto quant_store = [&](const u32x4& w, uint8_t* cache, float* scale, int hd) {
    float x[8];
    unpack8<DT>(w, x);
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[e]));
#pragma unroll
    for (int m = 1; m < CPR; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    const float sc = kv8_scale(amax);
    *reinterpret_cast<u32x2*>(cache + (tok + hd) * DH + c0) = kv8_quant8(x, sc);
    if (ch == 0) scale[tok + hd] = sc;
  };

  // this lane's chunk of one head row after the rotation, as T bits (columns >= rot are copied); lanes of one row may take either side
  // and meet again behind it
  const bool rot_lane = c0 < a.rot;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sn[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int pc = c0;
  float sign = 1.f;
  if (rot_lane) {
    const float* fr = a.freqs + (DEVLEN ? (long long)start + s : (long long)s * a.B + b) * a.rot + c0;
    const f32x4 f0 = *reinterpret_cast<const f32x4*>(fr), f1 = *reinterpret_cast<const f32x4*>(fr + 4);
    const float ang[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
    for (int e = 0; e < 8; ++e) sincosf(ang[e], &sn[e], &cs[e]);
    const bool first = c0 + half < a.rot;
    pc = first ? c0 + half : c0 - half;
    sign = first ? -1.f : 1.f;
  }
  auto rotated = [&](const uint16_t* hp) -> u32x4 {
    const u32x4 w = *reinterpret_cast<const u32x4*>(hp + c0);
    if (!rot_lane) return w;
    float x[8], y[8], res[8];
    unpack8<DT>(w, x);
    unpack8<DT>(*reinterpret_cast<const u32x4*>(hp + pc), y);
#pragma unroll
    for (int e = 0; e < 8; ++e) res[e] = __builtin_fmaf(x[e], cs[e], (sign * y[e]) * sn[e]);
    return pack8<DT>(res);
  };

  if constexpr (NORM) {
    const QkNormLane gq(a.nm.q_gamma, c0, pc), gk(a.nm.k_gamma, c0, pc);
    qk_norm_rotate_heads<DT, DH>(row, a.H, c0, pc, rot_lane, cs, sn, sign, gq, a.nm.eps,
                                 [&](int hd, const u32x4& w) { *reinterpret_cast<u32x4*>(qd + hd * DH) = w; });
    // (n = a.Hkv is the call's: every lane of the wave stores the same heads, so quant_store's butterfly meets all lanes of its token)
    qk_norm_rotate_heads<DT, DH>(ks, a.Hkv, c0, pc, rot_lane, cs, sn, sign, gk, a.nm.eps,
                                 [&](int hd, const u32x4& w) { quant_store(w, kc, ksc, hd); });
  } else {
    for (int hd = 0; hd < a.H; ++hd) *reinterpret_cast<u32x4*>(qd + hd * DH) = rotated(row + hd * DH);
    for (int hd = 0; hd < a.Hkv; ++hd) quant_store(rotated(ks + hd * DH), kc, ksc, hd);
  }
  for (int hd = 0; hd < a.Hkv; ++hd) quant_store(*reinterpret_cast<const u32x4*>(vs + hd * DH + c0), vc, vsc, hd);
}

}  // namespace

// launch_kv_store's FP8 half: the same forms (the rectangle or a packed step; host position, device positions, device positions over
// pools) with codes and scales
int launch_kv_store_fp8(const KvStoreCall& c, hipStream_t st) {
  const KvView& kv = c.kv;
  RopeStoreFp8Args a{(const uint16_t*)c.qkv, c.freqs, (uint16_t*)c.q_out, (uint8_t*)kv.k, (uint8_t*)kv.v, (float*)kv.k_scale, (float*)kv.v_scale,
                     c.bs, c.rs, c.B, c.S, c.H, c.Hkv, c.rot, kv.capacity(), c.cache_seqlens ? c.table_rows : c.start_pos, c.cache_seqlens};
  if (kv.block_table) {
    a.pg = PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer};
    a.k_ps = kv.k_os, a.k_rs = kv.k_rs, a.v_ps = kv.v_os, a.v_rs = kv.v_rs;
    a.ks_ps = kv.ks_os, a.ks_rs = kv.ks_rs, a.vs_ps = kv.vs_os, a.vs_rs = kv.vs_rs;
  }
  if (c.cu_seqlens_q) a.vq = VarQArgs{c.cu_seqlens_q, c.total_q, c.max_seqlen_q, 0};
  if (c.q_gamma) {  // the *_fp8_qknorm entries: the NORM instantiation of the same form
    RopeStoreFp8NormArgs an;
    static_cast<RopeStoreFp8Args&>(an) = a;
    an.nm = QkNormArgs{c.q_gamma, c.k_gamma, c.norm_eps};
    for_kv_store_form(c, [&](auto form) {
      for_dtype_dh<F16, BF16>(c.dtype, c.Dh, [&](auto dt, auto dh) {
        using DT = typename decltype(form)::template of<decltype(dt)>;
        hipLaunchKernelGGL((rope_kv_store_natural_fp8_kernel<DT, decltype(dh)::value, true>), dim3(kv_store_blocks(c)), dim3(256), 0, st, an);
      });
    });
    return 0;
  }
  for_kv_store_form(c, [&](auto form) {
    for_dtype_dh<F16, BF16>(c.dtype, c.Dh, [&](auto dt, auto dh) {
      using DT = typename decltype(form)::template of<decltype(dt)>;
      hipLaunchKernelGGL((rope_kv_store_natural_fp8_kernel<DT, decltype(dh)::value>), dim3(kv_store_blocks(c)), dim3(256), 0, st, a);
    });
  });
  return 0;
}

}  // namespace awq
