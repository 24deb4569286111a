// Prompt-side preparation of a chunk on the FasterTransformer KV cache, one launch (tinychat/modules/fused_attn.py:248-267, 439-454: two
// fused_rope_with_pos_forward_func calls, a reshape / permute / contiguous of K and two strided slice-assigns into the caches).
//
//   qkv [B, S, (H + 2 Hkv) Dh] (batch and row strides of its own)  ->  q_out [B, S, H, Dh]             rotated
//                                                                      k_cache[b, kvh, ch, start_pos + s, 0..7]   rotated
//                                                                      v_cache[b, kvh, start_pos + s, :]          copied
//
// The arithmetic is rope_with_pos_kernel's (awq_attn_prefill_cdna4.hip), expression for expression: the angle of (b, s, ., c), c < rot, is
// freqs[(s * B + b) * rot + c] (the reference's own flat index), sincosf once per column, fmaf(x, cos, (+-x_rot) * sin) rounded to T once,
// columns >= rot copied -- so q_out and the caches hold the bits the two rope calls followed by the torch stores would have left.
//
// Two thread mappings, one per half of the grid (the role is uniform over a block), every access 16 bytes:
//   * q / v blocks: one thread = 8 consecutive columns of one (b, s), the column chunk fastest, over the H query heads and then the Hkv
//     value heads.  The qkv row, the q_out row and the v_cache row are all contiguous along the chunk, so loads and stores coalesce.
//   * k blocks: one thread = 8 consecutive columns of one (b, s) over the Hkv key heads, the POSITION fastest: consecutive lanes write
//     consecutive positions of one chunk, which lie 16 bytes apart in k_cache [Bc, Hkv, Dh/8, Lmax, 8] (consecutive chunks of one position
//     would be Lmax * 16 bytes apart).  Their loads are 16 bytes per row of qkv; K is Hkv / (H + 2 Hkv) of the tensor.
// Nothing outside positions [start_pos, start_pos + S) of cache rows b < B is written.
#include "awq_device.hpp"
#include "awq_devlen.hpp"
#include "awq_kernels.hpp"
#include "awq_kvcache.hpp"
#include "awq_kvstore.hpp"
#include "awq_paged.hpp"
#include "awq_rope.hpp"
#include "awq_varq.hpp"

namespace awq {
namespace {

struct RopeStoreArgs {
  const uint16_t* qkv;
  const float* freqs;
  uint16_t* q_out;
  uint16_t* k_cache;
  uint16_t* v_cache;
  long long bs, rs;  // qkv batch / row strides, elements
  int B, S, H, Hkv, rot, lmax, start, qv_blocks;
  const int* seqlens;  // DevLen only: device int32 [B], the tokens already in each sequence's cache
  // Paged only (awq_paged.hpp): k_cache / v_cache are the pools, page and row strides in elements; lmax = min(pages_per_seq * page_size, INT_MAX)
  PageArgs pg;
  long long k_ps, k_rs, v_ps, v_rs;
  VarQArgs vq;  // VarQ only (awq_varq.hpp): qkv / q_out are packed rows, S the host's bound max_seqlen_q, bs unused
};
// what a NORM instantiation of rope_kv_store_natural_kernel takes: the same arguments and the per-head q/k RMSNorm behind them, so the
// plain instantiations keep their argument block
struct RopeStoreNormArgs : RopeStoreArgs {
  QkNormArgs nm;
};

template <typename DT, int DH>
__global__ __launch_bounds__(256) void rope_kv_store_kernel(RopeStoreArgs a) {
  constexpr int CPR = DH / 8;
  const bool k_role = (int)blockIdx.x >= a.qv_blocks;
  const long long id = (long long)(k_role ? blockIdx.x - a.qv_blocks : blockIdx.x) * 256 + threadIdx.x;
  if (id >= (long long)a.B * a.S * CPR) return;
  int b, s, ch;
  if (k_role) {
    s = (int)(id % a.S);
    ch = (int)((id / a.S) % CPR);
    b = (int)(id / ((long long)a.S * CPR));
  } else {
    ch = (int)(id % CPR);
    s = (int)((id / CPR) % a.S);
    b = (int)(id / ((long long)a.S * CPR));
  }
  const int c0 = ch * 8, half = a.rot >> 1;
  const uint16_t* row = a.qkv + b * a.bs + s * a.rs;
  const uint16_t* src = row + (k_role ? (long long)a.H * DH : 0);  // the K heads follow the H query heads
  const int heads = k_role ? a.Hkv : a.H;
  const long long pos = a.start + s;
  uint16_t* qd = a.q_out + ((long long)b * a.S + s) * a.H * DH + c0;
  uint16_t* kd = a.k_cache + (((long long)b * a.Hkv * CPR + ch) * a.lmax + pos) * 8;  // + kvh * CPR * lmax * 8
  const long long k_hs = (long long)CPR * a.lmax * 8;

  if (c0 >= a.rot) {
    for (int hd = 0; hd < heads; ++hd) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(src + hd * DH + c0);
      if (k_role) *reinterpret_cast<u32x4*>(kd + hd * k_hs) = w;
      else *reinterpret_cast<u32x4*>(qd + hd * DH) = w;
    }
  } else {
    const float* fr = a.freqs + ((long long)s * a.B + b) * a.rot + c0;
    const f32x4 f0 = *reinterpret_cast<const f32x4*>(fr), f1 = *reinterpret_cast<const f32x4*>(fr + 4);
    const float ang[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
    float cs[8], sn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sincosf(ang[e], &sn[e], &cs[e]);
    const bool first = c0 + half < a.rot;
    const int pc = first ? c0 + half : c0 - half;
    const float sign = first ? -1.f : 1.f;
    for (int hd = 0; hd < heads; ++hd) {
      float x[8], y[8], res[8];
      unpack8<DT>(*reinterpret_cast<const u32x4*>(src + hd * DH + c0), x);
      unpack8<DT>(*reinterpret_cast<const u32x4*>(src + hd * DH + pc), y);
#pragma unroll
      for (int e = 0; e < 8; ++e) res[e] = __builtin_fmaf(x[e], cs[e], (sign * y[e]) * sn[e]);
      if (k_role) *reinterpret_cast<u32x4*>(kd + hd * k_hs) = pack8<DT>(res);
      else *reinterpret_cast<u32x4*>(qd + hd * DH) = pack8<DT>(res);
    }
  }
  if (!k_role) {
    const uint16_t* vs = row + (long long)(a.H + a.Hkv) * DH + c0;
    uint16_t* vd = a.v_cache + ((long long)b * a.Hkv * a.lmax + pos) * DH + c0;  // + kvh * lmax * DH
    for (int hd = 0; hd < a.Hkv; ++hd)
      *reinterpret_cast<u32x4*>(vd + (long long)hd * a.lmax * DH) = *reinterpret_cast<const u32x4*>(vs + hd * DH);
  }
}

// The same preparation for natural-layout caches k_cache / v_cache [Bc, lmax, Hkv, DH] (tinychat's long-context path, fused_attn.py:527-537:
// two rope calls and two slice stores cache[:B, start : start + S] = x).  A cache row is Hkv * DH contiguous elements, like the K and the
// V part of a qkv row, so one mapping serves all three outputs: one thread = 8 consecutive columns of one (b, s), the column chunk
// fastest, over the H query heads, the Hkv key heads and the Hkv value heads.  The rotation is the expression above, unchanged.
//
// DevLen<..> (awq_devlen.hpp, awq_rope_kv_store_natural_pos): the position of sequence b is read on the device.  a.freqs is then the model's
// whole angle table [table rows, rot] (a.start carries the row count) and pos_b = a.seqlens[b]: token s goes to cache position pos_b + s and
// takes the angles of table row pos_b + s.  A sequence with pos_b < 0 or pos_b + S > min(lmax, table rows) is inactive: its q_out rows are
// written as zeros, nothing else is written and no address is formed from pos_b.
//
// Paged<DevLen<..>> (awq_paged.hpp, awq_rope_kv_store_paged_pos): token s of an active sequence goes to row p % page_size of page
// table[b][p / page_size], p = pos_b + s -- looked up per TOKEN, a chunk may cross page edges.  p < pages_per_seq * page_size for an active
// sequence, so the table index lies inside the row; the id is clamped into the pool.
//
// VarQ<..> over the two device forms (awq_varq.hpp, awq_rope_kv_store_natural_varq / awq_rope_kv_store_paged_varq): one thread = 8 columns
// of one PACKED token t < total_q.  Its sequence b is looked up in cu_seqlens_q (varq_owner), s = t - cu[b], and from there on the thread
// is the rectangular form's thread (b, s) of a chunk of Sq_b tokens: same position, same angles, same bits.  A sequence with
// Sq_b > max_seqlen_q is inactive as well.  Rows >= cu[B] leave before they read anything.
//
// NORM (the *_qknorm entries; awq_rope.hpp): every q and k head is RMS-normalised over its Dh columns before the rotation.  The Dh / 8
// lanes of a token own each head row together and meet in a butterfly per head, so the kernel takes the FP8 kernel's shape there: compute,
// then meet -- the lanes of a head may lie on either side of c0 < rot, and the butterfly runs before they part.  The lanes of a token
// share every early exit above it (the grid guard, a padding row, an inactive sequence: all are tests of the token or of its sequence), so
// they leave or stay together and the butterfly never meets a lane that has left.  NORM = false is the kernel without any of this.
template <typename DT, int DH, bool NORM = false>
__global__ __launch_bounds__(256) void rope_kv_store_natural_kernel(std::conditional_t<NORM, RopeStoreNormArgs, RopeStoreArgs> a) {
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
    if (id >= (long long)a.vq.total_q * CPR) return;
    ch = (int)(id % CPR);
    tok_row = id / CPR;
    long long s64;
    if (!varq_owner(as_const_i32(a.vq.cu_seqlens_q), a.B, (int)tok_row, b, s64, S)) return;  // a padding row: nobody's
    s = (int)s64;  // (beyond int only under an inactive S, which leaves below before s is used)
  } else {
    if (id >= (long long)a.B * a.S * CPR) return;
    ch = (int)(id % CPR);
    s = (int)((id / CPR) % a.S);
    b = (int)(id / ((long long)a.S * CPR));
  }
  const int c0 = ch * 8, half = a.rot >> 1;
  const uint16_t* row = a.qkv + (VARQ ? tok_row * a.rs : b * a.bs + s * a.rs);
  const uint16_t* ks = row + (long long)a.H * DH;  // the K heads follow the H query heads
  uint16_t* qd = a.q_out + (VARQ ? tok_row : (long long)b * a.S + s) * a.H * DH + c0;
  int start = a.start;
  if constexpr (DEVLEN) {
    start = a.seqlens[b];
    if (start < 0 || (VARQ && S > a.vq.max_seqlen_q) || (long long)start + S > (long long)min(a.lmax, a.start)) {
      for (int hd = 0; hd < a.H; ++hd) *reinterpret_cast<u32x4*>(qd + hd * DH) = u32x4{0u, 0u, 0u, 0u};
      return;
    }
  }
  long long crow = ((long long)b * a.lmax + start + s) * a.Hkv * DH + c0, vrow = crow;
  if constexpr (PAGED) {
    const int p = start + s, pi = p / a.pg.page_size;
    const long long page = page_id(a.pg.block_table + (long long)b * a.pg.bt_rs, pi, a.pg.num_pages), pr = p - pi * a.pg.page_size;
    crow = page * a.k_ps + pr * a.k_rs + c0;
    vrow = page * a.v_ps + pr * a.v_rs + c0;
  }
  uint16_t* kd = a.k_cache + crow;
  uint16_t* vd = a.v_cache + vrow;

  if constexpr (NORM) {
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
    const QkNormLane gq(a.nm.q_gamma, c0, pc), gk(a.nm.k_gamma, c0, pc);
    qk_norm_rotate_heads<DT, DH>(row, a.H, c0, pc, rot_lane, cs, sn, sign, gq, a.nm.eps,
                                 [&](int hd, const u32x4& w) { *reinterpret_cast<u32x4*>(qd + hd * DH) = w; });
    qk_norm_rotate_heads<DT, DH>(ks, a.Hkv, c0, pc, rot_lane, cs, sn, sign, gk, a.nm.eps,
                                 [&](int hd, const u32x4& w) { *reinterpret_cast<u32x4*>(kd + hd * DH) = w; });
  } else if (c0 >= a.rot) {
    for (int hd = 0; hd < a.H; ++hd) *reinterpret_cast<u32x4*>(qd + hd * DH) = *reinterpret_cast<const u32x4*>(row + hd * DH + c0);
    for (int hd = 0; hd < a.Hkv; ++hd) *reinterpret_cast<u32x4*>(kd + hd * DH) = *reinterpret_cast<const u32x4*>(ks + hd * DH + c0);
  } else {
    const float* fr = a.freqs + (DEVLEN ? (long long)start + s : (long long)s * a.B + b) * a.rot + c0;
    const f32x4 f0 = *reinterpret_cast<const f32x4*>(fr), f1 = *reinterpret_cast<const f32x4*>(fr + 4);
    const float ang[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
    float cs[8], sn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sincosf(ang[e], &sn[e], &cs[e]);
    const bool first = c0 + half < a.rot;
    const int pc = first ? c0 + half : c0 - half;
    const float sign = first ? -1.f : 1.f;
    for (int hd = 0; hd < a.H + a.Hkv; ++hd) {  // heads H .. H + Hkv - 1 of the row are the K heads
      float x[8], y[8], res[8];
      unpack8<DT>(*reinterpret_cast<const u32x4*>(row + hd * DH + c0), x);
      unpack8<DT>(*reinterpret_cast<const u32x4*>(row + hd * DH + pc), y);
#pragma unroll
      for (int e = 0; e < 8; ++e) res[e] = __builtin_fmaf(x[e], cs[e], (sign * y[e]) * sn[e]);
      if (hd < a.H) *reinterpret_cast<u32x4*>(qd + hd * DH) = pack8<DT>(res);
      else *reinterpret_cast<u32x4*>(kd + (hd - a.H) * DH) = pack8<DT>(res);
    }
  }
  const uint16_t* vs = row + (long long)(a.H + a.Hkv) * DH + c0;
  for (int hd = 0; hd < a.Hkv; ++hd) *reinterpret_cast<u32x4*>(vd + hd * DH) = *reinterpret_cast<const u32x4*>(vs + hd * DH);
}

}  // namespace

int launch_rope_kv_store(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int B, int S, int H, int Hkv, int Dh,
                         int rot, int lmax, int start_pos, long long bs, long long rs, int dtype, hipStream_t st) {
  const long long n = (long long)B * S * (Dh / 8);
  const int nb = (int)((n + 255) / 256);
  RopeStoreArgs a{(const uint16_t*)qkv, freqs, (uint16_t*)q_out, (uint16_t*)k_cache, (uint16_t*)v_cache, bs, rs, B, S, H, Hkv, rot, lmax,
                  start_pos, nb, nullptr};
  for_dtype_dh<F16, BF16>(dtype, Dh, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((rope_kv_store_kernel<decltype(dt), decltype(dh)::value>), dim3((unsigned)(2 * nb)), dim3(256), 0, st, a);
  });
  return 0;
}

// The natural-layout store on the T cache (a view with scales goes to awq_attn_kv8_cdna4.hip): the rectangle or a packed step, host or
// device positions, dense caches or pools -- the form is what the descriptor holds (for_kv_store_form, awq_kvstore.hpp).  Device positions:
// cache_seqlens in the place of start_pos and the whole angle table [table_rows, rot] in the place of the call's angles.  Paged: the pools
// and their table in the place of the caches, lmax = the capacity of a table row.  A packed call carries S = max_seqlen_q and bs = 0 in
// the descriptor already; its grid covers the total_q rows.
int launch_kv_store(const KvStoreCall& c, hipStream_t st) {
  const KvView& kv = c.kv;
  if (kv.k_scale) return launch_kv_store_fp8(c, st);
  RopeStoreArgs a{(const uint16_t*)c.qkv, c.freqs, (uint16_t*)c.q_out, (uint16_t*)kv.k, (uint16_t*)kv.v, c.bs, c.rs, c.B, c.S, c.H, c.Hkv,
                  c.rot, kv.capacity(), c.cache_seqlens ? c.table_rows : c.start_pos, (int)kv_store_blocks(c), c.cache_seqlens};
  if (kv.block_table) {
    a.pg = PageArgs{kv.block_table, kv.bt_rs, kv.rows, kv.outer};
    a.k_ps = kv.k_os, a.k_rs = kv.k_rs, a.v_ps = kv.v_os, a.v_rs = kv.v_rs;
  }
  if (c.cu_seqlens_q) a.vq = VarQArgs{c.cu_seqlens_q, c.total_q, c.max_seqlen_q, 0};
  if (c.q_gamma) {  // the *_qknorm entries: the NORM instantiation of the same form
    RopeStoreNormArgs an;
    static_cast<RopeStoreArgs&>(an) = a;
    an.nm = QkNormArgs{c.q_gamma, c.k_gamma, c.norm_eps};
    for_kv_store_form(c, [&](auto form) {
      for_dtype_dh<F16, BF16>(c.dtype, c.Dh, [&](auto dt, auto dh) {
        using DT = typename decltype(form)::template of<decltype(dt)>;
        hipLaunchKernelGGL((rope_kv_store_natural_kernel<DT, decltype(dh)::value, true>), dim3((unsigned)a.qv_blocks), dim3(256), 0, st, an);
      });
    });
    return 0;
  }
  for_kv_store_form(c, [&](auto form) {
    for_dtype_dh<F16, BF16>(c.dtype, c.Dh, [&](auto dt, auto dh) {
      using DT = typename decltype(form)::template of<decltype(dt)>;
      hipLaunchKernelGGL((rope_kv_store_natural_kernel<DT, decltype(dh)::value>), dim3((unsigned)a.qv_blocks), dim3(256), 0, st, a);
    });
  });
  return 0;
}

// ---- awq_kv_page_copy[_fp8]: the copy-on-write of a fork's partly filled tail page (PageTable.fork, awq_shared.hpp) ------------------
// One thread = one 16-byte chunk of one row of one (src, dst) pair, in K and in V; under FP8 the threads of chunks 0 .. Hkv - 1 move the
// row's K and V scales as well (a row of codes has Hkv * Dh / 16 >= Hkv chunks).  A pair whose ids are equal or not both inside the pool
// is skipped; rows and pages are addressed by their strides, so no byte between rows or pages is touched.
namespace {

struct PageCopyArgs {
  uint8_t* k;
  uint8_t* v;
  float* ks;
  float* vs;
  long long k_os, k_rs, v_os, v_rs;      // bytes
  long long ks_os, ks_rs, vs_os, vs_rs;  // floats
  const int* src;
  const int* dst;
  int n, page_size, num_pages, cpr, Hkv;  // cpr: 16-byte chunks per row
};

__global__ __launch_bounds__(256) void kv_page_copy_kernel(PageCopyArgs a) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)a.n * a.page_size * a.cpr) return;
  const int ch = (int)(id % a.cpr);
  const long long pr = id / a.cpr;
  const int row = (int)(pr % a.page_size);
  const long long pair = pr / a.page_size;
  const int s = as_const_i32(a.src)[pair], d = as_const_i32(a.dst)[pair];
  if (s < 0 || s >= a.num_pages || d < 0 || d >= a.num_pages || s == d) return;
  *reinterpret_cast<u32x4*>(a.k + d * a.k_os + row * a.k_rs + ch * 16) = *reinterpret_cast<const u32x4*>(a.k + s * a.k_os + row * a.k_rs + ch * 16);
  *reinterpret_cast<u32x4*>(a.v + d * a.v_os + row * a.v_rs + ch * 16) = *reinterpret_cast<const u32x4*>(a.v + s * a.v_os + row * a.v_rs + ch * 16);
  if (a.ks && ch < a.Hkv) {
    a.ks[d * a.ks_os + row * a.ks_rs + ch] = a.ks[s * a.ks_os + row * a.ks_rs + ch];
    a.vs[d * a.vs_os + row * a.vs_rs + ch] = a.vs[s * a.vs_os + row * a.vs_rs + ch];
  }
}

}  // namespace

int launch_kv_page_copy(const KvPageCopyCall& c, hipStream_t st) {
  const KvView& kv = c.kv;
  const int eb = kv.k_scale ? 1 : 2;  // bytes per element: codes or T
  PageCopyArgs a{(uint8_t*)kv.k, (uint8_t*)kv.v, (float*)kv.k_scale, (float*)kv.v_scale, kv.k_os * eb, kv.k_rs * eb, kv.v_os * eb, kv.v_rs * eb,
                 kv.ks_os, kv.ks_rs, kv.vs_os, kv.vs_rs, c.src_pages, c.dst_pages, c.n, kv.rows, kv.outer, c.Hkv * c.Dh * eb / 16, c.Hkv};
  const long long threads = (long long)c.n * kv.rows * a.cpr;
  hipLaunchKernelGGL(kv_page_copy_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
  return 0;
}

}  // namespace awq
