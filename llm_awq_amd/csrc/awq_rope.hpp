// The rotation of fused_rope_with_pos (awq/kernels/csrc/rope_new/fused_rope_with_pos.cu:45-70) and the 8-element pack / unpack of the
// rope and store kernels (awq_attn_prefill_cdna4.hip, awq_attn_chunk_cdna4.hip, awq_attn_kv8_cdna4.hip).  The caches' bit-identity across
// the rope and store entries rests on all of them evaluating THIS expression: sincosf once per column, partner column c + rot / 2 negated
// for the first half and c - rot / 2 for the second, fmaf(x, cos, (+-x_rot) * sin) in fp32, rounded to T once.  Columns >= rot are the
// caller's to copy.  rope_with_pos_kernel uses RopeLane; the three store kernels (rope_kv_store_kernel, rope_kv_store_natural_kernel,
// rope_kv_store_natural_fp8_kernel) still spell the same steps out themselves -- on RopeLane their instantiations measured up to 6 %
// slower than before (profiles/kv_store_refactor_ab.json) -- and share only unpack8 / pack8.
//
// A lane owns 8 consecutive columns c0 .. c0 + 7 of one token, over every head of the row: 16-byte loads and stores.
#pragma once
#include "awq_device.hpp"

#include <math.h>

namespace awq {

// 8 consecutive T elements <-> fp32
template <typename DT>
__device__ __forceinline__ void unpack8(const u32x4& w, float (&f)[8]) {
  const u32 ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = DT::to_float((uint16_t)(ws[e] & 0xFFFFu));
    f[2 * e + 1] = DT::to_float((uint16_t)(ws[e] >> 16));
  }
}
template <typename DT>
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  u32 ws[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ws[e] = (u32)DT::from_float(f[2 * e]) | ((u32)DT::from_float(f[2 * e + 1]) << 16);
  return u32x4{ws[0], ws[1], ws[2], ws[3]};
}

struct RopeLane {
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sn[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int pc = 0;  // the partner chunk's first column
  float sign = 1.f;

  // a lane that does not rotate (c0 >= rot): nothing is loaded, rotate() is not for it
  __device__ __forceinline__ RopeLane() {}
  // fr: the angles of columns c0 .. c0 + 7 of the lane's token, 16-byte aligned; c0 < rot
  __device__ __forceinline__ RopeLane(const float* fr, int c0, int rot) {
    const f32x4 f0 = *reinterpret_cast<const f32x4*>(fr), f1 = *reinterpret_cast<const f32x4*>(fr + 4);
    const float ang[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
    for (int e = 0; e < 8; ++e) sincosf(ang[e], &sn[e], &cs[e]);
    const int half = rot >> 1;
    const bool first = c0 + half < rot;
    pc = first ? c0 + half : c0 - half;
    sign = first ? -1.f : 1.f;
  }

  // columns c0 .. c0 + 7 of one head row after the rotation, as T bits
  template <typename DT>
  __device__ __forceinline__ u32x4 rotate(const uint16_t* head_row, int c0) const {
    float x[8], y[8], res[8];
    unpack8<DT>(*reinterpret_cast<const u32x4*>(head_row + c0), x);
    unpack8<DT>(*reinterpret_cast<const u32x4*>(head_row + pc), y);
#pragma unroll
    for (int e = 0; e < 8; ++e) res[e] = __builtin_fmaf(x[e], cs[e], (sign * y[e]) * sn[e]);
    return pack8<DT>(res);
  }
};

// ---- per-head q/k RMSNorm in front of the rotation (Qwen3, Gemma-3): the NORM instantiations of the two natural-layout store kernels ----
// A head row of Dh columns lies in the Dh / 8 consecutive lanes of its token, so the row's sum of squares is a butterfly over those lanes,
// as the FP8 kernel's max |x| is.  The arithmetic is rmsnorm_kernel's (awq_util.hip) on that head as a row of K = Dh, bit for bit: each lane
// folds its 8 columns in ascending order with fmaf from 0, the lanes combine with ss += __shfl_xor(ss, d) for d = 1, 2, .., Dh / 16 (that
// kernel's butterfly goes on over lanes that hold 0, which changes nothing; a + b = b + a, so every lane of the head ends with the same
// bits), rstd = rsqrtf(ss / Dh + eps), y = T((x * rstd) * gamma) with one rounding.  The rotation then acts on y as it acts on x without
// the norm.  gamma is fp32: Gemma-3's 1 + w is formed in fp32 and no T holds it.
struct QkNormArgs {
  const float* q_gamma;  // fp32 [Dh], 16-byte aligned
  const float* k_gamma;
  float eps;
};

// gamma of the lane's own columns c0 .. c0 + 7 and of its rotation partner's pc .. pc + 7 (pc = c0 for a lane that does not rotate)
struct QkNormLane {
  float g[8], gp[8];
  __device__ __forceinline__ QkNormLane(const float* gamma, int c0, int pc) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(gamma + c0), a1 = *reinterpret_cast<const f32x4*>(gamma + c0 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(gamma + pc), b1 = *reinterpret_cast<const f32x4*>(gamma + pc + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = a0[e], g[4 + e] = a1[e], gp[e] = b0[e], gp[4 + e] = b1[e];
  }
};

// T((x * rstd) * gamma) with one rounding, the product held in a register before it is rounded.  Left to itself the compiler folds the
// second multiply and the rounding to F16 into v_fma_mixlo_f16 (a * b + 0) for some of the columns, and a product of -0 comes out as +0
// (seen on the all-zero head under a negative gamma); rmsnorm_kernel's v_mul_f32 / v_cvt_pk_f16_f32 keeps the sign, and so does this.
template <typename DT>
__device__ __forceinline__ uint16_t qk_norm_round(float x, float rstd, float gamma) {
  float p = (x * rstd) * gamma;
  asm("" : "+v"(p));
  return DT::from_float(p);
}

// Columns c0 .. c0 + 7 of n consecutive head rows (heads, heads + DH, ..) after norm and rotation, as T bits: store(hd, bits) for hd = 0 ..
// n - 1 in order.  EVERY lane of the token calls this together (the butterflies meet all DH / 8 of them; n is the call's, so the trip counts
// agree); the lanes part only in what they keep: a lane with rot_lane the rotation against the partner chunk, which it loads and normalises
// itself (the partner lane's bits: same x, same rstd, same gamma), the others the normalised chunk (their pc is c0 and cs / sn are zeros;
// what they rotate is discarded).
//
// Eight heads at a time.  One head at a time, the launch of a single token is one lane's serial chain of H + Hkv x (load, DH / 16 cross-lane
// steps, rsqrt, multiply, store) and measured twice the plain store; the loads, butterflies and rsqrts of eight heads are independent
// chains that overlap (about 180 VGPRs, no scratch; four at a time measured between the two: profiles/qknorm_store_bench.json holds the
// eight).  A tail group repeats the last head and keeps only what it has not stored.  Per head the arithmetic is the one stated above,
// whatever the grouping.
template <typename DT, int DH, typename Store>
__device__ __forceinline__ void qk_norm_rotate_heads(const uint16_t* heads, int n, int c0, int pc, bool rot_lane, const float (&cs)[8],
                                                     const float (&sn)[8], float sign, const QkNormLane& gm, float eps, Store&& store) {
  constexpr int G = 8;
  for (int h0 = 0; h0 < n; h0 += G) {
    float x[G][8], y[G][8], ss[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const uint16_t* hp = heads + (long long)min(h0 + j, n - 1) * DH;
      unpack8<DT>(*reinterpret_cast<const u32x4*>(hp + c0), x[j]);
      unpack8<DT>(*reinterpret_cast<const u32x4*>(hp + pc), y[j]);
      ss[j] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) ss[j] = __builtin_fmaf(x[j][e], x[j][e], ss[j]);
    }
#pragma unroll
    for (int d = 1; d < DH / 8; d <<= 1) {
#pragma unroll
      for (int j = 0; j < G; ++j) ss[j] += __shfl_xor(ss[j], d, 64);
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float rstd = rsqrtf(ss[j] / (float)DH + eps);
      uint16_t xb[8];
      float res[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xb[e] = qk_norm_round<DT>(x[j][e], rstd, gm.g[e]);
        const float yn = DT::to_float(qk_norm_round<DT>(y[j][e], rstd, gm.gp[e]));
        res[e] = __builtin_fmaf(DT::to_float(xb[e]), cs[e], (sign * yn) * sn[e]);
        asm("" : "+v"(res[e]));  // (the plain kernels' v_fma_f32 / v_cvt pair, not a mixed-precision fma fed with the F16 bits of xb)
      }
      const u32x4 rotated = pack8<DT>(res);
      const u32x4 normed = u32x4{(u32)xb[0] | ((u32)xb[1] << 16), (u32)xb[2] | ((u32)xb[3] << 16), (u32)xb[4] | ((u32)xb[5] << 16),
                                 (u32)xb[6] | ((u32)xb[7] << 16)};
      if (h0 + j < n) store(h0 + j, rot_lane ? rotated : normed);
    }
  }
}

}  // namespace awq
