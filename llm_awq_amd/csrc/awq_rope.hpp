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

}  // namespace awq
