// FP8 KV cache, natural layout: codes [Bc, L, Hkv, Dh] of OCP e4m3fn (one byte per element) with one fp32 scale per (token, KV head),
// scales [Bc, L, Hkv].  The format is fixed in DESIGN.md ("FP8 KV cache"); ops.kv8_quant / ops.kv8_dequant state it in torch.
//
//   quantise a head row x[0..Dh) of T:   s = max(max|x|, 2^-60) / 448 (IEEE division);  code = e4m3fn_RNE(clamp(x / s, -448, 448))
//   dequantise:                          T(float(code) * s): one fp32 multiply, one RNE rounding to T
//
// The attention kernels dequantise in their staging step (global -> registers -> LDS), so that everything behind the LDS write is the
// kernel of the T cache and the result is, bit for bit, that kernel's on the dequantised tensors.  They select the form by the element
// traits -- Kv8<F16> / Kv8<BF16>, the same traits under another name, as FtCache<DT> is -- so the T-cache kernels keep their names
// and their code.
#pragma once
#include "awq_device.hpp"

namespace awq {

template <typename DT>
struct Kv8 : DT {};
template <typename DT>
struct IsKv8 {
  static constexpr bool value = false;
};
template <typename DT>
struct IsKv8<Kv8<DT>> {
  static constexpr bool value = true;
};

typedef float kv8_f32x2 __attribute__((ext_vector_type(2)));

// eight codes (bytes 0..3 of c.x, then of c.y) times s -> eight T values, one 16-byte chunk (v_cvt_pk_f32_fp8: OCP e4m3fn on gfx950)
template <typename DT>
__device__ __forceinline__ u32x4 kv8_dequant8(const u32x2& c, float s) {
  u32 w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const u32 src = e < 2 ? c.x : c.y;
    const kv8_f32x2 f = (e & 1) ? __builtin_amdgcn_cvt_pk_f32_fp8((int)src, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)src, false);
    w[e] = (u32)DT::from_float(f[0] * s) | ((u32)DT::from_float(f[1] * s) << 16);
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// eight fp32 values (exact images of T values) -> eight codes at scale s (v_cvt_pk_fp8_f32 rounds to nearest even; the clamp keeps
// every operand inside the finite range, so the convert's overflow behaviour is never asked)
__device__ __forceinline__ u32x2 kv8_quant8(const float (&x)[8], float s) {
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = fminf(fmaxf(x[e] / s, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
  return u32x2{(u32)lo, (u32)hi};
}

// the scale of a row whose largest magnitude is amax (no special case for a zero row, no fp32 denormal)
__device__ __forceinline__ float kv8_scale(float amax) { return fmaxf(amax, 0x1p-60f) / 448.f; }

}  // namespace awq
