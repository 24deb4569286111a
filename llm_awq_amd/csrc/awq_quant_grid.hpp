// The asymmetric per-group grid of the reference's pseudo_quantize_tensor(zero_point=True) (awq/quantize/quantizer.py:61-103), evaluated the way
// torch evaluates it on fp16 / bf16 tensors: every operation in fp32 on T values, rounded to T (nearest-even) before the next one.  Host and
// device compile the same text: awq_quantize_group_host runs it on the CPU, where the non-GPU tests hold it to the torch composition
// (DESIGN.md "AWQ quantisation").
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWQ_QG_FN __host__ __device__ __forceinline__
#else
#define AWQ_QG_FN inline
#endif

namespace awq {
namespace qgrid {

AWQ_QG_FN uint32_t f2u(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
AWQ_QG_FN float u2f(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// T = fp16 (BF = false) or bf16 (BF = true); values travel as fp32 that are exactly representable in T
template <bool BF>
struct T16 {
  // nearest-even rounding of an fp32 value to T, returned as fp32 (finite or infinite input; subnormals of T are kept)
  static AWQ_QG_FN float round(float x) {
    if (BF) {
      uint32_t u = f2u(x);
      u += 0x7fffu + ((u >> 16) & 1u);
      return u2f(u & 0xffff0000u);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // opaque to the optimiser, which would otherwise narrow round(a / b) to an fp16 division: the quotient is taken in fp32 (IEEE) and
    // rounded here (the wave's fp16 mode: nearest-even, subnormals kept)
    _Float16 h;
    asm("v_cvt_f16_f32 %0, %1" : "=v"(h) : "v"(x));
    return (float)h;
#else
    return (float)(_Float16)x;
#endif
  }
  static AWQ_QG_FN float from_bits(uint16_t b) {
    if (BF) return u2f((uint32_t)b << 16);
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
  }
  static AWQ_QG_FN uint16_t to_bits(float x) {  // x is exactly representable in T
    if (BF) return (uint16_t)(f2u(x) >> 16);
    _Float16 h = (_Float16)x;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
  }
};

// torch's clamp with scalar bounds: a value equal to a bound is kept as it is, so clamp(-0.0, 0, qmax) stays -0.0
AWQ_QG_FN float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scale and zero point of a group whose extremes are lo <= hi (T values): scales = (hi - lo).clamp(min=1e-5) / qmax,
// zeros = (-round(lo / scales)).clamp_(0, qmax)
template <bool BF>
struct Grid {
  float scale, zero, qmax;
  AWQ_QG_FN Grid(float lo, float hi, int n_bit) {
#pragma clang fp contract(off)
    using R = T16<BF>;
    qmax = (float)((1 << n_bit) - 1);
    float rng = R::round(hi - lo);
    rng = fmaxf(rng, R::round(1e-5f));  // the clamp's scalar is cast to T first
    scale = R::round(rng / qmax);
    const float zr = -rintf(R::round(lo / scale));
    zero = clampf(zr, 0.0f, qmax);
  }
  // (clamp(round(v / scales) + zeros, 0, qmax) - zeros) * scales
  AWQ_QG_FN float fake(float v) const {
#pragma clang fp contract(off)
    using R = T16<BF>;
    float q = rintf(R::round(v / scale));
    q = R::round(q + zero);
    q = clampf(q, 0.0f, qmax) - zero;  // small integers: exact
    return R::round(q * scale);
  }
  // WQLinear.from_linear's integer recovery (qmodule.py:176-184): round((fake + zeros * scales) / scales) in T, not clamped
  AWQ_QG_FN int recover(float fk) const {
#pragma clang fp contract(off)
    using R = T16<BF>;
    const float sz = R::round(zero * scale);
    const float t = R::round(fk + sz);
    return (int)rintf(R::round(t / scale));
  }
  // from_linear's scaled_zeros: -(T(scale) * float(int(zero))) rounded to T
  AWQ_QG_FN float scaled_zero() const {
#pragma clang fp contract(off)
    return -T16<BF>::round(scale * (float)(int)zero);  // (the integer conversion drops the sign of a zero that is -0.0)
  }
};

}  // namespace qgrid
}  // namespace awq
