// Soft-capping (Gemma-2, Grok-1): a logit z becomes cap * tanh(z / cap).  On packed steps (awq_attn_varq_softcap[_kv8],
// awq_attn_paged_varq_softcap[_kv8]) the attention logits are
//
//   z_j = cap * tanh(softmax_scale * (q . k_j) / cap),   then the causal / window mask by selection, then softmax
//
// so a masked logit is -inf (never -cap) and a dead key's score, a NaN included, contributes nothing.  awq_logit_softcap caps logits that
// already exist.  Every kernel calls softcap_tanh below and nothing else: one error analysis covers them all.
//
// The kernels select the form by the element traits -- Softcap<Window<VarQMix<..>>> of the one-pass kernel, Softcap<Window<VarQ<..>>> of
// the split kernel -- so every other instantiation keeps its name, its argument block and its code.  There is no unwindowed softcap form:
// a global layer rides the windowed one with left = max_seqlen_k - 1, which hides no key.  The combine launch sees only (m, l, o)
// partials and is the windowed one.
#pragma once
#include "awq_window.hpp"

namespace awq {

template <typename DT>
struct Softcap : DT {};
template <typename DT>
using SoftcapWindowVarQDevLen = Softcap<Window<VarQ<DevLen<DT>>>>;
template <typename DT>
using SoftcapWindowVarQPagedDevLen = Softcap<Window<VarQ<Paged<DevLen<DT>>>>>;
template <typename DT>
using SoftcapWindowVarQMixDevLen = Softcap<Window<VarQMix<DevLen<DT>>>>;
template <typename DT>
using SoftcapWindowVarQMixPagedDevLen = Softcap<Window<VarQMix<Paged<DevLen<DT>>>>>;
template <typename DT>
struct IsSoftcap {
  static constexpr bool value = false;
};
template <typename DT>
struct IsSoftcap<Softcap<DT>> {
  static constexpr bool value = true;
};
template <typename DT>
struct IsWindow<Softcap<DT>> {
  static constexpr bool value = IsWindow<DT>::value;
};
template <typename DT>
struct IsVarQ<Softcap<DT>> {
  static constexpr bool value = IsVarQ<DT>::value;
};
template <typename DT>
struct IsVarQMix<Softcap<DT>> {
  static constexpr bool value = IsVarQMix<DT>::value;
};
template <typename DT>
struct IsPaged<Softcap<DT>> {
  static constexpr bool value = IsPaged<DT>::value;
};
template <typename DT>
struct IsDevLen<Softcap<DT>> {
  static constexpr bool value = IsDevLen<DT>::value;
};
template <typename DT>
struct IsKv8<Softcap<DT>> {
  static constexpr bool value = IsKv8<DT>::value;
};

// the launch arguments of a cap, formed by the host; a struct of its own behind the argument structs of the windowed kernels.  Base 2
// stays OUTSIDE the tanh: x = cap_log2e * softcap_tanh(s * scale_over_cap) stands where x = s * scale_log2e stands without a cap.
struct SoftcapArgs {
  float scale_over_cap;  // softmax_scale / cap
  float cap_log2e;       // cap * log2 e
};
inline SoftcapArgs softcap_args(float scale, float cap) { return SoftcapArgs{scale / cap, cap * 1.4426950408889634f}; }
// 0 is "no cap" (the entries route it to the uncapped kernels); anything else must be finite and positive
inline bool softcap_ok(float cap) { return cap >= 0.f && cap <= 3.4028234663852886e38f; }

// tanh(y) = 1 - 2 / (1 + e^(2y)) in fp32 from the hardware exp2 and rcp: one multiply, v_exp_f32, one add, v_rcp_f32, one fma.  Every
// step is an explicit builtin or a single IEEE operation whose operands are builtins' results, so there is nothing for -ffp-contract to
// fuse and the bits do not depend on the caller.
//
//   y -> +inf: e = +inf, d = +inf, r = 0, result  1.   y -> -inf: e = 0, d = 1, r = 1, result -1.   NaN stays NaN through every step.
//
// |softcap_tanh(y) - tanh(y)| <= 10 * 2^-24 for every finite y; the derivation stands in tests/attn_softcap_oracle.py and in DESIGN.md
// "Soft-capping".  Near 0 the error is absolute, not relative: a cap multiplies it by cap, which the oracles' bounds carry.
__device__ __forceinline__ float softcap_tanh(float y) {
  const float t = __builtin_fmaf(y, 2.8853900817779268f, 0.f);  // 2 log2 e * y, one rounding
  const float e = __builtin_amdgcn_exp2f(t);
  const float d = __builtin_fmaf(e, 1.f, 1.f);  // 1 + e, one rounding
  const float r = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(-2.f, r, 1.f);
}

// a logit that already exists: cap * tanh(z / cap) in fp32.  The division is IEEE's and the product is an fma with +0, which no later
// subtraction can be fused into: awq_logit_softcap, the LM head's epilogue and the log-prob tiles give the same bits on the same fp32 sum.
__device__ __forceinline__ float softcap_logit(float z, float cap) { return __builtin_fmaf(cap, softcap_tanh(__fdiv_rn(z, cap)), 0.f); }

}  // namespace awq
