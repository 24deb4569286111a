// extern "C" entry points declared in include/awq_cdna4.h: argument validation + dispatch.
// No torch types; errors are returned as codes (the Python/pybind layer turns them into
// RuntimeError with the reference's messages).
#include "../../include/awq_cdna4.h"

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "awq_kernels.hpp"
#include "awq_kvcache.hpp"

namespace {
thread_local char g_last_hip_error[256] = "";

int finish_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    strncpy(g_last_hip_error, hipGetErrorString(e), sizeof(g_last_hip_error) - 1);
    return AWQ_ERR_LAUNCH;
  }
  return AWQ_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_common(const void* x, const void* qweight, const void* scales, const void* zeros, const void* out, int m, int n,
                 int k, int group_size, int dtype) {
  if (!x || !qweight || !scales || !zeros || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (m < 1 || n < 8 || k < 128 || (n % 8) != 0 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight) || !aligned16(out) || (reinterpret_cast<uintptr_t>(scales) & 1u) ||
      (reinterpret_cast<uintptr_t>(zeros) & 1u))
    return AWQ_ERR_ALIGN;
  return AWQ_OK;
}

// Steps 2 - 5 of a dense W4 cdna4 entry, behind its own argument checks: the route (awq_linear_route.hpp), the ONE launcher of its leaf, the separate bias
// launch where the route says so.  No fall-through: a launcher cannot refuse a call its own predicate routed to it (tests/linear_route_check.cpp).
int launch_routed(int entry, const void* x, const void* qw, const void* scales, const void* zeros, const void* szp, const void* szh, const void* bias, void* out, int m,
                  int n, int k, int dtype, void* ws, size_t ws_bytes, int flags, hipStream_t st) {
  using namespace awq;
  const LinearRoute r = linear_route(entry, m, n, k, flags, device_cu_count(), g_linear);
  if (r.bias_align16 && bias && !aligned16(bias)) return AWQ_ERR_ALIGN;
  const void *sz = r.szfmt ? szh : szp, *b = r.bias == kBiasFused ? bias : nullptr;
  const int pair = r.epilogue == kEpiPair ? 2 : 0, f32 = r.epilogue == kEpiPartial ? 1 : 0;
  if (!r.ws) ws = nullptr, ws_bytes = 0;
  int rc = -1;
  switch (r.leaf) {
    case kLeafDecode: rc = launch_gemv_dma(x, qw, sz, b, out, m, n, k, pair, dtype, r.szfmt, st, f32); break;
    case kLeafGemvRing: rc = launch_gemv_cdna4(x, qw, szp, b, out, m, n, k, 0, 4, dtype, st); break;
    case kLeafMidm: rc = launch_midm_cdna4(x, qw, sz, b, out, m, n, k, pair, dtype, r.szfmt, 4, f32, ws, ws_bytes, st); break;
    case kLeafSkinny16: rc = launch_skinny_decode(x, qw, sz, b, out, m, n, k, pair, dtype, r.szfmt, st, f32); break;
    case kLeafSkinny: rc = launch_skinny_cdna4(x, qw, szp, b, out, m, n, k, dtype, st, f32, ws, ws_bytes); break;
    case kLeafSkinnyGateUp: rc = launch_skinny_gate_up(x, qw, szp, out, m, n, k, dtype, st); break;
    case kLeafTiles: rc = launch_gemm_cdna4_v3(x, qw, szp, b, out, m, n, k, 0, dtype, ws, ws_bytes, st, 4, pair ? 2 : (f32 ? 3 : 0), r.szfmt ? szh : nullptr); break;
    case kLeafGeneric:
      rc = entry == kEntryGemv ? launch_gemv(x, qw, scales, zeros, szp, out, m, n, k, dtype, 1, st) : launch_gemm(x, qw, scales, zeros, szp, out, m, n, k, dtype, 1, ws, ws_bytes, st);
      break;
  }
  if (rc != 0) return AWQ_ERR_SHAPE;
  if (r.bias == kBiasAdd) launch_bias_add(out, bias, m, n, dtype, st);
  return finish_launch();
}
inline int route_flags(const void* szp, const void* szh, const void* bias, const void* ws) {
  return (szp ? awq::kHasSzPacked : 0) | (szh ? awq::kHasSzHalf : 0) | (bias ? awq::kHasBias : 0) | (ws ? awq::kHasWs : 0);
}
}  // namespace

namespace awq {
LinearKnobs g_linear;
}

extern "C" {

int awq_abi_version(void) { return AWQ_ABI_VERSION; }

const char* awq_last_hip_error(void) { return g_last_hip_error; }

const char* awq_status_string(int status) {
  switch (status) {
    case AWQ_OK: return "ok";
    case AWQ_ERR_BATCH: return "Unsupported batch size for gemv kernel.";
    case AWQ_ERR_GROUP: return "Unsupported group size for gemv kernel.";
    case AWQ_ERR_DTYPE: return "Unsupported dtype: expected float16 or bfloat16.";
    case AWQ_ERR_SHAPE: return "Unsupported shape: need n % 8 == 0, k % 128 == 0, m >= 1.";
    case AWQ_ERR_ALIGN: return "Pointer is not 16-byte aligned (tensors must be contiguous).";
    case AWQ_ERR_NULL: return "NULL pointer argument.";
    case AWQ_ERR_WORKSPACE: return "Workspace too small.";
    case AWQ_ERR_LAUNCH: return "HIP launch failed.";
    case AWQ_ERR_BITS: return "Only 4-bit (and the repo's 3-bit extension) are supported.";
    default: return "unknown status";
  }
}

int awq_w4a16_gemv(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, void* out, int m,
                   int n, int k, int group_size, int dtype, void* stream) {
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (m < 1 || m > 16) return AWQ_ERR_BATCH;
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  awq::launch_gemv(x, qweight, scales, scaled_zeros, nullptr, out, m, n, k, dtype, 0, (hipStream_t)stream);
  return finish_launch();
}

size_t awq_w4a16_gemm_workspace_bytes(int m, int n, int k) { return awq::gemm_workspace_bytes(m, n, k); }

int awq_w4a16_gemm(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, void* out, int m,
                   int n, int k, int group_size, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  const size_t need = awq::gemm_workspace_bytes(m, n, k);
  if (need > 0 && (!workspace || workspace_bytes < need)) return AWQ_ERR_WORKSPACE;
  awq::launch_gemm(x, qweight, scales, scaled_zeros, nullptr, out, m, n, k, dtype, 0, workspace, workspace_bytes, (hipStream_t)stream);
  return finish_launch();
}

int awq_w4a16_forward(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, const void* bias,
                      void* out, int m, int n, int k, int group_size, int dtype, void* workspace, size_t workspace_bytes,
                      void* stream) {
  int st;
  if (m < 8 && bias && group_size == 128 &&
      check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype) == AWQ_OK && awq::gemv_v2fast_enabled() &&
      awq::launch_gemv_v2fast(x, qweight, scales, scaled_zeros, bias, out, m, n, k, k / 128, dtype, (hipStream_t)stream) == 0)
    return finish_launch();  // bias fused into the decode kernel's epilogue
  if (m > 8 && m <= 255 && bias && group_size == 128 && awq::g_linear.gemm_variant == 0 &&
      check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype) == AWQ_OK &&
      awq::launch_skinny_v2(x, qweight, scales, scaled_zeros, bias, out, m, n, k, k / 128, dtype, (hipStream_t)stream) == 0)
    return finish_launch();  // bias fused into the skinny kernel's epilogue
  if (m < 8)
    st = awq_w4a16_gemv(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype, stream);
  else
    st = awq_w4a16_gemm(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype, workspace, workspace_bytes,
                        stream);
  if (st != AWQ_OK || !bias) return st;
  awq::launch_bias_add(out, bias, m, n, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_unpack_v2(const void* qweight, void* out_u8, int n, int k, void* stream) {
  if (!qweight || !out_u8) return AWQ_ERR_NULL;
  if (n < 4 || (n % 4) != 0 || k < 64 || (k % 64) != 0) return AWQ_ERR_SHAPE;
  awq::launch_unpack_v2(qweight, out_u8, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_dequant_v2(const void* qweight, const void* scales, const void* scaled_zeros, void* out, int n, int k,
                   int group_size, int dtype, void* stream) {
  if (!qweight || !scales || !scaled_zeros || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (n < 4 || (n % 4) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_dequant_v2(qweight, scales, scaled_zeros, out, n, k, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_pack_v2(const void* q_u8, void* qweight, int n, int k, void* stream) {
  if (!q_u8 || !qweight) return AWQ_ERR_NULL;
  if (n < 4 || (n % 4) != 0 || k < 64 || (k % 64) != 0) return AWQ_ERR_SHAPE;
  awq::launch_pack_v2(q_u8, qweight, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_repack_v1_to_v2(const void* qweight_v1, const void* scales_v1, const void* qzeros_v1, void* qweight_v2,
                        void* scales_v2, void* scaled_zeros_v2, int n, int k, int gpad, int dtype, void* stream) {
  if (!qweight_v1 || !scales_v1 || !qzeros_v1 || !qweight_v2 || !scales_v2 || !scaled_zeros_v2) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (n < 4 || (n % 4) != 0 || k < 64 || (k % 64) != 0 || gpad < 8 || (gpad % 8) != 0) return AWQ_ERR_SHAPE;
  awq::launch_repack_v1_to_v2(qweight_v1, scales_v1, qzeros_v1, qweight_v2, scales_v2, scaled_zeros_v2, n, k, gpad, dtype,
                              (hipStream_t)stream);
  return finish_launch();
}

// ---- cdna4 interleave (bf16) ----
int awq_repack_v2_to_cdna4(const void* qweight_v2, void* qweight_cdna4, int n, int k, void* stream) {
  if (!qweight_v2 || !qweight_cdna4) return AWQ_ERR_NULL;
  if (qweight_v2 == qweight_cdna4) return AWQ_ERR_ALIGN;  // not an in-place permutation
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_repack_v2_cdna4(qweight_v2, qweight_cdna4, n, k, 1, (hipStream_t)stream);
  return finish_launch();
}

int awq_repack_cdna4_to_v2(const void* qweight_cdna4, void* qweight_v2, int n, int k, void* stream) {
  if (!qweight_v2 || !qweight_cdna4) return AWQ_ERR_NULL;
  if (qweight_v2 == qweight_cdna4) return AWQ_ERR_ALIGN;
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_repack_v2_cdna4(qweight_cdna4, qweight_v2, n, k, 0, (hipStream_t)stream);
  return finish_launch();
}

int awq_unpack_cdna4(const void* qweight, void* out_u8, int n, int k, void* stream) {
  if (!qweight || !out_u8) return AWQ_ERR_NULL;
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_unpack_cdna4(qweight, out_u8, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_dequant_cdna4(const void* qweight, const void* scales, const void* scaled_zeros, void* out, int n, int k,
                      int group_size, int dtype, void* stream) {
  if (!qweight || !scales || !scaled_zeros || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_dequant_cdna4(qweight, scales, scaled_zeros, out, n, k, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_pack_sz_cdna4(const void* scales, const void* scaled_zeros, void* sz_packed, int n, int k, void* stream) {
  if (!scales || !scaled_zeros || !sz_packed) return AWQ_ERR_NULL;
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_pack_sz_cdna4(scales, scaled_zeros, sz_packed, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_pack_szh_cdna4(const void* scales, const void* scaled_zeros, void* sz_half, int* inexact_dev, int n, int k, int dtype,
                       void* stream) {
  if (!scales || !scaled_zeros || !sz_half || !inexact_dev) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  awq::launch_pack_szh_cdna4(scales, scaled_zeros, sz_half, inexact_dev, n, k, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_w4a16_decode_cdna4(const void* x, const void* qweight, const void* sz_half, const void* bias, void* out, int m, int n, int k,
                           int group_size, int dtype, int epilogue, void* stream) {
  if (!x || !qweight || !sz_half || !out) return AWQ_ERR_NULL;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1 || m > 8) return AWQ_ERR_BATCH;
  if (epilogue < 0 || epilogue > 2 || (epilogue != 0 && bias)) return AWQ_ERR_SHAPE;
  const int mult = epilogue == 1 ? 32 : 16;
  if (n < mult || (n % mult) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight) || !aligned16(out) || !aligned16(sz_half)) return AWQ_ERR_ALIGN;
  if (awq::launch_gemv_dma(x, qweight, sz_half, bias, out, m, n, k, epilogue, dtype, 1, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_w4a16_gemv_cdna4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                         const void* sz_packed, void* out, int m, int n, int k, int group_size, int dtype, void* stream) {
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (m < 1 || m > 16) return AWQ_ERR_BATCH;
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if ((n % 16) != 0) return AWQ_ERR_SHAPE;
  return launch_routed(awq::kEntryGemv, x, qweight, scales, scaled_zeros, sz_packed, nullptr, nullptr, out, m, n, k, dtype, nullptr, 0, route_flags(sz_packed, nullptr, nullptr, nullptr),
                       (hipStream_t)stream);
}

int awq_w4a16_mlp_gate_up_cdna4(const void* x, const void* qweight_gate_up, const void* sz_packed, void* out, int m,
                                int n2, int k, int group_size, int dtype, void* stream) {
  if (!x || !qweight_gate_up || !sz_packed || !out) return AWQ_ERR_NULL;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1 || m > 8) return AWQ_ERR_BATCH;
  if (n2 < 32 || (n2 % 32) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight_gate_up) || !aligned16(out) || !aligned16(sz_packed)) return AWQ_ERR_ALIGN;
  if (awq::launch_gemv_cdna4(x, qweight_gate_up, sz_packed, nullptr, out, m, n2, k, 1, 4, dtype, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_w4a16_mlp_gate_up_forward_cdna4(const void* x, const void* qweight_interleaved, const void* sz_packed, const void* sz_half,
                                        void* out, int m, int n2, int k, int group_size, int dtype, void* stream) {
  return awq_w4a16_mlp_gate_up_forward_cdna4_ws(x, qweight_interleaved, sz_packed, sz_half, out, m, n2, k, group_size, dtype, nullptr, 0, stream);
}

size_t awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes(int m, int n2, int k) {
  if (m <= 8) return 0;
  const size_t a = awq::gemm_cdna4_v3_workspace_bytes(m, n2, k), b = awq::midm_workspace_bytes(m, n2, k);
  return a > b ? a : b;
}

int awq_w4a16_mlp_gate_up_forward_cdna4_ws(const void* x, const void* qweight_interleaved, const void* sz_packed, const void* sz_half,
                                           void* out, int m, int n2, int k, int group_size, int dtype, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  if (!x || !qweight_interleaved || !sz_packed || !out) return AWQ_ERR_NULL;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1) return AWQ_ERR_BATCH;
  if (n2 < 16 || (n2 % 16) != 0 || k < 128 || (k % 128) != 0 || (size_t)m * (size_t)k >= (1ull << 31)) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight_interleaved) || !aligned16(out) || !aligned16(sz_packed) || (sz_half && !aligned16(sz_half)))
    return AWQ_ERR_ALIGN;
  // (a workspace that is misaligned or below the tile kernels' size is dropped by their row only: the mid-M row before it is offered the workspace as it came)
  const bool ws_tiles = workspace && m > 8 && (reinterpret_cast<uintptr_t>(workspace) & 63) == 0 && workspace_bytes >= awq::gemm_cdna4_v3_workspace_bytes(m, n2, k);
  return launch_routed(awq::kEntryGateUp, x, qweight_interleaved, nullptr, nullptr, sz_packed, sz_half, nullptr, out, m, n2, k, dtype, workspace, workspace_bytes,
                       route_flags(sz_packed, sz_half, nullptr, workspace) | (ws_tiles ? awq::kWsTiles : 0), (hipStream_t)stream);
}

int awq_w4a16_rmsnorm_forward_cdna4(const void* x, const void* gamma, float eps, const void* qweight, const void* sz_packed,
                                    const void* bias, void* out, int m, int n, int k, int group_size, int dtype,
                                    int fused_gate_up, void* stream) {
  if (!x || !gamma || !qweight || !sz_packed || !out) return AWQ_ERR_NULL;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1 || m > 4) return AWQ_ERR_BATCH;
  const int mult = fused_gate_up ? 32 : 16;
  if (n < mult || (n % mult) != 0 || k < 128 || (k % 128) != 0 || (fused_gate_up && bias)) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(qweight) || !aligned16(out) || !aligned16(sz_packed)) return AWQ_ERR_ALIGN;
  if (awq::launch_gemv_cdna4_norm(x, gamma, eps, qweight, sz_packed, bias, out, m, n, k, fused_gate_up ? 1 : 0, dtype,
                                  (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_rmsnorm(const void* x, const void* gamma, float eps, void* out, int m, int k, int dtype, void* stream) {
  if (!x || !gamma || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1) return AWQ_ERR_BATCH;
  if (k < 8 || (k % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(out)) return AWQ_ERR_ALIGN;
  if (awq::launch_rmsnorm(x, gamma, eps, out, m, k, dtype, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_attn_decode_plan(int batch, int nheads_kv, int head_dim, int timestep, int lmax, int* splits, int* chunk) {
  if (!splits || !chunk) return AWQ_ERR_NULL;
  if (batch < 1 || nheads_kv < 1 || head_dim < 32 || head_dim > 256 || (head_dim % 16) != 0 || timestep < 0 || lmax < 1) return AWQ_ERR_SHAPE;
  return awq::attn_decode_plan(batch, nheads_kv, head_dim, timestep, lmax, splits, chunk);
}

size_t awq_attn_decode_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int timestep, int lmax) {
  if (batch < 1 || nheads_kv < 1 || nheads < nheads_kv || head_dim < 32 || head_dim > 256 || (head_dim % 16) != 0 || timestep < 0 || lmax < 1)
    return 0;
  return awq::attn_decode_workspace_bytes(batch, nheads, nheads_kv, head_dim, timestep, lmax);
}

int awq_attn_decode(const void* q, const void* k, const void* v, void* k_cache, void* v_cache, const int* length_per_sample,
                    const float* alibi_slopes, void* out, int batch, int cache_batch, int nheads, int nheads_kv, int head_dim, int lmax,
                    long long q_batch_stride, long long k_batch_stride, long long v_batch_stride, int timestep, int rotary_dim,
                    float rotary_base, float rotary_scale, int neox, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !k || !v || !k_cache || !v_cache || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (batch < 1 || cache_batch < batch || nheads < 1 || nheads_kv < 1 || (nheads % nheads_kv) != 0 || head_dim < 32 || head_dim > 256 ||
      (head_dim % 16) != 0 || lmax < 1 || timestep < 0 || rotary_dim < 0 || rotary_dim > head_dim || (rotary_dim % 2) != 0 ||
      q_batch_stride < 0 || k_batch_stride < 0 || v_batch_stride < 0)
    return AWQ_ERR_SHAPE;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) ||
      (q_batch_stride % 8) != 0 || (k_batch_stride % 8) != 0 || (v_batch_stride % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(length_per_sample) & 3u) || (reinterpret_cast<uintptr_t>(alibi_slopes) & 3u))
    return AWQ_ERR_ALIGN;
  const size_t need = awq::attn_decode_workspace_bytes(batch, nheads, nheads_kv, head_dim, timestep, lmax);
  if (need > 0 && (!workspace || workspace_bytes < need)) return AWQ_ERR_WORKSPACE;
  if (need > 0 && !aligned16(workspace)) return AWQ_ERR_ALIGN;
  awq::launch_attn_decode(q, k, v, k_cache, v_cache, length_per_sample, alibi_slopes, out, batch, nheads, nheads_kv, head_dim, lmax,
                          q_batch_stride, k_batch_stride, v_batch_stride, timestep, rotary_dim, rotary_base, rotary_scale, neox, dtype,
                          workspace, (hipStream_t)stream);
  return finish_launch();
}

static bool prefill_shape_ok(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal) {
  return batch >= 1 && nheads >= 1 && nheads_kv >= 1 && (nheads % nheads_kv) == 0 &&
         (head_dim == 64 || head_dim == 128 || (head_dim == 72 && !causal)) && seqlen_q >= 1 && seqlen_k >= 1 &&
         !(causal && seqlen_q > seqlen_k) && (long long)batch * nheads * (head_dim == 72 ? (seqlen_q + 31) / 32 : (seqlen_q + 63) / 64) <= 0x7FFFFFFFll;
}

int awq_attn_prefill_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* q_tile_rows,
                          int* blocks) {
  if (!q_tile_rows || !blocks) return AWQ_ERR_NULL;
  if (!prefill_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal)) return AWQ_ERR_SHAPE;
  if (head_dim == 72) return awq::attn_varlen_plan(batch, nheads, head_dim, seqlen_q, q_tile_rows, blocks);  // the tower kernel's dense form
  return awq::attn_prefill_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal, q_tile_rows, blocks);
}

int awq_attn_prefill(const void* q, const void* k, const void* v, void* out, int batch, int seqlen_q, int seqlen_k, int nheads, int nheads_kv,
                     int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                     long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  if (!q || !k || !v || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (!prefill_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal) || q_batch_stride < 0 || k_batch_stride < 0 ||
      v_batch_stride < 0 || q_row_stride < (long long)nheads * head_dim || k_row_stride < (long long)nheads_kv * head_dim ||
      v_row_stride < (long long)nheads_kv * head_dim)
    return AWQ_ERR_SHAPE;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || (q_batch_stride % 8) != 0 || (k_batch_stride % 8) != 0 ||
      (v_batch_stride % 8) != 0 || (q_row_stride % 8) != 0 || (k_row_stride % 8) != 0 || (v_row_stride % 8) != 0)
    return AWQ_ERR_ALIGN;
  if (head_dim == 72)  // non-causal only (prefill_shape_ok): the tower kernel's dense form
    awq::launch_attn_tower(q, k, v, out, nullptr, batch, seqlen_q, seqlen_k, (long long)batch * seqlen_q, nheads, nheads_kv, head_dim,
                           q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, softmax_scale, dtype,
                           (hipStream_t)stream);
  else
    awq::launch_attn_prefill(q, k, v, out, batch, seqlen_q, seqlen_k, nheads, nheads_kv, head_dim, q_batch_stride, q_row_stride, k_batch_stride,
                             k_row_stride, v_batch_stride, v_row_stride, softmax_scale, causal, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_attn_prefill_ftcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int cache_batch, int seqlen_q,
                             int kv_start, int seqlen_k, int nheads, int nheads_kv, int head_dim, int lmax, long long q_batch_stride,
                             long long q_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  if (!q || !k_cache || !v_cache || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if ((head_dim != 64 && head_dim != 128) || !prefill_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal) ||
      cache_batch < batch || lmax < 1 || kv_start < 0 || (long long)kv_start + seqlen_k > lmax || q_batch_stride < 0 ||
      q_row_stride < (long long)nheads * head_dim)
    return AWQ_ERR_SHAPE;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) || (q_batch_stride % 8) != 0 || (q_row_stride % 8) != 0)
    return AWQ_ERR_ALIGN;
  awq::launch_attn_prefill_ftcache(q, k_cache, v_cache, out, batch, seqlen_q, kv_start, seqlen_k, nheads, nheads_kv, head_dim, lmax,
                                   q_batch_stride, q_row_stride, softmax_scale, causal, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_rope_kv_store(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int batch, int cache_batch, int seqlen,
                      int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos, long long qkv_batch_stride,
                      long long qkv_row_stride, int dtype, void* stream) {
  if (!qkv || !freqs || !q_out || !k_cache || !v_cache) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (batch < 1 || cache_batch < batch || seqlen < 1 || nheads < 1 || nheads_kv < 1 || (head_dim != 64 && head_dim != 128) ||
      (head_dim % 8) != 0 || rot_dim < 16 || (rot_dim % 16) != 0 || rot_dim > head_dim || lmax < 1 || start_pos < 0 ||
      (long long)start_pos + seqlen > lmax || qkv_batch_stride < 0 ||
      qkv_row_stride < ((long long)nheads + 2ll * nheads_kv) * head_dim || (long long)batch * seqlen * (head_dim / 8) > 0x3FFFFFFFll * 256)
    return AWQ_ERR_SHAPE;
  if (!aligned16(qkv) || !aligned16(freqs) || !aligned16(q_out) || !aligned16(k_cache) || !aligned16(v_cache) ||
      (qkv_batch_stride % 8) != 0 || (qkv_row_stride % 8) != 0)
    return AWQ_ERR_ALIGN;
  awq::launch_rope_kv_store(qkv, freqs, q_out, k_cache, v_cache, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim, lmax, start_pos,
                            qkv_batch_stride, qkv_row_stride, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_attn_splitkv_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* splits, int* chunk) {
  if (!splits || !chunk) return AWQ_ERR_NULL;
  if (!prefill_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal)) return AWQ_ERR_SHAPE;
  return awq::attn_splitkv_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal, splits, chunk);
}

size_t awq_attn_splitkv_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal) {
  if (!prefill_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal)) return 0;
  return awq::attn_splitkv_workspace_bytes(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, causal);
}

// ---- The natural-layout KV cache family (awq_kvcache.hpp): the rope + store of a chunk and the split-KV attention of few query rows, over
//      dense caches or a pool of pages (awq_paged.hpp), T or FP8 (awq_kv8.hpp), positions / lengths from the host or read on the device
//      (awq_devlen.hpp).  Every entry below builds one descriptor from its positional arguments; the checks exist once per phase -- null,
//      dtype, shape, alignment, then the attention tail -- and take the format-dependent terms from the descriptor and the entry's format.
using awq::KvAttnCall;
using awq::KvStoreCall;
using awq::KvView;
// what an entry requires of its descriptor; KV_ONEPASS: the one-pass prefill kernel serves, any seqlen_q (no seqlen_q * G <= 128 term)
// KV_VARQ: packed tokens / queries (awq_varq.hpp) -- cu_seqlens_q, max_seqlen_q and total_q in the place of one seqlen for the batch
// KV_MIX: a mixed step (awq_attn_varq and its siblings) -- split_seqlen_q and split_min_keys join the shape phase
// KV_WINDOW: a sliding window on a mixed step (awq_window.hpp) -- window_left >= 0 and causal join the shape phase
// KV_QKNORM: a store with the per-head q/k RMSNorm (the *_qknorm entries) -- q_gamma, k_gamma and norm_eps join the null, shape and
// alignment phases
enum { KV_FP8 = 1, KV_PAGED = 2, KV_DEVLEN = 4, KV_ONEPASS = 8, KV_VARQ = 16, KV_MIX = 32, KV_WINDOW = 64, KV_QKNORM = 128 };

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

static KvView kv_view(const void* k, const void* v, int outer, int rows, long long k_os = 0, long long k_rs = 0, long long v_os = 0,
                      long long v_rs = 0) {
  KvView kv;
  kv.k = k, kv.v = v, kv.outer = outer, kv.rows = rows;
  kv.k_os = k_os, kv.k_rs = k_rs, kv.v_os = v_os, kv.v_rs = v_rs;
  return kv;
}
static KvView with_scales(KvView kv, const float* k_scale, const float* v_scale, long long ks_os = 0, long long ks_rs = 0, long long vs_os = 0,
                          long long vs_rs = 0) {
  kv.k_scale = k_scale, kv.v_scale = v_scale;
  kv.ks_os = ks_os, kv.ks_rs = ks_rs, kv.vs_os = vs_os, kv.vs_rs = vs_rs;
  return kv;
}
static KvView with_table(KvView kv, const int* block_table, long long table_row_stride, int pages_per_seq) {
  kv.block_table = block_table, kv.bt_rs = table_row_stride, kv.pages_per_seq = pages_per_seq;
  return kv;
}

// The view's terms of the null, shape and alignment phases.  strided: the entry gives the caches' strides (every attention entry and the
// paged stores; the dense stores take contiguous caches).
static bool kv_has_null(const KvView& kv, int fmt) {
  return !kv.k || !kv.v || ((fmt & KV_FP8) && (!kv.k_scale || !kv.v_scale)) || ((fmt & KV_PAGED) && !kv.block_table);
}
static bool kv_shape_ok(const KvView& kv, int fmt, bool strided, int nheads_kv, int head_dim) {
  if ((fmt & KV_PAGED) && !(kv.rows >= 64 && (kv.rows % 64) == 0 && kv.outer >= 1 && kv.pages_per_seq >= 1 && kv.bt_rs >= kv.pages_per_seq))
    return false;
  if (!strided) return true;
  const long long row = (long long)nheads_kv * head_dim;
  if (kv.k_os < 0 || kv.v_os < 0 || kv.k_rs < row || kv.v_rs < row) return false;
  return !(fmt & KV_FP8) || (kv.ks_os >= 0 && kv.vs_os >= 0 && kv.ks_rs >= nheads_kv && kv.vs_rs >= nheads_kv);
}
static bool kv_aligned(const KvView& kv, int fmt, bool strided) {
  const int unit = (fmt & KV_FP8) ? 16 : 8;  // 16 bytes of T or of codes
  return aligned16(kv.k) && aligned16(kv.v) && (!(fmt & KV_FP8) || (aligned4(kv.k_scale) && aligned4(kv.v_scale))) &&
         (!(fmt & KV_PAGED) || aligned4(kv.block_table)) &&
         (!strided || ((kv.k_os % unit) == 0 && (kv.k_rs % unit) == 0 && (kv.v_os % unit) == 0 && (kv.v_rs % unit) == 0));
}

// the packed step's own terms of the null, shape and alignment phases (KV_VARQ); the grid term is the caller's
static bool varq_shape_ok(int batch, int max_seqlen_q, int total_q) { return batch <= 65535 && max_seqlen_q >= 1 && total_q >= 1; }

static int kv_store(const KvStoreCall& c, int fmt, void* stream) {
  const KvView& kv = c.kv;
  const bool paged = fmt & KV_PAGED, devlen = fmt & KV_DEVLEN, varq = fmt & KV_VARQ, norm = fmt & KV_QKNORM;
  if (!c.qkv || !c.freqs || !c.q_out || kv_has_null(kv, fmt) || (devlen && !c.cache_seqlens) || (varq && !c.cu_seqlens_q) ||
      (norm && (!c.q_gamma || !c.k_gamma)))
    return AWQ_ERR_NULL;
  if (c.dtype != AWQ_F16 && c.dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  // tokens of the call: the rectangle, or the packed rows (c.S is then max_seqlen_q)
  const long long tokens = varq ? (long long)c.total_q : (long long)c.B * c.S;
  if (c.B < 1 || c.S < 1 || c.H < 1 || c.Hkv < 1 || (c.Dh != 64 && c.Dh != 128) || c.rot < 16 || (c.rot % 16) != 0 || c.rot > c.Dh || c.bs < 0 ||
      c.rs < ((long long)c.H + 2ll * c.Hkv) * c.Dh || (varq && !varq_shape_ok(c.B, c.max_seqlen_q, c.total_q)) ||
      tokens * (c.Dh / 8) > 0x3FFFFFFFll * 256 || (!paged && (kv.outer < c.B || kv.rows < 1)) || !kv_shape_ok(kv, fmt, paged, c.Hkv, c.Dh) ||
      (devlen ? c.table_rows < 1 : (c.start_pos < 0 || (long long)c.start_pos + c.S > kv.rows)) ||
      (norm && !(c.norm_eps >= 0.f && c.norm_eps <= 3.402823466e38f)))  // negative, infinite or NaN
    return AWQ_ERR_SHAPE;
  if (!aligned16(c.qkv) || !aligned16(c.freqs) || !aligned16(c.q_out) || !kv_aligned(kv, fmt, paged) || (devlen && !aligned4(c.cache_seqlens)) ||
      (varq && !aligned4(c.cu_seqlens_q)) || (c.bs % 8) != 0 || (c.rs % 8) != 0 || (norm && (!aligned16(c.q_gamma) || !aligned16(c.k_gamma))))
    return AWQ_ERR_ALIGN;
  awq::launch_kv_store(c, (hipStream_t)stream);
  return finish_launch();
}

// a packed-token store call: the device-position descriptor with the packed step's three fields; S carries max_seqlen_q
static KvStoreCall varq_store_call(const void* qkv, const float* freqs_table, void* q_out, const KvView& kv, const int* cache_seqlens, int table_rows,
                                   int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim,
                                   int rot_dim, long long qkv_row_stride, int dtype) {
  KvStoreCall c{qkv, freqs_table, q_out, kv, 0, cache_seqlens, table_rows, batch, max_seqlen_q, nheads, nheads_kv, head_dim, rot_dim, 0,
                qkv_row_stride, dtype};
  c.cu_seqlens_q = cu_seqlens_q, c.max_seqlen_q = max_seqlen_q, c.total_q = total_q;
  return c;
}

// a *_qknorm entry's descriptor: its sibling's with the norm's three fields
static KvStoreCall with_qk_norm(KvStoreCall c, const float* q_gamma, const float* k_gamma, float norm_eps) {
  c.q_gamma = q_gamma, c.k_gamma = k_gamma, c.norm_eps = norm_eps;
  return c;
}

// the split pair always runs under device lengths: Sq * G <= 128 and Dh 64 / 128 are requirements, not routing conditions.  one_pass
// (awq_attn_prefill_kvcache and its siblings): any seqlen_q whose grid of 64-row q tiles fits an int, as in prefill_shape_ok
static bool kvcache_shape_ok(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k, bool one_pass = false) {
  return batch >= 1 && nheads >= 1 && nheads_kv >= 1 && (nheads % nheads_kv) == 0 && (head_dim == 64 || head_dim == 128) && seqlen_q >= 1 &&
         (one_pass ? (long long)batch * nheads * ((seqlen_q + 63) / 64) <= 0x7FFFFFFFll : (long long)seqlen_q * (nheads / nheads_kv) <= 128) &&
         max_seqlen_k >= 1;
}

int awq_attn_kvcache_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k, int* splits, int* chunk) {
  if (!splits || !chunk) return AWQ_ERR_NULL;
  if (!kvcache_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, max_seqlen_k)) return AWQ_ERR_SHAPE;
  return awq::attn_kvcache_plan(batch, nheads_kv, max_seqlen_k, splits, chunk);
}

size_t awq_attn_kvcache_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k) {
  if (!kvcache_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, max_seqlen_k)) return 0;
  return awq::attn_kvcache_workspace_bytes(batch, nheads, nheads_kv, head_dim, seqlen_q, max_seqlen_k);
}

// the four phases every attention entry shares; AWQ_OK: the tail (kv_attn) or the one-pass launch may go on
static int kv_attn_check(const KvAttnCall& c, int fmt) {
  const KvView& kv = c.kv;
  const bool devlen = fmt & KV_DEVLEN, varq = fmt & KV_VARQ;
  if (!c.q || !c.out || kv_has_null(kv, fmt) || (devlen && !c.seqlens_k) || (varq && !c.cu_seqlens_q)) return AWQ_ERR_NULL;
  if (c.dtype != AWQ_F16 && c.dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  // (packed queries: c.Sq is max_seqlen_q, so the one-pass grid term bounds ceil(max_seqlen_q / 64) * batch * nheads)
  if (varq && !varq_shape_ok(c.B, c.max_seqlen_q, c.total_q)) return AWQ_ERR_SHAPE;
  // (a mixed step: the split pair's rows per KV head fit its four waves; c.H / c.Hkv is formed only behind the terms that make it safe)
  if ((fmt & KV_MIX) && (c.split_seqlen_q < 0 || c.split_min_keys < 1 ||
                         (c.H >= 1 && c.Hkv >= 1 && (c.H % c.Hkv) == 0 && (long long)c.split_seqlen_q * (c.H / c.Hkv) > 128)))
    return AWQ_ERR_SHAPE;
  if ((fmt & KV_WINDOW) && (c.window_left < 0 || !c.causal)) return AWQ_ERR_SHAPE;
  // (a cap, awq_softcap.hpp: 0 is none, anything else finite and positive; the comparison refuses a NaN)
  if (!(c.softcap >= 0.f && c.softcap <= 3.4028234663852886e38f)) return AWQ_ERR_SHAPE;
  // (host lengths: the T entry keeps the one-pass kernel's head dim 72 for the calls the plan hands to it; the FP8 kernels have 64 / 128)
  if (!(devlen ? kvcache_shape_ok(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.max_seqlen_k, fmt & KV_ONEPASS)
               : ((!(fmt & KV_FP8) || c.Dh == 64 || c.Dh == 128) && prefill_shape_ok(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.Sk, c.causal))) ||
      !kv_shape_ok(kv, fmt, true, c.Hkv, c.Dh) || c.q_bs < 0 || c.q_rs < (long long)c.H * c.Dh)
    return AWQ_ERR_SHAPE;
  if (!aligned16(c.q) || !aligned16(c.out) || !kv_aligned(kv, fmt, true) || (c.q_bs % 8) != 0 || (c.q_rs % 8) != 0 ||
      (varq && !aligned4(c.cu_seqlens_q)))
    return AWQ_ERR_ALIGN;
  return AWQ_OK;
}

// check, plan, workspace, launch.  Under a host length a plan of one split is the one-pass launch, bit for bit.
static int kv_attn(const KvAttnCall& c, int fmt, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView& kv = c.kv;
  const int rc = kv_attn_check(c, fmt);
  if (rc != AWQ_OK) return rc;
  int splits = 1, chunk = 0;
  size_t need = 0;
  if (fmt & KV_DEVLEN) {
    if (c.max_seqlen_k > kv.capacity() || c.seqlen_offset < 0) return AWQ_ERR_SHAPE;
    if (!aligned4(c.seqlens_k)) return AWQ_ERR_ALIGN;
    awq::attn_kvcache_plan(c.B, c.Hkv, c.max_seqlen_k, &splits, &chunk);
    need = awq::attn_kvcache_workspace_bytes(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.max_seqlen_k);
  } else {
    awq::attn_splitkv_plan(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.Sk, c.causal, &splits, &chunk);
    if (splits <= 1)
      return kv.k_scale ? awq_attn_prefill_kv8(c.q, kv.k, kv.v, kv.k_scale, kv.v_scale, c.out, c.B, c.Sq, c.Sk, c.H, c.Hkv, c.Dh, c.q_bs, c.q_rs,
                                               kv.k_os, kv.k_rs, kv.v_os, kv.v_rs, kv.ks_os, kv.ks_rs, kv.vs_os, kv.vs_rs, c.scale, c.causal,
                                               c.dtype, stream)
                        : awq_attn_prefill(c.q, kv.k, kv.v, c.out, c.B, c.Sq, c.Sk, c.H, c.Hkv, c.Dh, c.q_bs, c.q_rs, kv.k_os, kv.k_rs, kv.v_os,
                                           kv.v_rs, c.scale, c.causal, c.dtype, stream);
    need = awq::attn_splitkv_workspace_bytes(c.B, c.H, c.Hkv, c.Dh, c.Sq, c.Sk, c.causal);
  }
  if (!workspace || workspace_bytes < need) return AWQ_ERR_WORKSPACE;
  if (!aligned16(workspace)) return AWQ_ERR_ALIGN;
  if ((long long)c.B * c.Hkv * splits > 0x7FFFFFFFll) return AWQ_ERR_SHAPE;
  awq::launch_kv_attn(c, splits, chunk, workspace, (hipStream_t)stream);
  return finish_launch();
}

// The one-pass prefill kernel under device lengths (awq_attn_prefill_kvcache[_kv8], awq_attn_prefill_paged[_kv8]): the same four phases
// with the seqlen_q * G <= 128 term lifted, the tail of the device-length entries, no plan and no workspace.
static int kv_prefill(const KvAttnCall& c, int fmt, void* stream) {
  const int rc = kv_attn_check(c, fmt | KV_ONEPASS);
  if (rc != AWQ_OK) return rc;
  if (c.max_seqlen_k > c.kv.capacity() || c.seqlen_offset < 0) return AWQ_ERR_SHAPE;
  if (!aligned4(c.seqlens_k)) return AWQ_ERR_ALIGN;
  awq::launch_kv_prefill(c, (hipStream_t)stream);
  return finish_launch();
}

int awq_rope_kv_store_natural(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int batch, int cache_batch,
                              int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos, long long qkv_batch_stride,
                              long long qkv_row_stride, int dtype, void* stream) {
  return kv_store({qkv, freqs, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), start_pos, nullptr, 0, batch, seqlen, nheads, nheads_kv,
                   head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype},
                  0, stream);
}

int awq_rope_kv_store_natural_fp8(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                  int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                  int start_pos, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream) {
  return kv_store({qkv, freqs, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale), start_pos, nullptr, 0, batch,
                   seqlen, nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype},
                  KV_FP8, stream);
}

int awq_rope_kv_store_natural_pos(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens,
                                  int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                  int table_rows, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream) {
  return kv_store({qkv, freqs_table, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), 0, cache_seqlens, table_rows, batch, seqlen, nheads,
                   nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype},
                  KV_DEVLEN, stream);
}

int awq_rope_kv_store_natural_pos_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, float* k_scale,
                                      float* v_scale, const int* cache_seqlens, int batch, int cache_batch, int seqlen, int nheads,
                                      int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_batch_stride,
                                      long long qkv_row_stride, int dtype, void* stream) {
  return kv_store({qkv, freqs_table, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale), 0, cache_seqlens,
                   table_rows, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype},
                  KV_FP8 | KV_DEVLEN, stream);
}

int awq_rope_kv_store_paged_pos(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, const int* block_table,
                                const int* cache_seqlens, int batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_store({qkv, freqs_table, q_out, kv, 0, cache_seqlens, table_rows, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim,
                   qkv_batch_stride, qkv_row_stride, dtype},
                  KV_PAGED | KV_DEVLEN, stream);
}

int awq_rope_kv_store_paged_pos_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, float* k_scale,
                                    float* v_scale, const int* block_table, const int* cache_seqlens, int batch, int seqlen, int nheads,
                                    int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                    long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                    long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                    long long v_scale_page_stride, long long v_scale_row_stride, long long qkv_batch_stride,
                                    long long qkv_row_stride, int dtype, void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_store({qkv, freqs_table, q_out, kv, 0, cache_seqlens, table_rows, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim,
                   qkv_batch_stride, qkv_row_stride, dtype},
                  KV_FP8 | KV_PAGED | KV_DEVLEN, stream);
}

// The six rectangle stores with the per-head q/k RMSNorm in front of the rotation (awq_rope.hpp): each is its sibling's descriptor with
// q_gamma, k_gamma (fp32 [head_dim]) and norm_eps set; the NORM instantiation of the same kernel serves.
int awq_rope_kv_store_natural_qknorm(const void* qkv, const float* freqs, const float* q_gamma, const float* k_gamma, float norm_eps, void* q_out,
                                     void* k_cache, void* v_cache, int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim,
                                     int rot_dim, int lmax, int start_pos, long long qkv_batch_stride, long long qkv_row_stride, int dtype,
                                     void* stream) {
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), start_pos, nullptr, 0, batch, seqlen,
      nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma, norm_eps), KV_QKNORM, stream);
}

int awq_rope_kv_store_natural_fp8_qknorm(const void* qkv, const float* freqs, const float* q_gamma, const float* k_gamma, float norm_eps, void* q_out,
                                         void* k_cache, void* v_cache, float* k_scale, float* v_scale, int batch, int cache_batch, int seqlen,
                                         int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos, long long qkv_batch_stride,
                                         long long qkv_row_stride, int dtype, void* stream) {
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale), start_pos,
      nullptr, 0, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma, norm_eps),
      KV_FP8 | KV_QKNORM, stream);
}

int awq_rope_kv_store_natural_pos_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                         void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens, int batch, int cache_batch, int seqlen,
                                         int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_batch_stride,
                                         long long qkv_row_stride, int dtype, void* stream) {
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs_table, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), 0, cache_seqlens, table_rows, batch,
      seqlen, nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma, norm_eps), KV_DEVLEN | KV_QKNORM,
      stream);
}

int awq_rope_kv_store_natural_pos_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                             void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const int* cache_seqlens,
                                             int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                             int table_rows, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream) {
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs_table, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale), 0,
      cache_seqlens, table_rows, batch, seqlen, nheads, nheads_kv, head_dim, rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma,
      norm_eps), KV_FP8 | KV_DEVLEN | KV_QKNORM, stream);
}

int awq_rope_kv_store_paged_pos_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                       void* q_out, void* k_pool, void* v_pool, const int* block_table, const int* cache_seqlens, int batch,
                                       int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size,
                                       int pages_per_seq, long long table_row_stride, long long k_page_stride, long long k_row_stride,
                                       long long v_page_stride, long long v_row_stride, long long qkv_batch_stride, long long qkv_row_stride,
                                       int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride), block_table,
      table_row_stride, pages_per_seq);
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs_table, q_out, kv, 0, cache_seqlens, table_rows, batch, seqlen, nheads, nheads_kv, head_dim,
      rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma, norm_eps), KV_PAGED | KV_DEVLEN | KV_QKNORM, stream);
}

int awq_rope_kv_store_paged_pos_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                           void* q_out, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* block_table,
                                           const int* cache_seqlens, int batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                           int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                           long long k_scale_page_stride, long long k_scale_row_stride, long long v_scale_page_stride,
                                           long long v_scale_row_stride, long long qkv_batch_stride, long long qkv_row_stride, int dtype,
                                           void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
      k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride), block_table, table_row_stride,
      pages_per_seq);
  return kv_store(with_qk_norm(KvStoreCall{qkv, freqs_table, q_out, kv, 0, cache_seqlens, table_rows, batch, seqlen, nheads, nheads_kv, head_dim,
      rot_dim, qkv_batch_stride, qkv_row_stride, dtype}, q_gamma, k_gamma, norm_eps), KV_FP8 | KV_PAGED | KV_DEVLEN | KV_QKNORM, stream);
}

int awq_attn_splitkv(const void* q, const void* k, const void* v, void* out, int batch, int seqlen_q, int seqlen_k, int nheads, int nheads_kv,
                     int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                     long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* workspace,
                     size_t workspace_bytes, void* stream) {
  const KvView kv = kv_view(k, v, batch, seqlen_k, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_attn({q, out, kv, seqlen_k, nullptr, 0, 0, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride, q_row_stride, softmax_scale,
                  causal, dtype},
                 0, workspace, workspace_bytes, stream);
}

// k / v [batch, seqlen_k, Hkv, Dh] of e4m3 codes with their scales, as one descriptor (both host-length FP8 entries)
static KvAttnCall kv8_attn_call(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int batch,
                                int seqlen_q, int seqlen_k, int nheads, int nheads_kv, int head_dim, long long q_batch_stride,
                                long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                                long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                                long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype) {
  const KvView kv = with_scales(kv_view(k, v, batch, seqlen_k, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale, v_scale,
                                k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return {q, out, kv, seqlen_k, nullptr, 0, 0, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride, q_row_stride, softmax_scale, causal,
          dtype};
}

int awq_attn_prefill_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, int seqlen_k, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                         long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                         long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                         long long v_scale_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  const int rc = kv_attn_check(kv8_attn_call(q, k, v, k_scale, v_scale, out, batch, seqlen_q, seqlen_k, nheads, nheads_kv, head_dim, q_batch_stride,
                                             q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, k_scale_batch_stride,
                                             k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride, softmax_scale, causal, dtype),
                               KV_FP8);
  if (rc != AWQ_OK) return rc;
  awq::launch_attn_prefill_kv8(q, k, v, k_scale, v_scale, out, batch, seqlen_q, seqlen_k, nheads, nheads_kv, head_dim, q_batch_stride,
                               q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, k_scale_batch_stride,
                               k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride, softmax_scale, causal, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_attn_splitkv_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, int seqlen_k, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                         long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                         long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                         long long v_scale_row_stride, float softmax_scale, int causal, int dtype, void* workspace, size_t workspace_bytes,
                         void* stream) {
  return kv_attn(kv8_attn_call(q, k, v, k_scale, v_scale, out, batch, seqlen_q, seqlen_k, nheads, nheads_kv, head_dim, q_batch_stride, q_row_stride,
                               k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, k_scale_batch_stride, k_scale_row_stride,
                               v_scale_batch_stride, v_scale_row_stride, softmax_scale, causal, dtype),
                 KV_FP8, workspace, workspace_bytes, stream);
}

int awq_attn_kvcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int seqlen_q, const int* seqlens_k,
                     int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_batch_stride,
                     long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                     float softmax_scale, int causal, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_attn({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                  q_row_stride, softmax_scale, causal, dtype},
                 KV_DEVLEN, workspace, workspace_bytes, stream);
}

int awq_attn_kvcache_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                         long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                         long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                         void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_attn({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                  q_row_stride, softmax_scale, causal, dtype},
                 KV_FP8 | KV_DEVLEN, workspace, workspace_bytes, stream);
}

int awq_attn_kvcache_paged(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch, int seqlen_q,
                           const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq,
                           long long table_row_stride, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, float softmax_scale,
                           int causal, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_attn({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                  q_row_stride, softmax_scale, causal, dtype},
                 KV_PAGED | KV_DEVLEN, workspace, workspace_bytes, stream);
}

int awq_attn_kvcache_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                               const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                               int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                               int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                               long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_attn({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                  q_row_stride, softmax_scale, causal, dtype},
                 KV_FP8 | KV_PAGED | KV_DEVLEN, workspace, workspace_bytes, stream);
}

// ---- shared-prefix decode on the paged cache (awq_shared.hpp): attn_kvcache_paged's phases with the group arrays' terms in each ----
using awq::KvSharedCall;

static bool shared_shape_ok(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix, int max_seqlen_k) {
  return kvcache_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, max_seqlen_k) && max_prefix >= 64 && (max_prefix % 64) == 0 &&
         max_prefix <= max_seqlen_k;
}

int awq_attn_kvcache_shared_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix, int max_seqlen_k,
                                 int* splits_p, int* chunk_p, int* splits_s, int* chunk_s) {
  if (!splits_p || !chunk_p || !splits_s || !chunk_s) return AWQ_ERR_NULL;
  if (!shared_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, max_prefix, max_seqlen_k)) return AWQ_ERR_SHAPE;
  return awq::attn_kvcache_shared_plan(batch, nheads_kv, max_prefix, max_seqlen_k, splits_p, chunk_p, splits_s, chunk_s);
}

size_t awq_attn_kvcache_shared_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix,
                                               int max_seqlen_k) {
  if (!shared_shape_ok(batch, nheads, nheads_kv, head_dim, seqlen_q, max_prefix, max_seqlen_k)) return 0;
  return awq::attn_kvcache_shared_workspace_bytes(batch, nheads, nheads_kv, head_dim, seqlen_q, max_prefix, max_seqlen_k);
}

static int kv_attn_shared(const KvAttnCall& c, const KvSharedCall& s, int fmt, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView& kv = c.kv;
  if (!s.group_members || !s.group_prefix || !s.seq_prefix) return AWQ_ERR_NULL;
  const int rc = kv_attn_check(c, fmt);
  if (rc != AWQ_OK) return rc;
  // (every row of a group shares one MFMA tile: group_cap * Sq * G <= 128; kv_attn_check has made H / Hkv safe)
  if (s.num_groups < 1 || s.group_cap < 1 || s.members_row_stride < s.group_cap || (long long)s.group_cap * c.Sq * (c.H / c.Hkv) > 128 ||
      s.max_prefix < 64 || (s.max_prefix % 64) != 0 || s.max_prefix > c.max_seqlen_k || c.max_seqlen_k > kv.capacity() || c.seqlen_offset < 0)
    return AWQ_ERR_SHAPE;
  if (!aligned4(c.seqlens_k) || !aligned4(s.group_members) || !aligned4(s.group_prefix) || !aligned4(s.seq_prefix)) return AWQ_ERR_ALIGN;
  int splits_p = 1, chunk_p = 0, splits_s = 1, chunk_s = 0;
  awq::attn_kvcache_shared_plan(c.B, c.Hkv, s.max_prefix, c.max_seqlen_k, &splits_p, &chunk_p, &splits_s, &chunk_s);
  const size_t need = awq::attn_kvcache_shared_workspace_bytes(c.B, c.H, c.Hkv, c.Dh, c.Sq, s.max_prefix, c.max_seqlen_k);
  if (!workspace || workspace_bytes < need) return AWQ_ERR_WORKSPACE;
  if (!aligned16(workspace)) return AWQ_ERR_ALIGN;
  if ((long long)c.B * c.Hkv * splits_s > 0x7FFFFFFFll || (long long)s.num_groups * c.Hkv * splits_p > 0x7FFFFFFFll) return AWQ_ERR_SHAPE;
  awq::launch_kv_attn_shared(c, s, workspace, (hipStream_t)stream);
  return finish_launch();
}

int awq_attn_kvcache_paged_shared(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                                  int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size,
                                  int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                  long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                                  long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype,
                                  const int* group_members, const int* group_prefix, const int* seq_prefix, int num_groups, int group_cap,
                                  long long members_row_stride, int max_prefix, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  KvSharedCall s;
  s.group_members = group_members, s.group_prefix = group_prefix, s.seq_prefix = seq_prefix, s.members_row_stride = members_row_stride;
  s.num_groups = num_groups, s.group_cap = group_cap, s.max_prefix = max_prefix;
  return kv_attn_shared({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                         q_row_stride, softmax_scale, causal, dtype},
                        s, KV_PAGED | KV_DEVLEN, workspace, workspace_bytes, stream);
}

int awq_attn_kvcache_paged_shared_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                      const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                                      int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                                      int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride,
                                      long long k_row_stride, long long v_page_stride, long long v_row_stride, long long k_scale_page_stride,
                                      long long k_scale_row_stride, long long v_scale_page_stride, long long v_scale_row_stride,
                                      float softmax_scale, int causal, int dtype, const int* group_members, const int* group_prefix,
                                      const int* seq_prefix, int num_groups, int group_cap, long long members_row_stride, int max_prefix,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  KvSharedCall s;
  s.group_members = group_members, s.group_prefix = group_prefix, s.seq_prefix = seq_prefix, s.members_row_stride = members_row_stride;
  s.num_groups = num_groups, s.group_cap = group_cap, s.max_prefix = max_prefix;
  return kv_attn_shared({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                         q_row_stride, softmax_scale, causal, dtype},
                        s, KV_FP8 | KV_PAGED | KV_DEVLEN, workspace, workspace_bytes, stream);
}

// the copy-on-write of a fork's tail page: n (src, dst) pairs of pages of the pools, K and V rows (and the scales of FP8 pools)
static int kv_page_copy(const KvView& kv, int fmt, const int* src_pages, const int* dst_pages, int n, int nheads_kv, int head_dim, void* stream) {
  if (!kv.k || !kv.v || ((fmt & KV_FP8) && (!kv.k_scale || !kv.v_scale)) || !src_pages || !dst_pages) return AWQ_ERR_NULL;
  if (n < 1 || nheads_kv < 1 || (head_dim != 64 && head_dim != 128) || kv.outer < 1 || kv.rows < 64 || (kv.rows % 64) != 0 ||
      !kv_shape_ok(kv, fmt & KV_FP8, true, nheads_kv, head_dim) ||
      ((long long)n * kv.rows * (nheads_kv * head_dim / 8) + 255) / 256 > 0x7FFFFFFFll)
    return AWQ_ERR_SHAPE;
  if (!kv_aligned(kv, fmt & KV_FP8, true) || !aligned4(src_pages) || !aligned4(dst_pages)) return AWQ_ERR_ALIGN;
  awq::launch_kv_page_copy({kv, src_pages, dst_pages, n, nheads_kv, head_dim}, (hipStream_t)stream);
  return finish_launch();
}

int awq_kv_page_copy(void* k_pool, void* v_pool, const int* src_pages, const int* dst_pages, int n, int num_pages, int page_size, int nheads_kv,
                     int head_dim, long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, void* stream) {
  return kv_page_copy(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride), 0, src_pages,
                      dst_pages, n, nheads_kv, head_dim, stream);
}

int awq_kv_page_copy_fp8(void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* src_pages, const int* dst_pages, int n,
                         int num_pages, int page_size, int nheads_kv, int head_dim, long long k_page_stride, long long k_row_stride,
                         long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                         long long v_scale_page_stride, long long v_scale_row_stride, void* stream) {
  return kv_page_copy(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride), k_scale,
                                  v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                      KV_FP8, src_pages, dst_pages, n, nheads_kv, head_dim, stream);
}

int awq_attn_prefill_kvcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int seqlen_q, const int* seqlens_k,
                             int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_batch_stride,
                             long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                             long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_prefill({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                     q_row_stride, softmax_scale, causal, dtype},
                    KV_DEVLEN, stream);
}

int awq_attn_prefill_kvcache_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                                 int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int lmax, int nheads,
                                 int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride,
                                 long long k_row_stride, long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride,
                                 long long k_scale_row_stride, long long v_scale_batch_stride, long long v_scale_row_stride,
                                 float softmax_scale, int causal, int dtype, void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_prefill({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                     q_row_stride, softmax_scale, causal, dtype},
                    KV_FP8 | KV_DEVLEN, stream);
}

int awq_attn_prefill_paged(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch, int seqlen_q,
                           const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq,
                           long long table_row_stride, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, float softmax_scale,
                           int causal, int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_prefill({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                     q_row_stride, softmax_scale, causal, dtype},
                    KV_PAGED | KV_DEVLEN, stream);
}

int awq_attn_prefill_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                               const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                               int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                               int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                               long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                               void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_prefill({q, out, kv, 0, seqlens_k, seqlen_offset, max_seqlen_k, batch, seqlen_q, nheads, nheads_kv, head_dim, q_batch_stride,
                     q_row_stride, softmax_scale, causal, dtype},
                    KV_FP8 | KV_PAGED | KV_DEVLEN, stream);
}

// ---- packed queries (awq_varq.hpp): one store launch and one attention launch for any mix of new-token counts
int awq_attn_varq_plan(int batch, int nheads, int nheads_kv, int head_dim, int max_seqlen_q, int* q_tile_rows, int* blocks) {
  if (!q_tile_rows || !blocks) return AWQ_ERR_NULL;
  if (!kvcache_shape_ok(batch, nheads, nheads_kv, head_dim, max_seqlen_q, 1, true) || batch > 65535) return AWQ_ERR_SHAPE;
  return awq::attn_varq_plan(batch, nheads, nheads_kv, head_dim, max_seqlen_q, q_tile_rows, blocks);
}

// a packed-query attention call: the device-length descriptor with the packed step's three fields; Sq carries max_seqlen_q and
// seqlen_offset the flag
static KvAttnCall varq_attn_call(const void* q, void* out, const KvView& kv, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                 const int* seqlens_k, int lens_before_step, int max_seqlen_k, int nheads, int nheads_kv, int head_dim,
                                 long long q_row_stride, float softmax_scale, int causal, int dtype) {
  KvAttnCall c{q, out, kv, 0, seqlens_k, lens_before_step ? 1 : 0, max_seqlen_k, batch, max_seqlen_q, nheads, nheads_kv, head_dim, 0, q_row_stride,
               softmax_scale, causal, dtype};
  c.cu_seqlens_q = cu_seqlens_q, c.max_seqlen_q = max_seqlen_q, c.total_q = total_q;
  return c;
}

int awq_attn_prefill_kvcache_varq(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q,
                                  int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax,
                                  int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_batch_stride,
                                  long long k_row_stride, long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal,
                                  int dtype, void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_prefill(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                   nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                    KV_DEVLEN | KV_VARQ, stream);
}

int awq_attn_prefill_kvcache_varq_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                                      void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k,
                                      int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim,
                                      long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                                      long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                                      long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                      void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_prefill(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                   nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                    KV_FP8 | KV_DEVLEN | KV_VARQ, stream);
}

int awq_attn_prefill_paged_varq(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                                const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                                int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                                int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                                long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_prefill(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                   nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                    KV_PAGED | KV_DEVLEN | KV_VARQ, stream);
}

int awq_attn_prefill_paged_varq_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                    const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                    const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                    int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                    long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                    long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                    long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                    void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_prefill(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                   nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                    KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ, stream);
}

// ---- a mixed step (awq_varq.hpp): the packed one-pass launch for the prompt chunks and the packed split pair for the short sequences over a
//      long history, three launches whose set never depends on what the step holds.  The plan is awq_attn_kvcache_plan's for the same bound.
static bool varq_split_shape_ok(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k) {
  return split_seqlen_q >= 0 && batch <= 65535 &&
         kvcache_shape_ok(batch, nheads, nheads_kv, head_dim, split_seqlen_q > 0 ? split_seqlen_q : 1, max_seqlen_k);
}

int awq_attn_varq_split_plan(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int* splits, int* chunk) {
  if (!splits || !chunk) return AWQ_ERR_NULL;
  if (!varq_split_shape_ok(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k)) return AWQ_ERR_SHAPE;
  return awq::attn_kvcache_plan(batch, nheads_kv, max_seqlen_k, splits, chunk);
}

size_t awq_attn_varq_split_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k) {
  if (!varq_split_shape_ok(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k)) return 0;
  return awq::attn_kvcache_workspace_bytes(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k);
}

// check, workspace, then the one-pass launch, the split launch and the combine in one stream.  Every check stands in front of the first
// launch.  split_seqlen_q = 0: awq_attn_prefill_*_varq, that launch alone and no workspace.
static int window_clamped(int window_left, int max_seqlen_k) { return window_left < max_seqlen_k - 1 ? window_left : max_seqlen_k - 1; }

// windowed (awq_window.hpp, the *_window entries): window_left >= 0 and causal join the shape phase, the window is clamped to
// max_seqlen_k - 1 (beyond that it hides no key), and the plan and the workspace are the window's.
// softcap (awq_softcap.hpp, the *_softcap entries): a windowed call whose logits are capped; 0 is the windowed call itself, bit for bit.
static int kv_varq_attn(KvAttnCall c, int fmt, int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes, void* stream,
                        bool windowed = false, int window_left = 0, float softcap = 0.f) {
  c.split_seqlen_q = split_seqlen_q, c.split_min_keys = split_min_keys;
  if (windowed) c.window_left = window_left, c.softcap = softcap;
  const int rc = kv_attn_check(c, fmt | KV_ONEPASS | KV_MIX | (windowed ? KV_WINDOW : 0));
  if (rc != AWQ_OK) return rc;
  if (c.max_seqlen_k > c.kv.capacity() || c.seqlen_offset < 0) return AWQ_ERR_SHAPE;
  if (!aligned4(c.seqlens_k)) return AWQ_ERR_ALIGN;
  if (windowed) c.window_left = window_clamped(window_left, c.max_seqlen_k);
  int splits = 1, chunk = 0;
  if (split_seqlen_q > 0) {
    if (windowed) awq::attn_varq_window_plan(c.B, c.Hkv, split_seqlen_q, c.max_seqlen_k, c.window_left, &splits, &chunk);
    else awq::attn_kvcache_plan(c.B, c.Hkv, c.max_seqlen_k, &splits, &chunk);
    const size_t need = windowed ? awq::attn_varq_window_workspace_bytes(c.B, c.H, c.Hkv, c.Dh, split_seqlen_q, c.max_seqlen_k, c.window_left)
                                 : awq::attn_kvcache_workspace_bytes(c.B, c.H, c.Hkv, c.Dh, split_seqlen_q, c.max_seqlen_k);
    if (!workspace || workspace_bytes < need) return AWQ_ERR_WORKSPACE;
    if (!aligned16(workspace)) return AWQ_ERR_ALIGN;
    if ((long long)c.B * c.Hkv * splits > 0x7FFFFFFFll) return AWQ_ERR_SHAPE;
  }
  awq::launch_kv_prefill(c, (hipStream_t)stream);
  if (split_seqlen_q > 0) awq::launch_kv_attn(c, splits, chunk, workspace, (hipStream_t)stream);
  return finish_launch();
}

int awq_attn_varq(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                  int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim,
                  long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                  float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes,
                  void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream);
}

int awq_attn_varq_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out, int batch,
                      const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k,
                      int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                      long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                      long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                      int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream);
}

int awq_attn_paged_varq(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                        const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k,
                        int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                        long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                        float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream);
}

int awq_attn_paged_varq_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                            const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k,
                            int lens_before_step, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                            int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                            long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                            long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                            int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream);
}

// ---- a sliding window on a mixed step (awq_window.hpp): the four entries above with window_left behind split_min_keys

int awq_attn_varq_window_plan(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int window_left,
                              int* splits, int* chunk) {
  if (!splits || !chunk) return AWQ_ERR_NULL;
  if (!varq_split_shape_ok(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k) || window_left < 0) return AWQ_ERR_SHAPE;
  return awq::attn_varq_window_plan(batch, nheads_kv, split_seqlen_q, max_seqlen_k, window_clamped(window_left, max_seqlen_k), splits, chunk);
}

size_t awq_attn_varq_window_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k,
                                            int window_left) {
  if (!varq_split_shape_ok(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k) || window_left < 0) return 0;
  return awq::attn_varq_window_workspace_bytes(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k,
                                               window_clamped(window_left, max_seqlen_k));
}

int awq_attn_varq_window(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                         int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                         long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                         int window_left, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left);
}

int awq_attn_varq_window_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                             int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                             int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride,
                             long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                             long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                             long long v_scale_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                             int window_left, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left);
}

int awq_attn_paged_varq_window(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                               const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                               int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                               int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q,
                               int split_min_keys, int window_left, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left);
}

int awq_attn_paged_varq_window_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                   const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                   const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                   int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                   long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                   long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                   long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                   int split_seqlen_q, int split_min_keys, int window_left, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left);
}

// ---- a cap on the logits of a windowed mixed step (awq_softcap.hpp): the four entries above with softcap behind window_left.  The plan
//      and the workspace are awq_attn_varq_window_plan / awq_attn_varq_window_workspace_bytes; softcap = 0 is the *_window entry

int awq_attn_varq_softcap(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                         int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                         long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                         int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left, softcap);
}

int awq_attn_varq_softcap_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                             int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                             int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride,
                             long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                             long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                             long long v_scale_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                             int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_scales(kv_view(k_cache, v_cache, batch, lmax, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride), k_scale,
                                v_scale, k_scale_batch_stride, k_scale_row_stride, v_scale_batch_stride, v_scale_row_stride);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left, softcap);
}

int awq_attn_paged_varq_softcap(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                               const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                               int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                               int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q,
                               int split_min_keys, int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left, softcap);
}

int awq_attn_paged_varq_softcap_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                   const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                   const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                   int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                   long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                   long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                   long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                   int split_seqlen_q, int split_min_keys, int window_left, float softcap, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_varq_attn(varq_attn_call(q, out, kv, batch, cu_seqlens_q, max_seqlen_q, total_q, seqlens_k, lens_before_step, max_seqlen_k, nheads,
                                     nheads_kv, head_dim, q_row_stride, softmax_scale, causal, dtype),
                      KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ, split_seqlen_q, split_min_keys, workspace, workspace_bytes, stream, true, window_left, softcap);
}

int awq_rope_kv_store_natural_varq(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens,
                                   int batch, int cache_batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                   int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype,
                                   void* stream) {
  return kv_store(varq_store_call(qkv, freqs_table, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), cache_seqlens, table_rows, batch,
                                  cu_seqlens_q, max_seqlen_q, total_q, nheads, nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype),
                  KV_DEVLEN | KV_VARQ, stream);
}

int awq_rope_kv_store_natural_varq_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, float* k_scale,
                                       float* v_scale, const int* cache_seqlens, int batch, int cache_batch, const int* cu_seqlens_q,
                                       int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                       int table_rows, long long qkv_row_stride, int dtype, void* stream) {
  return kv_store(varq_store_call(qkv, freqs_table, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale),
                                  cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q, nheads, nheads_kv, head_dim, rot_dim,
                                  qkv_row_stride, dtype),
                  KV_FP8 | KV_DEVLEN | KV_VARQ, stream);
}

int awq_rope_kv_store_paged_varq(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, const int* block_table,
                                 const int* cache_seqlens, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                 int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                 long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                 long long v_row_stride, long long qkv_row_stride, int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_store(varq_store_call(qkv, freqs_table, q_out, kv, cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q, nheads,
                                  nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype),
                  KV_PAGED | KV_DEVLEN | KV_VARQ, stream);
}

int awq_rope_kv_store_paged_varq_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, float* k_scale,
                                     float* v_scale, const int* block_table, const int* cache_seqlens, int batch, const int* cu_seqlens_q,
                                     int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim, int table_rows,
                                     int num_pages, int page_size, int pages_per_seq, long long table_row_stride, long long k_page_stride,
                                     long long k_row_stride, long long v_page_stride, long long v_row_stride, long long k_scale_page_stride,
                                     long long k_scale_row_stride, long long v_scale_page_stride, long long v_scale_row_stride,
                                     long long qkv_row_stride, int dtype, void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
                                           k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride),
                               block_table, table_row_stride, pages_per_seq);
  return kv_store(varq_store_call(qkv, freqs_table, q_out, kv, cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q, nheads,
                                  nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype),
                  KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ, stream);
}

// the four packed stores with the per-head q/k RMSNorm
int awq_rope_kv_store_natural_varq_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                          void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens, int batch, int cache_batch,
                                          const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim,
                                          int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype, void* stream) {
  return kv_store(with_qk_norm(varq_store_call(qkv, freqs_table, q_out, kv_view(k_cache, v_cache, cache_batch, lmax), cache_seqlens, table_rows,
      batch, cu_seqlens_q, max_seqlen_q, total_q, nheads, nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype), q_gamma, k_gamma, norm_eps),
      KV_DEVLEN | KV_VARQ | KV_QKNORM, stream);
}

int awq_rope_kv_store_natural_varq_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                              void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const int* cache_seqlens,
                                              int batch, int cache_batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                              int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype,
                                              void* stream) {
  return kv_store(with_qk_norm(varq_store_call(qkv, freqs_table, q_out, with_scales(kv_view(k_cache, v_cache, cache_batch, lmax), k_scale, v_scale),
      cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q, nheads, nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype), q_gamma,
      k_gamma, norm_eps), KV_FP8 | KV_DEVLEN | KV_VARQ | KV_QKNORM, stream);
}

int awq_rope_kv_store_paged_varq_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                        void* q_out, void* k_pool, void* v_pool, const int* block_table, const int* cache_seqlens, int batch,
                                        const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                        int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                        long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                        long long qkv_row_stride, int dtype, void* stream) {
  const KvView kv = with_table(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride), block_table,
      table_row_stride, pages_per_seq);
  return kv_store(with_qk_norm(varq_store_call(qkv, freqs_table, q_out, kv, cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q,
      nheads, nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype), q_gamma, k_gamma, norm_eps), KV_PAGED | KV_DEVLEN | KV_VARQ | KV_QKNORM, stream);
}

int awq_rope_kv_store_paged_varq_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                            void* q_out, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* block_table,
                                            const int* cache_seqlens, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                            int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                            long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                            long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                            long long v_scale_page_stride, long long v_scale_row_stride, long long qkv_row_stride, int dtype,
                                            void* stream) {
  const KvView kv = with_table(with_scales(kv_view(k_pool, v_pool, num_pages, page_size, k_page_stride, k_row_stride, v_page_stride, v_row_stride),
      k_scale, v_scale, k_scale_page_stride, k_scale_row_stride, v_scale_page_stride, v_scale_row_stride), block_table, table_row_stride,
      pages_per_seq);
  return kv_store(with_qk_norm(varq_store_call(qkv, freqs_table, q_out, kv, cache_seqlens, table_rows, batch, cu_seqlens_q, max_seqlen_q, total_q,
      nheads, nheads_kv, head_dim, rot_dim, qkv_row_stride, dtype), q_gamma, k_gamma, norm_eps), KV_FP8 | KV_PAGED | KV_DEVLEN | KV_VARQ | KV_QKNORM,
      stream);
}

static bool varlen_shape_ok(int nseq, int nheads, int head_dim, int max_seqlen) {
  return nseq >= 1 && nheads >= 1 && (head_dim == 64 || head_dim == 72) && max_seqlen >= 1 &&
         (long long)nseq * nheads * ((max_seqlen + 31) / 32) <= 0x7FFFFFFFll;
}

int awq_attn_varlen_plan(int nseq, int nheads, int head_dim, int max_seqlen, int* q_tile_rows, int* blocks) {
  if (!q_tile_rows || !blocks) return AWQ_ERR_NULL;
  if (!varlen_shape_ok(nseq, nheads, head_dim, max_seqlen)) return AWQ_ERR_SHAPE;
  return awq::attn_varlen_plan(nseq, nheads, head_dim, max_seqlen, q_tile_rows, blocks);
}

int awq_attn_varlen(const void* q, const void* k, const void* v, void* out, const int* cu_seqlens, int nseq, int max_seqlen,
                    long long total_rows, int nheads, int head_dim, long long q_row_stride, long long k_row_stride,
                    long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream) {
  if (!q || !k || !v || !out || !cu_seqlens) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  const long long hd = (long long)nheads * head_dim;
  if (!varlen_shape_ok(nseq, nheads, head_dim, max_seqlen) || causal != 0 || total_rows < 1 || q_row_stride < hd || k_row_stride < hd ||
      v_row_stride < hd)
    return AWQ_ERR_SHAPE;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || (q_row_stride % 8) != 0 || (k_row_stride % 8) != 0 ||
      (v_row_stride % 8) != 0 || (reinterpret_cast<uintptr_t>(cu_seqlens) & 3u))
    return AWQ_ERR_ALIGN;
  awq::launch_attn_tower(q, k, v, out, cu_seqlens, nseq, max_seqlen, max_seqlen, total_rows, nheads, nheads, head_dim, 0, q_row_stride, 0,
                         k_row_stride, 0, v_row_stride, softmax_scale, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_rope_with_pos(const void* input, const float* freqs, void* out, int n0, int n1, int nheads, int head_dim, int rot_dim,
                      long long in_stride0, long long in_stride1, long long in_stride_head, long long out_stride0, long long out_stride1,
                      long long out_stride_head, int dtype, void* stream) {
  if (!input || !freqs || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (n0 < 1 || n1 < 1 || nheads < 1 || head_dim < 8 || (head_dim % 8) != 0 || rot_dim < 16 || (rot_dim % 16) != 0 || rot_dim > head_dim ||
      in_stride0 < 0 || in_stride1 < 0 || in_stride_head < head_dim || out_stride0 < 0 || out_stride1 < 0 || out_stride_head < head_dim)
    return AWQ_ERR_SHAPE;
  if (!aligned16(input) || !aligned16(freqs) || !aligned16(out) || (in_stride0 % 8) != 0 || (in_stride1 % 8) != 0 || (in_stride_head % 8) != 0 ||
      (out_stride0 % 8) != 0 || (out_stride1 % 8) != 0 || (out_stride_head % 8) != 0)
    return AWQ_ERR_ALIGN;
  awq::launch_rope_with_pos(input, freqs, out, n0, n1, nheads, head_dim, rot_dim, in_stride0, in_stride1, in_stride_head, out_stride0,
                            out_stride1, out_stride_head, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_rope_neox_inplace(const long long* positions, void* query, void* key, const void* cos_sin_cache, int num_tokens, int nheads,
                          int head_size, int rot_dim, int max_position, int dtype, void* stream) {
  if (!positions || !query || !key || !cos_sin_cache) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (num_tokens < 1 || nheads < 1 || head_size < 16 || (head_size % 8) != 0 || rot_dim < 16 || (rot_dim % 16) != 0 || rot_dim > head_size ||
      max_position < 1)
    return AWQ_ERR_SHAPE;
  if (!aligned16(query) || !aligned16(key) || !aligned16(cos_sin_cache) || (reinterpret_cast<uintptr_t>(positions) & 7u)) return AWQ_ERR_ALIGN;
  awq::launch_rope_neox(positions, query, key, cos_sin_cache, num_tokens, nheads, head_size, rot_dim, max_position, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_w8a8_gemm_plan(int m, int n, int k, int* tile_m, int* tile_n) { return awq::w8a8_gemm_plan(m, n, k, tile_m, tile_n); }

int awq_w8a8_gemm(const void* x, const void* w, const void* wscales, const void* ascales, const void* bias, void* out, int m, int n, int k,
                  void* stream) {
  if (!x || !w || !wscales || !ascales || !out) return AWQ_ERR_NULL;
  if (awq::w8a8_gemm_plan(m, n, k, nullptr, nullptr) == 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(w) || !aligned16(wscales) || !aligned16(ascales) || !aligned16(out) || (bias && !aligned16(bias)))
    return AWQ_ERR_ALIGN;
  if (awq::launch_w8a8_gemm(x, w, wscales, ascales, bias, out, m, n, k, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_quant_per_token(const void* x, void* out_i8, void* scale, int m, int k, int dtype, void* stream) {
  if (!x || !out_i8 || !scale) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1 || k < 8 || (k % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(out_i8) || !aligned16(scale)) return AWQ_ERR_ALIGN;
  awq::launch_quant_per_token(x, out_i8, scale, m, k, dtype, (hipStream_t)stream);
  return finish_launch();
}

int awq_gelu_quant_per_token(const void* x, void* out_i8, void* scale, void* tmp, int m, int k, void* stream) {
  if (!x || !out_i8 || !scale || !tmp) return AWQ_ERR_NULL;
  if (m < 1 || k < 8 || (k % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(out_i8) || !aligned16(scale) || !aligned16(tmp)) return AWQ_ERR_ALIGN;
  awq::launch_gelu_quant_per_token(x, out_i8, scale, tmp, m, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_layernorm_quant(const void* x, const void* gamma, const void* beta, float eps, void* out_i8, void* scale, int m, int k, int per_token,
                        int dtype, void* stream) {
  if (!x || !gamma || !out_i8 || !scale) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1 || k < 8 || (k % 8) != 0 || k > 16384) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(gamma) || (beta && !aligned16(beta)) || !aligned16(out_i8) || !aligned16(scale)) return AWQ_ERR_ALIGN;
  if (awq::launch_layernorm_quant(x, gamma, beta, eps, out_i8, scale, m, k, per_token ? 1 : 0, dtype, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// The scratch a caller of the forward entries should bring: the largest any leaf of its row class can use -- NOT always what the routed leaf uses: the first row
// speaks for the mid-M kernel whenever midm_takes accepts the shape, also where a forward row in front of it decides (no sz_packed: the generic kernels;
// gemm_variant != 0), and the third for the tile kernels on calls launch_gemm keeps on its generic kernels.  Pinned by tests/linear_route_cases.py.
size_t awq_w4a16_forward_cdna4_workspace_bytes(int m, int n, int k) {
  if (awq::midm_takes(m, n, k)) return awq::midm_workspace_bytes(m, n, k);  // 9 .. 255 rows: the fp32 parts of the mid-M kernel's K split
  if (m > 8 && m < 256 && !awq::gemm_cdna4_v3_takes(m, k)) return awq::skinny_splitk_workspace_bytes(m, n, k);  // (knob midm = 0) the skinny launch's K split
  return awq::gemm_cdna4_v3_workspace_bytes(m, n, k);
}
// The route of a call of entry `entry` (LinearEntry) with pointer facts `flags` (LinearFlags): returns the leaf (LinearLeaf; 0 = the entry refuses the arguments or
// no launcher serves them) and writes leaf, scale format, epilogue, bias handling, workspace handed on, bias read as 16-byte vectors, deciding row, 0
int awq_w4a16_linear_route_cdna4(int entry, int m, int n, int k, int flags, int out[8]) {
  if (entry < awq::kEntryForward || entry > awq::kEntryPartial || flags < 0 || flags > 31 || m < 1 || n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) return 0;
  if ((entry == awq::kEntryGemv && m > 16) || (entry == awq::kEntryGateUp && (size_t)m * (size_t)k >= (1ull << 31))) return 0;
  const awq::LinearRoute r = awq::linear_route(entry, m, n, k, flags, awq::device_cu_count(), awq::g_linear);
  const int w[8] = {r.leaf, r.szfmt, r.epilogue, r.bias, r.ws ? 1 : 0, r.bias_align16 ? 1 : 0, r.row, 0};
  for (int i = 0; out != nullptr && r.leaf != awq::kLeafNone && i < 8; ++i) out[i] = w[i];
  return r.leaf;
}
int awq_midm_init(void) { return awq::midm_init() == 0 ? AWQ_OK : AWQ_ERR_LAUNCH; }
int awq_w4a16_gemm_cdna4_pair_plan(int m, int n, int k) { return awq::gemm_cdna4_v3_pair_plan(m, n, k); }
int awq_w4a16_gemm_cdna4_pair_lost(unsigned int* count) { return awq::gemm_v6_pair_lost(count) == 0 ? AWQ_OK : AWQ_ERR_LAUNCH; }
int awq_w4a16_gemm_cdna4_plan(int m, int n, int bits, int* mode, int* cols_main) { return awq::gemm_cdna4_v3_plan(m, n, bits, mode, cols_main); }
int awq_w4a16_gemm_cdna4_narrow_kernel(int m, int n_cols, int k, int bits, int has_workspace, int epilogue) {
  return awq::gemm_cdna4_v3_narrow_kernel(m, n_cols, k, bits, has_workspace, epilogue);
}
int awq_w4a16_decode_cdna4_plan(int m, int n, int k, int epilogue, int* kernel) { return awq::gemv_dma_plan(m, n, k, epilogue, kernel); }
int awq_w4a16_decode_cdna4_plan_detail(int m, int n, int k, int epilogue, int chunk, int out[8]) { return awq::gemv_dma_plan_detail(m, n, k, epilogue, chunk, out); }

int awq_w4a16_gemm_cdna4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                         const void* sz_packed, void* out, int m, int n, int k, int group_size, int dtype, void* workspace,
                         size_t workspace_bytes, void* stream) {
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if ((n % 16) != 0) return AWQ_ERR_SHAPE;
  return launch_routed(awq::kEntryGemm, x, qweight, scales, scaled_zeros, sz_packed, nullptr, nullptr, out, m, n, k, dtype, workspace, workspace_bytes,
                       route_flags(sz_packed, nullptr, nullptr, workspace), (hipStream_t)stream);
}

int awq_w4a16_forward_cdna4_szh(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, const void* sz_packed,
                                const void* sz_half, const void* bias, void* out, int m, int n, int k, int group_size, int dtype, void* workspace,
                                size_t workspace_bytes, void* stream) {
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if ((n % 16) != 0) return AWQ_ERR_SHAPE;
  return launch_routed(awq::kEntryForwardSzh, x, qweight, scales, scaled_zeros, sz_packed, sz_half, bias, out, m, n, k, dtype, workspace, workspace_bytes,
                       route_flags(sz_packed, aligned16(sz_half) ? sz_half : nullptr, bias, workspace), (hipStream_t)stream);  // (a misaligned sz_half: the sz_packed path)
}

int awq_w4a16_forward_cdna4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                            const void* sz_packed, const void* bias, void* out, int m, int n, int k, int group_size,
                            int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  int st = check_common(x, qweight, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if ((n % 16) != 0) return AWQ_ERR_SHAPE;
  return launch_routed(awq::kEntryForward, x, qweight, scales, scaled_zeros, sz_packed, nullptr, bias, out, m, n, k, dtype, workspace, workspace_bytes,
                       route_flags(sz_packed, nullptr, bias, workspace), (hipStream_t)stream);
}

// ---- tensor-parallel row split: the K shard's fp32 partial + the single rounding after the sum ----
int awq_w4a16_partial_cdna4(const void* x, const void* qweight, const void* sz_packed, const void* sz_half, float* out_f32, int m, int n, int k,
                            int group_size, int dtype, void* stream) {
  if (!x || !qweight || !sz_packed || !out_f32) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (m < 1 || n < 16 || k < 128 || (n % 16) != 0 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight) || !aligned16(out_f32) || !aligned16(sz_packed) || !aligned16(sz_half)) return AWQ_ERR_ALIGN;
  return launch_routed(awq::kEntryPartial, x, qweight, nullptr, nullptr, sz_packed, sz_half, nullptr, out_f32, m, n, k, dtype, nullptr, 0, route_flags(sz_packed, sz_half, nullptr, nullptr),
                       (hipStream_t)stream);
}

int awq_round_bias_f32(const float* in_f32, const void* bias, void* out, int m, int n, int dtype, void* stream) {
  if (!in_f32 || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (!aligned16(in_f32) || !aligned16(out) || !aligned16(bias)) return AWQ_ERR_ALIGN;
  if (awq::launch_round_bias_f32(in_f32, bias, out, m, n, dtype, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_w4a16_moe_gemm(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* expert_offsets, void* out, int total_tokens, int num_experts, int n, int k, int gpad,
                       int group_size, int dtype, int layout, void* stream) {
  if (!expert_offsets) return AWQ_ERR_NULL;
  if (num_experts < 1 || gpad * 128 < k || total_tokens < 0) return AWQ_ERR_SHAPE;
  if (layout != 0 && layout != 1) return AWQ_ERR_SHAPE;
  if (layout == 1 && (n % 16) != 0) return AWQ_ERR_SHAPE;
  if (total_tokens == 0) return AWQ_OK;
  int st = check_common(x_sorted, qweight, scales, scaled_zeros, out, total_tokens, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  awq::launch_moe_gemm(x_sorted, qweight, scales, scaled_zeros, expert_offsets, out, total_tokens, num_experts, n, k, gpad,
                       dtype, layout, (hipStream_t)stream);
  return finish_launch();
}

int awq_w4a16_moe_forward_cdna4(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros,
                                const void* sz_packed, const void* expert_offsets, void* out, int total_tokens,
                                int num_experts, int n, int k, int gpad, int group_size, int dtype, void* stream) {
  return awq_w4a16_moe_forward_cdna4_szh(x_sorted, qweight, scales, scaled_zeros, sz_packed, nullptr, expert_offsets, out, total_tokens, num_experts, n, k, gpad,
                                         group_size, dtype, stream);
}

int awq_w4a16_moe_forward_cdna4_szh(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros, const void* sz_packed,
                                    const void* sz_half, const void* expert_offsets, void* out, int total_tokens, int num_experts, int n, int k,
                                    int gpad, int group_size, int dtype, void* stream) {
  if (!expert_offsets || !sz_packed) return AWQ_ERR_NULL;
  if (sz_half && !aligned16(sz_half)) return AWQ_ERR_ALIGN;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (num_experts < 1 || gpad * 128 < k || total_tokens < 0 || (n % 16) != 0) return AWQ_ERR_SHAPE;
  if (total_tokens == 0) return AWQ_OK;
  int st = check_common(x_sorted, qweight, scales, scaled_zeros, out, total_tokens, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if (total_tokens <= 8 && awq::launch_moe_gemv_cdna4(x_sorted, qweight, sz_packed, expert_offsets, out, total_tokens, num_experts, n,
                                                      k, dtype, (hipStream_t)stream) == 0)
    return finish_launch();
  if (total_tokens > 8 && total_tokens < 256 && awq::moe_v4_enabled() &&
      awq::launch_moe_skinny_cdna4(x_sorted, qweight, sz_packed, expert_offsets, out, total_tokens, num_experts, n, k, dtype,
                                   (hipStream_t)stream) == 0)
    return finish_launch();
  if (total_tokens >= 256 && awq::moe_v6_enabled() && awq::moe_v4_enabled() &&
      awq::launch_moe_gemm_cdna4_v6(x_sorted, qweight, sz_packed, expert_offsets, out, total_tokens, num_experts, n, k, dtype,
                                    (hipStream_t)stream, 0, sz_half) == 0)
    return finish_launch();
  awq::launch_moe_gemm(x_sorted, qweight, scales, scaled_zeros, expert_offsets, out, total_tokens, num_experts, n, k, gpad, dtype, 1,
                       (hipStream_t)stream);
  return finish_launch();
}

int awq_silu_mul(const void* gate, const void* up, void* out, size_t count, int dtype, void* stream) {
  if (!gate || !up || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (!aligned16(gate) || !aligned16(up) || !aligned16(out)) return AWQ_ERR_ALIGN;
  if (count == 0) return AWQ_OK;
  if (awq::launch_silu_mul(gate, up, out, count, dtype, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_w4a16_moe_mlp_gate_up_cdna4(const void* x_sorted, const void* qweight_interleaved, const void* scales, const void* scaled_zeros,
                                    const void* sz_packed, const void* expert_offsets, void* out, void* scratch, size_t scratch_bytes,
                                    int total_tokens, int num_experts, int n2, int k, int gpad, int group_size, int dtype, void* stream) {
  return awq_w4a16_moe_mlp_gate_up_cdna4_szh(x_sorted, qweight_interleaved, scales, scaled_zeros, sz_packed, nullptr, expert_offsets, out, scratch, scratch_bytes,
                                             total_tokens, num_experts, n2, k, gpad, group_size, dtype, stream);
}

int awq_w4a16_moe_mlp_gate_up_cdna4_szh(const void* x_sorted, const void* qweight_interleaved, const void* scales, const void* scaled_zeros,
                                        const void* sz_packed, const void* sz_half, const void* expert_offsets, void* out, void* scratch,
                                        size_t scratch_bytes, int total_tokens, int num_experts, int n2, int k, int gpad, int group_size, int dtype,
                                        void* stream) {
  if (!expert_offsets || !sz_packed || !x_sorted || !qweight_interleaved || !out) return AWQ_ERR_NULL;
  if (sz_half && !aligned16(sz_half)) return AWQ_ERR_ALIGN;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (num_experts < 1 || total_tokens < 0 || n2 < 32 || (n2 % 32) != 0 || k < 128 || (k % 128) != 0) return AWQ_ERR_SHAPE;
  if (total_tokens == 0) return AWQ_OK;
  if (!aligned16(x_sorted) || !aligned16(qweight_interleaved) || !aligned16(out) || !aligned16(sz_packed) || !aligned16(scratch)) return AWQ_ERR_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  if (total_tokens >= 256 && awq::moe_v6_enabled() &&
      awq::launch_moe_gemm_cdna4_v6(x_sorted, qweight_interleaved, sz_packed, expert_offsets, out, total_tokens, num_experts, n2, k, dtype, st, 2, sz_half) == 0)
    return finish_launch();
  // fewer than 256 sorted rows (grouped GEMV / grouped skinny kernel) -- or the v6 tile switched off: the pair's [total, n2] product goes
  // through the caller's scratch, then the SiLU * mul tail as its own launch
  if (!scratch || scratch_bytes < (size_t)total_tokens * n2 * 2) return AWQ_ERR_WORKSPACE;
  const int rc = awq_w4a16_moe_forward_cdna4(x_sorted, qweight_interleaved, scales, scaled_zeros, sz_packed, expert_offsets, scratch, total_tokens,
                                             num_experts, n2, k, gpad, group_size, dtype, stream);
  if (rc != AWQ_OK) return rc;
  if (awq::launch_silu_mul_interleaved(scratch, out, total_tokens, n2, dtype, st) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- MoE routing on the device (awq_moe_route_cdna4.hip) ----
static int check_moe_sizes(int tokens, int num_experts, int top_k) {
  if (num_experts < 1 || num_experts > 64 || top_k < 1 || top_k > 8 || top_k > num_experts || tokens < 1 || (long long)tokens * top_k > (1ll << 20))
    return AWQ_ERR_SHAPE;
  return AWQ_OK;
}
static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int awq_moe_route(const void* router_logits, int logits_dtype, int tokens, int num_experts, int top_k, int renormalize, void* topk_ids,
                  void* topk_w, void* order, void* inv, void* offsets, void* stream) {
  if (!router_logits || !topk_ids || !topk_w || !order || !inv || !offsets) return AWQ_ERR_NULL;
  if (logits_dtype != AWQ_F16 && logits_dtype != AWQ_BF16 && logits_dtype != AWQ_F32) return AWQ_ERR_DTYPE;
  if (check_moe_sizes(tokens, num_experts, top_k)) return AWQ_ERR_SHAPE;
  if (!aligned_to(router_logits, logits_dtype == AWQ_F32 ? 4 : 2) || !aligned_to(topk_ids, 4) || !aligned_to(topk_w, 4) || !aligned_to(order, 4) ||
      !aligned_to(inv, 4) || !aligned_to(offsets, 4))
    return AWQ_ERR_ALIGN;
  if (awq::launch_moe_route(router_logits, logits_dtype, tokens, num_experts, top_k, renormalize, topk_ids, topk_w, order, inv, offsets,
                            (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_moe_gather(const void* x, const void* order, void* xs, int tokens, int top_k, int hidden, int dtype, void* stream) {
  if (!x || !order || !xs) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (check_moe_sizes(tokens, 64, top_k) || hidden < 8 || (hidden % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(xs) || !aligned_to(order, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_moe_gather(x, order, xs, tokens, top_k, hidden, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_moe_combine(const void* ys, const void* inv, const void* topk_w, void* out, int tokens, int top_k, int hidden, int dtype, void* stream) {
  if (!ys || !inv || !topk_w || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (check_moe_sizes(tokens, 64, top_k) || hidden < 8 || (hidden % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(ys) || !aligned16(out) || !aligned_to(inv, 4) || !aligned_to(topk_w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_moe_combine(ys, inv, topk_w, out, tokens, top_k, hidden, dtype, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- next-token sampling on the device (awq_sample_cdna4.hip) ----
int awq_sample_logits(const void* logits, int logits_dtype, int batch, int vocab, const void* u, const void* temperature, const void* top_k,
                      const void* top_p, const void* repetition_penalty, void* history, void* hist_len, int max_history, void* seqlens,
                      const void* stop_ids, int num_stop, void* finished, int max_len, int flags, void* tokens, void* stream) {
  if (!logits || !u || !tokens) return AWQ_ERR_NULL;
  if ((history != nullptr) != (hist_len != nullptr)) return AWQ_ERR_NULL;  // a history comes with its lengths
  if ((flags & AWQ_SAMPLE_APPEND) && !history) return AWQ_ERR_NULL;
  if ((flags & AWQ_SAMPLE_ADVANCE) && !seqlens) return AWQ_ERR_NULL;
  if (num_stop > 0 && !stop_ids) return AWQ_ERR_NULL;
  if (logits_dtype != AWQ_F16 && logits_dtype != AWQ_BF16 && logits_dtype != AWQ_F32) return AWQ_ERR_DTYPE;
  if (batch < 1 || vocab < 1 || vocab > (1 << 20) || (history && max_history < 1) || num_stop < 0 || (flags & ~3)) return AWQ_ERR_SHAPE;
  if (!aligned_to(logits, logits_dtype == AWQ_F32 ? 4 : 2)) return AWQ_ERR_ALIGN;  // rows are walked from the 16-byte boundary below them
  const void* words[] = {u, temperature, top_k, top_p, repetition_penalty, history, hist_len, seqlens, stop_ids, finished, tokens};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_sample_logits(logits, logits_dtype, batch, vocab, u, temperature, top_k, top_p, repetition_penalty, history, hist_len, max_history,
                                seqlens, stop_ids, num_stop, finished, max_len, flags, tokens, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- prompt-lookup speculative decoding on the device (awq_spec_cdna4.hip) ----
int awq_spec_draft_ngram(const void* history, const void* hist_len, const void* seqlens, const void* max_draft, void* drafts, void* draft_len,
                         int batch, int max_history, int vocab, int kmax, int ngram_min, int ngram_max, int max_len, void* stream) {
  if (!history || !hist_len || !seqlens || !draft_len || (kmax > 0 && !drafts)) return AWQ_ERR_NULL;
  if (batch < 1 || max_history < 1 || vocab < 1 || kmax < 0 || kmax > 15 || ngram_min < 1 || ngram_min > ngram_max || ngram_max > 8)
    return AWQ_ERR_SHAPE;
  const void* words[] = {history, hist_len, seqlens, max_draft, drafts, draft_len};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_spec_draft_ngram(history, hist_len, seqlens, max_draft, drafts, draft_len, batch, max_history, vocab, kmax, ngram_min, ngram_max,
                                   max_len, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_spec_pack(const void* last_tokens, void* drafts, void* draft_len, const void* seqlens, void* cu_seqlens_q, void* input_ids, int batch,
                  int kmax, int total_q, void* stream) {
  if (!last_tokens || !draft_len || !seqlens || !cu_seqlens_q || !input_ids || (kmax > 0 && !drafts)) return AWQ_ERR_NULL;
  if (batch < 1 || batch > 65535 || kmax < 0 || kmax > 15 || total_q < batch) return AWQ_ERR_SHAPE;
  const void* words[] = {last_tokens, drafts, draft_len, seqlens, cu_seqlens_q, input_ids};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_spec_pack(last_tokens, drafts, draft_len, seqlens, cu_seqlens_q, input_ids, batch, kmax, total_q, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_spec_verify(const void* logits, int logits_dtype, int total_q, int vocab, const void* u, const void* cu_seqlens_q, const void* input_ids,
                    int batch, const void* temperature, const void* top_k, const void* top_p, const void* repetition_penalty, const void* history,
                    const void* hist_len, int max_history, void* row_tokens, void* stream) {
  if (!logits || !u || !cu_seqlens_q || !input_ids || !row_tokens) return AWQ_ERR_NULL;
  if ((history != nullptr) != (hist_len != nullptr)) return AWQ_ERR_NULL;  // a history comes with its lengths
  if (logits_dtype != AWQ_F16 && logits_dtype != AWQ_BF16 && logits_dtype != AWQ_F32) return AWQ_ERR_DTYPE;
  if (total_q < 1 || batch < 1 || batch > 65535 || vocab < 1 || vocab > (1 << 20) || (history && max_history < 1)) return AWQ_ERR_SHAPE;
  if (!aligned_to(logits, logits_dtype == AWQ_F32 ? 4 : 2)) return AWQ_ERR_ALIGN;  // rows are walked from the 16-byte boundary below them
  const void* words[] = {u, cu_seqlens_q, input_ids, temperature, top_k, top_p, repetition_penalty, history, hist_len, row_tokens};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_spec_verify(logits, logits_dtype, total_q, vocab, u, cu_seqlens_q, input_ids, batch, temperature, top_k, top_p, repetition_penalty,
                              history, hist_len, max_history, row_tokens, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_spec_accept(const void* row_tokens, const void* input_ids, const void* cu_seqlens_q, int batch, int total_q, int kmax, void* history,
                    void* hist_len, int max_history, void* seqlens, const void* stop_ids, int num_stop, void* finished, int max_len, int flags,
                    void* out_tokens, void* num_emitted, void* last_tokens, void* stream) {
  if (!row_tokens || !input_ids || !cu_seqlens_q || !out_tokens || !num_emitted || !last_tokens) return AWQ_ERR_NULL;
  if ((history != nullptr) != (hist_len != nullptr)) return AWQ_ERR_NULL;  // a history comes with its lengths
  if ((flags & AWQ_SAMPLE_APPEND) && !history) return AWQ_ERR_NULL;
  if ((flags & AWQ_SAMPLE_ADVANCE) && !seqlens) return AWQ_ERR_NULL;
  if (num_stop > 0 && !stop_ids) return AWQ_ERR_NULL;
  if (batch < 1 || batch > 65535 || total_q < 1 || kmax < 0 || kmax > 15 || (history && max_history < 1) || num_stop < 0 || (flags & ~3))
    return AWQ_ERR_SHAPE;
  const void* words[] = {row_tokens, input_ids, cu_seqlens_q, history, hist_len, seqlens, stop_ids, finished, out_tokens, num_emitted, last_tokens};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_spec_accept(row_tokens, input_ids, cu_seqlens_q, batch, total_q, kmax, history, hist_len, max_history, seqlens, stop_ids, num_stop,
                              finished, max_len, flags, out_tokens, num_emitted, last_tokens, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// a cap (awq_softcap.hpp): 0 is none, anything else finite and positive; the comparison refuses a NaN
static bool softcap_ok(float cap) { return cap >= 0.f && cap <= 3.4028234663852886e38f; }

// ---- LM head for decode and the token embedding gather (awq_lm_head_cdna4.hip) ----
int awq_lm_head(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                int out_dtype, int m, int v, int k, int dtype, int max_blocks, void* stream) {
  return awq_lm_head_softcap(x, ldx, gamma, eps, weight, bias, seqlens, out, out_dtype, m, v, k, dtype, 0.f, max_blocks, stream);
}

// softcap = 0 is awq_lm_head: the same checks, the same kernels
int awq_lm_head_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                        int out_dtype, int m, int v, int k, int dtype, float softcap, int max_blocks, void* stream) {
  if (!x || !weight || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (out_dtype != AWQ_F32 && out_dtype != dtype) return AWQ_ERR_DTYPE;
  if (m < 1 || m > 64) return AWQ_ERR_BATCH;
  if (v < 1 || k < 8 || (k % 8) != 0 || ldx < k || (ldx % 8) != 0 || max_blocks < 0 || !softcap_ok(softcap)) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(weight) || !aligned16(out) || !aligned16(gamma) || !aligned16(bias) || !aligned_to(seqlens, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_lm_head_softcap(x, ldx, gamma, eps, weight, bias, seqlens, out, out_dtype == AWQ_F32 ? 1 : 0, m, v, k, dtype, softcap, max_blocks,
                                  (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_lm_head_plan(int m, int v, int k, int out[4]) {
  if (!out) return AWQ_ERR_NULL;
  if (m < 1 || m > 64) return AWQ_ERR_BATCH;
  return awq::lm_head_plan(m, v, k, out) != 0 ? AWQ_ERR_SHAPE : AWQ_OK;
}

int awq_embed_tokens(const int* tokens, const void* table, void* out, int n, int v, int k, int dtype, void* stream) {
  if (!tokens || !table || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (n < 1 || v < 1 || k < 8 || (k % 8) != 0) return AWQ_ERR_SHAPE;
  if (!aligned16(table) || !aligned16(out) || !aligned_to(tokens, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_embed_tokens(tokens, table, out, n, v, k, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- Token log-probabilities: LM head fused with log-sum-exp, and the companion for existing logits (awq_lm_logprobs_cdna4.hip) ----
int awq_lm_head_logprobs_plan(int t, int v, int k, int out[4]) {
  if (!out) return AWQ_ERR_NULL;
  return awq::lm_logprobs_plan(t, v, k, out) != 0 ? AWQ_ERR_SHAPE : AWQ_OK;
}

size_t awq_lm_head_logprobs_workspace_bytes(int t, int v, int k, int with_gamma) { return awq::lm_logprobs_workspace_bytes(t, v, k, with_gamma); }

int awq_lm_head_logprobs(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                         float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                         void* workspace, size_t workspace_bytes, int max_blocks, void* stream) {
  return awq_lm_head_logprobs_softcap(x, ldx, gamma, eps, weight, bias, targets, logprob, lse, target_logit, argmax, t, v, k, dtype, round_logits, 0.f,
                                      workspace, workspace_bytes, max_blocks, stream);
}

// softcap = 0 is awq_lm_head_logprobs: the same checks, the same kernels
int awq_lm_head_logprobs_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                                 float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                                 float softcap, void* workspace, size_t workspace_bytes, int max_blocks, void* stream) {
  if (!x || !weight) return AWQ_ERR_NULL;
  if (!targets && (logprob || target_logit)) return AWQ_ERR_NULL;  // without targets there is no target logit to report
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  int plan[4];
  if (awq::lm_logprobs_plan(t, v, k, plan) != 0 || ldx < k || (ldx % 8) != 0 || max_blocks < 0 || (gamma && ldx != k) || !softcap_ok(softcap))
    return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(weight) || !aligned16(gamma) || !aligned16(bias) || !aligned16(workspace)) return AWQ_ERR_ALIGN;
  const void* words[] = {targets, logprob, lse, target_logit, argmax};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (!workspace || workspace_bytes < awq::lm_logprobs_workspace_bytes(t, v, k, gamma != nullptr)) return AWQ_ERR_WORKSPACE;
  if (awq::launch_lm_logprobs_softcap(x, ldx, gamma, eps, weight, bias, targets, logprob, lse, target_logit, argmax, t, v, k, dtype, round_logits,
                                      softcap, workspace, max_blocks, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_token_logprobs(const void* logits, int logits_dtype, long ld, const int* targets, float* logprob, float* lse, int* argmax, int b, int v,
                       void* stream) {
  if (!logits) return AWQ_ERR_NULL;
  if (!targets && logprob) return AWQ_ERR_NULL;
  if (logits_dtype != AWQ_F16 && logits_dtype != AWQ_BF16 && logits_dtype != AWQ_F32) return AWQ_ERR_DTYPE;
  if (b < 1 || b > 65535 * 1024 || v < 1 || v > (1 << 30) || ld < v) return AWQ_ERR_SHAPE;
  if (!aligned_to(logits, logits_dtype == AWQ_F32 ? 4 : 2)) return AWQ_ERR_ALIGN;
  const void* words[] = {targets, logprob, lse, argmax};
  for (const void* w : words)
    if (!aligned_to(w, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_token_logprobs(logits, logits_dtype, ld, targets, logprob, lse, argmax, b, v, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// logits that already exist, capped in place (awq_util.hip).  softcap = 0 is "no cap": nothing is launched and the logits keep their bits
int awq_logit_softcap(void* logits, int logits_dtype, long ld, const int* seqlens, int b, int v, float softcap, void* stream) {
  if (!logits) return AWQ_ERR_NULL;
  if (logits_dtype != AWQ_F16 && logits_dtype != AWQ_BF16 && logits_dtype != AWQ_F32) return AWQ_ERR_DTYPE;
  if (b < 1 || b > 65535 * 1024 || v < 1 || v > (1 << 30) || ld < v || !softcap_ok(softcap)) return AWQ_ERR_SHAPE;
  if (!aligned_to(logits, logits_dtype == AWQ_F32 ? 4 : 2) || !aligned_to(seqlens, 4)) return AWQ_ERR_ALIGN;
  if (softcap == 0.f) return AWQ_OK;
  if (awq::launch_logit_softcap(logits, logits_dtype, ld, seqlens, b, v, softcap, (hipStream_t)stream) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- Multi-LoRA on packed steps: shrink + expand (awq_lora_cdna4.hip) ----
static int lora_check_batch(const int* cu_seqlens_q, int batch, int max_seqlen_q, int total_q, int slots) {
  if (batch < 1 || batch > 65535 || max_seqlen_q < 1 || max_seqlen_q > 1048560 || total_q < 1 || slots < 1) return AWQ_ERR_BATCH;
  if (!cu_seqlens_q && (long long)batch * max_seqlen_q != (long long)total_q) return AWQ_ERR_BATCH;  // rectangular: every row is owned
  return AWQ_OK;
}

int awq_lora_plan(int k, int r, int n_slices, int out[4]) {
  if (!out) return AWQ_ERR_NULL;
  return awq::lora_plan(k, r, n_slices, out) != 0 ? AWQ_ERR_SHAPE : AWQ_OK;
}

size_t awq_lora_workspace_bytes(int total_q, int k, int r, int n_slices) { return awq::lora_workspace_bytes(total_q, k, r, n_slices); }

int awq_lora_shrink(const void* x, long ldx, const void* a_pool, const int* adapter_ids, const int* cu_seqlens_q, void* workspace,
                    size_t workspace_bytes, int batch, int max_seqlen_q, int total_q, int slots, int k, int r, int n_slices, int dtype, void* stream) {
  if (!x || !a_pool || !adapter_ids || !workspace) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  int plan[4];
  if (awq::lora_plan(k, r, n_slices, plan) != 0 || ldx < k || (ldx % 8) != 0) return AWQ_ERR_SHAPE;
  if (const int st = lora_check_batch(cu_seqlens_q, batch, max_seqlen_q, total_q, slots)) return st;
  if (workspace_bytes < awq::lora_workspace_bytes(total_q, k, r, n_slices)) return AWQ_ERR_WORKSPACE;
  if (!aligned16(x) || !aligned16(a_pool) || !aligned16(workspace) || !aligned_to(adapter_ids, 4) || !aligned_to(cu_seqlens_q, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_lora_shrink(x, ldx, a_pool, adapter_ids, cu_seqlens_q, workspace, batch, max_seqlen_q, total_q, slots, k, r, n_slices, dtype,
                              (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_lora_expand(const void* workspace, size_t workspace_bytes, const void* b_pool, const float* scaling, const int* adapter_ids,
                    const int* cu_seqlens_q, void* y, int batch, int max_seqlen_q, int total_q, int slots, int n, int k, int r, const int* slice_end,
                    int n_slices, int dtype, void* stream) {
  if (!workspace || !b_pool || !scaling || !adapter_ids || !y || !slice_end) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  int plan[4];
  if (awq::lora_plan(k, r, n_slices, plan) != 0 || n < 16 || (n % 16) != 0) return AWQ_ERR_SHAPE;
  for (int j = 0, prev = 0; j < n_slices; prev = slice_end[j++])
    if (slice_end[j] <= prev || (slice_end[j] % 16) != 0 || slice_end[j] > n) return AWQ_ERR_SHAPE;
  if (slice_end[n_slices - 1] != n) return AWQ_ERR_SHAPE;
  if (const int st = lora_check_batch(cu_seqlens_q, batch, max_seqlen_q, total_q, slots)) return st;
  if (workspace_bytes < awq::lora_workspace_bytes(total_q, k, r, n_slices)) return AWQ_ERR_WORKSPACE;
  if (!aligned16(workspace) || !aligned16(b_pool) || !aligned16(y) || !aligned_to(scaling, 4) || !aligned_to(adapter_ids, 4) ||
      !aligned_to(cu_seqlens_q, 4))
    return AWQ_ERR_ALIGN;
  if (awq::launch_lora_expand(workspace, b_pool, scaling, adapter_ids, cu_seqlens_q, y, batch, max_seqlen_q, total_q, slots, n, k, r, slice_end,
                              n_slices, dtype, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_lora_expand_gate_up(const void* workspace, size_t workspace_bytes, const void* b_pool, const float* scaling, const int* adapter_ids,
                            const int* cu_seqlens_q, const void* y2, void* h, int batch, int max_seqlen_q, int total_q, int slots, int n2, int k,
                            int r, int dtype, void* stream) {
  if (!workspace || !b_pool || !scaling || !adapter_ids || !y2 || !h) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  int plan[4];
  if (awq::lora_plan(k, r, 2, plan) != 0 || n2 < 16 || (n2 % 16) != 0) return AWQ_ERR_SHAPE;
  if (const int st = lora_check_batch(cu_seqlens_q, batch, max_seqlen_q, total_q, slots)) return st;
  if (workspace_bytes < awq::lora_workspace_bytes(total_q, k, r, 2)) return AWQ_ERR_WORKSPACE;
  if (!aligned16(workspace) || !aligned16(b_pool) || !aligned16(y2) || !aligned16(h) || !aligned_to(scaling, 4) || !aligned_to(adapter_ids, 4) ||
      !aligned_to(cu_seqlens_q, 4))
    return AWQ_ERR_ALIGN;
  if (awq::launch_lora_expand_gate_up(workspace, b_pool, scaling, adapter_ids, cu_seqlens_q, y2, h, batch, max_seqlen_q, total_q, slots, n2, k, r,
                                      dtype, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- AWQ quantisation: group quantiser + packer, clip search (awq_quant_cdna4.hip) ----
int awq_quantize_group(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                       void* zeros, void* qweight, int qweight_layout, int n, int k, int group_size, int n_bit, int dtype, void* stream) {
  if (!w) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (n_bit != 3 && n_bit != 4) return AWQ_ERR_BITS;
  if (n < 1 || k < 128 || (k % 128) != 0 || ldw < k || (ldw % 8) != 0) return AWQ_ERR_SHAPE;
  if (qweight) {
    if (n_bit != 4) return AWQ_ERR_BITS;  // a packed 3-bit (w3c) output is not produced here
    if (qweight_layout != AWQ_QWEIGHT_V2 && qweight_layout != AWQ_QWEIGHT_CDNA4) return AWQ_ERR_SHAPE;
    if ((n % (qweight_layout == AWQ_QWEIGHT_CDNA4 ? 16 : 8)) != 0) return AWQ_ERR_SHAPE;
  }
  if (!aligned16(w) || !aligned16(col_scale) || !aligned16(w_fake) || !aligned16(qweight) || !aligned_to(clip_max, 2) || !aligned_to(scales, 2) ||
      !aligned_to(scaled_zeros, 2) || !aligned_to(zeros, 2))
    return AWQ_ERR_ALIGN;
  if (awq::launch_quantize_group(w, ldw, col_scale, clip_max, w_fake, scales, scaled_zeros, zeros, qweight, qweight_layout, n, k, n_bit, dtype,
                                 (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_quantize_group_host(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                            void* zeros, void* intweight, int n, int k, int group_size, int n_bit, int dtype) {
  if (!w) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (n_bit != 3 && n_bit != 4) return AWQ_ERR_BITS;
  if (n < 1 || k < 128 || (k % 128) != 0 || ldw < k) return AWQ_ERR_SHAPE;
  awq::quantize_group_host(w, ldw, col_scale, clip_max, w_fake, scales, scaled_zeros, zeros, intweight, n, k, n_bit, dtype);
  return AWQ_OK;
}

int awq_clip_search(const void* w, long ldw, const void* x, long ldx, void* best_max_val, int* best_idx, float* err, int n, int k, int s,
                    int group_size, int n_bit, int n_grid, int n_steps, int dtype, void* stream) {
  if (!w || !x || !best_max_val || !best_idx) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (n_bit != 3 && n_bit != 4) return AWQ_ERR_BITS;
  if (n < 1 || s < 1 || k < 128 || (k % 128) != 0 || ldw < k || (ldw % 8) != 0 || ldx < k || (ldx % 8) != 0 || n_grid < 1 || n_steps < 1 ||
      n_steps > 16)
    return AWQ_ERR_SHAPE;
  if (!aligned16(w) || !aligned16(x) || !aligned_to(best_max_val, 2) || !aligned_to(best_idx, 4) || !aligned_to(err, 4)) return AWQ_ERR_ALIGN;
  if (awq::launch_clip_search(w, ldw, x, ldx, best_max_val, best_idx, err, n, k, s, n_bit, n_grid, n_steps, dtype, (hipStream_t)stream) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// ---- W3 ("w3c") : the repository's 3-bit format (bf16 only; no reference counterpart) ----
static int check_w3_shape(int n, int k) { return (n < 16 || (n % 16) != 0 || k < 128 || (k % 128) != 0) ? AWQ_ERR_SHAPE : AWQ_OK; }

int awq_pack_w3(const void* q_u8, void* qweight_w3, int n, int k, void* stream) {
  if (!q_u8 || !qweight_w3) return AWQ_ERR_NULL;
  if (check_w3_shape(n, k)) return AWQ_ERR_SHAPE;
  awq::launch_pack_w3(q_u8, qweight_w3, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_unpack_w3(const void* qweight_w3, void* out_u8, int n, int k, void* stream) {
  if (!qweight_w3 || !out_u8) return AWQ_ERR_NULL;
  if (check_w3_shape(n, k)) return AWQ_ERR_SHAPE;
  awq::launch_unpack_w3(qweight_w3, out_u8, n, k, (hipStream_t)stream);
  return finish_launch();
}

int awq_dequant_w3(const void* qweight_w3, const void* scales, const void* scaled_zeros, void* out, int n, int k,
                   int group_size, int dtype, void* stream) {
  if (!qweight_w3 || !scales || !scaled_zeros || !out) return AWQ_ERR_NULL;
  if (dtype != AWQ_BF16 && dtype != AWQ_F16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (check_w3_shape(n, k)) return AWQ_ERR_SHAPE;
  awq::launch_dequant_w3(qweight_w3, scales, scaled_zeros, out, n, k, dtype, (hipStream_t)stream);
  return finish_launch();
}

static int g_w3_skinny_max = 64;  // knob w3_skinny_max: 3-bit row counts up to this go to the skinny kernel (8 = never: the masked tile of the prefill GEMM)
// w3c tiles are read natively by every kernel: the only workspace is the OPTIONAL split-K scratch of short prompts (as for W4)
size_t awq_w3a16_forward_workspace_bytes(int m, int n, int k) { return m <= 8 ? 0 : awq::gemm_cdna4_v3_workspace_bytes_w3(m, n, k); }

int awq_w3a16_forward(const void* x, const void* qweight_w3, const void* scales, const void* scaled_zeros,
                      const void* sz_packed, const void* bias, void* out, int m, int n, int k, int group_size, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!sz_packed) return AWQ_ERR_NULL;
  int st = check_common(x, qweight_w3, scales, scaled_zeros, out, m, n, k, group_size, dtype);
  if (st != AWQ_OK) return st;
  if (check_w3_shape(n, k)) return AWQ_ERR_SHAPE;
  if (m <= 8) {
    // decode: the register-ring kernel (the LDS-DMA streaming kernel on w3c tiles measured equal to 4 % slower: profiles/r05_w3_streaming.txt)
    if (awq::launch_gemv_cdna4(x, qweight_w3, sz_packed, bias, out, m, n, k, 0, 3, dtype, (hipStream_t)stream) != 0)
      return AWQ_ERR_SHAPE;
    return finish_launch();
  }
  if (bias && !aligned16(bias)) return AWQ_ERR_ALIGN;
  // 9 .. 64 rows: one weight pass on the skinny kernel (w3c tiles), instead of a 256-row tile masked down to m rows
  if (m <= g_w3_skinny_max && awq::launch_skinny_w3(x, qweight_w3, sz_packed, bias, out, m, n, k, 0, dtype, (hipStream_t)stream) == 0) return finish_launch();
  // prefill / batched decode: the v4 / v4n weight producers read the 768-byte tiles directly (three words per lane, the fourth
  // rebuilt with six VALU operations per group); bias fused into the epilogue
  if (workspace && (!aligned16(workspace) || workspace_bytes < awq_w3a16_forward_workspace_bytes(m, n, k))) {
    workspace = nullptr;
    workspace_bytes = 0;
  }
  if (awq::launch_gemm_cdna4_v3(x, qweight_w3, sz_packed, bias, out, m, n, k, 0, dtype, workspace, workspace_bytes, (hipStream_t)stream, 3) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// QuantLlamaMLP on 3-bit gate / up projections (tinychat/modules/fused_mlp.py:33-83 with this repository's w_bit = 3): the two projections'
// rows interleaved 8 + 8 per 16-row slab (integer rows, then packed into w3c tiles), out[m, n2 / 2] = silu(gate) * up in the kernels' epilogue
size_t awq_w3a16_mlp_gate_up_forward_workspace_bytes(int m, int n2, int k) { return m > 8 ? awq::gemm_cdna4_v3_workspace_bytes_w3(m, n2, k) : 0; }

int awq_w3a16_mlp_gate_up_forward(const void* x, const void* qweight_w3_interleaved, const void* sz_packed, void* out, int m, int n2, int k,
                                  int group_size, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !qweight_w3_interleaved || !sz_packed || !out) return AWQ_ERR_NULL;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (m < 1) return AWQ_ERR_BATCH;
  if (n2 < 32 || (n2 % 32) != 0 || k < 128 || (k % 128) != 0 || (size_t)m * (size_t)k >= (1ull << 31)) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight_w3_interleaved) || !aligned16(out) || !aligned16(sz_packed)) return AWQ_ERR_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  if (m <= 8) {
    if (awq::launch_gemv_cdna4(x, qweight_w3_interleaved, sz_packed, nullptr, out, m, n2, k, 2, 3, dtype, st) != 0) return AWQ_ERR_SHAPE;
    return finish_launch();
  }
  if (m <= g_w3_skinny_max && awq::launch_skinny_w3(x, qweight_w3_interleaved, sz_packed, nullptr, out, m, n2, k, 2, dtype, st) == 0) return finish_launch();
  if (workspace && ((reinterpret_cast<uintptr_t>(workspace) & 63) != 0 || workspace_bytes < awq_w3a16_mlp_gate_up_forward_workspace_bytes(m, n2, k))) {
    workspace = nullptr;
    workspace_bytes = 0;
  }
  if (awq::launch_gemm_cdna4_v3(x, qweight_w3_interleaved, sz_packed, nullptr, out, m, n2, k, 0, dtype, workspace, workspace_bytes, st, 3, 2) != 0)
    return AWQ_ERR_SHAPE;
  return finish_launch();
}

// tensor-parallel row split of a 3-bit layer: the K shard's product as fp32 [m, n], unrounded, no bias (the W3 twin of
// awq_w4a16_partial_cdna4; awq_round_bias_f32 rounds the reduced sum once)
int awq_w3a16_partial(const void* x, const void* qweight_w3, const void* sz_packed, float* out_f32, int m, int n, int k,
                      int group_size, int dtype, void* stream) {
  if (!x || !qweight_w3 || !sz_packed || !out_f32) return AWQ_ERR_NULL;
  if (dtype != AWQ_F16 && dtype != AWQ_BF16) return AWQ_ERR_DTYPE;
  if (group_size != 128) return AWQ_ERR_GROUP;
  if (m < 1 || check_w3_shape(n, k)) return AWQ_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(qweight_w3) || !aligned16(out_f32) || !aligned16(sz_packed)) return AWQ_ERR_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  if (m <= 8) {
    if (awq::launch_gemv_cdna4(x, qweight_w3, sz_packed, nullptr, out_f32, m, n, k, 3, 3, dtype, st) != 0) return AWQ_ERR_SHAPE;
    return finish_launch();
  }
  if (m <= g_w3_skinny_max && awq::launch_skinny_w3(x, qweight_w3, sz_packed, nullptr, out_f32, m, n, k, 0, dtype, st, 1) == 0) return finish_launch();
  if (awq::launch_gemm_cdna4_v3(x, qweight_w3, sz_packed, nullptr, out_f32, m, n, k, 0, dtype, nullptr, 0, st, 3, 3) != 0) return AWQ_ERR_SHAPE;
  return finish_launch();
}

int awq_tune_set(const char* key, int value) {
  if (!key) return AWQ_ERR_NULL;
  // the knobs select between shipped code paths (tests force each of them) or, in AWQ_PROBES builds, timing probes; all of them
  // can change the summation order of results, so a default process cannot reach them: AWQ_TUNING=1 in the environment opts in
  const char* gate = getenv("AWQ_TUNING");
  if (!gate || gate[0] != '1') return AWQ_ERR_SHAPE;
  using K = awq::LinearKnobs;
  static const struct {
    const char* key;
    int K::*knob;
  } kLinear[] = {{"gemm_variant", &K::gemm_variant}, {"midm", &K::midm}, {"midm_min", &K::midm_min}, {"midm_max", &K::midm_max}, {"midm_waves", &K::midm_waves},
                 {"midm_ns", &K::midm_ns}, {"midm_ks", &K::midm_ks}, {"gemm_small_m", &K::gemm_small_m}, {"gemm_v4", &K::gemm_v4}, {"gemv_dma", &K::gemv_dma},
                 {"mlp_skinny_max", &K::mlp_skinny_max}, {"skinny16_szh", &K::skinny16_szh}};
  for (const auto& e : kLinear)
    if (!strcmp(key, e.key)) {
      awq::g_linear.*e.knob = value;
      return AWQ_OK;
    }
  if (awq::gemv_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::gemv_cdna4_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::skinny_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::midm_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::gemm_v3_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::attn_prefill_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::attn_tower_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::attn_splitkv_tune_set(key, value) == 0) return AWQ_OK;
  if (awq::w8a8_tune_set(key, value) == 0) return AWQ_OK;
  if (!strcmp(key, "w3_skinny_max")) {
    g_w3_skinny_max = value;
    return AWQ_OK;
  }
  return AWQ_ERR_SHAPE;
}

}  // extern "C"
