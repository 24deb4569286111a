/*
 * awq_cdna4.h -- C ABI of the MI355X-native (gfx950 / CDNA4) W4A16 fused dequant+matmul path.
 *
 * This is the drop-in boundary for the ONE hot path of mit-han-lab/llm-awq that this repository
 * accelerates: the two extension entry points behind `awq.quantize.qmodule.WQLinear.forward`
 *     awq_inference_engine.gemv_forward_cuda_new   (awq/kernels/csrc/quantization_new/gemv/gemv_cuda.h:4-12,
 *                                                   gemv_cuda.cu:245-338, bound at awq/kernels/csrc/pybind.cpp:23)
 *     awq_inference_engine.gemm_forward_cuda_new   (awq/kernels/csrc/quantization_new/gemm/gemm_cuda.h:3,
 *                                                   gemm_cuda.cu:1126-1236, bound at awq/kernels/csrc/pybind.cpp:22)
 * plus the data-format helpers either side of it (tinychat/offline-weight-repacker.py).
 *
 * Plain pointers and sizes only -- no torch types.  All pointers are DEVICE pointers unless
 * stated; `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every function
 * returns AWQ_OK (0) or a negative AWQ_ERR_* code and never throws; kernels are enqueued
 * asynchronously on `stream`.  Tensors follow the reference's v2 contract:
 *     qweight       int16 [N/4, K]      (awq/quantize/qmodule.py:26-65, 98-108)
 *     scales        T     [Gpad, N]     (qmodule.py:109-119), Gpad = 8*ceil(K/G/8) rows, only K/G used
 *     scaled_zeros  T     [Gpad, N]     (qmodule.py:120-130), = -(scales * zeros)
 *     x             T     [M, K] row-major contiguous,  out  T [M, N]
 * with T = fp16 or bf16 (`dtype`), G = group_size = 128.
 *
 * Numerics: each weight is materialised as round_T(q*s + sz) exactly as the
 * reference's __hfma2 does, products are accumulated in fp32 (MFMA), the result is rounded once to T.
 */
#ifndef AWQ_CDNA4_H_
#define AWQ_CDNA4_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWQ_ABI_VERSION 1

/* status codes */
#define AWQ_OK 0
#define AWQ_ERR_BATCH (-1)      /* gemv: m outside [1,16] ("Unsupported batch size for gemv kernel", gemv_cuda.cu:328-329) */
#define AWQ_ERR_GROUP (-2)      /* group_size != 128 ("Unsupported group size for gemv kernel", gemv_cuda.cu:332-335) */
#define AWQ_ERR_DTYPE (-3)      /* dtype is neither AWQ_F16 nor AWQ_BF16 (dispatch_utils.cuh:7-18) */
#define AWQ_ERR_SHAPE (-4)      /* n % 8 != 0, k % 128 != 0, non-positive sizes */
#define AWQ_ERR_ALIGN (-5)      /* a pointer is not 16-byte aligned */
#define AWQ_ERR_NULL (-6)       /* NULL pointer */
#define AWQ_ERR_WORKSPACE (-7)  /* workspace too small */
#define AWQ_ERR_LAUNCH (-8)     /* hipLaunch / runtime error (hipGetLastError text via awq_last_hip_error) */
#define AWQ_ERR_BITS (-9)       /* unsupported w_bit */

/* activation / scale element type */
#define AWQ_F16 0
#define AWQ_BF16 1

int awq_abi_version(void);
const char* awq_status_string(int status);
const char* awq_last_hip_error(void);

/* Replaces gemv_forward_cuda_new (gemv_cuda.cu:245-338): out[m,n] = x[m,k] . Wdeq[n,k]^T for
 * 1 <= m <= 16 (the reference accepts 1..7; the Python binding keeps that limit). */
int awq_w4a16_gemv(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                   void* out, int m, int n, int k, int group_size, int dtype, void* stream);

/* Replaces gemm_forward_cuda_new (gemm_cuda.cu:1126-1236) for any m >= 1.  `workspace` may be
 * NULL when awq_w4a16_gemm_workspace_bytes(m,n,k) == 0. It is zero-initialised by the callee when
 * used (the reference's uninitialised semaphore tensor, gemm_cuda.cu:28, is not reproduced). */
size_t awq_w4a16_gemm_workspace_bytes(int m, int n, int k);
int awq_w4a16_gemm(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                   void* out, int m, int n, int k, int group_size, int dtype,
                   void* workspace, size_t workspace_bytes, void* stream);

/* WQLinear.forward's dispatch (qmodule.py:201-224): m < 8 -> gemv, else gemm; optional bias[n]
 * (may be NULL) added in T after the matmul result was rounded to T, like `out + self.bias`. */
int awq_w4a16_forward(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                      const void* bias, void* out, int m, int n, int k, int group_size, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Parity / format helpers running the SAME device unpack + dequant code as the matmul kernels. */
/* out_u8[n, k] = logical 4-bit integer Q[n,k]  (inverse of pack_intweight, qmodule.py:26-65) */
int awq_unpack_v2(const void* qweight, void* out_u8, int n, int k, void* stream);
/* out[n, k] = round_T(Q[n,k] * scales[k/G, n] + scaled_zeros[k/G, n])  (gemv_cuda.cu:159-166) */
int awq_dequant_v2(const void* qweight, const void* scales, const void* scaled_zeros, void* out,
                   int n, int k, int group_size, int dtype, void* stream);
/* qweight_v2[n/4, k] from logical Q u8 [n, k]  (pack_intweight / packing_v2_from_unpacked) */
int awq_pack_v2(const void* q_u8, void* qweight, int n, int k, void* stream);
/* v1 checkpoint tensors -> v2 (tinychat/offline-weight-repacker.py:111-152):
 *   qweight_v1 int32 [n, k/8] -> qweight_v2 int16 [n/4, k]
 *   scales_v1 T [n, gpad], qzeros_v1 int32 [n, gpad/8] -> scales_v2 T [gpad, n], scaled_zeros_v2 T [gpad, n] */
int awq_repack_v1_to_v2(const void* qweight_v1, const void* scales_v1, const void* qzeros_v1,
                        void* qweight_v2, void* scales_v2, void* scaled_zeros_v2,
                        int n, int k, int gpad, int dtype, void* stream);

/* ---- "cdna4" interleave: this repository's MI355X-native int4 layout (what the rewritten
 * tinychat/offline-weight-repacker.py equivalent emits; DESIGN.md "cdna4 interleave").  Same bytes and
 * shape as v2 (int16 [N/4, K]); a pure nibble permutation that makes one 16-row x 128-k tile a contiguous
 * 1-KiB wave-load and lets the weights be dequantised on the matrix core.  bf16 and fp16; n % 16 == 0.
 * scales / scaled_zeros keep the v2 contract. ---- */
int awq_repack_v2_to_cdna4(const void* qweight_v2, void* qweight_cdna4, int n, int k, void* stream);
int awq_repack_cdna4_to_v2(const void* qweight_cdna4, void* qweight_v2, int n, int k, void* stream);
int awq_unpack_cdna4(const void* qweight_cdna4, void* out_u8, int n, int k, void* stream);
int awq_dequant_cdna4(const void* qweight_cdna4, const void* scales, const void* scaled_zeros, void* out,
                      int n, int k, int group_size, int dtype, void* stream);
/* sz_packed u32 [n/16][k/128][16] = {scale | scaled_zero << 16}: the scales re-laid next to the tiles so a lane
 * fetches both with one dword load per step.  Optional for the matmul entry points (NULL = read scales/zeros). */
int awq_pack_sz_cdna4(const void* scales, const void* scaled_zeros, void* sz_packed, int n, int k, void* stream);
/* sz_half u32 [n/16][k/128][16] = {f16(s') | f16(scaled_zero) << 16}, s' = scale for rows n % 4 < 2 and scale / 16 for the
 * others: the side buffer of the decode kernels' "f16-mantissa" dequant (csrc/awq_device.hpp Cdna4DequantH: two of the four
 * nibble extractions of a word need no shift when the dequant MFMA runs in its f16 form; exact, same single rounding).
 * *inexact_dev (device int, zeroed by the caller) is set when a scale or scaled zero is not exactly representable as a
 * normal f16 number: such a layer must keep using sz_packed.  dtype = type of scales / scaled_zeros. */
int awq_pack_szh_cdna4(const void* scales, const void* scaled_zeros, void* sz_half, int* inexact_dev, int n, int k, int dtype,
                       void* stream);
/* Decode (1 <= m <= 8) on cdna4 weights + sz_half: the fast path behind WQLinear.forward for m < 8 (replaces gemv_forward_cuda_new,
 * awq/kernels/csrc/quantization_new/gemv/gemv_cuda.cu:245-338) and QuantLlamaMLP's gate/up pair (tinychat/modules/fused_mlp.py:36-83).
 *   epilogue 0: out[m, n] = x . W^T (+ bias, in T)
 *   epilogue 1: qweight = [gate; up] stacked along N (n = 2 ffn), out[m, n/2] = silu(x . Wg^T) * (x . Wu^T), bias must be NULL
 *   epilogue 2: as 1 with gate / up rows interleaved 8 + 8 inside every 16-row slab (rows 16 j .. 16 j + 7 = gate rows 8 j ..,
 *               rows 16 j + 8 .. = the matching up rows): twice the blocks, every block one tile stream */
int awq_w4a16_decode_cdna4(const void* x, const void* qweight_cdna4, const void* sz_half, const void* bias, void* out, int m, int n,
                           int k, int group_size, int dtype, int epilogue, void* stream);
/* gemv on cdna4-interleaved weights (same contract as awq_w4a16_gemv otherwise) */
int awq_w4a16_gemv_cdna4(const void* x, const void* qweight_cdna4, const void* scales, const void* scaled_zeros,
                         const void* sz_packed, void* out, int m, int n, int k, int group_size, int dtype, void* stream);

/* QuantLlamaMLP's gate/up pair + SiLU*mul in ONE launch (tinychat/modules/fused_mlp.py:36-83 issues two
 * gemv_forward_cuda_new calls, F.silu and a multiply): qweight_gate_up = the gate and up projections' cdna4 buffers
 * stacked along N (n2 = 2 * intermediate rows, exactly what torch.cat([gate.qweight, up.qweight], 0) gives),
 * sz_packed built from the equally concatenated scales / scaled_zeros; out[m, n2/2] = silu(x.Wg^T) * (x.Wu^T), every
 * intermediate rounded to T like the reference's separate ops.  1 <= m <= 8, bf16 / fp16. */
int awq_w4a16_mlp_gate_up_cdna4(const void* x, const void* qweight_gate_up, const void* sz_packed, void* out, int m,
                                int n2, int k, int group_size, int dtype, void* stream);

/* QuantLlamaMLP.our_llama_mlp for ANY row count (tinychat/modules/fused_mlp.py:36-83: decode = two gemv_forward_cuda_new + F.silu +
 * multiply, prefill = two gemm_forward_cuda_new + F.silu + multiply) on the pair as llm_awq_amd.fused_mlp stacks it: gate and up
 * rows interleaved 8 + 8 inside every 16-row slab (n2 = 2 * intermediate rows).  out[m, n2/2] = T(T(silu(x.Wg^T)) * (x.Wu^T)).
 * The [m, n2] intermediate is never written, whichever kernel serves the row count: linear_route (csrc/awq_linear_route.hpp) holds
 * the rule, awq_w4a16_linear_route_cdna4 (entry 4) answers it for a call.  sz_half may be NULL. */
int awq_w4a16_mlp_gate_up_forward_cdna4(const void* x, const void* qweight_interleaved, const void* sz_packed, const void* sz_half,
                                        void* out, int m, int n2, int k, int group_size, int dtype, void* stream);
/* the same with an optional scratch buffer (awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes, 64-byte aligned; NULL / too small: ignored): with it
 * the columns a prompt's full rounds of 256-wide tiles leave over run as block pairs (K split inside the launch, csrc/awq_gemm_v6.hip) instead of 256 x 128 blocks */
size_t awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes(int m, int n2, int k);
int awq_w4a16_mlp_gate_up_forward_cdna4_ws(const void* x, const void* qweight_interleaved, const void* sz_packed, const void* sz_half, void* out, int m,
                                           int n2, int k, int group_size, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* gemm / WQLinear.forward dispatch on cdna4-interleaved weights (any m >= 1): which kernel serves a call is linear_route's answer
 * (csrc/awq_linear_route.hpp; query: awq_w4a16_linear_route_cdna4) */
/* RMSNorm fused in front of the quantised linear: replaces the FTLlamaRMSNorm launch
 * (tinychat/modules/fused_norm.py:7-21 -> awq/kernels/csrc/layernorm/layernorm.cu:39-61, layernorm_forward_cuda) followed by
 * WQLinear.forward / QuantLlamaMLP's gate/up pair.  x is the UN-normalised activation [m, k], gamma the norm weight [k]:
 *   xn = T((float(x) * rsqrtf(mean(x^2) + eps)) * float(gamma))          (layernorm.cu:55,60)
 *   fused_gate_up == 0: out[m, n]   = xn . W^T (+ bias)                  (qmodule.py:201-224)
 *   fused_gate_up != 0: out[m, n/2] = silu(xn . Wg^T) * (xn . Wu^T)      (fused_mlp.py:36-83; qweight = [gate; up], n = 2 * ffn)
 * Decode rows only: 1 <= m <= 4, k <= 16384; returns AWQ_ERR_BATCH / AWQ_ERR_SHAPE otherwise (run norm and linear separately). */
int awq_w4a16_rmsnorm_forward_cdna4(const void* x, const void* gamma, float eps, const void* qweight, const void* sz_packed,
                                    const void* bias, void* out, int m, int n, int k, int group_size, int dtype,
                                    int fused_gate_up, void* stream);

/* The norm alone, any row count (the prefill side of the same step; replaces layernorm_forward_cuda, awq/kernels/csrc/layernorm/
 * layernorm.cu:39-89 as tinychat's FTLlamaRMSNorm calls it, fused_norm.py:7-21): out[m, k] = T((float(x) * rsqrtf(mean(x^2) + eps)) *
 * float(gamma)), fp32 sum of squares, one rounding.  k % 8 == 0; x, gamma, out 16-byte aligned. */
int awq_rmsnorm(const void* x, const void* gamma, float eps, void* out, int m, int k, int dtype, void* stream);

/* OPTIONAL fp32 workspace of awq_w4a16_gemm_cdna4 / awq_w4a16_forward_cdna4 (0 = none useful).  Prompts of 256 .. ~1 k tokens
 * against narrow projections produce too few output tiles to fill the 256 CUs; given this many bytes (16-byte aligned) the
 * K loop is split over blocks and a second kernel adds the partial tiles in a fixed order -- the role of the reference's
 * split_k_iters + semaphore (gemm_cuda.cu:546-619); for awq_w4a16_gemm_cdna4_pair_plan's shapes the two halves of K meet inside
 * ONE launch (64-byte aligned workspace, any contents; one launch at a time per workspace).  Short prompts on the skinny kernel
 * (17 .. 146 rows) against n = 4096-class projections split K over two blocks per slab group the same way inside one
 * launch: fp32 parts in the workspace, added in part order by the block that draws the group's last ticket (the ticket words live in a
 * small zero-initialised per-device array the library allocates at the first such call outside a stream capture).  Without a workspace
 * the call runs unsplit (slower, same contract). */
size_t awq_w4a16_forward_cdna4_workspace_bytes(int m, int n, int k);
/* 9 .. 255 rows (round 6): the mid-M kernel (csrc/awq_midm_cdna4.hip) -- the row range of the reference's 16 / 32 / 64-row tiles + split_k_iters,
 * gemm_cuda.cu:1155-1206, :546-619.  Its K split across blocks keeps the fp32 parts in the caller's workspace and the ticket words in a library-owned,
 * zero-initialised per-device array in which a word belongs to ONE launch at a time: eager launches use the lane of their stream, a launch recorded
 * during a stream capture gets words of its own that are never handed out again (so graphs may be replayed on any streams); no lane / region left, or
 * no workspace: the call runs unsplit.  hipStreamPerThread (a different stream in every thread under one handle value) never gets a lane: its calls
 * run unsplit, so threads that share that handle never share ticket words.  awq_midm_init allocates that array for the current device ahead of the first call (optional; the first
 * split launch outside a capture does it otherwise).  Returns AWQ_OK or AWQ_ERR_LAUNCH. */
int awq_midm_init(void);
/* host-side query (no GPU work): the tiles the prefill GEMM launches for an [m, n] output of a 3- or 4-bit matrix.  *mode: 0 = 256 x 256
 * blocks, 1 = 256 x 128, 2 = 256 x 256 for the first *cols_main column tiles and 256 x 128 for the rest, 3 = 256 x 192; returns the number
 * of thread blocks, 0 if the GEMM does not take this m (decode / skinny kernels do).  The counterpart of the reference's tile table,
 * gemm_cuda.cu:1155-1232. */
int awq_w4a16_gemm_cdna4_plan(int m, int n, int bits, int* mode, int* cols_main);
/* host-side query: 1 if a W4 prefill call of this shape, GIVEN its workspace, runs as pairs of 256 x 256 blocks that each sum half of K and
 * combine inside the launch (tiles that fill at most half the chip and K >= 8192: down_proj of Llama-3-8B at 1536 .. 2048 rows) -- the role
 * of the reference's split_k_iters + Semaphore, gemm_cuda.cu:546-619, without a second kernel; 0 = the tiles awq_w4a16_gemm_cdna4_plan names.
 * The two halves' fp32 sums are added once (lower K range + upper K range): another association than the unsplit kernels', same products. */
int awq_w4a16_gemm_cdna4_pair_plan(int m, int n, int k);
/* The two blocks of a pair wait for each other's partial sums with a BOUNDED spin; a block whose partner never arrives (a launch that cannot own
 * the chip: CU masks, another tenant holding every CU) writes NaN to its outputs instead of hanging the queue and counts itself in a library-owned
 * per-device word.  This query copies that word to the host (it synchronises with the device): *count = pair blocks of the CURRENT device that
 * gave up since the library was loaded; 0 on a healthy run.  The reference's Semaphore (semaphore.h:44-103) spins without a bound.  Returns
 * AWQ_OK or AWQ_ERR_LAUNCH. */
int awq_w4a16_gemm_cdna4_pair_lost(unsigned int* count);
/* host-side query: which kernel runs the 256 x 128 blocks of such a launch over n_cols weight rows.  Returns 1 = awq_gemm_v6.hip (one wave
 * per SIMD, two slabs per wave: every unsplit launch of W4 tiles at m >= 256), 0 = awq_gemm_v4n.hip unsplit (m < 256: masked single row
 * tile; W3 tiles), ks >= 2 = awq_gemm_v4n.hip with the K loop split into ks ranges (needs the workspace and no fused SiLU*mul tail). */
int awq_w4a16_gemm_cdna4_narrow_kernel(int m, int n_cols, int k, int bits, int has_workspace, int epilogue);
/* host-side query: how awq_w4a16_decode_cdna4 / awq_w4a16_mlp_gate_up_forward_cdna4 serve m <= 8 rows of an [n, k] matrix.  *kernel: 0 =
 * the LDS-DMA streaming kernel (awq_gemv_dma.hip; x staged per slab), 1 = the skinny kernel (awq_skinny_cdna4.hip; x through registers,
 * one weight pass -- where the streaming kernel's staging of m x k x 2 bytes per slab would crowd its ring out of LDS, and, since round 6, from two rows on
 * every launch that is not a wide fused pair or between one and 1.5 slabs per CU).  Returns the number of weight passes (1; more when
 * the streaming kernel serves the rows in chunks), 0 if the shape is not served.  The reference's GEMV handles its batch inside one pass,
 * gemv_cuda.cu:187-208, 291-329.
 * Both queries read the plan the launcher walks: decode_plan in csrc/awq_decode_plan.hpp, one pure function of (m, n, k, epilogue, CU
 * count, knobs) whose rules are one commented row each.  The knobs awq_tune_set can force on it: decode_skinny_from, gemvd_waves, gemvd_d,
 * gemvd_want, gemvd_il (and gemvd_probe, which no rule reads).  *kernel names ONE kernel for the call -- 1 when a single skinny launch serves
 * all rows, else 0 -- while a call served in row chunks asks the rule per chunk; the rule is monotonic in the row count, and no chunk of any
 * shape with epilogue 0 - 2, 1 - 8 rows, n / 16 in 1 - 4200, k / 128 in 1 - 129, 224, 448 runs the skinny kernel under an answer of 0 (default
 * knobs, decode_skinny_from 1 and 9). */
int awq_w4a16_decode_cdna4_plan(int m, int n, int k, int epilogue, int* kernel);
/* the same plan chunk by chunk.  Returns the number of chunks (= launches = weight passes), 0 if the shape is not served; for
 * 0 <= chunk < that number, out = { rows, kernel (0 streaming, 1 skinny), then for a streaming chunk: waves per block, k-steps per wave,
 * ring depth, dynamic LDS bytes, flags (bit 0: K split interleaved over the waves, bit 1: the straight-line one-row kernel), 0; for a skinny
 * chunk: 0, 0, 0, 0, 0, block shape x 8 + x pieces staged per step (shape 0 = 8 waves x 1 slab, 1 = 16 x 1, 2 = 8 x 2, 3 = 8 x 7; pieces 1 - 4) }.
 * out may be NULL. */
int awq_w4a16_decode_cdna4_plan_detail(int m, int n, int k, int epilogue, int chunk, int out[8]);
/* Which launcher serves a call of one of the six dense W4 cdna4 entries below -- the route the entry itself switches on (linear_route,
 * csrc/awq_linear_route.hpp: the one place where the rules are written; tests/linear_route_cases.py pins it).  entry: 0 awq_w4a16_forward_cdna4,
 * 1 ..._forward_cdna4_szh, 2 awq_w4a16_gemm_cdna4, 3 awq_w4a16_gemv_cdna4, 4 awq_w4a16_mlp_gate_up_forward_cdna4_ws (n = n2), 5 awq_w4a16_partial_cdna4.
 * flags, the facts about the call's pointers: 1 sz_packed given, 2 sz_half given and 16-byte aligned, 4 bias given, 8 workspace given, 16 the
 * workspace is 64-byte aligned and at least the entry's ..._workspace_bytes (read by entry 4).  Returns the leaf: 1 streaming decode kernel,
 * 2 register-ring GEMV, 3 mid-M kernel, 4 skinny kernel's 16-row form, 5 skinny kernel, 6 skinny gate/up form, 7 tile kernels, 8 the generic
 * launch (launch_gemm / the entry-3 GEMV); 0 = the entry refuses these arguments (out untouched).  out = { leaf, scale format (0 sz_packed,
 * 1 sz_half), epilogue (0 plain / bias, 1 SiLU * mul pair, 2 fp32 partial), bias (0 none, 1 fused, 2 a separate bias-add launch), workspace
 * handed on, bias must be 16-byte aligned, deciding row of the entry's table, 0 }.  out may be NULL.  Host only. */
int awq_w4a16_linear_route_cdna4(int entry, int m, int n, int k, int flags, int out[8]);
int awq_w4a16_gemm_cdna4(const void* x, const void* qweight_cdna4, const void* scales, const void* scaled_zeros,
                         const void* sz_packed, void* out, int m, int n, int k, int group_size, int dtype,
                         void* workspace, size_t workspace_bytes, void* stream);
int awq_w4a16_forward_cdna4(const void* x, const void* qweight_cdna4, const void* scales, const void* scaled_zeros,
                            const void* sz_packed, const void* bias, void* out, int m, int n, int k, int group_size,
                            int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* the same with the layer's sz_half side buffer (awq_pack_szh_cdna4 reported exact; NULL = awq_w4a16_forward_cdna4): prompts of >= 256 rows dequantise
 * in the f16-mantissa form the decode kernels use (fewer VALU instructions per weight beside the MFMAs) -- identical results, sz_packed still serves every
 * other row count */
int awq_w4a16_forward_cdna4_szh(const void* x, const void* qweight_cdna4, const void* scales, const void* scaled_zeros, const void* sz_packed,
                                const void* sz_half, const void* bias, void* out, int m, int n, int k, int group_size, int dtype, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- grouped (per-expert) W4A16 GEMM for MoE layers: BASELINE.json's Mixtral-8x7B configuration.  New capability
 * (the reference has no MoE path).  Tokens are sorted by expert: expert e owns rows
 * [expert_offsets[e], expert_offsets[e+1]) of x_sorted [T, k] / out [T, n]; expert_offsets is a DEVICE int32 [E+1]
 * array (offsets[0] = 0, offsets[E] = T), so routing never synchronises the host.  Weights are stacked per expert:
 * qweight int16 [E, n/4, k], scales / scaled_zeros T [E, gpad, n].  layout 0 = v2, 1 = cdna4 (bf16). ---- */
int awq_w4a16_moe_gemm(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* expert_offsets, void* out, int total_tokens, int num_experts, int n, int k, int gpad,
                       int group_size, int dtype, int layout, void* stream);

/* the same on cdna4 buffers with the stacked packed scales (int32 [E, n/16, k/128, 16]): decode batches (total_tokens <= 8,
 * hence at most 8 rows per expert) stream each expert's tiles once with the GEMV structure (block = (expert, slab));
 * larger batches run the grouped GEMM.  bf16 and fp16. */
int awq_w4a16_moe_forward_cdna4(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros,
                                const void* sz_packed, const void* expert_offsets, void* out, int total_tokens,
                                int num_experts, int n, int k, int gpad, int group_size, int dtype, void* stream);
/* the same with the experts' stacked sz_half side buffers (int32 [E, N/16, K/128, 16], every expert reported exact by awq_pack_szh_cdna4; NULL = the call
 * above): the grouped tile launch (>= 256 sorted rows) dequantises in the f16-mantissa form, identical results */
int awq_w4a16_moe_forward_cdna4_szh(const void* x_sorted, const void* qweight, const void* scales, const void* scaled_zeros, const void* sz_packed,
                                    const void* sz_half, const void* expert_offsets, void* out, int total_tokens, int num_experts, int n, int k,
                                    int gpad, int group_size, int dtype, void* stream);

/* out = T(T(silu(gate)) * up) elementwise over `count` values (count % 8 == 0): the activation step between the projections where it is not
 * fused into a kernel epilogue (tinychat/modules/fused_mlp.py:79-82: c = F.silu(gate_output) * up_output, every op rounded to T). */
int awq_silu_mul(const void* gate, const void* up, void* out, size_t count, int dtype, void* stream);
/* The expert MLP's first half in ONE grouped launch: every expert's w1 (gate) and w3 (up) rows interleaved 8 + 8 inside each 16-row slab
 * (n2 = 2 x ffn rows per expert: qweight int16 [E, n2/4, k], sz_packed int32 [E, n2/16, k/128, 16], scales / scaled_zeros T [E, gpad, n2] of
 * the same interleaved rows), out[T, n2/2] = T(T(silu(x . W1^T)) * T(x . W3^T)) -- the dense pair's epilogue (tinychat/modules/
 * fused_mlp.py:36-83) generalised to sorted tokens; the reference has no MoE path.  >= 256 sorted rows: fused into the grouped tile's
 * epilogue, the [T, n2] intermediate is never written (scratch may be NULL).  Fewer rows: the grouped GEMV / skinny kernels write the pair's
 * product to `scratch` (>= total_tokens * n2 * 2 bytes, 16-byte aligned; AWQ_ERR_WORKSPACE otherwise) and the SiLU * mul tail runs as its own
 * launch.  scales / scaled_zeros are only read by the fallback kernels of that small-batch path. */
int awq_w4a16_moe_mlp_gate_up_cdna4(const void* x_sorted, const void* qweight_interleaved, const void* scales, const void* scaled_zeros,
                                    const void* sz_packed, const void* expert_offsets, void* out, void* scratch, size_t scratch_bytes,
                                    int total_tokens, int num_experts, int n2, int k, int gpad, int group_size, int dtype, void* stream);
int awq_w4a16_moe_mlp_gate_up_cdna4_szh(const void* x_sorted, const void* qweight_interleaved, const void* scales, const void* scaled_zeros,
                                        const void* sz_packed, const void* sz_half, const void* expert_offsets, void* out, void* scratch,
                                        size_t scratch_bytes, int total_tokens, int num_experts, int n2, int k, int gpad, int group_size, int dtype,
                                        void* stream);

/* ---- MoE routing on the device: what surrounds the grouped launches above in a Mixtral-style block (new capability: the reference has no MoE
 * path).  One launch each, no workspace, no atomics, no host read; every size that shapes a grid is an argument.  Limits (AWQ_ERR_SHAPE
 * otherwise, before anything is launched): 1 <= num_experts <= 64, 1 <= top_k <= min(num_experts, 8), tokens >= 1, tokens * top_k <= 2^20.
 * Pointers: AWQ_ERR_NULL / AWQ_ERR_ALIGN (activations 16 bytes, int32 / fp32 arrays 4 bytes, logits their element size). ---- */
#define AWQ_F32 2 /* router logits only */
/* router_logits [tokens, num_experts] (logits_dtype AWQ_F16 / AWQ_BF16 / AWQ_F32; AWQ_ERR_DTYPE otherwise), contiguous ->
 *   topk_ids int32 [tokens, top_k]  the top_k largest logits of the row in descending order; among equal logits the lower index wins (compared
 *                                   through the monotone float -> unsigned key, a total order whatever the bits)
 *   topk_w   fp32  [tokens, top_k]  exp(l_j - l_0) / sum_{i < top_k} exp(l_i - l_0) (renormalize != 0: softmax -> topk -> w / w.sum()), or
 *                                   exp(l_j - l_0) / sum_{e < num_experts} exp(l_e - l_0) (renormalize == 0: plain softmax weights)
 *   order    int32 [tokens top_k]   the flat slots s = t top_k + j sorted by expert, stable;  inv [tokens top_k]: inv[order[r]] = r
 *   offsets  int32 [num_experts+1]  first sorted row of every expert, offsets[num_experts] = tokens top_k (the grouped launches' expert_offsets)
 * A row that holds a NaN, or whose largest logit is infinite, has unspecified weights; its ids are still top_k distinct experts and the three index
 * arrays a valid sort. */
int awq_moe_route(const void* router_logits, int logits_dtype, int tokens, int num_experts, int top_k, int renormalize, void* topk_ids,
                  void* topk_w, void* order, void* inv, void* offsets, void* stream);
/* xs[r] = x[order[r] / top_k]: x T [tokens, hidden] -> xs T [tokens top_k, hidden]; hidden % 8 == 0 (16-byte loads and stores) */
int awq_moe_gather(const void* x, const void* order, void* xs, int tokens, int top_k, int hidden, int dtype, void* stream);
/* out[t] = T( sum_j f32( T( f32(ys[inv[t top_k + j]]) * f32(T(topk_w[t, j])) ) ) ): the sum in fp32, j ascending from +0, one final rounding; writes
 * every element of out T [tokens, hidden] (no zero-fill, no scatter).  ys T [tokens top_k, hidden], hidden % 8 == 0. */
int awq_moe_combine(const void* ys, const void* inv, const void* topk_w, void* out, int tokens, int top_k, int hidden, int dtype, void* stream);

/* ---- Next-token sampling on the device: what tinychat/stream_generators/stream_gen.py:19-32,120-134 does between two decode steps
 * (temperature -> repetition penalty -> top-p -> top-k -> softmax -> multinomial -> int()), as ONE launch without a host read.  logits
 * [batch, vocab] (AWQ_F16 / AWQ_BF16 / AWQ_F32, contiguous, aligned to its element) -> tokens int32 [batch].  Every parameter is a per-row device array
 * and may be NULL, which switches that step off: u fp32 [batch] in [0, 1) (required), temperature / top_p / repetition_penalty fp32 [batch],
 * top_k int32 [batch] (<= 0 or >= vocab: off), history int32 [batch, max_history] with hist_len int32 [batch] (both or neither), seqlens int32
 * [batch] (a negative entry = an inactive slot: tokens[b] = -1 and nothing else is read or written for the row), stop_ids int32 [num_stop],
 * finished int32 [batch].  DESIGN.md "Sampling" states the result by values (fp32 arithmetic, IEEE division by the temperature, whole tie groups
 * kept, fixed-point masses so that the launch is bit-stable from run to run).  flags: AWQ_SAMPLE_APPEND writes the token to
 * history[b, hist_len[b]] (if it fits) and adds one to hist_len[b]; AWQ_SAMPLE_ADVANCE sets seqlens[b] to -1 if the token is a stop id or
 * seqlens[b] + 1 >= max_len, else to seqlens[b] + 1; a token in stop_ids sets finished[b] = 1 whenever both arrays are given.  A row that holds a
 * NaN or +inf returns an unspecified token in [0, vocab) and does not disturb the other rows; history ids outside [0, vocab) are ignored.
 * Limits: 1 <= vocab <= 2^20, batch >= 1 (AWQ_ERR_SHAPE), checked with the pointers (AWQ_ERR_NULL / AWQ_ERR_DTYPE / AWQ_ERR_ALIGN) before anything
 * is launched.  No workspace, no global atomics; capturable. ---- */
#define AWQ_SAMPLE_APPEND 1
#define AWQ_SAMPLE_ADVANCE 2
int awq_sample_logits(const void* logits, int logits_dtype, int batch, int vocab, const void* u, const void* temperature, const void* top_k,
                      const void* top_p, const void* repetition_penalty, void* history, void* hist_len, int max_history, void* seqlens,
                      const void* stop_ids, int num_stop, void* finished, int max_len, int flags, void* tokens, void* stream);

/* ---- Prompt-lookup speculative decoding on the device: four launches around a packed step of the KV-cache path (cu_seqlens_q, a token budget
 * total_q, awq_attn_varq*), none of which reads anything on the host.  DESIGN.md "Speculative decoding" states each result by values.  batch = the
 * slots of the sampler; history int32 [batch, max_history], hist_len / seqlens int32 [batch] are awq_sample_logits' arrays (seqlens[b] < 0 = an
 * inactive slot); 0 <= kmax <= 15 is the longest draft.  Every array is device memory, 4-byte aligned (AWQ_ERR_ALIGN); required pointers give
 * AWQ_ERR_NULL, sizes outside the limits AWQ_ERR_SHAPE, all checked before anything is launched.  No workspace, no global atomics; capturable.
 *
 * awq_spec_draft_ngram: with L = hist_len[b], draft_len[b] = 0 for an inactive slot, for L > max_history and for L < ngram_min + 1.  Otherwise
 *   m_i = the length of the longest common suffix of history[.. i] and history[.. L - 1], capped at ngram_max, for the ends 0 <= i <= L - 2; the
 *   match is the i that maximises (m_i, i) among m_i >= ngram_min (none: draft_len[b] = 0); the draft is history[i + 1 ..] cut to the first of kmax,
 *   max(0, max_draft[b]) (max_draft int32 [batch] or NULL), L - 1 - i, max_len - seqlens[b] - 1 and the first id outside [0, vocab).  drafts int32
 *   [batch, kmax] holds it with -1 behind; every element of both outputs is written.  1 <= ngram_min <= ngram_max <= 8, batch, max_history, vocab >= 1.
 * awq_spec_pack: A = the active slots; the R = total_q - A extra rows go to the drafts in slot order, c_b = clamp(R - sum_{a < b} draft_len[a], 0,
 *   draft_len[b]) (draft_len clamped into [0, kmax], 0 for inactive slots); draft_len[b] = c_b and drafts[b, c_b:] = -1 are written back; n_b = 1 + c_b
 *   for an active slot, else 0; cu_seqlens_q int32 [batch + 1] = its exclusive prefix sum; input_ids int32 [total_q]: last_tokens[b], then the
 *   slot's c_b drafts, at cu[b]; -1 from cu[batch] on.  1 <= batch <= 65535, total_q >= batch.
 * awq_spec_verify: row_tokens[r] for every row r < total_q of logits [total_q, vocab] (dtype, alignment and vocab limit of awq_sample_logits) = steps
 *   1 to 8 of the sampling contract with the parameters of the row's owner b (temperature / top_k / top_p / repetition_penalty [batch], each may be
 *   NULL) and u[r] (fp32 [total_q]); the penalty set is history[b, :min(hist_len[b], max_history)] plus, for the row j = r - cu[b], the inputs
 *   input_ids[cu[b] + i], 1 <= i <= j, with 0 <= hist_len[b] + i - 1 < max_history.  A row at or behind cu[batch] gets -1.  Nothing else is written.
 * awq_spec_accept: per slot with n_b = cu[b + 1] - cu[b] >= 1 rows (capped at kmax + 1) and seqlens[b] >= 0: a = the number of leading j in
 *   [0, n_b - 2] with row_tokens[cu + j] == input_ids[cu + j + 1]; for j = 0 .. a in order the token row_tokens[cu + j] is emitted and taken through
 *   the append / stop / advance of awq_sample_logits (same flags, same arrays), stopping after the first that sets seqlens[b] = -1.  out_tokens
 *   int32 [batch, kmax + 1] holds the emitted tokens with -1 behind, num_emitted [batch] their count, last_tokens [batch] the last one (the next
 *   awq_spec_pack's input).  Any other slot: num_emitted 0, last_tokens -1, out_tokens -1, nothing else touched. ---- */
int awq_spec_draft_ngram(const void* history, const void* hist_len, const void* seqlens, const void* max_draft, void* drafts, void* draft_len,
                         int batch, int max_history, int vocab, int kmax, int ngram_min, int ngram_max, int max_len, void* stream);
int awq_spec_pack(const void* last_tokens, void* drafts, void* draft_len, const void* seqlens, void* cu_seqlens_q, void* input_ids, int batch,
                  int kmax, int total_q, void* stream);
int awq_spec_verify(const void* logits, int logits_dtype, int total_q, int vocab, const void* u, const void* cu_seqlens_q, const void* input_ids,
                    int batch, const void* temperature, const void* top_k, const void* top_p, const void* repetition_penalty, const void* history,
                    const void* hist_len, int max_history, void* row_tokens, void* stream);
int awq_spec_accept(const void* row_tokens, const void* input_ids, const void* cu_seqlens_q, int batch, int total_q, int kmax, void* history,
                    void* hist_len, int max_history, void* seqlens, const void* stop_ids, int num_stop, void* finished, int max_len, int flags,
                    void* out_tokens, void* num_emitted, void* last_tokens, void* stream);

/* ---- LM head for decode: the reference's `self.norm` + `lm_head` (tinychat/models/llama.py:395,412: an RMSNorm and an unquantised
 * nn.Linear(hidden, vocab)) as ONE launch that reads the weight matrix once whatever m is.  DESIGN.md "LM head" states the result by values:
 *   x       T [m, k], row stride ldx elements (ldx % 8 == 0, ldx >= k): a prompt's last rows are selected by ldx, nothing is copied
 *   gamma   T [k] or NULL: xn = T((f32(x) * rsqrtf(sum x^2 / k + eps)) * f32(gamma)), awq_rmsnorm's arithmetic bit for bit; NULL: xn = x
 *   weight  T [v, k] row-major contiguous (nn.Linear.weight as it is loaded, no repack); bias T [v] or NULL, added in fp32 after the k sum
 *   seqlens int32 [m] or NULL: a row with seqlens[b] < 0 is inactive -- out[b, :] is left untouched and whatever x[b, :] holds changes no other
 *           row; if every row is inactive nothing is read
 *   out     [m, v] contiguous, out_dtype AWQ_F32 (the fp32 sum: what awq_sample_logits should be fed) or dtype (rounded once, nearest-even)
 * The fp32 sum is taken in an order that depends on k alone (not on m, gamma or max_blocks), so a row's logits do not depend on its batch.
 * Limits: 1 <= m <= 64 (AWQ_ERR_BATCH), v >= 1, k >= 8 and k % 8 == 0, ldx as above (AWQ_ERR_SHAPE), out_dtype AWQ_F32 or dtype (AWQ_ERR_DTYPE),
 * x / weight / out / gamma / bias 16-byte aligned, seqlens 4-byte aligned (AWQ_ERR_ALIGN); checked before anything is launched.  max_blocks: 0 =
 * the plan's grid, otherwise a cap on it (tests).  No workspace, no atomics, bit-stable from run to run; capturable.
 * awq_lm_head_plan (host only, no device call): out[4] = {blocks, vocabulary rows per tile, waves per block, k split}. ---- */
int awq_lm_head(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                int out_dtype, int m, int v, int k, int dtype, int max_blocks, void* stream);
int awq_lm_head_plan(int m, int v, int k, int out[4]);
/* out T [n, k] = table T [v, k] rows named by tokens int32 [n]; ZEROS for an id outside [0, v) (-1 = the sampler's finished slot), which never
 * causes a read outside the table.  n >= 1, v >= 1, k >= 8, k % 8 == 0 (AWQ_ERR_SHAPE); table / out 16-byte, tokens 4-byte aligned. */
int awq_embed_tokens(const int* tokens, const void* table, void* out, int n, int v, int k, int dtype, void* stream);

/* ---- Token log-probabilities: the LM head fused with log-sum-exp, for scoring text (perplexity, `logprobs`, lm-eval's loglikelihood).  No logit is
 * ever written to memory.  DESIGN.md "Token log-probabilities" states the result by values; per row i of x (T = dtype):
 *   xn          as awq_lm_head: with gamma, awq_rmsnorm's arithmetic bit for bit (that launch runs first, into the head of the workspace; ldx must
 *               then equal k); gamma NULL: xn = x, row stride ldx elements (ldx % 8 == 0, ldx >= k)
 *   z[i, j]     = sum_k f32(xn[i, k]) f32(weight[j, k]) in fp32, + f32(bias[j]) in fp32 when bias is given; with round_logits != 0 every z is then
 *               rounded once to T, nearest-even, as an nn.Linear would store it
 *   lse[i]      = log sum_j exp(z[i, j]);  argmax[i] = the LOWEST j among the maxima of z[i, :] (awq_sample_logits' tie rule)
 *   target_logit[i] = z[i, targets[i]];  logprob[i] = target_logit[i] - lse[i], one fp32 subtraction
 *   targets     int32 [t] or NULL.  A row whose target lies outside [0, v) (-1: the sampler's finished slot, -100: torch's ignore_index) is IGNORED:
 *               its four outputs keep what they held and whatever its x holds, NaN included, changes no other row; a launch whose rows are all
 *               ignored reads no weight.  With targets NULL every row is active and logprob / target_logit must be NULL (AWQ_ERR_NULL).
 *   outputs     fp32 [t] (argmax int32 [t]); each may be NULL
 * Two launches (tiles, combine), no atomics, no host read, capturable.  The vocabulary tile and every sum order depend on (v, k) alone -- not on t, the
 * row's index, the other rows or max_blocks -- so a row's outputs are the same bits wherever it is served.
 * Limits: t >= 1, 1 <= v <= 2^30 (both entries), k >= 8, k % 8 == 0, ldx as above, max_blocks >= 0 (0 = the plan's grid, otherwise a cap on it) (AWQ_ERR_SHAPE); dtype
 * AWQ_F16 / AWQ_BF16 (AWQ_ERR_DTYPE); x / weight / gamma / bias / workspace 16-byte, targets and the outputs 4-byte aligned (AWQ_ERR_ALIGN);
 * workspace NULL or below awq_lm_head_logprobs_workspace_bytes(t, v, k, gamma != NULL) (AWQ_ERR_WORKSPACE); all checked before anything is launched.
 * awq_lm_head_logprobs_plan (host only): out[4] = {rows of x per tile, vocabulary rows per tile, blocks, k per step}.
 * awq_token_logprobs: the same lse / argmax / logprob for logits that already exist -- logits [b, v] of logits_dtype (AWQ_F32 / AWQ_F16 / AWQ_BF16),
 * row stride ld elements (ld >= v), element-size aligned; one block per row, no workspace; ignored rows and NULL rules as above. ---- */
int awq_lm_head_logprobs(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                         float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                         void* workspace, size_t workspace_bytes, int max_blocks, void* stream);
size_t awq_lm_head_logprobs_workspace_bytes(int t, int v, int k, int with_gamma);
int awq_lm_head_logprobs_plan(int t, int v, int k, int out[4]);
int awq_token_logprobs(const void* logits, int logits_dtype, long ld, const int* targets, float* logprob, float* lse, int* argmax, int b, int v,
                       void* stream);

/* ---- FINAL-LOGIT SOFT-CAPPING (Gemma-2: final_logit_softcapping = 30): every logit z becomes softcap * tanh(z / softcap), evaluated in fp32 with
 * the device function of the attention cap (absolute error of tanh <= 10 * 2^-24).  DESIGN.md "Soft-capping" states the results by values.
 *   awq_lm_head_softcap           awq_lm_head's arguments with softcap in front of max_blocks.  The cap is applied to the fp32 sum behind the bias,
 *                                 before the one rounding to out_dtype: with out_dtype AWQ_F32 the result carries the bits of awq_logit_softcap on
 *                                 awq_lm_head's fp32 output.
 *   awq_lm_head_logprobs_softcap  awq_lm_head_logprobs' arguments with softcap behind round_logits.  Every z is capped before it enters the max / sum-exp,
 *                                 the target pick and the argmax.  With round_logits != 0: z is rounded to T, capped in fp32 and rounded to T once more.
 *   awq_logit_softcap             logits that already exist, in place: logits [b, v] of logits_dtype (AWQ_F32 / AWQ_F16 / AWQ_BF16), row stride ld
 *                                 elements (ld >= v), element-size aligned; computed in fp32 and rounded once.  seqlens int32 [b] or NULL: a row with
 *                                 seqlens[row] < 0 is neither read nor written.  One elementwise launch, no workspace.  1 <= b <= 65535 * 1024,
 *                                 1 <= v <= 2^30 (AWQ_ERR_SHAPE).
 * softcap == 0 is "no cap": the first two ARE awq_lm_head / awq_lm_head_logprobs and return their bits, the third launches nothing.  softcap < 0,
 * infinite or NaN: AWQ_ERR_SHAPE.  Otherwise the codes of the uncapped entries; all checked before anything is launched. ---- */
int awq_lm_head_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                        int out_dtype, int m, int v, int k, int dtype, float softcap, int max_blocks, void* stream);
int awq_lm_head_logprobs_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                                 float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                                 float softcap, void* workspace, size_t workspace_bytes, int max_blocks, void* stream);
int awq_logit_softcap(void* logits, int logits_dtype, long ld, const int* seqlens, int b, int v, float softcap, void* stream);

/* ---- Multi-LoRA on packed steps: y[t, :] += scaling[a] (x[t, :] A_a^T) B_a^T with a = adapter_ids[owner of row t], in TWO launches per adapted
 * linear whatever the mix of adapters, decodes and prompt chunks (shrink, then expand).  DESIGN.md "Multi-LoRA" states the result by values:
 *   x             T [total_q, k], row stride ldx elements (ldx % 8 == 0, ldx >= k): the packed rows of the step
 *   a_pool        T [slots, rs, k] contiguous, rs = n_slices * r: slot a, slice j owns rows j r .. (j + 1) r - 1
 *   b_pool        T [slots, n, r] contiguous: output column n of slot a is row n
 *   scaling       fp32 [slots]: alpha / rank of every slot
 *   adapter_ids   int32 [batch]: the slot of sequence b; any value outside [0, slots) = no adapter (-1 is the canonical value)
 *   cu_seqlens_q  int32 [batch + 1] or NULL: the packed-step contract of awq_attn_prefill_kvcache_varq (Sq_b = cu[b + 1] - cu[b], 0 is legal,
 *                 Sq_b > max_seqlen_q is inactive, rows >= cu[batch] are padding).  NULL = rectangular: sequence b owns rows b max_seqlen_q ..
 *                 (b + 1) max_seqlen_q - 1 and total_q must equal batch * max_seqlen_q (AWQ_ERR_BATCH)
 *   slice_end     HOST ints [n_slices]: slice j is output columns [slice_end[j - 1], slice_end[j]), multiples of 16, strictly increasing, last == n
 *   y             T [total_q, n] contiguous, updated in place (the base linear's output)
 *   workspace     fp32 [KS, total_q, rs], awq_lora_workspace_bytes: the K-split partials carried from shrink to expand
 * For every row t of an active sequence b with 0 <= a = adapter_ids[b] < slots:
 *   shrink: workspace[s, t, c] = sum over the k of split s of f32(x[t, k]) f32(A_a[c, k]), fp32, c < rs
 *   expand: hT[t, c] = T(scaling[a] * (workspace[0, t, c] + workspace[1, t, c] + ... in this order)): one fp32 product, one nearest-even rounding;
 *           y[t, n] = T(f32(y[t, n]) + sum_{i < r} f32(hT[t, j(n) r + i]) f32(B_a[n, i])): the fp32 delta is NOT rounded before the add
 * Every other row (padding, no adapter, inactive or empty sequence) keeps every bit of y; its x is not read, its workspace rows are neither written
 * nor read; pool slots no active sequence names are not read.  KS and the order of every sum depend on (k, rs) alone, so a row's bits do not depend
 * on the batch it is served in.  No atomics, no host read, bit-stable from run to run; both launches can be captured.  A row index formed from
 * cu_seqlens_q is clamped into [0, total_q - 1] before it forms an address and every write is guarded.
 * Limits, checked before anything is launched: r in {16, 32, 64}, n_slices in {1, 2, 3}, k >= 64, k % 64 == 0, n % 16 == 0, ldx and slice_end as
 * above (AWQ_ERR_SHAPE); 1 <= batch <= 65535, 1 <= max_seqlen_q <= 1048560, total_q >= 1, slots >= 1 (AWQ_ERR_BATCH); workspace_bytes
 * (AWQ_ERR_WORKSPACE); x / a_pool / b_pool / y / workspace 16-byte, the int32 and fp32 vectors 4-byte aligned (AWQ_ERR_ALIGN).
 * awq_lora_plan (host only): out[4] = {KS, k per split, output columns per expand block, waves per block}; split s sums k in
 * [s out[1], min(k, (s + 1) out[1])).  awq_lora_workspace_bytes (host only): 0 for sizes outside the limits. ---- */
int awq_lora_plan(int k, int r, int n_slices, int out[4]);
size_t awq_lora_workspace_bytes(int total_q, int k, int r, int n_slices);
int awq_lora_shrink(const void* x, long ldx, const void* a_pool, const int* adapter_ids, const int* cu_seqlens_q, void* workspace,
                    size_t workspace_bytes, int batch, int max_seqlen_q, int total_q, int slots, int k, int r, int n_slices, int dtype, void* stream);
int awq_lora_expand(const void* workspace, size_t workspace_bytes, const void* b_pool, const float* scaling, const int* adapter_ids,
                    const int* cu_seqlens_q, void* y, int batch, int max_seqlen_q, int total_q, int slots, int n, int k, int r, const int* slice_end,
                    int n_slices, int dtype, void* stream);

/* The expand launch on QuantLlamaMLP's gate / up pair, fused with the SiLU * mul tail (F = n2 / 2, two slices: 0 = gate, 1 = up):
 *   workspace     the shrink launch's fp32 [KS, total_q, 2 r] with n_slices = 2 (gate's A rows first)
 *   b_pool        T [slots, n2, r] in natural order: rows 0 .. F - 1 are B_gate, rows F .. 2F - 1 are B_up
 *   y2            T [total_q, n2] contiguous, READ ONLY: the output of the 8 + 8 interleaved gate / up stream without its epilogue -- columns
 *                 16 j .. 16 j + 7 are gate rows 8 j .., columns 16 j + 8 .. 16 j + 15 the matching up rows
 *   h             T [total_q, F] contiguous, written
 * For every row t of an active sequence b and every f < F, j = f / 8, c = f % 8:
 *   with 0 <= a = adapter_ids[b] < slots:  g' = T(f32(y2[t, 16 j + c]) + sum_i f32(hT[t, i]) f32(B_a[f, i])),
 *                                          u' = T(f32(y2[t, 16 j + 8 + c]) + sum_i f32(hT[t, r + i]) f32(B_a[F + f, i]))   (hT as in awq_lora_expand)
 *   otherwise:                             g' = y2[t, 16 j + c], u' = y2[t, 16 j + 8 + c]; no workspace row, pool slot or scaling entry is read
 *   h[t, f] = T(T(silu(g')) u'), the library's one SiLU * mul tail.
 * The bits are those of awq_lora_expand with slice_end = {F, 2F} on the de-interleaved pair followed by awq_silu_mul (F % 16 == 8: with each slice
 * zero-padded to a multiple of 16 columns, which that call asks of its slice ends).  Rows of inactive or empty
 * sequences and padding rows: y2 is not read, h is not written.  Grid from host arguments only, no atomics, no host read; can be captured.
 * Limits and error codes as awq_lora_expand with n = n2 and n_slices = 2 (n2 >= 16, n2 % 16 == 0); y2 / h 16-byte aligned. ---- */
int awq_lora_expand_gate_up(const void* workspace, size_t workspace_bytes, const void* b_pool, const float* scaling, const int* adapter_ids,
                            const int* cu_seqlens_q, const void* y2, void* h, int batch, int max_seqlen_q, int total_q, int slots, int n2, int k,
                            int r, int dtype, void* stream);

/* ---- AWQ quantisation: the asymmetric per-group grid of the reference's pseudo_quantize_tensor(zero_point=True)
 * (awq/quantize/quantizer.py:61-103) evaluated as torch evaluates it on T tensors -- every operation in fp32 on T values and rounded to T
 * (nearest-even, fp16 subnormals kept) before the next one, IEEE division, no fused multiply-add across two of torch's roundings.  DESIGN.md
 * "AWQ quantisation" holds the contract.  Group size 128 only (AWQ_ERR_GROUP), n_bit 3 or 4 (AWQ_ERR_BITS), k % 128 == 0, n >= 1.  Inputs must be
 * finite and every group's hi - lo finite in T: nothing checks it.  Row limit (one grid dimension holds the row tiles): n <= 1 048 560 for
 * awq_quantize_group, n <= 2 097 120 for awq_clip_search (AWQ_ERR_SHAPE above).  No workspace, no atomics, no host read: both calls can be captured.
 *
 * awq_quantize_group: one launch per weight matrix.  Per group of 128 along k:  v = round_T(w * col_scale) (col_scale given),
 * v = clamp(v, -clip_max, clip_max) (clip_max given), then the grid.  Every output is optional (NULL = not wanted, left untouched); every
 * element of a requested output is written:
 *   w        T [n, k], row stride ldw elements (ldw >= k, ldw % 8 == 0);  col_scale T [k] or NULL;  clip_max T [n, k/128] or NULL
 *   w_fake   T [n, k] contiguous: the fake-quantised v, divided by col_scale again (round_T(fake / col_scale)) when col_scale is given --
 *            with col_scale one evaluation of the scale search's w_quantize_func(w * s) / s (auto_scale.py:128-148)
 *   scales, scaled_zeros   T [gpad, n], gpad = calculate_zeros_width(k) * 8, pad rows written as zeros; scaled_zeros = -(T(scale) * float(int(zero)))
 *            rounded to T: WQLinear.from_linear's buffers (qmodule.py:155-197)
 *   zeros    T [n, k/128]
 *   qweight  int16 [n/4, k], layout 0 = v2 (n % 8 == 0), 1 = cdna4 (n % 16 == 0; equals awq_repack_v2_to_cdna4 of the v2 output); n_bit 4 only
 *            (a packed 3-bit output is AWQ_ERR_BITS).  The integers are the ones from_linear recovers, round((fake + zero * scale) / scale) in T,
 *            not clamped, low four bits kept.
 * w / col_scale / w_fake / qweight 16-byte aligned, the others 2-byte (AWQ_ERR_ALIGN).
 *
 * awq_clip_search: the reference's auto_clip_layer (awq/quantize/auto_clip.py:11-63) for one weight matrix in one launch.  Per (row, group):
 * m = amax|w|, candidates mv_i = round_T(m * float(1 - i / n_grid)) for i < n_steps (the factor in double, as Python computes it, rounded to fp32;
 * the product in fp32), q_i = the grid on clamp(w, -mv_i, mv_i), err_i = (1/s) sum_t (x_t . q_i - x_t . w)^2 with the products of T values on the
 * matrix cores and everything else in fp32 (the reference sums in T: DESIGN.md says why this differs).  The result is the first i whose err_i is
 * strictly below 1e9 and every earlier one (i = 0 if there is none).  A cell's sum order depends on s alone, not on n or the launch shape.
 *   w  T [n, k], row stride ldw;  x  T [s, k], row stride ldx (a token subsample is a strided view);  ld* >= k, ld* % 8 == 0;  any n >= 1 up to the row limit, s >= 1
 *   best_max_val T [n, k/128] (the bits of mv_i*), best_idx int32 [n, k/128], err fp32 [n, k/128, n_steps] or NULL
 *   1 <= n_steps <= 16, n_grid >= 1 (AWQ_ERR_SHAPE). ---- */
#define AWQ_QWEIGHT_V2 0
#define AWQ_QWEIGHT_CDNA4 1
int awq_quantize_group(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                       void* zeros, void* qweight, int qweight_layout, int n, int k, int group_size, int n_bit, int dtype, void* stream);
/* awq_quantize_group's arithmetic on the HOST, for host memory and without a device: the same source text (csrc/awq_quant_grid.hpp) compiled for the
 * CPU, so the grid can be held to the torch composition where there is no GPU.  Same inputs and outputs (a)-(c); instead of a packed qweight,
 * intweight uint8 [n, k] receives the recovered integers' low four bits.  A reference, not a fast path. */
int awq_quantize_group_host(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                            void* zeros, void* intweight, int n, int k, int group_size, int n_bit, int dtype);
int awq_clip_search(const void* w, long ldw, const void* x, long ldx, void* best_max_val, int* best_idx, float* err, int n, int k, int s,
                    int group_size, int n_bit, int n_grid, int n_steps, int dtype, void* stream);

/* ---- W3A16 ("w3c" tiles): BASELINE.json's INT3 configuration.  The reference has NO packed 3-bit format
 * (awq/quantize/qmodule.py:82-83 raises for w_bit != 4; INT3 exists only as pseudo-quantisation,
 * awq/quantize/quantizer.py:61-103 with n_bit = 3), so the format is this repository's: per 16-row x 128-k tile
 * 64 lanes x 3 words (768 B) = the cdna4 W4 tile of the same integers (0..7) with its fourth word folded into the
 * free bit 3 of every nibble of the other three.  qweight_w3 is int16 [N/4, 3K/4] (N*K*3/8 bytes); scales /
 * scaled_zeros / sz_packed keep the W4 contract.  bf16 and fp16, n % 16 == 0, k % 128 == 0. ---- */
int awq_pack_w3(const void* q_u8 /* u8 [n, k], values 0..7 */, void* qweight_w3, int n, int k, void* stream);
int awq_unpack_w3(const void* qweight_w3, void* out_u8, int n, int k, void* stream);
int awq_dequant_w3(const void* qweight_w3, const void* scales, const void* scaled_zeros, void* out, int n, int k,
                   int group_size, int dtype, void* stream);
/* WQLinear.forward for w_bit = 3.  Every kernel reads the 3-bit tiles natively: m <= 8 streams them through the decode GEMV;
 * larger m runs the prefill tile kernels whose weight producer loads three words per lane and rebuilds the fourth (no expanded
 * copy).  `workspace` is OPTIONAL (NULL / 0 is always accepted): awq_w3a16_forward_workspace_bytes is the fp32 split-K
 * scratch that lets short prompts on narrow projections fill the chip, 0 for m <= 8 and for launches that already do. */
size_t awq_w3a16_forward_workspace_bytes(int m, int n, int k);
int awq_w3a16_forward(const void* x, const void* qweight_w3, const void* scales, const void* scaled_zeros,
                      const void* sz_packed, const void* bias, void* out, int m, int n, int k, int group_size, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- Tensor-parallel row split (K-sharded WQLinear; SURVEY.md 8(e): new capability, the reference has no multi-GPU path for
 * awq/quantize/qmodule.py:201-224).  Rank r holds the k range [k0, k1) of the cdna4 buffers and computes
 *     out_f32[m, n] = x[:, k0:k1] . W[:, k0:k1]^T        fp32 accumulators, UNROUNDED, no bias
 * with the same kernels as the unsharded forward (decode streaming / skinny / prefill tiles by m); the ranks' partials are summed in fp32
 * (awq_oneshot_allreduce_f32 for the latency-class messages, RCCL on the float tensor above that) and rounded to T ONCE, then the bias
 * is added in T -- what the single-device kernel does with its one accumulator, so the sharded output stays within the 1e-3 budget of
 * the single-device result in bf16 as well (T-rounded partials: 2.6-2.9e-3).  sz_half is optional (NULL = read sz_packed). ---- */
int awq_w4a16_partial_cdna4(const void* x, const void* qweight_cdna4, const void* sz_packed, const void* sz_half, float* out_f32, int m,
                            int n, int k, int group_size, int dtype, void* stream);
/* QuantLlamaMLP's gate / up pair + SiLU * mul (tinychat/modules/fused_mlp.py:33-83) for 3-bit projections: qweight_w3_interleaved holds the
 * two projections' INTEGER rows interleaved 8 + 8 per 16-row slab (gate rows 8 j .. 8 j + 7, then the matching up rows) packed into w3c
 * tiles, sz_packed the same interleave of their scales / zeros; out[m, n2 / 2] = T(T(silu(T(gate))) * T(up)).  m <= 8: the register-ring
 * decode kernel pairs the rows in its epilogue; 9 .. 64 rows: the skinny kernel's paired epilogue; above that the prefill tiles' fused tail.  workspace: optional split-K scratch (NULL / 0 ok). */
size_t awq_w3a16_mlp_gate_up_forward_workspace_bytes(int m, int n2, int k);
int awq_w3a16_mlp_gate_up_forward(const void* x, const void* qweight_w3_interleaved, const void* sz_packed, void* out, int m, int n2, int k,
                                  int group_size, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a 3-bit layer (w3c tiles, awq_pack_w3_from_v1; the reference's w_bit = 3 is NotImplemented at
 * awq/quantize/qmodule.py:95-96, so the sharded form is new as well): m <= 8 the register-ring decode kernel with an fp32
 * epilogue, above that the prefill tiles' fp32 epilogue. */
int awq_w3a16_partial(const void* x, const void* qweight_w3, const void* sz_packed, float* out_f32, int m, int n, int k,
                      int group_size, int dtype, void* stream);
/* out[m, n] = T(in_f32[m, n]) (+ bias[n] in T; may be NULL): the single rounding after an RCCL sum of the partials.  n % 8 == 0. */
int awq_round_bias_f32(const float* in_f32, const void* bias, void* out, int m, int n, int dtype, void* stream);

/* ---- One-shot all-reduce (sum, fp32 accumulation in rank order, one rounding to T) for the latency-class messages of
 * K-sharded decode: M * N * 2 bytes = 8 .. 16 KiB after o_proj / down_proj (the reference has no multi-GPU path).
 * Every rank owns one exchange buffer (awq_oneshot_alloc: fine-grained device memory, awq_oneshot_buffer_bytes(world, max_bytes)
 * bytes), exports it with awq_oneshot_ipc_export (a 64-byte hipIpc handle) and opens its peers' with awq_oneshot_ipc_open;
 * peer_buffers[q] is rank q's buffer as mapped in THIS process (peer_buffers[rank] = the local allocation).  A call stores
 * `in` (count elements, count % 8 == 0, count * 2 <= max_bytes) into every rank's buffer over xGMI, raises one flag per peer and
 * reduces locally when the `world` flags of this round have arrived.  `round` must be 1, 2, 3, ... in call order and equal on
 * all ranks, or 0 on every call of a communicator: the epoch then lives in the rank's own buffer and advances by one per call, which
 * is what a captured and replayed hipGraph needs (its kernel arguments are frozen); the two modes must not be mixed on one buffer set.  *status_dev (optional device int) is set to 1 if a peer's flag did not arrive within the spin bound (the kernel
 * returns instead of hanging the queue).  world <= 8.  Messages above max_bytes belong to RCCL (bandwidth-bound). ---- */
size_t awq_oneshot_buffer_bytes(int world, int max_bytes);
int awq_oneshot_alloc(void** buffer, int world, int max_bytes);
int awq_oneshot_free(void* buffer);
int awq_oneshot_ipc_export(void* buffer, void* handle64);
int awq_oneshot_ipc_open(const void* handle64, void** buffer);
int awq_oneshot_ipc_close(void* buffer);
int awq_oneshot_allreduce(void* const* peer_buffers, const void* in, void* out, int count, int dtype, int rank, int world,
                          unsigned round, int max_bytes, int* status_dev, void* stream);
/* The same exchange on fp32 partials (count floats, count * 4 <= max_bytes): out = T(sum over ranks, fp32, rank order) (+ bias in T, bias_n =
 * its length, count % bias_n == 0; NULL = none).  A communicator serves both forms; a call after *status_dev was set poisons its output. */
int awq_oneshot_allreduce_f32(void* const* peer_buffers, const float* in_f32, const void* bias, int bias_n, void* out, int count, int dtype,
                              int rank, int world, unsigned round, int max_bytes, int* status_dev, void* stream);
/* Spin bound of the flag wait (polls of ~1 us; default 40 M: a peer may be tens of seconds late before the round is declared lost). */
int awq_oneshot_set_spin_limit(unsigned spins);
/* Single-GPU self-test of the device protocol: ONE launch of `world` co-resident blocks, block r playing rank r against the
 * others on `world` exchange buffers of the same device (in_all / out_all: [world][count]).  Tests only. */
int awq_oneshot_allreduce_selftest(void* const* peer_buffers, const void* in_all, void* out_all, int count, int dtype, int world,
                                   unsigned round, int max_bytes, int* status_dev, void* stream);

int awq_oneshot_allreduce_f32_selftest(void* const* peer_buffers, const float* in_all_f32, const void* bias, int bias_n, void* out_all, int count,
                                       int dtype, int world, unsigned round, int max_bytes, int* status_dev, void* stream);

/* ---- Decode attention over the FasterTransformer KV cache (tinychat's single_query_attention, ft_attention.cpp:112-185).
 * One decode step of multi-head / grouped-query attention:
 *     q [B, H, Dh], k / v [B, Hkv, Dh] (own batch strides, in elements; heads contiguous), out [B, H, Dh] contiguous
 *     k_cache [Bc, Hkv, Dh/8, Lmax, 8], v_cache [Bc, Hkv, Lmax, Dh] (contiguous; rows b < B are used), B <= Bc
 * tlength = length_per_sample[b] (device int32 [B], may be NULL) or timestep; positions max(0, tlength + 1 - Lmax) .. tlength are
 * attended at cache index pos % Lmax; the rotated k and v of the current token are written at tlength % Lmax (nothing else is).
 * rotary_dim 0 = none, neox != 0 = rotate-half, else GPT-J interleaved; alibi_slopes fp32 [H] or NULL.  With a length tensor,
 * `timestep` is the host-side upper bound that sizes the context split.  T = fp16 / bf16 (`dtype`), 32 <= Dh <= 256, Dh % 16 == 0.
 * Softmax weights and P.V stay in fp32; the output is bit-deterministic (csrc/awq_attn_cdna4.hip).
 * Returns AWQ_ERR_SHAPE (head dim, H % Hkv, B > Bc, odd or too large rotary_dim, timestep < 0, ...), AWQ_ERR_DTYPE, AWQ_ERR_NULL,
 * AWQ_ERR_ALIGN (16 bytes for the tensors and the strides, 4 for lengths / slopes), AWQ_ERR_WORKSPACE, AWQ_ERR_LAUNCH. */
/* Host-side plan: the context is cut into *splits chunks of *chunk positions (one launch of B * Hkv * splits blocks, plus a
 * combine launch when *splits > 1).  Depends on these host arguments only. */
int awq_attn_decode_plan(int batch, int nheads_kv, int head_dim, int timestep, int lmax, int* splits, int* chunk);
/* fp32 partials of the split plan: 0 when the plan has one split (workspace may then be NULL). */
size_t awq_attn_decode_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int timestep, int lmax);
int awq_attn_decode(const void* q, const void* k, const void* v, void* k_cache, void* v_cache, const int* length_per_sample,
                    const float* alibi_slopes, void* out, int batch, int cache_batch, int nheads, int nheads_kv, int head_dim, int lmax,
                    long long q_batch_stride, long long k_batch_stride, long long v_batch_stride, int timestep, int rotary_dim,
                    float rotary_base, float rotary_scale, int neox, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Prefill attention (flash_attn_func's forward: tinychat llama.py:218, fused_attn.py:477,539).
 *     q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] (own batch and row strides, in elements; heads contiguous: head stride = Dh),
 *     out [B, Sq, H, Dh] contiguous;  O = softmax(softmax_scale * Q K^T + mask) V, plain softmax.
 * causal != 0: query row i attends keys j <= i + (Sk - Sq) (bottom-right aligned; needs Sq <= Sk); causal == 0: every key.
 * H % Hkv == 0, query head h reads KV head h / (H / Hkv).  T = fp16 / bf16 (`dtype`), Dh = 64 or 128, and 72 with causal == 0 (SigLIP's
 * head dim, served by the tower kernel below); Sq and Sk need no alignment, and
 * no row >= Sq of q or >= Sk of k / v is read.  One pass over K / V per q tile with an online softmax on the matrix cores, fp32
 * accumulation; each softmax weight is rounded to T once and that rounded value feeds both P.V and the row sum; O is rounded to T
 * once.  No workspace, no atomics: bit-deterministic and capturable (csrc/awq_attn_prefill_cdna4.hip).
 * Returns AWQ_ERR_SHAPE (head dim, H % Hkv, Sq > Sk with causal, non-positive sizes, a row stride below heads * Dh), AWQ_ERR_DTYPE,
 * AWQ_ERR_NULL, AWQ_ERR_ALIGN (16 bytes for the pointers and the strides), AWQ_ERR_LAUNCH; all but the last without a GPU call. */
/* Host-side plan: one launch of *blocks blocks, each a q tile of *q_tile_rows rows (32, 64, 128 or 256) of one (batch, query head).
 * Depends on these host arguments only; no GPU call. */
int awq_attn_prefill_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* q_tile_rows,
                          int* blocks);
int awq_attn_prefill(const void* q, const void* k, const void* v, void* out, int batch, int seqlen_q, int seqlen_k, int nheads, int nheads_kv,
                     int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                     long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream);

/* ---- Chunk prefill on the FasterTransformer KV cache (tinychat/modules/fused_attn.py:248-302, 439-483): the prompt side in two launches,
 *      with no copy whose size grows with the history.
 *     k_cache [cache_batch, Hkv, Dh/8, lmax, 8], v_cache [cache_batch, Hkv, lmax, Dh], contiguous: the caches awq_attn_decode reads and writes.
 * awq_rope_kv_store: qkv [B, S, (H + 2 Hkv) Dh] (own batch and row strides, in elements; q heads, then k heads, then v heads), freqs fp32
 *     with B * S * rot_dim angles.  q_out [B, S, H, Dh] contiguous <- rotated q; k_cache[b, kvh, ch, start_pos + s, 0..7] <- rotated k;
 *     v_cache[b, kvh, start_pos + s, :] <- v.  The rotation is awq_rope_with_pos's with n0 = B, n1 = S (angle index
 *     (s * B + b) * rot_dim + c, one rounding, columns >= rot_dim copied): the results are bit-identical to two awq_rope_with_pos calls
 *     followed by the stores.  Nothing outside positions [start_pos, start_pos + S) of rows b < B is written; no wrap on the prompt side.
 *     Returns AWQ_ERR_SHAPE (Dh not 64 / 128, rot_dim % 16 != 0 or > Dh, B > cache_batch, start_pos < 0, start_pos + S > lmax, a row
 *     stride below (H + 2 Hkv) Dh, non-positive sizes), AWQ_ERR_DTYPE, AWQ_ERR_NULL, AWQ_ERR_ALIGN (16 bytes for the pointers and the
 *     strides), AWQ_ERR_LAUNCH; all but the last without a GPU call (csrc/awq_attn_chunk_cdna4.hip).
 * awq_attn_prefill_ftcache: awq_attn_prefill with K / V read from the caches: key j of the attention is cache position kv_start + j,
 *     j < seqlen_k.  kv_start = 0, seqlen_k = start_pos + S is chunk prefill; kv_start = start_pos, seqlen_k = S attends the new chunk
 *     only.  q [B, Sq, H, Dh] with its own batch and row strides, out [B, Sq, H, Dh] contiguous.  Same plan (awq_attn_prefill_plan), tile
 *     walk, masks and rounding points: the output is bit-identical to awq_attn_prefill on a contiguous copy of the same keys and values.
 *     No cache position outside [kv_start, kv_start + seqlen_k) and no cache row >= B is read.  No workspace, no atomics; capturable.
 *     Returns the codes of awq_attn_prefill, with AWQ_ERR_SHAPE also for Dh not 64 / 128, kv_start < 0, kv_start + seqlen_k > lmax and
 *     B > cache_batch; all but AWQ_ERR_LAUNCH without a GPU call. */
int awq_rope_kv_store(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int batch, int cache_batch, int seqlen,
                      int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos, long long qkv_batch_stride,
                      long long qkv_row_stride, int dtype, void* stream);
int awq_attn_prefill_ftcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int cache_batch, int seqlen_q,
                             int kv_start, int seqlen_k, int nheads, int nheads_kv, int head_dim, int lmax, long long q_batch_stride,
                             long long q_row_stride, float softmax_scale, int causal, int dtype, void* stream);

/* ---- Split-KV attention (flash-decoding) for few query rows over a long natural-layout history: the decode phase of tinychat's long-context
 *      path (fused_attn.py:389-415, 505-546: flash_attn_func(q, cache_k[:, :pos], cache_v[:, :pos], causal=True) with Sq = 1).
 * awq_attn_splitkv: awq_attn_prefill's contract and arguments, plus a workspace.  Where the plan splits, one block serves one (batch, KV
 *     head, split of *chunk keys): the Sq * G query rows of the KV head's group (G = H / Hkv) share one fetch of K / V, each block writes an
 *     unnormalised fp32 partial (O, running max, row sum) per (row, split), and a second launch combines them in ascending split order
 *     with 2^(m_s - M) weights, one division, one rounding to T.  Same rounding points as awq_attn_prefill inside a split.  No atomics:
 *     bit-deterministic and capturable, workspace included (csrc/awq_attn_splitkv_cdna4.hip).  Where the plan does not split, the call IS
 *     awq_attn_prefill (same launch, same bits) and the workspace may be NULL.
 *     Returns the codes of awq_attn_prefill, plus AWQ_ERR_WORKSPACE (NULL or smaller than awq_attn_splitkv_workspace_bytes; a workspace
 *     that is not 16-byte aligned is AWQ_ERR_ALIGN); all but AWQ_ERR_LAUNCH without a GPU call.
 * awq_attn_splitkv_plan: host only, no GPU call.  *splits == 1: not taken -- always so for seqlen_k < 2048, Sq * G > 128, a head dim other
 *     than 64 / 128, or a one-pass launch (awq_attn_prefill_plan) of at least 256 blocks.  Otherwise *chunk % 64 == 0, *chunk >= 1024,
 *     (*splits - 1) * *chunk < seqlen_k <= *splits * *chunk, and batch * nheads_kv * *splits >= 256 wherever seqlen_k / 1024 allows.
 *     Knob "attn_splitkv_chunk" (awq_tune_set): a multiple of 64 forces the chunk for any seqlen_k (the Sq * G and head dim limits hold).
 * awq_attn_splitkv_workspace_bytes: batch * nheads * seqlen_q * splits * (head_dim + 2) * 4 (fp32 O [n][Dh] | m [n] | l [n], n = batch *
 *     nheads * seqlen_q * splits), 0 when the plan does not split; follows the knob. */
int awq_attn_splitkv_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal, int* splits, int* chunk);
size_t awq_attn_splitkv_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int seqlen_k, int causal);
int awq_attn_splitkv(const void* q, const void* k, const void* v, void* out, int batch, int seqlen_q, int seqlen_k, int nheads, int nheads_kv,
                     int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                     long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* workspace,
                     size_t workspace_bytes, void* stream);
/* awq_rope_kv_store for natural-layout caches k_cache / v_cache [cache_batch, lmax, Hkv, Dh] (tinychat's long_forward, fused_attn.py:527-537),
 * one launch: q_out [B, S, H, Dh] <- rotated q, k_cache[b, start_pos + s, kvh, :] <- rotated k, v_cache[b, start_pos + s, kvh, :] <- v.
 * Same arithmetic and freqs index as awq_rope_with_pos (quirk included): bit-identical to two awq_rope_with_pos calls followed by the two
 * slice stores.  Nothing outside positions [start_pos, start_pos + S) of rows b < B is written.  Same error rules as awq_rope_kv_store
 * (csrc/awq_attn_chunk_cdna4.hip). */
int awq_rope_kv_store_natural(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, int batch, int cache_batch,
                              int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos,
                              long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream);

/* ---- FP8 KV cache on the natural layout (csrc/awq_kv8.hpp).  k_cache / v_cache [cache_batch, lmax, Hkv, Dh] hold one byte per element, an
 *      OCP e4m3fn code (not fnuz); k_scale / v_scale [cache_batch, lmax, Hkv] hold one fp32 scale per (token, KV head).  A head row x of T is
 *      quantised as s = max(max|x|, 2^-60) / 448 (IEEE division), code = e4m3fn_RNE(clamp(x / s, -448, 448)), and dequantised as
 *      T(float(code) * s): one fp32 multiply, one rounding to T.  Head dims 64 and 128.
 * awq_rope_kv_store_natural_fp8: awq_rope_kv_store_natural with quantised stores.  q_out holds awq_rope_kv_store_natural's bits; the K
 *     row that is quantised is the rotated row after its rounding to T (the bits that entry would have stored), the V row is the qkv
 *     tensor's.  Nothing outside positions [start_pos, start_pos + S) of rows b < B is written, in the caches or in the scales.  Same
 *     error rules as awq_rope_kv_store_natural; the scale pointers must be 4-byte aligned (AWQ_ERR_ALIGN) and non-NULL.
 * awq_attn_prefill_kv8 / awq_attn_splitkv_kv8: awq_attn_prefill / awq_attn_splitkv with k / v read from the codes and the scales.  k / v
 *     strides count codes (bytes) and must be multiples of 16, the scale strides count floats (row stride >= Hkv); head dim 72 is
 *     AWQ_ERR_SHAPE.  The kernels dequantise between their global load and their LDS write and are the T kernels behind it: the result
 *     is bit-identical to awq_attn_prefill / awq_attn_splitkv on the dequantised T tensors.  Same plans (awq_attn_prefill_plan,
 *     awq_attn_splitkv_plan), same workspace (awq_attn_splitkv_workspace_bytes), same knobs; where the plan does not split,
 *     awq_attn_splitkv_kv8 IS awq_attn_prefill_kv8.  Every code but AWQ_ERR_LAUNCH is returned without a GPU call. */
int awq_rope_kv_store_natural_fp8(const void* qkv, const float* freqs, void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                  int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                  int start_pos, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream);
int awq_attn_prefill_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, int seqlen_k, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                         long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                         long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                         long long v_scale_row_stride, float softmax_scale, int causal, int dtype, void* stream);
int awq_attn_splitkv_kv8(const void* q, const void* k, const void* v, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, int seqlen_k, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                         long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                         long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                         long long v_scale_row_stride, float softmax_scale, int causal, int dtype, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- The natural-layout decode path with per-sequence lengths read ON THE DEVICE (flash_attn_with_kvcache's cache_seqlens): a batch whose
 *      sequences have different lengths in one call, and one captured graph for the whole decode phase (nothing that changes from token to
 *      token is a launch argument).  The host never reads the length arrays and never synchronises.
 * awq_rope_kv_store_natural_pos[_fp8]: awq_rope_kv_store_natural[_fp8] with cache_seqlens (device int32 [batch], 4-byte aligned: the tokens
 *     already in each sequence's cache) in the place of start_pos, and freqs_table (fp32 [table_rows, rot_dim], contiguous, 16-byte
 *     aligned: the model's whole angle table) in the place of the call's angles.  Token s of sequence b is written at cache position
 *     cache_seqlens[b] + s with the angles freqs_table[(cache_seqlens[b] + s) * rot_dim + c].  The arithmetic is the host-position kernel's,
 *     expression for expression: for every active sequence q_out[b], the written cache rows and scales hold the bits
 *     awq_rope_kv_store_natural[_fp8] leaves when called with batch = 1, start_pos = cache_seqlens[b] and freqs = freqs_table + start_pos *
 *     rot_dim.  A sequence is ACTIVE iff 0 <= cache_seqlens[b] and cache_seqlens[b] + seqlen <= min(lmax, table_rows).  For an inactive
 *     sequence (a finished slot of a static batch, -1, or a corrupt length) nothing is written to the caches or the scales, its q_out rows
 *     are written as zeros and no address outside the tensors is formed.  Error rules of awq_rope_kv_store_natural[_fp8] without those of
 *     start_pos; table_rows < 1 is AWQ_ERR_SHAPE, cache_seqlens NULL is AWQ_ERR_NULL, not 4-byte aligned AWQ_ERR_ALIGN.
 * awq_attn_kvcache[_kv8]: the split-KV kernel pair of awq_attn_splitkv[_kv8] with seqlen_k replaced by seqlens_k (device int32 [batch],
 *     4-byte aligned), seqlen_offset (a host int added to every entry: pass seqlen_q with the cache_seqlens the store launch took, 0 when
 *     the caller holds total lengths) and max_seqlen_k (the host bound that sizes the plan, as timestep does in awq_attn_decode).  k_cache /
 *     v_cache are the caches [>= batch, lmax, Hkv, Dh] with their batch and row strides; max_seqlen_k <= lmax.
 *     Sk_b = seqlens_k[b] + seqlen_offset; sequence b is ACTIVE iff 1 <= Sk_b <= max_seqlen_k.  The causal mask is bottom-right aligned per
 *     sequence: row i attends keys j <= i + Sk_b - seqlen_q; a row whose limit is negative (Sk_b < seqlen_q) attends nothing and returns
 *     zeros; an inactive sequence returns zeros and nothing of its cache rows is read.  No NaN or Inf is produced from finite attended
 *     inputs, and the combine never divides by L = 0.  Cache rows >= Sk_b are never read.
 *     ALWAYS the split pair: seqlen_q * (nheads / nheads_kv) <= 128 and head_dim 64 / 128 are requirements (AWQ_ERR_SHAPE otherwise); a
 *     longer prompt goes through the host-length entries.  Both launches run for any *splits, 1 included.  A block whose split begins at
 *     or beyond Sk_b, or whose sequence is inactive, writes m = -inf, l = 0 and leaves before its first load of K / V: a ragged batch
 *     costs what its lengths cost.  The per-split arithmetic is awq_attn_splitkv's and the combine skips m = -inf partials in ascending
 *     order, so for every active sequence with Sk_b > *chunk, out[b] is bit-identical to awq_attn_splitkv on that sequence alone (batch
 *     1, seqlen_k = Sk_b) under the same forced chunk; the _kv8 form is bit-identical to the T form on the dequantised caches.  No atomics:
 *     bit-deterministic and capturable, workspace included.
 *     Returns the codes of awq_attn_splitkv[_kv8], all but AWQ_ERR_LAUNCH without a GPU call; in addition AWQ_ERR_NULL for seqlens_k,
 *     AWQ_ERR_ALIGN when it is not 4-byte aligned, AWQ_ERR_SHAPE for max_seqlen_k < 1, max_seqlen_k > lmax or seqlen_offset < 0.  The
 *     workspace is always needed (AWQ_ERR_WORKSPACE when NULL or smaller than awq_attn_kvcache_workspace_bytes).
 * awq_attn_kvcache_plan: host only, made from the bound alone (never from a length).  awq_attn_splitkv_plan's chunk rule -- two blocks per
 *     CU, *chunk % 64 == 0, *chunk >= 1024 -- without the 2048-key floor and the one-pass test: *splits >= 1, *splits * *chunk >=
 *     max_seqlen_k.  The rule counts the nheads_kv groups of ONE sequence: batch is validated but does not enter, because any sequence
 *     of a ragged batch may be the only long one.  Follows the knob "attn_splitkv_chunk".
 * awq_attn_kvcache_workspace_bytes: batch * nheads * seqlen_q * splits * (head_dim + 2) * 4; 0 for a shape the plan refuses. */
int awq_rope_kv_store_natural_pos(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens,
                                  int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                  int table_rows, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_natural_pos_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, float* k_scale,
                                      float* v_scale, const int* cache_seqlens, int batch, int cache_batch, int seqlen, int nheads,
                                      int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_batch_stride,
                                      long long qkv_row_stride, int dtype, void* stream);
int awq_attn_kvcache_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k, int* splits, int* chunk);
size_t awq_attn_kvcache_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_seqlen_k);
int awq_attn_kvcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int seqlen_q, const int* seqlens_k,
                     int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_batch_stride,
                     long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                     float softmax_scale, int causal, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_kvcache_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out, int batch,
                         int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                         long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                         long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- The same decode path over a PAGED KV cache (flash_attn_with_kvcache's block_table): a pool of fixed-size pages and a per-sequence
 *      block table in the place of the dense [batch, lmax, Hkv, Dh] rectangle, so a sequence holds the pages its tokens need and a finished
 *      slot holds none.  Nothing about the table or the lengths reaches the host: capturable, and a replay follows the table's contents.
 * Pool: k_pool / v_pool [num_pages, page_size, Hkv, Dh] of T (the _fp8 / _kv8 entries: e4m3 codes) with a page stride and a row stride each,
 *     in elements (codes: bytes), heads contiguous; the scale pools k_scale / v_scale [num_pages, page_size, Hkv] fp32 with a page and a row
 *     stride each, in floats.  page_size >= 64 and page_size % 64 == 0 (the key tile of the kernels is 64 keys and every chunk is a multiple
 *     of 64, so a tile never straddles a page).
 * Table: block_table, device int32 [batch, pages_per_seq], 4-byte aligned, row stride table_row_stride >= pages_per_seq (entries).  Logical
 *     position p of sequence b is row p % page_size of page block_table[b * table_row_stride + p / page_size].  A page id is clamped into
 *     [0, num_pages) before it forms an address, so no address outside the pools is ever formed; the result for a sequence with such an
 *     entry inside its live range is unspecified.  No entry at index >= ceil(Sk_b / page_size) (store: >= ceil((pos_b + seqlen) /
 *     page_size)) is read.  Two sequences may name the same page (a shared prefix): the attention only reads.
 * awq_rope_kv_store_paged_pos[_fp8]: awq_rope_kv_store_natural_pos[_fp8] writing token s of sequence b at logical position p =
 *     cache_seqlens[b] + s through the table, the page looked up per token (a chunk may cross page edges).  A sequence is ACTIVE iff
 *     0 <= cache_seqlens[b] and cache_seqlens[b] + seqlen <= min(pages_per_seq * page_size, table_rows); an inactive sequence gets zero
 *     q_out rows and nothing else.  The pool rows (and scale rows) the table names hold the bits awq_rope_kv_store_natural_pos[_fp8] leaves
 *     in the dense cache, q_out is that entry's, and no other byte of the pools or the scale pools is written.
 * awq_attn_kvcache_paged[_kv8]: awq_attn_kvcache[_kv8] with the K / V rows and the scales fetched through the table: same plan
 *     (awq_attn_kvcache_plan from max_seqlen_k alone), same workspace (awq_attn_kvcache_workspace_bytes), same combine launch, empty-block
 *     rule, masks and rounding points.  For every active sequence out[b] is bit-identical to awq_attn_kvcache[_kv8] on the dense gather
 *     cache[b, p] = pool[block_table[b, p / page_size], p % page_size] under the same (forced or planned) chunk.  The page id of a 64-key
 *     tile is one scalar load, issued a tile ahead of the K / V loads that use it.  No atomics: bit-deterministic, workspace included.
 * Returns the codes of the dense entries (without those of cache_batch and lmax), all but AWQ_ERR_LAUNCH without a GPU call; in addition
 *     AWQ_ERR_NULL for block_table, AWQ_ERR_ALIGN when it is not 4-byte aligned or a pool stride is not a multiple of 16 bytes,
 *     AWQ_ERR_SHAPE for page_size < 64 or page_size % 64 != 0, num_pages < 1, pages_per_seq < 1, table_row_stride < pages_per_seq, a negative
 *     page stride, a row stride below Hkv * Dh (scales: below Hkv) and, for the attention, max_seqlen_k > pages_per_seq * page_size. */
int awq_rope_kv_store_paged_pos(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, const int* block_table,
                                const int* cache_seqlens, int batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_paged_pos_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, float* k_scale,
                                    float* v_scale, const int* block_table, const int* cache_seqlens, int batch, int seqlen, int nheads,
                                    int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                    long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                    long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                    long long v_scale_page_stride, long long v_scale_row_stride, long long qkv_batch_stride,
                                    long long qkv_row_stride, int dtype, void* stream);
int awq_attn_kvcache_paged(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch, int seqlen_q,
                           const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq,
                           long long table_row_stride, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, float softmax_scale,
                           int causal, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_kvcache_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                               const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                               int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                               int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                               long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- Shared-prefix decode on the paged cache: the sequences of a GROUP hold the same keys below a common prefix (one system prompt, the n
 *      samples of a request, beams) and the prefix is fetched ONCE for the group, with the query rows of all members in one MFMA tile.
 * awq_attn_kvcache_paged_shared[_kv8]: the arguments of awq_attn_kvcache_paged[_kv8], and
 *     group_members  device int32 [num_groups, group_cap], row stride members_row_stride >= group_cap (entries), -1 padding
 *     group_prefix   device int32 [num_groups]: the tokens group g shares
 *     seq_prefix     device int32 [batch]: the tokens sequence b shares with its group; below 64: ungrouped
 *     num_groups >= 1, group_cap >= 1 with group_cap * seqlen_q * (nheads / nheads_kv) <= 128; max_prefix % 64 == 0 and
 *     64 <= max_prefix <= max_seqlen_k, the host bound of every effective prefix.
 *   Sk_b = seqlens_k[b] + seqlen_offset, b ACTIVE iff 1 <= Sk_b <= max_seqlen_k.  The effective prefix of P tokens for a sequence of Sk keys
 *     is pfx(P, Sk) = min(P, max_prefix, max(0, Sk - seqlen_q)) & ~63, and 0 for P < 64.
 *   Suffix: P_b = pfx(seq_prefix[b], Sk_b).  Suffix split s owns keys [P_b + s * chunk_s, min(Sk_b, P_b + (s + 1) * chunk_s)), read through
 *     b's own table row with the masks, clamps, empty-block rule and rounding points of awq_attn_kvcache_paged.  No key, scale or table
 *     entry of b below P_b is read.
 *   Prefix: the LEAD of group g is its first member in list order that is a slot index in [0, batch) and active; P_g =
 *     pfx(group_prefix[g], Sk_lead).  Without a lead, or with P_g = 0, the group's blocks write nothing.  Prefix split s owns keys
 *     [s * chunk_p, min(P_g, (s + 1) * chunk_p)), read through the lead's table row ONLY; every row attends every key of it (the prefix
 *     lies below every causal limit; P_g % 64 == 0 leaves nothing to clamp).  MFMA row (j * seqlen_q + i) * G + gh is query position i,
 *     head gh of the KV head's group, of member j; it is stored, into the workspace rows of that member's slot, only when the member is a
 *     valid, active slot.
 *   Combine: awq_attn_kvcache's rule (partials with m = -inf skipped, ascending order, one division, zeros when nothing was attended) over
 *     the first ceil(P_b / chunk_p) prefix splits, then all suffix splits.
 *   Defined results.  Required of every active b with seq_prefix[b] >= 64: b is listed in exactly one group; that group's group_prefix
 *     equals seq_prefix[b] and is <= Sk_m - seqlen_q for every active member m; the members' keys below the prefix hold the same values
 *     (normally the same page ids).  Then out[b] is the function awq_attn_kvcache_paged computes for b.  A row's partial depends only on
 *     its q row, its keys and the split boundaries -- not on the other rows of its tile nor on whose table named the pages -- so with
 *     chunk_p == chunk_s == c and P_b % c == 0 out[b] is BIT-IDENTICAL to awq_attn_kvcache_paged[_kv8] under chunk c.  An ungrouped
 *     sequence gets awq_attn_kvcache_paged's bits under chunk_s.  A violated requirement gives unspecified values for the sequences
 *     involved and never an address outside a tensor: every index taken from a device array is clamped or guarded before it forms one.
 *   Plan: awq_attn_kvcache_shared_plan gives (splits_p, chunk_p) = awq_attn_kvcache_plan's rule for the bound max_prefix and (splits_s,
 *     chunk_s) = the rule for max_seqlen_k; the knob attn_splitkv_chunk forces both chunks.  Workspace: batch * nheads * seqlen_q *
 *     (splits_p + splits_s) * (head_dim + 2) * 4 bytes (awq_attn_kvcache_shared_workspace_bytes), 16-byte aligned.
 *   Three launches, their set and grids from host arguments only: num_groups * Hkv * splits_p prefix blocks, batch * Hkv * splits_s suffix
 *     blocks, the combine.  No atomics, no host read; capturable, a replay follows in-place changes of lengths, tables and group arrays.
 *   Returns the codes of awq_attn_kvcache_paged[_kv8], and AWQ_ERR_NULL for a null group array, AWQ_ERR_ALIGN for one that is not 4-byte
 *     aligned, AWQ_ERR_SHAPE for num_groups < 1, group_cap < 1, members_row_stride < group_cap, group_cap * seqlen_q * G > 128 or a
 *     max_prefix that is not a multiple of 64 in [64, max_seqlen_k]; all of them before any launch.
 * awq_kv_page_copy[_fp8]: ONE launch copies the K and V rows (and, _fp8, the K and V scale rows) of n pages inside the pools: page
 *     dst_pages[i] := page src_pages[i], both device int32 [n], 4-byte aligned.  A pair with an id outside [0, num_pages) or with equal
 *     ids is skipped.  K / V moves are 16 bytes wide; page and row strides are honoured and no other byte is written.  A page that is both
 *     a source and a destination of one call gives unspecified contents.  Capturable.  This is the copy-on-write of the partly filled tail
 *     page of a fork.  AWQ_ERR_NULL / AWQ_ERR_SHAPE (n < 1, the pool terms above, head_dim not 64 / 128) / AWQ_ERR_ALIGN as above. */
int awq_attn_kvcache_shared_plan(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix, int max_seqlen_k,
                                 int* splits_p, int* chunk_p, int* splits_s, int* chunk_s);
size_t awq_attn_kvcache_shared_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int seqlen_q, int max_prefix,
                                               int max_seqlen_k);
int awq_attn_kvcache_paged_shared(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                                  int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size,
                                  int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                  long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                                  long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype,
                                  const int* group_members, const int* group_prefix, const int* seq_prefix, int num_groups, int group_cap,
                                  long long members_row_stride, int max_prefix, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_kvcache_paged_shared_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                      const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                                      int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                                      int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride,
                                      long long k_row_stride, long long v_page_stride, long long v_row_stride, long long k_scale_page_stride,
                                      long long k_scale_row_stride, long long v_scale_page_stride, long long v_scale_row_stride,
                                      float softmax_scale, int causal, int dtype, const int* group_members, const int* group_prefix,
                                      const int* seq_prefix, int num_groups, int group_cap, long long members_row_stride, int max_prefix,
                                      void* workspace, size_t workspace_bytes, void* stream);
int awq_kv_page_copy(void* k_pool, void* v_pool, const int* src_pages, const int* dst_pages, int n, int num_pages, int page_size, int nheads_kv,
                     int head_dim, long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, void* stream);
int awq_kv_page_copy_fp8(void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* src_pages, const int* dst_pages, int n,
                         int num_pages, int page_size, int nheads_kv, int head_dim, long long k_page_stride, long long k_row_stride,
                         long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                         long long v_scale_page_stride, long long v_scale_row_stride, void* stream);

/* ---- Prompt chunks of any length on the device-length and paged caches: the ONE-PASS prefill kernel of awq_attn_prefill[_kv8] with every
 *      sequence's length read on the device, K / V from the dense caches or fetched from the pool through the table.  The arguments are
 *      those of awq_attn_kvcache[_kv8] / awq_attn_kvcache_paged[_kv8] without the workspace; seqlen_q >= 1 of ANY size (the split pair above
 *      keeps its seqlen_q * (nheads / nheads_kv) <= 128), head_dim 64 / 128.
 * Length: Sk_b = seqlens_k[b] + seqlen_offset; sequence b is ACTIVE iff 1 <= Sk_b <= max_seqlen_k.  The causal mask is bottom-right aligned
 *     per sequence: row i attends keys j <= i + Sk_b - seqlen_q; causal = 0 attends keys 0 .. Sk_b - 1.  A row whose limit is negative
 *     (Sk_b < seqlen_q) attends nothing and returns zeros; no NaN or Inf is produced from finite attended inputs and nothing divides by 0.
 * Inactive sequences and unused tiles: a block of an inactive sequence, or one whose q tile attends no key, writes zero rows for its q
 *     tile and leaves before its first K / V load; a block visits no 64-key tile behind the last key its q tile attends; cache or pool
 *     rows >= Sk_b are never read (addresses are clamped to row Sk_b - 1).
 * Grid: from host arguments only -- awq_attn_prefill_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, ..) ignores seqlen_k, so the q
 *     tile and the block count are the host-length launch's and the knob "attn_prefill_rows" applies.  No workspace, no atomics:
 *     bit-deterministic and capturable; a replay follows the lengths (and the table) the tensors hold then.
 * Paged: the pool and table rules above.  Tiles begin at multiples of 64 from key 0, so a tile has one page; its id is a scalar load issued
 *     a tile ahead of the K / V loads that use it, clamped into [0, num_pages); no entry at or behind ceil(Sk_b / page_size) is read, the
 *     look-ahead included.  _kv8: codes and scale pools go through the same page id.
 * Bits: tile walk, masks, LDS images and rounding points are awq_attn_prefill's.  For every active sequence with Sk_b >= seqlen_q, out[b]
 *     is bit-identical to awq_attn_prefill[_kv8] on that sequence alone (batch 1, seqlen_k = Sk_b, k / v = its cache rows or the gather
 *     of its pages) under the same q tile.
 * Returns the codes of awq_attn_kvcache[_kv8] / awq_attn_kvcache_paged[_kv8], all but AWQ_ERR_LAUNCH without a GPU call, with two
 *     differences: seqlen_q * (nheads / nheads_kv) > 128 is accepted (AWQ_ERR_SHAPE only when batch * nheads * ceil(seqlen_q / 64) exceeds
 *     2^31 - 1), and AWQ_ERR_WORKSPACE is never returned. */
int awq_attn_prefill_kvcache(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, int seqlen_q, const int* seqlens_k,
                             int seqlen_offset, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_batch_stride,
                             long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                             long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream);
int awq_attn_prefill_kvcache_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                                 int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int lmax, int nheads,
                                 int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride, long long k_batch_stride,
                                 long long k_row_stride, long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride,
                                 long long k_scale_row_stride, long long v_scale_batch_stride, long long v_scale_row_stride,
                                 float softmax_scale, int causal, int dtype, void* stream);
int awq_attn_prefill_paged(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch, int seqlen_q,
                           const int* seqlens_k, int seqlen_offset, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq,
                           long long table_row_stride, int nheads, int nheads_kv, int head_dim, long long q_batch_stride, long long q_row_stride,
                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride, float softmax_scale,
                           int causal, int dtype, void* stream);
int awq_attn_prefill_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                               const int* block_table, int batch, int seqlen_q, const int* seqlens_k, int seqlen_offset, int max_seqlen_k,
                               int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv,
                               int head_dim, long long q_batch_stride, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                               long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                               void* stream);

/* ---- Continuous batching ("varq"): per-sequence numbers of NEW tokens on the KV-cache path.  The tokens of a step are PACKED: one flat run
 *      of rows in which sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1.  One store launch and one attention launch serve any
 *      mix -- decodes of one token, prompt chunks, the tail of a prompt -- and one captured graph replays every step of a fixed token budget.
 * The packed step (all eight entries):
 *     cu_seqlens_q  device int32 [batch + 1], 4-byte aligned, non-decreasing, cu[0] = 0 (taken for granted).  The host never reads it.
 *     Sq_b          cu[b + 1] - cu[b].  0 is legal -- a slot with nothing to do: nothing of that sequence is read or written.
 *     total_q       (host) rows of the packed tensors, cu[batch] <= total_q.  Rows >= cu[batch] are the padding of a fixed token budget and
 *                   belong to nobody: neither launch reads or writes them.
 *     max_seqlen_q  (host) bounds every Sq_b and sizes the attention grid.  batch <= 65535.
 *     Every row index formed from cu_seqlens_q is clamped into [0, total_q - 1] before it forms an address and every write is guarded by
 *     row < min(cu[b + 1], total_q): a corrupt array gives unspecified results, never an address outside the tensors (awq_attn_varlen's rule).
 *
 * awq_attn_prefill_kvcache_varq[_kv8] / awq_attn_prefill_paged_varq[_kv8]: awq_attn_prefill_kvcache[_kv8] / awq_attn_prefill_paged[_kv8] with
 *     q [total_q, nheads, head_dim] under a row stride (elements; heads contiguous) and out [total_q, nheads, head_dim] contiguous;
 *     (batch, seqlen_q) replaced by (batch, cu_seqlens_q, max_seqlen_q, total_q); seqlen_offset replaced by the flag lens_before_step.
 * Length: lens_before_step != 0: Sk_b = seqlens_k[b] + Sq_b -- seqlens_k is then the cache_seqlens the store launch took; 0: Sk_b =
 *     seqlens_k[b], total lengths.  The sum is formed in 64 bits.  Sequence b is ACTIVE iff 0 <= Sq_b <= max_seqlen_q and
 *     1 <= Sk_b <= max_seqlen_k.
 * Mask: causal: row s of sequence b attends keys j <= s + Sk_b - Sq_b; a row with a negative limit returns zeros.  causal = 0 attends keys
 *     0 .. Sk_b - 1.
 * Inactive sequences: rows s < min(Sq_b, max_seqlen_q) are written as zeros, further rows are not written, nothing of the sequence's cache
 *     or pages is read.
 * Grid: ceil(max_seqlen_q / rows) * batch * nheads blocks from host arguments only, rows from awq_attn_varq_plan (64 or 128; the knob
 *     "attn_prefill_rows" forces either, a forced 256 leaves the plan's choice).  A block reads cu[b] and cu[b + 1] (two scalar loads); one
 *     whose rank is at or beyond ceil(Sq_b / rows) returns before any vector load -- a loose max_seqlen_q costs empty blocks, nothing else.
 *     No workspace, no atomics: bit-deterministic and capturable; a replay follows whatever cu_seqlens_q, the lengths and the table hold then.
 * Bits: tile walk, masks, LDS images and rounding points are the rectangular kernel's.  For every active sequence with Sk_b >= Sq_b its out
 *     rows are bit-identical to awq_attn_prefill_kvcache[_kv8] / awq_attn_prefill_paged[_kv8] on that sequence alone (batch 1, seqlen_q =
 *     Sq_b, its own length and its own table row) under the same q tile.
 * Returns the codes of the rectangular entries, all but AWQ_ERR_LAUNCH without a GPU call, and: cu_seqlens_q NULL AWQ_ERR_NULL; not 4-byte
 *     aligned AWQ_ERR_ALIGN; max_seqlen_q < 1, total_q < 1, batch > 65535 or batch * nheads * ceil(max_seqlen_q / 64) > 2^31 - 1
 *     AWQ_ERR_SHAPE.
 *
 * awq_attn_varq_plan: *q_tile_rows = 64 when max_seqlen_q <= 64, otherwise awq_attn_prefill_plan's choice for seqlen_q = max_seqlen_q capped
 *     at 128; *blocks = the grid above.  A PROVISIONAL rule, not a measurement.  Host only.
 *
 * awq_rope_kv_store_natural_varq[_fp8] / awq_rope_kv_store_paged_varq[_fp8]: awq_rope_kv_store_natural_pos[_fp8] /
 *     awq_rope_kv_store_paged_pos[_fp8] with qkv [total_q, (nheads + 2 nheads_kv) head_dim] under a row stride, q_out [total_q, nheads,
 *     head_dim] contiguous, and (batch, seqlen) replaced by (batch, cu_seqlens_q, max_seqlen_q, total_q).
 * Owner: token t < cu[batch] belongs to the sequence b with cu[b] <= t < cu[b + 1] -- a binary search over cu_seqlens_q per thread, at most
 *     17 cached loads; a tie at zero-length sequences resolves to the owner.  It is token s = t - cu[b] of b: written at position
 *     cache_seqlens[b] + s with the angles of that table row; the paged form looks the page up per token.
 * Sequence b is ACTIVE iff 0 <= cache_seqlens[b], Sq_b <= max_seqlen_q and cache_seqlens[b] + Sq_b <= min(capacity, table_rows).  An inactive
 *     sequence gets zero q_out rows and nothing else.
 * Bits: for every active sequence the q_out rows, the cache / pool rows and the scales are those the _pos entry leaves for that sequence
 *     alone; no other byte of the caches, pools or scale pools is written.
 * Grid: ceil(total_q * head_dim / 8 / 256) blocks, from host arguments only.
 * Returns the codes of the _pos entries with the packed-step codes above (the grid term: total_q * head_dim / 8 beyond 2^38). */
int awq_attn_varq_plan(int batch, int nheads, int nheads_kv, int head_dim, int max_seqlen_q, int* q_tile_rows, int* blocks);
int awq_attn_prefill_kvcache_varq(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q,
                                  int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax,
                                  int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_batch_stride,
                                  long long k_row_stride, long long v_batch_stride, long long v_row_stride, float softmax_scale, int causal,
                                  int dtype, void* stream);
int awq_attn_prefill_kvcache_varq_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                                      void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k,
                                      int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim,
                                      long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                                      long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                                      long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                      void* stream);
int awq_attn_prefill_paged_varq(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                                const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                                int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                                int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                                long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream);
int awq_attn_prefill_paged_varq_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                    const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                    const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                    int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                    long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                    long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                    long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                    void* stream);
int awq_rope_kv_store_natural_varq(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens,
                                   int batch, int cache_batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                   int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype,
                                   void* stream);
int awq_rope_kv_store_natural_varq_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_cache, void* v_cache, float* k_scale,
                                       float* v_scale, const int* cache_seqlens, int batch, int cache_batch, const int* cu_seqlens_q,
                                       int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                       int table_rows, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_paged_varq(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, const int* block_table,
                                 const int* cache_seqlens, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                 int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                 long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                 long long v_row_stride, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_paged_varq_fp8(const void* qkv, const float* freqs_table, void* q_out, void* k_pool, void* v_pool, float* k_scale,
                                     float* v_scale, const int* block_table, const int* cache_seqlens, int batch, const int* cu_seqlens_q,
                                     int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim, int table_rows,
                                     int num_pages, int page_size, int pages_per_seq, long long table_row_stride, long long k_page_stride,
                                     long long k_row_stride, long long v_page_stride, long long v_row_stride, long long k_scale_page_stride,
                                     long long k_scale_row_stride, long long v_scale_page_stride, long long v_scale_row_stride,
                                     long long qkv_row_stride, int dtype, void* stream);

/* ---- A MIXED packed step: who serves a sequence.  awq_attn_varq[_kv8] / awq_attn_paged_varq[_kv8] take the arguments of
 *      awq_attn_prefill_kvcache_varq[_kv8] / awq_attn_prefill_paged_varq[_kv8] and, behind dtype, split_seqlen_q, split_min_keys, workspace and
 *      workspace_bytes.  Three launches in one stream -- the packed one-pass kernel, the packed split-KV kernel, its combine -- whose set
 *      and grids depend on host arguments only; each sequence is served by exactly one of the two kernels, chosen ON THE DEVICE:
 *          the split pair takes sequence b  iff  b is active with 1 <= Sq_b (above), Sq_b <= split_seqlen_q and Sk_b >= split_min_keys;
 *          everything else -- prompt chunks, short histories, Sq_b = 0, inactive sequences (zero rows) -- is the one-pass kernel's, exactly
 *          as in awq_attn_prefill_*_varq.
 *      A one-token sequence over a long history then shares the K / V fetch among the heads of a KV group and spreads over the chip, inside
 *      the same call (and the same captured graph) that serves the prompt chunks.
 * split_seqlen_q >= 0 with split_seqlen_q * (nheads / nheads_kv) <= 128; 0: nothing is split -- the call IS awq_attn_prefill_*_varq, one
 *     launch, workspace unused (NULL is fine).  split_min_keys >= 1.
 * Plan: awq_attn_varq_split_plan returns awq_attn_kvcache_plan's (splits, chunk) for the bound max_seqlen_k (the knob "attn_splitkv_chunk"
 *     applies); split grid batch * nheads_kv * splits, combine grid ceil(batch * nheads * split_seqlen_q * head_dim / 8 / 256).
 * Workspace: awq_attn_varq_split_workspace_bytes = batch * nheads * split_seqlen_q * splits * (head_dim + 2) * 4 bytes, 16-byte aligned;
 *     entry ((b * nheads_kv + kvh) * split_seqlen_q * G + row) * splits + s.  Rows of sequences the pair does not take are never touched.
 * Bits: a taken sequence's rows are those of awq_attn_kvcache[_kv8] / awq_attn_kvcache_paged[_kv8] on that sequence alone (batch 1,
 *     seqlen_q = Sq_b, seqlen_offset = Sq_b under lens_before_step, else 0; same max_seqlen_k and chunk); every other row below
 *     cu[batch] is awq_attn_prefill_*_varq's; rows >= cu[batch] are not written.  No atomics: bit-deterministic and capturable.
 * Returns the codes of awq_attn_prefill_*_varq, and: split_seqlen_q < 0, split_min_keys < 1 or split_seqlen_q * G > 128 AWQ_ERR_SHAPE;
 *     with split_seqlen_q > 0 a NULL or short workspace AWQ_ERR_WORKSPACE, a misaligned one AWQ_ERR_ALIGN.  Every check precedes the first
 *     launch.  The plan refuses head dims other than 64 / 128 and split_seqlen_q * G > 128 with AWQ_ERR_SHAPE; the byte count is then 0. */
int awq_attn_varq_split_plan(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int* splits, int* chunk);
size_t awq_attn_varq_split_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k);
int awq_attn_varq(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                  int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim,
                  long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                  float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes,
                  void* stream);
int awq_attn_varq_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out, int batch,
                      const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k,
                      int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride,
                      long long v_batch_stride, long long v_row_stride, long long k_scale_batch_stride, long long k_scale_row_stride,
                      long long v_scale_batch_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                      int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_paged_varq(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                        const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k,
                        int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                        long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                        float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys, void* workspace,
                        size_t workspace_bytes, void* stream);
int awq_attn_paged_varq_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                            const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k,
                            int lens_before_step, int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                            int nheads, int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                            long long v_page_stride, long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                            long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                            int split_seqlen_q, int split_min_keys, void* workspace, size_t workspace_bytes, void* stream);

/* ---- A SLIDING WINDOW on a mixed packed step: awq_attn_varq_window[_kv8] / awq_attn_paged_varq_window[_kv8] take the arguments of
 *      awq_attn_varq[_kv8] / awq_attn_paged_varq[_kv8] with window_left behind split_min_keys (flash-attn's window_size = (window_left, 0)):
 *          row s of sequence b stands at position p = s + Sk_b - Sq_b and attends keys j with max(0, p - window_left) <= j <= p;
 *          Sk_b as above (64 bits, with lens_before_step).  p < 0: zeros, as without a window; every other row attends at least its own
 *          key.  Activity, padding rows, the cu_seqlens_q clamps and Sq_b = 0 are awq_attn_prefill_*_varq's.
 *      window_left >= max_seqlen_k - 1 hides no key: the rows then carry the bits of awq_attn_varq* on the same step.
 *      Rule: the split pair takes sequence b  iff  b is active with 1 <= Sq_b <= split_seqlen_q and keys_b >= split_min_keys, where
 *          keys_b = min(Sk_b, window_left + Sq_b) is the number of keys the sequence attends at all -- a decode over a long history with a
 *          short window is not "long".  split_seqlen_q = 0: the one-pass launch alone, workspace unused.
 *      Reads: the one-pass kernel walks 64-key tiles from the tile of max(0, q0 + Sk_b - Sq_b - window_left) (q0 = first row of the q tile);
 *          the split pair anchors its splits at anchor_b = max(0, Sk_b - Sq_b - window_left) & ~63: split s owns keys
 *          [anchor_b + s * chunk, min(Sk_b, .. + chunk)).  No key, no scale and no block-table entry below max(0, Sk_b - Sq_b -
 *          window_left) & ~63 is read: pages wholly below it may be freed or reused.
 * Plan: awq_attn_varq_window_plan returns awq_attn_kvcache_plan's (splits, chunk) for the bound min(max_seqlen_k, window_left +
 *     split_seqlen_q + 63), the most keys an anchored walk covers (the knob "attn_splitkv_chunk" applies).  Host arguments only.
 * Workspace: awq_attn_varq_window_workspace_bytes = batch * nheads * split_seqlen_q * splits * (head_dim + 2) * 4 bytes for that plan.
 * No atomics, no host read: bit-deterministic and capturable; the launch set depends on host arguments only.
 * Returns the codes of awq_attn_varq*, and: window_left < 0 AWQ_ERR_SHAPE, causal == 0 AWQ_ERR_SHAPE.  Every check precedes the first
 *     launch.  The plan refuses what awq_attn_varq_split_plan refuses and window_left < 0 with AWQ_ERR_SHAPE; the byte count is then 0. */
int awq_attn_varq_window_plan(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k, int window_left,
                              int* splits, int* chunk);
size_t awq_attn_varq_window_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int split_seqlen_q, int max_seqlen_k,
                                            int window_left);
int awq_attn_varq_window(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                         int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                         long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                         int window_left, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_varq_window_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                             int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                             int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride,
                             long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                             long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                             long long v_scale_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                             int window_left, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_paged_varq_window(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                               const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                               int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                               int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q,
                               int split_min_keys, int window_left, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_paged_varq_window_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                   const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                   const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                   int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                   long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                   long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                   long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                   int split_seqlen_q, int split_min_keys, int window_left, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- SOFT-CAPPED logits on a windowed mixed step (Gemma-2: cap 50, Grok-1: cap 30): awq_attn_varq_softcap[_kv8] /
 *      awq_attn_paged_varq_softcap[_kv8] take the arguments of awq_attn_varq_window[_kv8] / awq_attn_paged_varq_window[_kv8] with softcap
 *      directly behind window_left.  The logits of row s of sequence b become
 *          z_j = softcap * tanh(softmax_scale * (q . k_j) / softcap),   then the causal / window mask, then softmax.
 *      The mask is applied behind the cap, by selection: a masked logit is -inf (not -softcap) and a dead key's score, a NaN included,
 *      contributes nothing.  softmax_scale is free (Gemma-2-27B: 144^-0.5).  Everything else is the contract of the *_window entries:
 *      positions and rows with p < 0, activity and padding rows, the rule on keys_b, the anchor, and "no key, scale or table entry below
 *      the first tile is read".  A layer without a window passes window_left = max_seqlen_k - 1 (larger values are clamped to it).
 *      tanh is evaluated in fp32 from the hardware exp2 and rcp, absolute error <= 10 * 2^-24.
 * softcap == 0: no cap -- the call IS the *_window entry and returns its bits.
 * Plan and workspace: awq_attn_varq_window_plan / awq_attn_varq_window_workspace_bytes, unchanged.
 * Returns the codes of the *_window entries, and: softcap < 0, infinite or NaN AWQ_ERR_SHAPE.  Every check precedes the first launch. */
int awq_attn_varq_softcap(const void* q, const void* k_cache, const void* v_cache, void* out, int batch, const int* cu_seqlens_q, int max_seqlen_q,
                         int total_q, const int* seqlens_k, int lens_before_step, int max_seqlen_k, int lmax, int nheads, int nheads_kv,
                         int head_dim, long long q_row_stride, long long k_batch_stride, long long k_row_stride, long long v_batch_stride,
                         long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                         int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_varq_softcap_kv8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale, void* out,
                             int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                             int max_seqlen_k, int lmax, int nheads, int nheads_kv, int head_dim, long long q_row_stride,
                             long long k_batch_stride, long long k_row_stride, long long v_batch_stride, long long v_row_stride,
                             long long k_scale_batch_stride, long long k_scale_row_stride, long long v_scale_batch_stride,
                             long long v_scale_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q, int split_min_keys,
                             int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_paged_varq_softcap(const void* q, const void* k_pool, const void* v_pool, void* out, const int* block_table, int batch,
                               const int* cu_seqlens_q, int max_seqlen_q, int total_q, const int* seqlens_k, int lens_before_step,
                               int max_seqlen_k, int num_pages, int page_size, int pages_per_seq, long long table_row_stride, int nheads,
                               int nheads_kv, int head_dim, long long q_row_stride, long long k_page_stride, long long k_row_stride,
                               long long v_page_stride, long long v_row_stride, float softmax_scale, int causal, int dtype, int split_seqlen_q,
                               int split_min_keys, int window_left, float softcap, void* workspace, size_t workspace_bytes, void* stream);
int awq_attn_paged_varq_softcap_kv8(const void* q, const void* k_pool, const void* v_pool, const float* k_scale, const float* v_scale, void* out,
                                   const int* block_table, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q,
                                   const int* seqlens_k, int lens_before_step, int max_seqlen_k, int num_pages, int page_size,
                                   int pages_per_seq, long long table_row_stride, int nheads, int nheads_kv, int head_dim,
                                   long long q_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                   long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                   long long v_scale_page_stride, long long v_scale_row_stride, float softmax_scale, int causal, int dtype,
                                   int split_seqlen_q, int split_min_keys, int window_left, float softcap, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- Encoder-tower attention over packed sequences (flash_attn_varlen_qkvpacked_func's forward: tinychat/models/internvl/internvit.py:45-90).
 *     q / k / v [total_rows, H, Dh] with row strides of their own (elements; heads contiguous), out [total_rows, H, Dh] contiguous; a
 *     packed qkv [total_rows, 3, H, Dh] is three pointers into one buffer with row stride 3 H Dh.
 *     cu_seqlens: int32 [nseq + 1] ON THE DEVICE; sequence s owns rows cu_seqlens[s] .. cu_seqlens[s + 1] - 1 and a row attends exactly
 *     the keys of its own sequence: O = softmax(softmax_scale * Q K^T) V.  The host never reads cu_seqlens and never synchronises: the
 *     grid comes from nseq and max_seqlen alone (rows of a sequence beyond max_seqlen are not computed), zero-length sequences are
 *     allowed, and every row index is clamped into [0, total_rows - 1], so a wrong cu_seqlens cannot make the kernel leave the tensors.
 *     Rows >= cu_seqlens[nseq] are neither read nor written.
 * T = fp16 / bf16, Dh = 64 or 72 (no byte outside a (row, head)'s 2 Dh bytes is read), causal must be 0.  Same arithmetic as
 * awq_attn_prefill; no workspace, no atomics: bit-deterministic and capturable (csrc/awq_attn_tower_cdna4.hip).
 * Returns AWQ_ERR_SHAPE (head dim, causal != 0, non-positive sizes, a row stride below H * Dh), AWQ_ERR_DTYPE, AWQ_ERR_NULL (cu_seqlens
 * included: the dense form is awq_attn_prefill), AWQ_ERR_ALIGN (16 bytes for the pointers and the strides, 4 for cu_seqlens),
 * AWQ_ERR_LAUNCH; all but the last without a GPU call. */
/* Host-side plan: *blocks blocks, each a q tile of *q_tile_rows rows (32, 64 or 128) of one (sequence, head); no GPU call. */
int awq_attn_varlen_plan(int nseq, int nheads, int head_dim, int max_seqlen, int* q_tile_rows, int* blocks);
int awq_attn_varlen(const void* q, const void* k, const void* v, void* out, const int* cu_seqlens, int nseq, int max_seqlen,
                    long long total_rows, int nheads, int head_dim, long long q_row_stride, long long k_row_stride,
                    long long v_row_stride, float softmax_scale, int causal, int dtype, void* stream);

/* ---- Rotary embeddings of a prompt.
 * awq_rope_with_pos (fused_rope_with_pos_forward_func, rope_new/fused_rope_with_pos.cu:33-72,263-333): input [n0, n1, nheads, head_dim]
 * with element strides (in_stride0, in_stride1, in_stride_head, 1), out the same shape with its own strides; the angle of element
 * (i0, i1, ., c), c < rot_dim, is freqs[(i1 * n0 + i0) * rot_dim + c] (fp32; the reference's index, quirk included); partner
 * c + rot_dim/2 negated (first half) or c - rot_dim/2; out = T(x cos + x_rot sin) in fp32, one rounding; columns >= rot_dim are copied.
 * rot_dim % 16 == 0, head_dim % 8 == 0, strides % 8 == 0, pointers 16-byte aligned.
 * awq_rope_neox_inplace (rotary_embedding_neox, position_embedding/pos_encoding_kernels.cu:12-87): query and key
 * [num_tokens, nheads, head_size] contiguous, rotated in place over the first rot_dim dims (rotate-half) at positions[token] (int64) with
 * cos_sin_cache T [max_position, rot_dim] = cos | sin.  Evaluated in fp32 and rounded to T once (the reference rounds every product
 * and sum); a position outside [0, max_position) is clamped into it. */
int awq_rope_with_pos(const void* input, const float* freqs, void* out, int n0, int n1, int nheads, int head_dim, int rot_dim,
                      long long in_stride0, long long in_stride1, long long in_stride_head, long long out_stride0, long long out_stride1,
                      long long out_stride_head, int dtype, void* stream);
int awq_rope_neox_inplace(const long long* positions, void* query, void* key, const void* cos_sin_cache, int num_tokens, int nheads,
                          int head_size, int rot_dim, int max_position, int dtype, void* stream);

/* ---- W8A8 linear (the reference's awq/kernels/csrc/w8a8/ family, called by the vision towers: tinychat/modules/fused_siglipdecoder.py,
 * fused_internencoder.py, awq/quantize/w8a8_linear.py).  int8 activations and weights, fp16 scales and output.
 *
 * awq_w8a8_gemm replaces w8a8_gemm_forward_cuda (w8a8_gemm_cuda.cu:907-953, kernel :635-905) when bias == NULL and
 * w8a8_gemm_fuse_bias_forward_cuda (:586-633, kernel :299-584) otherwise:
 *     x int8 [m, k], w int8 [n, k] (both row-major, k contiguous), wscales fp16 [n], ascales fp16 [m], bias fp16 [n] or NULL, out fp16 [m, n]
 *     acc = x . w^T in int32 on the int8 matrix cores (exact; no fp32 accumulation, no split-K, no workspace, no atomics: bit-deterministic
 *     and capturable), then in fp32
 *         bias:     out = half_rn(fmaf(float(acc) * float(wscales[n]), float(ascales[m]), float(bias[n])))     (:575-578)
 *         no bias:  out = half_rn(float(acc) * (float(wscales[n]) * float(ascales[m])))                        (:896-898)
 * k % 16 == 0 (k <= 2^20), n % 8 == 0, any m >= 1; all pointers 16-byte aligned.  Every such shape is served by both forms: the reference's
 * no-bias launch drops a partial column tile (:73) and its fuse-bias kernel reads bias past n; neither is reproduced.  Rows >= m and columns
 * >= n are neither read nor written.  Returns AWQ_ERR_NULL, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN before any GPU call, or AWQ_ERR_LAUNCH. */
int awq_w8a8_gemm(const void* x, const void* w, const void* wscales, const void* ascales, const void* bias, void* out, int m, int n, int k,
                  void* stream);
/* Host-side plan (no GPU call): the launch is ceil(m / *tile_m) * ceil(n / *tile_n) blocks, the return value; 0 if the shape is not served.
 * Two tiles, one rule: 128 x 128 when that yields at least one block per CU (256), else 64 x 64 -- the counterpart of the reference's
 * two tile shapes split at m = 128 (w8a8_gemm_cuda.cu:610-631).  tile_m / tile_n may be NULL. */
int awq_w8a8_gemm_plan(int m, int n, int k, int* tile_m, int* tile_n);
/* Replaces invoke_quant (w8a8/quantization.cu:56-112): per-token int8 quantisation of x T [m, k]:
 *     amax = max_k |float(x)|, scale[m] = half_rn(amax / 127), out_i8 = sat_s8(rne(float(x) * (127 / amax)))
 * in IEEE fp32 with correctly rounded divisions (independent of the reduction order).  An all-zero row gives scale 0 and zeros (the
 * reference reaches the same through NaN -> 0).  T = fp16 / bf16, scale fp16 [m]; k % 8 == 0. */
int awq_quant_per_token(const void* x, void* out_i8, void* scale, int m, int k, int dtype, void* stream);
/* Replaces gelu_and_quant (w8a8/act.cu:22-96), fp16 only: g = gelu_fast(x) with every step an fp16 operation rounded on its own (:23-28),
 * tmp[m, k] = g (fp16; the callers read it), amax = max_k (g > 0.0001h ? g : -g) starting from 0 (positive values up to 1e-4 do not count:
 * the reference's quirk, :45,52-54, kept), scale[m] = half_rn(amax / 127), out_i8 = sat_s8(rne(float(half_rn(127 / amax) * g))) with that
 * product in fp16 (:65-68).  k % 8 == 0. */
int awq_gelu_quant_per_token(const void* x, void* out_i8, void* scale, void* tmp, int m, int k, void* stream);
/* Replaces rms_norm_general (w8a8/layernorm.cu:55-188, launch :193-232) -- a LayerNorm despite the name:
 *     v = (x - mean) * rsqrt(var + eps) * gamma (+ beta) in fp32 (centred variance; the reference's E[x^2] - mean^2 agrees in exact arithmetic)
 *     per_token != 0 (:142-187): amax = max(max_k |T(v)|, T(1e-6)) over v rounded to T, out_i8 = sat_s8(rne(v * (127 / amax))) on the unrounded
 *                                v, scale[m] = half_rn(amax / 127) is WRITTEN
 *     per_token == 0 (:156-160, :224-229): out_i8 = sat_s8(rne(v * float(scale[0]))), scale[0] is READ; beta is ignored and the scale
 *                                multiplies -- the reference's behaviour, kept
 * T = fp16 / bf16 (x, gamma, beta), scale fp16; beta may be NULL; k % 8 == 0, k <= 16384 (the row stays on chip). */
int awq_layernorm_quant(const void* x, const void* gamma, const void* beta, float eps, void* out_i8, void* scale, int m, int k, int per_token,
                        int dtype, void* stream);

/* ---- Per-head q/k RMSNorm in front of the rotation (Qwen3, Gemma-3): the ten natural-layout stores, each with a _qknorm sibling that takes
 *      its argument list and, directly after the angles, q_gamma, k_gamma (device fp32 [head_dim], 16-byte aligned) and norm_eps.  Every q head
 *      and every k head of a token is normalised over its head_dim columns BEFORE the rotation; v is untouched.  One launch, the sibling's
 *      grid; no workspace, no atomics: bit-deterministic and capturable.
 * Arithmetic, per (token, head), x the head's head_dim values: ss = the fp32 sum of x[c]^2 (8 consecutive columns folded in ascending order
 *     with fmaf from 0, the head_dim / 8 partial sums combined pairwise at distances 1, 2, .., head_dim / 16); rstd = rsqrtf(ss / head_dim +
 *     norm_eps); y[c] = T((x[c] * rstd) * gamma[c]), ONE rounding -- awq_rmsnorm's arithmetic on the head as a row of k = head_dim.  The
 *     rotation, the FP8 quantiser and the stores then act on y exactly as the sibling's act on x.
 * Bits: with gammas that T holds, q_out, the caches or pools and the scales are those the sibling leaves on a copy of qkv whose q and k heads
 *     were replaced by awq_rmsnorm(head rows, gamma in T, norm_eps).  The gammas are fp32 because Gemma-3's 1 + w is formed in fp32 and no
 *     T holds it.  An inactive sequence gets zero q_out rows and nothing else; padding rows of a packed step are not touched.
 * Returns the sibling's codes, and: q_gamma or k_gamma NULL AWQ_ERR_NULL; one of them not 16-byte aligned AWQ_ERR_ALIGN; norm_eps negative,
 *     infinite or NaN AWQ_ERR_SHAPE.  Every check precedes the launch. */
int awq_rope_kv_store_natural_qknorm(const void* qkv, const float* freqs, const float* q_gamma, const float* k_gamma, float norm_eps, void* q_out,
                                     void* k_cache, void* v_cache, int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim,
                                     int rot_dim, int lmax, int start_pos, long long qkv_batch_stride, long long qkv_row_stride, int dtype,
                                     void* stream);
int awq_rope_kv_store_natural_fp8_qknorm(const void* qkv, const float* freqs, const float* q_gamma, const float* k_gamma, float norm_eps, void* q_out,
                                         void* k_cache, void* v_cache, float* k_scale, float* v_scale, int batch, int cache_batch, int seqlen,
                                         int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int start_pos, long long qkv_batch_stride,
                                         long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_natural_pos_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                         void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens, int batch, int cache_batch, int seqlen,
                                         int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_batch_stride,
                                         long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_natural_pos_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                             void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const int* cache_seqlens,
                                             int batch, int cache_batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int lmax,
                                             int table_rows, long long qkv_batch_stride, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_paged_pos_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                       void* q_out, void* k_pool, void* v_pool, const int* block_table, const int* cache_seqlens, int batch,
                                       int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size,
                                       int pages_per_seq, long long table_row_stride, long long k_page_stride, long long k_row_stride,
                                       long long v_page_stride, long long v_row_stride, long long qkv_batch_stride, long long qkv_row_stride,
                                       int dtype, void* stream);
int awq_rope_kv_store_paged_pos_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                           void* q_out, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* block_table,
                                           const int* cache_seqlens, int batch, int seqlen, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                           int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                           long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                           long long k_scale_page_stride, long long k_scale_row_stride, long long v_scale_page_stride,
                                           long long v_scale_row_stride, long long qkv_batch_stride, long long qkv_row_stride, int dtype,
                                           void* stream);
int awq_rope_kv_store_natural_varq_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                          void* q_out, void* k_cache, void* v_cache, const int* cache_seqlens, int batch, int cache_batch,
                                          const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim,
                                          int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_natural_varq_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                              void* q_out, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const int* cache_seqlens,
                                              int batch, int cache_batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                              int nheads_kv, int head_dim, int rot_dim, int lmax, int table_rows, long long qkv_row_stride, int dtype,
                                              void* stream);
int awq_rope_kv_store_paged_varq_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                        void* q_out, void* k_pool, void* v_pool, const int* block_table, const int* cache_seqlens, int batch,
                                        const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads, int nheads_kv, int head_dim, int rot_dim,
                                        int table_rows, int num_pages, int page_size, int pages_per_seq, long long table_row_stride,
                                        long long k_page_stride, long long k_row_stride, long long v_page_stride, long long v_row_stride,
                                        long long qkv_row_stride, int dtype, void* stream);
int awq_rope_kv_store_paged_varq_fp8_qknorm(const void* qkv, const float* freqs_table, const float* q_gamma, const float* k_gamma, float norm_eps,
                                            void* q_out, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const int* block_table,
                                            const int* cache_seqlens, int batch, const int* cu_seqlens_q, int max_seqlen_q, int total_q, int nheads,
                                            int nheads_kv, int head_dim, int rot_dim, int table_rows, int num_pages, int page_size, int pages_per_seq,
                                            long long table_row_stride, long long k_page_stride, long long k_row_stride, long long v_page_stride,
                                            long long v_row_stride, long long k_scale_page_stride, long long k_scale_row_stride,
                                            long long v_scale_page_stride, long long v_scale_row_stride, long long qkv_row_stride, int dtype,
                                            void* stream);

/* Tuning hook for tests, experiments and benchmarks (not part of the reference surface): integer knobs that force one of the
 * shipped code paths ("gemm_variant", "gemm_splitk", "gemv_dma", "gemvd_waves", "attn_prefill_rows", "attn_splitkv_chunk", "tower_rows", "w8a8_tile", ...) so that tests can cover each of them; 0
 * restores the default heuristic.  A default process cannot reach it: unless AWQ_TUNING=1 is set in the environment every
 * call returns AWQ_ERR_SHAPE and changes nothing.  Timing probes and experiment-only kernel instantiations exist only in
 * builds made with AWQ_PROBES=1.  Returns AWQ_OK, or AWQ_ERR_SHAPE for an unknown key.  Process-global, not thread-safe. */
int awq_tune_set(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* AWQ_CDNA4_H_ */
