// W8A8 linear for gfx950: the int8 GEMM with its dequantising epilogue, and the three per-token quantisers that feed it.
// Replaces the reference's awq/kernels/csrc/w8a8/ family (w8a8_gemm_cuda.cu, quantization.cu, act.cu, layernorm.cu) as the vision
// towers call it (tinychat/modules/fused_siglipdecoder.py, fused_internencoder.py, awq/quantize/w8a8_linear.py).
//
// GEMM: out[M, N] (fp16) = epilogue(x_i8[M, K] . w_i8[N, K]^T), both operands row-major with K contiguous.
//  * v_mfma_i32_32x32x32_i8, int32 accumulation: the sum is exact, whatever the order.  No fp32 accumulation, no split-K, no workspace,
//    no atomics -- bit-deterministic and capturable.
//  * w is the MFMA's A operand (result rows = n), x its B operand (result columns = m): a lane then owns four consecutive n of one row m
//    per accumulator quad and stores them as 8 bytes.  A and B fragments are both 16 K-contiguous bytes per lane, lanes 0-31 the
//    first and lanes 32-63 the second 16 of a 32-k step.
//  * Two tiles: 128 x 128 and 64 x 64 (four waves as 2 x 2, a wave owns a quarter).  ONE rule: the 128 x 128 tile when it yields at
//    least one block per CU (256), else the 64 x 64 tile (w8a8_gemm_plan; the reference's two tiles split at M = 128, :610-631).
//  * k-step = 64.  A stage holds [TM rows of x | TN rows of w] x 64 bytes; the stages form a ring of 4 (64 x 64) or 3 (128 x 128): the DMAs
//    of step t + S - 1 are issued while step t is multiplied (more than a double buffer, because a 64-byte step is shorter than the
//    latency of its loads), one s_barrier per step, counted vmcnt waits.  Operands arrive by LDS-DMA
//    (awq_dma.hpp) in 1-KiB pieces of 16 rows; the DMA image is lane-linear, so the XOR swizzle sits in the per-lane SOURCE address:
//    the 16-byte chunk c of row r lives at slot c ^ ((r >> 2) & 3) of the row.  A ds_read_b128 group of 16 lanes (MI355X: lanes
//    {0-3, 12-15, 20-27}, ...) then touches rows with four distinct (r >> 2) & 3 and four distinct r & 3: 16 distinct 16-byte slots of
//    the 256-byte bank row, conflict-free.
//  * K tail (K % 64 in {16, 32, 48}): chunks at k >= K are not fetched (their DMA is issued out of bounds) and the x fragment of such a
//    chunk is zeroed in registers, so whatever the LDS slot held contributes nothing.
//  * Rows >= M of x and >= N of w are not read (the block's descriptors end at its last valid row; lanes of rows past it re-read that
//    row) and rows >= M / columns >= N of out are not written.
//  * Epilogue in fp32, in the reference's two associations (w8a8_gemm_cuda.cu:575-578 with bias, :896-898 without), fp contraction off:
//        bias:     t = float(acc) * float(wscale[n]);  out = half_rn(fmaf(t, float(ascale[m]), float(bias[n])))
//        no bias:  out = half_rn(float(acc) * (float(wscale[n]) * float(ascale[m])))
//    float(acc) is v_cvt_f32_i32 (nearest-even; |acc| passes 2^24 at K = 4304).
//  * Unlike the reference, every N % 8 == 0 is served by BOTH entries: its no-bias launch floors N / CTA_N and drops a partial column
//    tile (w8a8_gemm_cuda.cu:73), and its fuse-bias kernel loads bias for a whole column tile, past N.  Neither is reproduced.
//
// Quantisers (one block per row; IEEE fp32 with correctly rounded division, so results do not depend on the reduction order):
//  * quant_rows        invoke_quant            quantization.cu:56-92
//  * gelu_quant_rows   gelu_and_quant          act.cu:22-77      (fp16 op-by-op GELU, tmp write, the 1e-4 quirk of its amax)
//  * layernorm_quant   rms_norm_general        layernorm.cu:55-188,193-232 (a LayerNorm despite its name; per-token or per-tensor)
#include <string.h>

#include "awq_dma.hpp"
#include "awq_kernels.hpp"

#pragma clang fp contract(off)

namespace awq {
namespace {

int g_force_tile = 0;  // knob w8a8_tile (awq_tune_set): 64 / 128 forces the tile, 0 = the plan's rule

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kBK = 64;                   // bytes (= int8 k) per row per stage
constexpr u32 kOobW8 = 0x80000000u;       // a DMA offset past every descriptor: nothing is fetched
constexpr int kW8MaxK = 1 << 20;          // 128 rows x K stays below 2^31 descriptor bytes
constexpr int kNumCU = 256;

// ---------------------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------------------
template <int TM, int TN, int S, bool BIAS>
__global__ __launch_bounds__(256) void w8a8_gemm_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ w,
                                                       const _Float16* __restrict__ wscales, const _Float16* __restrict__ ascales,
                                                       const _Float16* __restrict__ bias, _Float16* __restrict__ out, int M, int N, int K) {
  constexpr int WTM = TM / 2, WTN = TN / 2;  // a wave's share of the tile
  constexpr int MB = WTM / 32, NB = WTN / 32;  // 32 x 32 MFMA blocks per wave along m / n
  constexpr int PX = TM / 16, PW = TN / 16;    // 1-KiB DMA pieces (16 rows x 64 B) of the x / w part of a stage
  constexpr int PPW = (PX + PW) / 4;           // pieces per wave per stage
  constexpr int STAGE = (TM + TN) * kBK;
  static_assert(PX % 4 == 0 && PW % 4 == 0, "piece wv + 4 q is an x piece for 4 q < PX whatever the wave");
  static_assert(S >= 2 && S * STAGE <= 65536, "the ring lives in static LDS");
  __shared__ __attribute__((aligned(1024))) char smem[S * STAGE];

  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wv & 1, wn = wv >> 1;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const int mrows = min(TM, M - m0), nrows = min(TN, N - n0);  // valid rows of the block's x / w panels (>= 1)

  // descriptors of the block's panels: they end at the last valid row
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(x) + (size_t)m0 * K, 0, mrows * K, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(w) + (size_t)n0 * K, 0, nrows * K, 0x00020000);

  // this wave's pieces: q-th piece = piece wv + 4 q of [x pieces | w pieces]; lane -> row 16 piece + lane / 4, slot lane % 4, which
  // receives source chunk slot ^ ((row >> 2) & 3) = slot ^ ((lane >> 4) & 3)
  const int pchunk = (lane & 3) ^ ((lane >> 4) & 3);
  u32 pvoff[PPW];
#pragma unroll
  for (int q = 0; q < PPW; ++q) {
    const bool is_x = 4 * q < PX;
    const int piece = wv + 4 * q - (is_x ? 0 : PX);
    const int r = min(16 * piece + (lane >> 2), (is_x ? mrows : nrows) - 1);
    pvoff[q] = (u32)r * (u32)K + (u32)(16 * pchunk);
  }
  // k-step kb -> stage; chunks at k >= K (the K tail, and whole steps past the last one: same operation count, no traffic) are issued
  // out of bounds
  auto issue = [&](int stage, int kb) {
    const int k0 = kb * kBK;
    const u32 dead = (k0 + 16 * pchunk < K) ? 0u : kOobW8;
#pragma unroll
    for (int q = 0; q < PPW; ++q) {
      const bool is_x = 4 * q < PX;
      char* dst = smem + stage * STAGE + (is_x ? 0 : TM * kBK) + (wv + 4 * q - (is_x ? 0 : PX)) * 1024;
      dma_to_lds<16, 0>(is_x ? rx : rw, dst, pvoff[q] | dead, (u32)k0);
    }
  };

  // fragment addresses in stage 0, 32-k half step 0: row (lane & 31) of the wave's block, chunk lane >> 5 (half step 1: chunk + 2)
  u32 xrd[MB], wrd[NB];
  const int half = lane >> 5;
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int r = wm * WTM + b * 32 + (lane & 31);
    xrd[b] = (u32)(r * kBK) | ((u32)(half ^ ((r >> 2) & 3)) << 4);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int r = wn * WTN + b * 32 + (lane & 31);
    wrd[b] = (u32)(TM * kBK + r * kBK) | ((u32)(half ^ ((r >> 2) & 3)) << 4);
  }

  i32x16 acc[NB][MB];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0;

  const int nk = (K + kBK - 1) / kBK;
  const int tail_chunks = (K % kBK) / 16;  // valid 16-byte chunks of the last k-step when K % 64 != 0
  asm volatile("" ::: "memory");
#pragma unroll
  for (int j = 0; j < S - 1; ++j) issue(j, j);
  int rd = 0, wr = S - 1;  // ring slots of the step being multiplied / being fetched
  for (int it = 0; it < nk; ++it) {
    // this wave's pieces of step `it` have landed (the S - 2 younger groups may still be in flight) and its reads of step it - 1 are done ...
    dma_wait_vm<(S - 2) * PPW>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // ... and so for every wave: slot `wr` (read in step it - 1) is free, slot `rd` is complete
    asm volatile("" ::: "memory");
    issue(wr, it + S - 1);
    asm volatile("" ::: "memory");
    const char* st = smem + rd * STAGE;
    rd = rd + 1 == S ? 0 : rd + 1;
    wr = wr + 1 == S ? 0 : wr + 1;
    const bool tail = tail_chunks != 0 && it == nk - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      i32x4 xf[MB], wf[NB];
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        xf[b] = *reinterpret_cast<const i32x4*>(st + (xrd[b] ^ (u32)(ks << 5)));
        if (tail && 2 * ks + half >= tail_chunks) xf[b] = i32x4{0, 0, 0, 0};  // k >= K: zero, whatever the slot holds
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) wf[b] = *reinterpret_cast<const i32x4*>(st + (wrd[b] ^ (u32)(ks << 5)));
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[a], xf[b], acc[a][b], 0, 0, 0);
    }
  }

  // ---- epilogue: accumulator register r of block (a, b) = out[m = .. + lane % 32][n = .. + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)] ----
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int m = m0 + wm * WTM + b * 32 + (lane & 31);
    if (m >= M) continue;
    const float as = (float)ascales[m];
#pragma unroll
    for (int a = 0; a < NB; ++a) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * WTN + a * 32 + 8 * g + 4 * half;
        if (n >= N) continue;  // n % 4 == 0 and N % 8 == 0: the quad is inside or outside as a whole
        const f16x4 ws = *reinterpret_cast<const f16x4*>(wscales + n);
        f16x4 o;
        if constexpr (BIAS) {
          const f16x4 bs = *reinterpret_cast<const f16x4*>(bias + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = (float)acc[a][b][4 * g + r] * (float)ws[r];
            o[r] = (_Float16)__builtin_fmaf(t, as, (float)bs[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s = (float)ws[r] * as;
            o[r] = (_Float16)((float)acc[a][b][4 * g + r] * s);
          }
        }
        *reinterpret_cast<f16x4*>(out + (size_t)m * N + n) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// per-token quantisers: 256 threads per row
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kQT = 256;

__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();  // (red may still be read from an earlier reduction)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// sat_s8(rne(v)); NaN -> 0 like the reference's cvt.rni.sat.s8.f32 (utils.cuh float_to_int8_rn)
__device__ __forceinline__ u32 to_s8(float v) {
  const float r = fminf(fmaxf(__builtin_rintf(v), -128.0f), 127.0f);
  return (u32)(v == v ? (int)r : 0) & 0xFFu;
}

template <typename DT>
__device__ __forceinline__ void unpack8(const u32x4& v, float (&f)[8]) {
  const u32 wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = DT::to_float((uint16_t)(wd[j] & 0xFFFFu));
    f[2 * j + 1] = DT::to_float((uint16_t)(wd[j] >> 16));
  }
}
__device__ __forceinline__ u32x2 pack_s8(const float (&f)[8]) {
  return u32x2{to_s8(f[0]) | (to_s8(f[1]) << 8) | (to_s8(f[2]) << 16) | (to_s8(f[3]) << 24),
               to_s8(f[4]) | (to_s8(f[5]) << 8) | (to_s8(f[6]) << 16) | (to_s8(f[7]) << 24)};
}

// invoke_quant (quantization.cu:56-92): amax = max |float(x)|, scale = half_rn(amax / 127), q = sat_s8(rne(float(x) * (127 / amax))).
// An all-zero row: 127 / 0 = inf, 0 * inf = NaN -> q = 0, scale = 0 -- the reference's own path.
template <typename DT>
__global__ __launch_bounds__(kQT) void quant_rows_kernel(const uint16_t* __restrict__ x, int8_t* __restrict__ q, _Float16* __restrict__ scale, int K) {
  __shared__ float red[4];
  const size_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * K);
  u32x2* qr = reinterpret_cast<u32x2*>(q + row * K);
  const int nv = K >> 3;
  float amax = 0.0f;
  for (int i = threadIdx.x; i < nv; i += kQT) {
    float f[8];
    unpack8<DT>(xr[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  }
  amax = block_max(amax, red);
  if (threadIdx.x == 0) scale[row] = (_Float16)__fdiv_rn(amax, 127.0f);
  const float inv = __fdiv_rn(127.0f, amax);
  for (int i = threadIdx.x; i < nv; i += kQT) {
    float f[8];
    unpack8<DT>(xr[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] * inv;
    qr[i] = pack_s8(f);
  }
}

// gelu_and_quant (act.cu:22-77), fp16: gelu_fast with every step an fp16 operation rounded on its own (:23-28), tmp = g, then
// amax over (g > 0.0001h ? g : -g) starting from 0 -- positive values up to 1e-4 do not count, the reference's quirk (:45,52-54) --
// scale = half_rn(amax / 127), q = sat_s8(rne(float(half_rn(127 / amax) * g))) with that product in fp16 (:65-68).
__device__ __forceinline__ _Float16 gelu_fast_h(_Float16 x) {
  const _Float16 a = x * (_Float16)0.79788456f;
  const _Float16 c = (_Float16)0.044715f * x;
  const _Float16 p = c * x;
  const _Float16 e = (_Float16)1.0f + p;
  const _Float16 u = a * e;
  const _Float16 t = (_Float16)tanhf((float)u);
  const _Float16 hx = (_Float16)0.5f * x;
  const _Float16 ot = (_Float16)1.0f + t;
  return hx * ot;
}
__global__ __launch_bounds__(kQT) void gelu_quant_rows_kernel(const uint16_t* __restrict__ x, int8_t* __restrict__ q, _Float16* __restrict__ scale,
                                                              uint16_t* __restrict__ tmp, int K) {
  __shared__ float red[4];
  const size_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * K);
  u32x4* tr = reinterpret_cast<u32x4*>(tmp + row * K);
  u32x2* qr = reinterpret_cast<u32x2*>(q + row * K);
  const int nv = K >> 3;
  const _Float16 tiny = (_Float16)0.0001f;
  float amax = 0.0f;
  for (int i = threadIdx.x; i < nv; i += kQT) {
    const f16x8 xv = __builtin_bit_cast(f16x8, xr[i]);
    f16x8 gv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const _Float16 g = gelu_fast_h(xv[j]);
      gv[j] = g;
      const _Float16 t = g > tiny ? g : -g;
      if ((float)t > amax) amax = (float)t;
    }
    tr[i] = __builtin_bit_cast(u32x4, gv);
  }
  amax = block_max(amax, red);
  if (threadIdx.x == 0) scale[row] = (_Float16)__fdiv_rn(amax, 127.0f);
  const _Float16 inv = (_Float16)__fdiv_rn(127.0f, amax);
  for (int i = threadIdx.x; i < nv; i += kQT) {  // a thread re-reads the vectors it wrote itself
    const f16x8 gv = __builtin_bit_cast(f16x8, tr[i]);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const _Float16 pr = inv * gv[j];
      f[j] = (float)pr;
    }
    qr[i] = pack_s8(f);
  }
}

// rms_norm_general (layernorm.cu:55-188): v = (x - mean) * rsqrt(var + eps) * gamma + beta in fp32; the row stays in registers
// (k <= 16384) and the variance is the centred sum (the reference's E[x^2] - mean^2, :111, agrees in exact arithmetic).
//   per token  (:142-187): amax = max(max |T(v)|, T(1e-6)) over v ROUNDED to T, q = sat_s8(rne(v * (127 / amax))) on the unrounded v,
//                          scale = half_rn(amax / 127)
//   per tensor (:156-160, :224-229): q = sat_s8(rne(v * float(scaling[0]))) -- beta is not applied (the launch passes nullptr) and the
//                          scale multiplies; both are the reference's behaviour and are kept.
constexpr int kLnVec = 8;  // vectors of 8 per thread: 256 x 8 x 8 = 16384 columns
template <typename DT>
__global__ __launch_bounds__(kQT) void layernorm_quant_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ gamma,
                                                              const uint16_t* __restrict__ beta, float eps, int8_t* __restrict__ q,
                                                              _Float16* __restrict__ scale, int K, int per_token) {
  __shared__ float red[4];
  const size_t row = blockIdx.x;
  const u32x4* xr = reinterpret_cast<const u32x4*>(x + row * K);
  const u32x4* gr = reinterpret_cast<const u32x4*>(gamma);
  const u32x4* br = reinterpret_cast<const u32x4*>(beta);
  u32x2* qr = reinterpret_cast<u32x2*>(q + row * K);
  const int nv = K >> 3;
  const bool use_beta = per_token && beta != nullptr;
  u32x4 xv[kLnVec];
  float sum = 0.0f;
#pragma unroll
  for (int t = 0; t < kLnVec; ++t) {
    const int i = threadIdx.x + t * kQT;
    xv[t] = u32x4{0, 0, 0, 0};
    if (i < nv) {
      xv[t] = xr[i];
      float f[8];
      unpack8<DT>(xv[t], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += f[j];
    }
  }
  const float mean = __fdiv_rn(block_sum(sum, red), (float)K);
  float sq = 0.0f;
#pragma unroll
  for (int t = 0; t < kLnVec; ++t) {
    if (threadIdx.x + t * kQT < nv) {
      float f[8];
      unpack8<DT>(xv[t], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = f[j] - mean;
        sq += d * d;
      }
    }
  }
  const float rstd = rsqrtf(__fdiv_rn(block_sum(sq, red), (float)K) + eps);
  auto norm8 = [&](int t, int i, float (&v)[8]) {
    float f[8], g[8];
    unpack8<DT>(xv[t], f);
    unpack8<DT>(gr[i], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ((f[j] - mean) * rstd) * g[j];
    if (use_beta) {
      float b[8];
      unpack8<DT>(br[i], b);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + b[j];
    }
  };
  float mul;
  if (per_token) {
    float amax = DT::to_float(DT::from_float(1e-6f));
#pragma unroll
    for (int t = 0; t < kLnVec; ++t) {
      const int i = threadIdx.x + t * kQT;
      if (i < nv) {
        float v[8];
        norm8(t, i, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(DT::to_float(DT::from_float(v[j]))));
      }
    }
    amax = block_max(amax, red);
    if (threadIdx.x == 0) scale[row] = (_Float16)__fdiv_rn(amax, 127.0f);
    mul = __fdiv_rn(127.0f, amax);
  } else {
    mul = (float)scale[0];
  }
#pragma unroll
  for (int t = 0; t < kLnVec; ++t) {
    const int i = threadIdx.x + t * kQT;
    if (i < nv) {
      float v[8];
      norm8(t, i, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] * mul;
      qr[i] = pack_s8(v);
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
int w8a8_tune_set(const char* key, int value) {
  if (strcmp(key, "w8a8_tile") != 0 || (value != 0 && value != 64 && value != 128)) return -1;
  g_force_tile = value;
  return 0;
}

// The rule: the 128 x 128 tile when it yields at least one block per CU (256), else the 64 x 64 tile.
int w8a8_gemm_plan(int m, int n, int k, int* tile_m, int* tile_n) {
  if (m < 1 || n < 8 || (n % 8) != 0 || k < 16 || (k % 16) != 0 || k > kW8MaxK) return 0;
  auto blocks = [&](int t) { return (long long)((m + t - 1) / t) * ((n + t - 1) / t); };
  const int t = g_force_tile ? g_force_tile : (blocks(128) >= kNumCU ? 128 : 64);
  if ((n + t - 1) / t > 65535 || blocks(t) > 0x7FFFFFFFll) return 0;
  if (tile_m) *tile_m = t;
  if (tile_n) *tile_n = t;
  return (int)blocks(t);
}

int launch_w8a8_gemm(const void* x, const void* w, const void* wscales, const void* ascales, const void* bias, void* out, int m, int n, int k,
                     hipStream_t st) {
  int tm = 0, tn = 0;
  if (w8a8_gemm_plan(m, n, k, &tm, &tn) == 0) return -1;
  const dim3 grid((m + tm - 1) / tm, (n + tn - 1) / tn);
  const auto* xi = static_cast<const int8_t*>(x);
  const auto* wi = static_cast<const int8_t*>(w);
  const auto* wsc = static_cast<const _Float16*>(wscales);
  const auto* asc = static_cast<const _Float16*>(ascales);
  const auto* bs = static_cast<const _Float16*>(bias);
  auto* o = static_cast<_Float16*>(out);
  if (tm == 128) {
    if (bias) w8a8_gemm_kernel<128, 128, 3, true><<<grid, 256, 0, st>>>(xi, wi, wsc, asc, bs, o, m, n, k);
    else w8a8_gemm_kernel<128, 128, 3, false><<<grid, 256, 0, st>>>(xi, wi, wsc, asc, bs, o, m, n, k);
  } else {
    if (bias) w8a8_gemm_kernel<64, 64, 4, true><<<grid, 256, 0, st>>>(xi, wi, wsc, asc, bs, o, m, n, k);
    else w8a8_gemm_kernel<64, 64, 4, false><<<grid, 256, 0, st>>>(xi, wi, wsc, asc, bs, o, m, n, k);
  }
  return 0;
}

int launch_quant_per_token(const void* x, void* out_i8, void* scale, int m, int k, int dtype, hipStream_t st) {
  const auto* xi = static_cast<const uint16_t*>(x);
  if (dtype == 0) quant_rows_kernel<F16><<<m, kQT, 0, st>>>(xi, static_cast<int8_t*>(out_i8), static_cast<_Float16*>(scale), k);
  else quant_rows_kernel<BF16><<<m, kQT, 0, st>>>(xi, static_cast<int8_t*>(out_i8), static_cast<_Float16*>(scale), k);
  return 0;
}

int launch_gelu_quant_per_token(const void* x, void* out_i8, void* scale, void* tmp, int m, int k, hipStream_t st) {
  gelu_quant_rows_kernel<<<m, kQT, 0, st>>>(static_cast<const uint16_t*>(x), static_cast<int8_t*>(out_i8), static_cast<_Float16*>(scale),
                                            static_cast<uint16_t*>(tmp), k);
  return 0;
}

int launch_layernorm_quant(const void* x, const void* gamma, const void* beta, float eps, void* out_i8, void* scale, int m, int k,
                           int per_token, int dtype, hipStream_t st) {
  if (k > kQT * kLnVec * 8) return -1;
  const auto* xi = static_cast<const uint16_t*>(x);
  const auto* gi = static_cast<const uint16_t*>(gamma);
  const auto* bi = static_cast<const uint16_t*>(beta);
  if (dtype == 0) layernorm_quant_kernel<F16><<<m, kQT, 0, st>>>(xi, gi, bi, eps, static_cast<int8_t*>(out_i8), static_cast<_Float16*>(scale), k, per_token);
  else layernorm_quant_kernel<BF16><<<m, kQT, 0, st>>>(xi, gi, bi, eps, static_cast<int8_t*>(out_i8), static_cast<_Float16*>(scale), k, per_token);
  return 0;
}

}  // namespace awq
