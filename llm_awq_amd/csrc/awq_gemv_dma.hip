// Decode GEMV on cdna4-interleaved weights, LDS-DMA streaming form, 1 <= M <= 8, bf16 and fp16 (gfx950).
// Replaces gemv_kernel (awq/kernels/csrc/quantization_new/gemv/gemv_cuda.cu:74-229) behind WQLinear.forward for decode and, with
// EPI = 1 / 2, QuantLlamaMLP's gate/up pair + SiLU*mul (tinychat/modules/fused_mlp.py:36-83).
//
// Why this form (DESIGN.md "Decode GEMV"; profiles/r02_*): the register-ring kernel (awq_gemv_cdna4.hip) keeps ONE chunk per wave in
// flight -- ~28 KiB per CU -- and its slowest waves receive their first bytes last and then pay one full queue round trip per
// chunk (profiles/r01_gemv_trace.txt: the median wave of the gate/up launch ends at 9.8 us, the last at 15.7 us).  Here every wave
// requests its weight tiles up front with `buffer_load_dwordx4 ... lds` (LDS-DMA: no VGPRs, one instruction per KiB), up to D tiles
// deep into a wave-private LDS ring, so a CU has ~100 KiB in flight from the first microsecond and the memory system is never
// waiting for a dependent request; the math trails the stream and reads the tiles back from LDS (one ds_read_b128 per tile).
//   * block = one 16-row slab (EPI 1: the gate slab and its up slab, NS = 2), WAVES waves split K into CONTIGUOUS ranges of TX
//     128-k steps (the slab's K extent is one contiguous stream in the cdna4 layout);
//   * up front per wave: its x slices (M rows x TX x 256 B) and its packed {scale | zero} dwords (NS x TX x 64 B), also by LDS-DMA
//     (older in the vmcnt order than every weight tile, so the first tile wait covers them);
//   * ring of D steps (NS KiB each): step t waits with a COUNTED vmcnt ((D - 1) NS tiles may stay in flight), reads its tile(s), and
//     re-issues the slot for step t + D; the last D steps count down.  All LDS reads of the loop are inline asm: hipcc would
//     otherwise drain the DMA queue (vmcnt(0)) in front of every LDS read that may alias an in-flight DMA;
//   * dequant on the matrix core (Cdna4DequantT: exact q*s+sz, one v_cvt_pk = the reference's rounding), product on
//     v_mfma_f32_16x16x32, fp32 accumulate, split-K partials reduced through LDS, bias / SiLU*mul fused.
#include <string.h>

#include <type_traits>
#include <utility>

#include "../../include/awq_cdna4.h"
#include "awq_decode_plan.hpp"
#include "awq_device.hpp"
#include "awq_dma.hpp"
#include "awq_kernels.hpp"

namespace awq {

// timing probes (builds with AWQ_PROBES=1 only; wrong results): bit 0 = no math (stream only), bit 1 = no weight DMA and no
// waits for it (math only, on whatever the ring holds), bit 2 = no x staging DMA, bit 3 = no scale (sz) staging DMA (tools/gemvd_xprobe.py)
#ifdef AWQ_ENABLE_PROBES
#define DMA_PROBE(p) ((p) & 0xFF)
#else
#define DMA_PROBE(p) 0
#endif
// bit 8 of the same kernel argument (every build): EPI 0 stores its fp32 sums to `out` as float [M, N] instead of rounding them to T
constexpr int kDmaF32Out = 0x100;
// bit 9: the waves split K in INTERLEAVED 128-k steps (wave w: steps w, w + WAVES, ...) instead of contiguous ranges: the tiles a block has in flight at any
// moment are one contiguous run of its slab's stream (launches whose ring is shallower than a wave's K range: down_proj, qkv, o_proj)
constexpr int kDmaInterleave = 0x200;
// The tail of every form of the kernel: split-K reduction of the waves' fp32 partials through LDS, bias / SiLU*mul, store (EPI below)
template <typename DT, int WAVES, int EPI, int NS>
__device__ __forceinline__ void gemv_dma_reduce(char* smem, char* wbase, int wave_bytes, const f32x4 (&acc)[NS], const uint16_t* __restrict__ bias,
                                                uint16_t* __restrict__ out, int M, int N, int probe_, int nb, int lane, int wv) {
  const int i = lane & 15, g = lane >> 4;
  // ---- split-K reduction across the block's waves (fp32) through each wave's own (now idle) ring slots ----
  // acc[r] = C[n = 4g + r][m = i];  wave q's partial of slab s lives at smem + q * wave_bytes + s * 1024
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) reinterpret_cast<float*>(wbase + s * 1024)[r * 64 + lane] = acc[s][r];
  __syncthreads();
  auto to_f = [](uint16_t b) { return DT::to_float(b); };
  if (EPI != 2) {
    if (wv < 4 && i < M) {
      const int r = wv;
      float v[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        float tsum = 0.f;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) tsum += reinterpret_cast<const float*>(smem + q * wave_bytes + s * 1024)[r * 64 + lane];
        v[s] = tsum;
      }
      const int nn = nb * 16 + 4 * g + r;
      if (EPI == 0 && (probe_ & kDmaF32Out)) {
        // K shard of a tensor-parallel row split (awq_w4a16_partial_cdna4): the fp32 sum goes out unrounded, no bias
        reinterpret_cast<float*>(out)[(size_t)i * N + nn] = v[0];
      } else if (EPI == 0) {
        uint16_t o = DT::from_float(v[0]);
        if (bias != nullptr) o = DT::from_float(to_f(o) + to_f(bias[nn]));  // `out + self.bias` in T (qmodule.py:221)
        out[(size_t)i * N + nn] = o;
      } else {
        // fused_mlp.py:79-82: c = F.silu(gate_output) * up_output, every op rounded to T
        const float gt = to_f(DT::from_float(v[0])), up = to_f(DT::from_float(v[NS - 1]));
        const float sl = to_f(DT::from_float(silu_f32(gt)));
        out[(size_t)i * (N >> 1) + nn] = DT::from_float(sl * up);
      }
    }
  } else {
    // rows 0..7 of the slab are gate rows 8 nb .. 8 nb + 7, rows 8..15 the matching up rows: lane (g < 2) pairs with lane + 32
    auto h_of = [&](int r) {  // T(T(silu(gate)) * up) of accumulator register r: the block's fp32 partials summed over its waves
      float gsum = 0.f, usum = 0.f;
#pragma unroll
      for (int q = 0; q < WAVES; ++q) {
        const float* p = reinterpret_cast<const float*>(smem + q * wave_bytes);
        gsum += p[r * 64 + lane];
        usum += p[r * 64 + lane + 32];
      }
      const float gt = to_f(DT::from_float(gsum)), up = to_f(DT::from_float(usum));
      const float sl = to_f(DT::from_float(silu_f32(gt)));
      return DT::from_float(sl * up);
    };
    if (wv < 4 && i < M && g < 2) {
      out[(size_t)i * (N >> 1) + nb * 8 + 4 * g + wv] = h_of(wv);
    }
  }
}

// EPI 0: out[m, n] (+ bias);  EPI 1: qw = [gate; up] stacked along N, out[m, n/2] = silu(gate) * up (two slabs per block);
// EPI 2: gate / up rows interleaved 8 + 8 inside every 16-row slab (fused_mlp.QuantLlamaMLP stacks them that way), out[m, n/2]
template <typename DT, int WAVES, int D, int DQ, int EPI>
__device__ __forceinline__ void gemv_dma_body(char* smem, const uint16_t* __restrict__ x, const u32* __restrict__ qw,
                                              const u32* __restrict__ szp, const uint16_t* __restrict__ bias,
                                              uint16_t* __restrict__ out, int M, int N, int K, int TX, int probe_, int nb) {
  constexpr int NS = EPI == 1 ? 2 : 1;
  const int probe = DMA_PROBE(probe_);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int nit = K >> 7;
  const int TXp = (TX + 3) & ~3;                 // steps covered by the 4-step DMA pieces of x / sz
  const int xrow = TXp * 256 + 16;               // bytes per staged x row (+16: the M rows of an operand land in different banks)
  const int wave_bytes = D * NS * 1024 + NS * TXp * 64 + M * xrow;
  char* wbase = smem + wv * wave_bytes;
  char* ring = wbase;                            // [D][NS] tiles of 1 KiB
  char* szs = wbase + D * NS * 1024;             // [NS][TXp] x 64 B
  char* xs = szs + NS * TXp * 64;                // [M][xrow]
  const bool il = (probe_ & kDmaInterleave) != 0;
  const int s0 = il ? wv : wv * TX;              // this wave's first k-step
  const int sk = il ? WAVES : 1;                 // ... and the distance to its next one

  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(qw), 0, (N >> 4) * nit * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(szp), 0, (N >> 4) * nit * 64, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), 0, M * K * 2, 0x00020000);
  u32 slab_tile[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) slab_tile[s] = ((u32)nb + (u32)s * (u32)(N >> 5)) * (u32)nit;

  const u32 lane16 = lane * 16u;
  auto issue = [&](int t, int slot) {  // weight tile(s) of local step t into ring slot `slot`
    const u32 kg = (u32)min(s0 + sk * t, nit - 1);  // steps past the end (ragged K split) re-read the last tile; their math is skipped
    if (probe & 2) return;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      dma_to_lds<16, 2>(rw, ring + (slot * NS + s) * 1024, lane16, (slab_tile[s] + kg) * 1024u);
  };
  // ---- up front.  The first weight tile goes out FIRST (it has the longest way to come), then the packed scales and the x
  // slices (out-of-range pieces read 0 through the buffer descriptor), then the rest of the ring: step 0's counted wait
  // (D - 1 tiles may stay in flight) covers everything older than tile 1 ----
  issue(0, 0);
  // a staging piece covers four of the wave's steps: lane / 16 picks the step (sk steps apart in the source), lane % 16 its 4 / 16 bytes
  const u32 sz_voff = (u32)(lane >> 4) * (u32)(sk * 64) + (u32)(lane & 15) * 4u, x_voff = (u32)(lane >> 4) * (u32)(sk * 256) + (u32)(lane & 15) * 16u;
  if (!(probe & 8)) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
      for (int q = 0; q < TXp; q += 4)
        dma_to_lds<4, 0>(rs, szs + (s * TXp + q) * 64, sz_voff, (slab_tile[s] + (u32)(s0 + sk * q)) * 64u);
  }
  if (!(probe & 4)) {
    for (int r = 0; r < M; ++r)
      for (int q = 0; q < TXp; q += 4)
        dma_to_lds<16, 0>(rx, xs + r * xrow + q * 256, x_voff, ((u32)r * (u32)K + (u32)(s0 + sk * q) * 128u) * 2u);
  }
#pragma unroll
  for (int d = 1; d < D; ++d) issue(d, d);
  using vec8 = typename DT::vec8;
  Cdna4DequantT<DT> cd;   // DQ 0: sz_packed in T
  Cdna4DequantH<DT> ch;   // DQ 1: sz_half, f16-mantissa extraction
  if (DQ == 0) cd.init(lane);
  else ch.init(lane);
  const int mrow = min(i, M - 1);
  const u32 lds0 = (u32)(size_t)(__attribute__((address_space(3))) char*)wbase;
  const u32 ring_lane = lds0 + lane16;
  const u32 sz_lane = lds0 + D * NS * 1024 + i * 4;
  const u32 x_lane = lds0 + D * NS * 1024 + NS * TXp * 64 + mrow * xrow + g * 16;

  f32x4 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};

  int slot = 0;
  auto step = [&](int t, auto vm_, auto reissue_) {
    constexpr int VM = decltype(vm_)::value;
    constexpr bool REISSUE = decltype(reissue_)::value;
    u32x4 w[NS], xo[4];
    u32 sz[NS];
    const u32 ra = ring_lane + slot * (NS * 1024), sa = sz_lane + t * 64, xa = x_lane + t * 256;
    if (!(probe & 2)) dma_wait_vm<VM>();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s == 0) asm volatile("ds_read_b128 %0, %1 offset:0" : "=v"(w[s]) : "v"(ra) : "memory");
      else asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(w[s]) : "v"(ra) : "memory");
      asm volatile("ds_read_b32 %0, %1" : "=v"(sz[s]) : "v"(sa + s * TXp * 64) : "memory");
    }
    asm volatile("ds_read_b128 %0, %1 offset:0" : "=v"(xo[0]) : "v"(xa) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(xo[1]) : "v"(xa) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(xo[2]) : "v"(xa) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(xo[3]) : "v"(xa) : "memory");
    if (NS == 1)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(sz[0]), "+v"(xo[0]), "+v"(xo[1]), "+v"(xo[2]), "+v"(xo[3]) : : "memory");
    else
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(w[0]), "+v"(w[NS - 1]), "+v"(sz[0]), "+v"(sz[NS - 1]), "+v"(xo[0]), "+v"(xo[1]), "+v"(xo[2]), "+v"(xo[3])
                   :
                   : "memory");
    if (REISSUE) issue(t + D, slot);  // the slot's bytes are in registers: refill it for step t + D
    if (s0 + sk * t < nit && !(probe & 1)) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        vec8 op[4];
        if (DQ == 0) cd.tile_packed(w[s], sz[s], op);
        else ch.tile(w[s], sz[s], op);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[s] = DT::mfma(op[a], __builtin_bit_cast(vec8, xo[a]), acc[s]);
      }
    }
    slot = slot + 1 == D ? 0 : slot + 1;
  };
  int t = 0;
  for (; t < TX - D; ++t) step(t, std::integral_constant<int, (D - 1) * NS>{}, std::true_type{});
  // the last D steps: nothing left to issue, the waits count down
  static_for<0, D>([&](auto j_) {
    constexpr int J = decltype(j_)::value;
    step(t + J, std::integral_constant<int, (D - 1 - J) * NS>{}, std::false_type{});
  });

  gemv_dma_reduce<DT, WAVES, EPI, NS>(smem, wbase, wave_bytes, acc, bias, out, M, N, probe_, nb, lane, wv);
}

// ---- ONE ROW (the decoded token), a wave's TX steps known at compile time and K = WAVES * TX * 128 exactly (launch_dma_cfg picks it) ----
// The same DMAs into the same LDS layout, the same MFMAs on the same operands in the same order as gemv_dma_body at M = 1, TX steps; what
// differs is how a wave issues them (profiles/decode_step_pipeline.txt):
//   * head: with one row and TXp / 4 staging pieces known, the up-front DMAs are a straight line -- tile 0, scale pieces, x pieces, tiles
//     1 .. D - 1 without a branch in between (the run-time loops over rows and pieces put 198 lines between tile 0 and tile 1);
//   * the loop is fully unrolled and software-pipelined over LDS: while step t's dequant and products issue, the x fragments and the
//     scale dword of step t + 1 are being read (they arrived with the first counted wait), and its v_perm / v_fma_mix prep runs under the
//     latency of its weight tile's ds_read_b128 -- the only LDS read that has to follow the step's vmcnt wait;
//   * LDS addresses are `offset:` immediates on three per-lane bases, ring slots are constants, there is no ragged-K test, and the
//     dequant prep is Cdna4DequantH::prep_lean: 36 + 5 VALU and 12 MFMA per step.
// LDS reads return in order: the scale dword(s) and the x fragments of a step go out ahead of its weight tile(s), so a counted
// lgkmcnt(NS) hands over the former while the latter are still on their way.  One asm statement per group of reads (hipcc pads every
// statement boundary with an s_nop); the outputs are early-clobber: a read may not land in the address register of the next one.
template <int NS, int SZ0, int SZ1, int XO>
__device__ __forceinline__ void lds_read_sx(u32 (&sz)[NS], u32x4 (&xo)[4], u32 sz_lane, u32 x_lane) {
  if constexpr (NS == 1)
    asm volatile("ds_read_b32 %0, %5 offset:%7\n\tds_read_b128 %1, %6 offset:%8\n\tds_read_b128 %2, %6 offset:%9\n\t"
                 "ds_read_b128 %3, %6 offset:%10\n\tds_read_b128 %4, %6 offset:%11"
                 : "=&v"(sz[0]), "=&v"(xo[0]), "=&v"(xo[1]), "=&v"(xo[2]), "=&v"(xo[3])
                 : "v"(sz_lane), "v"(x_lane), "n"(SZ0), "n"(XO), "n"(XO + 64), "n"(XO + 128), "n"(XO + 192)
                 : "memory");
  else
    asm volatile("ds_read_b32 %0, %6 offset:%8\n\tds_read_b32 %1, %6 offset:%9\n\tds_read_b128 %2, %7 offset:%10\n\t"
                 "ds_read_b128 %3, %7 offset:%11\n\tds_read_b128 %4, %7 offset:%12\n\tds_read_b128 %5, %7 offset:%13"
                 : "=&v"(sz[0]), "=&v"(sz[NS - 1]), "=&v"(xo[0]), "=&v"(xo[1]), "=&v"(xo[2]), "=&v"(xo[3])
                 : "v"(sz_lane), "v"(x_lane), "n"(SZ0), "n"(SZ1), "n"(XO), "n"(XO + 64), "n"(XO + 128), "n"(XO + 192)
                 : "memory");
}
// counted vmcnt wait for a weight tile (VM 63 = none), its ds_read_b128(s) from ring offset WO, and the hand-over of the step's scale dword(s) and x fragments
template <int NS, int VM, int WO>
__device__ __forceinline__ void lds_wait_read_w(u32x4 (&w)[NS], u32 (&sz)[NS], u32x4 (&xo)[4], u32 ring_lane) {
  if constexpr (NS == 1)
    asm volatile("s_waitcnt vmcnt(%7)\n\tds_read_b128 %0, %6 offset:%8\n\ts_waitcnt lgkmcnt(1)"
                 : "=&v"(w[0]), "+v"(sz[0]), "+v"(xo[0]), "+v"(xo[1]), "+v"(xo[2]), "+v"(xo[3])
                 : "v"(ring_lane), "n"(VM), "n"(WO)
                 : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%9)\n\tds_read_b128 %0, %8 offset:%10\n\tds_read_b128 %1, %8 offset:%11\n\ts_waitcnt lgkmcnt(2)"
                 : "=&v"(w[0]), "=&v"(w[NS - 1]), "+v"(sz[0]), "+v"(sz[NS - 1]), "+v"(xo[0]), "+v"(xo[1]), "+v"(xo[2]), "+v"(xo[3])
                 : "v"(ring_lane), "n"(VM), "n"(WO), "n"(WO + 1024)
                 : "memory");
}
template <typename DT, int WAVES, int D, int DQ, int EPI, int TX>
__device__ __forceinline__ void gemv_dma_body_m1(char* smem, const uint16_t* __restrict__ x, const u32* __restrict__ qw,
                                                 const u32* __restrict__ szp, const uint16_t* __restrict__ bias,
                                                 uint16_t* __restrict__ out, int N, int probe_, int nb) {
  constexpr int NS = EPI == 1 ? 2 : 1;
  constexpr int nit = WAVES * TX, K = nit * 128;
  constexpr int TXp = (TX + 3) & ~3, NP = TXp / 4;      // 4-step DMA pieces of x / sz
  constexpr int kSz = D * NS * 1024;                    // wave-private LDS as in gemv_dma_body: [D][NS] tiles | [NS][TXp] x 64 B | one x row
  constexpr int kX = kSz + NS * TXp * 64;
  constexpr int wave_bytes = kX + TXp * 256 + 16;
  static_assert(D <= TX && wave_bytes <= 65535, "ds_read offsets are 16-bit immediates");
  const int probe = DMA_PROBE(probe_);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  char* wbase = smem + wv * wave_bytes;
  const bool il = (probe_ & kDmaInterleave) != 0;
  const int s0 = il ? wv : wv * TX;              // this wave's first k-step
  const int sk = il ? WAVES : 1;                 // ... and the distance to its next one

  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(qw), 0, (N >> 4) * nit * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(szp), 0, (N >> 4) * nit * 64, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), 0, K * 2, 0x00020000);
  u32 slab_step[NS];                             // global index of this wave's first tile in slab s
#pragma unroll
  for (int s = 0; s < NS; ++s) slab_step[s] = ((u32)nb + (u32)s * (u32)(N >> 5)) * (u32)nit + (u32)s0;

  const u32 lane16 = lane * 16u;
  auto issue = [&](int t, int slot) {  // weight tile(s) of local step t into ring slot `slot` (both compile-time after unrolling)
    if (probe & 2) return;
#pragma unroll
    for (int s = 0; s < NS; ++s) dma_to_lds<16, 2>(rw, wbase + (slot * NS + s) * 1024, lane16, (slab_step[s] + (u32)(sk * t)) * 1024u);
  };
  // ---- up front, one straight line.  Order as in gemv_dma_body: tile 0 first (it has the longest way to come; x and the scales are
  // L2 hits), then the scale and x pieces, then the rest of the ring, so that step 0's counted wait covers everything older than tile 1 ----
  issue(0, 0);
  const u32 sz_voff = (u32)g * (u32)(sk * 64) + (u32)i * 4u, x_voff = (u32)g * (u32)(sk * 256) + (u32)i * 16u;
  if (!(probe & 8)) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int q = 0; q < NP; ++q) dma_to_lds<4, 0>(rs, wbase + kSz + (s * TXp + 4 * q) * 64, sz_voff, (slab_step[s] + (u32)(sk * 4 * q)) * 64u);
  }
  if (!(probe & 4)) {
#pragma unroll
    for (int q = 0; q < NP; ++q) dma_to_lds<16, 0>(rx, wbase + kX + q * 1024, x_voff, (u32)(s0 + sk * 4 * q) * 256u);
  }
#pragma unroll
  for (int d = 1; d < D; ++d) issue(d, d);

  using vec8 = typename DT::vec8;
  Cdna4DequantT<DT> cd;   // DQ 0: sz_packed in T
  Cdna4DequantH<DT> ch;   // DQ 1: sz_half, f16-mantissa extraction
  if (DQ == 0) cd.init(lane);
  else ch.init(lane);
  using Prep = std::conditional_t<DQ == 0, typename Cdna4DequantT<DT>::Prep, typename Cdna4DequantH<DT>::Prep>;
  const u32 lds0 = (u32)(size_t)(__attribute__((address_space(3))) char*)wbase;
  const u32 ring_lane = lds0 + lane16, sz_lane = lds0 + i * 4, x_lane = lds0 + g * 16;

  f32x4 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 w[NS], xo[2][4];   // xo / sz / pp: step t uses half t & 1 while step t + 1's half fills
  u32 sz[2][NS];
  Prep pp[2][NS];

  auto read_sx = [&](auto t_) {
    constexpr int T = decltype(t_)::value, H = T & 1;
    lds_read_sx<NS, kSz + T * 64, kSz + (TXp + T) * 64, kX + T * 256>(sz[H], xo[H], sz_lane, x_lane);
  };
  // tile T (ISSUED = tiles requested so far): wait, read, and step T's prep under that read's latency
  auto fetch_w = [&](auto t_, auto issued_) {
    constexpr int T = decltype(t_)::value, H = T & 1, ISSUED = decltype(issued_)::value;
    __builtin_amdgcn_sched_barrier(0);  // (step T - 1's math stays ahead of the wait for tile T)
    if constexpr (T == 0) {  // (step 0's x fragments and scale dword arrive with tile 0's wait; later steps read theirs a step ahead)
      if (!(probe & 2)) dma_wait_vm<(ISSUED - 1 - T) * NS>();
      read_sx(t_);
    }
    if (probe & 2) lds_wait_read_w<NS, 63, (T % D) * NS * 1024>(w, sz[H], xo[H], ring_lane);
    else lds_wait_read_w<NS, (ISSUED - 1 - T) * NS, (T % D) * NS * 1024>(w, sz[H], xo[H], ring_lane);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if constexpr (DQ == 0) pp[H][s] = cd.prep(sz[H][s]);
      else {
        pp[H][s] = ch.prep_lean(sz[H][s]);
      }
    }
    // (the prep's results are operands of this wait: it stays in front of it, two and more instructions ahead of the first dequant MFMA)
    if constexpr (DQ == 0) {
      if (NS == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(pp[H][0].cv) : : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[NS - 1]), "+v"(pp[H][0].cv), "+v"(pp[H][NS - 1].cv) : : "memory");
    } else {
      if (NS == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(pp[H][0].c), "+v"(pp[H][0].b) : : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[NS - 1]), "+v"(pp[H][0].c), "+v"(pp[H][NS - 1].c), "+v"(pp[H][0].b), "+v"(pp[H][NS - 1].b) : : "memory");
    }
  };
  fetch_w(std::integral_constant<int, 0>{}, std::integral_constant<int, D>{});
  static_for<0, TX>([&](auto t_) {
    constexpr int T = decltype(t_)::value, H = T & 1;
    constexpr bool REISSUE = T + D < TX;
    if (REISSUE) issue(T + D, T % D);  // the slot's bytes are in registers: refill it for step T + D
    if constexpr (T + 1 < TX) {
      read_sx(std::integral_constant<int, T + 1>{});
      __builtin_amdgcn_sched_barrier(0);  // (or the scheduler sinks the reads to the end of the step's math)
    }
    if (!(probe & 1)) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const u32 ws[4] = {w[s].x, w[s].y, w[s].z, w[s].w};
        vec8 op[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          if constexpr (DQ == 0) op[a] = cd.word(ws[a], pp[H][s]);
          else op[a] = ch.word(ws[a], pp[H][s]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[s] = DT::mfma(op[a], __builtin_bit_cast(vec8, xo[H][a]), acc[s]);
      }
    }
    if constexpr (T + 1 < TX) fetch_w(std::integral_constant<int, T + 1>{}, std::integral_constant<int, (T + D < TX ? T + D : TX - 1) + 1>{});
  });
  // (nothing of the tail inside the steps: the scheduler stops here, and the tail's lane arithmetic starts from a value it cannot trace back)
  __builtin_amdgcn_sched_barrier(0);
  int lane_tail = lane;
  asm volatile("" : "+v"(lane_tail));
  gemv_dma_reduce<DT, WAVES, EPI, NS>(smem, wbase, wave_bytes, acc, bias, out, 1, N, probe_, nb, lane_tail, wv);
}

template <typename DT, int WAVES, int D, int DQ, int EPI>
__global__ __launch_bounds__(64 * WAVES) void gemv_dma_kernel(const uint16_t* __restrict__ x, const u32* __restrict__ qw,
                                                               const u32* __restrict__ szp, const uint16_t* __restrict__ bias,
                                                               uint16_t* __restrict__ out, int M, int N, int K, int TX, int probe_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_dma_body<DT, WAVES, D, DQ, EPI>(smem, x, qw, szp, bias, out, M, N, K, TX, probe_, blockIdx.x);
}
// the one-row form; same arguments (M, K, TX are what the template says)
template <typename DT, int WAVES, int D, int DQ, int EPI, int TXC>
__global__ __launch_bounds__(64 * WAVES) void gemv_dma_kernel_m1(const uint16_t* __restrict__ x, const u32* __restrict__ qw,
                                                                  const u32* __restrict__ szp, const uint16_t* __restrict__ bias,
                                                                  uint16_t* __restrict__ out, int M, int N, int K, int TX, int probe_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_dma_body_m1<DT, WAVES, D, DQ, EPI, TXC>(smem, x, qw, szp, bias, out, N, probe_, blockIdx.x);
}

namespace {
DecodeKnobs& g_knobs = g_linear.decode;  // awq_tune_set (tests, tools); the rules that read them: awq_decode_plan.hpp
}  // namespace

int gemv_dma_tune_set(const char* key, int value) {
  if (!strcmp(key, "gemvd_waves")) g_knobs.waves = value;
  else if (!strcmp(key, "gemvd_d")) g_knobs.d = value;
  else if (!strcmp(key, "gemvd_probe")) g_knobs.probe = value;
  else if (!strcmp(key, "gemvd_want")) g_knobs.want = value;
  else if (!strcmp(key, "gemvd_il")) g_knobs.il = value;
  else if (!strcmp(key, "decode_skinny_from")) g_knobs.skinny_from = value;
  else return -1;
  return 0;
}

template <typename DT, int WAVES, int D, int DQ, int EPI>
static void launch_dma_cfg(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                           const DecodeChunk& c, hipStream_t st, int f32out) {
  constexpr int NS = EPI == 1 ? 2 : 1;
  const int flags = (g_knobs.probe & 0xFF) | (f32out ? kDmaF32Out : 0) | (c.interleaved ? kDmaInterleave : 0);
  // one row against the K ranges of the decoded token (Llama-3-8B: K = 4096 over eight waves -- gate/up, o, qkv; K = 14336 over sixteen -- down_proj):
  // the straight-line, pipelined form.  Everything else -- more rows, other step counts, a ragged K split -- runs the general body.
  constexpr int TXC = EPI == 1 ? 0 : ((WAVES == 8 && (D == 2 || D == 4)) ? 4 : ((WAVES == 16 && D == 1) ? 7 : 0));  // (EPI 1's two slabs per step would not fit 80 VGPRs: general body)
  static_assert(TXC == one_row_tx(EPI, WAVES, D), "the plan's one_row_form speaks of this mapping");
  if constexpr (TXC != 0) {
    if (c.one_row_form) {
      auto kern1 = gemv_dma_kernel_m1<DT, WAVES, D, DQ, EPI, TXC>;
      static LdsOptIn optin1;
      if (c.smem_bytes > 64 * 1024) optin1.ensure(reinterpret_cast<const void*>(kern1));
      hipLaunchKernelGGL(kern1, dim3(n / 16 / NS), dim3(64 * WAVES), c.smem_bytes, st, (const uint16_t*)x, (const u32*)qw, (const u32*)szp,
                         (const uint16_t*)bias, (uint16_t*)out, m, n, k, c.tx, flags);
      return;
    }
  }
  auto kern = gemv_dma_kernel<DT, WAVES, D, DQ, EPI>;
  static LdsOptIn optin;
  if (c.smem_bytes > 64 * 1024) optin.ensure(reinterpret_cast<const void*>(kern));
  hipLaunchKernelGGL(kern, dim3(n / 16 / NS), dim3(64 * WAVES), c.smem_bytes, st, (const uint16_t*)x, (const u32*)qw, (const u32*)szp,
                     (const uint16_t*)bias, (uint16_t*)out, m, n, k, c.tx, flags);
}

template <typename DT, int EPI, int DQ>
static int launch_dma_dt(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k,
                         const DecodeChunk& c, hipStream_t st, int f32out) {
#define AWQ_DCASE(W_, D_)                                                           \
  if (c.waves == W_ && c.d == D_) {                                                 \
    launch_dma_cfg<DT, W_, D_, DQ, EPI>(x, qw, szp, bias, out, m, n, k, c, st, f32out); \
    return 0;                                                                       \
  }
  AWQ_DCASE(8, 1) AWQ_DCASE(8, 2) AWQ_DCASE(8, 4) AWQ_DCASE(8, 8)
  AWQ_DCASE(16, 1) AWQ_DCASE(16, 2) AWQ_DCASE(16, 4) AWQ_DCASE(16, 7)
  AWQ_DCASE(4, 1) AWQ_DCASE(4, 2) AWQ_DCASE(4, 4) AWQ_DCASE(4, 7) AWQ_DCASE(4, 8)
#undef AWQ_DCASE
  return -1;  // (a forced gemvd_waves / gemvd_d pair that is not compiled)
}

static int launch_dma_chunk(const void* x, const void* qw, const void* szp, const void* bias, void* out, int n, int k, int epi, int dtype,
                            int szfmt, const DecodeChunk& c, hipStream_t st, int f32out) {
#define AWQ_DDT(DT_, DQ_)                                                                           \
  if (epi == 0) return launch_dma_dt<DT_, 0, DQ_>(x, qw, szp, bias, out, c.rows, n, k, c, st, f32out); \
  if (epi == 1) return launch_dma_dt<DT_, 1, DQ_>(x, qw, szp, bias, out, c.rows, n, k, c, st, 0);      \
  return launch_dma_dt<DT_, 2, DQ_>(x, qw, szp, bias, out, c.rows, n, k, c, st, 0);
  if (szfmt == 1) {
    if (dtype == 0) {
      AWQ_DDT(F16, 1)
    }
    AWQ_DDT(BF16, 1)
  }
  if (dtype == 0) {
    AWQ_DDT(F16, 0)
  }
  AWQ_DDT(BF16, 0)
#undef AWQ_DDT
}

// host-side readers of the plan launch_gemv_dma walks (awq_w4a16_decode_cdna4_plan, awq_w4a16_decode_cdna4_plan_detail).
// gemv_dma_plan: weight passes (0 = not served), *kernel 0 streaming / 1 skinny.  It names ONE kernel for the call: 1 when a single skinny
// launch serves all rows, else 0.  A call served in row chunks asks skinny_takes per chunk, so a chunk could in principle run the skinny
// kernel under an answer of 0; skinny_takes is monotonic in the row count, and over the grid epilogue 0 - 2 x 1 - 8 rows x 1 - 4200 slabs x
// k / 128 in 1 - 129, 224, 448 no chunk does, at the default knobs or with decode_skinny_from forced to 1 or 9.
int gemv_dma_plan(int m, int n, int k, int epi, int* kernel) {
  const DecodePlan p = decode_plan(m, n, k, epi, device_cu_count(), g_knobs);
  if (kernel && p.in_range) *kernel = p.served && p.nchunks == 1 && p.chunk[0].kernel == kDecodeSkinny ? 1 : 0;
  return p.served ? p.nchunks : 0;
}
// out: rows, kernel, waves, tx, d, smem bytes, flags (bit 0 interleaved, bit 1 one-row form), skinny shape x 8 + x_pieces; returns the chunk count
int gemv_dma_plan_detail(int m, int n, int k, int epi, int chunk, int out[8]) {
  const DecodePlan p = decode_plan(m, n, k, epi, device_cu_count(), g_knobs);
  if (!p.served) return 0;
  if (out != nullptr && chunk >= 0 && chunk < p.nchunks) {
    const DecodeChunk& c = p.chunk[chunk];
    const int w[8] = {c.rows, c.kernel, c.waves, c.tx, c.d, c.smem_bytes, (c.interleaved ? 1 : 0) | (c.one_row_form ? 2 : 0),
                      c.kernel == kDecodeSkinny ? c.shape * 8 + c.x_pieces : 0};
    for (int i = 0; i < 8; ++i) out[i] = w[i];
  }
  return p.nchunks;
}

// epi as in the kernel header; returns -1 if the shape is not served.  One launch per chunk of the plan, each a pass over the weights.
int launch_gemv_dma(const void* x, const void* qw, const void* szp, const void* bias, void* out, int m, int n, int k, int epi,
                    int dtype, int szfmt, hipStream_t st, int f32out) {
  const DecodePlan p = decode_leaf_plan(m, n, k, epi, szp != nullptr, bias != nullptr, f32out != 0, device_cu_count(), g_linear);  // (decode_serves: its .served)
  if (!p.served) return -1;
  const size_t ncols = epi ? (size_t)n / 2 : (size_t)n;
  for (int i = 0, r = 0; i < p.nchunks; r += p.chunk[i].rows, ++i) {  // r: the chunk's first row
    const DecodeChunk& c = p.chunk[i];
    const void* xr = (const char*)x + (size_t)r * k * 2;
    void* outr = (char*)out + (size_t)r * ncols * (f32out ? 4 : 2);
    const int rc = c.kernel == kDecodeSkinny ? launch_skinny_decode(xr, qw, szp, bias, outr, c.rows, n, k, epi, dtype, szfmt, st, f32out)
                                             : launch_dma_chunk(xr, qw, szp, bias, outr, n, k, epi, dtype, szfmt, c, st, f32out);
    if (rc != 0) return rc;
  }
  return 0;
}

}  // namespace awq
