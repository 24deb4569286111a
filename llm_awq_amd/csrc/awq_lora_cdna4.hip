// Multi-LoRA on packed steps (gfx950, wave64): y[t, :] += scaling[a] * (x[t, :] A_a^T) B_a^T with a = adapter_ids[owner of row t], as two launches
// per adapted linear whatever the mix of adapters, decodes and prompt chunks (the BGMV / SGMV pair of the literature).  DESIGN.md "Multi-LoRA"
// states the result by values; tests/lora_oracle.py restates it.
//
//   shrink   ws[s, t, c] = sum over the k of split s of f32(x[t, k]) f32(A_a[c, k])                 grid (KS, ceil(max_seqlen_q / 16), B)
//            One block per (sequence, tile of 16 rows, K split).  The block reads cu[b], cu[b + 1] and adapter_ids[b] as scalar loads (constant
//            address space) and leaves before its first vector load when the tile lies beyond Sq_b, the sequence is inactive or the id names
//            no slot.  Its four waves split the 64-k steps of the split (wave w takes steps w, w + 4, ...); a step is two v_mfma_f32_16x16x32
//            per 16 columns of h: lane (c = lane % 16, g = lane / 16) holds k = 64 i + 32 h + 8 g + {0..7} of x row c (A operand) and of row c
//            of the adapter's A matrix (B operand), loaded straight from global memory to VGPRs.  The four partial tiles meet in LDS and are
//            added as (p0 + p1) + (p2 + p3).  Rows of the tile beyond Sq_b are computed on the clamped address of the sequence's last row and
//            not stored.
//   expand   y[t, n] = T(f32(y[t, n]) + sum_r f32(hT[t, j(n) R + r]) f32(B_a[n, r])),  hT = T(scaling[a] (ws[0] + ws[1] + ...))
//                                                                                                  grid (ceil(N / 256), ceil(max_seqlen_q / 16), B)
//            One block per (sequence, row tile, tile of 256 output columns).  The block sums the KS partials of the h columns its slices need
//            once, in split order, scales and rounds them to T into an LDS image (rows beyond Sq_b are zeros), then every wave takes the
//            16-column groups w, w + 4, ... of the tile: one k-step (R = 16: its upper half zero; R = 32) or two (R = 64) of
//            v_mfma_f32_16x16x32 against B_a fragments loaded straight to VGPRs, and the fused read-add-round-store of y.  A group never
//            straddles a slice (slice ends are multiples of 16).
//   expand on the gate / up pair   h[t, 8 j + c] = T(T(silu(g')) u'),  g' = T(f32(y2[t, 16 j + c]) + d_gate),  u' = T(f32(y2[t, 16 j + 8 + c]) + d_up)
//                                                                                                  grid (ceil(2F / 256), ceil(max_seqlen_q / 16), B)
//            y2 [total_q, 2F] is the UNFUSED output of QuantLlamaMLP's 8 + 8 interleaved gate / up stream (read only), h [total_q, F] is written.
//            A 16-column group of y2 holds 8 gate and 8 up columns: lane c < 8 loads row f of B_gate, lane c >= 8 row F + f of B_up, and the
//            k-step(s) are issued twice with these B registers, once against the gate half of hT and once against the up half; a lane keeps the
//            accumulator of its own slice, so every column's MFMA operands are those of lora_expand_kernel and g' / u' are its bits.  The
//            rounded pair meets in an LDS image of the block's [16][256] tile; after one barrier thread (row, group) reads a gate octet and an
//            up octet from it, silu_mul_octet, one 16-byte store of h.  A tile of an active sequence WITHOUT an adapter leaves in front of the
//            first barrier through the same 16-byte tail on y2 itself (no ws row, pool slot or scaling entry is read).
// All grids come from host arguments only.  KS and the order of every sum depend on (K, RS) alone: a row's bits do not depend on the batch it
// was served in.  No atomics: the fp32 workspace carries the partials from one launch to the next.
// Row indices formed from cu_seqlens_q are clamped into [0, total_q - 1] before they form an address and every write is guarded (awq_varq.hpp).
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_varq.hpp"

namespace awq {
namespace {

constexpr int kLoraThreads = 256, kLoraWaves = 4;
constexpr int kLoraRows = 16;          // rows of x per tile: one MFMA's M
constexpr int kLoraStep = 64;          // k per shrink step (two MFMAs deep)
constexpr int kLoraColTile = 256;      // output columns per expand block: four 16-column groups per wave
constexpr int kLoraSplitBytes = 65536; // bytes of A one shrink block streams (the K-split rule, DESIGN.md "Multi-LoRA")
constexpr int kLoraMaxSplits = 32;
constexpr int kLoraMaxRS = 192;

struct LoraShrinkArgs {
  const uint16_t* x;
  const uint16_t* a_pool;
  const int* ids;
  const int* cu;  // NULL: rectangular
  float* ws;
  long ldx;
  int max_sq, total_q, slots, k, rs, kper;
};

struct LoraExpandArgs {
  const float* ws;
  const uint16_t* b_pool;
  const float* scaling;
  const int* ids;
  const int* cu;
  uint16_t* y;
  int max_sq, total_q, slots, n, r, rs, ks, n_slices;
  int slice_end[3];
};

// The rows of sequence b, block-uniform: false = nothing to do for tile rt (inactive or empty sequence, tile beyond Sq_b, no adapter).
// start and sq are 64 bits: whatever the array holds, the comparisons do not wrap.
__device__ __forceinline__ bool lora_tile(const int* cu_p, const int* ids_p, int b, int rt, int max_sq, int slots, long long& start, long long& sq,
                                          int& slot) {
  if (cu_p) {
    const const_i32_t cu = as_const_i32(cu_p);
    const int c0 = cu[b], c1 = cu[b + 1];
    start = c0;
    sq = (long long)c1 - c0;
  } else {
    start = (long long)b * max_sq;
    sq = max_sq;
  }
  slot = as_const_i32(ids_p)[b];
  return sq >= 1 && sq <= max_sq && (long long)rt * kLoraRows < sq && (unsigned)slot < (unsigned)slots;
}

// row r of tile rt -> the packed row whose address is formed: rows beyond the sequence fall on its last row, everything into [0, total_q - 1]
__device__ __forceinline__ long long lora_clamped_row(long long start, long long sq, int rt, int r, int total_q) {
  long long t = start + (long long)rt * kLoraRows + r;
  const long long last = start + sq - 1;
  t = t > last ? last : t;
  t = t < 0 ? 0 : t;
  return t > total_q - 1 ? total_q - 1 : t;
}

// ... and whether that row is the tile's own (a write is guarded by it)
__device__ __forceinline__ bool lora_row_owned(long long start, long long sq, int rt, int r, int total_q) {
  const long long s = (long long)rt * kLoraRows + r, t = start + s;
  return s < sq && t >= 0 && t < total_q;
}

template <typename DT, int CT>
__global__ __launch_bounds__(kLoraThreads) void lora_shrink_kernel(const LoraShrinkArgs a) {
  constexpr int NR = CT * 4;  // accumulator registers of a lane
  __shared__ float part[kLoraWaves * NR * 64];
  const int split = blockIdx.x, rt = blockIdx.y, b = blockIdx.z;
  long long start, sq;
  int slot;
  if (!lora_tile(a.cu, a.ids, b, rt, a.max_sq, a.slots, start, sq, slot)) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int K = a.k, RS = a.rs;
  const uint16_t* xrow = a.x + (size_t)lora_clamped_row(start, sq, rt, c, a.total_q) * (size_t)a.ldx;
  const uint16_t* arow[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) arow[ct] = a.a_pool + ((size_t)slot * RS + ct * 16 + c) * (size_t)K;

  const int k0 = split * a.kper, k1 = k0 + a.kper < K ? k0 + a.kper : K;
  const int nsteps = (k1 - k0) / kLoraStep;
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = wave; i < nsteps; i += kLoraWaves) {
    const int ka = k0 + i * kLoraStep + 8 * g;
    u32x4 xv[2], wv[CT][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      xv[h] = *reinterpret_cast<const u32x4*>(xrow + ka + 32 * h);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) wv[ct][h] = *reinterpret_cast<const u32x4*>(arow[ct] + ka + 32 * h);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const typename DT::vec8 av = __builtin_bit_cast(typename DT::vec8, xv[h]);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = DT::mfma(av, __builtin_bit_cast(typename DT::vec8, wv[ct][h]), acc[ct]);
    }
  }
  // D: column lane % 16 = column of h inside its 16-column tile, row 4 (lane / 16) + j = row of x
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) part[(wave * NR + ct * 4 + j) * 64 + lane] = acc[ct][j];
  __syncthreads();
  for (int idx = tid; idx < NR * 64; idx += kLoraThreads) {
    const int r = idx >> 6, ln = idx & 63;
    const int row = (ln >> 4) * 4 + (r & 3), col = (r >> 2) * 16 + (ln & 15);
    if (lora_row_owned(start, sq, rt, row, a.total_q)) {
      const long long t = start + (long long)rt * kLoraRows + row;
      a.ws[((size_t)split * (size_t)a.total_q + (size_t)t) * (size_t)RS + col] =
          (part[idx] + part[NR * 64 + idx]) + (part[2 * NR * 64 + idx] + part[3 * NR * 64 + idx]);
    }
  }
}

template <typename DT, int R>
__global__ __launch_bounds__(kLoraThreads) void lora_expand_kernel(const LoraExpandArgs a) {
  constexpr int LDH = kLoraMaxRS + 8;  // elements per row of the LDS image: 16 bytes of padding
  constexpr int KSTEPS = R == 64 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t hs[kLoraRows * LDH];
  const int ctile = blockIdx.x, rt = blockIdx.y, b = blockIdx.z;
  long long start, sq;
  int slot;
  if (!lora_tile(a.cu, a.ids, b, rt, a.max_sq, a.slots, start, sq, slot)) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int N = a.n, RS = a.rs;
  const int e0 = a.slice_end[0], e1 = a.slice_end[1];
  auto slice_of = [&](int n) { return (n >= e0 ? 1 : 0) + (n >= e1 ? 1 : 0); };  // (ends past the last slice are N: never reached)
  const int nbeg = ctile * kLoraColTile, nend = nbeg + kLoraColTile < N ? nbeg + kLoraColTile : N;
  const int jlo = slice_of(nbeg), jhi = slice_of(nend - 1);

  // hT of the tile's rows and of the slices this column tile meets: KS partials in split order, one product, one rounding
  const float scale = a.scaling[slot];
  const int q4 = R / 4, ncol4 = (jhi - jlo + 1) * q4;  // float4 granules per row
  const size_t split_stride = (size_t)a.total_q * (size_t)RS;
  for (int idx = tid; idx < kLoraRows * ncol4; idx += kLoraThreads) {
    const int row = idx / ncol4, col = jlo * R + (idx - row * ncol4) * 4;
    u32x2 packed = {0u, 0u};
    if (lora_row_owned(start, sq, rt, row, a.total_q)) {
      const float* p = a.ws + (size_t)(start + (long long)rt * kLoraRows + row) * (size_t)RS + col;
      f32x4 sum = *reinterpret_cast<const f32x4*>(p);
      for (int s = 1; s < a.ks; ++s) sum += *reinterpret_cast<const f32x4*>(p + (size_t)s * split_stride);
      packed.x = (u32)DT::from_float(scale * sum[0]) | ((u32)DT::from_float(scale * sum[1]) << 16);
      packed.y = (u32)DT::from_float(scale * sum[2]) | ((u32)DT::from_float(scale * sum[3]) << 16);
    }
    *reinterpret_cast<u32x2*>(&hs[row * LDH + col]) = packed;
  }
  __syncthreads();

  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int n0 = nbeg + wave * 16; n0 < nend; n0 += kLoraWaves * 16) {
    const int j = slice_of(n0);
    const uint16_t* brow = a.b_pool + ((size_t)slot * (size_t)N + n0 + c) * (size_t)R;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      const int r0 = kk * 32 + 8 * g;  // lane (c, g) holds r = r0 + {0..7} of row c of h (A operand) and of row n0 + c of B_a (B operand)
      u32x4 hv = zero, bv = zero;
      if (r0 < R) {
        bv = *reinterpret_cast<const u32x4*>(brow + r0);
        hv = *reinterpret_cast<const u32x4*>(&hs[c * LDH + j * R + r0]);
      }
      acc = DT::mfma(__builtin_bit_cast(typename DT::vec8, hv), __builtin_bit_cast(typename DT::vec8, bv), acc);
    }
    // D: column lane % 16 = output column n0 + c, row 4 g + i = row of the tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * g + i;
      if (lora_row_owned(start, sq, rt, row, a.total_q)) {
        uint16_t* py = a.y + (size_t)(start + (long long)rt * kLoraRows + row) * (size_t)N + n0 + c;
        *py = DT::from_float(DT::to_float(*py) + acc[i]);
      }
    }
  }
}

struct LoraGateUpArgs {
  const float* ws;
  const uint16_t* b_pool;
  const float* scaling;
  const int* ids;
  const int* cu;
  const uint16_t* y2;
  uint16_t* h;
  int max_sq, total_q, slots, n2, ks;
};

// lora_tile that also answers "active, but no adapter": false = the tile has no rows (inactive or empty sequence, tile beyond Sq_b);
// has_adapter says whether slot names one.
__device__ __forceinline__ bool lora_tile_active(const int* cu_p, const int* ids_p, int b, int rt, int max_sq, int slots, long long& start,
                                                 long long& sq, int& slot, bool& has_adapter) {
  if (cu_p) {
    const const_i32_t cu = as_const_i32(cu_p);
    const int c0 = cu[b], c1 = cu[b + 1];
    start = c0;
    sq = (long long)c1 - c0;
  } else {
    start = (long long)b * max_sq;
    sq = max_sq;
  }
  slot = as_const_i32(ids_p)[b];
  has_adapter = (unsigned)slot < (unsigned)slots;
  return sq >= 1 && sq <= max_sq && (long long)rt * kLoraRows < sq;
}

template <typename DT, int R>
__global__ __launch_bounds__(kLoraThreads) void lora_expand_gate_up_kernel(const LoraGateUpArgs a) {
  constexpr int RS = 2 * R;
  constexpr int LDH = RS + 8;            // elements per row of the hT image: 16 bytes of padding
  constexpr int LDP = kLoraColTile + 8;  // ... and of the g' / u' image
  constexpr int KSTEPS = R == 64 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t hs[kLoraRows * LDH];
  __shared__ __attribute__((aligned(16))) uint16_t ps[kLoraRows * LDP];
  const int ctile = blockIdx.x, rt = blockIdx.y, b = blockIdx.z;
  long long start, sq;
  int slot;
  bool has_adapter;
  if (!lora_tile_active(a.cu, a.ids, b, rt, a.max_sq, a.slots, start, sq, slot, has_adapter)) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int N2 = a.n2, F = N2 >> 1;
  const int nbeg = ctile * kLoraColTile, nend = nbeg + kLoraColTile < N2 ? nbeg + kLoraColTile : N2;
  // the tail's share of the tile: thread (row, group) owns the gate octet and the up octet of one 16-column group of one row
  const int trow = tid >> 4, tn0 = nbeg + 16 * (tid & 15);
  const bool town = tn0 < nend && lora_row_owned(start, sq, rt, trow, a.total_q);
  const size_t tt = (size_t)(start + (long long)rt * kLoraRows + trow);  // (formed into an address only where town holds)

  if (!has_adapter) {  // block-uniform, in front of the first barrier: the interleaved tail on y2 itself
    if (town) {
      const uint16_t* py = a.y2 + tt * (size_t)N2 + tn0;
      *reinterpret_cast<u32x4*>(a.h + tt * (size_t)F + (tn0 >> 1)) =
          silu_mul_octet<DT>(*reinterpret_cast<const u32x4*>(py), *reinterpret_cast<const u32x4*>(py + 8));
    }
    return;
  }

  // hT of the tile's rows, both slices: KS partials in split order, one product, one rounding (lora_expand_kernel's statement)
  const float scale = a.scaling[slot];
  constexpr int ncol4 = RS / 4;  // float4 granules per row
  const size_t split_stride = (size_t)a.total_q * (size_t)RS;
  for (int idx = tid; idx < kLoraRows * ncol4; idx += kLoraThreads) {
    const int row = idx / ncol4, col = (idx - row * ncol4) * 4;
    u32x2 packed = {0u, 0u};
    if (lora_row_owned(start, sq, rt, row, a.total_q)) {
      const float* p = a.ws + (size_t)(start + (long long)rt * kLoraRows + row) * (size_t)RS + col;
      f32x4 sum = *reinterpret_cast<const f32x4*>(p);
      for (int s = 1; s < a.ks; ++s) sum += *reinterpret_cast<const f32x4*>(p + (size_t)s * split_stride);
      packed.x = (u32)DT::from_float(scale * sum[0]) | ((u32)DT::from_float(scale * sum[1]) << 16);
      packed.y = (u32)DT::from_float(scale * sum[2]) | ((u32)DT::from_float(scale * sum[3]) << 16);
    }
    *reinterpret_cast<u32x2*>(&hs[row * LDH + col]) = packed;
  }
  __syncthreads();

  const u32x4 zero = {0u, 0u, 0u, 0u};
  const bool is_up = c >= 8;
  for (int n0 = nbeg + wave * 16; n0 < nend; n0 += kLoraWaves * 16) {
    const int f = (n0 >> 1) + (c & 7);  // y2 column n0 + c is gate row f (c < 8) or up row f (c >= 8): pool row f or F + f
    const uint16_t* brow = a.b_pool + ((size_t)slot * (size_t)N2 + (is_up ? F + f : f)) * (size_t)R;
    f32x4 acc_g = {0.f, 0.f, 0.f, 0.f}, acc_u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      const int r0 = kk * 32 + 8 * g;  // lane (c, g) holds r = r0 + {0..7} of row c of a half of hT (A operand) and of its row of B_a (B operand)
      u32x4 hg = zero, hu = zero, bv = zero;
      if (r0 < R) {
        bv = *reinterpret_cast<const u32x4*>(brow + r0);
        hg = *reinterpret_cast<const u32x4*>(&hs[c * LDH + r0]);
        hu = *reinterpret_cast<const u32x4*>(&hs[c * LDH + R + r0]);
      }
      const typename DT::vec8 bf = __builtin_bit_cast(typename DT::vec8, bv);
      acc_g = DT::mfma(__builtin_bit_cast(typename DT::vec8, hg), bf, acc_g);
      acc_u = DT::mfma(__builtin_bit_cast(typename DT::vec8, hu), bf, acc_u);
    }
    // D: column lane % 16 = y2 column n0 + c, row 4 g + i = row of the tile; the lane keeps the accumulator of its own slice
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * g + i;
      if (lora_row_owned(start, sq, rt, row, a.total_q)) {
        const uint16_t yv = a.y2[(size_t)(start + (long long)rt * kLoraRows + row) * (size_t)N2 + n0 + c];
        ps[row * LDP + (n0 - nbeg) + c] = DT::from_float(DT::to_float(yv) + (is_up ? acc_u[i] : acc_g[i]));
      }
    }
  }
  __syncthreads();
  if (town) {
    const uint16_t* pp = &ps[trow * LDP + (tn0 - nbeg)];
    *reinterpret_cast<u32x4*>(a.h + tt * (size_t)F + (tn0 >> 1)) =
        silu_mul_octet<DT>(*reinterpret_cast<const u32x4*>(pp), *reinterpret_cast<const u32x4*>(pp + 8));
  }
}

template <typename DT>
int lora_shrink_dispatch(const LoraShrinkArgs& a, dim3 grid, hipStream_t st) {
  switch (a.rs / 16) {
    case 1: hipLaunchKernelGGL((lora_shrink_kernel<DT, 1>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 2: hipLaunchKernelGGL((lora_shrink_kernel<DT, 2>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 3: hipLaunchKernelGGL((lora_shrink_kernel<DT, 3>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 4: hipLaunchKernelGGL((lora_shrink_kernel<DT, 4>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 6: hipLaunchKernelGGL((lora_shrink_kernel<DT, 6>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 8: hipLaunchKernelGGL((lora_shrink_kernel<DT, 8>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 12: hipLaunchKernelGGL((lora_shrink_kernel<DT, 12>), grid, dim3(kLoraThreads), 0, st, a); break;
    default: return -1;
  }
  return 0;
}

template <typename DT>
int lora_expand_dispatch(const LoraExpandArgs& a, dim3 grid, hipStream_t st) {
  switch (a.r) {
    case 16: hipLaunchKernelGGL((lora_expand_kernel<DT, 16>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 32: hipLaunchKernelGGL((lora_expand_kernel<DT, 32>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 64: hipLaunchKernelGGL((lora_expand_kernel<DT, 64>), grid, dim3(kLoraThreads), 0, st, a); break;
    default: return -1;
  }
  return 0;
}

template <typename DT>
int lora_gate_up_dispatch(const LoraGateUpArgs& a, int r, dim3 grid, hipStream_t st) {
  switch (r) {
    case 16: hipLaunchKernelGGL((lora_expand_gate_up_kernel<DT, 16>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 32: hipLaunchKernelGGL((lora_expand_gate_up_kernel<DT, 32>), grid, dim3(kLoraThreads), 0, st, a); break;
    case 64: hipLaunchKernelGGL((lora_expand_gate_up_kernel<DT, 64>), grid, dim3(kLoraThreads), 0, st, a); break;
    default: return -1;
  }
  return 0;
}

bool lora_batch_ok(int batch, int max_seqlen_q, int total_q, int slots) {
  return batch >= 1 && batch <= 65535 && max_seqlen_q >= 1 && (max_seqlen_q + kLoraRows - 1) / kLoraRows <= 65535 && total_q >= 1 && slots >= 1;
}

}  // namespace

// {KS, k per split, expand column tile, waves per block}.  A shrink block streams about kLoraSplitBytes of A: k per split = that many bytes over
// the RS rows of A, in whole 64-k steps, at least one step per wave; KS is capped, and the steps are then dealt evenly (every split but the last
// takes `k per split`, the last the rest, never nothing).  A function of (k, rs) alone.
int lora_plan(int k, int r, int n_slices, int out[4]) {
  if ((r != 16 && r != 32 && r != 64) || n_slices < 1 || n_slices > 3 || k < kLoraStep || (k % kLoraStep) != 0) return -1;
  const int rs = r * n_slices, steps = k / kLoraStep;
  int per = kLoraSplitBytes / (2 * rs) / kLoraStep;  // steps of a split by bytes
  if (per < kLoraWaves) per = kLoraWaves;
  int ks = (steps + per - 1) / per;
  if (ks > kLoraMaxSplits) ks = kLoraMaxSplits;
  per = (steps + ks - 1) / ks;
  ks = (steps + per - 1) / per;
  out[0] = ks;
  out[1] = per * kLoraStep;
  out[2] = kLoraColTile;
  out[3] = kLoraWaves;
  return 0;
}

size_t lora_workspace_bytes(int total_q, int k, int r, int n_slices) {
  int plan[4];
  if (total_q < 1 || lora_plan(k, r, n_slices, plan) != 0) return 0;
  return (size_t)plan[0] * (size_t)total_q * (size_t)(r * n_slices) * sizeof(float);
}

int launch_lora_shrink(const void* x, long ldx, const void* a_pool, const int* adapter_ids, const int* cu_seqlens_q, void* ws, int batch,
                       int max_seqlen_q, int total_q, int slots, int k, int r, int n_slices, int dtype, hipStream_t st) {
  int plan[4];
  if (lora_plan(k, r, n_slices, plan) != 0 || !lora_batch_ok(batch, max_seqlen_q, total_q, slots) || ldx < k || (ldx % 8) != 0) return -1;
  const LoraShrinkArgs a = {(const uint16_t*)x, (const uint16_t*)a_pool, adapter_ids, cu_seqlens_q, (float*)ws, ldx, max_seqlen_q, total_q, slots, k,
                            r * n_slices, plan[1]};
  const dim3 grid(plan[0], (max_seqlen_q + kLoraRows - 1) / kLoraRows, batch);
  return dtype == 0 ? lora_shrink_dispatch<F16>(a, grid, st) : lora_shrink_dispatch<BF16>(a, grid, st);
}

int launch_lora_expand(const void* ws, const void* b_pool, const float* scaling, const int* adapter_ids, const int* cu_seqlens_q, void* y, int batch,
                       int max_seqlen_q, int total_q, int slots, int n, int k, int r, const int* slice_end, int n_slices, int dtype, hipStream_t st) {
  int plan[4];
  if (lora_plan(k, r, n_slices, plan) != 0 || !lora_batch_ok(batch, max_seqlen_q, total_q, slots) || n < 16 || (n % 16) != 0) return -1;
  LoraExpandArgs a = {(const float*)ws, (const uint16_t*)b_pool, scaling, adapter_ids, cu_seqlens_q, (uint16_t*)y, max_seqlen_q, total_q, slots, n, r,
                      r * n_slices, plan[0], n_slices, {n, n, n}};
  int prev = 0;
  for (int j = 0; j < n_slices; ++j) {
    if (slice_end[j] <= prev || (slice_end[j] % 16) != 0) return -1;
    a.slice_end[j] = prev = slice_end[j];
  }
  if (prev != n) return -1;
  const dim3 grid((n + kLoraColTile - 1) / kLoraColTile, (max_seqlen_q + kLoraRows - 1) / kLoraRows, batch);
  return dtype == 0 ? lora_expand_dispatch<F16>(a, grid, st) : lora_expand_dispatch<BF16>(a, grid, st);
}

int launch_lora_expand_gate_up(const void* ws, const void* b_pool, const float* scaling, const int* adapter_ids, const int* cu_seqlens_q,
                               const void* y2, void* h, int batch, int max_seqlen_q, int total_q, int slots, int n2, int k, int r, int dtype,
                               hipStream_t st) {
  int plan[4];
  if (lora_plan(k, r, 2, plan) != 0 || !lora_batch_ok(batch, max_seqlen_q, total_q, slots) || n2 < 16 || (n2 % 16) != 0) return -1;
  const LoraGateUpArgs a = {(const float*)ws, (const uint16_t*)b_pool, scaling, adapter_ids, cu_seqlens_q, (const uint16_t*)y2, (uint16_t*)h,
                            max_seqlen_q, total_q, slots, n2, plan[0]};
  const dim3 grid((n2 + kLoraColTile - 1) / kLoraColTile, (max_seqlen_q + kLoraRows - 1) / kLoraRows, batch);
  return dtype == 0 ? lora_gate_up_dispatch<F16>(a, r, grid, st) : lora_gate_up_dispatch<BF16>(a, r, grid, st);
}

}  // namespace awq
