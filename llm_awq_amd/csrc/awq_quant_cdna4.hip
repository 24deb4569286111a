// AWQ quantisation on the device (gfx950): the group quantiser + packer and the clip search.  Both evaluate the grid of awq_quant_grid.hpp, the
// reference's pseudo_quantize_tensor(zero_point=True) as torch evaluates it on T tensors; DESIGN.md "AWQ quantisation" holds the contract.
//
//  quantize_group_kernel  one block = 16 rows x one group of 128 k, 256 threads, 8 consecutive k per thread (one 16-byte load / store); the
//                         group's extremes meet by four lane exchanges inside a 16-lane row; the recovered integers pass through 2 KiB of LDS
//                         and leave as one u32 per thread: the tile's 1 KiB of the cdna4 interleave, or four packed rows x 128 columns of v2.
//                         Blocks with a group index in [K/128, gpad) write the zero pad rows of scales / scaled_zeros.
//  clip_search_kernel     one block = 32 rows x one group, four waves.  Phase A: the waves build w and the n_steps quantised candidates as
//                         [set][32 rows][128 k] T images in LDS (8 KiB each, 16-byte chunks XOR-swizzled by the row).  Phase B: wave v takes the
//                         32-token tiles v, v + 4, ...; x is the A operand straight from global memory (16 bytes per lane and k-step), a set is
//                         the B operand (ds_read_b128), so a lane of v_mfma_f32_32x32x16 holds ONE weight row and 16 tokens and the squared
//                         difference sums into one fp32 per lane and candidate.  Phase C: the 4 x 2 partials of a row are added in a fixed
//                         order.  A cell's sum order depends on S alone.  No workspace, no atomics.
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_quant_grid.hpp"

namespace awq {
namespace {

using qgrid::Grid;
using qgrid::T16;

// torch.clamp(v, lo, hi): a value equal to a bound is kept as it is (its sign of zero included)
__device__ __forceinline__ float clamp_keep(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool BF>
__device__ __forceinline__ void unpack8(const u32x4& raw, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = T16<BF>::from_bits((uint16_t)(raw[j] & 0xffffu));
    v[2 * j + 1] = T16<BF>::from_bits((uint16_t)(raw[j] >> 16));
  }
}

template <bool BF>
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (u32)T16<BF>::to_bits(v[2 * j]) | ((u32)T16<BF>::to_bits(v[2 * j + 1]) << 16);
  return r;
}

constexpr int kQRows = 16;  // rows of a quantiser block: one cdna4 tile

template <bool BF>
__global__ __launch_bounds__(256) void quantize_group_kernel(const uint16_t* __restrict__ w, long ldw, const uint16_t* __restrict__ col_scale,
                                                            const uint16_t* __restrict__ clip_max, uint16_t* __restrict__ w_fake,
                                                            uint16_t* __restrict__ scales, uint16_t* __restrict__ scaled_zeros,
                                                            uint16_t* __restrict__ zeros, u32* __restrict__ qweight, int N, int K, int G,
                                                            int n_bit, int cdna4) {
  using R = T16<BF>;
  __shared__ __attribute__((aligned(16))) uint8_t q_lds[kQRows][kGroup];
  const int g = blockIdx.x, n0 = blockIdx.y * kQRows, tid = threadIdx.x;
  if (g >= G) {  // a pad row of the checkpoint layout [gpad, N]
    if (tid < kQRows && n0 + tid < N) {
      if (scales) scales[(size_t)g * N + n0 + tid] = 0;
      if (scaled_zeros) scaled_zeros[(size_t)g * N + n0 + tid] = 0;
    }
    return;
  }
  const int r = tid >> 4, c = tid & 15, n = n0 + r;
  const bool valid = n < N;
  const int k0 = g * kGroup + c * 8;
  float v[8], cs[8];
  u32x4 raw = {0u, 0u, 0u, 0u};
  if (valid) raw = *reinterpret_cast<const u32x4*>(w + (size_t)n * ldw + k0);
  unpack8<BF>(raw, v);
  if (col_scale) {
    unpack8<BF>(*reinterpret_cast<const u32x4*>(col_scale + k0), cs);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = R::round(v[j] * cs[j]);
  }
  if (clip_max && valid) {
    const float cm = R::from_bits(clip_max[(size_t)n * G + g]);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = clamp_keep(v[j], -cm, cm);
  }
  float lo = v[0], hi = v[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    lo = fminf(lo, v[j]);
    hi = fmaxf(hi, v[j]);
  }
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {  // the 16 lanes of a row are consecutive lanes of one wave
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
  }
  const Grid<BF> gr(lo, hi, n_bit);
  float out[8];
  uint8_t qi[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float fk = gr.fake(v[j]);
    qi[j] = (uint8_t)(gr.recover(fk) & 0xF);
    out[j] = col_scale ? R::round(fk / cs[j]) : fk;
  }
  if (valid) {
    if (w_fake) *reinterpret_cast<u32x4*>(w_fake + (size_t)n * K + k0) = pack8<BF>(out);
    if (c == 0) {
      if (scales) scales[(size_t)g * N + n] = R::to_bits(gr.scale);
      if (scaled_zeros) scaled_zeros[(size_t)g * N + n] = R::to_bits(gr.scaled_zero());
      if (zeros) zeros[(size_t)n * G + g] = R::to_bits(gr.zero);
    }
  }
  if (!qweight) return;  // (uniform over the block)
  {
    u32x2 pk;
    pk[0] = (u32)qi[0] | ((u32)qi[1] << 8) | ((u32)qi[2] << 16) | ((u32)qi[3] << 24);
    pk[1] = (u32)qi[4] | ((u32)qi[5] << 8) | ((u32)qi[6] << 16) | ((u32)qi[7] << 24);
    *reinterpret_cast<u32x2*>(&q_lds[r][c * 8]) = pk;
  }
  __syncthreads();
  if (cdna4) {
    // word a of lane `lane` of the tile, nibble p (i = p & 3, hi = p >> 2) = Q[4 nq + 2 (i & 1) + hi][32 a + 8 g8 + 4 (i >> 1) + rr]  (N % 16 == 0)
    const int lane = tid >> 2, a = tid & 3;
    const int g8 = lane >> 4, nq = (lane >> 2) & 3, rr = lane & 3;
    u32 word = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int i = p & 3, h = p >> 2;
      word |= (u32)q_lds[4 * nq + 2 * (i & 1) + h][32 * a + 8 * g8 + 4 * (i >> 1) + rr] << (4 * p);
    }
    qweight[((size_t)blockIdx.y * G + g) * 256 + tid] = word;
  } else {
    // v2 (qmodule.py:26-65): nibble j of int16 column cc of packed row pr; p = 4 (cc % 64) + j is the nibble's place in the 256-nibble block
    const int pr = tid >> 6, cc0 = (tid & 63) * 2;
    if (n0 + 4 * pr < N) {
      u32 word = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int cc = cc0 + e;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = (cc & 63) * 4 + j;
          const int rr = p >> 6, chunk = (p & 63) >> 5, t = p & 31, a = t >> 3, u = t & 7;
          const int kk = (cc >> 6) * 64 + chunk * 32 + 8 * (u & 3) + 2 * a + (u >> 2);
          word |= (u32)q_lds[4 * pr + rr][kk] << (16 * e + 4 * j);
        }
      }
      qweight[((size_t)(n0 / 4 + pr) * K + g * kGroup + cc0) >> 1] = word;
    }
  }
}

// ---- clip search ----
constexpr int kCRows = 32;                          // rows of a clip-search block: the N of one 32x32x16 MFMA
constexpr int kSetBytes = kCRows * kGroup * 2;      // one operand set: 8 KiB
constexpr int kClipHead = 256;                      // per-row amax in front of the sets
constexpr int kMaxSteps = 16;

struct ClipFactors {
  float v[kMaxSteps];
};

__device__ __forceinline__ int set_off(int row, int chunk) { return row * 256 + ((chunk ^ (row & 15)) << 4); }

template <typename DT, bool BF>
__global__ __launch_bounds__(256) void clip_search_kernel(const uint16_t* __restrict__ w, long ldw, const uint16_t* __restrict__ x, long ldx,
                                                         uint16_t* __restrict__ best_max_val, int* __restrict__ best_idx,
                                                         float* __restrict__ err_out, int N, int K, int S, int n_bit, int n_steps,
                                                         ClipFactors f) {
  using R = T16<BF>;
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  float* mrow = reinterpret_cast<float*>(lds);
  uint8_t* sets = lds + kClipHead;
  const int g = blockIdx.x, G = K / kGroup, n0 = blockIdx.y * kCRows, tid = threadIdx.x;

  // ---- phase A: w and the candidates, 16 consecutive k of one row per thread ----
  {
    const int r = tid >> 3, c0 = (tid & 7) * 2, n = n0 + r;
    float v[16];
    u32x4 raw0 = {0u, 0u, 0u, 0u}, raw1 = {0u, 0u, 0u, 0u};
    if (n < N) {
      const uint16_t* p = w + (size_t)n * ldw + g * kGroup + c0 * 8;
      raw0 = *reinterpret_cast<const u32x4*>(p);
      raw1 = *reinterpret_cast<const u32x4*>(p + 8);
    }
    {
      float a[8], b[8];
      unpack8<BF>(raw0, a);
      unpack8<BF>(raw1, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a[j], v[8 + j] = b[j];
    }
    float lo = v[0], hi = v[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      lo = fminf(lo, v[j]);
      hi = fmaxf(hi, v[j]);
    }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      lo = fminf(lo, __shfl_xor(lo, d));
      hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    const float m = fmaxf(fabsf(lo), fabsf(hi));
    if ((tid & 7) == 0) mrow[r] = m;
    *reinterpret_cast<u32x4*>(sets + set_off(r, c0)) = raw0;
    *reinterpret_cast<u32x4*>(sets + set_off(r, c0 + 1)) = raw1;
    for (int i = 0; i < n_steps; ++i) {
      const float mv = R::round(m * f.v[i]);
      // the extremes of the clamped group are the clamped extremes of the group
      const Grid<BF> gr(clamp_keep(lo, -mv, mv), clamp_keep(hi, -mv, mv), n_bit);
      float q0[8], q1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q0[j] = gr.fake(clamp_keep(v[j], -mv, mv));
        q1[j] = gr.fake(clamp_keep(v[8 + j], -mv, mv));
      }
      uint8_t* s = sets + (size_t)(i + 1) * kSetBytes;
      *reinterpret_cast<u32x4*>(s + set_off(r, c0)) = pack8<BF>(q0);
      *reinterpret_cast<u32x4*>(s + set_off(r, c0 + 1)) = pack8<BF>(q1);
    }
  }
  __syncthreads();

  // ---- phase B: D[token][row] = x_tile . set^T on the matrix cores; lane (r, h) holds weight row r and 16 tokens of the tile ----
  const int wv = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  float acc[kMaxSteps];
#pragma unroll
  for (int i = 0; i < kMaxSteps; ++i) acc[i] = 0.0f;
  for (int tile = wv; tile * 32 < S; tile += 4) {
    const int t = tile * 32 + r;
    u32x4 a[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      a[s] = u32x4{0u, 0u, 0u, 0u};
      if (t < S) a[s] = *reinterpret_cast<const u32x4*>(x + (size_t)t * ldx + g * kGroup + 16 * s + 8 * h);
    }
    f32x16 dw = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const u32x4 b = *reinterpret_cast<const u32x4*>(sets + set_off(r, 2 * s + h));
      dw = DT::mfma32(__builtin_bit_cast(typename DT::vec8, a[s]), __builtin_bit_cast(typename DT::vec8, b), dw);
    }
#pragma unroll
    for (int i = 0; i < kMaxSteps; ++i) {
      if (i < n_steps) {  // (uniform)
        const uint8_t* sp = sets + (size_t)(i + 1) * kSetBytes;
        f32x16 dq = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const u32x4 b = *reinterpret_cast<const u32x4*>(sp + set_off(r, 2 * s + h));
          dq = DT::mfma32(__builtin_bit_cast(typename DT::vec8, a[s]), __builtin_bit_cast(typename DT::vec8, b), dq);
        }
        float e = acc[i];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float d = dq[j] - dw[j];
          e = __builtin_fmaf(d, d, e);
        }
        acc[i] = e;
      }
    }
  }

  // ---- phase C: the row's partials (wave, lane half) in a fixed order, selection ----
  __syncthreads();  // every wave is done with the sets: their memory now holds the partials [wave][half][row][16]
  float* part = reinterpret_cast<float*>(sets);
#pragma unroll
  for (int i = 0; i < kMaxSteps; ++i) part[((wv * 2 + h) * kCRows + r) * kMaxSteps + i] = acc[i];
  __syncthreads();
  if (tid < kCRows && n0 + tid < N) {
    const int n = n0 + tid;
    const float m = mrow[tid];
    float best = 1e9f;  // auto_clip.py:37
    int idx = 0;
    for (int i = 0; i < n_steps; ++i) {
      float tot = 0.0f;
#pragma unroll
      for (int p = 0; p < 8; ++p) tot += part[(p * kCRows + tid) * kMaxSteps + i];
      const float e = tot / (float)S;
      if (err_out) err_out[((size_t)n * G + g) * n_steps + i] = e;
      if (e < best) {
        best = e;
        idx = i;
      }
    }
    best_max_val[(size_t)n * G + g] = R::to_bits(R::round(m * f.v[idx]));
    best_idx[(size_t)n * G + g] = idx;
  }
}

}  // namespace

int launch_quantize_group(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                          void* zeros, void* qweight, int layout, int n, int k, int n_bit, int dtype, hipStream_t st) {
  const int G = k / kGroup, gpad = (G + 7) / 8 * 8;
  const long row_tiles = ((long)n + kQRows - 1) / kQRows;
  if (row_tiles > 65535) return -1;
  // (the pad blocks are launched only when a [gpad, N] output is wanted)
  const dim3 grid((scales || scaled_zeros) ? gpad : G, (unsigned)row_tiles);
  auto kern = dtype == 1 ? quantize_group_kernel<true> : quantize_group_kernel<false>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const uint16_t*)w, ldw, (const uint16_t*)col_scale, (const uint16_t*)clip_max,
                     (uint16_t*)w_fake, (uint16_t*)scales, (uint16_t*)scaled_zeros, (uint16_t*)zeros, (u32*)qweight, n, k, G, n_bit,
                     layout);
  return 0;
}

// The same arithmetic text on the host, for host memory: the CPU check of awq_quant_grid.hpp against the torch composition (no GPU involved).
template <bool BF>
static void quantize_group_host_t(const uint16_t* w, long ldw, const uint16_t* col_scale, const uint16_t* clip_max, uint16_t* w_fake, uint16_t* scales,
                                  uint16_t* scaled_zeros, uint16_t* zeros, uint8_t* intweight, int n, int k, int n_bit) {
  using R = T16<BF>;
  const int G = k / kGroup, gpad = (G + 7) / 8 * 8;
  for (int g = G; g < gpad; ++g)
    for (int r = 0; r < n; ++r) {
      if (scales) scales[(size_t)g * n + r] = 0;
      if (scaled_zeros) scaled_zeros[(size_t)g * n + r] = 0;
    }
  for (int r = 0; r < n; ++r)
    for (int g = 0; g < G; ++g) {
      float v[kGroup], cs[kGroup];
      for (int j = 0; j < kGroup; ++j) {
        v[j] = R::from_bits(w[(size_t)r * ldw + g * kGroup + j]);
        if (col_scale) {
          cs[j] = R::from_bits(col_scale[g * kGroup + j]);
          v[j] = R::round(v[j] * cs[j]);
        }
        if (clip_max) {
          const float cm = R::from_bits(clip_max[(size_t)r * G + g]);
          v[j] = v[j] < -cm ? -cm : (v[j] > cm ? cm : v[j]);
        }
      }
      float lo = v[0], hi = v[0];
      for (int j = 1; j < kGroup; ++j) {
        lo = fminf(lo, v[j]);
        hi = fmaxf(hi, v[j]);
      }
      const Grid<BF> gr(lo, hi, n_bit);
      for (int j = 0; j < kGroup; ++j) {
        const float fk = gr.fake(v[j]);
        const size_t at = (size_t)r * k + g * kGroup + j;
        if (intweight) intweight[at] = (uint8_t)(gr.recover(fk) & 0xF);
        if (w_fake) w_fake[at] = R::to_bits(col_scale ? R::round(fk / cs[j]) : fk);
      }
      if (scales) scales[(size_t)g * n + r] = R::to_bits(gr.scale);
      if (scaled_zeros) scaled_zeros[(size_t)g * n + r] = R::to_bits(gr.scaled_zero());
      if (zeros) zeros[(size_t)r * G + g] = R::to_bits(gr.zero);
    }
}

void quantize_group_host(const void* w, long ldw, const void* col_scale, const void* clip_max, void* w_fake, void* scales, void* scaled_zeros,
                         void* zeros, void* intweight, int n, int k, int n_bit, int dtype) {
  auto fn = dtype == 1 ? quantize_group_host_t<true> : quantize_group_host_t<false>;
  fn((const uint16_t*)w, ldw, (const uint16_t*)col_scale, (const uint16_t*)clip_max, (uint16_t*)w_fake, (uint16_t*)scales, (uint16_t*)scaled_zeros,
     (uint16_t*)zeros, (uint8_t*)intweight, n, k, n_bit);
}

int launch_clip_search(const void* w, long ldw, const void* x, long ldx, void* best_max_val, int* best_idx, float* err, int n, int k, int s,
                       int n_bit, int n_grid, int n_steps, int dtype, hipStream_t st) {
  if (n_steps < 1 || n_steps > kMaxSteps || n_grid < 1) return -1;
  const long row_tiles = ((long)n + kCRows - 1) / kCRows;
  if (row_tiles > 65535) return -1;
  ClipFactors f;
  for (int i = 0; i < kMaxSteps; ++i) f.v[i] = i < n_steps ? (float)(1.0 - (double)i / (double)n_grid) : 0.0f;  // auto_clip.py:42, a double
  const int lds = kClipHead + (n_steps + 1 > 2 ? n_steps + 1 : 2) * kSetBytes;  // (the partials of phase C take 16 KiB)
  static LdsOptIn optin[2];
  const dim3 grid(k / kGroup, (unsigned)row_tiles);
  if (dtype == 1) {
    auto kern = clip_search_kernel<BF16, true>;
    optin[1].ensure(reinterpret_cast<const void*>(kern));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const uint16_t*)w, ldw, (const uint16_t*)x, ldx, (uint16_t*)best_max_val, best_idx, err,
                       n, k, s, n_bit, n_steps, f);
  } else {
    auto kern = clip_search_kernel<F16, false>;
    optin[0].ensure(reinterpret_cast<const void*>(kern));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const uint16_t*)w, ldw, (const uint16_t*)x, ldx, (uint16_t*)best_max_val, best_idx, err,
                       n, k, s, n_bit, n_steps, f);
  }
  return 0;
}

}  // namespace awq
