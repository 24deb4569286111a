// LM head for decode (gfx950, wave64): the final RMSNorm and the vocabulary GEMV out[M, V] = xn[M, K] W[V, K]^T (+ bias) in ONE launch, and the token
// embedding gather that accepts the sampler's -1 (DESIGN.md "LM head" states both contracts by values; tests/lm_head_oracle.py restates them).
//
// W is nn.Linear.weight as it is loaded (T [V, K] row-major, no repack) and is read ONCE per call whatever M is: up to 64 rows of x are served
// while a weight fragment sits in registers.
//   grid     persistent: block b walks the 64-row vocabulary tiles b, b + grid, ...; the last tile is partial for V % 64 != 0 (rows past V are
//            clamped to row V - 1 for the load and never stored)
//   block    256 threads = 4 waves that split K: wave w takes the 64-k steps w, w + 4, ...  A step is two v_mfma_f32_16x16x32 per (16 rows of x,
//            16 vocabulary rows): lane (c = lane % 16, g = lane / 16) holds k = 64 s + 8 g + {0..7} for the first and + 32 for the second, so
//            the four lanes of a row read 64 contiguous bytes per instruction and the step whole 128-byte lines of 64 weight rows.  Weight
//            fragments go straight from global memory to VGPRs (plain loads: non-temporal ones measured 3 ... 9 % slower), PF steps ahead, in straight-line
//            code so that the waits in front of the MFMAs are counted ones; the ring runs across tile boundaries.  No LDS staging of W.  A ragged
//            last step (K % 64 != 0) is the one predicated step, taken at the end of a tile by the wave whose turn it is.
//   x        A operand, from L2 per step: row r of x is row r % 16 of m-tile r / 16 (MT = ceil(M / 16) m-tiles, a template parameter), rows past M
//            are clamped to row M - 1 and never stored.  With gamma the step normalises its fragment in registers.
//   norm     every block sums the squares of the M rows itself, behind its first weight loads, in the order of rmsnorm_kernel (awq_util.hip):
//            thread t takes the 16-byte granules t, t + 256, ..., a wave butterfly, then (p0 + p1) + (p2 + p3) -- so the fused launch equals
//            ops.rmsnorm + the plain launch in every bit, for any input.
//   reduce   the four waves' partial tiles meet in LDS and are added as (p0 + p1) + (p2 + p3); the bias is added to that sum, in fp32.
// The order of every sum depends on K alone: not on M, not on gamma, not on the grid.  No workspace, no atomics.
// An MFMA row is a dot product of its own A row: a NaN in row b of x stays in row b of the result, so inactive rows (seqlens[b] < 0) need no
// masking on the way in; they are skipped on the way out.  A launch whose rows are all inactive returns before its first weight load.
//   cap      awq_lm_head_softcap (awq_softcap.hpp; Gemma-2's final_logit_softcapping): y <- cap * tanh(y / cap) behind the bias, in fp32, before the
//            one rounding to out_dtype.  A compile-time form: lm_head_softcap_kernel is lm_head_body<.., true>, lm_head_kernel stays <.., false>.
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_softcap.hpp"

namespace awq {
namespace {

using u64 = unsigned long long;
constexpr int kLmThreads = 256, kLmWaves = 4;
constexpr int kLmVT = 4;                  // 16-row vocabulary sub-tiles per tile
constexpr int kLmTile = 16 * kLmVT;       // vocabulary rows per tile
constexpr int kLmStep = 64;               // k per step (two MFMAs deep)
constexpr int kLmNumCU = 256, kLmBlocksPerCU = 2;

struct LmHeadArgs {
  const uint16_t* x;
  const uint16_t* gamma;
  const uint16_t* w;
  const uint16_t* bias;
  const int* seqlens;
  void* out;
  long ldx;
  float eps;
  int m, v, k, out_f32;
};

template <int MT, bool NORM>
struct LmFrag {
  u32x4 w[kLmVT][2];
  u32x4 x[MT][2];
  u32x4 g[NORM ? 2 : 1];
};

// T((f32(x) * rstd) * f32(gamma)) on eight packed values: rmsnorm_kernel's expression
template <typename DT>
__device__ __forceinline__ u32x4 lm_norm8(const u32x4& xv, const u32x4& gv, float rstd) {
  const u32 w4[4] = {xv.x, xv.y, xv.z, xv.w}, g4[4] = {gv.x, gv.y, gv.z, gv.w};
  u32 o4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = (DT::to_float((uint16_t)(w4[e] & 0xFFFFu)) * rstd) * DT::to_float((uint16_t)(g4[e] & 0xFFFFu));
    const float hi = (DT::to_float((uint16_t)(w4[e] >> 16)) * rstd) * DT::to_float((uint16_t)(g4[e] >> 16));
    o4[e] = (u32)DT::from_float(lo) | ((u32)DT::from_float(hi) << 16);
  }
  return u32x4{o4[0], o4[1], o4[2], o4[3]};
}

template <typename DT, int MT, bool NORM, int PF, bool CAP>
__device__ __forceinline__ void lm_head_body(const LmHeadArgs& a, float cap) {
  (void)cap;
  constexpr int NR = MT * kLmVT * 4;  // accumulator registers of a lane
  __shared__ float part[kLmWaves * NR * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int M = a.m, V = a.v, K = a.k;

  // bit b = row b is active; every wave computes the same mask, so the exit is uniform over the block
  const u64 active = __ballot(lane < M && (a.seqlens == nullptr || a.seqlens[lane] >= 0));
  if (active == 0) return;

  const uint16_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int r = mt * 16 + c;
    xrow[mt] = a.x + (size_t)(r < M ? r : M - 1) * (size_t)a.ldx;
  }

  float rstd[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) rstd[mt] = 0.f;
  // the norm's sums: run once per block, AFTER the first weight loads are in flight (they do not depend on it)
  auto row_norms = [&]() {
    if constexpr (!NORM) return;
    const int ng = K >> 3;
    for (int r0 = 0; r0 < M; r0 += 8) {  // eight rows' loads in flight per thread
      float ss[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) ss[j] = 0.f;
      for (int gi = tid; gi < ng; gi += kLmThreads) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = r0 + j < M ? r0 + j : M - 1;
          const u32x4 v = *reinterpret_cast<const u32x4*>(a.x + (size_t)r * (size_t)a.ldx + (size_t)gi * 8);
          const u32 w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = DT::to_float((uint16_t)(w4[e] & 0xFFFFu)), hi = DT::to_float((uint16_t)(w4[e] >> 16));
            ss[j] = __builtin_fmaf(lo, lo, ss[j]);
            ss[j] = __builtin_fmaf(hi, hi, ss[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) ss[j] += __shfl_xor(ss[j], d, 64);
        if (lane == 0 && r0 + j < M) part[(r0 + j) * 4 + wave] = ss[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int r = mt * 16 + c < M ? mt * 16 + c : M - 1;
      const float tot = (part[r * 4 + 0] + part[r * 4 + 1]) + (part[r * 4 + 2] + part[r * 4 + 3]);
      rstd[mt] = rsqrtf(tot / (float)K + a.eps);
    }
    __syncthreads();  // part is the reduction buffer from here on
  };

  const int ntiles = (V + kLmTile - 1) / kLmTile;
  const int nfull = K / kLmStep;                                                   // steps with all 64 k; the k tail (K % 64) is one more, ragged step
  const int cnt = wave < nfull ? (nfull - wave + kLmWaves - 1) / kLmWaves : 0;     // this wave's full steps: wave, wave + 4, ...
  const bool own_tail = (K % kLmStep) != 0 && (nfull % kLmWaves) == wave;          // ... and the ragged one is the last step of its wave
  const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;  // >= 1: the grid never exceeds the tiles

  f32x4 acc[MT][kLmVT];
  auto clear = [&]() {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int vt = 0; vt < kLmVT; ++vt) acc[mt][vt] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // the 16 vocabulary rows a lane column stands for, per sub-tile; rows past V (the last tile's tail, and the tiles a prefetch names past the
  // block's last) are clamped to row V - 1: a valid read whose result is never stored
  auto rows_of = [&](const uint16_t* (&wrow)[kLmVT], int tile) {
#pragma unroll
    for (int vt = 0; vt < kLmVT; ++vt) {
      const long n = (long)tile * kLmTile + vt * 16 + c;
      wrow[vt] = a.w + (size_t)(n < V ? n : V - 1) * (size_t)K;
    }
  };
  // a full step: no predicate, so the loads sit in straight-line code and the waits in front of the MFMAs are counted ones.  Lane (c, g) takes
  // k = 64 s + 32 h + 8 g + {0..7}: the four lanes of a row read 64 contiguous bytes per instruction, the two halves one 128-byte line
  auto load = [&](LmFrag<MT, NORM>& f, const uint16_t* const (&wrow)[kLmVT], int i) {
    const int ka = (wave + kLmWaves * i) * kLmStep + 8 * g;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kh = ka + 32 * h;
#pragma unroll
      for (int vt = 0; vt < kLmVT; ++vt) f.w[vt][h] = *reinterpret_cast<const u32x4*>(wrow[vt] + kh);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) f.x[mt][h] = *reinterpret_cast<const u32x4*>(xrow[mt] + kh);
      if constexpr (NORM) f.g[h] = *reinterpret_cast<const u32x4*>(a.gamma + kh);
    }
  };
  // the ragged step: granules past K are zeros and are not loaded
  auto load_tail = [&](LmFrag<MT, NORM>& f, const uint16_t* const (&wrow)[kLmVT]) {
    const int ka = nfull * kLmStep + 8 * g;
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kh = ka + 32 * h;
      const bool ok = kh < K;
#pragma unroll
      for (int vt = 0; vt < kLmVT; ++vt) f.w[vt][h] = ok ? ldg_nt_u32x4(reinterpret_cast<const u32*>(wrow[vt] + kh)) : zero;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) f.x[mt][h] = ok ? *reinterpret_cast<const u32x4*>(xrow[mt] + kh) : zero;
      if constexpr (NORM) f.g[h] = ok ? *reinterpret_cast<const u32x4*>(a.gamma + kh) : zero;
    }
  };
  auto compute = [&](const LmFrag<MT, NORM>& f) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        u32x4 xa = f.x[mt][h];
        if constexpr (NORM) xa = lm_norm8<DT>(xa, f.g[h], rstd[mt]);
        const typename DT::vec8 av = __builtin_bit_cast(typename DT::vec8, xa);
#pragma unroll
        for (int vt = 0; vt < kLmVT; ++vt) acc[mt][vt] = DT::mfma(av, __builtin_bit_cast(typename DT::vec8, f.w[vt][h]), acc[mt][vt]);
      }
  };
  // the end of a tile: this wave's ragged step if it owns it, then the four partial tiles meet in LDS and are added in a fixed order
  auto finish_tile = [&](int tile) {
    if (own_tail) {
      const uint16_t* wrow[kLmVT];
      rows_of(wrow, tile);
      LmFrag<MT, NORM> f;
      load_tail(f, wrow);
      compute(f);
    }
    const int n0 = tile * kLmTile;
    // D: column lane % 16 = vocabulary row, row 4 (lane / 16) + j = row of x
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int vt = 0; vt < kLmVT; ++vt)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(wave * NR + (mt * kLmVT + vt) * 4 + j) * 64 + lane] = acc[mt][vt][j];
    __syncthreads();
    for (int idx = tid; idx < NR * 64; idx += kLmThreads) {
      const int r = idx >> 6, ln = idx & 63;
      const int mrow = (r / (kLmVT * 4)) * 16 + (ln >> 4) * 4 + (r & 3);
      const int n = n0 + ((r >> 2) % kLmVT) * 16 + (ln & 15);
      if (mrow < M && ((active >> mrow) & 1ull) && n < V) {
        float y = (part[idx] + part[NR * 64 + idx]) + (part[2 * NR * 64 + idx] + part[3 * NR * 64 + idx]);
        if (a.bias) y += DT::to_float(a.bias[n]);
        if constexpr (CAP) y = softcap_logit(y, cap);
        const size_t o = (size_t)mrow * (size_t)V + (size_t)n;
        if (a.out_f32) reinterpret_cast<float*>(a.out)[o] = y;
        else reinterpret_cast<uint16_t*>(a.out)[o] = DT::from_float(y);
      }
    }
    __syncthreads();
    clear();
  };

  clear();
  if (cnt == 0) {  // K below this wave's first full step: nothing to stream, but the norm's and the tile's barriers are the block's
    row_norms();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) finish_tile(tile);
    return;
  }
  // The wave's steps of all the block's tiles are ONE sequence: the ring of PF steps in flight runs across tile boundaries, so the weight stream
  // does not drain where a tile ends.  The load cursor (lt, li) runs PF steps ahead of the compute cursor (ct, ci); past the block's last tile
  // it names clamped rows (see rows_of), which costs PF redundant steps per block.
  const int total = my_tiles * cnt;
  int lt = blockIdx.x, li = 0, ct = blockIdx.x, ci = 0;
  const uint16_t* wload[kLmVT];
  rows_of(wload, lt);
  auto advance_load = [&]() {
    if (++li == cnt) {
      li = 0;
      lt += gridDim.x;
      rows_of(wload, lt < ntiles ? lt : ntiles);
    }
  };
  LmFrag<MT, NORM> buf[PF];
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    load(buf[j], wload, li);
    advance_load();
  }
  row_norms();
  for (int q0 = 0; q0 < total; q0 += PF) {
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      if (q0 + j < total) {
        compute(buf[j]);
        if (++ci == cnt) {
          finish_tile(ct);
          ci = 0;
          ct += gridDim.x;
        }
      }
      load(buf[j], wload, li);
      advance_load();
    }
  }
}

template <typename DT, int MT, bool NORM, int PF>
__global__ __launch_bounds__(kLmThreads) void lm_head_kernel(const LmHeadArgs a) {
  lm_head_body<DT, MT, NORM, PF, false>(a, 0.f);
}
// the cap rides BEHIND LmHeadArgs: lm_head_kernel keeps its argument block
template <typename DT, int MT, bool NORM, int PF>
__global__ __launch_bounds__(kLmThreads) void lm_head_softcap_kernel(const LmHeadArgs a, float cap) {
  lm_head_body<DT, MT, NORM, PF, true>(a, cap);
}

// out[i, :] = table[tokens[i], :] for 0 <= tokens[i] < v, zeros otherwise; one 16-byte granule per thread and turn
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* __restrict__ tokens, const u32x4* __restrict__ table, u32x4* __restrict__ out,
                                                           size_t total, int v, int kg) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t row = i / (size_t)kg, gi = i - row * (size_t)kg;
    const u32 tok = (u32)tokens[row];
    u32x4 val = {0u, 0u, 0u, 0u};
    if (tok < (u32)v) val = table[(size_t)tok * (size_t)kg + gi];  // (a negative id is a large unsigned one)
    out[i] = val;
  }
}

template <typename DT, int MT, int PF>
void lm_head_launch_mt(const LmHeadArgs& a, float cap, int blocks, hipStream_t st) {
  if (cap > 0.f) {
    if (a.gamma) hipLaunchKernelGGL((lm_head_softcap_kernel<DT, MT, true, PF>), dim3(blocks), dim3(kLmThreads), 0, st, a, cap);
    else hipLaunchKernelGGL((lm_head_softcap_kernel<DT, MT, false, PF>), dim3(blocks), dim3(kLmThreads), 0, st, a, cap);
  } else if (a.gamma) hipLaunchKernelGGL((lm_head_kernel<DT, MT, true, PF>), dim3(blocks), dim3(kLmThreads), 0, st, a);
  else hipLaunchKernelGGL((lm_head_kernel<DT, MT, false, PF>), dim3(blocks), dim3(kLmThreads), 0, st, a);
}

template <typename DT>
void lm_head_launch(const LmHeadArgs& a, float cap, int blocks, hipStream_t st) {
  switch ((a.m + 15) / 16) {
    case 1: lm_head_launch_mt<DT, 1, 4>(a, cap, blocks, st); break;
    case 2: lm_head_launch_mt<DT, 2, 2>(a, cap, blocks, st); break;
    case 3: lm_head_launch_mt<DT, 3, 2>(a, cap, blocks, st); break;
    default: lm_head_launch_mt<DT, 4, 2>(a, cap, blocks, st); break;
  }
}

}  // namespace

int lm_head_plan(int m, int v, int k, int out[4]) {
  if (m < 1 || m > 64 || v < 1 || k < 8 || (k % 8) != 0) return -1;
  const int tiles = (v + kLmTile - 1) / kLmTile, cap = kLmNumCU * kLmBlocksPerCU;
  const int rounds = (tiles + cap - 1) / cap;
  out[0] = (tiles + rounds - 1) / rounds;  // every block walks `rounds` tiles (the last ones one fewer)
  out[1] = kLmTile;
  out[2] = kLmWaves;
  out[3] = kLmWaves;  // the k split: one share per wave, in 64-k steps dealt round-robin
  return 0;
}

int launch_lm_head(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                   int out_f32, int m, int v, int k, int dtype, int max_blocks, hipStream_t st) {
  return launch_lm_head_softcap(x, ldx, gamma, eps, weight, bias, seqlens, out, out_f32, m, v, k, dtype, 0.f, max_blocks, st);
}

// softcap > 0: the capped epilogue; 0: launch_lm_head, the same kernels
int launch_lm_head_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* seqlens, void* out,
                           int out_f32, int m, int v, int k, int dtype, float softcap, int max_blocks, hipStream_t st) {
  int plan[4];
  if (lm_head_plan(m, v, k, plan) != 0 || ldx < k || (ldx % 8) != 0 || max_blocks < 0) return -1;
  const int blocks = max_blocks > 0 && max_blocks < plan[0] ? max_blocks : plan[0];
  const LmHeadArgs a = {(const uint16_t*)x, (const uint16_t*)gamma, (const uint16_t*)weight, (const uint16_t*)bias, seqlens, out, ldx, eps, m, v, k,
                        out_f32};
  if (dtype == 0) lm_head_launch<F16>(a, softcap, blocks, st);
  else lm_head_launch<BF16>(a, softcap, blocks, st);
  return 0;
}

int launch_embed_tokens(const int* tokens, const void* table, void* out, int n, int v, int k, hipStream_t st) {
  if (n < 1 || v < 1 || k < 8 || (k % 8) != 0) return -1;
  const size_t total = (size_t)n * (size_t)(k / 8);
  const unsigned blocks = (total + 255) / 256 > 4096u ? 4096u : (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(blocks), dim3(256), 0, st, tokens, (const u32x4*)table, (u32x4*)out, total, v, k / 8);
  return 0;
}

}  // namespace awq
