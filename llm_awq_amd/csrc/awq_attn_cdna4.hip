// Decode attention over the FasterTransformer KV cache (tinychat's awq_inference_engine.single_query_attention).
//
// One decode step of multi-head / grouped-query attention, restating the semantics of FT's masked multi-head attention
// (awq/kernels/csrc/attention/decoder_masked_multihead_attention_template.hpp, "MMHA" below):
//   cache layouts          k_cache [Bc, Hkv, Dh/8, Lmax, 8] (16-byte packs), v_cache [Bc, Hkv, Lmax, Dh]   (ft_attention.cpp:125-138)
//   current position       tlength = length_per_sample[b] if given, else timestep                       (MMHA :975-978)
//   circular cache         positions first_step = max(0, tlength + 1 - Lmax) .. tlength, index pos % Lmax (MMHA :979-980)
//   rotary embedding       q and the new k over the first rotary_dim dims, GPT-J interleaved (:1080-1086) or NeoX rotate-half
//                          (:1088-1130); angle = (t * rotary_scale) / pow(base, 2i / rotary_dim) in fp32
//                          (decoder_masked_multihead_attention_utils.h:1282-1287); the rotated q and k are rounded to T
//   scores                 q.k / sqrt(Dh), plus slope[h] * (t - tlength) with ALiBi (MMHA :1335-1345)
//   softmax                exp(s - max) / (sum + 1e-6)                                                   (MMHA :1399)
//   grouped query          query head h reads KV head h / (H / Hkv)                                       (MMHA :944-945)
//   side effect            the rotated k (as T) and v are written at cache index tlength % Lmax          (MMHA :1029, :1540)
//
// Deliberate deviations from FT:
//   1. The softmax weights and the P.V accumulation stay in fp32 (FT rounds the logits to T: MMHA_USE_FP32_ACUM_FOR_LOGITS is
//      off, MMHA :38-40), and q.k is accumulated in fp32 (v_dot2_f32_{f16,bf16}).
//   2. q, k and v each use their own batch stride.  FT applies q's stride to k and v (MMHA :967-969), which is wrong at batch > 1
//      whenever q, k and v are separate tensors (tinychat's GQA llama.py layout).
//
// Structure (flash-decoding):
//   * One block (256 threads, 4 waves) serves up to 8 query heads of ONE KV head, so K and V are read once per group.
//     Grid = (splits, Hkv * head_groups, B).
//   * The context is split over positions: split j covers [first_step + j * chunk, first_step + (j + 1) * chunk), the last split
//     everything up to tlength.  The host plan (attn_decode_plan) depends on host arguments only.  With one split the block writes
//     the T output; otherwise it writes fp32 (max, sum, o[Dh]) partials and attn_combine_kernel reduces them in split order.
//     No atomics, no flags between blocks: the result is bit-deterministic.
//   * Positions are walked in tiles of 256: thread i scores position t0 + i over the Dh/8 16-byte slices of the FT K layout (one
//     wave = 64 consecutive positions of one slice = 1 KiB, coalesced), the tile's scores go through LDS, an online softmax per
//     head rescales the running (max, sum), and the P.V product reads V rows 16 bytes per thread (Dh/8 threads per row).
//   * The current token's k and v come from the inputs (rotated in LDS); no block reads cache index tlength % Lmax.  Block
//     (split 0, head group 0) of each (b, KV head) writes them to the caches.
//   * Pipeline: VALU.  QK runs on v_dot2_f32 (two products per instruction), P.V on fp32 FMAs.  A 16-row MFMA would pad the
//     group of <= 8 query heads to 16 rows (half the matrix core idle) and needs the K tile transposed through LDS; the VALU form
//     was chosen for simplicity and is not the bound at G <= 8 (see DESIGN.md for the measured fraction).
#include "awq_device.hpp"
#include "awq_kernels.hpp"

#include <math.h>

namespace awq {
namespace {

constexpr int kThreads = 256;  // 4 waves
constexpr int kTile = 256;     // positions per tile (one per thread in the score step)
constexpr int kMaxDh = 256;
constexpr int kMaxGroup = 8;   // query heads per block

struct AttnArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* k_cache;
  uint16_t* v_cache;
  const int* lens;
  const float* alibi;
  uint16_t* out;
  float* ws;
  int H, Hkv, Dh, Lmax, G, ngrp;
  long long q_bs, k_bs, v_bs;  // batch strides (elements)
  int timestep, rot, neox, splits, chunk;
  float rot_base, rot_scale, inv_sqrt_dh;
};

__device__ __forceinline__ float dot2(u32 a, u32 b, float c, F16) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c, false);
}
__device__ __forceinline__ float dot2(u32 a, u32 b, float c, BF16) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) x = fmaxf(x, __shfl_xor(x, d, 64));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__device__ __forceinline__ int current_length(const AttnArgs& a, int b) {
  const int t = a.lens ? a.lens[b] : a.timestep;
  return t < 0 ? 0 : t;  // (a negative device length is treated as position 0: no cache index outside [0, Lmax) is formed)
}

// Rotary embedding of one row `x` (T, Dh values, in LDS) in place at position t (MMHA :1080-1130, utils.h:1282-1297).
template <typename DT>
__device__ void rotate_row(uint16_t* x, int rot, int neox, int t, float base, float scale, int tid, int nthr) {
  const int half = rot >> 1;
  for (int i = tid; i < half; i += nthr) {
    const int i0 = neox ? i : 2 * i, i1 = neox ? i + half : 2 * i + 1;
    const float ang = ((float)t * scale) / powf(base, (float)(2 * i) / (float)rot);
    const float c = cosf(ang), s = sinf(ang);
    const float x0 = DT::to_float(x[i0]), x1 = DT::to_float(x[i1]);
    x[i0] = DT::from_float(c * x0 - s * x1);
    x[i1] = DT::from_float(c * x1 + s * x0);
  }
}

template <typename DT, int GM>
__global__ __launch_bounds__(kThreads) void attn_decode_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t q_s[GM][kMaxDh];   // rotated q, T
  __shared__ __attribute__((aligned(16))) uint16_t kn_s[kMaxDh];      // rotated new k, T
  __shared__ __attribute__((aligned(16))) uint16_t vn_s[kMaxDh];      // new v, T
  __shared__ __attribute__((aligned(16))) float p_s[GM][kTile];       // scores, then softmax weights of the tile
  __shared__ __attribute__((aligned(16))) float red_s[kThreads * 8];  // cross position-group reduction of o
  __shared__ float alpha_s[GM], m_s[GM], l_s[GM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x, b = blockIdx.z;
  const int kvh = blockIdx.y / a.ngrp, grp = blockIdx.y - kvh * a.ngrp;
  const int h0 = kvh * a.G + grp * GM;                       // first query head of this block
  const int gcnt = min(GM, a.G - grp * GM);                   // query heads served (<= GM)
  const int Dh = a.Dh, Lmax = a.Lmax, nslice = Dh >> 3;

  const int tlength = current_length(a, b);
  const int first_step = max(0, tlength + 1 - Lmax);
  const int p_begin = first_step + split * a.chunk;
  const int p_end = (split == a.splits - 1) ? tlength + 1 : min(tlength + 1, p_begin + a.chunk);
  const int t_idx = tlength % Lmax;

  // ---- q, k, v of the current token -> LDS (16 bytes per thread), rotary in place ----
  {
    const uint16_t* qb = a.q + (long long)b * a.q_bs + (long long)h0 * Dh;
    for (int i = tid; i < gcnt * nslice; i += kThreads) {
      const int h = i / nslice, s = i - h * nslice;
      *reinterpret_cast<u32x4*>(&q_s[h][s * 8]) = *reinterpret_cast<const u32x4*>(qb + (long long)h * Dh + s * 8);
    }
    for (int i = tid; i < (GM - gcnt) * nslice; i += kThreads) {  // unused head rows of the group: zeros (their results are dropped)
      const int h = gcnt + i / nslice, s = i % nslice;
      *reinterpret_cast<u32x4*>(&q_s[h][s * 8]) = u32x4{0, 0, 0, 0};
    }
    if (tid < nslice) {
      *reinterpret_cast<u32x4*>(&kn_s[tid * 8]) = *reinterpret_cast<const u32x4*>(a.k + (long long)b * a.k_bs + (long long)kvh * Dh + tid * 8);
    } else if (tid >= 128 && tid - 128 < nslice) {
      const int s = tid - 128;
      *reinterpret_cast<u32x4*>(&vn_s[s * 8]) = *reinterpret_cast<const u32x4*>(a.v + (long long)b * a.v_bs + (long long)kvh * Dh + s * 8);
    }
    __syncthreads();
    if (a.rot > 0) {
      // one wave per row: the q rows of the group, then k (wave (gcnt % 4) handles it)
      for (int r = wave; r <= gcnt; r += 4) {
        uint16_t* row = (r < gcnt) ? &q_s[r][0] : kn_s;
        rotate_row<DT>(row, a.rot, a.neox, tlength, a.rot_base, a.rot_scale, lane, 64);
      }
      __syncthreads();
    }
  }

  // ---- cache write of the current token (one block per (b, KV head)) ----
  if (split == 0 && grp == 0) {
    const size_t bh = (size_t)b * a.Hkv + kvh;
    if (tid < nslice) {
      uint16_t* kc = a.k_cache + ((bh * nslice + tid) * (size_t)Lmax + t_idx) * 8;
      *reinterpret_cast<u32x4*>(kc) = *reinterpret_cast<const u32x4*>(&kn_s[tid * 8]);
    } else if (tid >= 128 && tid - 128 < nslice) {
      const int s = tid - 128;
      uint16_t* vc = a.v_cache + (bh * Lmax + t_idx) * (size_t)Dh + s * 8;
      *reinterpret_cast<u32x4*>(vc) = *reinterpret_cast<const u32x4*>(&vn_s[s * 8]);
    }
  }

  const uint16_t* kcb = a.k_cache + ((size_t)b * a.Hkv + kvh) * (size_t)nslice * Lmax * 8;
  const uint16_t* vcb = a.v_cache + ((size_t)b * a.Hkv + kvh) * (size_t)Lmax * Dh;
  float slope[GM];
#pragma unroll
  for (int h = 0; h < GM; ++h) slope[h] = (a.alibi && h < gcnt) ? a.alibi[h0 + h] : 0.f;

  // P.V thread layout: TPR threads per V row (16 bytes each), PG position groups
  const int TPR = nslice, PG = kThreads / TPR;
  const int pv_c = tid % TPR, pv_g = tid / TPR;
  const bool pv_on = pv_g < PG;
  float acc[GM][8];
#pragma unroll
  for (int h = 0; h < GM; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[h][e] = 0.f;
  // online-softmax state of heads wave and wave + 4 (kept by every lane of the owning wave)
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};

  for (int t0 = p_begin; t0 < p_end; t0 += kTile) {
    const int tn = min(kTile, p_end - t0);
    // -- scores: thread tid <-> position t0 + tid --
    {
      const int pos = t0 + tid;
      float sc[GM];
#pragma unroll
      for (int h = 0; h < GM; ++h) sc[h] = 0.f;
      if (tid < tn) {
        const bool cur = pos == tlength;
        const int idx = pos % Lmax;
        const uint16_t* kp = kcb + (size_t)idx * 8;
        // 8 slices (128 bytes per thread) in flight per batch; nslice is even
        for (int s0 = 0; s0 < nslice; s0 += 8) {
          u32x4 kk[8];
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (s0 + u < nslice)
              kk[u] = cur ? *reinterpret_cast<const u32x4*>(&kn_s[(s0 + u) * 8])
                          : __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kp + (size_t)(s0 + u) * Lmax * 8));
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (s0 + u < nslice) {
#pragma unroll
              for (int h = 0; h < GM; ++h) {
                const u32x4 qq = *reinterpret_cast<const u32x4*>(&q_s[h][(s0 + u) * 8]);
                float d = sc[h];
                d = dot2(qq.x, kk[u].x, d, DT{});
                d = dot2(qq.y, kk[u].y, d, DT{});
                d = dot2(qq.z, kk[u].z, d, DT{});
                d = dot2(qq.w, kk[u].w, d, DT{});
                sc[h] = d;
              }
            }
          }
        }
        const float dist = (float)(pos - tlength);
#pragma unroll
        for (int h = 0; h < GM; ++h) {
          sc[h] *= a.inv_sqrt_dh;
          if (a.alibi) sc[h] += slope[h] * dist;
        }
      } else {
#pragma unroll
        for (int h = 0; h < GM; ++h) sc[h] = -INFINITY;
      }
#pragma unroll
      for (int h = 0; h < GM; ++h) p_s[h][tid] = sc[h];
    }
    __syncthreads();
    // -- online softmax: wave w owns heads w and w + 4 --
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int h = wave + 4 * r;
      if (h < GM) {
        float s4[4], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s4[j] = p_s[h][lane + 64 * j];
          mx = fmaxf(mx, s4[j]);
        }
        mx = wave_max(mx);
        const float m_new = fmaxf(m_run[r], mx);  // finite: the tile holds at least one position
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = __expf(s4[j] - m_new);  // exp(-inf) = 0 for the positions past the range
          p_s[h][lane + 64 * j] = p;
          sum += p;
        }
        sum = wave_sum(sum);
        const float alpha = __expf(m_run[r] - m_new);  // 0 on the first tile
        l_run[r] = l_run[r] * alpha + sum;
        m_run[r] = m_new;
        if (lane == 0) alpha_s[h] = alpha;
      }
    }
    __syncthreads();
    // -- P.V: thread (pv_g, pv_c) accumulates dims 8 pv_c .. 8 pv_c + 7 over positions pv_g, pv_g + PG, .. of the tile --
    if (pv_on) {
#pragma unroll
      for (int h = 0; h < GM; ++h) {
        const float al = alpha_s[h];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[h][e] *= al;
      }
      // 4 V rows in flight per batch
      for (int j0 = pv_g; j0 < tn; j0 += 4 * PG) {
        u32x4 vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * PG, pos = t0 + j;
          if (j < tn)
            vv[u] = (pos == tlength) ? *reinterpret_cast<const u32x4*>(&vn_s[pv_c * 8])
                                     : __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vcb + (size_t)(pos % Lmax) * Dh + pv_c * 8));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * PG;
          if (j < tn) {
            const u32 w4[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
            float vf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              vf[2 * e] = DT::to_float((uint16_t)(w4[e] & 0xFFFFu));
              vf[2 * e + 1] = DT::to_float((uint16_t)(w4[e] >> 16));
            }
#pragma unroll
            for (int h = 0; h < GM; ++h) {
              const float p = p_s[h][j];
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[h][e] = __builtin_fmaf(p, vf[e], acc[h][e]);
            }
          }
        }
      }
    }
    __syncthreads();  // p_s / alpha_s are rewritten by the next tile
  }

  // ---- softmax state -> LDS ----
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int h = wave + 4 * r;
    if (h < GM && lane == 0) {
      m_s[h] = m_run[r];
      l_s[h] = l_run[r];
    }
  }
  // ---- reduce o over the position groups (fixed order), one head at a time ----
  const bool single = a.splits == 1;
#pragma unroll
  for (int h = 0; h < GM; ++h) {
    if (h >= gcnt) break;  // (static register index h: acc stays in VGPRs)
#pragma unroll
    for (int e = 0; e < 8; ++e) red_s[tid * 8 + e] = pv_on ? acc[h][e] : 0.f;
    __syncthreads();
    if (tid < Dh) {
      const int c = tid >> 3, e = tid & 7;
      float o = 0.f;
      for (int g = 0; g < PG; ++g) o += red_s[(g * TPR + c) * 8 + e];
      const int hq = h0 + h;
      if (single) {
        const float inv = 1.f / (l_s[h] + 1e-6f);  // MMHA :1399
        a.out[((size_t)b * a.H + hq) * Dh + tid] = DT::from_float(o * inv);
      } else {
        float* rec = a.ws + (((size_t)b * a.H + hq) * a.splits + split) * (size_t)(Dh + 4);
        if (tid == 0) {
          rec[0] = m_s[h];
          rec[1] = l_s[h];
        }
        rec[4 + tid] = o;
      }
    }
    __syncthreads();
  }
}

// Reduce the split partials of one (b, query head): fixed split order, one thread per output dim.  The (max, sum) pairs go through
// LDS (thread j loads split j's), and the o loads are unrolled by 8: a partial sits in L2, and one dependent load per split
// would make the launch latency-bound.
template <typename DT>
__global__ __launch_bounds__(kMaxDh) void attn_combine_kernel(const float* __restrict__ ws, uint16_t* __restrict__ out, int H, int Dh, int splits) {
  __shared__ float m_s[kMaxDh], w_s[kMaxDh];  // splits <= 256 (attn_decode_plan)
  const int hq = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const size_t rs = (size_t)(Dh + 4);
  const float* rec = ws + ((size_t)b * H + hq) * splits * rs;
  float lj = 0.f;
  if (d < splits) {
    m_s[d] = rec[(size_t)d * rs];
    lj = rec[(size_t)d * rs + 1];
  }
  __syncthreads();
  float M = -INFINITY;
  for (int j = 0; j < splits; ++j) M = fmaxf(M, m_s[j]);
  if (d < splits) w_s[d] = __expf(m_s[d] - M);  // an empty split (m = -inf, l = 0, o = 0) weighs 0
  __syncthreads();
  if (d < splits) m_s[d] = lj * w_s[d];
  __syncthreads();
  if (d >= Dh) return;
  float L = 0.f, O = 0.f;
  for (int j = 0; j < splits; ++j) L += m_s[j];
#pragma unroll 8
  for (int j = 0; j < splits; ++j) O = __builtin_fmaf(rec[(size_t)j * rs + 4 + d], w_s[j], O);
  out[((size_t)b * H + hq) * Dh + d] = DT::from_float(O * (1.f / (L + 1e-6f)));  // MMHA :1399
}

template <typename DT>
void launch_dt(const AttnArgs& a, int gm, dim3 grid, hipStream_t st) {
  switch (gm) {
    case 1: hipLaunchKernelGGL((attn_decode_kernel<DT, 1>), grid, dim3(kThreads), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attn_decode_kernel<DT, 2>), grid, dim3(kThreads), 0, st, a); break;
    case 4: hipLaunchKernelGGL((attn_decode_kernel<DT, 4>), grid, dim3(kThreads), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_decode_kernel<DT, 8>), grid, dim3(kThreads), 0, st, a); break;
  }
  if (a.splits > 1)
    hipLaunchKernelGGL((attn_combine_kernel<DT>), dim3(a.H, grid.z), dim3(kMaxDh), 0, st, (const float*)a.ws, a.out, a.H, a.Dh, a.splits);
}

}  // namespace

// Host plan: splits over the context so that B * Hkv * splits reaches the CU count (256), in chunks of whole 256-position tiles.
//   one split when B * Hkv already fills the chip or the context fits in one tile.
int attn_decode_plan(int batch, int nheads_kv, int head_dim, int timestep, int lmax, int* splits, int* chunk) {
  (void)head_dim;
  const int n = min(timestep + 1, lmax);  // positions attended at the host-side upper bound
  const int base = batch * nheads_kv;
  constexpr int kCUs = 256;
  int s = 1;
  if (base < kCUs && n > kTile) {
    const int want = (kCUs + base - 1) / base;
    const int most = (n + kTile - 1) / kTile;  // at least one full tile per split
    s = min(want, most);
  }
  int c = (n + s - 1) / s;
  c = (c + kTile - 1) / kTile * kTile;
  s = (n + c - 1) / c;  // (rounding the chunk up may leave the last split empty: drop it)
  *splits = s;
  *chunk = c;
  return 0;
}

size_t attn_decode_workspace_bytes(int batch, int nheads, int nheads_kv, int head_dim, int timestep, int lmax) {
  int s = 1, c = 0;
  attn_decode_plan(batch, nheads_kv, head_dim, timestep, lmax, &s, &c);
  return s > 1 ? (size_t)batch * nheads * s * (size_t)(head_dim + 4) * sizeof(float) : 0;
}

int launch_attn_decode(const void* q, const void* k, const void* v, void* k_cache, void* v_cache, const int* lens, const float* alibi,
                       void* out, int B, int H, int Hkv, int Dh, int Lmax, long long q_bs, long long k_bs, long long v_bs, int timestep,
                       int rot, float rot_base, float rot_scale, int neox, int dtype, void* workspace, hipStream_t st) {
  AttnArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k;
  a.v = (const uint16_t*)v;
  a.k_cache = (uint16_t*)k_cache;
  a.v_cache = (uint16_t*)v_cache;
  a.lens = lens;
  a.alibi = alibi;
  a.out = (uint16_t*)out;
  a.ws = (float*)workspace;
  a.H = H;
  a.Hkv = Hkv;
  a.Dh = Dh;
  a.Lmax = Lmax;
  a.G = H / Hkv;
  const int gm = a.G <= 1 ? 1 : a.G <= 2 ? 2 : a.G <= 4 ? 4 : kMaxGroup;
  a.ngrp = (a.G + gm - 1) / gm;
  a.q_bs = q_bs;
  a.k_bs = k_bs;
  a.v_bs = v_bs;
  a.timestep = timestep;
  a.rot = rot;
  a.neox = neox;
  a.rot_base = rot_base;
  a.rot_scale = rot_scale;
  a.inv_sqrt_dh = 1.f / sqrtf((float)Dh);
  attn_decode_plan(B, Hkv, Dh, timestep, Lmax, &a.splits, &a.chunk);
  const dim3 grid(a.splits, Hkv * a.ngrp, B);
  if (dtype == 0) launch_dt<F16>(a, gm, grid, st);
  else launch_dt<BF16>(a, gm, grid, st);
  return 0;
}

}  // namespace awq
