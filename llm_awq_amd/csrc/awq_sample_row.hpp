// The sampler's row routine (gfx950, wave64), shared by the kernels that sample a row of logits: sample_kernel (awq_sample_cdna4.hip, one row per
// slot) and spec_verify_kernel (awq_spec_cdna4.hip, one row per packed token of a speculative step).  Both run THIS text on a block of 1024
// threads, so the same logits bits, parameters and uniform give the same token whichever kernel asks (DESIGN.md "Sampling", steps 1 to 8).
//
// A row (up to 2^20 logits) does not fit LDS, so the block walks it several times out of L2; how often is decided per row from the row's own
// parameters, so a mixed batch is one launch:
//   max pass      x_v = penalty(temperature(logit_v)), the largest key and its lowest index            (greedy rows stop here: 1 pass)
//   select passes 8-bit radix select over the monotone float key, most significant digit first: per bin a count and a mass, summed over the
//                 keys that share the digits chosen so far -> tau, the smallest kept key; top-k and top-p come out of the same four passes
//                 (rows with neither filter, and top-k 1, skip them)
//   sum pass      the kept mass of every 512-logit tile, in index order
//   find          one wave rescans the tile that holds u * Zk
// Masses are fixed-point integers, trunc(expf(x_v - max) * 2^40) in 64 bits (V <= 2^20: every sum is below 2^61), so every histogram, prefix and
// total is an integer sum whose value does not depend on the order of its terms: a launch is bit-stable from run to run although the
// histogram is built with LDS atomics.  (A token below 2^-40 of the top probability has mass 0 and is never drawn.)  No global atomics, no
// workspace, no global store: the token comes back in a register of every thread.
#pragma once
#include "awq_device.hpp"

namespace awq {
namespace sample_row {

using u64 = unsigned long long;
constexpr int kSampleThreads = 1024, kSampleWaves = kSampleThreads / 64;
constexpr int kUnroll = 4;                        // chunks whose loads are in flight together, per thread
constexpr int kHistCopies = 8;                    // lanes l and l + 8 share a copy: an 8-way instead of a 64-way pile-up on a popular bin
constexpr int kMaxTiles = ((1 << 20) + 8) / 512 + 2;  // 512-logit tiles of the longest row, counted from the 16-/32-byte boundary below its start

// monotone float -> unsigned key (awq_moe_route_cdna4.hip), with -0 folded onto +0 so that keys compare exactly as the values do
__device__ __forceinline__ u32 sample_key(float f) {
  const u32 b = __builtin_bit_cast(u32, f == 0.0f ? 0.0f : f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float sample_key_float(u32 k) { return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  return ((u64)(u32)__shfl((int)(v >> 32), src) << 32) | (u32)__shfl((int)(u32)v, src);
}
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int d) {
  return ((u64)(u32)__shfl_down((int)(v >> 32), d) << 32) | (u32)__shfl_down((int)(u32)v, d);
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
  return ((u64)(u32)__shfl_up((int)(v >> 32), d) << 32) | (u32)__shfl_up((int)(u32)v, d);
}
// sum over the lanes >= this one (lane 0 holds the wave's total) / over the lanes <= this one (lane 63 holds it)
__device__ __forceinline__ u64 wave_suffix_sum(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 t = shfl_down_u64(v, d);
    if (lane + d < 64) v += t;
  }
  return v;
}
__device__ __forceinline__ u64 wave_prefix_sum(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 t = shfl_up_u64(v, d);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 t = shfl_down_u64(v, d);
    v = t > v ? t : v;
  }
  return v;  // (lane 0)
}

// trunc(exp(x - max) * 2^40); 0 for -inf, for a NaN and for a row whose max is infinite or NaN (x - max is then NaN or -inf)
__device__ __forceinline__ u64 mass_of(float x, float mx) {
  const float e = expf(x - mx);
  return (e > 0.0f && e <= 1.0f) ? (u64)(e * 0x1p40f) : 0ull;
}

// the row as 8-logit chunks counted from the 16-byte (fp32: 32-byte) boundary at or below its first logit: chunk c holds the row indices
// 8 c - a0 .. 8 c - a0 + 7.  A chunk inside the row is one (fp32: two) 16-byte load(s); the first and the last chunk of a row whose ends are
// not on a boundary read their logits one by one, so nothing outside the row is touched.
template <int LT>
struct RowView {
  const char* base;  // address of chunk 0 (may lie below the row; never dereferenced outside [row, row + V))
  int a0, V;
  float t, r;
  bool div_t, pen;
  const u32* bitmap;

  // what a chunk's loads return: issued for several chunks before the first one is used, so that a pass is not one memory latency per chunk
  struct Raw {
    u32x4 lo, hi;  // (hi: fp32 only)
    u32 valid;     // bit i: logit i of the chunk is inside the row
  };
  __device__ __forceinline__ Raw fetch(int c, int nchunks) const {
    constexpr int ES = LT == 2 ? 4 : 2;
    Raw w;
    w.lo = u32x4{0u, 0u, 0u, 0u};
    w.hi = u32x4{0u, 0u, 0u, 0u};
    w.valid = 0u;
    if (c >= nchunks) return w;
    const int v0 = c * 8 - a0;
    if (v0 >= 0 && v0 + 8 <= V) {
      w.valid = 0xFFu;
      if constexpr (LT == 2) {
        w.lo = *reinterpret_cast<const u32x4*>(base + (size_t)c * 32);
        w.hi = *reinterpret_cast<const u32x4*>(base + (size_t)c * 32 + 16);
      } else {
        w.lo = *reinterpret_cast<const u32x4*>(base + (size_t)c * 16);
      }
    } else {
      u32 e[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int v = v0 + i;
        e[i] = 0u;
        if (v >= 0 && v < V) {
          w.valid |= 1u << i;
          const char* p = base + ((size_t)c * 8 + i) * ES;
          if constexpr (LT == 2) e[i] = *reinterpret_cast<const u32*>(p);
          else e[i] = *reinterpret_cast<const uint16_t*>(p);
        }
      }
      if constexpr (LT == 2) {
        w.lo = u32x4{e[0], e[1], e[2], e[3]};
        w.hi = u32x4{e[4], e[5], e[6], e[7]};
      } else {
        w.lo = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
      }
    }
    return w;
  }
  // the chunk's eight x_v: the dtype's value, then the temperature, then the penalty
  __device__ __forceinline__ void decode(const Raw& w, int c, float (&x)[8]) const {
    const int v0 = c * 8 - a0;
    const u32 valid = w.valid;
    const u32 ws[8] = {w.lo.x, w.lo.y, w.lo.z, w.lo.w, w.hi.x, w.hi.y, w.hi.z, w.hi.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if constexpr (LT == 2) {
        x[i] = __builtin_bit_cast(float, ws[i]);
      } else {
        const uint16_t h = (uint16_t)((i & 1) ? (ws[i >> 1] >> 16) : (ws[i >> 1] & 0xFFFFu));
        x[i] = LT == 1 ? BF16::to_float(h) : F16::to_float(h);
      }
    }
    if (div_t) {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = x[i] / t;  // IEEE division (no reciprocal): the contract is bit-equal to np.float32 division
    }
    if (pen) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int v = v0 + i;
        if (((valid >> i) & 1u) && ((bitmap[v >> 5] >> (v & 31)) & 1u)) x[i] = x[i] < 0.0f ? x[i] * r : x[i] / r;
      }
    }
  }
};

// row `index` of logits [rows, V] under temperature t and penalty r; pen: the bitmap holds the penalty set (and r > 1)
template <int LT>
__device__ __forceinline__ RowView<LT> make_row_view(const void* logits, size_t index, int V, float t, float r, bool pen, const u32* bitmap) {
  constexpr int ES = LT == 2 ? 4 : 2;
  RowView<LT> row;
  const char* rowp = reinterpret_cast<const char*>(logits) + index * V * ES;
  row.a0 = (int)((reinterpret_cast<uintptr_t>(rowp) & (LT == 2 ? 31u : 15u)) / ES);
  row.base = rowp - (size_t)row.a0 * ES;
  row.V = V;
  row.t = t;
  row.r = r;
  row.div_t = t >= 1e-5f && t != 1.0f;
  row.pen = pen;
  row.bitmap = bitmap;
  return row;
}

// (block-wide, under a block-uniform condition) the presence bitmap of the penalty set, V bits: the n ids at h and the n_extra ids at extra.
// OR is order-free; ids outside [0, V) are ignored.
__device__ __forceinline__ void build_bitmap(u32* bm, int V, const int* h, int n, const int* extra, int n_extra) {
  const int tid = threadIdx.x;
  for (int i = tid; i < (V + 31) / 32; i += kSampleThreads) bm[i] = 0u;
  __syncthreads();
  for (int i = tid; i < n; i += kSampleThreads) {
    const int id = h[i];
    if (id >= 0 && id < V) atomicOr(&bm[id >> 5], 1u << (id & 31));
  }
  for (int i = tid; i < n_extra; i += kSampleThreads) {
    const int id = extra[i];
    if (id >= 0 && id < V) atomicOr(&bm[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
}

// Steps 3 to 8 on one row by the whole block (every thread of the 1024 calls it, under block-uniform conditions only): -> the token, in every
// thread.  p, k: the row's top-p and top-k; u_row: the address of the row's uniform, read by one wave once the kept mass is known.
template <int LT>
__device__ __forceinline__ int sample_row_token(const RowView<LT>& row, float p, int k, const float* u_row) {
  // the select passes' histograms, then (they are done by then) the sum pass's tile sums
  __shared__ __attribute__((aligned(16))) u64 s_buf[kHistCopies * 256 + kHistCopies * 128];
  __shared__ u64 s_red[kSampleWaves];
  __shared__ u64 s_sel[6];  // prefix, mass above, count above, found | tile, base prefix, target
  __shared__ int s_token;
  u64* const h_mass = s_buf;                                           // [copies][256]
  u32* const h_cnt = reinterpret_cast<u32*>(s_buf + kHistCopies * 256);  // [copies][256]
  u64* const tile_sum = s_buf;                                         // [tiles]
  static_assert(kMaxTiles <= kHistCopies * 384, "tile sums must fit the histogram storage");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = row.V;
  const bool greedy = row.t < 1e-5f || p < 1e-8f;
  const bool use_p = p >= 1e-8f && p < 1.0f, use_k = k > 0 && k < V;
  const int nchunks = (row.a0 + V + 7) / 8, ntiles = (nchunks + 63) / 64;

  // ---- max pass: the largest key and, among its holders, the lowest index: max over (key << 32 | ~index) ----
  u64 best = 0ull;
  for (int c = tid; c < nchunks; c += kUnroll * kSampleThreads) {
    typename RowView<LT>::Raw w[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) w[j] = row.fetch(c + j * kSampleThreads, nchunks);
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int cj = c + j * kSampleThreads;
      float x[8];
      row.decode(w[j], cj, x);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const u64 cand = ((u64)sample_key(x[i]) << 32) | (u64)(0xFFFFFFFFu - (u32)(cj * 8 - row.a0 + i));
        if (((w[j].valid >> i) & 1u) && cand > best) best = cand;
      }
    }
  }
  best = wave_max(best);
  if (lane == 0) s_red[wave] = best;
  __syncthreads();
  best = s_red[0];
#pragma unroll
  for (int w = 1; w < kSampleWaves; ++w) best = s_red[w] > best ? s_red[w] : best;
  const u32 maxkey = (u32)(best >> 32);
  const float mx = sample_key_float(maxkey);
  int amax = (int)(0xFFFFFFFFu - (u32)best);
  amax = amax < 0 ? 0 : (amax >= V ? V - 1 : amax);
  if (tid == 0) s_token = amax;  // the greedy token, and the answer of a row without mass (NaN, +inf, all -inf)

  if (!greedy) {  // (block-uniform from here on: every condition around a barrier comes from the row's parameters or from LDS)
    u32 tau = 0u;  // smallest kept key; 0 keeps everything
    bool have_mass = true;
    if (use_k && k == 1) tau = maxkey;  // the top tie group, whatever top-p says: the maxima always pass it
    else if (use_p || use_k) {
      for (int i = tid; i < kHistCopies * 256; i += kSampleThreads) {
        h_mass[i] = 0ull;
        h_cnt[i] = 0u;
      }
      if (tid == 0) {
        s_sel[0] = 0ull;
        s_sel[1] = 0ull;
        s_sel[2] = 0ull;
        s_sel[3] = 1ull;
      }
      __syncthreads();
      const int copy = lane & (kHistCopies - 1);
      u64 pz = ~0ull;  // keep while (mass above) < pz: the integer form of S(x_v) < p (set and used by wave 0 alone)
      for (int shift = 24; shift >= 0; shift -= 8) {
        const u32 himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8)), prefix = (u32)s_sel[0];
        for (int c = tid; c < nchunks; c += kUnroll * kSampleThreads) {
          typename RowView<LT>::Raw w[kUnroll];
#pragma unroll
          for (int j = 0; j < kUnroll; ++j) w[j] = row.fetch(c + j * kSampleThreads, nchunks);
#pragma unroll
          for (int j = 0; j < kUnroll; ++j) {
            float x[8];
            row.decode(w[j], c + j * kSampleThreads, x);
            const u32 valid = w[j].valid;
            int cur = -1;  // runs of equal bins inside the chunk go out as one atomic
            u32 ccnt = 0u;
            u64 cmass = 0ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const u32 key = sample_key(x[i]);
              if (((valid >> i) & 1u) && (key & himask) == prefix) {
                const int bin = (int)((key >> shift) & 255u);
                if (bin != cur && cur >= 0) {
                  atomicAdd(&h_cnt[copy * 256 + cur], ccnt);
                  if (use_p) atomicAdd(&h_mass[copy * 256 + cur], cmass);
                  ccnt = 0u;
                  cmass = 0ull;
                }
                cur = bin;
                ccnt += 1u;
                if (use_p) cmass += mass_of(x[i], mx);
              }
            }
            if (cur >= 0) {
              atomicAdd(&h_cnt[copy * 256 + cur], ccnt);
              if (use_p) atomicAdd(&h_mass[copy * 256 + cur], cmass);
            }
          }
        }
        __syncthreads();
        if (wave == 0) {  // lane l owns bins 4 l .. 4 l + 3: sums the copies, clears them for the next pass
          u64 m[4], ms = 0ull;
          u32 n[4], ns = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            m[j] = 0ull;
            n[j] = 0u;
            for (int cp = 0; cp < kHistCopies; ++cp) {
              const int at = cp * 256 + lane * 4 + j;
              m[j] += h_mass[at];
              n[j] += h_cnt[at];
              h_mass[at] = 0ull;
              h_cnt[at] = 0u;
            }
            ms += m[j];
            ns += n[j];
          }
          const u64 msuf = wave_suffix_sum(ms, lane), nsuf = wave_suffix_sum((u64)ns, lane);
          if (shift == 24 && use_p) {  // Z = every mass of the row; G < p Z  <=>  G < ceil(p Z) for an integer G
            const u64 Z = shfl_u64(msuf, 0);
            const double pzd = ceil((double)p * (double)Z);
            pz = pzd < 1.8e19 ? (u64)pzd : ~0ull;
          }
          const u64 kk = use_k ? (u64)k : ~0ull;
          u64 G = s_sel[1] + (msuf - ms), N = s_sel[2] + (nsuf - (u64)ns);  // above this lane's highest bin
          int cand = 256;
          u64 cG = 0ull, cN = 0ull;
#pragma unroll
          for (int j = 3; j >= 0; --j) {  // downwards: the lowest non-empty bin whose largest key is still kept holds tau
            if (n[j] != 0u && G < pz && N < kk) {
              cand = lane * 4 + j;
              cG = G;
              cN = N;
            }
            G += m[j];
            N += (u64)n[j];
          }
          const u64 has = __ballot(cand < 256);
          const int src = has ? __ffsll((long long)has) - 1 : 0;
          cand = __shfl(cand, src);
          cG = shfl_u64(cG, src);
          cN = shfl_u64(cN, src);
          if (lane == 0) {
            if (has) {
              s_sel[0] = (u64)(prefix | ((u32)cand << shift));
              s_sel[1] = cG;
              s_sel[2] = cN;
            } else {
              s_sel[3] = 0ull;  // a row without mass: no bin is kept
            }
          }
        }
        __syncthreads();
      }
      tau = (u32)s_sel[0];
      have_mass = s_sel[3] != 0ull;
      __syncthreads();  // the histogram storage turns into the tile sums
    }

    if (have_mass) {
      // ---- sum pass: tile j = chunks 64 j .. 64 j + 63 = wave j % 16 in round j / 16; its kept mass, in index order ----
      for (int c0 = wave * 64; c0 < nchunks; c0 += kUnroll * kSampleThreads) {
        typename RowView<LT>::Raw w[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) w[j] = row.fetch(c0 + j * kSampleThreads + lane, nchunks);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
          const int cj = c0 + j * kSampleThreads;  // (wave-uniform)
          float x[8];
          row.decode(w[j], cj + lane, x);
          u64 s = 0ull;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (((w[j].valid >> i) & 1u) && sample_key(x[i]) >= tau) s += mass_of(x[i], mx);
          s = wave_suffix_sum(s, lane);
          if (lane == 0 && cj < nchunks) tile_sum[cj >> 6] = s;
        }
      }
      __syncthreads();
      if (wave == 0) {  // lane l owns a run of consecutive tiles; the run that holds the target is walked by its lane
        const int per = (ntiles + 63) / 64, j0 = lane * per, j1 = j0 + per < ntiles ? j0 + per : ntiles;
        u64 run = 0ull;
        for (int j = j0; j < j1; ++j) run += tile_sum[j];
        const u64 incl = wave_prefix_sum(run, lane), Zk = shfl_u64(incl, 63), excl = incl - run;
        // the first kept v with C_v > u Zk  <=>  C_v > floor(u Zk) for an integer C_v; the target stays below Zk, so such a v exists
        const double td = (double)*u_row * (double)Zk;
        u64 T = td >= 0.0 ? (td < (double)Zk ? (u64)td : Zk) : 0ull;
        if (Zk != 0ull && T >= Zk) T = Zk - 1ull;
        const bool mine = Zk != 0ull && excl <= T && T < incl;
        int tj = 0;
        u64 tb = 0ull;
        if (mine) {
          u64 acc = excl;
          for (int j = j0; j < j1; ++j) {
            const u64 nx = acc + tile_sum[j];
            if (T < nx) {
              tj = j;
              tb = acc;
              break;
            }
            acc = nx;
          }
        }
        const u64 has = __ballot(mine);
        const int src = has ? __ffsll((long long)has) - 1 : 0;
        tj = __shfl(tj, src);
        tb = shfl_u64(tb, src);
        if (lane == 0) {
          s_sel[3] = has ? (1ull << 32) | (u64)(u32)tj : 0ull;
          s_sel[4] = tb;
          s_sel[5] = T;
        }
      }
      __syncthreads();
      // ---- find: the wave that summed the target's tile scans it again; one lane holds the crossing and walks its eight logits ----
      const u64 found = s_sel[3];
      const int tj = (int)(u32)found;
      if ((found >> 32) != 0ull && wave == (tj & (kSampleWaves - 1))) {
        const int c = tj * 64 + lane;
        const u64 T = s_sel[5];
        float x[8];
        u64 q[8], s = 0ull;
        const typename RowView<LT>::Raw w = row.fetch(c, nchunks);
        const u32 valid = w.valid;
        row.decode(w, c, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          q[i] = (((valid >> i) & 1u) && sample_key(x[i]) >= tau) ? mass_of(x[i], mx) : 0ull;
          s += q[i];
        }
        const u64 incl = s_sel[4] + wave_prefix_sum(s, lane);
        u64 acc = incl - s;
        if (acc <= T && T < incl) {
          int tok = -1;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            acc += q[i];
            if (tok < 0 && T < acc) tok = c * 8 - row.a0 + i;
          }
          if (tok >= 0 && tok < V) s_token = tok;
        }
      }
    }
  }
  __syncthreads();
  return s_token;
}

// Step 9 for one token of one slot (a single thread): the append, the stop test and the advance.  hist_row / hist_len_b: the slot's history row
// and length word, or null = no append; seqlens_b: the slot's length word, or null = no advance.  hl_raw and seq are the values the caller read
// (or carried over from the token before).  -> the slot's new length (-1 = it has finished; seq itself without an advance).
__device__ __forceinline__ int sample_finish_token(int tok, int* hist_row, int max_history, int* hist_len_b, int hl_raw, const int* stop_ids,
                                                   int num_stop, int* finished_b, int* seqlens_b, int seq, int max_len) {
  if (hist_row && hist_len_b) {
    if (hl_raw >= 0 && hl_raw < max_history) hist_row[hl_raw] = tok;
    *hist_len_b = hl_raw + 1;
  }
  bool stop = false;
  if (stop_ids)
    for (int i = 0; i < num_stop; ++i) stop = stop || stop_ids[i] == tok;
  if (stop && finished_b) *finished_b = 1;
  if (!seqlens_b) return seq;
  const int next = (stop || seq + 1 >= max_len) ? -1 : seq + 1;
  *seqlens_b = next;
  return next;
}

}  // namespace sample_row
}  // namespace awq
