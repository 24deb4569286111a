// MoE routing on the device (gfx950, wave64): the three launches that surround the grouped expert matmuls of SparseMoeMLP(routing="device").
//
//   moe_route_kernel    router logits [T, E] -> topk_ids / topk_w [T, k], and the stable sort of the T k flat slots s = t k + j by expert:
//                       order [T k] (sorted row -> slot), inv [T k] (slot -> sorted row), offsets [E + 1] (first sorted row of every expert)
//   moe_gather_kernel   xs[r] = x[order[r] / k]
//   moe_combine_kernel  out[t] = T( sum_j f32( T( f32(ys[inv[t k + j]]) * f32(T(w[t, j])) ) ) ), fp32, j ascending, from +0
//
// No workspace, no atomics, no host read; every size that shapes a grid (T, k, E, H) is a host integer.  The route kernel is ONE block on
// purpose: nothing is ordered between blocks and there are no flags to reset, so a launch is a pure function of its inputs (and replays in a
// hipGraph).  A token picks an expert at most once, so among the slots of one expert the slot order is the token order, and a token's rank
// inside its wave is popcount(ballot(picked e) & lanes below): pass A counts per expert and scans the counts into `offsets`, pass B walks the
// tokens again in rounds of blockDim and places every slot at offsets[e] + earlier rounds + earlier waves of the round + lane rank.
#include "awq_device.hpp"
#include "awq_kernels.hpp"

namespace awq {
namespace {

constexpr int kRouteMaxE = 64, kRouteMaxK = 8, kRouteMaxWaves = 16;

// monotone float -> unsigned key: a total order whatever the bits (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN), and its inverse
__device__ __forceinline__ u32 float_key(float f) {
  const u32 b = __builtin_bit_cast(u32, f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_float(u32 k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

template <int LT>  // logits type: 0 fp16, 1 bf16, 2 fp32
__device__ __forceinline__ float load_logit(const void* p, size_t i) {
  if constexpr (LT == 2) return reinterpret_cast<const float*>(p)[i];
  else if constexpr (LT == 1) return BF16::to_float(reinterpret_cast<const uint16_t*>(p)[i]);
  else return F16::to_float(reinterpret_cast<const uint16_t*>(p)[i]);
}

// EMAX = 8 or 64: the row's keys live in registers (every index into key[] is a compile-time constant once the loops are unrolled)
template <int LT, int EMAX>
__global__ __launch_bounds__(1024) void moe_route_kernel(const void* __restrict__ logits, int* __restrict__ topk_ids, float* __restrict__ topk_w,
                                                         int* __restrict__ order, int* __restrict__ inv, int* __restrict__ offsets, int T, int E, int K,
                                                         int renorm) {
  __shared__ int s_cnt[kRouteMaxWaves][kRouteMaxE];  // pass A: a wave's totals; pass B: a wave's counts of the current round
  __shared__ int s_pre[kRouteMaxWaves][kRouteMaxE];  // pass B: first sorted row of (wave, expert) in the current round
  __shared__ int s_run[2][kRouteMaxE];               // pass B: first sorted row of an expert in the current round (double-buffered over rounds)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int rounds = (T + nthreads - 1) / nthreads, total = T * K;
  const unsigned long long below = (1ull << lane) - 1ull;

  int ids[kRouteMaxK] = {};  // the token of the LAST round keeps its picks in registers: a one-round launch never reads them back
  int my_cnt = 0;       // lane e: this wave's tokens that picked expert e, over all rounds
  for (int r = 0; r < rounds; ++r) {
    const int t = r * nthreads + tid;
    unsigned long long picked = 0;
    if (t < T) {
      u32 key[EMAX];
#pragma unroll
      for (int e = 0; e < EMAX; ++e) key[e] = e < E ? float_key(load_logit<LT>(logits, (size_t)t * E + e)) : 0u;
      float l[kRouteMaxK];
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j) {
        ids[j] = 0;
        l[j] = 0.0f;
        if (j < K) {
          // the largest key not picked yet; scanning upwards with a strict compare gives equal logits to the lower index.  K <= E: one is left.
          int be = -1;
          u32 bk = 0;
#pragma unroll
          for (int e = 0; e < EMAX; ++e) {
            const bool take = e < E && !((picked >> e) & 1ull) && (be < 0 || key[e] > bk);
            be = take ? e : be;
            bk = take ? key[e] : bk;
          }
          picked |= 1ull << be;
          ids[j] = be;
          l[j] = key_float(bk);
        }
      }
      // weights in fp32: exp(l_j - l_0) over the sum of the k picked (renormalize) or of all E (plain softmax); sums run upwards from +0
      float p[kRouteMaxK], den = 0.0f;
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j) {
        p[j] = j < K ? expf(l[j] - l[0]) : 0.0f;
        den += p[j];
      }
      if (!renorm) {
        den = 0.0f;
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
          if (e < E) den += expf(key_float(key[e]) - l[0]);
      }
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j)
        if (j < K) {
          topk_ids[(size_t)t * K + j] = ids[j];
          topk_w[(size_t)t * K + j] = p[j] / den;
        }
    }
    for (int e = 0; e < E; ++e) {
      const unsigned long long b = __ballot((picked >> e) & 1ull);
      if (lane == e) my_cnt += __popcll(b);
    }
  }
  if (lane < E) s_cnt[wave][lane] = my_cnt;
  __syncthreads();
  // thread e < E: the experts before e, summed over the waves -> offsets[e]; every token picked K experts, so the last offset is T K
  if (tid < E) {
    int off = 0;
    for (int e = 0; e < tid; ++e)
      for (int w = 0; w < nwaves; ++w) off += s_cnt[w][e];
    offsets[tid] = off;
    s_run[0][tid] = off;
  }
  if (tid == 0) offsets[E] = total;
  __syncthreads();

  for (int r = 0; r < rounds; ++r) {
    const int t = r * nthreads + tid;
    unsigned long long picked = 0;
    if (t < T) {
      if (rounds > 1) {
#pragma unroll
        for (int j = 0; j < kRouteMaxK; ++j)
          if (j < K) ids[j] = topk_ids[(size_t)t * K + j];  // this thread's own stores of pass A
      }
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j)
        if (j < K) picked |= 1ull << (ids[j] & 63);
    }
    int rank[kRouteMaxK];
#pragma unroll
    for (int j = 0; j < kRouteMaxK; ++j) rank[j] = 0;
    int cnt = 0;
    for (int e = 0; e < E; ++e) {
      const unsigned long long b = __ballot((picked >> e) & 1ull);
      if (lane == e) cnt = __popcll(b);
      const int rk = __popcll(b & below);
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j)
        if (j < K && t < T && ids[j] == e) rank[j] = rk;
    }
    const int cur = r & 1;
    if (lane < E) s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (lane < E) {
      int pre = s_run[cur][lane];
      for (int w = 0; w < wave; ++w) pre += s_cnt[w][lane];
      s_pre[wave][lane] = pre;
      if (wave == nwaves - 1) s_run[cur ^ 1][lane] = pre + cnt;
    }
    __syncthreads();
    if (t < T) {
#pragma unroll
      for (int j = 0; j < kRouteMaxK; ++j)
        if (j < K) {
          const int row = s_pre[wave][ids[j] & 63] + rank[j], slot = t * K + j;
          if ((unsigned)row < (unsigned)total) {  // (always: the counts of both passes come from the same ids)
            order[row] = slot;
            inv[slot] = row;
          }
        }
    }
  }
}

// one thread = 16 bytes of one sorted row; grid (column blocks of 256 threads, rows)
__global__ __launch_bounds__(256) void moe_gather_kernel(const u32x4* __restrict__ x, const int* __restrict__ order, u32x4* __restrict__ xs, int T, int K,
                                                         int rows, int chunks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const unsigned tok = (unsigned)order[r] / (unsigned)K;
    if (tok < (unsigned)T) xs[(size_t)r * chunks + c] = x[(size_t)tok * chunks + c];
  }
}

template <typename DT>
__global__ __launch_bounds__(256) void moe_combine_kernel(const u32x4* __restrict__ ys, const int* __restrict__ inv, const float* __restrict__ w,
                                                          u32x4* __restrict__ out, int T, int K, int chunks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const unsigned rows = (unsigned)T * (unsigned)K;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    for (int j = 0; j < K; ++j) {
      const unsigned r = (unsigned)inv[(size_t)t * K + j];
      if (r >= rows) continue;  // (never for a true permutation: no read outside ys)
      const float wt = DT::to_float(DT::from_float(w[(size_t)t * K + j]));
      const u32x4 y = ys[(size_t)r * chunks + c];
      const u32 yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[2 * i] += DT::to_float(DT::from_float(DT::to_float((uint16_t)(yw[i] & 0xFFFFu)) * wt));
        acc[2 * i + 1] += DT::to_float(DT::from_float(DT::to_float((uint16_t)(yw[i] >> 16)) * wt));
      }
    }
    u32 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (u32)DT::from_float(acc[2 * i]) | ((u32)DT::from_float(acc[2 * i + 1]) << 16);
    out[(size_t)t * chunks + c] = u32x4{o[0], o[1], o[2], o[3]};
  }
}

template <int LT>
void launch_route_t(const void* logits, int* ids, float* w, int* order, int* inv, int* offsets, int T, int E, int K, int renorm, hipStream_t st) {
  const int threads = T >= 1024 ? 1024 : ((T + 63) / 64) * 64;
  if (E <= 8) hipLaunchKernelGGL((moe_route_kernel<LT, 8>), dim3(1), dim3(threads), 0, st, logits, ids, w, order, inv, offsets, T, E, K, renorm);
  else hipLaunchKernelGGL((moe_route_kernel<LT, 64>), dim3(1), dim3(threads), 0, st, logits, ids, w, order, inv, offsets, T, E, K, renorm);
}

}  // namespace

int launch_moe_route(const void* logits, int logits_dtype, int tokens, int experts, int top_k, int renormalize, void* topk_ids, void* topk_w,
                     void* order, void* inv, void* offsets, hipStream_t st) {
  if (experts < 1 || experts > kRouteMaxE || top_k < 1 || top_k > kRouteMaxK || top_k > experts || tokens < 1 ||
      (long long)tokens * top_k > (1ll << 20))
    return -1;
  int *ids = (int*)topk_ids, *ord = (int*)order, *iv = (int*)inv, *off = (int*)offsets;
  if (logits_dtype == 0) launch_route_t<0>(logits, ids, (float*)topk_w, ord, iv, off, tokens, experts, top_k, renormalize, st);
  else if (logits_dtype == 1) launch_route_t<1>(logits, ids, (float*)topk_w, ord, iv, off, tokens, experts, top_k, renormalize, st);
  else if (logits_dtype == 2) launch_route_t<2>(logits, ids, (float*)topk_w, ord, iv, off, tokens, experts, top_k, renormalize, st);
  else return -1;
  return 0;
}

int launch_moe_gather(const void* x, const void* order, void* xs, int tokens, int top_k, int hidden, hipStream_t st) {
  if (tokens < 1 || top_k < 1 || hidden < 8 || (hidden % 8) != 0 || (long long)tokens * top_k > (1ll << 20)) return -1;
  const int chunks = hidden / 8, rows = tokens * top_k;
  hipLaunchKernelGGL(moe_gather_kernel, dim3((chunks + 255) / 256, rows > 65535 ? 65535 : rows), dim3(256), 0, st, (const u32x4*)x, (const int*)order,
                     (u32x4*)xs, tokens, top_k, rows, chunks);
  return 0;
}

int launch_moe_combine(const void* ys, const void* inv, const void* topk_w, void* out, int tokens, int top_k, int hidden, int dtype, hipStream_t st) {
  if (tokens < 1 || top_k < 1 || hidden < 8 || (hidden % 8) != 0 || (long long)tokens * top_k > (1ll << 20)) return -1;
  const int chunks = hidden / 8;
  const dim3 grid((chunks + 255) / 256, tokens > 65535 ? 65535 : tokens);
  if (dtype == 0) hipLaunchKernelGGL((moe_combine_kernel<F16>), grid, dim3(256), 0, st, (const u32x4*)ys, (const int*)inv, (const float*)topk_w, (u32x4*)out, tokens, top_k, chunks);
  else hipLaunchKernelGGL((moe_combine_kernel<BF16>), grid, dim3(256), 0, st, (const u32x4*)ys, (const int*)inv, (const float*)topk_w, (u32x4*)out, tokens, top_k, chunks);
  return 0;
}

}  // namespace awq
