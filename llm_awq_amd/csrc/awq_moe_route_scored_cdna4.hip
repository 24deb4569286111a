// MoE routing for many-expert models (gfx950, wave64): awq_moe_route_scored, 1 <= E <= 512, softmax or sigmoid scores, an optional selection
// bias, group-limited selection (DeepSeek-V2 / V3), renormalised and scaled weights -- and the stable sort of the T k slots by expert that
// awq_moe_route gives (same order / inv / offsets contract, so moe_gather, the grouped launches and moe_combine follow unchanged).
//
// SELECT is one wave per token.  Expert e sits in lane e % 64, slot e / 64 (S = ceil(E / 64) = 1, 2, 4 or 8 register slots, a template value), so
// a row is read with coalesced loads and never leaves the registers.  A wave-wide maximum of the unsigned keys is a DPP scan (row_shr 1 2 4 8,
// row_bcast 15 and 31: no LDS, no bpermute) read from lane 63; the lowest expert that holds the maximum is the first slot whose ballot is not
// empty, and the lowest lane of that ballot.  Group scores are per-group maxima (and, for group_top = 2, a second maximum with the first
// position masked), parked in lane g; the kept groups are topk_group rounds of the same arg-max over lanes 0 .. n_group - 1; the pick is k
// rounds over the experts still alive.  Lane j < k ends up with pick j, so ids and weights are written with one coalesced store each.
//
// SORT.  A block of 4 waves walks a chunk of C consecutive tokens and counts its picks per expert in LDS (LDS integer atomics: the counts are
// integers, so their order does not matter).  T <= 64 is ONE launch: a single block selects, scans its own histogram and places.  Larger T is
// three launches: select (counts[chunk][E] to the workspace), scan (one block: per expert an exclusive scan over the chunks, in place, and
// offsets[E + 1]), place (block b stages its chunk's C k ids in LDS, thread e walks them in slot order and writes order / inv from
// base[b][e] -- stable by construction).  C = max(8, ceil(T / 1024)) depends on T alone: at most 1024 chunks, a workspace of at most 2 MiB.
// No global atomics, no host read, no flags to reset: a call is a pure function of its inputs, bit-stable from run to run, capturable.
#include "awq_device.hpp"
#include "awq_kernels.hpp"

namespace awq {
namespace {

constexpr int kScoredMaxE = 512, kScoredMaxK = 8, kScoredMaxGroups = 16, kScoredOneLaunchT = 64, kScoredMinChunk = 8, kScoredMaxChunks = 1024;
constexpr int kScoredMaxChunkSlots = 1032;  // C k <= max(8 * 8, (T / 1024 + 1) k) <= 2^20 / 1024 + 8

// awq_moe_route_cdna4.hip's total order on floats (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN) and its inverse
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

// v of the lanes selected by a DPP control, 0 where the control has no source lane or the row is masked off
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u32 dpp_or_zero(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// wave-uniform maximum of v over the 64 lanes: an inclusive scan whose last lane holds the whole wave
__device__ __forceinline__ u32 wave_max(u32 v) {
  v = max(v, dpp_or_zero<0x111, 0xf>(v));  // row_shr:1
  v = max(v, dpp_or_zero<0x112, 0xf>(v));  // row_shr:2
  v = max(v, dpp_or_zero<0x114, 0xf>(v));  // row_shr:4
  v = max(v, dpp_or_zero<0x118, 0xf>(v));  // row_shr:8
  v = max(v, dpp_or_zero<0x142, 0xa>(v));  // row_bcast:15 into rows 1 and 3
  v = max(v, dpp_or_zero<0x143, 0xc>(v));  // row_bcast:31 into rows 2 and 3
  return (u32)__builtin_amdgcn_readlane((int)v, 63);
}
// the same walk with an fp32 add (+0 where there is no source): one fixed order of additions, so the sum is bit-stable
__device__ __forceinline__ float wave_sum(float x) {
#define AWQ_DPP_ADD(CTRL, ROW_MASK) x += __builtin_bit_cast(float, dpp_or_zero<CTRL, ROW_MASK>(__builtin_bit_cast(u32, x)))
  AWQ_DPP_ADD(0x111, 0xf);
  AWQ_DPP_ADD(0x112, 0xf);
  AWQ_DPP_ADD(0x114, 0xf);
  AWQ_DPP_ADD(0x118, 0xf);
  AWQ_DPP_ADD(0x142, 0xa);
  AWQ_DPP_ADD(0x143, 0xc);
#undef AWQ_DPP_ADD
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
__device__ __forceinline__ float lane_value(float x, int src) {  // src is wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src));
}
__device__ __forceinline__ float sigmoid(float l) { return 1.0f / (1.0f + expf(-l)); }

struct ScoredArgs {
  const void* logits;
  const float* bias;  // fp32 [E] or null
  int T, E, K, sigmoid, renorm, n_group, topk_group, group_top, chunk;
  float scale;
};

// One token on one wave: lane j < K returns pick j (id) and its weight (w); the other lanes return id 0.
template <int LT, int S>
__device__ __forceinline__ void select_token(const ScoredArgs& a, int t, int lane, int& id, float& w) {
  const int E = a.E;
  float l[S];
  u32 key[S], alive = 0;  // bit s of alive: this lane's expert of slot s can still be picked
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int e = s * 64 + lane;
    l[s] = 0.0f;
    key[s] = 0u;
    if (e < E) {
      l[s] = load_logit<LT>(a.logits, (size_t)t * E + e);
      key[s] = float_key(a.bias ? sigmoid(l[s]) + a.bias[e] : l[s]);
      alive |= 1u << s;
    }
  }
  u32 row_max = 0;  // softmax without renormalisation: the key of the row's largest logit, before the groups mask anything
  if (!a.sigmoid && !a.renorm) {
    u32 c = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) c = ((alive >> s) & 1u) ? max(c, key[s]) : c;
    row_max = wave_max(c);
  }

  if (a.n_group > 1) {
    const int gs = E / a.n_group;
    int grp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) grp[s] = ((alive >> s) & 1u) ? (s * 64 + lane) / gs : -1;
    u32 gkey = 0;  // lane g: the key of group g's score
    for (int g = 0; g < a.n_group; ++g) {
      u32 c = 0;
#pragma unroll
      for (int s = 0; s < S; ++s) c = grp[s] == g ? max(c, key[s]) : c;
      const u32 m1 = wave_max(c);
      float score = key_float(m1);
      if (a.group_top == 2) {  // the largest key of the group with the first position of m1 taken out (gs >= 2: checked on the host)
        bool found = false;
        c = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const bool hit = grp[s] == g && key[s] == m1;
          bool first = false;
          if (!found) {
            const unsigned long long b = __ballot(hit);
            if (b) {
              found = true;
              first = lane == __ffsll(b) - 1;
            }
          }
          c = (grp[s] == g && !first) ? max(c, key[s]) : c;
        }
        score += key_float(wave_max(c));
      }
      if (lane == g) gkey = float_key(score);
    }
    u32 kept = 0;  // wave-uniform: bit g = group g is kept; equal scores go to the lower group
    for (int r = 0; r < a.topk_group; ++r) {
      const bool open = lane < a.n_group && !((kept >> lane) & 1u);
      const u32 m = wave_max(open ? gkey : 0u);
      const unsigned long long b = __ballot(open && gkey == m);
      kept |= 1u << (b ? __ffsll(b) - 1 : 0);
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (grp[s] >= 0 && !((kept >> grp[s]) & 1u)) alive &= ~(1u << s);
  }

  id = 0;
  float lj = 0.0f;  // lane j: the logit of pick j
  for (int j = 0; j < a.K; ++j) {
    u32 c = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) c = ((alive >> s) & 1u) ? max(c, key[s]) : c;
    const u32 m = wave_max(c);
    int e = 0;  // (the host checks that k experts are alive, so a round always finds one)
    float le = 0.0f;
    bool found = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (!found) {
        const unsigned long long b = __ballot(((alive >> s) & 1u) && key[s] == m);
        if (b) {
          const int src = __ffsll(b) - 1;
          found = true;
          e = s * 64 + src;
          le = lane_value(l[s], src);
          if (lane == src) alive &= ~(1u << s);
        }
      }
    }
    if (lane == j) {
      id = e;
      lj = le;
    }
  }

  // weights in fp32 on lanes 0 .. K - 1; the sum over the picked runs upwards from +0 as in awq_moe_route
  float p, den = 0.0f;
  if (a.sigmoid) {
    p = sigmoid(lj);
    for (int j = 0; j < a.K; ++j) den += lane_value(p, j);
    w = (a.renorm ? p / (den + 1e-20f) : p) * a.scale;
  } else if (a.renorm) {
    p = expf(lj - lane_value(lj, 0));
    for (int j = 0; j < a.K; ++j) den += lane_value(p, j);
    w = p / den * a.scale;
  } else {
    const float top = key_float(row_max);
    float part = 0.0f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (s * 64 + lane < E) part += expf(l[s] - top);
    w = expf(lj - top) / wave_sum(part) * a.scale;
  }
}

// wave 0: cnt[0 .. epad) in LDS (counts per expert, 0 above E) -> their exclusive scan in place, and offsets[0 .. E] in global memory
__device__ __forceinline__ void scan_experts(int* cnt, int E, int epad, int* __restrict__ offsets, int lane) {
  const int per = epad >> 6;
  int sum = 0;
  for (int i = 0; i < per; ++i) sum += cnt[lane * per + i];
  int incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  int run = incl - sum;
  for (int i = 0; i < per; ++i) {
    const int e = lane * per + i, c = cnt[e];
    cnt[e] = run;
    if (e < E) offsets[e] = run;
    run += c;
  }
  if (lane == 63) offsets[E] = run;  // = T K: every token picked K experts
}

// thread e: the n staged ids in slot order; slot0 + i goes to the next sorted row of its expert
__device__ __forceinline__ void place_expert(const int* ids, int n, int slot0, int e, int row, int total, int* __restrict__ order,
                                             int* __restrict__ inv) {
  for (int i = 0; i < n; ++i) {
    if (ids[i] != e) continue;
    if ((unsigned)row < (unsigned)total) {  // (always: the bases are sums of the counts of these ids)
      order[row] = slot0 + i;
      inv[slot0 + i] = row;
    }
    ++row;
  }
}

// T <= 64: one block of min(T, 16) waves does everything
template <int LT, int S>
__global__ __launch_bounds__(1024) void moe_route_scored_one_kernel(ScoredArgs a, int* __restrict__ topk_ids, float* __restrict__ topk_w,
                                                                    int* __restrict__ order, int* __restrict__ inv, int* __restrict__ offsets) {
  __shared__ int s_cnt[kScoredMaxE];
  __shared__ int s_ids[kScoredOneLaunchT * kScoredMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  for (int e = tid; e < kScoredMaxE; e += nthreads) s_cnt[e] = 0;
  __syncthreads();
  for (int t = wave; t < a.T; t += nwaves) {
    int id;
    float w;
    select_token<LT, S>(a, t, lane, id, w);
    if (lane < a.K) {
      topk_ids[t * a.K + lane] = id;
      topk_w[t * a.K + lane] = w;
      s_ids[t * a.K + lane] = id;
      atomicAdd(&s_cnt[id], 1);
    }
  }
  __syncthreads();
  if (wave == 0) scan_experts(s_cnt, a.E, ((a.E + 63) >> 6) << 6, offsets, lane);
  __syncthreads();
  for (int e = tid; e < a.E; e += nthreads) place_expert(s_ids, a.T * a.K, 0, e, s_cnt[e], a.T * a.K, order, inv);
}

// T > 64, launch 1 of 3: block b selects tokens [b C, b C + C) and writes counts[b][E]
template <int LT, int S>
__global__ __launch_bounds__(256) void moe_route_scored_select_kernel(ScoredArgs a, int* __restrict__ topk_ids, float* __restrict__ topk_w,
                                                                      int* __restrict__ counts) {
  __shared__ int s_cnt[kScoredMaxE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < a.E; e += 256) s_cnt[e] = 0;
  __syncthreads();
  const int t0 = blockIdx.x * a.chunk, t1 = min(a.T, t0 + a.chunk);
  for (int t = t0 + wave; t < t1; t += 4) {
    int id;
    float w;
    select_token<LT, S>(a, t, lane, id, w);
    if (lane < a.K) {
      topk_ids[(size_t)t * a.K + lane] = id;
      topk_w[(size_t)t * a.K + lane] = w;
      atomicAdd(&s_cnt[id], 1);
    }
  }
  __syncthreads();
  for (int e = tid; e < a.E; e += 256) counts[(size_t)blockIdx.x * a.E + e] = s_cnt[e];
}

// launch 2 of 3, one block of 1024 threads = R rows of epad threads: row r sums its share of the chunks per expert, wave 0 scans the experts'
// totals into offsets, then every row walks its share again and replaces counts[b][e] by base[b][e], the first sorted row of (chunk b, expert e)
__global__ __launch_bounds__(1024) void moe_route_scored_scan_kernel(int* __restrict__ counts, int* __restrict__ offsets, int E, int chunks) {
  __shared__ int s_part[1024];
  __shared__ int s_tot[kScoredMaxE];
  const int tid = threadIdx.x, epad = ((E + 63) >> 6) << 6, R = 1024 / epad, r = tid / epad, e = tid - r * epad;
  const int per = (chunks + R - 1) / R, b0 = min(chunks, r * per), b1 = min(chunks, b0 + per);
  const bool active = r < R && e < E;
  int sum = 0;
  if (active)
    for (int b = b0; b < b1; ++b) sum += counts[(size_t)b * E + e];
  s_part[tid] = sum;
  __syncthreads();
  if (tid < epad) {
    int tot = 0;
    for (int q = 0; q < R; ++q) tot += s_part[q * epad + tid];
    s_tot[tid] = tot;
  }
  __syncthreads();
  if (tid < 64) scan_experts(s_tot, E, epad, offsets, tid);
  __syncthreads();
  if (active) {
    int run = s_tot[e];
    for (int q = 0; q < r; ++q) run += s_part[q * epad + e];
    for (int b = b0; b < b1; ++b) {
      const int c = counts[(size_t)b * E + e];
      counts[(size_t)b * E + e] = run;
      run += c;
    }
  }
}

// launch 3 of 3: block b (epad threads) stages its chunk's ids and thread e places the slots of expert e
__global__ __launch_bounds__(512) void moe_route_scored_place_kernel(const int* __restrict__ topk_ids, const int* __restrict__ base,
                                                                     int* __restrict__ order, int* __restrict__ inv, int T, int E, int K, int chunk) {
  __shared__ int s_ids[kScoredMaxChunkSlots];
  const int tid = threadIdx.x, t0 = blockIdx.x * chunk, t1 = min(T, t0 + chunk);
  const int n = min((t1 - t0) * K, kScoredMaxChunkSlots), slot0 = t0 * K;
  for (int i = tid; i < n; i += blockDim.x) s_ids[i] = topk_ids[slot0 + i];
  __syncthreads();
  if (tid < E) place_expert(s_ids, n, slot0, tid, base[(size_t)blockIdx.x * E + tid], T * K, order, inv);
}

int scored_chunk(int tokens) {
  const int c = (tokens + kScoredMaxChunks - 1) / kScoredMaxChunks;
  return c < kScoredMinChunk ? kScoredMinChunk : c;
}

template <int LT, int S>
void launch_scored_t(const ScoredArgs& a, int* ids, float* w, int* order, int* inv, int* offsets, int* counts, hipStream_t st) {
  const int epad = ((a.E + 63) / 64) * 64;
  if (a.T <= kScoredOneLaunchT) {
    hipLaunchKernelGGL((moe_route_scored_one_kernel<LT, S>), dim3(1), dim3(64 * (a.T < 16 ? a.T : 16)), 0, st, a, ids, w, order, inv, offsets);
    return;
  }
  const int chunks = (a.T + a.chunk - 1) / a.chunk;
  hipLaunchKernelGGL((moe_route_scored_select_kernel<LT, S>), dim3(chunks), dim3(256), 0, st, a, ids, w, counts);
  hipLaunchKernelGGL(moe_route_scored_scan_kernel, dim3(1), dim3(1024), 0, st, counts, offsets, a.E, chunks);
  hipLaunchKernelGGL(moe_route_scored_place_kernel, dim3(chunks), dim3(epad), 0, st, ids, counts, order, inv, a.T, a.E, a.K, a.chunk);
}

template <int LT>
void launch_scored_lt(const ScoredArgs& a, int* ids, float* w, int* order, int* inv, int* offsets, int* counts, hipStream_t st) {
  if (a.E <= 64) launch_scored_t<LT, 1>(a, ids, w, order, inv, offsets, counts, st);
  else if (a.E <= 128) launch_scored_t<LT, 2>(a, ids, w, order, inv, offsets, counts, st);
  else if (a.E <= 256) launch_scored_t<LT, 4>(a, ids, w, order, inv, offsets, counts, st);
  else launch_scored_t<LT, 8>(a, ids, w, order, inv, offsets, counts, st);
}

}  // namespace

bool moe_route_scored_sizes_ok(int tokens, int experts, int top_k, int score, int has_bias, int n_group, int topk_group, int group_top) {
  if (experts < 1 || experts > kScoredMaxE || top_k < 1 || top_k > kScoredMaxK || top_k > experts || tokens < 1 ||
      (long long)tokens * top_k > (1ll << 20))
    return false;
  if ((score != 0 && score != 1) || (has_bias && score != 1)) return false;
  if (n_group < 1 || n_group > kScoredMaxGroups || (experts % n_group) != 0 || topk_group < 1 || topk_group > n_group) return false;
  const int gs = experts / n_group;
  if (topk_group * gs < top_k || group_top < 1 || group_top > 2 || group_top > gs || (score == 0 && group_top != 1)) return false;
  return true;
}

size_t moe_route_scored_workspace_bytes(int tokens, int experts, int top_k) {
  if (!moe_route_scored_sizes_ok(tokens, experts, top_k, 0, 0, 1, 1, 1) || tokens <= kScoredOneLaunchT) return 0;
  const int chunk = scored_chunk(tokens);
  return (size_t)((tokens + chunk - 1) / chunk) * experts * sizeof(int);
}

int launch_moe_route_scored(const void* logits, int logits_dtype, int tokens, int experts, int top_k, int score, int renormalize, const void* bias,
                            int n_group, int topk_group, int group_top, float scale, void* topk_ids, void* topk_w, void* order, void* inv,
                            void* offsets, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!moe_route_scored_sizes_ok(tokens, experts, top_k, score, bias != nullptr, n_group, topk_group, group_top)) return -1;
  const size_t need = moe_route_scored_workspace_bytes(tokens, experts, top_k);
  if (need && (!workspace || workspace_bytes < need)) return -2;
  const ScoredArgs a{logits, (const float*)bias, tokens, experts, top_k, score, renormalize ? 1 : 0, n_group, topk_group, group_top,
                     scored_chunk(tokens), scale};
  int *ids = (int*)topk_ids, *ord = (int*)order, *iv = (int*)inv, *off = (int*)offsets, *cnt = (int*)workspace;
  if (logits_dtype == 0) launch_scored_lt<0>(a, ids, (float*)topk_w, ord, iv, off, cnt, st);
  else if (logits_dtype == 1) launch_scored_lt<1>(a, ids, (float*)topk_w, ord, iv, off, cnt, st);
  else if (logits_dtype == 2) launch_scored_lt<2>(a, ids, (float*)topk_w, ord, iv, off, cnt, st);
  else return -1;
  return 0;
}

}  // namespace awq
