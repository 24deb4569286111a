// Token log-probabilities (gfx950, wave64): the LM head fused with log-sum-exp.  For T rows of hidden states x [T, K] and nn.Linear.weight W [V, K]
// (as loaded, no repack) a row's lse, target logit, logprob and argmax come out WITHOUT a logit ever being written to memory (DESIGN.md "Token
// log-probabilities" states the contract by values; tests/lm_logprobs_oracle.py restates it).  Two launches, no atomics, no host read:
//
//   tiles    grid = (row tiles of kLpRT tokens) x (vocabulary tiles of kLpVT rows), block ids ordered so that the row tiles of one vocabulary tile are
//            neighbours, then dealt to the XCDs in contiguous ranges: a W tile is fetched into one L2 and reused by every row tile.  A capped grid
//            (max_blocks) walks the same tiles with a stride; a tile's result does not depend on the block that computes it.
//            256 threads = 4 waves as 2 (vocabulary halves) x 2 (token halves), each 64 x 64 on v_mfma_f32_32x32x16 with W as the A operand and x as B:
//            D has the TOKEN on the lane (lane % 32) and 16 vocabulary rows in the lane's registers, so the max / sum-exp over a tile's rows is
//            in-register, then one cross-lane step (lane ^ 32 holds the other 16 rows of the 32), then one LDS meeting of the two waves that split V.
//            Staging: both operands are k-contiguous; a k step is 64 k = one 128-byte line per row, brought in by 16-byte LDS-DMA (the LDS image is
//            lane-linear, the XOR swizzle is applied to the source address and to the ds_read), two buffers, vmcnt(0) + one barrier per step.  The k
//            tail (K % 64) is one more step staged by plain loads with zeros past K.  Rows past V / T are clamped for the load; logits of rows past V
//            are set to -inf BEFORE the reduction.
//            Per (vocabulary tile, token) the block writes (m, s = sum exp(z - m), first index of m); the tile holding targets[t] writes z[t, target].
//            A row tile whose rows are all ignored leaves before its first load.
//   combine  one wave per row: M = max_t m_t, S = sum_t s_t exp(m_t - M) with tile t on lane t % 64 in ascending order and a butterfly over the lanes,
//            lse = M + log S, argmax = the index of the lowest tile holding M, logprob = target_logit - lse.
// Every sum order depends on (V, K) and compile-time constants only -- not on T, the row's index, other rows or the grid: a row's outputs are the same
// bits wherever it is served.  A token is a COLUMN of the matrix product: whatever an ignored row of x holds (NaN included) stays in its own column.
//
// token_logprobs_kernel is the companion for logits that already exist ([B, V] fp32 / T with a row stride): one block per row, two passes, fixed order.
//
//   cap      awq_lm_head_logprobs_softcap (awq_softcap.hpp): every logit is capped in the tile epilogue, z <- cap * tanh(z / cap) in fp32 behind the
//            bias, BEFORE it enters the max / sum-exp, the target pick and the argmax.  With round_logits z is rounded to T, capped in fp32 and
//            rounded to T once more.  A compile-time form: lp_tile_softcap_kernel is lp_tile_body<.., true>, lp_tile_kernel stays <.., false>.
#include "awq_device.hpp"
#include "awq_kernels.hpp"
#include "awq_softcap.hpp"

namespace awq {
namespace {

constexpr int kLpThreads = 256;
constexpr int kLpRT = 128, kLpVT = 128, kLpBK = 64;          // tokens / vocabulary rows per tile, k per step
constexpr int kLpOpBytes = 128 * kLpBK * 2;                   // one operand's image of a k step: 128 rows x 128 bytes
constexpr int kLpBufBytes = 2 * kLpOpBytes;                   // W image, then x image
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
constexpr float kNegInf = -__builtin_inff();

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LpArgs {
  const uint16_t* x;
  const uint16_t* w;
  const uint16_t* bias;
  const int* targets;
  float* pm;    // [row tile][vocabulary tile][kLpRT]
  float* ps;
  int* pi;
  float* ptl;   // [row tile][kLpRT]: z[t, targets[t]]
  long ldx;
  int t, v, k, round_logits, ntr, ntv;
};

// exp(d) for d <= 0 (or -inf) on the hardware exp2: one rounding for the multiply, one ulp for v_exp_f32
__device__ __forceinline__ float lp_exp(float d) { return __builtin_amdgcn_exp2f(d * kLog2e); }

struct LpPart {
  float m, s;
  int i;
};
// two partial (max, sum, first index) of disjoint column sets, `a` the one the merge order names first; commutative in nothing: callers fix the order
__device__ __forceinline__ LpPart lp_merge(const LpPart& a, const LpPart& b) {
  LpPart r;
  r.m = fmaxf(a.m, b.m);
  const float ea = a.m == kNegInf ? 0.f : lp_exp(a.m - r.m), eb = b.m == kNegInf ? 0.f : lp_exp(b.m - r.m);
  r.s = a.s * ea + b.s * eb;
  r.i = a.m > b.m ? a.i : (b.m > a.m ? b.i : (a.i < b.i ? a.i : b.i));
  return r;
}

template <typename DT, bool CAP>
__device__ __forceinline__ void lp_tile_body(const LpArgs& a, float cap) {
  (void)cap;
  using vec8 = typename DT::vec8;
  __shared__ __attribute__((aligned(16))) char smem[2 * kLpBufBytes];  // ALL of the block's LDS: the two staging buffers; the epilogue's meeting reuses it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r32 = lane & 31, h = lane >> 5;
  const int T = a.t, V = a.v, K = a.k;
  const int ntiles = a.ntr * a.ntv, nfull = K / kLpBK, ktail = K % kLpBK;

  for (int id = blockIdx.x; id < ntiles; id += gridDim.x) {
    int tile = id;
    if ((int)gridDim.x == ntiles) {  // block b runs on XCD b % 8: give every XCD a contiguous range of tiles (bijective for any count)
      const int xcd = id & 7, idx = id >> 3, q = ntiles >> 3, r = ntiles & 7;
      tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int rt = tile % a.ntr, vt = tile / a.ntr, t0 = rt * kLpRT, v0 = vt * kLpVT;

    // every wave looks at all of the tile's rows, so the exit is uniform over the block without a barrier
    bool act = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = t0 + lane + 64 * j;
      if (t < T) act |= a.targets == nullptr || (u32)a.targets[t] < (u32)V;
    }
    if (__ballot(act) == 0) continue;

    // staging: granule p = q * 256 + tid of an image is row p / 8, LDS slot p % 8, and receives the row's 16-byte chunk slot ^ (row % 8)
    const int srow = tid >> 3, chunk = (tid & 7) ^ (srow & 7);
    const uint16_t *wsrc[4], *xsrc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = q * 32 + srow;
      wsrc[q] = a.w + (size_t)(v0 + row < V ? v0 + row : V - 1) * (size_t)K + chunk * 8;
      xsrc[q] = a.x + (size_t)(t0 + row < T ? t0 + row : T - 1) * (size_t)a.ldx + chunk * 8;
    }
    auto stage = [&](int kt, int buf) {
      char* dst = smem + buf * kLpBufBytes + wave * 1024;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[q] + (size_t)kt * kLpBK),
                                         (__attribute__((address_space(3))) void*)(dst + q * 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xsrc[q] + (size_t)kt * kLpBK),
                                         (__attribute__((address_space(3))) void*)(dst + kLpOpBytes + q * 4096), 16, 0, 0);
      }
    };

    f32x16 acc[2][2];  // [vocabulary sub-tile][token sub-tile]
#pragma unroll
    for (int vi = 0; vi < 2; ++vi)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[vi][ti][e] = 0.f;

    // lane (r32, h) of a 32x32x16 operand holds k = 8 h + {0..7} of row r32: chunk 2 kk + h of the step's line
    auto compute = [&](int buf, int nkk) {
      const char* wb = smem + buf * kLpBufBytes + (wr * 64 + r32) * 128;
      const char* xb = smem + buf * kLpBufBytes + kLpOpBytes + (wc * 64 + r32) * 128;
      for (int kk = 0; kk < nkk; ++kk) {
        const int off = ((2 * kk + h) ^ (r32 & 7)) << 4;
        vec8 av[2], bv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          av[i] = *reinterpret_cast<const vec8*>(wb + i * 32 * 128 + off);
          bv[i] = *reinterpret_cast<const vec8*>(xb + i * 32 * 128 + off);
        }
#pragma unroll
        for (int vi = 0; vi < 2; ++vi)
#pragma unroll
          for (int ti = 0; ti < 2; ++ti) acc[vi][ti] = DT::mfma32(av[vi], bv[ti], acc[vi][ti]);
      }
    };

    if (nfull > 0) stage(0, 0);
    for (int kt = 0; kt < nfull; ++kt) {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's share of step kt has landed ...
      __syncthreads();                     // ... and so has everybody's; all reads of the other buffer (step kt - 1) are done
      if (kt + 1 < nfull) stage(kt + 1, (kt + 1) & 1);
      compute(kt & 1, 4);
    }
    if (ktail) {  // the ragged step: plain loads, zeros past K
      __syncthreads();
      const bool ok = nfull * kLpBK + chunk * 8 < K;
      const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32x4 wv = ok ? *reinterpret_cast<const u32x4*>(wsrc[q] + (size_t)nfull * kLpBK) : zero;
        const u32x4 xv = ok ? *reinterpret_cast<const u32x4*>(xsrc[q] + (size_t)nfull * kLpBK) : zero;
        *reinterpret_cast<u32x4*>(smem + q * 4096 + tid * 16) = wv;
        *reinterpret_cast<u32x4*>(smem + kLpOpBytes + q * 4096 + tid * 16) = xv;
      }
      __syncthreads();
      compute(0, (ktail + 15) >> 4);
    }

    // ---- epilogue: the reduction.  Register e of sub-tile vi is vocabulary row v0 + 64 wr + 32 vi + (e % 4) + 8 (e / 4) + 4 h: ascending in (vi, e)
    float bz[32];  // the bias of this lane's 32 rows, loaded under ONE branch (a select per element would wait for every load on its own)
    if (a.bias != nullptr) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const int v = v0 + wr * 64 + (i >> 4) * 32 + (i & 3) + 8 * ((i & 15) >> 2) + 4 * h;
        bz[i] = DT::to_float(a.bias[v < V ? v : V - 1]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 32; ++i) bz[i] = 0.f;
    }
    LpPart part[2];
    float tl[2];
    bool has[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const int t = t0 + wc * 64 + ti * 32 + r32;
      const int tgt = (a.targets != nullptr && t < T) ? a.targets[t] : -1;
      float z[32];
      LpPart p = {kNegInf, 0.f, 0x7fffffff};
      tl[ti] = 0.f;
      has[ti] = false;
#pragma unroll
      for (int vi = 0; vi < 2; ++vi)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int v = v0 + wr * 64 + vi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          float zz = acc[vi][ti][e] + bz[vi * 16 + e];  // (+ 0.f without a bias: exact)
          if (a.round_logits) zz = DT::to_float(DT::from_float(zz));
          if constexpr (CAP) {
            zz = softcap_logit(zz, cap);
            if (a.round_logits) zz = DT::to_float(DT::from_float(zz));
          }
          if (v >= V) zz = kNegInf;
          z[vi * 16 + e] = zz;
          if (zz > p.m) {
            p.m = zz;
            p.i = v;
          }
          if (v == tgt) {
            tl[ti] = zz;
            has[ti] = true;
          }
        }
      if (p.m > kNegInf) {
#pragma unroll
        for (int e = 0; e < 32; ++e) p.s += lp_exp(z[e] - p.m);
      }
      // the other 16 rows of the 32 sit on lane ^ 32; the h = 0 half is named first on both sides, so both compute the same bits
      LpPart o = {__shfl_xor(p.m, 32, 64), __shfl_xor(p.s, 32, 64), __shfl_xor(p.i, 32, 64)};
      const float tlo = __shfl_xor(tl[ti], 32, 64);
      const bool haso = __shfl_xor((int)has[ti], 32, 64) != 0;
      part[ti] = h == 0 ? lp_merge(p, o) : lp_merge(o, p);
      if (haso) {
        tl[ti] = tlo;
        has[ti] = true;
      }
    }
    __syncthreads();  // the staging buffers are free: the waves that split V meet there
    struct Meet {
      float m, s;
      int i;
      float tl;
      int has;
    };
    Meet* meet = reinterpret_cast<Meet*>(smem);
    if (wr == 1 && h == 0) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) meet[(wc * 2 + ti) * 32 + r32] = Meet{part[ti].m, part[ti].s, part[ti].i, tl[ti], (int)has[ti]};
    }
    __syncthreads();
    if (wr == 0 && h == 0) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        const int row = wc * 64 + ti * 32 + r32, t = t0 + row;
        if (t >= T) continue;
        if (a.targets != nullptr && (u32)a.targets[t] >= (u32)V) continue;  // an ignored row: nothing of it is written
        const Meet mo = meet[(wc * 2 + ti) * 32 + r32];
        const LpPart r = lp_merge(part[ti], LpPart{mo.m, mo.s, mo.i});
        const size_t o = ((size_t)rt * (size_t)a.ntv + (size_t)vt) * kLpRT + row;
        a.pm[o] = r.m;
        a.ps[o] = r.s;
        a.pi[o] = r.i;
        if (has[ti]) a.ptl[(size_t)rt * kLpRT + row] = tl[ti];
        else if (mo.has) a.ptl[(size_t)rt * kLpRT + row] = mo.tl;
      }
    }
    __syncthreads();  // the next tile stages into the meeting's bytes
  }
}

template <typename DT>
__global__ __launch_bounds__(kLpThreads) void lp_tile_kernel(const LpArgs a) {
  lp_tile_body<DT, false>(a, 0.f);
}
// the cap rides BEHIND LpArgs: lp_tile_kernel keeps its argument block
template <typename DT>
__global__ __launch_bounds__(kLpThreads) void lp_tile_softcap_kernel(const LpArgs a, float cap) {
  lp_tile_body<DT, true>(a, cap);
}

struct LpOut {
  const int* targets;
  float* logprob;
  float* lse;
  float* target_logit;
  int* argmax;
};

__global__ __launch_bounds__(256) void lp_combine_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const int* __restrict__ pi,
                                                         const float* __restrict__ ptl, const LpOut o, int T, int V, int ntv) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  if (o.targets != nullptr && (u32)o.targets[row] >= (u32)V) return;
  const size_t base = ((size_t)(row / kLpRT) * (size_t)ntv) * kLpRT + (row % kLpRT);
  float M = kNegInf;
  for (int j = lane; j < ntv; j += 64) M = fmaxf(M, pm[base + (size_t)j * kLpRT]);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) M = fmaxf(M, __shfl_xor(M, d, 64));
  float S = 0.f;
  int I = 0x7fffffff;
  for (int j = lane; j < ntv; j += 64) {
    const float m = pm[base + (size_t)j * kLpRT];
    if (m == kNegInf) continue;
    S += ps[base + (size_t)j * kLpRT] * lp_exp(m - M);
    if (m == M) {
      const int i = pi[base + (size_t)j * kLpRT];
      I = i < I ? i : I;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    S += __shfl_xor(S, d, 64);
    const int io = __shfl_xor(I, d, 64);
    I = io < I ? io : I;
  }
  if (lane != 0) return;
  const float lse = M + __builtin_amdgcn_logf(S) * kLn2;
  if (o.lse) o.lse[row] = lse;
  if (o.argmax) o.argmax[row] = I;
  if (o.targets != nullptr) {
    const float tlv = ptl[row];
    if (o.target_logit) o.target_logit[row] = tlv;
    if (o.logprob) o.logprob[row] = tlv - lse;
  }
}

// ---- logits that already exist: one block of 1024 threads per row.  Thread t takes columns t, t + 1024, ... in ascending order, twice: the max with its
// first index, then the sum of exp(z - M) (eight independent loads in flight per thread; the additions stay in column order); the threads meet by a wave
// butterfly and the sixteen waves' partials are taken in wave order.  DTYPE 0 fp16, 1 bf16, 2 fp32.
constexpr int kRowThreads = 1024, kRowWaves = 16, kRowUnroll = 8;

template <int DTYPE>
__device__ __forceinline__ float lp_logit(const void* row, int v) {
  if constexpr (DTYPE == 2) return reinterpret_cast<const float*>(row)[v];
  else if constexpr (DTYPE == 0) return F16::to_float(reinterpret_cast<const uint16_t*>(row)[v]);
  else return BF16::to_float(reinterpret_cast<const uint16_t*>(row)[v]);
}
// columns v0, v0 + 1024, ...: every load is issued (past V: the last column, then replaced by -inf), so none waits for a branch
template <int DTYPE>
__device__ __forceinline__ void lp_logits8(const void* row, int v0, int V, float (&z)[kRowUnroll]) {
#pragma unroll
  for (int j = 0; j < kRowUnroll; ++j) {
    const int v = v0 + j * kRowThreads;
    z[j] = lp_logit<DTYPE>(row, v < V ? v : V - 1);
  }
#pragma unroll
  for (int j = 0; j < kRowUnroll; ++j)
    if (v0 + j * kRowThreads >= V) z[j] = kNegInf;
}

template <int DTYPE>
__global__ __launch_bounds__(kRowThreads) void token_logprobs_kernel(const void* __restrict__ logits, long ld, const LpOut o, int V) {
  __shared__ float sh[3 * kRowWaves];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tgt = -1;
  if (o.targets != nullptr) {
    tgt = o.targets[row];
    if ((u32)tgt >= (u32)V) return;  // uniform over the block
  }
  const void* zr = reinterpret_cast<const char*>(logits) + (size_t)row * (size_t)ld * (DTYPE == 2 ? 4 : 2);
  float m = kNegInf;
  int idx = 0x7fffffff;
  for (int v0 = tid; v0 < V; v0 += kRowThreads * kRowUnroll) {
    float z[kRowUnroll];
    lp_logits8<DTYPE>(zr, v0, V, z);
#pragma unroll
    for (int j = 0; j < kRowUnroll; ++j)
      if (z[j] > m) {
        m = z[j];
        idx = v0 + j * kRowThreads;
      }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float mo = __shfl_xor(m, d, 64);
    const int io = __shfl_xor(idx, d, 64);
    if (mo > m || (mo == m && io < idx)) {
      m = mo;
      idx = io;
    }
  }
  if (lane == 0) {
    sh[wave] = m;
    reinterpret_cast<int*>(sh)[kRowWaves + wave] = idx;
  }
  __syncthreads();
  float M = sh[0];
  int I = reinterpret_cast<int*>(sh)[kRowWaves];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) {
    const float mo = sh[w];
    const int io = reinterpret_cast<int*>(sh)[kRowWaves + w];
    if (mo > M || (mo == M && io < I)) {
      M = mo;
      I = io;
    }
  }
  float s = 0.f;
  for (int v0 = tid; v0 < V; v0 += kRowThreads * kRowUnroll) {
    float z[kRowUnroll];
    lp_logits8<DTYPE>(zr, v0, V, z);
#pragma unroll
    for (int j = 0; j < kRowUnroll; ++j) s += lp_exp(z[j] - M);  // (a column past V: exp(-inf) = 0, added exactly)
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) sh[2 * kRowWaves + wave] = s;
  __syncthreads();
  if (tid != 0) return;
  float S = sh[2 * kRowWaves];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) S += sh[2 * kRowWaves + w];
  const float lse = M + __builtin_amdgcn_logf(S) * kLn2;
  if (o.lse) o.lse[row] = lse;
  if (o.argmax) o.argmax[row] = I;
  if (o.targets != nullptr && o.logprob) o.logprob[row] = lp_logit<DTYPE>(zr, tgt) - lse;
}

size_t lp_align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int lm_logprobs_plan(int t, int v, int k, int out[4]) {
  if (t < 1 || v < 1 || v > (1 << 30) || k < 8 || (k % 8) != 0) return -1;
  const long long ntr = ((long long)t + kLpRT - 1) / kLpRT, ntv = ((long long)v + kLpVT - 1) / kLpVT;
  if (ntr * ntv > 0x7fffffffLL) return -1;
  out[0] = kLpRT;
  out[1] = kLpVT;
  out[2] = (int)(ntr * ntv);
  out[3] = kLpBK;
  return 0;
}

// [xn: T [t, k], only with gamma][pm][ps][pi: fp32 / int32 [row tiles][vocabulary tiles][kLpRT] each][ptl: fp32 [row tiles][kLpRT]], every part on a 256-byte boundary
size_t lm_logprobs_workspace_bytes(int t, int v, int k, int with_gamma) {
  int plan[4];
  if (lm_logprobs_plan(t, v, k, plan) != 0) return 0;
  const size_t ntr = ((size_t)t + kLpRT - 1) / kLpRT;
  return (with_gamma ? lp_align256((size_t)t * (size_t)k * 2) : 0) + 3 * lp_align256((size_t)plan[2] * kLpRT * 4) + lp_align256(ntr * kLpRT * 4);
}

int launch_lm_logprobs(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets, float* logprob,
                       float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits, void* workspace, int max_blocks,
                       hipStream_t st) {
  return launch_lm_logprobs_softcap(x, ldx, gamma, eps, weight, bias, targets, logprob, lse, target_logit, argmax, t, v, k, dtype, round_logits, 0.f,
                                    workspace, max_blocks, st);
}

// softcap > 0: the capped tile epilogue; 0: launch_lm_logprobs, the same kernels
int launch_lm_logprobs_softcap(const void* x, long ldx, const void* gamma, float eps, const void* weight, const void* bias, const int* targets,
                               float* logprob, float* lse, float* target_logit, int* argmax, int t, int v, int k, int dtype, int round_logits,
                               float softcap, void* workspace, int max_blocks, hipStream_t st) {
  int plan[4];
  if (lm_logprobs_plan(t, v, k, plan) != 0 || ldx < k || (ldx % 8) != 0 || max_blocks < 0 || (gamma && ldx != k)) return -1;
  char* ws = reinterpret_cast<char*>(workspace);
  if (gamma) {
    if (launch_rmsnorm(x, gamma, eps, ws, t, k, dtype, st) != 0) return -1;
    x = ws;
    ws += lp_align256((size_t)t * (size_t)k * 2);
  }
  const size_t part = lp_align256((size_t)plan[2] * kLpRT * 4);
  const int ntr = (t + kLpRT - 1) / kLpRT, ntv = (v + kLpVT - 1) / kLpVT;
  const LpArgs a = {(const uint16_t*)x, (const uint16_t*)weight, (const uint16_t*)bias, targets, (float*)ws, (float*)(ws + part), (int*)(ws + 2 * part),
                    (float*)(ws + 3 * part), ldx, t, v, k, round_logits != 0, ntr, ntv};
  const int blocks = max_blocks > 0 && max_blocks < plan[2] ? max_blocks : plan[2];
  if (softcap > 0.f) {
    if (dtype == 0) hipLaunchKernelGGL((lp_tile_softcap_kernel<F16>), dim3(blocks), dim3(kLpThreads), 0, st, a, softcap);
    else hipLaunchKernelGGL((lp_tile_softcap_kernel<BF16>), dim3(blocks), dim3(kLpThreads), 0, st, a, softcap);
  } else if (dtype == 0) hipLaunchKernelGGL((lp_tile_kernel<F16>), dim3(blocks), dim3(kLpThreads), 0, st, a);
  else hipLaunchKernelGGL((lp_tile_kernel<BF16>), dim3(blocks), dim3(kLpThreads), 0, st, a);
  const LpOut o = {targets, logprob, lse, target_logit, argmax};
  hipLaunchKernelGGL(lp_combine_kernel, dim3((t + 3) / 4), dim3(256), 0, st, a.pm, a.ps, a.pi, a.ptl, o, t, v, ntv);
  return 0;
}

int launch_token_logprobs(const void* logits, int logits_dtype, long ld, const int* targets, float* logprob, float* lse, int* argmax, int b, int v,
                          hipStream_t st) {
  if (b < 1 || v < 1 || ld < v) return -1;
  const LpOut o = {targets, logprob, lse, nullptr, argmax};
  if (logits_dtype == 2) hipLaunchKernelGGL((token_logprobs_kernel<2>), dim3(b), dim3(kRowThreads), 0, st, logits, ld, o, v);
  else if (logits_dtype == 0) hipLaunchKernelGGL((token_logprobs_kernel<0>), dim3(b), dim3(kRowThreads), 0, st, logits, ld, o, v);
  else hipLaunchKernelGGL((token_logprobs_kernel<1>), dim3(b), dim3(kRowThreads), 0, st, logits, ld, o, v);
  return 0;
}

}  // namespace awq
