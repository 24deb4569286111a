// Encoder-tower attention (the vision towers of NVILA / InternVL: tinychat/modules/fused_siglipdecoder.py:162-168 calls
// flash_attn_func(q, k, v, causal=False) at Dh = 72, tinychat/models/internvl/internvit.py:45-90 calls
// flash_attn_varlen_qkvpacked_func(qkv [nnz, 3, H, 64], cu_seqlens, max_s, ..., causal=False)).
//
//   O = softmax(scale * Q K^T) V, no mask but the end of the sequence.  Two forms of one kernel:
//   varlen (cu_seqlens != NULL)   rows packed [total_rows, H, Dh]; sequence s owns rows cu_seqlens[s] .. cu_seqlens[s + 1] - 1 and a row
//                                 attends exactly the keys of its own sequence.  cu_seqlens is read ON THE DEVICE: the grid comes from
//                                 (nseq, max_seqlen) alone, a block whose q tile starts at or beyond its sequence's length returns
//                                 before any barrier (zero-length sequences included), and begin / end are clamped into
//                                 [0, total_rows] so that no row index leaves the tensors whatever cu_seqlens holds.
//   dense  (cu_seqlens == NULL)   nseq sequences of Sq query / Sk key rows with batch strides, query head h reads KV head h / G:
//                                 awq_attn_prefill's layout, reached through it for Dh = 72.
//
// The loop is awq_attn_prefill_cdna4.hip's without the causal mask: one block = NW waves = a q tile of 32 NW rows of one (sequence, head),
// K / V walked in 64-key tiles double-buffered in LDS through registers, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16, P rounded
// to T once with the row sum taken from the rounded weights, V^T read with ds_read_b64_tr_b16, fp32 accumulation, no workspace, no atomics:
// bit-deterministic and capturable.
//
// Head dim 72: a (row, head) is 144 bytes = nine 16-byte chunks, and no global load touches a byte outside them.
//   * Q K^T has five k-steps; in the last one the lanes hh = 1 would hold columns 72 .. 79.  They load nothing: their Q operand is zero
//     and so is their K operand (the LDS read is replaced, not multiplied away: 0 x NaN is NaN).
//   * K image: pitch 72 elements = 36 dwords, unswizzled.  The 16 rows of one ds_read_b128 lane group cover the 16 residues mod 16 and
//     36 r mod 64 sends those to 16 distinct 4-dword bank groups.
//   * V image: pitch 96 elements = 48 dwords.  A transposed read takes, per 32-lane half, 4 consecutive rows x 16 dwords; 48 r mod 64
//     = 0, 48, 32, 16 puts the four rows on the four quarters of the banks.  O has three 32-column blocks; the last one reads chunks
//     8 .. 11 of the pitch, of which only chunk 8 is ever written -- the rest feeds output columns >= 72, which are not stored.
//   * 576 chunks per tile do not divide over 128 or 256 threads: the last staging step belongs to wave 0 alone (wave-uniform guard).
#include "awq_device.hpp"
#include "awq_kernels.hpp"

#include <math.h>
#include <string.h>

namespace awq {
namespace {

constexpr int kKV = 64;        // keys per tile
constexpr int kMfmaRows = 32;  // q rows per wave
constexpr int kCUs = 256;      // the MI355X; a constant because the plan is a host-only function that CPU tests pin
int g_force_rows = 0;          // knob tower_rows (awq_tune_set): 32 / 64 / 128 forces the q tile, 0 = the plan's choice

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

struct TowerArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* out;
  const int* cu;                                  // NULL: the dense form
  long long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;   // elements; the batch strides are used by the dense form only
  long long total_rows;                           // varlen: rows of q / k / v / out
  int nseq, Sq, Sk, H, G;                         // dense: Sq x Sk per sequence; varlen: both come from cu
  float scale_log2e;
};

// LDS images.  Dh = 64: awq_attn_prefill_cdna4.hip's XOR-swizzled rows of 64.  Dh = 72: see the head of the file.
template <int DH>
__device__ __forceinline__ int k_off(int row, int ch) {
  return DH == 64 ? row * 64 + ((ch ^ ((row >> 1) & 7)) << 3) : row * 72 + (ch << 3);
}
template <int DH>
__device__ __forceinline__ int v_off(int row, int ch) {
  return DH == 64 ? row * 64 + ((ch ^ (((row >> 1) & 1) << 2)) << 3) : row * 96 + (ch << 3);
}

template <typename DT, int DH, int NW>
__global__ __launch_bounds__(NW * 64) void attn_tower_kernel(TowerArgs a) {
  using vec8 = typename DT::vec8;
  using elem = typename DT::elem;
  static_assert(DH == 64 || DH == 72, "head dims 64 and 72");
  constexpr int NT = NW * 64;
  constexpr int CPR = DH / 8;                      // 16-byte chunks per (row, head)
  constexpr int CHUNKS = kKV * CPR;                // .. per K (or V) tile
  constexpr int LOADS = (CHUNKS + NT - 1) / NT;    // staging steps per thread; the last one may be partial
  constexpr int KS = (DH + 15) / 16;               // k-steps of Q K^T (Dh = 72: the upper half of the last one is padding)
  constexpr int DB = (DH + 31) / 32;               // 32-column blocks of O (Dh = 72: 8 columns of the last one exist)
  constexpr int KP = DH, VP = DH == 64 ? 64 : 96;  // row pitches of the two images
  __shared__ __attribute__((aligned(16))) uint16_t k_s[2][kKV * KP];
  __shared__ __attribute__((aligned(16))) uint16_t v_s[2][kKV * VP];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bi = blockIdx.x;
  const int h = bi % a.H;
  bi /= a.H;
  const int seq = bi % a.nseq;
  const int tile = bi / a.nseq;
  const int kvh = h / a.G;

  int lenq, lenk;
  long long qo, ko, vo, orow;  // element offsets of the sequence's first row in q / k / v, its first row in out
  if (a.cu) {
    const long long tr = a.total_rows;
    long long b = a.cu[seq], e = a.cu[seq + 1];
    b = b < 0 ? 0 : (b > tr ? tr : b);
    e = e < b ? b : (e > tr ? tr : e);  // 0 <= b <= e <= total_rows: every row b + i, i < e - b, exists
    lenq = lenk = (int)(e - b);
    qo = b * a.q_rs;
    ko = b * a.k_rs;
    vo = b * a.v_rs;
    orow = b;
  } else {
    lenq = a.Sq;
    lenk = a.Sk;
    qo = seq * a.q_bs;
    ko = seq * a.k_bs;
    vo = seq * a.v_bs;
    orow = (long long)seq * a.Sq;
  }
  const int q0 = tile * (NW * kMfmaRows);
  if (q0 >= lenq) return;  // block-uniform, before the first barrier; covers zero-length sequences
  const int nt = (lenk + kKV - 1) / kKV;

  const int wq0 = q0 + wave * kMfmaRows;
  const bool wave_on = wq0 < lenq;        // (a wave past the last row still stages K / V and meets the barriers)
  const int qi = min(wq0 + r, lenq - 1);  // rows >= lenq compute row lenq - 1 again and are not stored
  const int lim = lenk - 1;               // last key of the sequence

  // Q: the B operand of S^T = K Q^T, lane (r, hh) holds Q[row r][16 ks + 8 hh + 0..7]; columns >= Dh are zero and are not loaded
  vec8 qf[KS];
  {
    const uint16_t* qp = a.q + qo + (long long)qi * a.q_rs + (long long)h * DH + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (16 * ks + 16 <= DH || hh == 0) w = *reinterpret_cast<const u32x4*>(qp + 16 * ks);
      qf[ks] = __builtin_bit_cast(vec8, w);
    }
  }

  const uint16_t* kb = a.k + ko + (long long)kvh * DH;
  const uint16_t* vb = a.v + vo + (long long)kvh * DH;
  u32x4 kr[LOADS], vr[LOADS];
  auto stage_load = [&](int t0) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      if ((i + 1) * NT <= CHUNKS || c < CHUNKS) {
        const long long g = min(t0 + row, lenk - 1);  // rows >= lenk are never read: clamped here, masked below
        kr[i] = *reinterpret_cast<const u32x4*>(kb + g * a.k_rs + ch * 8);
        vr[i] = *reinterpret_cast<const u32x4*>(vb + g * a.v_rs + ch * 8);
      }
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
      if ((i + 1) * NT <= CHUNKS || c < CHUNKS) {
        *reinterpret_cast<u32x4*>(&k_s[buf][k_off<DH>(row, ch)]) = kr[i];
        *reinterpret_cast<u32x4*>(&v_s[buf][v_off<DH>(row, ch)]) = vr[i];
      }
    }
  };

  f32x16 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // l: this lane's 32 keys of every tile; the two halves are added at the end

  // transposed-read addressing: lane 4 qq + p of a 16-lane group supplies row qq, columns 4 p .. 4 p + 3 of the group's 4 x 16 block
  const int tr_q = (lane & 15) >> 2, tr_p = lane & 3, tr_g = (lane >> 4) & 1;

  stage_load(0);
  stage_write(0);
  // Q has arrived before the loop starts (a wait for it inside the loop would sit behind the loads the loop has just issued)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1, t0 = t * kKV;
    const bool more = t + 1 < nt;
    if (more) stage_load(t0 + kKV);

    if (wave_on) {
      // ---- S^T = K Q^T: s[kb2][e] = key t0 + 32 kb2 + (e & 3) + 8 (e >> 2) + 4 hh, query row r ----
      f32x16 s[2];
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kb2][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bool tail = 16 * ks + 16 > DH;  // the k-step whose upper half is padding: both halves address the last chunk ...
          const int ch = tail ? 2 * ks : 2 * ks + hh;
          u32x4 w = *reinterpret_cast<const u32x4*>(&k_s[buf][k_off<DH>(32 * kb2 + r, ch)]);
          if (tail && hh) w = u32x4{0u, 0u, 0u, 0u};  // ... and the upper half takes zeros instead
          s[kb2] = DT::mfma32(__builtin_bit_cast(vec8, w), qf[ks], s[kb2]);
        }
      }
      // ---- online softmax (base 2: the logits are scaled by scale * log2 e) ----
      const bool need_mask = t0 + kKV - 1 > lim;
      float mx = -INFINITY;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[kb2][e] * a.scale_log2e;
          if (need_mask) {
            const int key = t0 + 32 * kb2 + (e & 3) + 8 * (e >> 2) + 4 * hh;
            x = key <= lim ? x : -INFINITY;
          }
          s[kb2][e] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);  // finite from the first tile on: key 0 exists
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      vec8 pf[4];
      float sum = 0.f;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const elem pt = (elem)__builtin_amdgcn_exp2f(s[kb2][e] - m_new);  // the ONE rounding of a weight
          pf[2 * kb2 + (e >> 3)][e & 7] = pt;
          sum += (float)pt;
        }
      l_run = l_run * alpha + sum;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
      // ---- O^T += V^T P^T: k-step s2 = keys 16 s2 + 8 (j >> 2) + 4 hh + (j & 3), j = operand element ----
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const int row = 16 * s2 + 4 * hh + tr_q, ch = 4 * db + 2 * tr_g + (tr_p >> 1);  // ch < VP / 8: inside the row's pitch
          const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) i16x4*)(&v_s[buf][v_off<DH>(row, ch) + 4 * (tr_p & 1)]));
          const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) i16x4*)(&v_s[buf][v_off<DH>(row + 8, ch) + 4 * (tr_p & 1)]));
          const i16x8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = DT::mfma32(__builtin_bit_cast(vec8, va), pf[s2], o[db]);
        }
      }
    }

    if (more) stage_write(buf ^ 1);  // the other buffer: its readers finished before the barrier that ended tile t - 1
    __syncthreads();
  }

  // ---- O / l, rounded to T once; lane (r, hh) holds O[row r][32 db + 8 g4 + 4 hh + 0..3] in o[db][4 g4 + 0..3] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (wq0 + r < lenq) {
    const float inv = 1.0f / l_tot;
    uint16_t* op = a.out + ((orow + qi) * a.H + h) * DH + 4 * hh;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        if (32 * db + 8 * g4 >= DH) continue;  // columns that do not exist
        const u32 w0 = (u32)DT::from_float(o[db][4 * g4] * inv) | ((u32)DT::from_float(o[db][4 * g4 + 1] * inv) << 16);
        const u32 w1 = (u32)DT::from_float(o[db][4 * g4 + 2] * inv) | ((u32)DT::from_float(o[db][4 * g4 + 3] * inv) << 16);
        *reinterpret_cast<u32x2*>(op + 32 * db + 8 * g4) = u32x2{w0, w1};
      }
  }
}

template <typename DT, int DH>
void launch_nw(const TowerArgs& a, int nw, int blocks, hipStream_t st) {
  switch (nw) {
    case 4: hipLaunchKernelGGL((attn_tower_kernel<DT, DH, 4>), dim3(blocks), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attn_tower_kernel<DT, DH, 2>), dim3(blocks), dim3(128), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_tower_kernel<DT, DH, 1>), dim3(blocks), dim3(64), 0, st, a); break;
  }
}

}  // namespace

// Host plan: the q tile (rows per block) of a launch of nseq sequences of at most max_seqlen rows.  The rule is the prefill kernel's
// for Dh = 64: 128 rows (4 waves), 64 rows while 128-row tiles leave fewer than two blocks per CU -- a tower at B = 1 is 16 heads x
// 6 .. 9 tiles of 128 rows, far under 256 CUs.  32-row tiles exist behind the tower_rows knob for the measurement that decides
// (DESIGN.md "Tower attention").  Depends on host arguments only.
int attn_varlen_plan(int nseq, int nheads, int head_dim, int max_seqlen, int* q_tile_rows, int* blocks) {
  (void)head_dim;
  const long long sh = (long long)nseq * nheads;
  auto nblocks = [&](int rows) { return sh * ((max_seqlen + rows - 1) / rows); };
  int rows = nblocks(128) < 2 * kCUs ? 64 : 128;
  if (g_force_rows) rows = g_force_rows;
  *q_tile_rows = rows;
  *blocks = (int)nblocks(rows);
  return 0;
}

int attn_tower_tune_set(const char* key, int value) {
  if (strcmp(key, "tower_rows") != 0 || (value != 0 && value != 32 && value != 64 && value != 128)) return -1;
  g_force_rows = value;
  return 0;
}

int launch_attn_tower(const void* q, const void* k, const void* v, void* out, const int* cu_seqlens, int nseq, int Sq, int Sk,
                      long long total_rows, int H, int Hkv, int Dh, long long q_bs, long long q_rs, long long k_bs, long long k_rs,
                      long long v_bs, long long v_rs, float scale, int dtype, hipStream_t st) {
  TowerArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k;
  a.v = (const uint16_t*)v;
  a.out = (uint16_t*)out;
  a.cu = cu_seqlens;
  a.q_bs = q_bs;
  a.q_rs = q_rs;
  a.k_bs = k_bs;
  a.k_rs = k_rs;
  a.v_bs = v_bs;
  a.v_rs = v_rs;
  a.total_rows = total_rows;
  a.nseq = nseq;
  a.Sq = Sq;
  a.Sk = Sk;
  a.H = H;
  a.G = H / Hkv;
  a.scale_log2e = scale * 1.4426950408889634f;
  int rows = 0, blocks = 0;
  attn_varlen_plan(nseq, H, Dh, Sq, &rows, &blocks);
  const int nw = rows / kMfmaRows;
  if (dtype == 0) {
    if (Dh == 72) launch_nw<F16, 72>(a, nw, blocks, st);
    else launch_nw<F16, 64>(a, nw, blocks, st);
  } else {
    if (Dh == 72) launch_nw<BF16, 72>(a, nw, blocks, st);
    else launch_nw<BF16, 64>(a, nw, blocks, st);
  }
  return 0;
}

}  // namespace awq
