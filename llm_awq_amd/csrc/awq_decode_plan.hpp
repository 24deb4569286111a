// The launch plan of the W4 decode entry (1 .. 8 rows of x against an [n, k] matrix): which kernel serves the call, in how many row chunks, and the
// configuration of every chunk.  Pure host code: no HIP, no globals, integers only.  launch_gemv_dma (awq_gemv_dma.hip) walks the plan,
// launch_skinny_decode (awq_skinny_cdna4.hip) dispatches on skinny_decode_chunk, and the host queries awq_w4a16_decode_cdna4_plan /
// awq_w4a16_decode_cdna4_plan_detail read the same plan, so what is asked is what is launched.  tests/decode_plan_cases.py pins it row by row.
//
// Two integer classes carry every rule:
//   slabs   16-row slabs of ONE launch (n / 16; n / 32 for the stacked epilogue 1, whose blocks hold a gate and an up slab), against the CU
//           count `cus` (256 on the whole MI355X): per_cu = 1 / 2 / 3 / 4 for <= 1, <= 2, <= 3, more slabs per CU; half = at least 1.5 per CU
//   nit     k-steps of 128 (k / 128): < 32, 32 .. 63, 64 .. 95, >= 96
#pragma once

namespace awq {

enum DecodeKernel { kDecodeStreaming = 0, kDecodeSkinny = 1 };
// block shapes of the skinny kernel for one 16-row x block: waves x slabs per block
enum SkinnyShape { kSkinnyPlain8x1 = 0, kSkinnyDeep16x1 = 1, kSkinnyWide8x2 = 2, kSkinnyWide8x7 = 3 };

// What awq_tune_set can force (tests, tools/decode_cfg_sweep.py, tools/gemvd_xprobe.py); the defaults are the shipped plan.
struct DecodeKnobs {
  int skinny_from = 0;  // decode_skinny_from: 0 = by shape (skinny_takes), 1 .. 8 = the skinny kernel from that row count, 9 = never
  int waves = 0;        // gemvd_waves: waves per streaming block (0 = by shape)
  int d = 0;            // gemvd_d: ring depth of the streaming kernel (0 = by shape)
  int want = 0;         // gemvd_want: co-resident blocks per CU the LDS budget is sized for (0 = by shape)
  int il = 2;           // gemvd_il: 0 = contiguous K ranges per wave, 1 = interleaved, 2 = by configuration (streaming_chunk)
  int probe = 0;        // gemvd_probe: timing probes of the streaming kernel, handed to the kernel as they are; no rule reads them
};

struct DecodeChunk {
  int rows, kernel;                 // DecodeKernel
  int waves, tx, d, smem_bytes;     // streaming: waves per block, k-steps per wave, ring depth, dynamic LDS
  bool interleaved, one_row_form;   // streaming: K split interleaved over the waves; the straight-line one-row kernel runs
  int shape, x_pieces;              // skinny: SkinnyShape; 4-row x pieces staged per k-step (1 .. 4)
};
struct DecodePlan {
  bool in_range;  // the arguments are a decode call's (1 .. 8 rows, whole slabs, whole k-steps)
  bool served;    // ... and every row found a launch (else: not even one row's staging fits LDS)
  int nchunks;
  DecodeChunk chunk[8];  // in launch order; every chunk is one pass over the weights
};

inline int slabs_per_cu_class(int slabs, int cus) { return slabs <= cus ? 1 : (slabs <= 2 * cus ? 2 : (slabs <= 3 * cus ? 3 : 4)); }

// ---- the skinny kernel's chunk (also its 9 .. 16-row callers: x_pieces 3 / 4) --------------------------------------------------------
// seven slabs per block make ONE round of one block per CU (Llama-3-8B gate/up: 1792 slabs -> 256 blocks): the x slices are read by that many
// blocks instead of 1.75 - 3.5 times as many (profiles/r05_skinny_splitk.txt)
inline bool seven_slab_round(int slabs, int cus) {
  const int groups = (slabs + 6) / 7;
  return groups <= cus + 16 && groups >= cus * 9 / 10;
}
inline DecodeChunk skinny_decode_chunk(int m, int slabs, int nit, int cus) {
  DecodeChunk c = {m, kDecodeSkinny, 0, 0, 0, 0, false, false, kSkinnyPlain8x1, 4};
  if (slabs >= 1024) c.shape = seven_slab_round(slabs, cus) ? kSkinnyWide8x7 : kSkinnyWide8x2;  // wide: -2 % on the 7-row decode leg, -4 % at 16 rows with seven slabs
  else if (nit >= 96) c.shape = kSkinnyDeep16x1;                                // 16 waves split a long K (down_proj: 112 steps)
  else if (m <= 8 && nit >= 32 && slabs <= cus) c.shape = kSkinnyDeep16x1;      // ... and at most one slab per CU from 32 steps: o_proj -2 ... -3.5 %, Llama-2-7B down_proj (86 steps) 8.5 -> 6.6 us; at 12 / 16 rows 0.6-0.9 % slower
  // only the 4-row pieces of the x block that hold rows are staged (profiles/r06_decode_cfg.txt (8): 7-row leg 1.13 -> 1.09 ms)
  c.x_pieces = m <= 4 ? 1 : (m <= 8 ? 2 : (m <= 12 ? 3 : 4));
  return c;
}

// ---- which kernel ---------------------------------------------------------------------------------------------------------------
// The streaming kernel stages m x K x 2 bytes of x per SLAB by LDS-DMA -- at m = 4 as many bytes as the slab's weights -- and the staging
// region crowds the ring out of LDS or forces row chunks that re-stream the weights.  The skinny kernel (x through registers, shared by a
// block's slabs, one weight pass) costs the same for every m <= 8 (profiles/r03_decode_m_sweep.txt, profiles/r06_decode_cfg.txt).
// First matching row decides.
inline bool skinny_takes(int m, int slabs, int nit, int epi, int cus, const DecodeKnobs& kn) {
  const int per_cu = slabs_per_cu_class(slabs, cus);
  const bool half = 2 * slabs >= 3 * cus;             // at least 1.5 slabs per CU
  const long long xb = (long long)m * nit * 256;      // bytes of x ONE streaming block stages
  if (epi == 1) return false;                         // the stacked [gate; up] form has no skinny epilogue
  if (kn.skinny_from) return m >= kn.skinny_from;     // forced
  if (per_cu == 4 && nit >= 32 && nit < 96) return (long long)m * nit >= (nit >= 64 ? 128 : 150);  // fused gate/up pair, three co-resident eight-wave blocks stage 3 xb: K = 4096 from five rows (15.97 vs 16.99 us), K = 8192 (Llama-3-70B) from two (three rows: 47.5 vs 51.0 us)
  if (slabs < 1024 && half) return true;              // from ONE row: qkv 5.0 vs 5.35 us; Llama-3-70B qkv / o / down -8 ... -9 % (its decode layer 93.9 -> 91.2-92.7 us); profiles/r06_decode_cfg.txt (9), (11)
  if (slabs < 1024 && m >= 2 && nit >= 96) return true;                  // long K, 16-wave skinny shape: down_proj 7.85 vs 9.2 us at four rows; ONE row stays (isolated -6 % does not show in the token's chain: 0.9766-0.9801 vs 0.9704-0.9772 ms per step)
  if (slabs < 1024 && m >= 2 && per_cu == 1 && nit >= 32) return true;   // one slab per CU, 16-wave skinny shape: o_proj 4.15-4.44 vs 4.26-4.6 us at 2 .. 7 rows; at one row the deeper ring wins (o_proj 4.2 vs 4.5, Llama-2-7B down_proj 7.8 vs 9.1)
  // the staging rule: from five rows -- or from the row count at which ONE block's staging reaches 100 KiB (Llama-3-70B down_proj, 56 KiB per row: 39 / 64 / 75 us
  // streaming at 2 / 3 / 4 rows against 31.5 - 35) -- where the co-resident blocks stage 128 KiB per CU (profiles/r06_decode_cfg.txt (6))
  return (m >= 5 || xb >= 100 * 1024) && xb * per_cu >= 128 * 1024;
}

// ---- the streaming kernel's configuration ------------------------------------------------------------------------------------------------
inline long long streaming_smem(int waves, int d, int ns, int tx, int m) {
  const long long txp = (tx + 3) & ~3;
  return waves * ((long long)d * ns * 1024 + ns * txp * 64 + m * (txp * 256 + 16));
}
// the one-row kernel's compiled k-steps per wave for (epilogue, waves, ring depth); 0 = that instantiation has no one-row form.  (launch_dma_cfg
// keeps the mapping beside its templates and asserts that it is this one.)
constexpr int one_row_tx(int epi, int waves, int d) {
  return epi == 1 ? 0 : ((waves == 8 && (d == 2 || d == 4)) ? 4 : ((waves == 16 && d == 1) ? 7 : 0));
}
// K split and ring depth: as many tiles in flight per CU as LDS allows over the blocks that share it (tools/gemvd_sweep.py, profiles/r02_gemvd_*).
// false = m rows do not fit one launch.
inline bool streaming_chunk(int m, int slabs, int nit, int epi, int cus, const DecodeKnobs& kn, DecodeChunk& c) {
  const int ns = epi == 1 ? 2 : 1, per_cu = slabs_per_cu_class(slabs, cus);
  // waves per block, by class
  bool wide8 = per_cu == 4 && nit >= 32 && nit < 96;  // fused gate/up pair at K = 4096 / 8192: eight-wave blocks whose ring holds a wave's whole K range, gate/up -7 ... -13 % at 2 .. 4 rows, -2.5 % at one (profiles/r06_decode_cfg.txt (3))
  int waves = nit >= 96 ? 16                          // long K (down_proj): 16 waves x 1 .. 2 tiles
              : (per_cu == 4 && !wide8 ? 4            // many slabs per CU against a short K (tensor-parallel shards): four waves, deep ring, four ring-7 blocks per CU (+0.6 % decode tok/s, profiles/r03_gemvps.txt)
                                       : 8);          // 8 waves x 2 .. 4 tiles
  if (kn.waves) waves = kn.waves;
  while (waves > 4 && waves > nit) waves >>= 1;       // waves beyond the step count would idle
  while (waves > 4 && streaming_smem(waves, 1, ns, (nit + waves - 1) / waves, m) > 150 * 1024) waves >>= 1;  // x staging (m k 2 bytes per block whatever the wave count) crowds out the ring: fewer, longer waves
  if (waves != 8) wide8 = false;
  const int tx = (nit + waves - 1) / waves;
  // co-resident blocks per CU the LDS budget is sized for
  int want = wide8 ? (tx > 4 ? 2 : 3)                 // three eight-wave blocks per CU, two when a wave's K range is eight tiles (K = 8192)
                   : per_cu;
  if (kn.want) want = kn.want;
  // ring depth
  int d = tx < 8 ? tx : 8;
  if (kn.d) d = kn.d < tx ? kn.d : tx;
  else if (waves == 16) d = 1;                                            // 16 waves already keep 16+ KiB per CU in flight (8.2 vs 8.7 us at d = 2)
  else if (waves == 8 && d > 2 && !wide8 && (m < 3 || per_cu == 1)) d = 2;  // two blocks per CU from three rows: a ring of four, qkv -2 %; o_proj keeps two
  while (d > 1 && streaming_smem(waves, d, ns, tx, m) * want > 156 * 1024) --d;  // the co-resident blocks fit 160 KiB
  // compiled ring depths: 1, 2, 4, 8 (7 with 16 waves: K = 14336)
  if (d == 3) d = 2;
  if (d == 5 || d == 6 || (d == 7 && waves == 8)) d = 4;
  if (d == 8 && waves == 16) d = 7;
  const long long smem = streaming_smem(waves, d, ns, tx, m);
  if (smem > 160 * 1024 || tx < d) return false;
  c = {m, kDecodeStreaming, waves, tx, d, (int)smem, false, false, 0, 0};
  // interleaved K split: eight-wave blocks whose ring is shallower than a wave's K range (qkv -1.2 %, o_proj -3.2 % at one row; 16-wave down_proj no different: profiles/r06_decode_cfg.txt (7))
  c.interleaved = kn.il == 1 || (kn.il == 2 && d < tx && waves == 8);
  // one row against the K ranges of the decoded token (K = 4096 over eight waves, K = 14336 over sixteen): the straight-line, pipelined kernel
  const int txc = one_row_tx(epi, waves, d);
  c.one_row_form = txc != 0 && m == 1 && tx == txc && nit == waves * txc;
  return true;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------
// The streaming kernel stages every row's x slice in LDS up front: when the rows do not fit one launch they are served in chunks of as many
// rows as do fit, each chunk a pass over the weights (the reference's GEMV loops over the batch inside one pass, gemv_cuda.cu:187-208; here
// the LDS budget decides).  Every chunk asks skinny_takes for its own row count.
inline DecodePlan decode_plan(int m, int n, int k, int epi, int cus, const DecodeKnobs& kn) {
  DecodePlan p = {};
  const int unit = epi == 1 ? 32 : 16;
  if (m < 1 || m > 8 || k < 128 || (k % 128) != 0 || epi < 0 || epi > 2 || n < unit || (n % unit) != 0 || cus < 1) return p;
  p.in_range = true;
  const int slabs = n / unit, nit = k / 128;
  for (int left = m; left > 0;) {
    DecodeChunk c = {};
    int rows = left;
    if (skinny_takes(left, slabs, nit, epi, cus, kn)) c = skinny_decode_chunk(left, slabs, nit, cus);
    else {
      while (rows > 1 && !streaming_chunk(rows, slabs, nit, epi, cus, kn, c)) --rows;
      if (!streaming_chunk(rows, slabs, nit, epi, cus, kn, c)) return DecodePlan{true, false, 0, {}};
      if (rows < left && skinny_takes(rows, slabs, nit, epi, cus, kn)) c = skinny_decode_chunk(rows, slabs, nit, cus);
    }
    for (; left >= rows; left -= rows) p.chunk[p.nchunks++] = c;
  }
  p.served = true;
  return p;
}

}  // namespace awq
