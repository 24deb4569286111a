// The route of the dense W4 cdna4 linear entries (awq_capi.hip): which ONE launcher serves a call, with which scale format, epilogue, bias handling and
// workspace.  Pure host code: no HIP, no globals, integers and bools only.  The entries switch on linear_route, every launcher's guard is the predicate
// of its leaf below (route and launcher agree by construction), and the host query awq_w4a16_linear_route_cdna4 reads the same route, so what is asked
// is what is launched.  tests/linear_route_cases.py pins it row by row; tests/linear_route_check.cpp holds the invariants over the whole grid.
// A leaf's inner plan stays with its launcher: decode_plan (awq_decode_plan.hpp), the tile plan and the pair plan (awq_gemm_plan.hip), the mid-M kernel's
// K parts and passes, the skinny block shapes, launch_gemm's own choice among its GEMV, the tiles and the generic 128 / 256 kernels.
#pragma once

#include "awq_decode_plan.hpp"

namespace awq {

enum LinearEntry { kEntryForward = 0, kEntryForwardSzh = 1, kEntryGemm = 2, kEntryGemv = 3, kEntryGateUp = 4, kEntryPartial = 5 };
// 0 = no launcher serves the call (the entry answers AWQ_ERR_SHAPE)
enum LinearLeaf { kLeafNone = 0, kLeafDecode = 1, kLeafGemvRing = 2, kLeafMidm = 3, kLeafSkinny16 = 4, kLeafSkinny = 5, kLeafSkinnyGateUp = 6, kLeafTiles = 7, kLeafGeneric = 8 };
enum LinearEpilogue { kEpiPlain = 0, kEpiPair = 1, kEpiPartial = 2 };  // [m, n] (+ bias); silu(gate) * up of an interleaved pair, [m, n / 2]; unrounded fp32 [m, n]
enum LinearBias { kBiasNone = 0, kBiasFused = 1, kBiasAdd = 2 };       // fused into the leaf's epilogue; a separate launch_bias_add behind it
// the facts about a call's pointers that the routes test.  kHasSzHalf: sz_half present AND 16-byte aligned (a misaligned one silently takes the sz_packed path);
// kWsTiles: the workspace is 64-byte aligned and at least gemm_cdna4_v3_workspace_bytes (read by the gate/up entry only)
enum LinearFlags { kHasSzPacked = 1, kHasSzHalf = 2, kHasBias = 4, kHasWs = 8, kWsTiles = 16 };

// A snapshot of every knob a route reads (awq_tune_set: tests, sweeps); the defaults are the shipped values.
struct LinearKnobs {
  int gemm_variant = 0;     // 0 = auto, 1 / 2 = force the generic 128 x 128 / 256 x 256 kernel, 3 .. 5 = force the tile kernels (launch_gemm)
  int midm = 1;             // 0 = off (the skinny / masked-tile kernels of rounds 1-5 serve 9 .. 255 rows)
  int midm_min = 65, midm_max = 128;  // the row counts the forward entries hand to the mid-M kernel (tests: 9 .. 255); the defaults = the by-shape rules of midm_takes
  int midm_waves = 0, midm_ns = 0, midm_ks = 0;  // force a block shape / part count (experiments, tests)
  int gemm_small_m = 1;     // 0 = the prefill GEMM only takes m >= 256 (see tiles_take); 2 = every m the skinny kernel would take
  int gemm_v4 = 1;          // 0 = the tile kernels take no m below 256 (the skinny kernel serves 9 .. 255 rows); the loop it once selected is gone
  int gemv_dma = 1;         // 1 = the LDS-DMA streaming kernel (awq_gemv_dma.hip) serves W4 decode; 0 = the register-ring kernel
  int mlp_skinny_max = 64;  // row counts up to this go to the skinny kernel's fused gate/up epilogue (8 = never)
  int skinny16_szh = 1;     // 0 = 9 .. 16 rows on the T-typed sz_packed form as in rounds 1 - 5
  DecodeKnobs decode;       // the decode leaf's own knobs (awq_decode_plan.hpp)
};

struct LinearRoute {
  int leaf, szfmt, epilogue, bias;  // LinearLeaf; 0 sz_packed / 1 sz_half; LinearEpilogue; LinearBias
  bool ws, bias_align16;            // the caller's workspace is handed on; the leaf reads bias as 16-byte vectors (a misaligned one: AWQ_ERR_ALIGN)
  int row;                          // the row of the entry's table that decided (1-based, in the order written below)
};

// ---- the mid-M kernel (awq_midm_cdna4.hip) ---------------------------------------------------------------------------------------------------
// LDS of a block: DX x stages of 16 cb rows (padded to whole rounds of pieces), per wave a ring of DX + 1 slots of ns (tile + scale piece)
constexpr int midm_xstage(int cb, int waves) { return (4 * cb + waves - 1) / waves * waves * 1024; }
constexpr int midm_lds(int cb, int waves, int ns, int dx) { return dx * midm_xstage(cb, waves) + waves * ns * (dx + 1) * 1280; }
// ring depth: the DX - 1 groups in flight are what the CU has outstanding -- as deep as ~150 KiB of LDS allows, 3 .. 8 stages
constexpr int midm_dx(int cb, int waves, int ns) {
  int dx = 8;
  while (dx > 3 && midm_lds(cb, waves, ns, dx) > 150 * 1024) --dx;
  return dx;
}
inline int midm_ks_for(int groups, int nit, int cus) {
  int ks = 1;
  while (groups * ks * 2 <= cus && nit / (ks * 2) >= 2) ks *= 2;
  return ks;
}
// the rows of a call are served in passes of at most 128 (129 .. 255: two equal passes, each re-streaming the weights)
inline void midm_passes(int m, int& chunks, int& rows) {
  chunks = (m + 127) / 128;
  rows = (m + chunks - 1) / chunks;
}
// Block shape for a pass of m <= 128 rows (profiles/r06_midm_sweep.txt).  One slab per wave; eight waves (two per SIMD) unless the K split that fills the
// chip would then leave a block fewer than eight k-steps (o_proj: 4096 x 4096) -- four waves halve the slab group instead.  false = no compiled block fits.
inline bool midm_shape(int m, int n, int k, int cus, const LinearKnobs& kn, int& waves, int& ns, int& cb) {
  const int nslab = n / 16, nit = k / 128;
  cb = (m + 15) / 16;
  ns = kn.midm_ns ? kn.midm_ns : 1;
  waves = kn.midm_waves ? kn.midm_waves : (nit / midm_ks_for((nslab + 8 * ns - 1) / (8 * ns), nit, cus) >= 8 ? 8 : 4);
  return cb >= 1 && cb <= 8 && ((waves == 8 && ns == 1) || (waves == 4 && (ns == 1 || ns == 2))) && midm_lds(cb, waves, ns, midm_dx(cb, waves, ns)) <= 160 * 1024;
}
// Which calls the forward entries hand to the mid-M kernel.  Measured against the round-5 kernels on the Llama-3-8B shapes (profiles/r06_midm_sweep.txt) and, third session,
// on the Llama-3-70B / Llama-2-7B shapes and with the true round-5 baseline above 128 rows (profiles/r06_midm_routing.txt):
//   * 65 .. 128 rows always (one pass: 0.60 - 0.94 x the time of the skinny kernel's two chunks / the masked 256-row tile on every shape measured);
//   * 129 .. 192 rows NOT any more: two passes, each re-streaming the weights, lose to the masked tile + split-K wherever K is long (down_proj 14336 -> 4096: 1.22 - 1.32 x,
//     Llama-3-70B qkv / o: 1.2 - 1.36 x) and tie on the K = 4096 projections (0.96 - 1.13 x) -- the second session's figure for down_proj came from a baseline run with a
//     scratch sized for another plan;
//   * below 65 rows the skinny kernel (x through registers, up to seven slabs per block, no barrier) is as fast or faster on the Llama-3-8B shapes, but its block shapes leave
//     other shapes under-filled -- this kernel's K split across blocks takes: 17 .. 32 rows against n >= 16384 (0.81 - 0.88 x); every row count against a very long K and a
//     narrow n (Llama-3-70B down_proj, 28672 -> 8192: 0.57 - 0.87 x at 16 .. 64 rows); 33 .. 64 rows against n = 8192-class matrices (the skinny kernel's four-slab blocks fill
//     half the chip: Llama-3-70B o_proj 0.76 x); 49 .. 64 rows against wide pairs whose slab count is not one round of seven-slab blocks (gate/up of Llama-3-70B / Llama-2-7B: 0.84 - 0.89 x).
inline bool midm_small_takes(int m, int n, int k, int cus) {
  const int nslab = n / 16, nit = k / 128;
  if (m >= 17 && m <= 32 && n >= 16384) return true;
  if (nit >= 192 && nslab <= 512) return true;
  if (m >= 33 && nslab >= 512 && nslab < 640) return true;
  if (m >= 49 && n >= 16384 && !seven_slab_round(nslab, cus)) return true;
  return false;
}
inline bool midm_takes(int m, int n, int k, int cus, const LinearKnobs& kn) {
  if (!kn.midm || m < 9 || m > 255 || (n % 16) != 0 || (k % 128) != 0 || k < 256) return false;
  if (kn.midm_min == 65 && kn.midm_max == 128) {  // the product's rules
    if (m > 128 || (m < 65 && !midm_small_takes(m, n, k, cus))) return false;
  } else {  // knobs (tests, sweeps): a plain row range; 129 .. 192 rows against a wide n stay on the tiles as in the first two sessions
    if (m < kn.midm_min || m > kn.midm_max) return false;
    if (m > 128 && n >= 16384 && kn.midm_max <= 192) return false;
  }
  if ((unsigned long long)n * (unsigned long long)k / 2 >= (1ull << 31) || (unsigned long long)m * (unsigned long long)k * 2 >= (1ull << 31)) return false;
  int chunks, rows, waves, ns, cb;
  midm_passes(m, chunks, rows);
  return midm_shape(rows, n, k, cus, kn, waves, ns, cb);
}
// the guard of launch_midm_cdna4: epi 0 (bias fused; f32out: no bias) or 2 (pair, whole gate AND up slabs, no bias, no fp32 form)
inline bool midm_serves(int m, int n, int k, int epi, bool bias, bool f32out, int bits, int cus, const LinearKnobs& kn) {
  return bits == 4 && midm_takes(m, n, k, cus, kn) && (epi == 0 || epi == 2) && !(epi == 2 && ((n % 32) != 0 || bias || f32out)) && !(f32out && bias);
}

// ---- the skinny kernel (awq_skinny_cdna4.hip) ------------------------------------------------------------------------------------------------
// the guard of launch_skinny_cdna4: row chunks of <= 64, each re-streaming the weights, which still beats the 128 x 128 kernel's long serial K loop
// (profiles/r01_skinny_sweep.txt) except above 128 rows against a very wide n
inline bool skinny_serves(int m, int n, int k, bool bias, bool f32out) {
  return m >= 1 && m <= 255 && (n % 16) == 0 && (k % 128) == 0 && (unsigned long long)m * (unsigned long long)k < (1ull << 31) && !(f32out && bias) && !(m > 128 && n >= 16384);
}
// the guard of launch_skinny_gate_up: 9 .. 64 rows of an interleaved pair, whole gate AND up slabs
inline bool skinny_gate_up_serves(int m, int n2, int k) {
  return m >= 9 && m <= 64 && (n2 % 32) == 0 && (k % 128) == 0 && (unsigned long long)m * (unsigned long long)k < (1ull << 31);
}
// the guard of launch_skinny_decode: one 16-row x block, epi 0 (bias fused) or 2 (pair), fp32 only plain and without bias
inline bool skinny16_serves(int m, int n, int k, int epi, bool bias, bool f32out) {
  return m >= 1 && m <= 16 && (n % 16) == 0 && (k % 128) == 0 && (epi == 0 || epi == 2) && !(epi == 2 && bias) && !(f32out && (epi || bias));
}

// ---- the decode kernels ----------------------------------------------------------------------------------------------------------------------
// the guard of launch_gemv_dma and the plan it walks: fp32 sums only plain and without bias, and the decode plan serves every row (what launch_skinny_decode
// does not serve stays on the streaming kernel)
inline DecodePlan decode_leaf_plan(int m, int n, int k, int epi, bool has_sz, bool bias, bool f32out, int cus, const LinearKnobs& kn) {
  if (f32out && (epi != 0 || bias)) return DecodePlan{};
  DecodeKnobs dk = kn.decode;
  if (!has_sz || (epi == 2 && bias)) dk.skinny_from = 9;
  return decode_plan(m, n, k, epi, cus, dk);
}
inline bool decode_serves(int m, int n, int k, int epi, bool has_sz, bool bias, bool f32out, int cus, const LinearKnobs& kn) {
  return decode_leaf_plan(m, n, k, epi, has_sz, bias, f32out, cus, kn).served;
}
// the register-ring GEMV (launch_gemv_cdna4 behind its streaming attempt), W4: plain or the stacked [gate; up] form; every configuration its default
// knobs and the suite's forced ones pick is compiled
inline bool gemv_ring_serves(int m, int n, int k, int epi) { return m >= 1 && m <= 8 && (epi == 0 || epi == 1) && (n % (epi == 1 ? 32 : 16)) == 0 && (k % 128) == 0; }
// launch_gemv_cdna4 for a plain W4 call (a bias changes nothing): the streaming kernel, else the register ring
inline int gemv_leaf(int m, int n, int k, int cus, const LinearKnobs& kn) {
  if (kn.gemv_dma && decode_serves(m, n, k, 0, true, false, false, cus, kn)) return kLeafDecode;
  return gemv_ring_serves(m, n, k, 0) ? kLeafGemvRing : kLeafNone;
}

// ---- the tile kernels (awq_gemm_plan.hip) ----------------------------------------------------------------------------------------------------
// Which m the prefill GEMM takes.  m >= 256 always; below that the narrow-tile kernel runs ONE row tile whose missing rows are
// not stored, at the cost of a 256-row tile whatever m is, while the skinny kernel (awq_skinny_cdna4.hip) re-streams and
// re-dequantises the weights once per 64 rows: the crossover measured on the Llama shapes (profiles/r01_small_m_sweep.txt) sits
// at m ~ 75 for K >= 8192 and ~150 for K = 4096, which m * K >= 0.6 M approximates; at m = 255 the GEMM is 1.6 - 3.1x faster.
inline bool tiles_take(int m, int k, const LinearKnobs& kn) {
  if (m >= 256) return true;
  if (kn.gemm_small_m == 2) return kn.gemm_v4 && m > 8;  // experiments: every m the skinny kernel would take
  return kn.gemm_small_m && kn.gemm_v4 && m >= 72 && (long long)m * k >= 600000;
}
// the guard of launch_gemm_cdna4_v3 (w3c tiles and the fused epilogues have no skinny kernel behind them: the masked single-row-tile path serves every m > 8)
inline bool tiles_serve(int m, int n, int k, int bits, int epi, bool has_szp, const LinearKnobs& kn) {
  return has_szp && (tiles_take(m, k, kn) || ((bits == 3 || epi) && m > 8)) && (n % 16) == 0 && (k % 128) == 0 && (unsigned long long)m * (unsigned long long)k < (1ull << 31);
}

// ---- the route -------------------------------------------------------------------------------------------------------------------------------
// The arguments are the entry's own, already checked by it (check_common and whole 16-row slabs; the gate/up and partial entries: their own list).
// Every entry is an ordered list of rows: the first matching row decides.
inline LinearRoute linear_route(int entry, int m, int n, int k, int flags, int cus, const LinearKnobs& kn) {
  const bool szp = flags & kHasSzPacked, with_szh = entry == kEntryForwardSzh || entry == kEntryGateUp || entry == kEntryPartial;
  const bool szh = with_szh && (flags & kHasSzHalf), bias = (entry == kEntryForward || entry == kEntryForwardSzh) && (flags & kHasBias);
  const bool ws = entry != kEntryGemv && entry != kEntryPartial && (flags & kHasWs), v0 = kn.gemm_variant == 0;
  const int fused = bias ? kBiasFused : kBiasNone, added = bias ? kBiasAdd : kBiasNone;
  const int gemv = szp && m <= 8 && entry < kEntryGateUp ? gemv_leaf(m, n, k, cus, kn) : kLeafNone;  // the <= 8-row GEMV rows of the first four entries
  int row = 0;
#define AWQ_ROW(cond_, ...) \
  if (++row && (cond_)) return LinearRoute{__VA_ARGS__, row};
  if (entry == kEntryGateUp) {  // out is [m, n / 2]: the [m, n] intermediate of the reference's two GEMMs + F.silu + multiply never exists
    if (!szp) return LinearRoute{};
    // decode: one streaming launch, rows r and r + 8 of a slab paired in the epilogue
    AWQ_ROW(m <= 8, decode_serves(m, n, k, 2, true, false, false, cus, kn) ? kLeafDecode : kLeafNone, szh, kEpiPair, kBiasNone, false, false)
    // 9 .. 255 rows: the mid-M kernel (x tile shared by the block, waves split N, K split across blocks), pairing in its epilogue; it is offered the caller's workspace
    // as it came, before the tile kernels' test of it (like row szh-midm below it does not read gemm_variant)
    AWQ_ROW(midm_serves(m, n, k, 2, false, false, 4, cus, kn), kLeafMidm, szh, kEpiPair, kBiasNone, ws, false)
    // 9 .. 16 rows with the layer's sz_half side buffer: the skinny kernel's one-column-block shapes in the f16-mantissa dequant form (the batched-decode instantiations:
    // the same block shapes as launch_skinny_gate_up picks at <= 16 rows, ~10 VALU fewer per tile -- round 6, third session)
    AWQ_ROW(m <= 16 && szh && kn.skinny16_szh && skinny16_serves(m, n, k, 2, false, false), kLeafSkinny16, 1, kEpiPair, kBiasNone, false, false)
    // (knob midm = 0) 9 .. 64 rows: one weight pass on the skinny kernel (a 256-row tile masked down to m rows costs the same for every m: 46 vs 31 us at 64 rows on
    // Llama-3-8B's pair, profiles/r05_skinny_splitk.txt)
    AWQ_ROW(m <= kn.mlp_skinny_max && skinny_gate_up_serves(m, n, k), kLeafSkinnyGateUp, 0, kEpiPair, kBiasNone, false, false)
    // prefill / batched decode: the tile kernels with the SiLU * mul tail fused into their epilogue; a workspace that is misaligned or below their size is dropped
    // (optional scratch: without it the columns behind the full rounds run as 256 x 128 blocks)
    AWQ_ROW(tiles_serve(m, n, k, 4, 2, true, kn), kLeafTiles, szh, kEpiPair, kBiasNone, ws && (flags & kWsTiles), false)
    return LinearRoute{};
  }
  if (entry == kEntryPartial) {  // tensor-parallel row split: the K shard's fp32 partial, no bias, no workspace
    if (!szp) return LinearRoute{};
    // decode: the streaming kernel, f16-mantissa dequant when the layer allows it ...
    AWQ_ROW(m <= 8 && decode_serves(m, n, k, 0, true, false, true, cus, kn), kLeafDecode, szh, kEpiPartial, kBiasNone, false, false)
    // ... or the skinny kernel where the streaming kernel does not take the row count (sz_packed whatever the layer has)
    AWQ_ROW(m <= 8, skinny16_serves(m, n, k, 0, false, true) ? kLeafSkinny16 : kLeafNone, 0, kEpiPartial, kBiasNone, false, false)
    // row partial-midm: differs from kEntryForward's mid-M row -- no gemm_variant == 0 guard (unifying them changes behaviour: a later change)
    AWQ_ROW(midm_serves(m, n, k, 0, false, true, 4, cus, kn), kLeafMidm, szh, kEpiPartial, kBiasNone, false, false)
    AWQ_ROW(m < 256 && !tiles_take(m, k, kn) && skinny_serves(m, n, k, false, true), kLeafSkinny, 0, kEpiPartial, kBiasNone, false, false)
    AWQ_ROW(tiles_serve(m, n, k, 4, 3, true, kn), kLeafTiles, 0, kEpiPartial, kBiasNone, false, false)
    return LinearRoute{};
  }
  if (entry == kEntryGemv) {  // (its own GEMV for what the cdna4 kernels do not take: no sz_packed, 9 .. 16 rows)
    AWQ_ROW(gemv, gemv, 0, kEpiPlain, kBiasNone, false, false)
    AWQ_ROW(true, kLeafGeneric, 0, kEpiPlain, kBiasNone, false, false)
  }
  if (entry == kEntryForwardSzh && szh && szp) {  // the layer's sz_half side buffer: the f16-mantissa dequant form
    // row szh-midm, 9 .. 255 rows: differs from kEntryForward's mid-M row twice -- no gemm_variant == 0 guard, and it stands BEFORE the <= 8-row GEMV row, whose row
    // counts are disjoint from its own (unifying them changes behaviour: a later change)
    AWQ_ROW(midm_serves(m, n, k, 0, bias, false, 4, cus, kn), kLeafMidm, 1, kEpiPlain, fused, ws, true)
    // 9 .. 16 rows: the skinny kernel's one-column-block shapes
    AWQ_ROW(m >= 9 && m <= 16 && kn.skinny16_szh && v0 && skinny16_serves(m, n, k, 0, bias, false), kLeafSkinny16, 1, kEpiPlain, fused, false, true)
    // prefill: the tile kernels dequantise in the f16-mantissa form (every block width, the block pairs included)
    AWQ_ROW(m >= 256 && v0 && tiles_serve(m, n, k, 4, 0, true, kn), kLeafTiles, 1, kEpiPlain, fused, ws, true)
  } else if (entry == kEntryForwardSzh) row = 3;  // (the rows below keep their numbers)
  if (entry == kEntryForward || entry == kEntryForwardSzh) {
    // decode: bias fused into the GEMV epilogue
    AWQ_ROW(gemv, gemv, 0, kEpiPlain, fused, false, false)
    // 9 .. 255 rows: the mid-M kernel, bias fused
    AWQ_ROW(szp && v0 && midm_serves(m, n, k, 0, bias, false, 4, cus, kn), kLeafMidm, 0, kEpiPlain, fused, ws, true)
    // (knob midm = 0) short prompts / batched decode: skinny kernel, bias fused
    AWQ_ROW(m > 8 && m < 256 && szp && v0 && !tiles_take(m, k, kn) && skinny_serves(m, n, k, bias, false), kLeafSkinny, 0, kEpiPlain, fused, ws, false)
    // prefill: bias fused into the prefill GEMM epilogue (no second kernel)
    AWQ_ROW(bias && szp && v0 && tiles_take(m, k, kn) && tiles_serve(m, n, k, 4, 0, true, kn), kLeafTiles, 0, kEpiPlain, kBiasFused, ws, true)
  }
  // kEntryGemm, and what is left of the forward entries (the bias then by launch_bias_add)
  AWQ_ROW(szp && m > 8 && m < 256 && v0 && !tiles_take(m, k, kn) && skinny_serves(m, n, k, false, false), kLeafSkinny, 0, kEpiPlain, added, ws, false)
  AWQ_ROW(gemv, gemv, 0, kEpiPlain, added, false, false)
  // launch_gemm: its GEMV up to 16 rows, the tile kernels where they take the call, else the generic 128 x 128 / 256 x 256 kernels
  AWQ_ROW(true, kLeafGeneric, 0, kEpiPlain, added, ws, false)
#undef AWQ_ROW
  return LinearRoute{};
}

}  // namespace awq
