"""One soft-capped windowed mixed packed step (awq_attn_varq_softcap[_kv8], awq_attn_paged_varq_softcap[_kv8]; csrc/awq_softcap.hpp):
tests/attn_window_cases.py's `Step`, unchanged -- H 8 / Hkv 2, max_seqlen_k 512, the split chunk forced to 64, split_min_keys 128,
split_seqlen_q 8, max_seqlen_q 130, pages of 64 / 128 keys -- under every cap in CAPS, every window in LEFTS and both scales of `scales`.

The step's needles are keys aligned with a row's query, 8 q / |q|: their raw logit scale * q . k is near 8 at scale Dh ** -0.5 while the
other keys' logits are of order 1.  A cap of 2 or 5 flattens a needle to (almost) the cap, a cap of 50 moves it from 8 to 7.93 -- so a
missing, misplaced or mis-scaled cap shows on the needle rows far outside the bound at every cap (tests/test_attention_softcap_host.py
holds the table, computed on the CPU from the float64 oracle alone).

Left 0 is left out: every row attends one key, whose weight is 1 whatever its logit -- no value fault can be seen there."""
from __future__ import annotations

from tests import attn_window_cases as W

Step = W.Step
STEP, H, HKV, G, BOUND, MAX_Q = W.STEP, W.H, W.HKV, W.G, W.BOUND, W.MAX_Q
SPLIT_MIN_KEYS, SPLIT_SEQLEN_Q, CHUNK = W.SPLIT_MIN_KEYS, W.SPLIT_SEQLEN_Q, W.CHUNK
PAD_ROWS, SENTINEL, PAGE_SIZES, COMBOS = W.PAD_ROWS, W.SENTINEL, W.PAGE_SIZES, W.COMBOS
CAPS = (2.0, 5.0, 50.0)
LEFTS = (100, 511)
GEMMA2_SCALE = 144 ** -0.5          # Gemma-2-27B's query_pre_attn_scalar, at head dim 128


def scales(Dh):
    return (Dh ** -0.5, GEMMA2_SCALE)


def active_rows(b):
    """An active sequence that brings rows: the ones an oracle exists for."""
    return W.active(b) and STEP[b][0] > 0
