"""float64 statement of sliding-window attention on a packed step (awq_attn_varq_window and its siblings; csrc/awq_window.hpp):
`tests.attn_prefill_oracle.attention` (causal, bottom-right aligned) plus `window_left`.

    row i of a sequence with Sq rows over Sk keys stands at position p = i + Sk - Sq and attends keys max(0, p - left) <= j <= p
    p < 0: nothing attended, the row is zeros

The `stats` are those of attn_prefill_oracle -- A = sum_j p_j |v_j| / sum_j p_j and qk = max_j sum_d |q_d k_jd| over the ATTENDED keys -- so
that `attn_prefill_oracle.bound` applies unchanged.  `mutant` switches one fault in, for the tests that prove the inputs can see it:

    left+1 / left-1   the window one key longer / shorter
    topleft           the window start taken from the row index i and not from the position p
    tile-row          every row of a 64-row q tile uses the start of the tile's first row
    droptile          the 64-key tile that holds a row's window start is not visited
    nowindow          the window ignored

and the rule of a windowed mixed step (`takes`) carries `rule-sk`: Sk_b in the place of keys_b = min(Sk_b, left + Sq_b)."""
from __future__ import annotations

import torch

MUTANTS = ("left+1", "left-1", "topleft", "tile-row", "droptile", "nowindow")
RULE_MUTANTS = ("rule-sk",)
TILE = 64


def attention(q, k, v, window_left, scale=None, mutant=None, stats: bool = False):
    """q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] -> out float64 [B, Sq, H, Dh]; with stats also A [B, Sq, H, Dh] and qk [B, Sq, H]."""
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = H // Hkv
    sc = float(Dh) ** -0.5 if scale is None else float(scale)
    left = int(window_left) + {"left+1": 1, "left-1": -1}.get(mutant, 0)
    dev = q.device
    i = torch.arange(Sq, device=dev)[:, None]
    j = torch.arange(Sk, device=dev)[None, :]
    p = i + (Sk - Sq)
    if mutant == "topleft":
        start = i - left
    elif mutant == "tile-row":
        start = i // TILE * TILE + (Sk - Sq) - left
    elif mutant == "nowindow":
        start = torch.zeros_like(p)
    else:
        start = p - left
    start = start.clamp_min(0)
    if mutant == "droptile":
        start = (start // TILE + 1) * TILE
    dead = (j > p) | (j < start)
    out = torch.zeros(B, Sq, H, Dh, dtype=torch.float64, device=dev)
    A = torch.zeros_like(out) if stats else None
    qk = torch.zeros(B, Sq, H, dtype=torch.float64, device=dev) if stats else None
    for b in range(B):
        for h in range(H):
            kvh = h // G
            K, V, Q = k[b, :, kvh].double(), v[b, :, kvh].double(), q[b, :, h].double()
            s = ((Q @ K.T) * sc).masked_fill(dead, float("-inf"))
            pr = torch.softmax(s, -1)
            pr = pr.masked_fill(p < 0, 0.0)  # a row with p < 0: zeros.  (A row with p >= 0 that a mutant emptied stays NaN: it fails)
            # a dead key contributes exactly nothing, whatever it holds: its product is taken out, not multiplied by 0
            Vd = torch.where(torch.isfinite(V), V, torch.zeros_like(V))
            out[b, :, h] = pr @ Vd
            if stats:
                A[b, :, h] = pr @ Vd.abs()
                Kd = torch.where(torch.isfinite(K), K, torch.zeros_like(K))
                qk[b, :, h] = (Q.abs() @ Kd.abs().T).masked_fill(dead, 0.0).max(-1).values
    return (out, A, qk) if stats else out


def window_keys(sq, sk, left):
    """keys_b: the keys a sequence attends at all."""
    return min(sk, left + sq)


def takes(sq, seqlen_k, before, left, max_q, bound, split_q, floor, mutant=None):
    """The rule of a windowed mixed step for one sequence: sq = cu[b + 1] - cu[b], seqlen_k = seqlens_k[b], before = lens_before_step."""
    sk = seqlen_k + (sq if before else 0)
    active = 1 <= sq <= max_q and 1 <= sk <= bound
    keys = sk if mutant == "rule-sk" else window_keys(sq, sk, left)
    return active and sq <= split_q and keys >= floor
