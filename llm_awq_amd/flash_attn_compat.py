"""A `flash_attn` module for tinychat on MI355X.

tinychat imports `from flash_attn import flash_attn_func` at module level (tinychat/models/llama.py:21,
tinychat/modules/fused_attn.py:17) and sends every prompt through `flash_attn_func(q, k, v, causal=True)` (llama.py:218,
fused_attn.py:477,539).  The flash-attn package is CUDA-only; `llm_awq_amd.install_as_flash_attn()` puts this module into
`sys.modules["flash_attn"]` so that those imports resolve to the gfx950 prefill kernel of the engine (`attn_prefill`) -- and, for a few
query rows over at least 2048 keys (every decode step of tinychat's long-context path), to the split-KV kernels (`attn_splitkv`).

The vision towers import more (tinychat/modules/fused_siglipdecoder.py:15 `from flash_attn import flash_attn_func` at head dim 72;
tinychat/models/internvl/internvit.py:18-20 `from flash_attn.bert_padding import pad_input, unpad_input` and
`from flash_attn.flash_attn_interface import flash_attn_varlen_qkvpacked_func` inside a `try:` whose failure silently selects a naive
O(S^2) attention).  `flash_attn_interface` and `bert_padding` below are those two submodules; `install_as_flash_attn()` registers
them under `flash_attn.` as well.

Only what tinychat imports exists here: `flash_attn_func` and `flash_attn_varlen_qkvpacked_func`, forward only, no dropout, no sliding
window, no ALiBi.  Anything else that is asked for raises NotImplementedError naming the keyword -- never a silent approximation.

`flash_attn_with_kvcache` is what a decode engine with continuous batching or a captured decode graph asks of flash-attn: per-sequence
lengths in a device tensor.  It is served for an already updated cache (`k` / `v` None) by the split-KV kernels with device-side lengths
(`attn_kvcache`, csrc/awq_attn_splitkv_cdna4.hip) and, for more than 128 query rows per KV head -- a prompt chunk --, by the one-pass prefill
kernel under the same lengths (`attn_prefill_kvcache`, csrc/awq_attn_prefill_cdna4.hip).

`flash_attn_varlen_func` is the step of a continuous-batching scheduler: packed queries with per-sequence query lengths (`cu_seqlens_q`)
over a paged cache (`block_table`).  It is served by the packed-query form of the one-pass prefill kernel (`attn_prefill_paged_varq`);
packed K / V without a cache are not implemented.
"""
from __future__ import annotations

import types

__version__ = "0+llm_awq_amd"

# keyword -> values that mean "off"
_OFF = {
    "window_size": ((-1, -1), [-1, -1], None),
    "alibi_slopes": (None,),
    "return_attn_probs": (False, None),
    "softcap": (0, 0.0, None),
}


def _is_off(name, value) -> bool:
    if name in _OFF:
        return any(value is o or (not hasattr(value, "shape") and value == o) for o in _OFF[name])
    return value is None or (not hasattr(value, "shape") and not value)


def flash_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, **kw):
    """flash_attn.flash_attn_func's forward: q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] -> [B, Sq, H, Dh]."""
    if dropout_p:
        raise NotImplementedError("flash_attn_func on MI355X: dropout_p != 0 is not implemented (inference only)")
    kw.pop("deterministic", None)  # the kernel is always bit-deterministic
    for name, value in kw.items():
        if not _is_off(name, value):
            raise NotImplementedError(f"flash_attn_func on MI355X: keyword {name}={value!r} is not implemented")
    from . import load_engine

    scale = float(q.shape[-1]) ** -0.5 if softmax_scale is None else float(softmax_scale)
    eng = load_engine()
    # few query rows over a long history (the decode phase of tinychat's long_forward): the split-KV kernels where their plan splits
    if _plan_splits(eng, q, k, causal):
        return eng.attn_splitkv(q, k, v, scale, bool(causal))
    return eng.attn_prefill(q, k, v, scale, bool(causal))


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, rotary_cos=None, rotary_sin=None, cache_seqlens=None, cache_batch_idx=None,
                            cache_leftpad=None, block_table=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                            rotary_interleaved=True, alibi_slopes=None, num_splits=0, return_softmax_lse=False):
    """flash_attn.flash_attn_with_kvcache's forward for a cache that is already up to date: q [B, Sq, H, Dh], k_cache / v_cache
    [Bc >= B, Lmax, Hkv, Dh], cache_seqlens the TOTAL length of every sequence as an int32 tensor [B] on the GPU (read by the kernels only:
    no host copy, no sync, capturable) or an int -> [B, Sq, H, Dh].  Served with max_seqlen_k = Lmax by `attn_kvcache` while
    Sq * (H / Hkv) <= 128 and by `attn_prefill_kvcache` (the one-pass prefill kernel, any Sq) beyond; Dh 64 or 128.  A sequence whose length is < 1 or > Lmax returns zeros.  `cache_seqlens=None` attends the whole cache
    (`flash_attn_func`).  Appending k / v, rotary_cos / rotary_sin, block_table, cache_batch_idx, cache_leftpad, a window, softcap, ALiBi
    and the softmax LSE are not implemented and raise NotImplementedError naming the argument (`rotary_interleaved` and `num_splits`
    have nothing to act on and are ignored: there is no rotation here, and the split count is the plan's)."""
    asked = {"k": k, "v": v, "rotary_cos": rotary_cos, "rotary_sin": rotary_sin, "cache_batch_idx": cache_batch_idx,
             "cache_leftpad": cache_leftpad, "block_table": block_table, "window_size": window_size, "softcap": softcap,
             "alibi_slopes": alibi_slopes, "return_softmax_lse": return_softmax_lse}
    for name, value in asked.items():
        if not _is_off(name, value):
            shown = f"tensor{tuple(value.shape)}" if hasattr(value, "shape") else repr(value)
            hint = " -- a paged cache is served by llm_awq_amd.ops.attn_kvcache_paged, whose pools are [num_pages, page_size, Hkv, Dh]" \
                if name == "block_table" else ""
            raise NotImplementedError(f"flash_attn_with_kvcache on MI355X: {name}={shown} is not implemented (the cache must already hold "
                                      f"the new tokens; cache_seqlens are total lengths){hint}")
    if cache_seqlens is None:
        return flash_attn_func(q, k_cache[:q.shape[0]], v_cache[:q.shape[0]], softmax_scale=softmax_scale, causal=causal)
    import torch

    from . import load_engine

    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=q.device)
    scale = float(q.shape[-1]) ** -0.5 if softmax_scale is None else float(softmax_scale)
    eng = load_engine()
    prompt = q.dim() == 4 and k_cache.dim() == 4 and k_cache.shape[2] >= 1 and q.shape[1] * (q.shape[2] // k_cache.shape[2]) > 128
    attn = eng.attn_prefill_kvcache if prompt else eng.attn_kvcache
    return attn(q, k_cache, v_cache, cache_seqlens, int(k_cache.shape[1]), 0, scale, bool(causal))


def _plan_splits(eng, q, k, causal) -> bool:
    """Whether attn_splitkv_plan splits this call: never below 2048 keys (unless the test knob attn_splitkv_chunk forces a chunk).
    Shapes the plan would refuse go to attn_prefill, which names what is wrong with them."""
    if getattr(q, "dim", lambda: 0)() != 4 or getattr(k, "dim", lambda: 0)() != 4:
        return False
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    if min(B, Sq, Sk, Hkv) < 1 or Dh not in (64, 128) or H % Hkv or (causal and Sq > Sk):
        return False
    return eng.attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, bool(causal))[0] > 1


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False, **kw):
    """flash_attn.flash_attn_varlen_qkvpacked_func's forward: qkv [nnz, 3, H, Dh], cu_seqlens int32 [nseq + 1] on the GPU -> [nnz, H, Dh].
    Encoder attention only: every row attends the keys of its own sequence."""
    if dropout_p:
        raise NotImplementedError("flash_attn_varlen_qkvpacked_func on MI355X: dropout_p != 0 is not implemented (inference only)")
    if causal:
        raise NotImplementedError("flash_attn_varlen_qkvpacked_func on MI355X: causal=True is not implemented (encoder towers only)")
    kw.pop("deterministic", None)  # the kernel is always bit-deterministic
    for name, value in kw.items():
        if not _is_off(name, value):
            raise NotImplementedError(f"flash_attn_varlen_qkvpacked_func on MI355X: keyword {name}={value!r} is not implemented")
    from . import load_engine

    scale = float(qkv.shape[-1]) ** -0.5 if softmax_scale is None else float(softmax_scale)
    return load_engine().attn_varlen_qkvpacked(qkv, cu_seqlens, int(max_seqlen), scale, False)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False, block_table=None,
                           **kw):
    """flash_attn.flash_attn_varlen_func's forward over a PAGED KV cache (the continuous-batching step): q [total_q, H, Dh] packed rows,
    cu_seqlens_q int32 [B + 1] on the GPU, k / v the pools [num_pages, page_size, Hkv, Dh] with block_table int32 [B, pages_per_seq],
    cu_seqlens_k int32 [B + 1] whose differences are the TOTAL key lengths (formed on the device: no host read, capturable)
    -> [total_q, H, Dh].  Served by `attn_prefill_paged_varq` (the one-pass prefill kernel over packed queries; Dh 64 or 128, page_size a
    multiple of 64).  Packed K / V without a cache (block_table=None), dropout, a window, softcap, ALiBi and the attention probabilities
    are not implemented and raise NotImplementedError naming the argument."""
    if dropout_p:
        raise NotImplementedError("flash_attn_varlen_func on MI355X: dropout_p != 0 is not implemented (inference only)")
    asked = dict(kw, window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes, return_attn_probs=return_attn_probs)
    for name, value in asked.items():
        if not _is_off(name, value):
            shown = f"tensor{tuple(value.shape)}" if hasattr(value, "shape") else repr(value)
            raise NotImplementedError(f"flash_attn_varlen_func on MI355X: keyword {name}={shown} is not implemented")
    if block_table is None:
        raise NotImplementedError("flash_attn_varlen_func on MI355X: block_table=None is not implemented (packed k / v without a cache; "
                                  "k / v must be the pools [num_pages, page_size, Hkv, Dh] of a paged KV cache that already holds the new "
                                  "tokens -- an encoder's packed qkv is served by flash_attn_varlen_qkvpacked_func)")
    from . import load_engine

    scale = float(q.shape[-1]) ** -0.5 if softmax_scale is None else float(softmax_scale)
    seqlens_k = (cu_seqlens_k[1:] - cu_seqlens_k[:-1]).contiguous()  # total lengths, on the device
    return load_engine().attn_prefill_paged_varq(q, k, v, block_table, cu_seqlens_q, int(max_seqlen_q), seqlens_k, int(max_seqlen_k), False, scale,
                                                 bool(causal))


# ---- flash_attn.bert_padding: plain torch, any device ----
def index_first_axis(input, indices):
    """input [n, ...] -> input[indices] (flash_attn.bert_padding.index_first_axis's forward)."""
    return input[indices]


def unpad_input(hidden_states, attention_mask):
    """hidden_states [B, S, ...], attention_mask [B, S] (nonzero = kept) -> (hidden_states of the kept tokens [nnz, ...], their indices
    into the flattened [B * S] axis, cu_seqlens int32 [B + 1], the longest sequence as an int): the four values internvit.py:74 unpacks."""
    import torch

    lens = attention_mask.sum(dim=-1, dtype=torch.int32)
    indices = torch.nonzero(attention_mask.flatten(), as_tuple=False).flatten()
    max_seqlen = int(lens.max().item())
    cu_seqlens = torch.nn.functional.pad(torch.cumsum(lens, dim=0, dtype=torch.int32), (1, 0))
    flat = hidden_states.reshape(hidden_states.shape[0] * hidden_states.shape[1], *hidden_states.shape[2:])
    return index_first_axis(flat, indices), indices, cu_seqlens, max_seqlen


def pad_input(hidden_states, indices, batch, seqlen):
    """The inverse of unpad_input: hidden_states [nnz, ...] -> [batch, seqlen, ...] with zeros at the dropped positions."""
    import torch

    out = torch.zeros(batch * seqlen, *hidden_states.shape[1:], dtype=hidden_states.dtype, device=hidden_states.device)
    out[indices] = hidden_states
    return out.view(batch, seqlen, *hidden_states.shape[1:])


def _namespace(name, **members):
    m = types.ModuleType(__name__ + "." + name)
    m.__dict__.update(members)
    m.__all__ = sorted(members)
    return m


flash_attn_interface = _namespace("flash_attn_interface", flash_attn_func=flash_attn_func,
                                  flash_attn_varlen_qkvpacked_func=flash_attn_varlen_qkvpacked_func,
                                  flash_attn_varlen_func=flash_attn_varlen_func, flash_attn_with_kvcache=flash_attn_with_kvcache)
bert_padding = _namespace("bert_padding", unpad_input=unpad_input, pad_input=pad_input, index_first_axis=index_first_axis)
SUBMODULES = {"flash_attn_interface": flash_attn_interface, "bert_padding": bert_padding}

__all__ = ["flash_attn_func", "flash_attn_varlen_qkvpacked_func", "flash_attn_varlen_func", "flash_attn_with_kvcache", "flash_attn_interface", "bert_padding"]
