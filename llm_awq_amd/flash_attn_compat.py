"""A `flash_attn` module for tinychat on MI355X.

tinychat imports `from flash_attn import flash_attn_func` at module level (tinychat/models/llama.py:21,
tinychat/modules/fused_attn.py:17) and sends every prompt through `flash_attn_func(q, k, v, causal=True)` (llama.py:218,
fused_attn.py:477,539).  The flash-attn package is CUDA-only; `llm_awq_amd.install_as_flash_attn()` puts this module into
`sys.modules["flash_attn"]` so that those imports resolve to the gfx950 prefill kernel of the engine (`attn_prefill`).

Only what tinychat imports exists here: `flash_attn_func`, forward only, no dropout, no sliding window, no ALiBi.  Anything else
that is asked for raises NotImplementedError naming the keyword -- never a silent approximation.
"""
from __future__ import annotations

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
    return load_engine().attn_prefill(q, k, v, scale, bool(causal))


__all__ = ["flash_attn_func"]
