"""Making an AWQ checkpoint on the MI355X: the parts of the reference's search and final quantisation that are heavy enough to need kernels.

  pseudo_quantize_tensor   awq/quantize/quantizer.py:61-103      one launch (ops.quantize_pack)
  auto_clip_layer          awq/quantize/auto_clip.py:11-63       one launch (ops.clip_search)
  fake_quant_scaled        auto_scale.py:128-148's `w_quantize_func(w * s) / s`, one launch
  quantize_module          quantizer.py:126-164 (`real_quantize_model_weight`) without transformers: every nn.Linear -> WQLinear.quantize_linear

All of them run the same grid arithmetic, bit-identical to torch's on fp16 / bf16 tensors (DESIGN.md "AWQ quantisation").  GPU tensors, n_bit 3 or
4, group size 128 and zero_point=True only: anything else raises -- there is no torch fallback, like the rest of the package.  The reference's
activation capture (pre_quant.py), the scale search's block forwards and apply_scale stay the reference's Python; INTEGRATION.md shows the two
lines that bind its auto_clip_layer and pseudo_quantize_tensor to the functions here.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .qmodule import WQLinear

__all__ = ["pseudo_quantize_tensor", "auto_clip_layer", "clip_token_stride", "fake_quant_scaled", "quantize_module"]


def _check_config(n_bit, zero_point, q_group_size):
    if n_bit not in (3, 4):
        raise NotImplementedError(f"the quantisation kernels implement n_bit 3 and 4, got {n_bit}")
    if not zero_point:
        raise NotImplementedError("the quantisation kernels implement zero_point=True only (the reference never uses the other branch)")
    if q_group_size != 128:
        raise NotImplementedError(f"the quantisation kernels implement q_group_size 128 only, got {q_group_size}")


@torch.no_grad()
def pseudo_quantize_tensor(w, n_bit=8, zero_point=True, q_group_size=-1, inplace=False, get_scale_zp=False):
    """quantizer.py:61-103 for a GPU fp16 / bf16 tensor whose last dimension is a multiple of 128: same signature, same return values (the
    fake-quantised tensor in w's shape; with get_scale_zp also scales and zeros viewed as [w.shape[0], -1])."""
    _check_config(n_bit, zero_point, q_group_size)
    shape = w.shape
    w2 = w.reshape(-1, shape[-1])
    r = ops.quantize_pack(w2, n_bit=n_bit, w_fake=True, scales=get_scale_zp, scaled_zeros=False, zeros=get_scale_zp, qweight=False)
    if inplace:
        w.copy_(r["w_fake"].reshape(shape))
        fake = w
    else:
        fake = r["w_fake"].reshape(shape)
    if not get_scale_zp:
        return fake
    groups = shape[-1] // 128
    scales = r["scales"][:groups].t().contiguous()  # [rows, groups]: the reference's order over (row, group)
    return fake, scales.view(shape[0], -1), r["zeros"].view(shape[0], -1)


def clip_token_stride(n_tokens: int, n_sample_token: int = 512) -> int:
    """The step of the reference's token subsample `input_feat[0 :: n_tokens // n_sample_token]` (auto_clip.py:23), at least 1: the reference
    divides by zero (a slice step of 0) below n_sample_token tokens."""
    return max(1, int(n_tokens) // int(n_sample_token))


@torch.no_grad()
def auto_clip_layer(w, input_feat, n_bit, q_config, n_grid=20, max_shrink=0.5, n_sample_token=512):
    """auto_clip.py:11-63 in one launch: -> best_max_val T [N, K/G, 1], the shape `apply_clip` takes.  The token subsample is a strided view (copied to
    w's device first if it lives elsewhere, as the reference's captured activations do), there is no output-channel batching and no N % 64 requirement.  The errors are summed in fp32 (the reference sums in T)."""
    _check_config(n_bit, q_config.get("zero_point", True), q_config.get("q_group_size", -1))
    if w.dim() != 2:
        raise ValueError("auto_clip_layer: w must be [N, K]")
    x = input_feat.reshape(-1, input_feat.shape[-1])
    x = x[:: clip_token_stride(x.shape[0], n_sample_token)]
    if x.device != w.device:
        # the reference's capture keeps the activations on the CPU (pre_quant.py:182) and auto_clip.py:38 moves them: here only the subsample moves
        x = x.to(w.device)
    best, _ = ops.clip_search(w, x, n_bit, int(n_grid), int(max_shrink * n_grid))
    return best.unsqueeze(-1)


@torch.no_grad()
def fake_quant_scaled(w, col_scale, out=None, n_bit: int = 4):
    """The scale search's `w_quantize_func(w * s) / s` (auto_scale.py:128-148 with s broadcast over the rows) in one launch: w T [N, K],
    col_scale T [K] -> T [N, K] (`out` if given)."""
    r = ops.quantize_pack(w, col_scale=col_scale.reshape(-1), n_bit=n_bit, w_fake=True if out is None else out, scales=False,
                          scaled_zeros=False, zeros=False, qweight=False)
    return r["w_fake"]


@torch.no_grad()
def quantize_module(module, w_bit=4, group_size=128, clip_list=None, layout="cdna4", skip=("lm_head",)):
    """quantizer.py:126-164 without transformers: replaces every nn.Linear under `module` (names containing an entry of `skip` excepted) in place by
    WQLinear.quantize_linear of it.  clip_list: the reference's [(name, max_val [N, K/G, 1])] with names relative to `module`; a named
    linear is clamped to +-max_val inside the same launch (apply_clip, auto_clip.py:86-98, followed by the quantisation).  Returns `module`."""
    clips = dict(clip_list or [])
    targets = [(name, m) for name, m in module.named_modules() if name and isinstance(m, nn.Linear) and not any(s in name for s in skip)]
    unknown = set(clips) - {name for name, _ in targets}
    if unknown:
        raise KeyError(f"quantize_module: clip_list names no linear of the module: {sorted(unknown)}")
    for name, lin in targets:
        clip = clips.get(name)
        if clip is not None:
            clip = clip.to(device=lin.weight.device, dtype=lin.weight.dtype)
        q = WQLinear.quantize_linear(lin, w_bit, group_size, clip_max=clip, layout=layout)
        parent_name, _, leaf = name.rpartition(".")
        parent = module.get_submodule(parent_name) if parent_name else module
        setattr(parent, leaf, q)
    return module
