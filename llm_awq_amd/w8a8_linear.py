"""W8A8 linear modules on the MI355X int8 GEMM: the mirror of the reference's awq/quantize/w8a8_linear.py
(`W8A8OF16LinearStaticScale`, `W8A8OF16LinearDynamicInputScale`) with the same constructor signature, buffers and state-dict keys,
so the vision towers' checkpoints load and tinychat/modules/fused_siglipdecoder.py / fused_internencoder.py bind unchanged.

int8 activations [M, K] with per-token fp16 scales come from `invoke_quant`, `gelu_and_quant` or `rms_norm_general`; the output is
written into the caller's fp16 buffer.  `FakeW8A8Linear` / `fake_quant` (pseudo-quantisation for accuracy studies) are not mirrored.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import load_engine

__all__ = ["quantize_weight_per_channel", "W8A8OF16LinearStaticScale", "W8A8OF16LinearDynamicInputScale"]


def quantize_weight_per_channel(weight: torch.Tensor, s1_scale: Optional[torch.Tensor] = None):
    """The reference's weight quantisation (w8a8_linear.py:154-171, :192-210) as a pure function: per output row
    s = clamp(max |w|, 1e-5) / 127 in the WEIGHT's dtype, q = int8(round_half_even(w / s)); returns (q int8 [N, K], s [N, 1] in the
    weight's dtype).  The modules store s.half() while the division used the unrounded s -- the reference's behaviour, kept.  Unlike
    the reference (`div_`) the caller's weight is left untouched."""
    if s1_scale is None:
        s1_scale, _ = torch.max(weight.abs(), dim=-1, keepdim=True)
        s1_scale = s1_scale.clamp_(min=1e-5).div_(127)
    q = (weight / s1_scale.to(weight.device)).round_().to(torch.int8)
    return q, s1_scale


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class W8A8OF16LinearStaticScale(torch.nn.Module):
    def __init__(
        self,
        in_features: int,
        out_features: int,
        bias: bool = True,
        scale: Union[torch.Tensor, float] = 1.0,
        params_dtype: Optional[torch.dtype] = None,
    ):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        # size [oc]
        self.register_buffer("dequant_scale", torch.ones(out_features, dtype=torch.half))
        self.create_weights()
        if bias:
            # a plain tensor attribute, neither parameter nor buffer, as in the reference (w8a8_linear.py:36-41): it stays out of the state dict
            self.bias = torch.empty(self.out_features, device=_default_device(), dtype=torch.float16)
        else:
            self.register_parameter("bias", None)

    def create_weights(self) -> None:
        self.register_buffer("weight", torch.empty(self.out_features, self.in_features, dtype=torch.int8, requires_grad=False))

    def apply_weights(self, x: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
        raise NotImplementedError

    def forward(self, input_):
        output = self.apply_weights(input_, self.bias)
        output_bias = self.bias
        return output, output_bias


class W8A8OF16LinearDynamicInputScale(W8A8OF16LinearStaticScale):
    def __init__(
        self,
        in_features: int,
        out_features: int,
        bias: bool = True,
        scale: Union[torch.Tensor, float] = 1.0,
        params_dtype: Optional[torch.dtype] = None,
    ):
        super().__init__(in_features=in_features, out_features=out_features, bias=bias, scale=scale, params_dtype=params_dtype)
        self.apply_weights = self.apply_weights_bias if bias else self.apply_weights_no_bias

    @staticmethod
    def _check_2d(x):
        if x.dim() != 2:
            raise NotImplementedError("W8A8OF16LinearDynamicInputScale: int8 activations [tokens, channels] are expected")

    # with bias: bias fused into the GEMM's epilogue
    def apply_weights_bias(self, x: torch.Tensor, input_scale: torch.Tensor, output_buffer: torch.Tensor, bias: torch.Tensor = None):
        self._check_2d(x)
        load_engine().w8a8_gemm_fuse_bias_forward_cuda(x, self.weight, self.dequant_scale, input_scale, output_buffer, bias)

    def apply_weights_no_bias(self, x: torch.Tensor, input_scale: torch.Tensor, output_buffer: torch.Tensor, bias: torch.Tensor = None):
        self._check_2d(x)
        load_engine().w8a8_gemm_forward_cuda(x, self.weight, self.dequant_scale, input_scale, output_buffer)

    def forward(self, input_, input_scale, output_buffer):
        self.apply_weights(input_, input_scale, output_buffer, self.bias)

    @classmethod
    def _from_weight(cls, weight, bias, s1_scale):
        q_linear = cls(weight.shape[1], weight.shape[0], bias is not None)
        device = weight.device if weight.is_cuda else _default_device()
        q, s1_scale = quantize_weight_per_channel(weight, s1_scale)
        q_linear.weight.data[:, :] = q
        q_linear.dequant_scale.data[:] = s1_scale.reshape(-1).half()
        if bias is not None:
            q_linear.bias = bias.detach().clone().half().contiguous().to(device)  # (a plain attribute: Module.to() does not carry it)
        return q_linear.to(device)

    @classmethod
    def from_linear(cls, linear, init_only=False, s1_scale=None, fc1=False):
        if init_only:  # just prepare for loading a state dict
            return cls(linear.in_features, linear.out_features, linear.bias is not None)
        return cls._from_weight(linear.weight.data, None if linear.bias is None else linear.bias.data, s1_scale)

    @classmethod
    def from_qkv(cls, q, k, v, init_only=False, s1_scale=None):
        if init_only:
            return cls(q.in_features, q.out_features + k.out_features + v.out_features, q.bias is not None)
        weight = torch.cat([q.weight.data, k.weight.data, v.weight.data], dim=0)
        bias = None if q.bias is None else torch.cat([q.bias.data, k.bias.data, v.bias.data], dim=0)
        return cls._from_weight(weight, bias, s1_scale)
