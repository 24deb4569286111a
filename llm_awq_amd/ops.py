"""Torch-tensor conveniences over the C ABI (device memory + current stream are the only things
torch provides here).  Every function requires GPU tensors and the built HIP library."""
from __future__ import annotations

import torch

from . import _capi


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float16:
        return _capi.AWQ_F16
    if t.dtype == torch.bfloat16:
        return _capi.AWQ_BF16
    raise TypeError(f"expected float16/bfloat16, got {t.dtype}")


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise ValueError("tensors must be contiguous")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def gemv(x, qweight, scales, scaled_zeros, group_size: int = 128):
    """C-ABI awq_w4a16_gemv: x [..., K] with 1 <= M <= 16 rows."""
    _need_gpu(x, qweight, scales, scaled_zeros)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_gemv(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                                                scaled_zeros.data_ptr(), out.data_ptr(), m, n, k, group_size, _dt(x),
                                                _stream(x)))
    return out


def gemm(x, qweight, scales, scaled_zeros, group_size: int = 128):
    """C-ABI awq_w4a16_gemm: any M >= 1."""
    _need_gpu(x, qweight, scales, scaled_zeros)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    L = _capi.lib()
    wsb = L.awq_w4a16_gemm_workspace_bytes(m, n, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    with torch.cuda.device(x.device):
        _capi.check(L.awq_w4a16_gemm(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                     out.data_ptr(), m, n, k, group_size, _dt(x), ws.data_ptr() if wsb else None, wsb,
                                     _stream(x)))
    return out


def forward(x, qweight, scales, scaled_zeros, bias=None, group_size: int = 128):
    """C-ABI awq_w4a16_forward: WQLinear.forward's dispatch + optional bias."""
    _need_gpu(x, qweight, scales, scaled_zeros, bias)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    L = _capi.lib()
    wsb = L.awq_w4a16_gemm_workspace_bytes(m, n, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    with torch.cuda.device(x.device):
        _capi.check(L.awq_w4a16_forward(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                        bias.data_ptr() if bias is not None else None, out.data_ptr(), m, n, k,
                                        group_size, _dt(x), ws.data_ptr() if wsb else None, wsb, _stream(x)))
    return out


def unpack_v2(qweight):
    """int16 [N/4, K] -> uint8 [N, K] logical 4-bit integers (GPU kernel, same unpack code as the matmuls)."""
    _need_gpu(qweight)
    n, k = qweight.shape[0] * 4, qweight.shape[1]
    out = torch.empty(n, k, dtype=torch.uint8, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _capi.check(_capi.lib().awq_unpack_v2(qweight.data_ptr(), out.data_ptr(), n, k, _stream(qweight)))
    return out


def dequant_v2(qweight, scales, scaled_zeros, group_size: int = 128):
    """-> T [N, K] = round_T(q*s + sz) (GPU kernel, same dequant code as the matmuls)."""
    _need_gpu(qweight, scales, scaled_zeros)
    n, k = qweight.shape[0] * 4, qweight.shape[1]
    out = torch.empty(n, k, dtype=scales.dtype, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _capi.check(_capi.lib().awq_dequant_v2(qweight.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                                out.data_ptr(), n, k, group_size, _dt(scales), _stream(qweight)))
    return out


def pack_v2(q_u8):
    """uint8 [N, K] -> int16 [N/4, K] (GPU pack_intweight)."""
    _need_gpu(q_u8)
    assert q_u8.dtype == torch.uint8
    n, k = q_u8.shape
    out = torch.empty(n // 4, k, dtype=torch.int16, device=q_u8.device)
    with torch.cuda.device(q_u8.device):
        _capi.check(_capi.lib().awq_pack_v2(q_u8.data_ptr(), out.data_ptr(), n, k, _stream(q_u8)))
    return out


def repack_v1_to_v2(qweight_v1, scales_v1, qzeros_v1):
    """v1 (qweight int32 [N,K/8], scales T [N,Gpad], qzeros int32 [N,Gpad/8]) -> v2 triple."""
    _need_gpu(qweight_v1, scales_v1, qzeros_v1)
    n, k = qweight_v1.shape[0], qweight_v1.shape[1] * 8
    gpad = scales_v1.shape[1]
    dev = qweight_v1.device
    qw2 = torch.empty(n // 4, k, dtype=torch.int16, device=dev)
    s2 = torch.empty(gpad, n, dtype=scales_v1.dtype, device=dev)
    sz2 = torch.empty(gpad, n, dtype=scales_v1.dtype, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_repack_v1_to_v2(qweight_v1.data_ptr(), scales_v1.data_ptr(), qzeros_v1.data_ptr(),
                                                     qw2.data_ptr(), s2.data_ptr(), sz2.data_ptr(), n, k, gpad,
                                                     _dt(scales_v1), _stream(qweight_v1)))
    return qw2, s2, sz2


# ---- cdna4 interleave (bf16) ----

def repack_v2_to_cdna4(qweight_v2):
    _need_gpu(qweight_v2)
    n, k = qweight_v2.shape[0] * 4, qweight_v2.shape[1]
    out = torch.empty_like(qweight_v2)
    with torch.cuda.device(qweight_v2.device):
        _capi.check(_capi.lib().awq_repack_v2_to_cdna4(qweight_v2.data_ptr(), out.data_ptr(), n, k, _stream(qweight_v2)))
    return out


def repack_cdna4_to_v2(qweight_cdna4):
    _need_gpu(qweight_cdna4)
    n, k = qweight_cdna4.shape[0] * 4, qweight_cdna4.shape[1]
    out = torch.empty_like(qweight_cdna4)
    with torch.cuda.device(qweight_cdna4.device):
        _capi.check(_capi.lib().awq_repack_cdna4_to_v2(qweight_cdna4.data_ptr(), out.data_ptr(), n, k, _stream(qweight_cdna4)))
    return out


def unpack_cdna4(qweight):
    _need_gpu(qweight)
    n, k = qweight.shape[0] * 4, qweight.shape[1]
    out = torch.empty(n, k, dtype=torch.uint8, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _capi.check(_capi.lib().awq_unpack_cdna4(qweight.data_ptr(), out.data_ptr(), n, k, _stream(qweight)))
    return out


def dequant_cdna4(qweight, scales, scaled_zeros, group_size: int = 128):
    _need_gpu(qweight, scales, scaled_zeros)
    n, k = qweight.shape[0] * 4, qweight.shape[1]
    out = torch.empty(n, k, dtype=scales.dtype, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _capi.check(_capi.lib().awq_dequant_cdna4(qweight.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                                   out.data_ptr(), n, k, group_size, _dt(scales), _stream(qweight)))
    return out


def pack_sz_cdna4(scales, scaled_zeros, in_features: int):
    """-> int32 [N/16, K/128, 16] packed {scale | scaled_zero << 16} (bit patterns)."""
    _need_gpu(scales, scaled_zeros)
    n, k = scales.shape[1], in_features
    out = torch.empty(n // 16, k // 128, 16, dtype=torch.int32, device=scales.device)
    with torch.cuda.device(scales.device):
        _capi.check(_capi.lib().awq_pack_sz_cdna4(scales.data_ptr(), scaled_zeros.data_ptr(), out.data_ptr(), n, k,
                                                   _stream(scales)))
    return out


def pack_szh_cdna4(scales, scaled_zeros, in_features: int):
    """-> (int32 [N/16, K/128, 16] "sz_half" {f16(s') | f16(sz) << 16}, exact: bool).  `exact` False means a scale of this
    layer is not representable as a normal f16 number: keep sz_packed (pack_sz_cdna4) for it.  Synchronises (reads the flag)."""
    _need_gpu(scales, scaled_zeros)
    n, k = scales.shape[1], in_features
    out = torch.empty(n // 16, k // 128, 16, dtype=torch.int32, device=scales.device)
    flag = torch.zeros(1, dtype=torch.int32, device=scales.device)
    with torch.cuda.device(scales.device):
        _capi.check(_capi.lib().awq_pack_szh_cdna4(scales.data_ptr(), scaled_zeros.data_ptr(), out.data_ptr(), flag.data_ptr(), n, k,
                                                    _dt(scales), _stream(scales)))
    return out, int(flag.item()) == 0


def decode_cdna4(x, qweight, sz_half, bias=None, epilogue: int = 0, group_size: int = 128):
    """C-ABI awq_w4a16_decode_cdna4: 1 <= M <= 8 on cdna4 weights + sz_half.  epilogue 0: x.W^T (+ bias); 1: stacked [gate; up]
    -> silu(gate) * up; 2: the same with gate / up rows interleaved 8 + 8 per slab."""
    _need_gpu(x, qweight, sz_half, bias)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n // 2 if epilogue else n, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_decode_cdna4(x.data_ptr(), qweight.data_ptr(), sz_half.data_ptr(),
                                                        bias.data_ptr() if bias is not None else None, out.data_ptr(), m, n, k,
                                                        group_size, _dt(x), int(epilogue), _stream(x)))
    return out


def partial_cdna4(x, qweight, sz_packed, sz_half=None, group_size: int = 128):
    """C-ABI awq_w4a16_partial_cdna4: the K shard's product x . W^T as fp32 [..., N], unrounded, no bias (tensor-parallel row split)."""
    _need_gpu(x, qweight, sz_packed, sz_half)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=torch.float32, device=x.device)
    if m == 0:
        return out
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_partial_cdna4(x.data_ptr(), qweight.data_ptr(), sz_packed.data_ptr(),
                                                         sz_half.data_ptr() if sz_half is not None else None, out.data_ptr(), m, n, k,
                                                         group_size, _dt(x), _stream(x)))
    return out


def round_bias_f32(y32, dtype, bias=None):
    """C-ABI awq_round_bias_f32: T(y32) (+ bias in T) -- the single rounding after the fp32 partials of a row split were summed."""
    _need_gpu(y32, bias)
    if y32.dtype != torch.float32:
        raise TypeError("expected the float32 sum of the partials")
    n = y32.shape[-1]
    m = y32.numel() // n
    out = torch.empty(y32.shape, dtype=dtype, device=y32.device)
    if m == 0:
        return out
    with torch.cuda.device(y32.device):
        _capi.check(_capi.lib().awq_round_bias_f32(y32.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), m, n,
                                                    _dt(out), _stream(y32)))
    return out


def gemv_cdna4(x, qweight, scales, scaled_zeros, sz_packed=None, group_size: int = 128):
    _need_gpu(x, qweight, scales, scaled_zeros, sz_packed)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_gemv_cdna4(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                                                      scaled_zeros.data_ptr(),
                                                      sz_packed.data_ptr() if sz_packed is not None else None,
                                                      out.data_ptr(), m, n, k, group_size, _dt(x), _stream(x)))
    return out


def gemm_cdna4(x, qweight, scales, scaled_zeros, bias=None, sz_packed=None, group_size: int = 128, sz_half=None):
    """C-ABI awq_w4a16_forward_cdna4 (awq_w4a16_forward_cdna4_szh when the layer's sz_half side buffer is given): any M (M <= 16 -> GEMV), optional bias."""
    _need_gpu(x, qweight, scales, scaled_zeros, bias, sz_packed, sz_half)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        ws_bytes = _capi.lib().awq_w4a16_forward_cdna4_workspace_bytes(m, n, k)  # (inside the device context: the plan asks the CURRENT device for its CU count)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
        if sz_half is not None:
            _capi.check(_capi.lib().awq_w4a16_forward_cdna4_szh(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                                                 sz_packed.data_ptr() if sz_packed is not None else None, sz_half.data_ptr(),
                                                                 bias.data_ptr() if bias is not None else None, out.data_ptr(), m, n, k, group_size,
                                                                 _dt(x), ws.data_ptr() if ws is not None else None, ws_bytes, _stream(x)))
            return out
        _capi.check(_capi.lib().awq_w4a16_forward_cdna4(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                                                         scaled_zeros.data_ptr(),
                                                         sz_packed.data_ptr() if sz_packed is not None else None,
                                                         bias.data_ptr() if bias is not None else None,
                                                         out.data_ptr(), m, n, k, group_size, _dt(x),
                                                         ws.data_ptr() if ws is not None else None, ws_bytes, _stream(x)))
    return out


def mlp_gate_up_cdna4(x, qweight_gate_up, sz_packed, group_size: int = 128):
    """C-ABI awq_w4a16_mlp_gate_up_cdna4: silu(x.Wg^T) * (x.Wu^T) in one launch; qweight_gate_up = the gate and up
    cdna4 buffers stacked along N, sz_packed from the equally stacked scales.  1 <= M <= 8, bf16."""
    _need_gpu(x, qweight_gate_up, sz_packed)
    k = x.shape[-1]
    m = x.numel() // k
    n2 = qweight_gate_up.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n2 // 2, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_mlp_gate_up_cdna4(x.data_ptr(), qweight_gate_up.data_ptr(), sz_packed.data_ptr(),
                                                             out.data_ptr(), m, n2, k, group_size, _dt(x), _stream(x)))
    return out


def mlp_gate_up_forward_cdna4(x, qweight_interleaved, sz_packed, sz_half=None, group_size: int = 128):
    """C-ABI awq_w4a16_mlp_gate_up_forward_cdna4: QuantLlamaMLP.our_llama_mlp for any row count on the 8 + 8 interleaved pair."""
    _need_gpu(x, qweight_interleaved, sz_packed, sz_half)
    k = x.shape[-1]
    m = x.numel() // k
    n2 = qweight_interleaved.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n2 // 2, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        ws_bytes = _capi.lib().awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes(m, n2, k)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
        _capi.check(_capi.lib().awq_w4a16_mlp_gate_up_forward_cdna4_ws(x.data_ptr(), qweight_interleaved.data_ptr(), sz_packed.data_ptr(),
                                                                        sz_half.data_ptr() if sz_half is not None else None, out.data_ptr(),
                                                                        m, n2, k, group_size, _dt(x), ws.data_ptr() if ws is not None else None,
                                                                        ws_bytes, _stream(x)))
    return out


def rmsnorm(x, gamma, eps: float):
    """C-ABI awq_rmsnorm: T((float(x) * rsqrt(mean(x^2) + eps)) * float(gamma)) for every row of x [.., k] (layernorm.cu:39-61)."""
    _need_gpu(x, gamma)
    k = x.shape[-1]
    out = torch.empty_like(x)
    if x.numel() == 0:  # (an empty batch: as the torch binding, nothing to launch)
        return out
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_rmsnorm(x.data_ptr(), gamma.data_ptr(), float(eps), out.data_ptr(), x.numel() // k, k, _dt(x), _stream(x)))
    return out


def rmsnorm_forward_cdna4(x, gamma, eps: float, qweight, sz_packed, bias=None, fused_gate_up: bool = False, group_size: int = 128):
    """C-ABI awq_w4a16_rmsnorm_forward_cdna4: T5/Llama RMSNorm (FTLlamaRMSNorm, fused_norm.py:7-21) fused in front of the
    quantised linear -- or, with fused_gate_up, of the gate/up pair + SiLU*mul.  x: un-normalised [.., K], 1 <= M <= 4."""
    _need_gpu(x, gamma, qweight, sz_packed)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n // 2 if fused_gate_up else n, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w4a16_rmsnorm_forward_cdna4(x.data_ptr(), gamma.data_ptr(), float(eps), qweight.data_ptr(),
                                                                 sz_packed.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                                 out.data_ptr(), m, n, k, group_size, _dt(x), 1 if fused_gate_up else 0,
                                                                 _stream(x)))
    return out


# ---- W3 ("w3c" tiles, bf16) ----

def pack_w3(q_u8):
    """uint8 [N, K] (0..7) -> int16 [N/4, 3K/4] w3c tiles (GPU kernel)."""
    _need_gpu(q_u8)
    assert q_u8.dtype == torch.uint8
    n, k = q_u8.shape
    out = torch.empty(n // 4, k * 3 // 4, dtype=torch.int16, device=q_u8.device)
    with torch.cuda.device(q_u8.device):
        _capi.check(_capi.lib().awq_pack_w3(q_u8.data_ptr(), out.data_ptr(), n, k, _stream(q_u8)))
    return out


def unpack_w3(qweight_w3):
    _need_gpu(qweight_w3)
    n, k = qweight_w3.shape[0] * 4, qweight_w3.shape[1] * 4 // 3
    out = torch.empty(n, k, dtype=torch.uint8, device=qweight_w3.device)
    with torch.cuda.device(qweight_w3.device):
        _capi.check(_capi.lib().awq_unpack_w3(qweight_w3.data_ptr(), out.data_ptr(), n, k, _stream(qweight_w3)))
    return out


def dequant_w3(qweight_w3, scales, scaled_zeros, group_size: int = 128):
    _need_gpu(qweight_w3, scales, scaled_zeros)
    n, k = qweight_w3.shape[0] * 4, qweight_w3.shape[1] * 4 // 3
    out = torch.empty(n, k, dtype=scales.dtype, device=qweight_w3.device)
    with torch.cuda.device(qweight_w3.device):
        _capi.check(_capi.lib().awq_dequant_w3(qweight_w3.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                                out.data_ptr(), n, k, group_size, _dt(scales), _stream(qweight_w3)))
    return out


def forward_w3(x, qweight_w3, scales, scaled_zeros, sz_packed, bias=None, group_size: int = 128):
    """C-ABI awq_w3a16_forward: any M; every kernel reads the 3-bit tiles natively (the workspace is the optional split-K scratch)."""
    _need_gpu(x, qweight_w3, scales, scaled_zeros, sz_packed, bias)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight_w3.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    L = _capi.lib()
    with torch.cuda.device(x.device):
        wsb = L.awq_w3a16_forward_workspace_bytes(m, n, k)
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
        _capi.check(L.awq_w3a16_forward(x.data_ptr(), qweight_w3.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(),
                                        sz_packed.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                        m, n, k, group_size, _dt(x), ws.data_ptr() if wsb else None, wsb, _stream(x)))
    return out


def mlp_gate_up_forward_w3(x, qweight_w3_interleaved, sz_packed, group_size: int = 128):
    """C-ABI awq_w3a16_mlp_gate_up_forward: QuantLlamaMLP.our_llama_mlp on 3-bit projections (rows interleaved 8 + 8, w3c tiles), any row count."""
    _need_gpu(x, qweight_w3_interleaved, sz_packed)
    k = x.shape[-1]
    m = x.numel() // k
    n2 = qweight_w3_interleaved.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n2 // 2, dtype=x.dtype, device=x.device)
    L = _capi.lib()
    with torch.cuda.device(x.device):
        wsb = L.awq_w3a16_mlp_gate_up_forward_workspace_bytes(m, n2, k)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=x.device) if wsb else None
        _capi.check(L.awq_w3a16_mlp_gate_up_forward(x.data_ptr(), qweight_w3_interleaved.data_ptr(), sz_packed.data_ptr(), out.data_ptr(), m, n2, k,
                                                     group_size, _dt(x), ws.data_ptr() if ws is not None else None, wsb, _stream(x)))
    return out


def partial_w3(x, qweight_w3, sz_packed, group_size: int = 128):
    """C-ABI awq_w3a16_partial: the K shard's product of a 3-bit layer as fp32 [..., N], unrounded, no bias (tensor-parallel row split)."""
    _need_gpu(x, qweight_w3, sz_packed)
    k = x.shape[-1]
    m = x.numel() // k
    n = qweight_w3.shape[0] * 4
    out = torch.empty(*x.shape[:-1], n, dtype=torch.float32, device=x.device)
    if m == 0:
        return out
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_w3a16_partial(x.data_ptr(), qweight_w3.data_ptr(), sz_packed.data_ptr(), out.data_ptr(), m, n, k,
                                                   group_size, _dt(x), _stream(x)))
    return out


# ---- grouped (per-expert) GEMM for MoE layers ----

def moe_gemm(x_sorted, qweight, scales, scaled_zeros, expert_offsets, layout: str = "v2", group_size: int = 128):
    """C-ABI awq_w4a16_moe_gemm.  x_sorted [T, K] (tokens sorted by expert), qweight int16 [E, N/4, K],
    scales / scaled_zeros T [E, Gpad, N], expert_offsets int32 [E + 1] on the device -> out [T, N]."""
    _need_gpu(x_sorted, qweight, scales, scaled_zeros, expert_offsets)
    assert expert_offsets.dtype == torch.int32 and qweight.dim() == 3 and scales.dim() == 3
    e, n, k = qweight.shape[0], qweight.shape[1] * 4, qweight.shape[2]
    t = x_sorted.shape[0]
    out = torch.empty(t, n, dtype=x_sorted.dtype, device=x_sorted.device)
    with torch.cuda.device(x_sorted.device):
        _capi.check(_capi.lib().awq_w4a16_moe_gemm(x_sorted.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                                                    scaled_zeros.data_ptr(), expert_offsets.data_ptr(), out.data_ptr(), t, e,
                                                    n, k, scales.shape[1], group_size, _dt(x_sorted),
                                                    1 if layout == "cdna4" else 0, _stream(x_sorted)))
    return out


def moe_forward_cdna4(x_sorted, qweight, scales, scaled_zeros, sz_packed, expert_offsets, group_size: int = 128, sz_half=None):
    """C-ABI awq_w4a16_moe_forward_cdna4(_szh): grouped GEMV for <= 8 sorted rows (decode), grouped GEMM otherwise; sz_half = the experts' stacked
    sz_half side buffers (every expert exact) for the f16-mantissa dequant form of the grouped tile launch."""
    _need_gpu(x_sorted, qweight, scales, scaled_zeros, sz_packed, expert_offsets, sz_half)
    assert expert_offsets.dtype == torch.int32 and qweight.dim() == 3 and sz_packed.dtype == torch.int32
    e, n, k = qweight.shape[0], qweight.shape[1] * 4, qweight.shape[2]
    t = x_sorted.shape[0]
    out = torch.empty(t, n, dtype=x_sorted.dtype, device=x_sorted.device)
    with torch.cuda.device(x_sorted.device):
        _capi.check(_capi.lib().awq_w4a16_moe_forward_cdna4_szh(x_sorted.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                                                                 scaled_zeros.data_ptr(), sz_packed.data_ptr(),
                                                                 sz_half.data_ptr() if sz_half is not None else None,
                                                                 expert_offsets.data_ptr(), out.data_ptr(), t, e, n, k,
                                                                 scales.shape[1], group_size, _dt(x_sorted), _stream(x_sorted)))
    return out


def moe_mlp_gate_up_cdna4(x_sorted, qweight_interleaved, scales, scaled_zeros, sz_packed, expert_offsets, group_size: int = 128, sz_half=None):
    """C-ABI awq_w4a16_moe_mlp_gate_up_cdna4: silu(x . W1_e^T) * (x . W3_e^T) for tokens sorted by expert, every expert's w1 / w3 rows
    interleaved 8 + 8 per slab (qweight int16 [E, 2F/4, K]); out [T, F].  One grouped launch from 256 sorted rows on."""
    _need_gpu(x_sorted, qweight_interleaved, scales, scaled_zeros, sz_packed, expert_offsets, sz_half)
    e, n2, k = qweight_interleaved.shape[0], qweight_interleaved.shape[1] * 4, qweight_interleaved.shape[2]
    t = x_sorted.shape[0]
    out = torch.empty(t, n2 // 2, dtype=x_sorted.dtype, device=x_sorted.device)
    # the fused grouped launch serves >= 256 sorted rows and needs no scratch; below that -- and whenever the launch declines a large call
    # (t * k or n * k / 8 beyond 2^31, knob moe_v6 = 0: AWQ_ERR_WORKSPACE) -- the unfused route wants a [T, 2F] buffer: allocate and retry once
    scratch = torch.empty(t, n2, dtype=x_sorted.dtype, device=x_sorted.device) if 0 < t < 256 else None
    with torch.cuda.device(x_sorted.device):
        for attempt in (0, 1):
            rc = _capi.lib().awq_w4a16_moe_mlp_gate_up_cdna4_szh(
                x_sorted.data_ptr(), qweight_interleaved.data_ptr(), scales.data_ptr(), scaled_zeros.data_ptr(), sz_packed.data_ptr(),
                sz_half.data_ptr() if sz_half is not None else None,
                expert_offsets.data_ptr(), out.data_ptr(), scratch.data_ptr() if scratch is not None else None,
                scratch.numel() * 2 if scratch is not None else 0, t, e, n2, k, scales.shape[1], group_size, _dt(x_sorted), _stream(x_sorted))
            if rc == _capi.AWQ_ERR_WORKSPACE and scratch is None and attempt == 0 and t > 0:
                scratch = torch.empty(t, n2, dtype=x_sorted.dtype, device=x_sorted.device)
                continue
            _capi.check(rc)
            break
    return out


def silu_mul(gate, up):
    """C-ABI awq_silu_mul: T(T(silu(gate)) * up), elementwise (fused_mlp.py:79-82)."""
    _need_gpu(gate, up)
    if gate.shape != up.shape or gate.dtype != up.dtype or gate.numel() % 8:
        raise ValueError("silu_mul: gate and up must have the same shape / dtype and a multiple of 8 elements")
    out = torch.empty_like(gate)
    with torch.cuda.device(gate.device):
        _capi.check(_capi.lib().awq_silu_mul(gate.data_ptr(), up.data_ptr(), out.data_ptr(), gate.numel(), _dt(gate), _stream(gate)))
    return out


# ---- MoE routing on the device (awq_moe_route_cdna4.hip): one launch each, nothing read back to the host ----

def moe_route(router_logits, top_k: int, renormalize: bool = True):
    """C-ABI awq_moe_route.  router_logits [T, E] (fp32 / bf16 / fp16) -> (topk_ids int32 [T, k], topk_w fp32 [T, k], order int32 [T k],
    inv int32 [T k], offsets int32 [E + 1]): the k largest logits of a row in descending order (ties: the lower index), their softmax weights
    (renormalize: over the k picked, Mixtral; else over all E), and the stable sort of the flat slots t k + j by expert -- `order` is
    moe.sort_by_expert's, `inv` its inverse, `offsets` the grouped launches' expert_offsets."""
    _need_gpu(router_logits)
    if router_logits.dim() != 2:
        raise ValueError("moe_route: router_logits must be [T, E]")
    code = {torch.float16: _capi.AWQ_F16, torch.bfloat16: _capi.AWQ_BF16, torch.float32: _capi.AWQ_F32}.get(router_logits.dtype)
    if code is None:
        raise TypeError(f"moe_route: expected float32/bfloat16/float16 logits, got {router_logits.dtype}")
    t, e = router_logits.shape
    k, dev = int(top_k), router_logits.device
    if k < 1:
        raise ValueError("moe_route: top_k must be at least 1")
    ids = torch.empty(t, k, dtype=torch.int32, device=dev)
    w = torch.empty(t, k, dtype=torch.float32, device=dev)
    order = torch.empty(t * k, dtype=torch.int32, device=dev)
    inv = torch.empty_like(order)
    offsets = torch.empty(e + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_moe_route(router_logits.data_ptr(), code, t, e, k, 1 if renormalize else 0, ids.data_ptr(), w.data_ptr(),
                                              order.data_ptr(), inv.data_ptr(), offsets.data_ptr(), _stream(router_logits)))
    return ids, w, order, inv, offsets


def moe_gather(x, order, top_k: int):
    """C-ABI awq_moe_gather: xs[r] = x[order[r] // top_k]; x [T, H] bf16 / fp16 with H % 8 == 0, order int32 [T top_k] -> xs [T top_k, H]."""
    _need_gpu(x, order)
    if x.dim() != 2 or order.dtype != torch.int32 or order.numel() != x.shape[0] * int(top_k):
        raise ValueError("moe_gather: x must be [T, H] and order int32 [T * top_k]")
    t, h = x.shape
    xs = torch.empty(order.numel(), h, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_moe_gather(x.data_ptr(), order.data_ptr(), xs.data_ptr(), t, int(top_k), h, _dt(x), _stream(x)))
    return xs


def moe_combine(ys, inv, topk_w):
    """C-ABI awq_moe_combine: out[t] = T(sum_j f32(T(f32(ys[inv[t k + j]]) * f32(T(topk_w[t, j]))))), summed in fp32 with j ascending, rounded
    once; ys [T k, H] bf16 / fp16 with H % 8 == 0, inv int32 [T k], topk_w fp32 [T, k] -> out [T, H] (every element written)."""
    _need_gpu(ys, inv, topk_w)
    if ys.dim() != 2 or topk_w.dim() != 2 or topk_w.dtype != torch.float32 or inv.dtype != torch.int32 or \
            inv.numel() != topk_w.numel() or ys.shape[0] != topk_w.numel():
        raise ValueError("moe_combine: ys must be [T * k, H], inv int32 [T * k] and topk_w float32 [T, k]")
    t, k = topk_w.shape
    h = ys.shape[1]
    out = torch.empty(t, h, dtype=ys.dtype, device=ys.device)
    with torch.cuda.device(ys.device):
        _capi.check(_capi.lib().awq_moe_combine(ys.data_ptr(), inv.data_ptr(), topk_w.data_ptr(), out.data_ptr(), t, k, h, _dt(ys), _stream(ys)))
    return out


# ---- next-token sampling on the device (awq_sample_cdna4.hip): one launch, nothing read back to the host ----

def sample_logits(logits, u, *, temperature=None, top_k=None, top_p=None, repetition_penalty=None, history=None, hist_len=None, seqlens=None,
                  stop_ids=None, finished=None, max_len=0, append=False, advance=False):
    """C-ABI awq_sample_logits.  logits [B, V] (fp32 / bf16 / fp16) and u fp32 [B] in [0, 1) -> tokens int32 [B]: temperature -> repetition penalty
    -> top-p -> top-k -> the first kept token whose running mass passes u times the kept mass (DESIGN.md "Sampling").  Every other argument is a
    per-row GPU tensor or None (= that step is off): temperature / top_p / repetition_penalty fp32 [B], top_k int32 [B], history int32 [B, Lh] with
    hist_len int32 [B], seqlens int32 [B] (negative = inactive slot, token -1), stop_ids int32 [S], finished int32 [B].  append / advance: the
    launch also writes the token into the history and moves seqlens on (-1 after a stop id or at max_len)."""
    params = (u, temperature, top_k, top_p, repetition_penalty, history, hist_len, seqlens, stop_ids, finished)
    _need_gpu(logits, *params)
    if logits.dim() != 2:
        raise ValueError("sample_logits: logits must be [B, V]")
    code = {torch.float16: _capi.AWQ_F16, torch.bfloat16: _capi.AWQ_BF16, torch.float32: _capi.AWQ_F32}.get(logits.dtype)
    if code is None:
        raise TypeError(f"sample_logits: expected float32/bfloat16/float16 logits, got {logits.dtype}")
    b, v = logits.shape
    for name, t, dt in (("u", u, torch.float32), ("temperature", temperature, torch.float32), ("top_p", top_p, torch.float32),
                        ("repetition_penalty", repetition_penalty, torch.float32), ("top_k", top_k, torch.int32),
                        ("hist_len", hist_len, torch.int32), ("seqlens", seqlens, torch.int32), ("finished", finished, torch.int32)):
        if t is not None and (t.dtype != dt or t.numel() != b or t.device != logits.device):
            raise ValueError(f"sample_logits: {name} must be {dt} [B] on the logits' device")
    if u is None:
        raise ValueError("sample_logits: u is required")
    if (history is None) != (hist_len is None):
        raise ValueError("sample_logits: history and hist_len come together")
    if history is not None and (history.dtype != torch.int32 or history.dim() != 2 or history.shape[0] != b or history.shape[1] < 1 or
                                history.device != logits.device):
        raise ValueError("sample_logits: history must be int32 [B, Lh] with Lh >= 1 on the logits' device")
    if stop_ids is not None and (stop_ids.dtype != torch.int32 or stop_ids.dim() != 1 or stop_ids.device != logits.device):
        raise ValueError("sample_logits: stop_ids must be int32 [S] on the logits' device")
    if append and history is None:
        raise ValueError("sample_logits: append needs history and hist_len")
    if advance and seqlens is None:
        raise ValueError("sample_logits: advance needs seqlens")
    tokens = torch.empty(b, dtype=torch.int32, device=logits.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    flags = (_capi.AWQ_SAMPLE_APPEND if append else 0) | (_capi.AWQ_SAMPLE_ADVANCE if advance else 0)
    with torch.cuda.device(logits.device):
        _capi.check(_capi.lib().awq_sample_logits(logits.data_ptr(), code, b, v, u.data_ptr(), ptr(temperature), ptr(top_k), ptr(top_p),
                                                  ptr(repetition_penalty), ptr(history), ptr(hist_len),
                                                  0 if history is None else history.shape[1], ptr(seqlens), ptr(stop_ids),
                                                  0 if stop_ids is None else stop_ids.numel(), ptr(finished), int(max_len), flags,
                                                  tokens.data_ptr(), _stream(logits)))
    return tokens


# ---- prompt-lookup speculative decoding on the device (awq_spec_cdna4.hip): four launches, nothing read back to the host ----

def _spec_i32(who, dev, **ts):
    """every given tensor: int32, contiguous, on the GPU `dev`"""
    for name, t in ts.items():
        if t is None:
            continue
        _need_gpu(t)
        if t.dtype != torch.int32 or t.device != dev:
            raise ValueError(f"{who}: {name} must be an int32 tensor on {dev}")


def spec_draft_ngram(history, hist_len, seqlens, *, vocab, kmax, ngram_min=1, ngram_max=3, max_len=2 ** 31 - 1, max_draft=None, drafts=None,
                     draft_len=None):
    """C-ABI awq_spec_draft_ngram: the prompt-lookup drafter over the sampler's history int32 [B, Lh] / hist_len [B] / seqlens [B] (-1 = inactive)
    -> (drafts int32 [B, kmax], -1 behind the draft; draft_len int32 [B]).  The longest earlier occurrence of the history's last n-gram
    (ngram_min .. ngram_max tokens, the most recent among equals) is continued for at most kmax / max_draft[b] tokens, never past the cache
    (max_len) and never over an id outside [0, vocab).  drafts / draft_len: persistent outputs to write into (a captured graph's)."""
    _need_gpu(history)
    dev = history.device
    _spec_i32("spec_draft_ngram", dev, history=history, hist_len=hist_len, seqlens=seqlens, max_draft=max_draft, drafts=drafts, draft_len=draft_len)
    if history.dim() != 2 or history.shape[1] < 1:
        raise ValueError("spec_draft_ngram: history must be int32 [B, Lh] with Lh >= 1")
    b, lh = history.shape
    for name, t in (("hist_len", hist_len), ("seqlens", seqlens), ("max_draft", max_draft), ("draft_len", draft_len)):
        if t is not None and t.numel() != b:
            raise ValueError(f"spec_draft_ngram: {name} must hold B values")
    kmax = int(kmax)
    if drafts is None:
        drafts = torch.empty(b, kmax, dtype=torch.int32, device=dev)
    elif tuple(drafts.shape) != (b, kmax):
        raise ValueError("spec_draft_ngram: drafts must be [B, kmax]")
    if draft_len is None:
        draft_len = torch.empty(b, dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_spec_draft_ngram(history.data_ptr(), hist_len.data_ptr(), seqlens.data_ptr(), ptr(max_draft),
                                                     drafts.data_ptr() if kmax > 0 else None, draft_len.data_ptr(), b, lh, int(vocab), kmax,
                                                     int(ngram_min), int(ngram_max), int(max_len), _stream(history)))
    return drafts, draft_len


def spec_pack(last_tokens, drafts, draft_len, seqlens, total_q, *, cu_seqlens_q=None, input_ids=None):
    """C-ABI awq_spec_pack: the layout of a speculative step.  last_tokens int32 [B] (what the previous sample_logits / spec_accept returned),
    drafts int32 [B, kmax] and draft_len int32 [B] (from any drafter; REWRITTEN to what the budget grants), seqlens int32 [B] -> (cu_seqlens_q int32
    [B + 1], input_ids int32 [total_q]).  Every active slot gets one row, the other total_q - A rows go to the drafts in slot order; the rows behind
    cu_seqlens_q[B] hold -1."""
    _need_gpu(last_tokens)
    dev = last_tokens.device
    _spec_i32("spec_pack", dev, last_tokens=last_tokens, drafts=drafts, draft_len=draft_len, seqlens=seqlens, cu_seqlens_q=cu_seqlens_q,
              input_ids=input_ids)
    b = last_tokens.numel()
    if drafts.dim() != 2 or drafts.shape[0] != b or draft_len.numel() != b or seqlens.numel() != b:
        raise ValueError("spec_pack: drafts must be [B, kmax], draft_len and seqlens [B]")
    kmax, total_q = drafts.shape[1], int(total_q)
    if cu_seqlens_q is None:
        cu_seqlens_q = torch.empty(b + 1, dtype=torch.int32, device=dev)
    elif cu_seqlens_q.numel() != b + 1:
        raise ValueError("spec_pack: cu_seqlens_q must be [B + 1]")
    if input_ids is None:
        input_ids = torch.empty(max(total_q, 0), dtype=torch.int32, device=dev)
    elif input_ids.numel() != total_q:
        raise ValueError("spec_pack: input_ids must be [total_q]")
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_spec_pack(last_tokens.data_ptr(), drafts.data_ptr() if kmax > 0 else None, draft_len.data_ptr(),
                                              seqlens.data_ptr(), cu_seqlens_q.data_ptr(), input_ids.data_ptr(), b, kmax, total_q,
                                              _stream(last_tokens)))
    return cu_seqlens_q, input_ids


def spec_verify(logits, u, cu_seqlens_q, input_ids, *, temperature=None, top_k=None, top_p=None, repetition_penalty=None, history=None,
                hist_len=None, row_tokens=None):
    """C-ABI awq_spec_verify: sample_logits' row routine on every row of a packed step.  logits [total_q, V] (fp32 / bf16 / fp16), u fp32 [total_q],
    cu_seqlens_q int32 [B + 1] and input_ids int32 [total_q] (spec_pack's) -> row_tokens int32 [total_q]: the token sample_logits would draw from
    the row with its owner's parameters ([B] tensors or None) and u[r], the penalty set being the owner's history plus the burst's earlier inputs
    (those the serial loop would have appended by then).  -1 for the padding rows.  Nothing is appended or advanced."""
    params = (u, temperature, top_k, top_p, repetition_penalty, history, hist_len, cu_seqlens_q, input_ids, row_tokens)
    _need_gpu(logits, *params)
    if logits.dim() != 2:
        raise ValueError("spec_verify: logits must be [total_q, V]")
    code = {torch.float16: _capi.AWQ_F16, torch.bfloat16: _capi.AWQ_BF16, torch.float32: _capi.AWQ_F32}.get(logits.dtype)
    if code is None:
        raise TypeError(f"spec_verify: expected float32/bfloat16/float16 logits, got {logits.dtype}")
    tq, v = logits.shape
    dev = logits.device
    _spec_i32("spec_verify", dev, cu_seqlens_q=cu_seqlens_q, input_ids=input_ids, top_k=top_k, history=history, hist_len=hist_len,
              row_tokens=row_tokens)
    b = cu_seqlens_q.numel() - 1
    if b < 1 or input_ids.numel() != tq or u is None or u.dtype != torch.float32 or u.numel() != tq or u.device != dev:
        raise ValueError("spec_verify: cu_seqlens_q must be [B + 1], input_ids int32 [total_q] and u float32 [total_q] on the logits' device")
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_p", top_p, torch.float32),
                        ("repetition_penalty", repetition_penalty, torch.float32), ("top_k", top_k, torch.int32), ("hist_len", hist_len, torch.int32)):
        if t is not None and (t.dtype != dt or t.numel() != b or t.device != dev):
            raise ValueError(f"spec_verify: {name} must be {dt} [B] on the logits' device")
    if (history is None) != (hist_len is None):
        raise ValueError("spec_verify: history and hist_len come together")
    if history is not None and (history.dim() != 2 or history.shape[0] != b or history.shape[1] < 1):
        raise ValueError("spec_verify: history must be int32 [B, Lh] with Lh >= 1")
    if row_tokens is None:
        row_tokens = torch.empty(tq, dtype=torch.int32, device=dev)
    elif row_tokens.numel() != tq:
        raise ValueError("spec_verify: row_tokens must be [total_q]")
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_spec_verify(logits.data_ptr(), code, tq, v, u.data_ptr(), cu_seqlens_q.data_ptr(), input_ids.data_ptr(), b,
                                                ptr(temperature), ptr(top_k), ptr(top_p), ptr(repetition_penalty), ptr(history), ptr(hist_len),
                                                0 if history is None else history.shape[1], row_tokens.data_ptr(), _stream(logits)))
    return row_tokens


def spec_accept(row_tokens, input_ids, cu_seqlens_q, kmax, *, history=None, hist_len=None, seqlens=None, stop_ids=None, finished=None, max_len=0,
                append=False, advance=False, out_tokens=None, num_emitted=None, last_tokens=None):
    """C-ABI awq_spec_accept: what a speculative step emits.  Per slot, the drafts (input_ids behind the slot's first row) are accepted while they
    equal the token sampled from the row before them; the samples up to and including the first mismatch (or the bonus token behind the last
    draft) are emitted, each through sample_logits' append / stop / advance, ending early once the slot has finished.  -> (out_tokens int32
    [B, kmax + 1] with -1 behind, num_emitted int32 [B], last_tokens int32 [B])."""
    _need_gpu(row_tokens)
    dev = row_tokens.device
    _spec_i32("spec_accept", dev, row_tokens=row_tokens, input_ids=input_ids, cu_seqlens_q=cu_seqlens_q, history=history, hist_len=hist_len,
              seqlens=seqlens, stop_ids=stop_ids, finished=finished, out_tokens=out_tokens, num_emitted=num_emitted, last_tokens=last_tokens)
    tq, b, kmax = row_tokens.numel(), cu_seqlens_q.numel() - 1, int(kmax)
    if b < 1 or input_ids.numel() != tq:
        raise ValueError("spec_accept: cu_seqlens_q must be [B + 1] and input_ids [total_q] like row_tokens")
    for name, t in (("hist_len", hist_len), ("seqlens", seqlens), ("finished", finished), ("num_emitted", num_emitted), ("last_tokens", last_tokens)):
        if t is not None and t.numel() != b:
            raise ValueError(f"spec_accept: {name} must hold B values")
    if (history is None) != (hist_len is None):
        raise ValueError("spec_accept: history and hist_len come together")
    if history is not None and (history.dim() != 2 or history.shape[0] != b or history.shape[1] < 1):
        raise ValueError("spec_accept: history must be int32 [B, Lh] with Lh >= 1")
    if append and history is None:
        raise ValueError("spec_accept: append needs history and hist_len")
    if advance and seqlens is None:
        raise ValueError("spec_accept: advance needs seqlens")
    if out_tokens is None:
        out_tokens = torch.empty(b, kmax + 1, dtype=torch.int32, device=dev)
    elif tuple(out_tokens.shape) != (b, kmax + 1):
        raise ValueError("spec_accept: out_tokens must be [B, kmax + 1]")
    num_emitted = torch.empty(b, dtype=torch.int32, device=dev) if num_emitted is None else num_emitted
    last_tokens = torch.empty(b, dtype=torch.int32, device=dev) if last_tokens is None else last_tokens
    ptr = lambda t: None if t is None else t.data_ptr()
    flags = (_capi.AWQ_SAMPLE_APPEND if append else 0) | (_capi.AWQ_SAMPLE_ADVANCE if advance else 0)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_spec_accept(row_tokens.data_ptr(), input_ids.data_ptr(), cu_seqlens_q.data_ptr(), b, tq, kmax, ptr(history),
                                                ptr(hist_len), 0 if history is None else history.shape[1], ptr(seqlens), ptr(stop_ids),
                                                0 if stop_ids is None else stop_ids.numel(), ptr(finished), int(max_len), flags,
                                                out_tokens.data_ptr(), num_emitted.data_ptr(), last_tokens.data_ptr(), _stream(row_tokens)))
    return out_tokens, num_emitted, last_tokens


# ---- LM head for decode and the token embedding gather (awq_lm_head_cdna4.hip) ----

def lm_head_plan(m: int, v: int, k: int) -> dict:
    """C-ABI awq_lm_head_plan (host only): the launch shape awq_lm_head takes for [m, k] x [v, k]."""
    import ctypes
    out = (ctypes.c_int * 4)()
    _capi.check(_capi.lib().awq_lm_head_plan(int(m), int(v), int(k), out))
    return {"blocks": out[0], "tile_rows": out[1], "waves": out[2], "k_split": out[3]}


def lm_head(x, weight, gamma=None, eps=0.0, bias=None, seqlens=None, out=None, out_dtype=torch.float32, max_blocks=0):
    """C-ABI awq_lm_head: logits [M, V] = rmsnorm(x)[M, K] @ weight[V, K]^T (+ bias) in one launch that reads the weights once for 1 <= M <= 64.
    x: [M, K] or a strided view with a contiguous last dimension (h[:, -1, :]): the row stride is passed on, nothing is copied.  gamma [K] (None:
    no norm), bias [V], weight as nn.Linear holds it.  seqlens int32 [M]: rows with a negative entry are left untouched in `out` (a fresh `out`
    is then allocated zeroed).  out_dtype: torch.float32 (what sample_logits should be fed) or x.dtype."""
    return _lm_head(x, weight, gamma, eps, bias, seqlens, out, out_dtype, max_blocks, None)


def lm_head_softcap(x, weight, softcap, gamma=None, eps=0.0, bias=None, seqlens=None, out=None, out_dtype=torch.float32, max_blocks=0):
    """C-ABI awq_lm_head_softcap: `lm_head` with every logit capped in the launch's epilogue, y <- softcap * tanh(y / softcap) on the fp32 sum behind
    the bias and before the one rounding to out_dtype (Gemma-2's final_logit_softcapping = 30).  With out_dtype float32 the result carries the bits of
    `logit_softcap_(lm_head(...), softcap)`.  softcap: a finite float >= 0; 0 is "no cap" and returns the bits of `lm_head`.  A function of its own:
    `lm_head` keeps its parameter list."""
    return _lm_head(x, weight, gamma, eps, bias, seqlens, out, out_dtype, max_blocks, _check_softcap("lm_head_softcap", softcap))


def logit_softcap_(logits, softcap, seqlens=None):
    """C-ABI awq_logit_softcap: logits [B, V] that already exist (fp32 / bf16 / fp16, any row stride, contiguous last dimension) capped IN PLACE,
    z <- softcap * tanh(z / softcap), computed in fp32 and rounded once.  seqlens int32 [B]: rows with a negative entry are left untouched.
    softcap: a finite float >= 0; 0 changes nothing.  Returns `logits`."""
    if logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("logit_softcap_: logits must be a [B, V] GPU tensor")
    codes = {torch.float16: _capi.AWQ_F16, torch.bfloat16: _capi.AWQ_BF16, torch.float32: _capi.AWQ_F32}
    if logits.dtype not in codes:
        raise TypeError(f"logit_softcap_: logits must be float32, bfloat16 or float16, got {logits.dtype}")
    cap = _check_softcap("logit_softcap_", softcap)
    b, v = logits.shape
    if logits.stride(1) != 1 and v > 1:
        raise ValueError("logit_softcap_: the last dimension of logits must be contiguous")
    if seqlens is not None and (seqlens.dtype != torch.int32 or seqlens.numel() != b or seqlens.device != logits.device or not seqlens.is_contiguous()):
        raise ValueError("logit_softcap_: seqlens must be contiguous int32 [B] on the logits' device")
    ld = logits.stride(0) if b > 1 else max(logits.stride(0), v)
    with torch.cuda.device(logits.device):
        _capi.check(_capi.lib().awq_logit_softcap(logits.data_ptr(), codes[logits.dtype], ld, None if seqlens is None else seqlens.data_ptr(), b, v,
                                                  cap, _stream(logits)))
    return logits


def _lm_head(x, weight, gamma, eps, bias, seqlens, out, out_dtype, max_blocks, softcap):
    """The body of `lm_head` (softcap None) and `lm_head_softcap` (softcap a checked float)."""
    if x.dim() != 2 or weight.dim() != 2:
        raise ValueError("lm_head: x must be [M, K] and weight [V, K]")
    for t in (x, weight, gamma, bias, seqlens, out):
        if t is not None and not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    _need_gpu(weight, gamma, bias, seqlens, out)
    m, k = x.shape
    v = weight.shape[0]
    if x.stride(1) != 1 and k > 1:
        raise ValueError("lm_head: the last dimension of x must be contiguous")
    if weight.shape[1] != k or weight.dtype != x.dtype:
        raise ValueError("lm_head: weight must be [V, K] of x's dtype")
    for name, t, n in (("gamma", gamma, k), ("bias", bias, v)):
        if t is not None and (t.dtype != x.dtype or t.numel() != n or t.device != x.device):
            raise ValueError(f"lm_head: {name} must hold {n} values of x's dtype on x's device")
    if seqlens is not None and (seqlens.dtype != torch.int32 or seqlens.numel() != m or seqlens.device != x.device):
        raise ValueError("lm_head: seqlens must be int32 [M] on x's device")
    if out_dtype not in (torch.float32, x.dtype):
        raise TypeError(f"lm_head: out_dtype must be torch.float32 or {x.dtype}, got {out_dtype}")
    if out is None:
        out = (torch.zeros if seqlens is not None else torch.empty)((m, v), dtype=out_dtype, device=x.device)
    elif out.shape != (m, v) or out.dtype != out_dtype or out.device != x.device:
        raise ValueError("lm_head: out must be a contiguous [M, V] tensor of out_dtype on x's device")
    ldx = x.stride(0) if m > 1 else max(x.stride(0), k) // 8 * 8  # (a single row's stride is never used)
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (x.data_ptr(), ldx, ptr(gamma), float(eps), weight.data_ptr(), ptr(bias), ptr(seqlens), out.data_ptr(),
            _capi.AWQ_F32 if out_dtype == torch.float32 else _dt(x), m, v, k, _dt(x))
    with torch.cuda.device(x.device):
        if softcap is None:
            _capi.check(_capi.lib().awq_lm_head(*head, int(max_blocks), _stream(x)))
        else:
            _capi.check(_capi.lib().awq_lm_head_softcap(*head, softcap, int(max_blocks), _stream(x)))
    return out


def embed_tokens(tokens, table):
    """C-ABI awq_embed_tokens: out[i] = table[tokens[i]] for tokens int32 [...] and table [V, K]; ZEROS for an id outside [0, V) (-1 is the sampler's
    finished slot).  Returns [..., K]."""
    _need_gpu(tokens, table)
    if tokens.dtype != torch.int32 or table.dim() != 2 or tokens.device != table.device:
        raise ValueError("embed_tokens: tokens must be int32 and table [V, K], on one device")
    v, k = table.shape
    out = torch.empty(*tokens.shape, k, dtype=table.dtype, device=table.device)
    if tokens.numel() == 0:
        return out
    with torch.cuda.device(table.device):
        _capi.check(_capi.lib().awq_embed_tokens(tokens.data_ptr(), table.data_ptr(), out.data_ptr(), tokens.numel(), v, k, _dt(table),
                                                 _stream(table)))
    return out


# ---- token log-probabilities: the LM head fused with log-sum-exp (awq_lm_logprobs_cdna4.hip) ----

_LOGPROB_OUTPUTS = ("logprob", "lse", "target_logit", "argmax")


def lm_head_logprobs_plan(t: int, v: int, k: int) -> dict:
    """C-ABI awq_lm_head_logprobs_plan (host only): the tiles awq_lm_head_logprobs cuts [t, k] x [v, k] into."""
    import ctypes
    out = (ctypes.c_int * 4)()
    _capi.check(_capi.lib().awq_lm_head_logprobs_plan(int(t), int(v), int(k), out))
    return {"row_tile": out[0], "vocab_tile": out[1], "blocks": out[2], "k_step": out[3]}


def lm_head_logprobs_workspace_bytes(t: int, v: int, k: int, with_gamma: bool = False) -> int:
    """C-ABI awq_lm_head_logprobs_workspace_bytes (host only)."""
    return int(_capi.lib().awq_lm_head_logprobs_workspace_bytes(int(t), int(v), int(k), int(bool(with_gamma))))


def _logprob_outputs(who, n, device, targets, want, out):
    want = tuple(want)
    for name in want:
        if name not in _LOGPROB_OUTPUTS:
            raise ValueError(f"{who}: unknown output {name!r} (one of {_LOGPROB_OUTPUTS})")
        if targets is None and name in ("logprob", "target_logit"):
            raise ValueError(f"{who}: {name} needs targets")
    res = {}
    for name in want:
        dt = torch.int32 if name == "argmax" else torch.float32
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.zeros(n, dtype=dt, device=device)
        elif t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{who}: out[{name!r}] must be a contiguous {dt} tensor of {n} values on the inputs' device")
        res[name] = t
    return res


def lm_head_logprobs(x, weight, targets=None, gamma=None, eps=0.0, bias=None, round_logits=False, ws=None, want=("logprob", "lse"), out=None,
                     max_blocks=0, *, softcap=0.0):
    """C-ABI awq_lm_head_logprobs: per row of x [T, K], against weight [V, K] (nn.Linear.weight as loaded): lse = log sum_v exp(z), target_logit =
    z[targets], logprob = target_logit - lse and argmax (lowest index among the maxima) of z = rmsnorm(x) @ weight^T (+ bias), without the logits ever
    being written to memory.  round_logits: every z is rounded once to x's dtype first, as an nn.Linear would store it.  targets int32 [T]: a row
    whose target is outside [0, V) (-1, -100) is ignored -- its outputs keep what they held (zeros in fresh ones).  x may be a strided view with a
    contiguous last dimension when gamma is None.  ws: a uint8 workspace of at least lm_head_logprobs_workspace_bytes (allocated when None; pass
    one, and `out`, to capture the call).  Returns a dict with the outputs named in `want`: fp32 [T], argmax int32 [T].

    softcap (keyword-only; C-ABI awq_lm_head_logprobs_softcap): every z is capped, z <- softcap * tanh(z / softcap) in fp32, before it enters the
    max / sum-exp, the target pick and the argmax (Gemma-2's final_logit_softcapping = 30); with round_logits z is rounded to x's dtype, capped in
    fp32 and rounded once more.  A finite float >= 0; 0 (the default) is no cap, the uncapped entry."""
    softcap = _check_softcap("lm_head_logprobs", softcap)
    if x.dim() != 2 or weight.dim() != 2:
        raise ValueError("lm_head_logprobs: x must be [T, K] and weight [V, K]")
    for t in (x, weight, gamma, bias, targets, ws):
        if t is not None and not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    n, k = x.shape
    v = weight.shape[0]
    if weight.shape[1] != k or weight.dtype != x.dtype or not weight.is_contiguous():
        raise ValueError("lm_head_logprobs: weight must be a contiguous [V, K] tensor of x's dtype")
    if gamma is not None:
        x = x.contiguous()
    elif x.stride(1) != 1 and k > 1:
        raise ValueError("lm_head_logprobs: the last dimension of x must be contiguous")
    for name, t, cnt in (("gamma", gamma, k), ("bias", bias, v)):
        if t is not None and (t.dtype != x.dtype or t.numel() != cnt or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"lm_head_logprobs: {name} must hold {cnt} contiguous values of x's dtype on x's device")
    if targets is not None and (targets.dtype != torch.int32 or targets.numel() != n or targets.device != x.device or not targets.is_contiguous()):
        raise ValueError("lm_head_logprobs: targets must be contiguous int32 [T] on x's device")
    res = _logprob_outputs("lm_head_logprobs", n, x.device, targets, want, out)
    need = lm_head_logprobs_workspace_bytes(n, v, k, gamma is not None)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif ws.dtype != torch.uint8 or ws.numel() < need or ws.device != x.device or not ws.is_contiguous():
        raise ValueError(f"lm_head_logprobs: ws must be a contiguous uint8 tensor of at least {need} bytes on x's device")
    ldx = x.stride(0) if n > 1 else max(x.stride(0), k) // 8 * 8  # (a single row's stride is never used)
    if gamma is not None:
        ldx = k
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (x.data_ptr(), ldx, ptr(gamma), float(eps), weight.data_ptr(), ptr(bias), ptr(targets), ptr(res.get("logprob")), ptr(res.get("lse")),
            ptr(res.get("target_logit")), ptr(res.get("argmax")), n, v, k, _dt(x), int(bool(round_logits)))
    tail = (ws.data_ptr(), ws.numel(), int(max_blocks), _stream(x))
    with torch.cuda.device(x.device):
        if softcap == 0.0:
            _capi.check(_capi.lib().awq_lm_head_logprobs(*head, *tail))
        else:
            _capi.check(_capi.lib().awq_lm_head_logprobs_softcap(*head, softcap, *tail))
    return res


def token_logprobs(logits, targets=None, want=None, out=None):
    """C-ABI awq_token_logprobs: lse, argmax and (with targets) logprob = logits[b, targets[b]] - lse[b] for logits [B, V] that already exist (fp32 /
    bf16 / fp16, any row stride, contiguous last dimension) -- what ops.lm_head hands to the sampler.  Same contract as lm_head_logprobs: rows whose
    target is outside [0, V) are ignored.  Returns a dict (default: lse, argmax, and logprob when targets is given)."""
    if logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("token_logprobs: logits must be a [B, V] GPU tensor")
    codes = {torch.float16: _capi.AWQ_F16, torch.bfloat16: _capi.AWQ_BF16, torch.float32: _capi.AWQ_F32}
    if logits.dtype not in codes:
        raise TypeError(f"token_logprobs: logits must be float32, bfloat16 or float16, got {logits.dtype}")
    b, v = logits.shape
    if logits.stride(1) != 1 and v > 1:
        raise ValueError("token_logprobs: the last dimension of logits must be contiguous")
    if targets is not None and (targets.dtype != torch.int32 or targets.numel() != b or targets.device != logits.device or not targets.is_contiguous()):
        raise ValueError("token_logprobs: targets must be contiguous int32 [B] on the logits' device")
    if want is None:
        want = ("lse", "argmax") + (("logprob",) if targets is not None else ())
    if "target_logit" in want:
        raise ValueError("token_logprobs: the target logit is logits[b, targets[b]] itself; it is not an output")
    res = _logprob_outputs("token_logprobs", b, logits.device, targets, want, out)
    ld = logits.stride(0) if b > 1 else max(logits.stride(0), v)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(logits.device):
        _capi.check(_capi.lib().awq_token_logprobs(logits.data_ptr(), codes[logits.dtype], ld, ptr(targets), ptr(res.get("logprob")),
                                                   ptr(res.get("lse")), ptr(res.get("argmax")), b, v, _stream(logits)))
    return res


# ---- multi-LoRA on packed steps: per-sequence adapters, read on the device (awq_lora_cdna4.hip) ----

def lora_plan(k: int, r: int, n_slices: int = 1) -> dict:
    """C-ABI awq_lora_plan (host only): the K split of the shrink launch and the shape of both launches for in_features k, pool rank r and
    n_slices output slices.  A function of (k, r * n_slices) alone: split s sums k in [s * k_per_split, min(k, (s + 1) * k_per_split))."""
    import ctypes
    out = (ctypes.c_int * 4)()
    _capi.check(_capi.lib().awq_lora_plan(int(k), int(r), int(n_slices), out))
    return {"k_splits": out[0], "k_per_split": out[1], "col_tile": out[2], "waves": out[3]}


def lora_workspace_bytes(total_q: int, k: int, r: int, n_slices: int = 1) -> int:
    """C-ABI awq_lora_workspace_bytes (host only): bytes of the fp32 [k_splits, total_q, n_slices * r] workspace; 0 for sizes outside the limits."""
    return int(_capi.lib().awq_lora_workspace_bytes(int(total_q), int(k), int(r), int(n_slices)))


def _lora_rows(who, name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.AwqNativeError(f"{who}: {name} must be a GPU tensor (llm_awq_amd ops run on the GPU only, no CPU fallback)")
    if t.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{who}: {name} must be float16 or bfloat16, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{who}: {name} must be a [total_q, features] matrix with at least one row")


def _lora_pool(who, name, t, ref, shape):
    if not t.is_cuda:
        raise _capi.AwqNativeError(f"{who}: {name} must be a GPU tensor (llm_awq_amd ops run on the GPU only, no CPU fallback)")
    if t.dtype != ref.dtype or t.device != ref.device:
        raise TypeError(f"{who}: {name} must have the rows' dtype {ref.dtype} and device, got {t.dtype} on {t.device}")
    if t.dim() != 3 or not t.is_contiguous() or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{who}: {name} must be a contiguous {list(shape)} tensor (None = any), got {list(t.shape)}")


def _lora_batch(who, ref, adapter_ids, cu_seqlens_q, max_seqlen_q):
    """adapter_ids int32 [B] and the optional cu_seqlens_q int32 [B + 1] of a step whose packed rows are `ref`; returns B"""
    for name, t in (("adapter_ids", adapter_ids), ("cu_seqlens_q", cu_seqlens_q)):
        if t is None:
            continue
        if not t.is_cuda:
            raise _capi.AwqNativeError(f"{who}: {name} must be a GPU tensor (it is read on the device, never by the host)")
        if t.dtype != torch.int32:
            raise TypeError(f"{who}: {name} must be int32, got {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous() or t.device != ref.device:
            raise ValueError(f"{who}: {name} must be a contiguous 1-D tensor on the rows' GPU")
    b = adapter_ids.shape[0]
    if b < 1 or b > 65535:
        raise ValueError(f"{who}: adapter_ids must hold 1 .. 65535 sequences, got {b}")
    if int(max_seqlen_q) < 1:
        raise ValueError(f"{who}: max_seqlen_q >= 1 is expected")
    if cu_seqlens_q is not None and cu_seqlens_q.shape[0] != b + 1:
        raise ValueError(f"{who}: cu_seqlens_q must be int32 [B + 1] = [{b + 1}], got {list(cu_seqlens_q.shape)}")
    if cu_seqlens_q is None and b * int(max_seqlen_q) != ref.shape[0]:
        raise ValueError(f"{who}: without cu_seqlens_q the rows are rectangular: {ref.shape[0]} rows != B * max_seqlen_q = {b * int(max_seqlen_q)}")
    return b


def _lora_ws(who, ws, ref, need):
    if ws is None:
        return torch.empty(need // 4, dtype=torch.float32, device=ref.device)
    if not ws.is_cuda or ws.device != ref.device or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError(f"{who}: ws must be a contiguous float32 tensor on the rows' GPU")
    if ws.numel() * 4 < need:
        raise ValueError(f"{who}: ws holds {ws.numel() * 4} bytes, lora_workspace_bytes asks for {need}")
    return ws


def lora_shrink(x, a_pool, adapter_ids, rank: int, cu_seqlens_q=None, max_seqlen_q: int = 1, ws=None):
    """C-ABI awq_lora_shrink: ws[s, t, :] = sum over the k of split s of x[t, k] * A_a[:, k] in fp32, a = adapter_ids[owner of row t].
    x [total_q, K] (a row-strided view is passed on, nothing is copied), a_pool [S, n_slices * rank, K].  Rows without an adapter, padding rows and
    the rows of inactive sequences are neither read nor written.  Returns ws (allocated when None)."""
    who = "lora_shrink"
    _lora_rows(who, "x", x)
    k = x.shape[1]
    if x.stride(1) != 1 and k > 1:
        raise ValueError(f"{who}: the last dimension of x must be contiguous")
    _lora_pool(who, "a_pool", a_pool, x, (None, None, k))
    rs = a_pool.shape[1]
    if int(rank) < 1 or rs % int(rank) != 0:
        raise ValueError(f"{who}: a_pool holds {rs} rows per slot, not a multiple of rank {rank}")
    b = _lora_batch(who, x, adapter_ids, cu_seqlens_q, max_seqlen_q)
    total_q, n_slices = x.shape[0], rs // int(rank)
    lora_plan(k, rank, n_slices)  # refuses the shape before anything is allocated
    ws = _lora_ws(who, ws, x, lora_workspace_bytes(total_q, k, rank, n_slices))
    ldx = x.stride(0) if total_q > 1 else max(x.stride(0), k) // 8 * 8
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_lora_shrink(x.data_ptr(), ldx, a_pool.data_ptr(), adapter_ids.data_ptr(),
                                                None if cu_seqlens_q is None else cu_seqlens_q.data_ptr(), ws.data_ptr(), ws.numel() * 4, b,
                                                int(max_seqlen_q), total_q, a_pool.shape[0], k, int(rank), n_slices, _dt(x), _stream(x)))
    return ws


def lora_expand(ws, b_pool, scaling, adapter_ids, y, k: int, slice_end=None, cu_seqlens_q=None, max_seqlen_q: int = 1):
    """C-ABI awq_lora_expand: y[t, n] = T(y[t, n] + sum_r hT[t, j(n) R + r] * B_a[n, r]) in place, hT = T(scaling[a] * sum_s ws[s, t, :]).
    b_pool [S, N, R], scaling float32 [S], slice_end: the ends of the output slices (default (N,)), k: the in_features the shrink launch summed
    over (it fixes the number of K splits)."""
    who = "lora_expand"
    _lora_rows(who, "y", y)
    if not y.is_contiguous():
        raise ValueError(f"{who}: y must be contiguous (it is updated in place)")
    total_q, n = y.shape
    _lora_pool(who, "b_pool", b_pool, y, (None, n, None))
    s, _, r = b_pool.shape
    if not scaling.is_cuda:
        raise _capi.AwqNativeError(f"{who}: scaling must be a GPU tensor (llm_awq_amd ops run on the GPU only, no CPU fallback)")
    if scaling.dtype != torch.float32 or scaling.numel() != s or scaling.device != y.device or not scaling.is_contiguous():
        raise ValueError(f"{who}: scaling must be a contiguous float32 [S] = [{s}] tensor on y's GPU")
    ends = [n] if slice_end is None else [int(e) for e in slice_end]
    if not 1 <= len(ends) <= 3:
        raise ValueError(f"{who}: slice_end must hold 1 .. 3 column ends, got {len(ends)}")
    b = _lora_batch(who, y, adapter_ids, cu_seqlens_q, max_seqlen_q)
    lora_plan(k, r, len(ends))
    need = lora_workspace_bytes(total_q, k, r, len(ends))
    if ws is None:
        raise ValueError(f"{who}: ws (the output of lora_shrink) is required")
    _lora_ws(who, ws, y, need)
    import ctypes
    with torch.cuda.device(y.device):
        _capi.check(_capi.lib().awq_lora_expand(ws.data_ptr(), ws.numel() * 4, b_pool.data_ptr(), scaling.data_ptr(), adapter_ids.data_ptr(),
                                                None if cu_seqlens_q is None else cu_seqlens_q.data_ptr(), y.data_ptr(), b, int(max_seqlen_q),
                                                total_q, s, n, int(k), r, (ctypes.c_int * len(ends))(*ends), len(ends), _dt(y), _stream(y)))
    return y


def lora_apply(x, y, a_pool, b_pool, scaling, adapter_ids, slice_end=None, cu_seqlens_q=None, max_seqlen_q: int = 1, ws=None):
    """Both launches: y[t, :] += scaling[a] * (x[t, :] @ A_a^T) @ B_a^T in place for a = adapter_ids[owner of row t]; every other row of y keeps its
    bits.  x [total_q, K], y [total_q, N] (the base linear's output), a_pool [S, n_slices * R, K], b_pool [S, N, R], scaling float32 [S],
    adapter_ids int32 [B] (outside [0, S): no adapter), slice_end: the ends of the output slices (multiples of 16, last == N; default one slice),
    cu_seqlens_q int32 [B + 1] (None: B sequences of max_seqlen_q rows each).  Nothing is read by the host: the pair can be captured with a
    workspace allocated beforehand (`ws`, lora_workspace_bytes).  Returns y."""
    _lora_rows("lora_apply", "x", x)
    _lora_rows("lora_apply", "y", y)
    if x.shape[0] != y.shape[0] or x.dtype != y.dtype or x.device != y.device:
        raise ValueError("lora_apply: x and y must hold the same rows, dtype and device")
    _lora_pool("lora_apply", "b_pool", b_pool, y, (None, y.shape[1], None))
    r = b_pool.shape[2]
    n_slices = 1 if slice_end is None else len(slice_end)
    _lora_pool("lora_apply", "a_pool", a_pool, x, (b_pool.shape[0], n_slices * r, x.shape[1]))
    ws = lora_shrink(x, a_pool, adapter_ids, r, cu_seqlens_q, max_seqlen_q, ws)
    return lora_expand(ws, b_pool, scaling, adapter_ids, y, x.shape[1], slice_end, cu_seqlens_q, max_seqlen_q)


def lora_expand_gate_up(ws, b_pool, scaling, adapter_ids, y2, k: int, h=None, cu_seqlens_q=None, max_seqlen_q: int = 1):
    """C-ABI awq_lora_expand_gate_up: the expand launch on QuantLlamaMLP's gate / up pair, fused with the SiLU * mul tail.  y2 [total_q, 2F] is the
    output of the 8 + 8 interleaved gate / up stream WITHOUT its epilogue (columns 16 j .. 16 j + 7 gate rows 8 j .., 16 j + 8 .. 16 j + 15 the
    matching up rows; read only), ws the shrink launch's workspace with n_slices = 2 (gate's A first), b_pool [S, 2F, R] in natural order (B_gate
    rows, then B_up rows).  h[t, f] = T(T(silu(g')) * u') with g' / u' the pair plus its deltas, one rounding each; rows of an active sequence
    without an adapter get the plain tail, every other row of h is not written.  Returns h [total_q, F] (allocated when None)."""
    who = "lora_expand_gate_up"
    _lora_rows(who, "y2", y2)
    if not y2.is_contiguous():
        raise ValueError(f"{who}: y2 must be contiguous")
    total_q, n2 = y2.shape
    if n2 < 16 or n2 % 16:
        raise ValueError(f"{who}: y2 must hold 2F columns, a multiple of 16 (the 8 + 8 interleaved pair), got {n2}")
    _lora_pool(who, "b_pool", b_pool, y2, (None, n2, None))
    s, _, r = b_pool.shape
    if not scaling.is_cuda:
        raise _capi.AwqNativeError(f"{who}: scaling must be a GPU tensor (llm_awq_amd ops run on the GPU only, no CPU fallback)")
    if scaling.dtype != torch.float32 or scaling.numel() != s or scaling.device != y2.device or not scaling.is_contiguous():
        raise ValueError(f"{who}: scaling must be a contiguous float32 [S] = [{s}] tensor on y2's GPU")
    b = _lora_batch(who, y2, adapter_ids, cu_seqlens_q, max_seqlen_q)
    lora_plan(k, r, 2)
    if ws is None:
        raise ValueError(f"{who}: ws (the output of lora_shrink with two slices) is required")
    _lora_ws(who, ws, y2, lora_workspace_bytes(total_q, k, r, 2))
    if h is None:
        h = torch.empty(total_q, n2 // 2, dtype=y2.dtype, device=y2.device)
    elif (not isinstance(h, torch.Tensor) or not h.is_cuda or h.dtype != y2.dtype or h.device != y2.device or tuple(h.shape) != (total_q, n2 // 2)
          or not h.is_contiguous()):
        raise ValueError(f"{who}: h must be a contiguous [{total_q}, {n2 // 2}] tensor of y2's dtype on y2's GPU")
    with torch.cuda.device(y2.device):
        _capi.check(_capi.lib().awq_lora_expand_gate_up(ws.data_ptr(), ws.numel() * 4, b_pool.data_ptr(), scaling.data_ptr(), adapter_ids.data_ptr(),
                                                        None if cu_seqlens_q is None else cu_seqlens_q.data_ptr(), y2.data_ptr(), h.data_ptr(), b,
                                                        int(max_seqlen_q), total_q, s, n2, int(k), r, _dt(y2), _stream(y2)))
    return h


def lora_apply_gate_up(x, y2, a_pool, b_pool, scaling, adapter_ids, cu_seqlens_q=None, max_seqlen_q: int = 1, ws=None, h=None):
    """Shrink with two slices plus lora_expand_gate_up: h = silu(gate + delta_gate) * (up + delta_up) for QuantLlamaMLP's pair.  x [total_q, K],
    y2 [total_q, 2F] (the interleaved stream's unfused output, read only), a_pool [S, 2R, K] (gate's A rows first), b_pool [S, 2F, R] (B_gate rows,
    then B_up rows), scaling float32 [S], adapter_ids int32 [B], cu_seqlens_q int32 [B + 1] or None.  x is read once for both projections; no
    [total_q, 2F] adapted intermediate is written.  The bits are those of lora_apply with slice_end = (F, 2F) on the de-interleaved pair followed
    by silu_mul (F % 16 == 8: with each slice zero-padded to whole 16-column groups, which lora_expand asks of its slice ends).  Returns h [total_q, F]."""
    who = "lora_apply_gate_up"
    _lora_rows(who, "x", x)
    _lora_rows(who, "y2", y2)
    if x.shape[0] != y2.shape[0] or x.dtype != y2.dtype or x.device != y2.device:
        raise ValueError(f"{who}: x and y2 must hold the same rows, dtype and device")
    _lora_pool(who, "b_pool", b_pool, y2, (None, y2.shape[1], None))
    r = b_pool.shape[2]
    _lora_pool(who, "a_pool", a_pool, x, (b_pool.shape[0], 2 * r, x.shape[1]))
    ws = lora_shrink(x, a_pool, adapter_ids, r, cu_seqlens_q, max_seqlen_q, ws)
    return lora_expand_gate_up(ws, b_pool, scaling, adapter_ids, y2, x.shape[1], h, cu_seqlens_q, max_seqlen_q)


# ---- AWQ quantisation: group quantiser + packer and clip search (awq_quant_cdna4.hip) ----

def _quant_weight(who, w):
    if w.dim() != 2:
        raise ValueError(f"{who}: w must be [N, K]")
    if not w.is_cuda:
        raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    _dt(w)
    n, k = w.shape
    if k < 128 or k % 128:
        raise ValueError(f"{who}: in_features must be a multiple of 128 (group size 128 only)")
    if w.stride(1) != 1 or (n > 1 and (w.stride(0) < k or w.stride(0) % 8)):
        raise ValueError(f"{who}: rows must be contiguous with a stride that is a multiple of 8 elements")
    return n, k


def quantize_pack(w, col_scale=None, clip_max=None, n_bit: int = 4, layout: str = "cdna4", *, w_fake=False, scales=True, scaled_zeros=True,
                  zeros=False, qweight=True) -> dict:
    """C-ABI awq_quantize_group: the per-group grid of pseudo_quantize_tensor(zero_point=True), group size 128, on w T [N, K] (rows may be
    strided) in one launch, bit-identical to the torch composition on T tensors.  col_scale T [K]: v = w * col_scale first, and w_fake is divided
    by it again; clip_max T [N, K/128] (or [N, K/128, 1]): v is clamped to +-clip_max.  Each output is False / None (not wanted), True (allocated)
    or a tensor to write into: w_fake T [N, K], scales / scaled_zeros T [gpad, N] (WQLinear's buffers), zeros T [N, K/128], qweight int16
    [N/4, K] in `layout` "cdna4" or "v2" (n_bit 4 only).  Returns {name: tensor} of the requested outputs."""
    n, k = _quant_weight("quantize_pack", w)
    if layout not in ("cdna4", "v2"):
        raise ValueError('quantize_pack: layout must be "cdna4" or "v2"')
    g = k // 128
    gpad = -(-g // 8) * 8
    if clip_max is not None and clip_max.dim() == 3:
        clip_max = clip_max.reshape(n, g)
    for name, t, numel in (("col_scale", col_scale, k), ("clip_max", clip_max, n * g)):
        if t is not None and (not t.is_cuda or t.dtype != w.dtype or t.numel() != numel or t.device != w.device or not t.is_contiguous()):
            raise ValueError(f"quantize_pack: {name} must hold {numel} contiguous values of w's dtype on w's device")
    spec = {"w_fake": (w_fake, (n, k), w.dtype), "scales": (scales, (gpad, n), w.dtype), "scaled_zeros": (scaled_zeros, (gpad, n), w.dtype),
            "zeros": (zeros, (n, g), w.dtype), "qweight": (qweight, (n // 4, k), torch.int16)}
    out = {}
    for name, (want, shape, dtype) in spec.items():
        if want is None or want is False:
            continue
        if want is True:
            out[name] = torch.empty(shape, dtype=dtype, device=w.device)
        elif tuple(want.shape) != shape or want.dtype != dtype or want.device != w.device or not want.is_contiguous():
            raise ValueError(f"quantize_pack: {name} must be a contiguous {shape} tensor of {dtype} on w's device")
        else:
            out[name] = want
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(w.device):
        _capi.check(_capi.lib().awq_quantize_group(w.data_ptr(), w.stride(0) if n > 1 else k, ptr(col_scale), ptr(clip_max), ptr(out.get("w_fake")),
                                                   ptr(out.get("scales")), ptr(out.get("scaled_zeros")), ptr(out.get("zeros")),
                                                   ptr(out.get("qweight")), 1 if layout == "cdna4" else 0, n, k, 128, int(n_bit), _dt(w),
                                                   _stream(w)))
    return out


def clip_search(w, x, n_bit: int = 4, n_grid: int = 20, n_steps: int = 10, return_err: bool = False):
    """C-ABI awq_clip_search: auto_clip_layer's search for w T [N, K] against tokens x T [S, K] (rows of either may be strided) in one launch.
    Returns (best_max_val T [N, K/128], best_idx int32 [N, K/128]) and, with return_err, the table err fp32 [N, K/128, n_steps]."""
    n, k = _quant_weight("clip_search", w)
    if x.dim() != 2 or not x.is_cuda or x.dtype != w.dtype or x.device != w.device or x.shape[1] != k or x.shape[0] < 1:
        raise ValueError("clip_search: x must be a [S, K] GPU tensor of w's dtype on w's device, S >= 1")
    s = x.shape[0]
    if x.stride(1) != 1 or (s > 1 and (x.stride(0) < k or x.stride(0) % 8)):
        raise ValueError("clip_search: the rows of x must be contiguous with a stride that is a multiple of 8 elements")
    g = k // 128
    best = torch.empty((n, g), dtype=w.dtype, device=w.device)
    idx = torch.empty((n, g), dtype=torch.int32, device=w.device)
    err = torch.empty((n, g, int(n_steps)), dtype=torch.float32, device=w.device) if return_err else None
    with torch.cuda.device(w.device):
        _capi.check(_capi.lib().awq_clip_search(w.data_ptr(), w.stride(0) if n > 1 else k, x.data_ptr(), x.stride(0) if s > 1 else k,
                                                best.data_ptr(), idx.data_ptr(), None if err is None else err.data_ptr(), n, k, s, 128,
                                                int(n_bit), int(n_grid), int(n_steps), _dt(w), _stream(w)))
    return (best, idx, err) if return_err else (best, idx)


def pair_lost_count(device=None) -> int:
    """C-ABI awq_w4a16_gemm_cdna4_pair_lost: blocks of the block-pair K split (down_proj-shaped prefill launches) of `device` that gave up waiting
    for their partner since the library was loaded -- their outputs are NaN.  0 on a healthy run; synchronises with the device.  A serving loop
    that shares the GPU (CU masks, other tenants) polls this between batches and sets the knob `gemm_v6_pair` = 0 when it ever moves."""
    import ctypes
    if not torch.cuda.is_available():
        raise RuntimeError("pair_lost_count needs the GPU the library runs on")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    c = ctypes.c_uint(0)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().awq_w4a16_gemm_cdna4_pair_lost(ctypes.byref(c)))
    return int(c.value)


def attn_decode_plan(batch: int, nheads_kv: int, head_dim: int, timestep: int, lmax: int):
    """Host-side awq_attn_decode_plan: (splits, chunk) of the decode attention launch (no GPU needed)."""
    import ctypes

    s, c = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_decode_plan(batch, nheads_kv, head_dim, timestep, lmax, ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def single_query_attention(q, k, v, k_cache, v_cache, length_per_sample=None, alibi_slopes=None, timestep: int = 0,
                           rotary_embedding_dim: int = 0, rotary_base: float = 10000.0, rotary_scale: float = 1.0,
                           neox_rotary_style: bool = True):
    """C-ABI awq_attn_decode: one decode step over the FasterTransformer KV cache (ft_attention.cpp:112-185).
    q [B, H, Dh], k / v [B, Hkv, Dh] (batch strides of their own, heads contiguous), k_cache [Bc, Hkv, Dh/8, Lmax, 8],
    v_cache [Bc, Hkv, Lmax, Dh] with B <= Bc.  Writes the current k / v into the caches; returns [B, H, Dh]."""
    for t in (q, k, v, k_cache, v_cache, length_per_sample, alibi_slopes):
        if t is not None and not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    for t in (q, k, v):
        if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError("q / k / v must be [B, heads, Dh] with contiguous heads")
    _need_gpu(k_cache, v_cache, length_per_sample, alibi_slopes)
    B, H, Dh = q.shape
    Bc, Hkv, Lmax = v_cache.shape[0], v_cache.shape[1], v_cache.shape[2]
    out = torch.empty(B, H, Dh, dtype=q.dtype, device=q.device)
    L = _capi.lib()
    wsb = L.awq_attn_decode_workspace_bytes(B, H, Hkv, Dh, timestep, Lmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device) if wsb else None
    with torch.cuda.device(q.device):
        _capi.check(L.awq_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                      length_per_sample.data_ptr() if length_per_sample is not None else None,
                                      alibi_slopes.data_ptr() if alibi_slopes is not None else None, out.data_ptr(),
                                      B, Bc, H, Hkv, Dh, Lmax, q.stride(0), k.stride(0), v.stride(0), int(timestep),
                                      int(rotary_embedding_dim), float(rotary_base), float(rotary_scale), int(bool(neox_rotary_style)),
                                      _dt(q), ws.data_ptr() if wsb else None, wsb, _stream(q)))
    return out


def attn_prefill_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, seqlen_q: int, seqlen_k: int, causal: bool = True):
    """Host-side awq_attn_prefill_plan: (q_tile_rows, blocks) of the prefill attention launch (no GPU needed)."""
    import ctypes

    r, n = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_prefill_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, int(bool(causal)),
                                                  ctypes.byref(r), ctypes.byref(n)))
    return r.value, n.value


def _check_qkv(who, q, k, v):
    for t in (q, k, v):
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
        if t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
            raise ValueError("q / k / v must be [B, S, heads, Dh] with contiguous heads")
    if k.device != q.device or v.device != q.device:
        raise ValueError(f"{who}: q, k and v must live on the same GPU")
    if k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3] or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"{who}: q [B, Sq, H, Dh] and k / v [B, Sk, Hkv, Dh] of one dtype are expected")


def attn_splitkv_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, seqlen_q: int, seqlen_k: int, causal: bool = True):
    """Host-side awq_attn_splitkv_plan: (splits, chunk) of the split-KV attention launch (no GPU needed).  splits == 1: the one-pass
    prefill kernel serves."""
    import ctypes

    s, c = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_splitkv_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, seqlen_k, int(bool(causal)),
                                                  ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def attn_splitkv(q, k, v, softmax_scale=None, causal: bool = False):
    """C-ABI awq_attn_splitkv: flash_attn_func's contract (see below) for few query rows over a long history.  Where attn_splitkv_plan
    splits, the G query heads of a KV group share one fetch of K / V, the keys are cut over blocks and fp32 partials are combined by a
    second launch; otherwise this is the one-pass launch, bit for bit."""
    _check_qkv("attn_splitkv", q, k, v)
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    out = torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    L = _capi.lib()
    wsb = L.awq_attn_splitkv_workspace_bytes(B, H, Hkv, Dh, Sq, Sk, int(bool(causal)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device) if wsb else None
    with torch.cuda.device(q.device):
        _capi.check(L.awq_attn_splitkv(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Sq, Sk, H, Hkv, Dh,
                                       q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                       scale, int(bool(causal)), _dt(q), ws.data_ptr() if wsb else None, wsb, _stream(q)))
    return out


def flash_attn_func(q, k, v, softmax_scale=None, causal: bool = False):
    """C-ABI awq_attn_prefill: softmax(scale * q k^T + mask) v with flash_attn_func's layout and masking.
    q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] (batch and row strides of their own, heads contiguous -- the q / k / v slices of one
    fused qkv tensor pass without a copy); causal is bottom-right aligned (row i attends keys j <= i + Sk - Sq).  Returns
    [B, Sq, H, Dh] contiguous.  Dh 64 or 128 (72 too when not causal), float16 / bfloat16.  A call for which attn_splitkv_plan splits
    (few query rows, Sk >= 2048) goes to attn_splitkv."""
    _check_qkv("flash_attn_func", q, k, v)
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    # (the plan never splits below 2048 keys unless the knob attn_splitkv_chunk forces a chunk; shapes it refuses go on to awq_attn_prefill)
    if min(B, Sq, Sk, Hkv) >= 1 and Dh in (64, 128) and H % Hkv == 0 and not (causal and Sq > Sk) and \
            attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, causal)[0] > 1:
        return attn_splitkv(q, k, v, softmax_scale, causal)
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    out = torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    with torch.cuda.device(q.device):
        _capi.check(_capi.lib().awq_attn_prefill(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Sq, Sk, H, Hkv, Dh,
                                                 q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                                 scale, int(bool(causal)), _dt(q), _stream(q)))
    return out


# ---- FP8 KV cache on the natural layout (csrc/awq_kv8.hpp) --------------------------------------------------------------------------
KV8_MAX = 448.0          # the largest finite e4m3fn value
KV8_AMAX_FLOOR = 2.0 ** -60  # a row's max |x| is raised to this: no special case for a zero row, no fp32 denormal scale


def kv8_quant(x):
    """The FP8 KV-cache format, in plain torch on any device: x [..., Dh] of float16 / bfloat16 -> (codes [..., Dh] float8_e4m3fn,
    scale [...] float32), one scale per head row.  s = max(max|x|, 2^-60) / 448 as an fp32 division, code = e4m3fn_RNE(clamp(x / s,
    -448, 448)) with x / s a correctly rounded fp32 division.  Rows with NaN / Inf are outside the contract."""
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"kv8_quant: expected float16/bfloat16, got {x.dtype}")
    xf = x.to(torch.float32)
    amax = xf.abs().amax(dim=-1).clamp_min(KV8_AMAX_FLOOR)
    scale = amax / torch.tensor(KV8_MAX, dtype=torch.float32, device=x.device)
    codes = (xf / scale.unsqueeze(-1)).clamp(-KV8_MAX, KV8_MAX).to(torch.float8_e4m3fn)
    return codes, scale


def kv8_dequant(codes, scale, dtype):
    """codes [..., Dh] (float8_e4m3fn, or uint8 holding the same bytes), scale [...] float32 -> T(float(code) * s): one fp32 multiply, one
    rounding to `dtype`.  This is what the FP8 attention kernels put into LDS, so attn_kv8 equals flash_attn_func on this tensor bit for bit."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"kv8_dequant: expected float16/bfloat16, got {dtype}")
    if codes.dtype == torch.uint8:
        codes = codes.view(torch.float8_e4m3fn)
    if codes.dtype != torch.float8_e4m3fn or scale.dtype != torch.float32 or tuple(scale.shape) != tuple(codes.shape[:-1]):
        raise ValueError("kv8_dequant: codes [..., Dh] of float8_e4m3fn / uint8 and scale [...] of float32 are expected")
    return (codes.to(torch.float32) * scale.unsqueeze(-1)).to(dtype)


def _kv8_codes(who, name, t):
    if t.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise ValueError(f"{who}: {name} must be float8_e4m3fn or uint8, got {t.dtype}")


def _on_gpu(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")


class _Kv:
    """Where K / V of one natural-layout call live, once whoever builds it has checked the tensors: dense caches [Bc, Lmax, Hkv, Dh] or,
    with block_table [>= B, pages_per_seq], pools [num_pages, page_size, Hkv, Dh]; with k_scale / v_scale [.., Hkv] the FP8 format.  The
    pieces of a C-ABI argument list come out in the order every entry of the family takes them."""

    def __init__(self, k, v, k_scale=None, v_scale=None, block_table=None):
        self.k, self.v, self.k_scale, self.v_scale, self.block_table = k, v, k_scale, v_scale, block_table
        self.outer, self.rows, self.Hkv, self.Dh = v.shape  # (cache_batch or num_pages, lmax or page_size, ..)
        self.fp8, self.paged = k_scale is not None, block_table is not None

    def ptrs(self):
        return (self.k.data_ptr(), self.v.data_ptr()) + ((self.k_scale.data_ptr(), self.v_scale.data_ptr()) if self.fp8 else ())

    def strides(self):
        s = (self.k.stride(0), self.k.stride(1), self.v.stride(0), self.v.stride(1))
        return s + ((self.k_scale.stride(0), self.k_scale.stride(1), self.v_scale.stride(0), self.v_scale.stride(1)) if self.fp8 else ())

    def table(self):  # num_pages, page_size, pages_per_seq, table_row_stride
        return (self.outer, self.rows, self.block_table.shape[1], self.block_table.stride(0))


def _fp8_pair(who, k_scale, v_scale):
    """Whether the call brings the scales of the FP8 format; one without the other is refused."""
    fp8 = k_scale is not None or v_scale is not None
    if fp8 and (k_scale is None or v_scale is None):
        raise ValueError(f"{who}: k_scale and v_scale come together")
    return fp8


def _caches(who, qkv, k_cache, v_cache, k_scale, v_scale):
    """The contiguous caches [Bc, Lmax, Hkv, Dh] of a store call (and their scales [Bc, Lmax, Hkv]), checked against qkv, as a _Kv."""
    fp8 = _fp8_pair(who, k_scale, v_scale)
    _on_gpu(k_cache, v_cache, *((k_scale, v_scale) if fp8 else ()))
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if fp8:
            _kv8_codes(who, name, t)
        elif t.dtype != qkv.dtype:
            raise ValueError(f"{who}: the caches must have the dtype of the input")
        if t.device != qkv.device or t.dim() != 4 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous [Bc, Lmax, Hkv, Dh] tensor on the GPU of qkv")
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"{who}: k_cache and v_cache must have one shape [Bc, Lmax, Hkv, Dh]")
    if fp8:
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t.device != qkv.device or t.dtype != torch.float32 or tuple(t.shape) != tuple(v_cache.shape[:3]) or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous float32 [Bc, Lmax, Hkv] tensor on the GPU of qkv")
    return _Kv(k_cache, v_cache, k_scale, v_scale)


def _norm_pair(who, q_norm, k_norm):
    """Whether the call brings the per-head q/k norm; one gamma without the other is refused (before anything else is looked at)."""
    if (q_norm is None) != (k_norm is None):
        raise ValueError(f"{who}: q_norm and k_norm come together")
    return q_norm is not None


def _qk_norm(who, qkv, Dh, q_norm, k_norm, norm_eps):
    """The per-head q/k RMSNorm of a store call: None without one, else (q_gamma, k_gamma, eps) with the gammas as float32 [Dh] on the GPU
    of qkv.  A gamma of T becomes float32 exactly; a float32 one (Gemma-3's 1 + w) is taken as it is."""
    if not _norm_pair(who, q_norm, k_norm):
        return None
    _on_gpu(q_norm, k_norm)
    gammas = []
    for name, g in (("q_norm", q_norm), ("k_norm", k_norm)):
        if g.device != qkv.device or g.dtype not in (torch.float32, qkv.dtype) or tuple(g.shape) != (Dh,):
            raise ValueError(f"{who}: {name} must be a [Dh] = [{Dh}] tensor of float32 or of the input's dtype on the GPU of qkv")
        g = g.float().contiguous()
        gammas.append(g if g.data_ptr() % 16 == 0 else g.clone())
    eps = float(norm_eps)
    if not (eps >= 0.0 and eps != float("inf")):
        raise ValueError(f"{who}: norm_eps must be finite and >= 0, got {norm_eps!r}")
    return gammas[0], gammas[1], eps


def _rope_store(who, qkv, freqs, kv, nheads, nheads_kv, start_pos=None, cache_seqlens=None, packed=None, norm=None):
    """The ten store entries of the C ABI over a described cache; with norm = (q_gamma, k_gamma, eps) of _qk_norm, their _qknorm
    siblings.  cache_seqlens None: the host position start_pos and the call's angles;
    otherwise the positions are read on the device and freqs is the model's whole angle table [P, rot_dim].  packed = (cu_seqlens_q,
    max_seqlen_q, q_out or None), checked by the caller: qkv is the packed tokens [total_q, ..] of a step (device positions only)."""
    devlen = cache_seqlens is not None
    if freqs.device != qkv.device or freqs.dtype != torch.float32 or (devlen and freqs.dim() != 2) or not freqs.is_contiguous():
        raise ValueError(f"{who}: freqs_table must be a contiguous float32 [P, rot_dim] tensor on the GPU of qkv" if devlen else
                         f"{who}: contiguous float32 freqs on the GPU of qkv are expected")
    if (packed is None and (qkv.dim() != 3 or qkv.stride(2) != 1)) or nheads_kv != kv.Hkv or qkv.shape[-1] != (nheads + 2 * nheads_kv) * kv.Dh:
        raise ValueError(f"{who}: qkv must be " + ("[total_q, (H + 2 Hkv) * Dh] with the " + ("pools'" if kv.paged else "caches'") + " Hkv and Dh"
                                                   if packed else "[B, S, (H + 2 Hkv) * Dh] with " +
                                                   ("the pools' Hkv and Dh" if kv.paged else "a unit last stride and the caches' Hkv and Dh")))
    if packed:
        cu, S, q_out = packed
        B, tokens = cu.shape[0] - 1, (cu.data_ptr(), int(S), qkv.shape[0])
    else:
        B, S = qkv.shape[0], qkv.shape[1]
        tokens = (S,)
    rot = freqs.shape[-1]
    if devlen:
        _check_seqlens(who, "cache_seqlens", cache_seqlens, qkv, B)
    elif freqs.numel() < B * S * rot:
        raise ValueError(f"{who}: freqs holds fewer than B * S * rot_dim angles")
    q_out = _packed_out(who, "q_out", q_out, qkv, int(nheads), kv.Dh) if packed else \
        torch.empty(B, S, nheads, kv.Dh, dtype=qkv.dtype, device=qkv.device)
    gammas = () if norm is None else (norm[0].data_ptr(), norm[1].data_ptr(), norm[2])  # directly after the angles
    head = (qkv.data_ptr(), freqs.data_ptr(), *gammas, q_out.data_ptr(), *kv.ptrs())
    shape = (*tokens, int(nheads), int(nheads_kv), kv.Dh, rot)
    tail = (*qkv.stride()[:-1], _dt(qkv), _stream(qkv))  # the batch stride (a rectangle's only) and the row stride
    form = "_varq" if packed else "_pos"
    if kv.paged:
        entry, args = "paged" + form, (*head, kv.block_table.data_ptr(), cache_seqlens.data_ptr(), B, *shape, freqs.shape[0], *kv.table(),
                                       *kv.strides(), *tail)
    elif devlen:
        entry, args = "natural" + form, (*head, cache_seqlens.data_ptr(), B, kv.outer, *shape, kv.rows, freqs.shape[0], *tail)
    else:
        entry, args = "natural", (*head, B, kv.outer, *shape, kv.rows, int(start_pos), *tail)
    with torch.cuda.device(qkv.device):
        _capi.check(getattr(_capi.lib(), "awq_rope_kv_store_" + entry + ("_fp8" if kv.fp8 else "") + ("" if norm is None else "_qknorm"))(*args))
    return q_out


def _attn_kvcache(who, q, kv, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, one_pass=False, packed=None, split=None,
                  window=None, softcap=None):
    """The device-length attention entries of the C ABI over a described cache (q and kv checked by the caller): the four of the split
    pair, or with one_pass the four of the one-pass prefill kernel (any Sq, no workspace).  packed = (cu_seqlens_q, max_seqlen_q, out or
    None), checked by the caller (one_pass only): q is the packed rows [total_q, H, Dh] of a step, the four varq entries serve and
    seqlen_offset carries the flag lens_before_step.  split = (split_seqlen_q, split_min_keys), with packed: a mixed step, the four
    awq_attn_[paged_]varq entries and the split pair's workspace.  window = window_left, with split: the four *_window entries and their plan.
    softcap (a float, with window): the four *_softcap entries, which take the window's plan and workspace."""
    if packed:
        cu, Sq, out = packed
        (T, H, Dh), B = q.shape, cu.shape[0] - 1
        rows = (cu.data_ptr(), int(Sq), T)
    else:
        B, Sq, H, Dh = q.shape
        rows = (Sq,)
    _check_seqlens(who, "seqlens_k", seqlens_k, q, B)
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    L = _capi.lib()
    out = _packed_out(who, "out", out, q, H, Dh) if packed else torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    lens = (B, *rows, seqlens_k.data_ptr(), int(seqlen_offset), int(max_seqlen_k))
    where = (kv.block_table.data_ptr(), *lens, *kv.table()) if kv.paged else (*lens, kv.rows)
    # q's strides: the batch stride (a rectangle's only) and the row stride
    head = (q.data_ptr(), *kv.ptrs(), out.data_ptr(), *where, H, kv.Hkv, Dh, *q.stride()[:-2], *kv.strides(), scale, int(bool(causal)), _dt(q))
    if split is not None:
        if window is None:
            wsb = L.awq_attn_varq_split_workspace_bytes(B, H, kv.Hkv, Dh, split[0], int(max_seqlen_k))
        else:
            wsb = L.awq_attn_varq_window_workspace_bytes(B, H, kv.Hkv, Dh, split[0], int(max_seqlen_k), window)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=q.device)
        form = "" if window is None else ("_window" if softcap is None else "_softcap")
        entry = getattr(L, "awq_attn_" + ("paged_" if kv.paged else "") + "varq" + form + ("_kv8" if kv.fp8 else ""))
        tail = () if window is None else ((window,) if softcap is None else (window, softcap))
        with torch.cuda.device(q.device):
            _capi.check(entry(*head, split[0], split[1], *tail, ws.data_ptr(), wsb, _stream(q)))
        return out
    if one_pass:
        entry = getattr(L, "awq_attn_prefill_" + ("paged" if kv.paged else "kvcache") + ("_varq" if packed else "") + ("_kv8" if kv.fp8 else ""))
        with torch.cuda.device(q.device):
            _capi.check(entry(*head, _stream(q)))
        return out
    wsb = L.awq_attn_kvcache_workspace_bytes(B, H, kv.Hkv, Dh, Sq, int(max_seqlen_k))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=q.device)
    entry = getattr(L, "awq_attn_kvcache" + ("_paged" if kv.paged else "") + ("_kv8" if kv.fp8 else ""))
    with torch.cuda.device(q.device):
        _capi.check(entry(*head, ws.data_ptr(), wsb, _stream(q)))
    return out


def rope_kv_store_natural_fp8(qkv, freqs, k_cache, v_cache, k_scale, v_scale, start_pos: int, nheads: int, nheads_kv: int):
    """C-ABI awq_rope_kv_store_natural_fp8: rope_kv_store_natural with k and v quantised on their way into the FP8 caches (kv8_quant's
    format).  k_cache / v_cache [Bc, Lmax, Hkv, Dh] float8_e4m3fn or uint8, k_scale / v_scale [Bc, Lmax, Hkv] float32.  Writes codes and
    scales at [b, start_pos + s]; returns the rotated q [B, S, H, Dh], rope_kv_store_natural's bits."""
    return rope_kv_store_natural_fp8_qknorm(qkv, freqs, k_cache, v_cache, k_scale, v_scale, start_pos, nheads, nheads_kv)


def rope_kv_store_natural_fp8_qknorm(qkv, freqs, k_cache, v_cache, k_scale, v_scale, start_pos: int, nheads: int, nheads_kv: int, *, q_norm=None,
                                     k_norm=None, norm_eps: float = 1e-6):
    """`rope_kv_store_natural_fp8` with the per-head q/k RMSNorm of `rope_kv_store_natural` (C-ABI awq_rope_kv_store_natural_fp8_qknorm): the
    same arguments and, keyword-only, q_norm / k_norm ([Dh], float32 or the input's dtype; both or neither) and norm_eps.  The quantiser
    sees the normalised, rotated k; v is untouched.  A function of its own: `rope_kv_store_natural_fp8` keeps its parameter list."""
    who = "rope_kv_store_natural_fp8"
    _norm_pair(who, q_norm, k_norm)
    _on_gpu(qkv, freqs, k_cache, v_cache, k_scale, v_scale)
    kv = _caches(who, qkv, k_cache, v_cache, k_scale, v_scale)
    return _rope_store(who, qkv, freqs, kv, nheads, nheads_kv, start_pos=start_pos, norm=_qk_norm(who, qkv, kv.Dh, q_norm, k_norm, norm_eps))


def _check_kv8(who, q, k, v, k_scale, v_scale):
    for t in (q, k, v, k_scale, v_scale):
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
        if t.device != q.device:
            raise ValueError(f"{who}: q, k, v and the scales must live on the same GPU")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
            raise ValueError(f"{who}: {name} must be [B, S, heads, Dh] with contiguous heads")
    _kv8_codes(who, "k", k)
    _kv8_codes(who, "v", v)
    if k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError(f"{who}: q [B, Sq, H, Dh] and k / v [B, Sk, Hkv, Dh] are expected")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t.dtype != torch.float32 or tuple(t.shape) != tuple(k.shape[:3]) or t.stride(2) != 1:
            raise ValueError(f"{who}: {name} must be float32 [B, Sk, Hkv] with a unit last stride")


def _attn_kv8(entry, q, k, v, k_scale, v_scale, softmax_scale, causal, checked=False):
    if not checked:  # (attn_kv8 has checked the tensors already)
        _check_kv8("attn_" + entry + "_kv8", q, k, v, k_scale, v_scale)
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    out = torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    L = _capi.lib()
    head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(), out.data_ptr(), B, Sq, Sk, H, Hkv, Dh,
            q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), k_scale.stride(0), k_scale.stride(1),
            v_scale.stride(0), v_scale.stride(1), scale, int(bool(causal)), _dt(q))
    with torch.cuda.device(q.device):
        if entry == "prefill":
            _capi.check(L.awq_attn_prefill_kv8(*head, _stream(q)))
        else:
            wsb = L.awq_attn_splitkv_workspace_bytes(B, H, Hkv, Dh, Sq, Sk, int(bool(causal)))
            ws = torch.empty(wsb, dtype=torch.uint8, device=q.device) if wsb else None
            _capi.check(L.awq_attn_splitkv_kv8(*head, ws.data_ptr() if wsb else None, wsb, _stream(q)))
    return out


def attn_prefill_kv8(q, k, v, k_scale, v_scale, softmax_scale=None, causal: bool = False):
    """C-ABI awq_attn_prefill_kv8: flash_attn_func's one-pass kernel with K / V read from the FP8 cache.  q [B, Sq, H, Dh] float16 /
    bfloat16, k / v [B, Sk, Hkv, Dh] float8_e4m3fn or uint8 (batch and row strides of their own, multiples of 16), k_scale / v_scale
    [B, Sk, Hkv] float32.  Bit-identical to the one-pass kernel on kv8_dequant(k, k_scale, q.dtype), kv8_dequant(v, v_scale, q.dtype)."""
    return _attn_kv8("prefill", q, k, v, k_scale, v_scale, softmax_scale, causal)


def attn_splitkv_kv8(q, k, v, k_scale, v_scale, softmax_scale=None, causal: bool = False):
    """C-ABI awq_attn_splitkv_kv8: attn_splitkv with K / V read from the FP8 cache (attn_prefill_kv8's arguments); the one-pass launch
    where attn_splitkv_plan does not split.  Bit-identical to attn_splitkv on the dequantised tensors."""
    return _attn_kv8("splitkv", q, k, v, k_scale, v_scale, softmax_scale, causal)


def attn_kv8(q, k, v, k_scale, v_scale, softmax_scale=None, causal: bool = False):
    """flash_attn_func on the FP8 cache: routed by attn_splitkv_plan exactly as flash_attn_func routes (the split-KV kernels where the plan
    splits, the one-pass kernel otherwise).  Dh 64 or 128."""
    _check_kv8("attn_kv8", q, k, v, k_scale, v_scale)
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    if min(B, Sq, Sk, Hkv) >= 1 and Dh in (64, 128) and H % Hkv == 0 and not (causal and Sq > Sk) and \
            attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, causal)[0] > 1:
        return _attn_kv8("splitkv", q, k, v, k_scale, v_scale, softmax_scale, causal, checked=True)
    return _attn_kv8("prefill", q, k, v, k_scale, v_scale, softmax_scale, causal, checked=True)


# ---- lengths on the device: ragged batched decode and whole-phase graph capture on the natural-layout caches ------------------------
def attn_kvcache_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, seqlen_q: int, max_seqlen_k: int):
    """Host-side awq_attn_kvcache_plan: (splits, chunk) of attn_kvcache, made from the bound max_seqlen_k alone (no GPU needed).  splits >= 1
    and splits * chunk >= max_seqlen_k; the split kernel pair runs for any splits.  Sized for one sequence at the bound: `batch` does
    not change it."""
    import ctypes

    s, c = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_kvcache_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, max_seqlen_k, ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def _check_seqlens(who, name, t, ref, batch):
    if not t.is_cuda:
        raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    if t.device != ref.device or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != batch or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous int32 [B] tensor on the GPU of the input")


def attn_kvcache(q, k_cache, v_cache, seqlens_k, max_seqlen_k: int, seqlen_offset: int = 0, softmax_scale=None, causal: bool = True,
                 k_scale=None, v_scale=None):
    """C-ABI awq_attn_kvcache[_kv8]: split-KV attention of q [B, Sq, H, Dh] over the natural-layout caches k_cache / v_cache
    [Bc >= B, Lmax, Hkv, Dh] with each sequence's length read on the device: Sk_b = seqlens_k[b] + seqlen_offset, seqlens_k int32 [B].
    max_seqlen_k <= Lmax is the host bound that sizes the launch; a sequence with Sk_b < 1 or Sk_b > max_seqlen_k is inactive and returns
    zeros.  Causal rows attend keys j <= i + Sk_b - Sq.  Sq * (H / Hkv) <= 128, Dh 64 or 128.  With k_scale / v_scale [Bc, Lmax, Hkv]
    float32 the caches are FP8 codes (kv8_quant's format).  The host never reads seqlens_k: the call is capturable and a replay follows the
    lengths the tensor holds then."""
    return _attn_dense("attn_kvcache", False, q, k_cache, v_cache, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, k_scale, v_scale)


def _check_caches(who, q, k, v, k_scale, v_scale, packed_batch=None):
    """The dense caches [Bc >= B, Lmax, Hkv, Dh] of an attention call (T, or FP8 codes with their scales), checked against q [B, Sq, H, Dh]
    -- or, with packed_batch = the B of a packed step, against the rows [total_q, H, Dh] the caller has checked -- as a _Kv."""
    packed = packed_batch is not None
    fp8 = _fp8_pair(who, k_scale, v_scale)
    if fp8:  # (the checks of the host-length FP8 entries, on the batch rows this call reads; packed rows stand as one batch row)
        nb = 1 if packed else q.shape[0]
        _check_kv8(who, q.unsqueeze(0) if packed else q, k[:nb], v[:nb], k_scale[:nb], v_scale[:nb])
    else:
        for t in ((k, v) if packed else (q, k, v)):
            _on_gpu(t)
            if t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
                raise ValueError(f"{who}: k / v must be [Bc, Lmax, Hkv, Dh] with contiguous heads" if packed else
                                 f"{who}: q / k_cache / v_cache must be [B, S, heads, Dh] with contiguous heads")
        if k.device != q.device or v.device != q.device or k.dtype != q.dtype or v.dtype != q.dtype:
            raise ValueError(f"{who}: q and the caches must share one GPU and one dtype")
    if packed:
        if k.shape != v.shape or k.shape[0] < packed_batch:
            raise ValueError(f"{who}: q [total_q, H, Dh] and k / v [Bc >= B, Lmax, Hkv, Dh] are expected")
    elif not fp8 and (k.shape != v.shape or k.shape[0] < q.shape[0] or k.shape[3] != q.shape[3]):
        raise ValueError(f"{who}: q [B, Sq, H, Dh] and k_cache / v_cache [Bc >= B, Lmax, Hkv, Dh] are expected")
    return _Kv(k, v, k_scale, v_scale)


def _attn_dense(who, one_pass, q, k_cache, v_cache, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, k_scale, v_scale):
    """attn_kvcache / attn_prefill_kvcache: the tensor checks of the dense caches, then the entry."""
    kv = _check_caches(who, q, k_cache, v_cache, k_scale, v_scale)
    return _attn_kvcache(who, q, kv, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, one_pass)


def attn_prefill_kvcache(q, k_cache, v_cache, seqlens_k, max_seqlen_k: int, seqlen_offset: int = 0, softmax_scale=None, causal: bool = True,
                         k_scale=None, v_scale=None):
    """C-ABI awq_attn_prefill_kvcache[_kv8]: `attn_kvcache`'s arguments and lengths served by the ONE-PASS prefill kernel, for a prompt
    chunk of any length: q [B, Sq, H, Dh] with Sq >= 1 of any size, Dh 64 or 128, no workspace.  Sk_b = seqlens_k[b] + seqlen_offset; a
    sequence with Sk_b < 1 or Sk_b > max_seqlen_k returns zeros and none of its cache rows is read; a row whose causal limit
    i + Sk_b - Sq is negative returns zeros.  For every active sequence with Sk_b >= Sq the result is bit-identical to `flash_attn_func`
    (`attn_prefill_kv8`) on (q[b:b+1], cache[b:b+1, :Sk_b]) under the same q tile.  Capturable: a replay follows the lengths the tensor
    holds then."""
    return _attn_dense("attn_prefill_kvcache", True, q, k_cache, v_cache, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, k_scale,
                       v_scale)


def rope_kv_store_natural_pos(qkv, freqs_table, k_cache, v_cache, cache_seqlens, nheads: int, nheads_kv: int, k_scale=None, v_scale=None, *,
                              q_norm=None, k_norm=None, norm_eps: float = 1e-6):
    """C-ABI awq_rope_kv_store_natural_pos[_fp8]: rope_kv_store_natural[_fp8] with each sequence's position read on the device.
    cache_seqlens int32 [B] holds the tokens already in each sequence's cache; token s of sequence b is rotated by row
    cache_seqlens[b] + s of freqs_table [P, rot_dim] (float32, the model's whole angle table) and stored at that cache position.  A
    sequence with cache_seqlens[b] < 0 or cache_seqlens[b] + S > min(Lmax, P) is inactive: nothing of it is stored and its q rows are
    zeros.  With k_scale / v_scale the caches are FP8 (rope_kv_store_natural_fp8's arguments).  Returns the rotated q [B, S, H, Dh].

    q_norm / k_norm (keyword-only, both or neither; [Dh], float32 or the input's dtype) and norm_eps: every q head and every k head is
    RMS-normalised over Dh before the rotation, in the same launch (C-ABI `_qknorm` sibling; Qwen3, Gemma-3) -- y = T((x * rsqrt(mean(x^2)
    + norm_eps)) * gamma), `rmsnorm`'s arithmetic on the head as a row.  v is untouched."""
    who = "rope_kv_store_natural_pos"
    _norm_pair(who, q_norm, k_norm)
    _on_gpu(qkv, freqs_table, cache_seqlens)
    kv = _caches(who, qkv, k_cache, v_cache, k_scale, v_scale)
    return _rope_store(who, qkv, freqs_table, kv, nheads, nheads_kv, cache_seqlens=cache_seqlens,
                       norm=_qk_norm(who, qkv, kv.Dh, q_norm, k_norm, norm_eps))


# ---- the paged KV cache: the two calls above over a pool of pages and a per-sequence block table ------------------------------------
def _check_pools(who, ref, k_pool, v_pool, block_table, k_scale, v_scale, batch):
    """The pools [num_pages, page_size, Hkv, Dh] and the table [>= B, pages_per_seq] of one call, checked against `ref`, as a _Kv."""
    fp8 = _fp8_pair(who, k_scale, v_scale)
    _on_gpu(ref, k_pool, v_pool, block_table, *((k_scale, v_scale) if fp8 else ()))
    for name, t in (("k_pool", k_pool), ("v_pool", v_pool)):
        if fp8:
            _kv8_codes(who, name, t)
        elif t.dtype != ref.dtype:
            raise ValueError(f"{who}: the pools must have the dtype of the input")
        if t.device != ref.device or t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
            raise ValueError(f"{who}: {name} must be a [num_pages, page_size, Hkv, Dh] tensor with contiguous heads on the GPU of the input")
    if k_pool.shape != v_pool.shape:
        raise ValueError(f"{who}: k_pool and v_pool must have one shape [num_pages, page_size, Hkv, Dh]")
    num_pages, page_size, Hkv, Dh = v_pool.shape
    if num_pages < 1 or page_size < 64 or page_size % 64:
        raise ValueError(f"{who}: pools [num_pages >= 1, page_size, Hkv, Dh] with page_size a multiple of 64 are expected, got "
                         f"{tuple(v_pool.shape)}")
    if fp8:
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t.device != ref.device or t.dtype != torch.float32 or tuple(t.shape) != (num_pages, page_size, Hkv) or t.stride(2) != 1:
                raise ValueError(f"{who}: {name} must be a float32 [num_pages, page_size, Hkv] tensor with a unit last stride on the GPU of "
                                 "the input")
    if block_table.device != ref.device or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] < batch or \
            block_table.shape[1] < 1 or block_table.stride(1) != 1 or block_table.stride(0) < block_table.shape[1]:
        raise ValueError(f"{who}: block_table must be an int32 [>= B, pages_per_seq] tensor with a unit last stride on the GPU of the input")
    return _Kv(k_pool, v_pool, k_scale, v_scale, block_table)


def attn_kvcache_paged(q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k: int, seqlen_offset: int = 0, softmax_scale=None,
                       causal: bool = True, k_scale=None, v_scale=None):
    """C-ABI awq_attn_kvcache_paged[_kv8]: `attn_kvcache` over a paged KV cache.  k_pool / v_pool [num_pages, page_size, Hkv, Dh] (page_size a
    multiple of 64), block_table int32 [>= B, pages_per_seq] on the GPU: key p of sequence b is row p % page_size of page
    block_table[b, p // page_size].  max_seqlen_k <= pages_per_seq * page_size.  For every active sequence the result is bit-identical to
    `attn_kvcache` on the dense gather of its pages.  Entries behind a sequence's live range are never read; a page id is clamped into the
    pool.  With k_scale / v_scale [num_pages, page_size, Hkv] float32 the pools are FP8 codes.  The host reads neither the table nor the
    lengths: capturable, and a replay follows what the tensors hold then."""
    return _attn_paged("attn_kvcache_paged", False, q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal,
                       k_scale, v_scale)


def _attn_paged(who, one_pass, q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, k_scale, v_scale):
    """attn_kvcache_paged / attn_prefill_paged: the tensor checks of the pools and the table, then the entry."""
    _on_gpu(q)
    if q.dim() != 4 or q.stride(3) != 1 or q.stride(2) != q.shape[3]:
        raise ValueError(f"{who}: q must be [B, Sq, H, Dh] with contiguous heads")
    kv = _check_pools(who, q, k_pool, v_pool, block_table, k_scale, v_scale, q.shape[0])
    if kv.Dh != q.shape[3]:
        raise ValueError(f"{who}: q [B, Sq, H, Dh] and k_pool / v_pool [num_pages, page_size, Hkv, Dh] must share Dh, got {q.shape[3]} and {kv.Dh}")
    return _attn_kvcache(who, q, kv, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal, one_pass)


# ---- shared-prefix decode: the sequences of a group read their common prefix once (csrc/awq_shared.hpp) -------------------------------
def attn_kvcache_shared_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, seqlen_q: int, max_prefix: int, max_seqlen_k: int):
    """Host-side awq_attn_kvcache_shared_plan: (splits_p, chunk_p, splits_s, chunk_s) of attn_kvcache_paged_shared (no GPU needed) --
    `attn_kvcache_plan`'s rule for the bound max_prefix of the prefix walk and again for max_seqlen_k of the suffix walk.  The knob
    attn_splitkv_chunk forces both chunks."""
    import ctypes

    v = [ctypes.c_int(0) for _ in range(4)]
    _capi.check(_capi.lib().awq_attn_kvcache_shared_plan(batch, nheads, nheads_kv, head_dim, seqlen_q, max_prefix, max_seqlen_k,
                                                         *(ctypes.byref(x) for x in v)))
    return tuple(x.value for x in v)


def _check_groups(who, ref, batch, group_members, group_prefix, seq_prefix):
    for t in (group_members, group_prefix, seq_prefix):
        _on_gpu(t)
        if t.device != ref.device or t.dtype != torch.int32:
            raise ValueError(f"{who}: the group arrays must be int32 tensors on the GPU of the input")
    if group_members.dim() != 2 or group_members.shape[0] < 1 or group_members.shape[1] < 1 or group_members.stride(1) != 1 or \
            group_members.stride(0) < group_members.shape[1]:
        raise ValueError(f"{who}: group_members must be [num_groups, group_cap] with a unit last stride")
    if group_prefix.dim() != 1 or group_prefix.shape[0] != group_members.shape[0] or not group_prefix.is_contiguous():
        raise ValueError(f"{who}: group_prefix must be a contiguous [num_groups] tensor")
    if seq_prefix.dim() != 1 or seq_prefix.shape[0] != batch or not seq_prefix.is_contiguous():
        raise ValueError(f"{who}: seq_prefix must be a contiguous [B] tensor")


def attn_kvcache_paged_shared(q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k: int, group_members, group_prefix, seq_prefix,
                              max_prefix: int, seqlen_offset: int = 0, softmax_scale=None, causal: bool = True, k_scale=None, v_scale=None):
    """C-ABI awq_attn_kvcache_paged_shared[_kv8]: `attn_kvcache_paged` for a batch whose sequences share prefixes.  group_members int32
    [num_groups, group_cap] (-1 padding) lists the slots of each group, group_prefix int32 [num_groups] the tokens a group shares,
    seq_prefix int32 [B] the tokens each sequence shares with its group (below 64: ungrouped); `llm_awq_amd.paged_kv.PrefixGroups` keeps
    the three consistent.  max_prefix is the host bound of every prefix, a multiple of 64 in [64, max_seqlen_k];
    group_cap * Sq * (H / Hkv) <= 128.  The keys below a group's prefix are fetched once per (group, KV head, split) through the table row
    of the group's first active member, each member's own keys as in `attn_kvcache_paged`, anchored behind the prefix.  For every active
    sequence of a consistent grouping the result is `attn_kvcache_paged`'s function, and its bits when both chunks of
    `attn_kvcache_shared_plan` are one c with the prefix a multiple of c.  Capturable: a replay follows the lengths, tables and group
    arrays the tensors hold then."""
    who = "attn_kvcache_paged_shared"
    _on_gpu(q)
    if q.dim() != 4 or q.stride(3) != 1 or q.stride(2) != q.shape[3]:
        raise ValueError(f"{who}: q must be [B, Sq, H, Dh] with contiguous heads")
    kv = _check_pools(who, q, k_pool, v_pool, block_table, k_scale, v_scale, q.shape[0])
    if kv.Dh != q.shape[3]:
        raise ValueError(f"{who}: q [B, Sq, H, Dh] and k_pool / v_pool [num_pages, page_size, Hkv, Dh] must share Dh, got {q.shape[3]} and {kv.Dh}")
    B, Sq, H, Dh = q.shape
    _check_seqlens(who, "seqlens_k", seqlens_k, q, B)
    _check_groups(who, q, B, group_members, group_prefix, seq_prefix)
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    L = _capi.lib()
    out = torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    wsb = L.awq_attn_kvcache_shared_workspace_bytes(B, H, kv.Hkv, Dh, Sq, int(max_prefix), int(max_seqlen_k))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=q.device)
    entry = getattr(L, "awq_attn_kvcache_paged_shared" + ("_kv8" if kv.fp8 else ""))
    with torch.cuda.device(q.device):
        _capi.check(entry(q.data_ptr(), *kv.ptrs(), out.data_ptr(), kv.block_table.data_ptr(), B, Sq, seqlens_k.data_ptr(), int(seqlen_offset),
                          int(max_seqlen_k), *kv.table(), H, kv.Hkv, Dh, *q.stride()[:-2], *kv.strides(), scale, int(bool(causal)), _dt(q),
                          group_members.data_ptr(), group_prefix.data_ptr(), seq_prefix.data_ptr(), group_members.shape[0],
                          group_members.shape[1], group_members.stride(0), int(max_prefix), ws.data_ptr(), wsb, _stream(q)))
    return out


def kv_page_copy(k_pool, v_pool, src_pages, dst_pages, k_scale=None, v_scale=None):
    """C-ABI awq_kv_page_copy[_fp8]: page dst_pages[i] of the pools := page src_pages[i] (K and V rows, and the scale rows of FP8 pools),
    one launch for the n pairs.  src_pages / dst_pages int32 [n] on the GPU; a pair with an id outside the pool or with equal ids is
    skipped.  No other byte of the pools is written.  The copy-on-write of the partly filled tail page `PageTable.fork` returns."""
    who = "kv_page_copy"
    fp8 = _fp8_pair(who, k_scale, v_scale)
    _on_gpu(k_pool, v_pool, src_pages, dst_pages, *((k_scale, v_scale) if fp8 else ()))
    for name, t in (("k_pool", k_pool), ("v_pool", v_pool)):
        if fp8:
            _kv8_codes(who, name, t)
        elif t.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"{who}: the pools must be float16 / bfloat16, or FP8 codes with their scales")
        if t.device != k_pool.device or t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
            raise ValueError(f"{who}: {name} must be a [num_pages, page_size, Hkv, Dh] tensor with contiguous heads")
    if k_pool.shape != v_pool.shape or k_pool.dtype != v_pool.dtype:
        raise ValueError(f"{who}: k_pool and v_pool must have one shape and dtype")
    num_pages, page_size, Hkv, Dh = v_pool.shape
    if fp8:
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t.device != k_pool.device or t.dtype != torch.float32 or tuple(t.shape) != (num_pages, page_size, Hkv) or t.stride(2) != 1:
                raise ValueError(f"{who}: {name} must be a float32 [num_pages, page_size, Hkv] tensor with a unit last stride")
    for name, t in (("src_pages", src_pages), ("dst_pages", dst_pages)):
        if t.device != k_pool.device or t.dtype != torch.int32 or t.dim() != 1 or t.shape != src_pages.shape or not t.is_contiguous():
            raise ValueError(f"{who}: src_pages and dst_pages must be contiguous int32 [n] tensors on the GPU of the pools")
    kv = _Kv(k_pool, v_pool, k_scale, v_scale)
    with torch.cuda.device(k_pool.device):
        _capi.check(getattr(_capi.lib(), "awq_kv_page_copy" + ("_fp8" if fp8 else ""))(
            *kv.ptrs(), src_pages.data_ptr(), dst_pages.data_ptr(), src_pages.shape[0], num_pages, page_size, Hkv, Dh, *kv.strides(),
            _stream(k_pool)))


def attn_prefill_paged(q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k: int, seqlen_offset: int = 0, softmax_scale=None,
                       causal: bool = True, k_scale=None, v_scale=None):
    """C-ABI awq_attn_prefill_paged[_kv8]: `attn_prefill_kvcache` over a paged KV cache (`attn_kvcache_paged`'s pools, table and bound): a
    prompt chunk of any length attends the pages its sequence holds.  For every active sequence the result is bit-identical to
    `attn_prefill_kvcache` on the dense gather of its pages.  Entries behind a sequence's live range are never read; a page id is clamped
    into the pool."""
    return _attn_paged("attn_prefill_paged", True, q, k_pool, v_pool, block_table, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal,
                       k_scale, v_scale)


def rope_kv_store_paged(qkv, freqs_table, k_pool, v_pool, block_table, cache_seqlens, nheads: int, nheads_kv: int, k_scale=None, v_scale=None):
    """C-ABI awq_rope_kv_store_paged_pos[_fp8]: `rope_kv_store_natural_pos` over a paged KV cache.  Token s of sequence b is rotated by row
    p = cache_seqlens[b] + s of freqs_table and stored in row p % page_size of page block_table[b, p // page_size] of the pools
    [num_pages, page_size, Hkv, Dh] (the page is looked up per token: a chunk may cross page edges).  A sequence with cache_seqlens[b] < 0
    or cache_seqlens[b] + S > min(pages_per_seq * page_size, P) is inactive: nothing of it is stored and its q rows are zeros.  With
    k_scale / v_scale [num_pages, page_size, Hkv] the pools are FP8.  Returns the rotated q [B, S, H, Dh]."""
    return rope_kv_store_paged_qknorm(qkv, freqs_table, k_pool, v_pool, block_table, cache_seqlens, nheads, nheads_kv, k_scale, v_scale)


def rope_kv_store_paged_qknorm(qkv, freqs_table, k_pool, v_pool, block_table, cache_seqlens, nheads: int, nheads_kv: int, k_scale=None,
                               v_scale=None, *, q_norm=None, k_norm=None, norm_eps: float = 1e-6):
    """`rope_kv_store_paged` with the per-head q/k RMSNorm of `rope_kv_store_natural_pos` (C-ABI awq_rope_kv_store_paged_pos[_fp8]_qknorm): the
    same arguments and, keyword-only, q_norm / k_norm ([Dh], float32 or the input's dtype; both or neither) and norm_eps.  A function of
    its own: `rope_kv_store_paged` keeps its parameter list."""
    who = "rope_kv_store_paged"
    _norm_pair(who, q_norm, k_norm)
    _on_gpu(qkv, freqs_table, cache_seqlens)
    if qkv.dim() != 3 or qkv.stride(2) != 1:
        raise ValueError(f"{who}: qkv must be [B, S, (H + 2 Hkv) * Dh] with a unit last stride")
    kv = _check_pools(who, qkv, k_pool, v_pool, block_table, k_scale, v_scale, qkv.shape[0])
    return _rope_store(who, qkv, freqs_table, kv, nheads, nheads_kv, cache_seqlens=cache_seqlens,
                       norm=_qk_norm(who, qkv, kv.Dh, q_norm, k_norm, norm_eps))


# ---- packed steps (continuous batching): per-sequence numbers of new tokens, read on the device ---------------------------------------
def attn_varq_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, max_seqlen_q: int):
    """Host-side awq_attn_varq_plan: (q_tile_rows, blocks) of a packed-query launch (no GPU needed).  64 rows when max_seqlen_q <= 64,
    otherwise `attn_prefill_plan`'s choice for seqlen_q = max_seqlen_q capped at 128; blocks = ceil(max_seqlen_q / rows) * batch * nheads.
    The rule is provisional, not a measurement.  The knob attn_prefill_rows forces 64 or 128; a forced 256 leaves the plan's own choice."""
    import ctypes

    r, b = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_varq_plan(batch, nheads, nheads_kv, head_dim, max_seqlen_q, ctypes.byref(r), ctypes.byref(b)))
    return r.value, b.value


def _check_packed(who, name, t, cu_seqlens_q, max_seqlen_q):
    """The packed rows `t` [total_q, ..] and their cu_seqlens_q int32 [B + 1]; returns B."""
    _on_gpu(t, cu_seqlens_q)
    if cu_seqlens_q.device != t.device or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 2 or \
            not cu_seqlens_q.is_contiguous():
        raise ValueError(f"{who}: cu_seqlens_q must be a contiguous int32 [B + 1] tensor on the GPU of {name}")
    if cu_seqlens_q.shape[0] - 1 > 65535:
        raise ValueError(f"{who}: batch {cu_seqlens_q.shape[0] - 1} exceeds 65535")
    if int(max_seqlen_q) < 1 or t.shape[0] < 1:
        raise ValueError(f"{who}: max_seqlen_q >= 1 and at least one packed row are expected")
    return cu_seqlens_q.shape[0] - 1


def _packed_out(who, name, given, ref, H, Dh):
    if given is None:
        return torch.empty(ref.shape[0], H, Dh, dtype=ref.dtype, device=ref.device)
    if given.device != ref.device or given.dtype != ref.dtype or tuple(given.shape) != (ref.shape[0], H, Dh) or not given.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous [total_q, H, Dh] tensor of the input's dtype on its GPU")
    return given


def rope_kv_store_varq(qkv, freqs_table, k, v, cu_seqlens_q, max_seqlen_q: int, cache_seqlens, nheads: int, nheads_kv: int, block_table=None,
                       k_scale=None, v_scale=None, q_out=None, *, q_norm=None, k_norm=None, norm_eps: float = 1e-6):
    """C-ABI awq_rope_kv_store_natural_varq[_fp8] / awq_rope_kv_store_paged_varq[_fp8]: `rope_kv_store_natural_pos` / `rope_kv_store_paged`
    over PACKED tokens.  qkv [total_q, (H + 2 Hkv) * Dh] with a unit last stride; sequence b owns rows cu_seqlens_q[b] ..
    cu_seqlens_q[b + 1] - 1 (int32 [B + 1] on the GPU, non-decreasing, cu[0] = 0; the host never reads it).  Token s = t - cu[b] of
    sequence b is rotated by row cache_seqlens[b] + s of freqs_table [P, rot_dim] and stored at that position of k / v -- the contiguous
    caches [Bc >= B, Lmax, Hkv, Dh], or with block_table [>= B, pages_per_seq] the pools [num_pages, page_size, Hkv, Dh]; with k_scale /
    v_scale the FP8 format.  Sq_b = 0 is a slot with nothing to do.  A sequence with cache_seqlens[b] < 0, Sq_b > max_seqlen_q or
    cache_seqlens[b] + Sq_b > min(capacity, P) is inactive: nothing of it is stored and its q rows are zeros.  Rows >= cu[B] (the padding
    of a fixed token budget) are neither read nor written: hand q_out in to keep what they hold.  For every active sequence the rows,
    the cache bytes and the scales are those of the rectangular call on that sequence alone.  Returns the rotated q [total_q, H, Dh].

    q_norm / k_norm (keyword-only, both or neither; [Dh], float32 or the input's dtype) and norm_eps: every q head and every k head is
    RMS-normalised over Dh before the rotation, in the same launch (C-ABI `_qknorm` sibling; Qwen3, Gemma-3) -- y = T((x * rsqrt(mean(x^2)
    + norm_eps)) * gamma), `rmsnorm`'s arithmetic on the head as a row.  v is untouched."""
    who = "rope_kv_store_varq"
    _norm_pair(who, q_norm, k_norm)
    _on_gpu(qkv, freqs_table, cache_seqlens)
    if qkv.dim() != 2 or qkv.stride(1) != 1:
        raise ValueError(f"{who}: qkv must be the packed tokens [total_q, (H + 2 Hkv) * Dh] with a unit last stride")
    B = _check_packed(who, "qkv", qkv, cu_seqlens_q, max_seqlen_q)
    if block_table is not None:
        kv = _check_pools(who, qkv, k, v, block_table, k_scale, v_scale, B)
    else:
        kv = _caches(who, qkv, k, v, k_scale, v_scale)
        if kv.outer < B:
            raise ValueError(f"{who}: batch {B} exceeds the cache batch {kv.outer}")
    return _rope_store(who, qkv, freqs_table, kv, nheads, nheads_kv, cache_seqlens=cache_seqlens, packed=(cu_seqlens_q, max_seqlen_q, q_out),
                       norm=_qk_norm(who, qkv, kv.Dh, q_norm, k_norm, norm_eps))


def attn_prefill_varq(q, k, v, cu_seqlens_q, max_seqlen_q: int, seqlens_k, max_seqlen_k: int, lens_before_step: bool = True, block_table=None,
                      softmax_scale=None, causal: bool = True, k_scale=None, v_scale=None, out=None):
    """C-ABI awq_attn_prefill_kvcache_varq[_kv8] / awq_attn_prefill_paged_varq[_kv8]: `attn_prefill_kvcache` / `attn_prefill_paged` over
    PACKED queries.  q [total_q, H, Dh] with contiguous heads; sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 and brings
    Sq_b = cu[b + 1] - cu[b] <= max_seqlen_q rows (0 is legal).  k / v are the caches [Bc >= B, Lmax, Hkv, Dh] or, with block_table, the
    pools; with k_scale / v_scale FP8 codes.  lens_before_step: Sk_b = seqlens_k[b] + Sq_b -- seqlens_k is then the cache_seqlens that
    `rope_kv_store_varq` took; otherwise Sk_b = seqlens_k[b].  Row s of sequence b attends keys j <= s + Sk_b - Sq_b (causal; a negative
    limit returns zeros) or keys 0 .. Sk_b - 1.  A sequence with Sq_b > max_seqlen_q, Sk_b < 1 or Sk_b > max_seqlen_k is inactive: its
    first min(Sq_b, max_seqlen_q) rows are zeros, nothing else of it is written and none of its keys is read.  Rows >= cu[B] are neither
    read nor written: hand `out` in to keep what they hold.  For every active sequence with Sk_b >= Sq_b the rows are bit-identical to the
    rectangular call on that sequence alone under the same q tile (`attn_varq_plan`).  max_seqlen_q sizes the grid: a loose bound costs
    empty blocks.  Capturable: a replay follows what cu_seqlens_q, the lengths and the table hold then.  Returns out [total_q, H, Dh]."""
    who = "attn_prefill_varq"
    _on_gpu(q)
    if q.dim() != 3 or q.stride(2) != 1 or q.stride(1) != q.shape[2]:
        raise ValueError(f"{who}: q must be the packed rows [total_q, H, Dh] with contiguous heads")
    B = _check_packed(who, "q", q, cu_seqlens_q, max_seqlen_q)
    if block_table is not None:
        kv = _check_pools(who, q, k, v, block_table, k_scale, v_scale, B)
    else:
        kv = _check_caches(who, q, k, v, k_scale, v_scale, packed_batch=B)
    if kv.Dh != q.shape[2]:
        raise ValueError(f"{who}: q [total_q, H, Dh] and k / v [.., Hkv, Dh] must share Dh, got {q.shape[2]} and {kv.Dh}")
    return _attn_kvcache(who, q, kv, seqlens_k, max_seqlen_k, bool(lens_before_step), softmax_scale, causal, one_pass=True,
                         packed=(cu_seqlens_q, max_seqlen_q, out))


# ---- mixed packed steps: the split-KV pair for the short sequences of a step, the one-pass kernel for the rest ---------------------------
ATTN_SPLIT_MIN_KEYS = 2048  # the host-length plan's floor (attn_splitkv_plan never splits below it): the default split_min_keys


def attn_varq_split_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, split_seqlen_q: int, max_seqlen_k: int):
    """Host-side awq_attn_varq_split_plan: (splits, chunk) of the split pair inside `attn_varq` (no GPU needed) -- `attn_kvcache_plan`'s for
    the same bound, the knob attn_splitkv_chunk included.  split_seqlen_q * (H / Hkv) > 128 and head dims other than 64 / 128 are refused."""
    import ctypes

    s, c = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_varq_split_plan(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k, ctypes.byref(s),
                                                     ctypes.byref(c)))
    return s.value, c.value


def attn_varq_window_plan(batch: int, nheads: int, nheads_kv: int, head_dim: int, split_seqlen_q: int, max_seqlen_k: int, window_left: int):
    """Host-side awq_attn_varq_window_plan: (splits, chunk) of the split pair inside `attn_varq_window` (no GPU needed) --
    `attn_kvcache_plan`'s for the bound min(max_seqlen_k, window_left + split_seqlen_q + 63), the most keys a walk anchored at the window
    covers; the knob attn_splitkv_chunk included.  A negative window_left is refused, and whatever `attn_varq_split_plan` refuses."""
    import ctypes

    s, c = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_varq_window_plan(batch, nheads, nheads_kv, head_dim, split_seqlen_q, max_seqlen_k,
                                                      min(int(window_left), 0x7FFFFFFF), ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def attn_varq(q, k, v, cu_seqlens_q, max_seqlen_q: int, seqlens_k, max_seqlen_k: int, split_seqlen_q: int = 1, split_min_keys=None,
              lens_before_step: bool = True, block_table=None, softmax_scale=None, causal: bool = True, k_scale=None, v_scale=None, out=None):
    """C-ABI awq_attn_varq[_kv8] / awq_attn_paged_varq[_kv8]: `attn_prefill_varq`'s arguments and contract for a MIXED packed step.  Three
    launches in one stream -- the packed one-pass kernel, the packed split-KV kernel and its combine -- and every sequence is served by
    exactly one of the two kernels, chosen on the device: the split pair takes sequence b iff it is active with 1 <= Sq_b <=
    split_seqlen_q and Sk_b >= split_min_keys (default 2048, the floor below which `attn_splitkv_plan` never splits); prompt chunks, short
    histories, Sq_b = 0 and inactive sequences stay with the one-pass kernel exactly as in `attn_prefill_varq`.  A taken sequence's rows
    are bit-identical to `attn_kvcache` (`attn_kvcache_paged`) on that sequence alone with seqlen_offset = Sq_b under lens_before_step
    (else 0) and the same max_seqlen_k; every other row to `attn_prefill_varq`.  split_seqlen_q * (H / Hkv) <= 128; split_seqlen_q = 0
    splits nothing and is `attn_prefill_varq`, one launch.  The launch set depends on host arguments only: one captured graph replays any
    mix of decodes, short bursts and prompt chunks.  Errors are raised before any work.  Returns out [total_q, H, Dh].

    `attn_varq_window` is the same step under a sliding window."""
    return _attn_varq("attn_varq", q, k, v, cu_seqlens_q, max_seqlen_q, seqlens_k, max_seqlen_k, split_seqlen_q, split_min_keys, lens_before_step,
                      block_table, softmax_scale, causal, k_scale, v_scale, out, None)


def attn_varq_window(q, k, v, cu_seqlens_q, max_seqlen_q: int, seqlens_k, max_seqlen_k: int, window_left: int, split_seqlen_q: int = 1,
                     split_min_keys=None, lens_before_step: bool = True, block_table=None, softmax_scale=None, causal: bool = True,
                     k_scale=None, v_scale=None, out=None):
    """C-ABI awq_attn_varq_window[_kv8] / awq_attn_paged_varq_window[_kv8]: `attn_varq`'s arguments and contract under a sliding window,
    flash-attn's window_size = (L, 0) with L = window_left (an int >= 0): row s of sequence b stands at position p = s + Sk_b - Sq_b and
    attends keys max(0, p - L) .. p.  A row with p < 0 is zeros as before; every other row attends at least its own key.  The split pair
    takes a sequence iff keys_b = min(Sk_b, L + Sq_b) >= split_min_keys -- the keys it attends at all -- and anchors its splits at
    max(0, Sk_b - Sq_b - L) & ~63 (`attn_varq_window_plan`); no key, scale or table entry below that is read
    (`PageTable.release_before`).  L >= max_seqlen_k - 1 hides nothing and returns the bits of `attn_varq`.  causal = False and a negative
    L are refused before any work.  A function of its own: `attn_varq` keeps its parameter list."""
    if window_left is None:
        raise ValueError("attn_varq_window: window_left must be an int >= 0 (`attn_varq` is the call without a window)")
    return _attn_varq("attn_varq_window", q, k, v, cu_seqlens_q, max_seqlen_q, seqlens_k, max_seqlen_k, split_seqlen_q, split_min_keys,
                      lens_before_step, block_table, softmax_scale, causal, k_scale, v_scale, out, window_left)


def attn_varq_softcap(q, k, v, cu_seqlens_q, max_seqlen_q: int, seqlens_k, max_seqlen_k: int, softcap: float, window_left=None,
                      split_seqlen_q: int = 1, split_min_keys=None, lens_before_step: bool = True, block_table=None, softmax_scale=None,
                      causal: bool = True, k_scale=None, v_scale=None, out=None):
    """C-ABI awq_attn_varq_softcap[_kv8] / awq_attn_paged_varq_softcap[_kv8]: `attn_varq_window`'s arguments and contract with the
    attention logits soft-capped (Gemma-2: softcap 50 with softmax_scale 144 ** -0.5; Grok-1: softcap 30):

        z_j = softcap * tanh(softmax_scale * (q . k_j) / softcap),   then the causal / window mask, then softmax.

    The mask is applied behind the cap, by selection: a masked logit is -inf, not -softcap, and a dead key's score contributes nothing.
    window_left None is a layer without a window, max_seqlen_k - 1.  softcap must be a finite float >= 0; 0 is "no cap" and returns the
    bits of `attn_varq_window`.  A negative, infinite or NaN softcap and causal = False are refused before any work.  The plan is
    `attn_varq_window_plan`.  A function of its own: `attn_varq` and `attn_varq_window` keep their parameter lists."""
    softcap = _check_softcap("attn_varq_softcap", softcap)
    if window_left is None:
        window_left = max(int(max_seqlen_k) - 1, 0)
    return _attn_varq("attn_varq_softcap", q, k, v, cu_seqlens_q, max_seqlen_q, seqlens_k, max_seqlen_k, split_seqlen_q, split_min_keys,
                      lens_before_step, block_table, softmax_scale, causal, k_scale, v_scale, out, window_left, softcap)


def _check_softcap(who, softcap):
    """A cap as a float: finite and >= 0 (0: no cap), as it fits fp32."""
    import math

    try:
        cap = float(softcap)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: softcap must be a float, got {softcap!r}") from None
    if not (math.isfinite(cap) and 0.0 <= cap <= 3.4028234663852886e38):
        raise ValueError(f"{who}: softcap {cap} must be finite and not negative (0: no cap)")
    return cap


def _attn_varq(who, q, k, v, cu_seqlens_q, max_seqlen_q, seqlens_k, max_seqlen_k, split_seqlen_q, split_min_keys, lens_before_step, block_table,
               softmax_scale, causal, k_scale, v_scale, out, window_left, softcap=None):
    """The body of `attn_varq` (window_left None), `attn_varq_window` and `attn_varq_softcap` (softcap a checked float)."""
    if window_left is not None:
        window_left = int(window_left)
        if window_left < 0:
            raise ValueError(f"{who}: window_left {window_left} must not be negative")
        if not causal:
            raise ValueError(f"{who}: a sliding window (window_left) needs causal = True")
        window_left = min(window_left, 0x7FFFFFFF)
    split_seqlen_q = int(split_seqlen_q)
    split_min_keys = ATTN_SPLIT_MIN_KEYS if split_min_keys is None else int(split_min_keys)
    if split_seqlen_q < 0:
        raise ValueError(f"{who}: split_seqlen_q {split_seqlen_q} must not be negative")
    if split_min_keys < 1:
        raise ValueError(f"{who}: split_min_keys {split_min_keys} must be at least 1")
    _on_gpu(q)
    if q.dim() != 3 or q.stride(2) != 1 or q.stride(1) != q.shape[2]:
        raise ValueError(f"{who}: q must be the packed rows [total_q, H, Dh] with contiguous heads")
    B = _check_packed(who, "q", q, cu_seqlens_q, max_seqlen_q)
    if block_table is not None:
        kv = _check_pools(who, q, k, v, block_table, k_scale, v_scale, B)
    else:
        kv = _check_caches(who, q, k, v, k_scale, v_scale, packed_batch=B)
    if kv.Dh != q.shape[2]:
        raise ValueError(f"{who}: q [total_q, H, Dh] and k / v [.., Hkv, Dh] must share Dh, got {q.shape[2]} and {kv.Dh}")
    if kv.Hkv >= 1 and q.shape[1] % kv.Hkv == 0 and split_seqlen_q * (q.shape[1] // kv.Hkv) > 128:
        raise ValueError(f"{who}: split_seqlen_q * (H / Hkv) = {split_seqlen_q * (q.shape[1] // kv.Hkv)} exceeds 128")
    return _attn_kvcache(who, q, kv, seqlens_k, max_seqlen_k, bool(lens_before_step), softmax_scale, causal, one_pass=True,
                         packed=(cu_seqlens_q, max_seqlen_q, out), split=(split_seqlen_q, min(split_min_keys, 0x7FFFFFFF)), window=window_left,
                         softcap=softcap)


def _ft_caches(who, ref, k_cache, v_cache):
    """(Bc, Hkv, Lmax, Dh) of the FT caches k_cache [Bc, Hkv, Dh/8, Lmax, 8] / v_cache [Bc, Hkv, Lmax, Dh], checked against `ref`."""
    for t in (ref, k_cache, v_cache):
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    if k_cache.device != ref.device or v_cache.device != ref.device or k_cache.dtype != ref.dtype or v_cache.dtype != ref.dtype:
        raise ValueError(f"{who}: the caches must have the device and dtype of the input")
    if v_cache.dim() != 4 or k_cache.dim() != 5 or not v_cache.is_contiguous() or not k_cache.is_contiguous():
        raise ValueError(f"{who}: contiguous k_cache [Bc, Hkv, Dh/8, Lmax, 8] and v_cache [Bc, Hkv, Lmax, Dh] are expected")
    Bc, Hkv, Lmax, Dh = v_cache.shape
    if tuple(k_cache.shape) != (Bc, Hkv, Dh // 8, Lmax, 8) or Dh % 8:
        raise ValueError(f"{who}: k_cache must be [Bc, Hkv, Dh/8, Lmax, 8] for v_cache [Bc, Hkv, Lmax, Dh]")
    return Bc, Hkv, Lmax, Dh


def rope_kv_store(qkv, freqs, k_cache, v_cache, start_pos: int, nheads: int, nheads_kv: int):
    """C-ABI awq_rope_kv_store: the prompt side of tinychat's QuantLlamaAttentionFused before the attention, in one launch.
    qkv [B, S, (H + 2 Hkv) Dh] with a unit last stride (batch and row strides of its own), freqs contiguous fp32 with last dim rot_dim
    and B * S * rot_dim angles, read at (s * B + b) * rot_dim + c as fused_rope_with_pos does.  Writes the rotated k into
    k_cache[b, kvh, :, start_pos + s, :] and v into v_cache[b, kvh, start_pos + s, :]; returns the rotated q [B, S, H, Dh]."""
    if not freqs.is_cuda:
        raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    Bc, Hkv, Lmax, Dh = _ft_caches("rope_kv_store", qkv, k_cache, v_cache)
    if freqs.device != qkv.device or freqs.dtype != torch.float32 or not freqs.is_contiguous():
        raise ValueError("rope_kv_store: contiguous float32 freqs on the GPU of qkv are expected")
    if qkv.dim() != 3 or qkv.stride(2) != 1 or nheads_kv != Hkv or qkv.shape[2] != (nheads + 2 * nheads_kv) * Dh:
        raise ValueError("rope_kv_store: qkv must be [B, S, (H + 2 Hkv) * Dh] with a unit last stride and the caches' Hkv and Dh")
    B, S = qkv.shape[0], qkv.shape[1]
    rot = freqs.shape[-1]
    if freqs.numel() < B * S * rot:
        raise ValueError("rope_kv_store: freqs holds fewer than B * S * rot_dim angles")
    q_out = torch.empty(B, S, nheads, Dh, dtype=qkv.dtype, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _capi.check(_capi.lib().awq_rope_kv_store(qkv.data_ptr(), freqs.data_ptr(), q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                                  B, Bc, S, int(nheads), int(nheads_kv), Dh, rot, Lmax, int(start_pos), qkv.stride(0),
                                                  qkv.stride(1), _dt(qkv), _stream(qkv)))
    return q_out


def rope_kv_store_natural(qkv, freqs, k_cache, v_cache, start_pos: int, nheads: int, nheads_kv: int, *, q_norm=None, k_norm=None,
                          norm_eps: float = 1e-6):
    """C-ABI awq_rope_kv_store_natural: rope_kv_store for natural-layout caches k_cache / v_cache [Bc, Lmax, Hkv, Dh] (tinychat's
    long-context path).  Writes the rotated k into k_cache[b, start_pos + s] and v into v_cache[b, start_pos + s]; returns the rotated
    q [B, S, H, Dh].

    q_norm / k_norm (keyword-only, both or neither; [Dh], float32 or the input's dtype) and norm_eps: every q head and every k head is
    RMS-normalised over Dh before the rotation, in the same launch (C-ABI `_qknorm` sibling; Qwen3, Gemma-3) -- y = T((x * rsqrt(mean(x^2)
    + norm_eps)) * gamma), `rmsnorm`'s arithmetic on the head as a row.  v is untouched."""
    _norm_pair("rope_kv_store_natural", q_norm, k_norm)
    _on_gpu(qkv, freqs, k_cache, v_cache)
    if k_cache.device != qkv.device or v_cache.device != qkv.device or k_cache.dtype != qkv.dtype or v_cache.dtype != qkv.dtype:
        raise ValueError("rope_kv_store_natural: the caches must have the device and dtype of the input")
    if v_cache.dim() != 4 or k_cache.shape != v_cache.shape or not v_cache.is_contiguous() or not k_cache.is_contiguous():
        raise ValueError("rope_kv_store_natural: contiguous k_cache / v_cache [Bc, Lmax, Hkv, Dh] of one shape are expected")
    return _rope_store("rope_kv_store_natural", qkv, freqs, _Kv(k_cache, v_cache), nheads, nheads_kv, start_pos=start_pos,
                       norm=_qk_norm("rope_kv_store_natural", qkv, v_cache.shape[3], q_norm, k_norm, norm_eps))


def attn_prefill_ftcache(q, k_cache, v_cache, kv_start: int, seqlen_k: int, softmax_scale=None, causal: bool = True):
    """C-ABI awq_attn_prefill_ftcache: flash_attn_func with K / V read straight from the FT caches; key j of the attention is cache
    position kv_start + j, j < seqlen_k.  q [B, Sq, H, Dh] (batch and row strides of its own, heads contiguous), B <= Bc.  Returns
    [B, Sq, H, Dh] contiguous, bit-identical to flash_attn_func on a contiguous copy of the same keys and values.  Dh 64 or 128."""
    Bc, Hkv, Lmax, Dh = _ft_caches("attn_prefill_ftcache", q, k_cache, v_cache)
    if q.dim() != 4 or q.stride(3) != 1 or q.stride(2) != q.shape[3] or q.shape[3] != Dh:
        raise ValueError("attn_prefill_ftcache: q must be [B, Sq, H, Dh] with contiguous heads and the caches' Dh")
    B, Sq, H, _ = q.shape
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    out = torch.empty(B, Sq, H, Dh, dtype=q.dtype, device=q.device)
    with torch.cuda.device(q.device):
        _capi.check(_capi.lib().awq_attn_prefill_ftcache(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), B, Bc, Sq,
                                                         int(kv_start), int(seqlen_k), H, Hkv, Dh, Lmax, q.stride(0), q.stride(1), scale,
                                                         int(bool(causal)), _dt(q), _stream(q)))
    return out


def attn_varlen_plan(nseq: int, nheads: int, head_dim: int, max_seqlen: int):
    """Host-side awq_attn_varlen_plan: (q_tile_rows, blocks) of the tower attention launch (no GPU needed)."""
    import ctypes

    r, n = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().awq_attn_varlen_plan(nseq, nheads, head_dim, max_seqlen, ctypes.byref(r), ctypes.byref(n)))
    return r.value, n.value


def attn_varlen(q, k, v, cu_seqlens, max_seqlen: int, softmax_scale=None, causal: bool = False, out=None):
    """C-ABI awq_attn_varlen: non-causal attention over packed sequences.  q / k / v [total_rows, H, Dh] with row strides of their own and
    contiguous heads (the three slices qkv[:, i] of a packed [total_rows, 3, H, Dh] tensor pass without a copy), cu_seqlens int32
    [nseq + 1] on the same GPU (read by the kernel only).  Returns [total_rows, H, Dh] contiguous (`out` if given); rows >=
    cu_seqlens[-1] are not written.  Dh 64 or 72, float16 / bfloat16."""
    for t in (q, k, v, cu_seqlens):
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
        if t.device != q.device:
            raise ValueError("attn_varlen: q, k, v and cu_seqlens must live on the same GPU")
    for t in (q, k, v):
        if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError("q / k / v must be [total_rows, heads, Dh] with contiguous heads")
    if k.shape != q.shape or v.shape != q.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("attn_varlen: q, k and v of one shape and dtype are expected")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or not cu_seqlens.is_contiguous():
        raise ValueError("attn_varlen: cu_seqlens must be a contiguous int32 tensor of nseq + 1 entries")
    T, H, Dh = q.shape
    scale = float(Dh) ** -0.5 if softmax_scale is None else float(softmax_scale)
    if out is None:
        out = torch.empty(T, H, Dh, dtype=q.dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != q.dtype or not out.is_contiguous() or out.device != q.device:
        raise ValueError("attn_varlen: out must be a contiguous [total_rows, H, Dh] tensor of q's dtype and device")
    with torch.cuda.device(q.device):
        _capi.check(_capi.lib().awq_attn_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), cu_seqlens.data_ptr(),
                                                cu_seqlens.numel() - 1, int(max_seqlen), T, H, Dh, q.stride(0), k.stride(0), v.stride(0),
                                                scale, int(bool(causal)), _dt(q), _stream(q)))
    return out


def fused_rope_with_pos(x, freqs, transpose_output_memory: bool = False):
    """C-ABI awq_rope_with_pos (the reference's fused_rope_with_pos_forward_func): x [n0, n1, h, d] with a unit last stride, freqs fp32
    with n0 * n1 * d2 elements read at (i1 * n0 + i0) * d2 + c.  The result has x's shape and, when transpose_output_memory, the memory of
    a contiguous [n1, n0, h, d] tensor."""
    for t in (x, freqs):
        if not t.is_cuda:
            raise _capi.AwqNativeError("llm_awq_amd ops run on the GPU only (no CPU fallback)")
    if freqs.device != x.device:
        raise ValueError("fused_rope_with_pos: x and freqs must live on the same GPU")
    if x.dim() != 4 or x.stride(3) != 1 or freqs.dtype != torch.float32 or not freqs.is_contiguous():
        raise ValueError("fused_rope_with_pos: x [n0, n1, h, d] with a unit last stride and contiguous float32 freqs are expected")
    n0, n1, h, d = x.shape
    d2 = freqs.shape[-1]
    if freqs.numel() < n0 * n1 * d2:
        raise ValueError("fused_rope_with_pos: freqs holds fewer than n0 * n1 * d2 angles")
    out = torch.empty(n1, n0, h, d, dtype=x.dtype, device=x.device).transpose(0, 1) if transpose_output_memory else \
        torch.empty(n0, n1, h, d, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_rope_with_pos(x.data_ptr(), freqs.data_ptr(), out.data_ptr(), n0, n1, h, d, d2, x.stride(0), x.stride(1),
                                                  x.stride(2), out.stride(0), out.stride(1), out.stride(2), _dt(x), _stream(x)))
    return out


def rotary_embedding_neox(positions, query, key, head_size: int, cos_sin_cache):
    """C-ABI awq_rope_neox_inplace (the reference's rotary_embedding_neox): rotates contiguous query and key [..., heads, head_size] in place."""
    _need_gpu(positions, query, key, cos_sin_cache)
    if any(t.device != query.device for t in (positions, key, cos_sin_cache)):
        raise ValueError("rotary_embedding_neox: all tensors must live on the same GPU")
    if positions.dtype != torch.int64 or key.shape != query.shape or cos_sin_cache.dtype != query.dtype or key.dtype != query.dtype:
        raise ValueError("rotary_embedding_neox: int64 positions, query and key of one shape, cache of their dtype are expected")
    heads = query.shape[-2]
    tokens = query.numel() // (heads * head_size)
    if positions.numel() != tokens or query.shape[-1] != head_size:
        raise ValueError("rotary_embedding_neox: one position per token and query [..., heads, head_size] are expected")
    with torch.cuda.device(query.device):
        _capi.check(_capi.lib().awq_rope_neox_inplace(positions.data_ptr(), query.data_ptr(), key.data_ptr(), cos_sin_cache.data_ptr(), tokens,
                                                      heads, int(head_size), cos_sin_cache.shape[1], cos_sin_cache.shape[0], _dt(query),
                                                      _stream(query)))


def w8a8_gemm_plan(m: int, n: int, k: int):
    """Host-side awq_w8a8_gemm_plan: (blocks, tile_m, tile_n) of the W8A8 GEMM launch, (0, 0, 0) if the shape is not served (no GPU needed)."""
    import ctypes

    tm, tn = ctypes.c_int(0), ctypes.c_int(0)
    blocks = _capi.lib().awq_w8a8_gemm_plan(int(m), int(n), int(k), ctypes.byref(tm), ctypes.byref(tn))
    return blocks, tm.value, tn.value


def w8a8_gemm(x_i8, w_i8, wscales, ascales, out, bias=None):
    """C-ABI awq_w8a8_gemm: out[M, N] (fp16) = epilogue(x_i8[M, K] . w_i8[N, K]^T) with per-channel wscales [N], per-token ascales [M] and an
    optional fp16 bias [N]; int32 accumulation on the int8 matrix cores.  Written into `out`, which is returned."""
    _need_gpu(x_i8, w_i8, wscales, ascales, out, bias)
    if x_i8.dtype != torch.int8 or w_i8.dtype != torch.int8 or any(t.dtype != torch.float16 for t in (wscales, ascales, out)) or \
            (bias is not None and bias.dtype != torch.float16):
        raise TypeError("w8a8_gemm: int8 x and w, float16 wscales, ascales, bias and out are expected")
    m, k = x_i8.shape
    n = w_i8.shape[0]
    if w_i8.shape[1] != k or out.numel() != m * n or out.shape[-1] != n or wscales.numel() != n or ascales.numel() < m or \
            (bias is not None and bias.numel() != n):
        raise ValueError("w8a8_gemm: x [M, K], w [N, K], wscales [N], ascales [M], bias [N], out [M, N] are expected")
    with torch.cuda.device(x_i8.device):
        _capi.check(_capi.lib().awq_w8a8_gemm(x_i8.data_ptr(), w_i8.data_ptr(), wscales.data_ptr(), ascales.data_ptr(),
                                               None if bias is None else bias.data_ptr(), out.data_ptr(), m, n, k, _stream(x_i8)))
    return out


def quant_per_token(x, out_i8, scale):
    """C-ABI awq_quant_per_token (the reference's invoke_quant): per-token int8 quantisation of x [.., K] into out_i8, scales into scale (fp16)."""
    _need_gpu(x, out_i8, scale)
    if out_i8.dtype != torch.int8 or scale.dtype != torch.float16:
        raise TypeError("quant_per_token: int8 out and float16 scale are expected")
    k = x.shape[-1]
    m = x.numel() // k
    if out_i8.numel() != x.numel() or scale.numel() < m:
        raise ValueError("quant_per_token: out of x's size and one scale per token are expected")
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_quant_per_token(x.data_ptr(), out_i8.data_ptr(), scale.data_ptr(), m, k, _dt(x), _stream(x)))


def gelu_quant_per_token(x, out_i8, scale, tmp):
    """C-ABI awq_gelu_quant_per_token (the reference's gelu_and_quant): tmp = fp16 gelu_fast(x), out_i8 / scale its per-token quantisation."""
    _need_gpu(x, out_i8, scale, tmp)
    if x.dtype != torch.float16 or tmp.dtype != torch.float16 or out_i8.dtype != torch.int8 or scale.dtype != torch.float16:
        raise TypeError("gelu_quant_per_token: float16 x, tmp and scale and int8 out are expected")
    k = x.shape[-1]
    m = x.numel() // k
    if out_i8.numel() != x.numel() or tmp.numel() < x.numel() or scale.numel() < m:
        raise ValueError("gelu_quant_per_token: out and tmp of x's size and one scale per token are expected")
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_gelu_quant_per_token(x.data_ptr(), out_i8.data_ptr(), scale.data_ptr(), tmp.data_ptr(), m, k, _stream(x)))


def layernorm_quant(x, gamma, beta, scale, out_i8, eps: float, per_token: bool = True):
    """C-ABI awq_layernorm_quant (the reference's rms_norm_general): LayerNorm of x [.., K] followed by int8 quantisation.  per_token: scale
    (fp16 [tokens]) is written; otherwise scale[0] is read and multiplied and beta is ignored (the reference's behaviour)."""
    _need_gpu(x, gamma, beta, scale, out_i8)
    if gamma.dtype != x.dtype or (beta is not None and beta.dtype != x.dtype) or out_i8.dtype != torch.int8 or scale.dtype != torch.float16:
        raise TypeError("layernorm_quant: gamma and beta of x's dtype, int8 out and float16 scale are expected")
    k = x.shape[-1]
    m = x.numel() // k
    if out_i8.numel() != x.numel() or gamma.numel() != k or (beta is not None and beta.numel() != k) or scale.numel() < (m if per_token else 1):
        raise ValueError("layernorm_quant: out of x's size, gamma / beta [K] and one scale per token are expected")
    with torch.cuda.device(x.device):
        _capi.check(_capi.lib().awq_layernorm_quant(x.data_ptr(), gamma.data_ptr(), None if beta is None else beta.data_ptr(), float(eps),
                                                     out_i8.data_ptr(), scale.data_ptr(), m, k, int(bool(per_token)), _dt(x), _stream(x)))
