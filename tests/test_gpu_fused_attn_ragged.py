"""QuantLlamaAttentionFused(kv_layout="natural") with `start_pos` as a device tensor: a batch of two sequences of different lengths
decoded in one call per step equals, bit for bit, two single-sequence modules stepped with int positions -- on the T cache and on the
FP8 cache."""
from types import SimpleNamespace

import pytest
import torch

from llm_awq_amd import _capi
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID, H, HKV, DH, L = 512, 8, 2, 64, 192
W = (H + 2 * HKV) * DH
PROMPTS, STEPS = (70, 150), 3


def bits(t):
    return t.contiguous().view(torch.int16)


def _module(max_batch_size, kv_layout="natural", kv_dtype=None):
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    # the projections are stand-ins (tests/test_gpu_chunk_prefill.py): x already is the qkv tensor and the output is returned as it is
    return QuantLlamaAttentionFused(HID, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=max_batch_size,
                                    kv_layout=kv_layout, kv_dtype=kv_dtype)


def _table():
    inv = 1.0 / (10000.0 ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(L, device=DEV).float(), inv)
    return torch.cat([f, f], -1).contiguous()  # [L, Dh]: the whole angle table, one row per position


def _draw(g, B, S, dtype):
    mul = torch.cat([torch.full((H * DH,), 1.5), torch.ones(HKV * DH), torch.full((HKV * DH,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * DH), torch.ones(HKV * DH)]).to(DEV)
    return (torch.randn(B, S, W, generator=g, device=DEV) * mul + add).to(dtype)


CACHES = ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale")


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
def test_batched_decode_with_tensor_start_pos_equals_two_single_sequence_modules(kv_dtype, dtype):
    table = _table()
    g = torch.Generator(device=DEV).manual_seed(41)
    batched = _module(2, kv_dtype=kv_dtype)
    singles = [_module(1, kv_dtype=kv_dtype) for _ in PROMPTS]
    names = [n for n in CACHES if hasattr(batched, n)]
    assert len(names) == (4 if kv_dtype else 2)
    _capi.tune(attn_splitkv_chunk=64)
    try:
        # the prompts, one sequence at a time with an int start_pos: sequence b of the batched module lives in row b of its caches
        whole = {n: getattr(batched, n) for n in names}
        for b, n_prompt in enumerate(PROMPTS):
            x = _draw(g, 1, n_prompt, dtype)
            want = singles[b](x, 0, table[:n_prompt])
            for n in names:
                setattr(batched, n, whole[n][b:b + 1])
            got = batched(x, 0, table[:n_prompt])
            for n in names:
                setattr(batched, n, whole[n])
            assert torch.equal(bits(got), bits(want))
        start = torch.tensor(PROMPTS, dtype=torch.int32, device=DEV)
        for t in range(STEPS):
            x = _draw(g, 2, 1, dtype)
            out = batched(x, start, table)
            assert out.shape == (2, 1, H * DH) and torch.isfinite(out.float()).all()
            for b, n_prompt in enumerate(PROMPTS):
                pos = n_prompt + t
                want = singles[b](x[b:b + 1], pos, table[pos:pos + 1])
                assert torch.equal(bits(out[b:b + 1]), bits(want)), (t, b)
            start += 1
        for n in names:  # the caches hold the same bytes: every token landed where the int path puts it
            for b, n_prompt in enumerate(PROMPTS):
                end = n_prompt + STEPS
                assert torch.equal(getattr(batched, n)[b, :end].view(torch.uint8), getattr(singles[b], n)[0, :end].view(torch.uint8)), (n, b)
                assert not getattr(batched, n)[b, end:].view(torch.uint8).any()
        # a finished slot: nothing is stored, its rows are zeros, the other sequence does not notice
        x = _draw(g, 2, 1, dtype)
        before = {n: getattr(batched, n).clone() for n in names}
        out = batched(x, torch.tensor([-1, PROMPTS[1] + STEPS], dtype=torch.int32, device=DEV), table, decode_max_seqlen=160)
        assert not out[0].view(torch.int16).any()
        want = singles[1](x[1:2], PROMPTS[1] + STEPS, table[PROMPTS[1] + STEPS:PROMPTS[1] + STEPS + 1])
        assert torch.equal(bits(out[1:2]), bits(want))
        for n in names:
            assert torch.equal(getattr(batched, n)[0].view(torch.uint8), before[n][0].view(torch.uint8))
    finally:
        _capi.tune(attn_splitkv_chunk=0)


def test_ft_layout_refuses_a_tensor_start_pos():
    m = _module(2, kv_layout="ft")
    x = torch.zeros(2, 1, W, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="natural"):
        m(x, torch.zeros(2, dtype=torch.int32, device=DEV), _table())
    assert not m.cache_k.any() and not m.cache_v.any()
