"""The rotary-embedding exports without a GPU: self-checks of the float64 restatements (tests/rope_oracle.py) and the binding's refusals.
(The C entries' argument codes are checked in tests/test_attention_prefill_host.py next to the attention's.)"""
import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_oracle as A
from tests import rope_oracle as R


def test_with_pos_restatement_is_rotate_half_at_one_batch_row():
    """n0 = 1 (tinychat's bsz = 1): the flat index is the sequence position, and the formula is the NeoX rotation of attn_oracle.rotate."""
    torch.manual_seed(1)
    n1, h, d = 9, 3, 64
    x = torch.randn(1, n1, h, d)
    inv = 1.0 / (10000.0 ** (np.arange(0, d, 2) / d))
    pos = np.arange(5, 5 + n1)
    fr = torch.from_numpy(np.concatenate([np.outer(pos, inv)] * 2, -1)).float()[None]
    ref, mag = R.fused_rope_with_pos(x, fr)
    for j, t in enumerate(pos):
        want = A.rotate(x[0, j].double(), int(t), d, 10000.0, 1.0, True, emulate_fp32=False)
        assert float((ref[0, j] - want).abs().max()) < 1e-5  # (freqs are fp32 angles)
    assert (mag > 0).all()


def test_with_pos_flat_index_quirk_and_tail_copy():
    n0, n1, h, d, d2 = 2, 3, 1, 32, 16
    x = torch.ones(n0, n1, h, d)
    fr = torch.arange(n0 * n1 * d2, dtype=torch.float32).reshape(n1, n0, d2) * 0.01
    ref, mag = R.fused_rope_with_pos(x, fr)
    # element (i0, i1, ., c) reads flat[(i1 * n0 + i0) * d2 + c]: not freqs[i0, i1, c]
    i0, i1, c = 1, 2, 3
    a = 0.01 * ((i1 * n0 + i0) * d2 + c)
    assert abs(float(ref[i0, i1, 0, c]) - (np.cos(np.float32(a)) - np.sin(np.float32(a)))) < 1e-6      # first half: partner negated
    c = 11
    a = 0.01 * ((i1 * n0 + i0) * d2 + c)
    assert abs(float(ref[i0, i1, 0, c]) - (np.cos(np.float32(a)) + np.sin(np.float32(a)))) < 1e-6
    assert torch.equal(ref[..., d2:], x[..., d2:].double()) and (mag[..., d2:] == 0).all()


def test_neox_restatement_rotates_pairs_and_leaves_the_tail():
    torch.manual_seed(2)
    T, h, hs, rot = 5, 2, 32, 16
    x = torch.randn(T, h, hs)
    ang = torch.rand(40, rot // 2).double()
    cache = torch.cat([ang.cos(), ang.sin()], -1)
    pos = torch.tensor([3, 0, 39, 7, 7])
    ref, _ = R.rotary_embedding_neox(pos, x, hs, cache)
    xd = x.double()
    for t in range(T):
        a = ang[pos[t]]
        assert torch.allclose(ref[t, :, :8], xd[t, :, :8] * a.cos() - xd[t, :, 8:16] * a.sin())
        assert torch.allclose(ref[t, :, 8:16], xd[t, :, 8:16] * a.cos() + xd[t, :, :8] * a.sin())
        # a rotation keeps the length of every pair
        assert torch.allclose(ref[t, :, :8] ** 2 + ref[t, :, 8:16] ** 2, xd[t, :, :8] ** 2 + xd[t, :, 8:16] ** 2)
    assert torch.equal(ref[..., rot:], xd[..., rot:])


def test_bindings_refuse_cpu_tensors_and_float32():
    eng = llm_awq_amd.load_engine()
    x = torch.zeros(1, 4, 2, 64, dtype=torch.float16)
    fr = torch.zeros(1, 4, 64)
    pos = torch.zeros(1, 4, dtype=torch.int64)
    cache = torch.zeros(8, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.fused_rope_with_pos_forward_func(x, fr, True)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.rotary_embedding_neox(pos, x, x.clone(), 64, cache)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.attn_prefill(x, x, x, 0.125, True)
    # float32 is refused by name, before the device is looked at
    xf = x.float()
    with pytest.raises(RuntimeError, match="float32"):
        eng.fused_rope_with_pos_forward_func(xf, fr, True)
    with pytest.raises(RuntimeError, match="float32"):
        eng.rotary_embedding_neox(pos, xf, xf.clone(), 64, cache.float())
    with pytest.raises(RuntimeError, match="float32"):
        eng.attn_prefill(xf, xf, xf, 0.125, True)
    with pytest.raises(_capi.AwqNativeError):
        ops.fused_rope_with_pos(x, fr)
    with pytest.raises(_capi.AwqNativeError):
        ops.flash_attn_func(x, x, x)
