"""The latent KV cache of MLA on the GPU (awq_mla_kv_store; csrc/awq_attn_mla_cdna4.hip): the store of a packed step, bit for bit against
the project's rmsnorm and rope ops, dense and paged, with a chunk that crosses a page edge, an inactive sequence and padding rows."""
import pytest
import torch

from llm_awq_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAGE = 64


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def freqs(P):
    inv = 1.0 / (10000.0 ** (torch.arange(32, dtype=torch.float32) / 32))
    a = torch.arange(P, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([a, a], dim=1).contiguous().to(DEV)


def make_cache(B, Lmax, dtype, paged, fill=None, seed=0):
    """(cache, table): dense [B, Lmax, 576], or a pool of shuffled pages with two spare ones; rows(b) reads a sequence back."""
    g = torch.Generator().manual_seed(seed)
    pps = (Lmax + PAGE - 1) // PAGE
    if not paged:
        c = torch.randn(B, Lmax, 576, generator=g).to(dtype).to(DEV) if fill is None else torch.full((B, Lmax, 576), fill, dtype=dtype, device=DEV)
        return c, None, lambda b: c[b]
    n = B * pps + 2
    c = torch.randn(n, PAGE, 576, generator=g).to(dtype).to(DEV) if fill is None else torch.full((n, PAGE, 576), fill, dtype=dtype, device=DEV)
    table = torch.randperm(n, generator=g)[:B * pps].view(B, pps).to(torch.int32).to(DEV)
    return c, table, lambda b: c[table[b].long()].reshape(pps * PAGE, 576)


@pytest.mark.parametrize("dtype, paged, interleaved", [(torch.bfloat16, False, True), (torch.bfloat16, True, False), (torch.float16, True, True),
                                                       (torch.float16, False, False)])
def test_store_bits(dtype, paged, interleaved):
    H, eps, SENT = 20, 1e-6, 7.0
    sq, cs = [9, 2, 1], [60, -1, 0]  # sequence 0 crosses the page edge at 64, sequence 1 is inactive
    cu = [0, 9, 11, 12]
    T = 14                           # two padding rows behind cu[B]
    g = torch.Generator().manual_seed(1)
    kv_buf = torch.randn(T, 640, generator=g).to(dtype).to(DEV)
    q_buf = (torch.randn(T, H, 192, generator=g) * 2).to(dtype).to(DEV)
    kv_a, q_pe = kv_buf[:, :576], q_buf[:, :, 128:]  # strided views
    gamma_t = (1 + 0.1 * torch.randn(512, generator=g)).to(dtype).to(DEV)
    table_f = freqs(128)
    cache, table, rows = make_cache(3, 128, dtype, paged, fill=SENT)
    q_abs = torch.full((T, H, 576), SENT, dtype=dtype, device=DEV)
    ops.mla_kv_store(kv_a, q_pe, q_abs, cache, i32(cu), 9, i32(cs), table_f, gamma_t.float(), eps, block_table=table, rope_interleaved=interleaved)

    pos = torch.tensor([cs[b] + s for b in range(3) for s in range(sq[b])], device=DEV).clamp(min=0)
    perm = torch.cat([torch.arange(0, 64, 2), torch.arange(1, 64, 2)]).to(DEV) if interleaved else torch.arange(64, device=DEV)
    lat = ops.rmsnorm(kv_a[:12, :512].contiguous(), gamma_t, eps)
    fr = table_f[pos].contiguous()
    k_rot = ops.fused_rope_with_pos(kv_a[:12, 512:][:, perm].contiguous().view(1, 12, 1, 64), fr)[0, :, 0]
    q_rot = ops.fused_rope_with_pos(q_pe[:12][:, :, perm].contiguous().view(1, 12, H, 64), fr)[0]
    want = torch.full((3, 128, 576), SENT, dtype=dtype, device=DEV)
    for b in (0, 2):
        sl = slice(cu[b], cu[b + 1])
        want[b, cs[b]:cs[b] + sq[b]] = torch.cat([lat[sl], k_rot[sl]], dim=1)
    for b in range(3):
        assert torch.equal(rows(b).view(torch.int16), want[b].view(torch.int16)), b
    assert torch.equal(q_abs[:, :, :512], torch.full_like(q_abs[:, :, :512], SENT))
    assert torch.equal(q_abs[:9, :, 512:].view(torch.int16), q_rot[:9].view(torch.int16))
    assert torch.equal(q_abs[11, :, 512:].view(torch.int16), q_rot[11].view(torch.int16))
    assert torch.equal(q_abs[9:11, :, 512:], torch.zeros_like(q_abs[9:11, :, 512:]))       # the inactive sequence
    assert torch.equal(q_abs[12:, :, 512:], torch.full_like(q_abs[12:, :, 512:], SENT))    # the padding
