"""The per-head q/k RMSNorm in front of the rotation (Qwen3, Gemma-3; the rope_kv_store_*_qknorm entries), in torch, device-agnostic:

  * `compose`: the composition the fused launch replaces -- copy the q and k heads out of a qkv tensor, normalise them as rows of Dh, write
    them back into a copy of qkv (v untouched).  `norm` is the row kernel: `ops.rmsnorm` on the GPU for the bit-equality tests,
    `rmsnorm_f32` here for anything on the CPU;
  * `y_fp64`: the norm evaluated in float64, for the one case whose gamma no T holds (Gemma-3's 1 + w);
  * the inputs of that case and the ulp arithmetic both test files share.
"""
import torch


def rmsnorm_f32(rows, gamma, eps):
    """T((x * rsqrt(mean(x^2) + eps)) * gamma) with float32 arithmetic and ONE rounding to T: rows [n, Dh] of T, gamma [Dh] of any dtype."""
    x = rows.float()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return ((x * rstd) * gamma.float()).to(rows.dtype)


def y_fp64(rows, gamma, eps):
    """The same value in float64, not rounded: rows [n, Dh] of T, gamma [Dh] float32."""
    x = rows.double()
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)) * gamma.double()


def compose(qkv, H, Hkv, Dh, q_gamma, k_gamma, eps, norm=rmsnorm_f32):
    """A contiguous copy of qkv [..., (H + 2 Hkv) * Dh] whose q heads are norm(rows, q_gamma, eps) and whose k heads are
    norm(rows, k_gamma, eps); the v heads are qkv's."""
    out = qkv.contiguous().clone()
    lead = out.shape[:-1]
    q = out[..., :H * Dh].reshape(-1, Dh).contiguous()
    k = out[..., H * Dh:(H + Hkv) * Dh].reshape(-1, Dh).contiguous()
    out[..., :H * Dh] = norm(q, q_gamma, eps).reshape(*lead, H * Dh)
    out[..., H * Dh:(H + Hkv) * Dh] = norm(k, k_gamma, eps).reshape(*lead, Hkv * Dh)
    return out


def ordered(t):
    """The bits of a T tensor as integers that grow with the value (-0 and +0 both 0): two finite values are n ulps of T apart iff their
    images differ by n."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b)


def ulp_diff(a, b):
    return (ordered(a) - ordered(b)).abs()


# ---- the case whose gamma no T holds: gamma = 1 + w in float32, eps 1e-6, an angle table of zeros ----------------------------------
ULP_CASE = dict(B=2, S=8, H=4, Hkv=2, Dh=128, eps=1e-6, seed=20260117)
ULP_SHARE_CAP = 0.02  # of the elements may differ from round_T(fp64), each by one ulp of T (the derived expectation: 2^-10 bf16, 2^-7 fp16)


def ulp_case(dtype):
    """(qkv [B, S, (H + 2 Hkv) Dh] of T, q_gamma, k_gamma float32 [Dh]) on the CPU, from the fixed seed.  w is a T value of a few
    hundredths, so 1 + w needs more mantissa bits than T has."""
    c = ULP_CASE
    g = torch.Generator().manual_seed(c["seed"])
    qkv = torch.randn(c["B"], c["S"], (c["H"] + 2 * c["Hkv"]) * c["Dh"], generator=g).to(dtype)
    w = [(0.05 * torch.randn(c["Dh"], generator=g)).to(dtype) for _ in range(2)]
    q_gamma, k_gamma = (1.0 + wi.float() for wi in w)
    assert not torch.equal(q_gamma.to(dtype).float(), q_gamma) and not torch.equal(k_gamma.to(dtype).float(), k_gamma)
    return qkv, q_gamma, k_gamma


def ulp_case_want(qkv, q_gamma, k_gamma):
    """round_T of the float64 evaluation: (q [B, S, H, Dh], k [B, S, Hkv, Dh]) of T."""
    c = ULP_CASE
    B, S, H, Hkv, Dh = c["B"], c["S"], c["H"], c["Hkv"], c["Dh"]
    q = y_fp64(qkv[..., :H * Dh].reshape(-1, Dh), q_gamma, c["eps"]).to(qkv.dtype).reshape(B, S, H, Dh)
    k = y_fp64(qkv[..., H * Dh:(H + Hkv) * Dh].reshape(-1, Dh), k_gamma, c["eps"]).to(qkv.dtype).reshape(B, S, Hkv, Dh)
    return q, k
