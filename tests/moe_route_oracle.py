"""numpy / float64 statement of the device-routing contract (include/awq_cdna4.h: awq_moe_route / awq_moe_gather / awq_moe_combine; DESIGN.md
"MoE routing").  No torch arithmetic except the casts to and from bf16 / fp16, which numpy does not have.

  select    the k largest logits of a row in descending order; among equal logits the lower expert index wins; compared through the monotone
            float -> unsigned key (a total order whatever the bits)
  weights   exp(l_j - l_0) / sum_{i < k} exp(l_i - l_0)  (renormalize)   or   / sum_{e < E} exp(l_e - l_0), in float64
  sort      stable sort of the flat slots s = t k + j by expert: order, inv (inv[order[r]] = r), offsets [E + 1]
  gather    xs[r] = x[order[r] // k]
  combine   out[t] = T( sum_j f32( T( f32(ys[inv[t k + j]]) * f32(T(w[t, j])) ) ) ), the sum in fp32, j = 0 .. k - 1 from +0, one final rounding
"""
import numpy as np
import torch


def float_key(a32: np.ndarray) -> np.ndarray:
    """float32 -> uint32, monotone: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    b = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def logits_f32(logits: torch.Tensor) -> np.ndarray:
    """the logits as float32 (exact for fp32 / bf16 / fp16 inputs)"""
    return logits.detach().cpu().float().numpy()


def select(l32: np.ndarray, k: int) -> np.ndarray:
    keys = float_key(l32).astype(np.int64)
    return np.argsort(-keys, axis=1, kind="stable")[:, :k].astype(np.int32)


def weights(l32: np.ndarray, ids: np.ndarray, renormalize: bool = True) -> np.ndarray:
    l = l32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ls = np.take_along_axis(l, ids.astype(np.int64), axis=1)
        p = np.exp(ls - ls[:, :1])
        den = p.sum(1, keepdims=True) if renormalize else np.exp(l - ls[:, :1]).sum(1, keepdims=True)
        return p / den


def sort_slots(ids: np.ndarray, num_experts: int):
    flat = ids.reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=num_experts))]).astype(np.int32)
    return order, inv, offsets


def route(logits: torch.Tensor, k: int, renormalize: bool = True):
    """-> ids int32 [T, k], w float64 [T, k], order int32 [T k], inv int32 [T k], offsets int32 [E + 1]"""
    l32 = logits_f32(logits)
    ids = select(l32, k)
    return (ids, weights(l32, ids, renormalize)) + sort_slots(ids, l32.shape[1])


def gather(x: torch.Tensor, order: np.ndarray, k: int) -> torch.Tensor:
    return x[torch.from_numpy(order.astype(np.int64) // k)]


def combine(ys: torch.Tensor, inv: np.ndarray, w32: np.ndarray) -> torch.Tensor:
    """ys T [T k, H], inv [T k], w32 float32 [T, k] -> T [T, H].  The products of two T values are exact in float64 (and in fp32), so the only
    roundings are the ones the contract names: w to T, each product to T, each fp32 add, the sum to T."""
    dtype = ys.dtype
    T, k = w32.shape
    wt = torch.from_numpy(np.ascontiguousarray(w32, dtype=np.float32)).to(dtype).double()            # T(w)
    rows = ys[torch.from_numpy(inv.astype(np.int64))].view(T, k, -1).double()
    prod = (rows * wt.unsqueeze(-1)).to(dtype).float()                                               # f32(T(y * w))
    acc = torch.zeros(T, rows.shape[2], dtype=torch.float32)
    for j in range(k):
        acc = acc + prod[:, j]
    return acc.to(dtype)


def lattice_logits(rng: np.random.Generator, T: int, E: int) -> np.ndarray:
    """every row a random permutation of E distinct multiples of 1/8 in [-4, 4]: exact in bf16 and fp16, no ties"""
    assert E <= 65
    pick = np.argsort(rng.random((T, 65)), axis=1)[:, :E]
    return ((pick - 32) / 8.0).astype(np.float32)
