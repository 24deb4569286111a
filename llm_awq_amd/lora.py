"""Multi-LoRA serving on packed steps: many fine-tunes of one 4-bit base model in one batch.

`qweight` cannot absorb a low-rank delta, so the adapters stay beside the base: every adapted linear keeps a pool of `num_slots` adapters
(`a_pool` [S, n_slices * R, K], `b_pool` [S, N, R], `scaling` [S]) and adds `scaling[a] * (x A_a^T) B_a^T` to the base output with
`ops.lora_apply` -- two launches whatever the mix of adapters, decodes and prompt chunks, the adapter of every sequence read on the device
(DESIGN.md "Multi-LoRA").  The step's `adapter_ids` / `cu_seqlens_q` live in ONE `LoRAPool` that every adapted layer reads, so a model's
forward keeps its signature: `QuantLlamaAttentionFused.forward_packed[_split]` calls its linears on the flat [T, hidden] matrix and needs no change.

    pool = LoRAPool(num_slots=8, rank=16, dtype=torch.bfloat16, device="cuda")
    attach_lora(attn, pool)                                   # qkv_proj, o_proj (and down_proj of an MLP) become LoRALinear
    attn.qkv_proj.load_adapter(3, {"q": (A_q, B_q), "k": (A_k, B_k), "v": (A_v, B_v)}, alpha=32, rank=16)
    pool.set_batch(adapter_ids, cu_seqlens_q, max_seqlen_q)   # device tensors, kept by reference: a captured graph sees in-place updates
    out = attn.forward_packed(x, start_pos, freqs, cu_seqlens_q, max_seqlen_q)

The gate / up pair of `QuantLlamaMLP` is adapted by `LoRAGateUp` (`attach_lora_mlp`).  The fused SiLU * mul epilogue of the base launch consumes
gate and up before a delta could be added, so a step with a batch set runs the interleaved gate / up stream WITHOUT its epilogue (`forward_cdna4`
on the same weight), the shrink launch with two slices (x is read once for gate's and up's A) and `ops.lora_expand_gate_up`, which adds the two
deltas and applies the SiLU * mul tail in the same pass: three launches, no adapted [T, 2F] intermediate.  A sequence without an adapter inside such
a step goes through the unfused base launch too; with no batch set the fused launch runs untouched.

    done = attach_lora_mlp(block, pool)                       # {"mlp": LoRAGateUp, "mlp.down_proj": LoRALinear}
    block.mlp.load_adapter(3, {"gate_proj": (A_g, B_g), "up_proj": (A_u, B_u)}, alpha=32, rank=16)

`attach_lora` itself keeps refusing the names gate_proj / up_proj: they are no WQLinear children of the fused module.  3-bit MLPs are out of scope.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops

RANKS = (16, 32, 64)


class LoRAPool:
    """The batch state every adapted layer of a model reads, and the workspace they share.

    `set_batch` keeps REFERENCES to the device tensors it is given: an in-place update of `adapter_ids` or `cu_seqlens_q` is seen by the next
    call and by the next replay of a captured graph.  The workspace is grown by `reserve` (every `LoRALinear` reserves its own need when it is
    built and when a batch is set), never while a stream is being captured."""

    def __init__(self, num_slots: int, rank: int, dtype=torch.bfloat16, device="cuda"):
        if int(rank) not in RANKS:
            raise ValueError(f"LoRAPool: rank {rank} is not supported (supported pool ranks: {RANKS}; smaller adapters are zero-padded)")
        if int(num_slots) < 1:
            raise ValueError("LoRAPool: num_slots >= 1 is expected")
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"LoRAPool: dtype must be float16 or bfloat16, got {dtype}")
        self.num_slots, self.rank, self.dtype, self.device = int(num_slots), int(rank), dtype, torch.device(device)
        self.adapter_ids = None
        self.cu_seqlens_q = None
        self.max_seqlen_q = 1
        self.ws = None
        self.layers = []  # the LoRALinear modules built on this pool (load_adapter / unload by layer name)

    # ---- batch state ----
    def set_batch(self, adapter_ids, cu_seqlens_q=None, max_seqlen_q: int = 1):
        """adapter_ids int32 [B] (outside [0, num_slots): no adapter, -1 is the canonical value), cu_seqlens_q int32 [B + 1] or None (B sequences
        of max_seqlen_q rows each), both on the device and kept by reference."""
        for name, t in (("adapter_ids", adapter_ids), ("cu_seqlens_q", cu_seqlens_q)):
            if t is None and name == "cu_seqlens_q":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"LoRAPool.set_batch: {name} must be a contiguous int32 1-D tensor")
        if cu_seqlens_q is not None and cu_seqlens_q.shape[0] != adapter_ids.shape[0] + 1:
            raise ValueError("LoRAPool.set_batch: cu_seqlens_q must be [B + 1] for adapter_ids [B]")
        if int(max_seqlen_q) < 1:
            raise ValueError("LoRAPool.set_batch: max_seqlen_q >= 1 is expected")
        self.adapter_ids, self.cu_seqlens_q, self.max_seqlen_q = adapter_ids, cu_seqlens_q, int(max_seqlen_q)

    def clear_batch(self):
        self.adapter_ids = self.cu_seqlens_q = None
        self.max_seqlen_q = 1

    @property
    def has_batch(self) -> bool:
        return self.adapter_ids is not None

    # ---- workspace ----
    def reserve(self, nbytes: int):
        """Grow the shared fp32 workspace to at least nbytes.  Refused during a capture: reserve (or run one warm-up step) beforehand."""
        if self.ws is not None and self.ws.numel() * 4 >= nbytes:
            return self.ws
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"LoRAPool: the workspace ({0 if self.ws is None else self.ws.numel() * 4} bytes) must grow to {nbytes} bytes while "
                               "the stream is being captured; call pool.reserve or run the step once before the capture")
        self.ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        return self.ws

    # ---- adapters by layer name ----
    def load_adapter(self, slot: int, tensors: dict, alpha: float, rank: int):
        """tensors: {layer name (as attach_lora recorded it): what that layer's load_adapter takes}.  Every named layer must exist."""
        by_name = {l.lora_name: l for l in self.layers}
        missing = [n for n in tensors if n not in by_name]
        if missing:
            raise KeyError(f"LoRAPool.load_adapter: no adapted layer named {missing} (layers: {sorted(by_name)})")
        for name, t in tensors.items():
            by_name[name].load_adapter(slot, t, alpha, rank)

    def unload(self, slot: int):
        for l in self.layers:
            l.unload(slot)


def _pair(t, who):
    """one (lora_A.weight [r, K], lora_B.weight [N, r]) pair out of a tuple or a PEFT-keyed dict"""
    if isinstance(t, dict):
        a = [v for k, v in t.items() if "lora_A" in k]
        b = [v for k, v in t.items() if "lora_B" in k]
        if len(a) != 1 or len(b) != 1:
            raise ValueError(f"{who}: expected exactly one lora_A.weight and one lora_B.weight, got keys {sorted(t)}")
        return a[0], b[0]
    a, b = t
    return a, b


class LoRALinear(nn.Module):
    """`base` ([.., K] -> [.., N]; a WQLinear in any layout is the intended base) plus this layer's adapter pool.  forward(x) is base(x), then
    ops.lora_apply in place on that output when the pool holds a batch; with no batch set the base output is returned untouched.
    slice_end: the ends of the output slices that carry their own A (the fused qkv layer: (q, q + k, q + k + v) columns); default one slice."""

    def __init__(self, base, pool: LoRAPool, slice_end=None, in_features=None, out_features=None, name=None):
        super().__init__()
        k = int(in_features if in_features is not None else base.in_features)
        n = int(out_features if out_features is not None else base.out_features)
        ends = (n,) if slice_end is None else tuple(int(e) for e in slice_end)
        if not 1 <= len(ends) <= 3 or ends[-1] != n or any(e % 16 for e in ends) or any(b <= a for a, b in zip((0,) + ends, ends)):
            raise ValueError(f"LoRALinear: slice_end {ends} must hold 1 .. 3 strictly increasing multiples of 16 ending at out_features {n}")
        if k < 64 or k % 64 or n % 16:
            raise ValueError(f"LoRALinear: in_features {k} must be a multiple of 64 and out_features {n} a multiple of 16")
        self.base, self.pool, self.slice_end, self.in_features, self.out_features = base, pool, ends, k, n
        self.lora_name = name
        s, r = pool.num_slots, pool.rank
        self.register_buffer("a_pool", torch.zeros(s, len(ends) * r, k, dtype=pool.dtype, device=pool.device))
        self.register_buffer("b_pool", torch.zeros(s, n, r, dtype=pool.dtype, device=pool.device))
        self.register_buffer("scaling", torch.zeros(s, dtype=torch.float32, device=pool.device))
        pool.layers.append(self)

    @property
    def n_slices(self) -> int:
        return len(self.slice_end)

    # what QuantLlamaMLP asks of its down_proj: the base's weight layout, and the switch to the cdna4 interleave
    @property
    def layout(self):
        return getattr(self.base, "layout", None)

    def to_cdna4(self):
        self.base.to_cdna4()
        return self

    def load_adapter(self, slot: int, tensors, alpha: float, rank: int):
        """PEFT-shaped tensors of one adapter into slot `slot`, IN PLACE (a captured graph serves the new adapter on its next replay).
        One slice: (lora_A.weight [r, K], lora_B.weight [N, r]) or a dict holding those two keys.  Several slices: one such pair per slice, as a
        list in slice order or a dict whose values are in slice order.  r <= the pool's rank; rows r .. R - 1 of A and columns r .. R - 1 of B are
        zeros and scaling[slot] = alpha / r."""
        who = "LoRALinear.load_adapter"
        R, r = self.pool.rank, int(rank)
        if not 0 <= int(slot) < self.pool.num_slots:
            raise IndexError(f"{who}: slot {slot} outside [0, {self.pool.num_slots})")
        if r < 1 or r > R:
            raise ValueError(f"{who}: rank {r} outside [1, {R}] (the pool's rank; build the pool with a larger one)")
        if self.n_slices == 1 and (isinstance(tensors, tuple) or (isinstance(tensors, dict) and any("lora_A" in str(k) for k in tensors))):
            tensors = [tensors]
        pairs = [_pair(t, who) for t in (tensors.values() if isinstance(tensors, dict) else tensors)]
        if len(pairs) != self.n_slices:
            raise ValueError(f"{who}: {len(pairs)} (A, B) pairs for {self.n_slices} slices")
        lo = 0
        for j, (a, b) in enumerate(pairs):
            hi = self.slice_end[j]
            if tuple(a.shape) != (r, self.in_features) or tuple(b.shape) != (hi - lo, r):
                raise ValueError(f"{who}: slice {j} expects lora_A.weight [{r}, {self.in_features}] and lora_B.weight [{hi - lo}, {r}], got "
                                 f"{list(a.shape)} and {list(b.shape)}")
            lo = hi
        with torch.no_grad():
            lo = 0
            for j, (a, b) in enumerate(pairs):
                hi = self.slice_end[j]
                rows = self.a_pool[slot, j * R:(j + 1) * R]
                rows[:r].copy_(a)
                rows[r:].zero_()
                cols = self.b_pool[slot, lo:hi]
                cols[:, :r].copy_(b)
                cols[:, r:].zero_()
                lo = hi
            self.scaling[slot] = float(alpha) / r

    def unload(self, slot: int):
        with torch.no_grad():
            self.a_pool[slot].zero_()
            self.b_pool[slot].zero_()
            self.scaling[slot] = 0.0

    @torch.no_grad()
    def forward(self, x):
        y = self.base(x)
        p = self.pool
        if not p.has_batch:
            return y
        y2 = y.view(-1, self.out_features)  # in place: the base output is a fresh contiguous tensor
        x2 = x.reshape(-1, self.in_features)
        ws = p.reserve(ops.lora_workspace_bytes(x2.shape[0], self.in_features, p.rank, self.n_slices))
        ops.lora_apply(x2, y2, self.a_pool, self.b_pool, self.scaling, p.adapter_ids, self.slice_end if self.n_slices > 1 else None,
                       p.cu_seqlens_q, p.max_seqlen_q, ws)
        return y

    def extra_repr(self) -> str:
        return f"slots={self.pool.num_slots}, rank={self.pool.rank}, slice_end={self.slice_end}"


class LoRAGateUp(nn.Module):
    """A `QuantLlamaMLP` (w_bit = 4) plus the adapter pool of its gate / up pair: `a_pool` [S, 2R, K] (gate's rows first, then up's), `b_pool`
    [S, 2F, R] in natural order (B_gate rows, then B_up rows), `scaling` [S].  forward(x) with no batch set on the pool is `mlp(x)`, the fused
    launch untouched; with a batch it is the unfused interleaved stream, `ops.lora_apply_gate_up` and `mlp.down_proj` (which may itself be a
    LoRALinear)."""

    def __init__(self, mlp, pool: LoRAPool, name=None):
        super().__init__()
        from .fused_mlp import QuantLlamaMLP
        if not isinstance(mlp, QuantLlamaMLP):
            raise TypeError(f"LoRAGateUp: a QuantLlamaMLP is expected, got {type(mlp).__name__}")
        if mlp.w_bit != 4:
            raise ValueError(f"LoRAGateUp: w_bit = {mlp.w_bit} is not supported: only the 4-bit gate / up stream has an unfused base launch (W3 is out of scope)")
        k, f = int(mlp.in_features), int(mlp.intermediate_size)
        if k < 64 or k % 64 or f < 8 or f % 8:
            raise ValueError(f"LoRAGateUp: in_features {k} must be a multiple of 64 and the intermediate size {f} a multiple of 8")
        self.mlp, self.pool, self.in_features, self.intermediate_size = mlp, pool, k, f
        self.lora_name = name
        s, r = pool.num_slots, pool.rank
        self.register_buffer("a_pool", torch.zeros(s, 2 * r, k, dtype=pool.dtype, device=pool.device))
        self.register_buffer("b_pool", torch.zeros(s, 2 * f, r, dtype=pool.dtype, device=pool.device))
        self.register_buffer("scaling", torch.zeros(s, dtype=torch.float32, device=pool.device))
        pool.layers.append(self)

    # what the users of a QuantLlamaMLP read of it
    @property
    def down_proj(self):
        return self.mlp.down_proj

    @property
    def out_features(self):
        return self.mlp.out_features

    @property
    def w_bit(self):
        return self.mlp.w_bit

    def load_adapter(self, slot: int, tensors: dict, alpha: float, rank: int):
        """{"gate_proj": pair, "up_proj": pair} into slot `slot`, IN PLACE; a pair is (lora_A.weight [r, K], lora_B.weight [F, r]) or a dict holding
        those two PEFT keys.  Either key may be missing (an adapter that targets one of the two): that half is zeros.  r <= the pool's rank, the rest
        is zero-padded, scaling[slot] = alpha / r.  A refused load writes nothing."""
        who = "LoRAGateUp.load_adapter"
        R, r, K, F = self.pool.rank, int(rank), self.in_features, self.intermediate_size
        if not 0 <= int(slot) < self.pool.num_slots:
            raise IndexError(f"{who}: slot {slot} outside [0, {self.pool.num_slots})")
        if r < 1 or r > R:
            raise ValueError(f"{who}: rank {r} outside [1, {R}] (the pool's rank; build the pool with a larger one)")
        if not isinstance(tensors, dict) or not tensors or any(k not in ("gate_proj", "up_proj") for k in tensors):
            raise ValueError(f"{who}: expected a dict with the keys gate_proj and / or up_proj, got {sorted(tensors) if isinstance(tensors, dict) else type(tensors).__name__}")
        pairs = {}
        for key, t in tensors.items():
            a, b = _pair(t, who)
            if tuple(a.shape) != (r, K) or tuple(b.shape) != (F, r):
                raise ValueError(f"{who}: {key} expects lora_A.weight [{r}, {K}] and lora_B.weight [{F}, {r}], got {list(a.shape)} and {list(b.shape)}")
            pairs[key] = (a, b)
        with torch.no_grad():
            for j, key in enumerate(("gate_proj", "up_proj")):
                rows, cols = self.a_pool[slot, j * R:(j + 1) * R], self.b_pool[slot, j * F:(j + 1) * F]
                if key in pairs:
                    rows[:r].copy_(pairs[key][0])
                    rows[r:].zero_()
                    cols[:, :r].copy_(pairs[key][1])
                    cols[:, r:].zero_()
                else:
                    rows.zero_()
                    cols.zero_()
            self.scaling[slot] = float(alpha) / r

    def unload(self, slot: int):
        with torch.no_grad():
            self.a_pool[slot].zero_()
            self.b_pool[slot].zero_()
            self.scaling[slot] = 0.0

    @torch.no_grad()
    def gate_up(self, x):
        """h [.., F] of a step with a batch set: the unfused interleaved stream, shrink, the fused expand"""
        from . import load_engine
        m, p = self.mlp, self.pool
        if m._fused is None or m._fused[0].device != x.device:
            m._build(x.device)
        c4, s, z, szp, szh = m._fused
        x2 = x.reshape(-1, self.in_features)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        y2 = load_engine().forward_cdna4(x2, c4, s, z, szp, None, szh)  # [T, 2F], columns interleaved 8 + 8, no epilogue
        ws = p.reserve(ops.lora_workspace_bytes(x2.shape[0], self.in_features, p.rank, 2))
        h = ops.lora_apply_gate_up(x2, y2, self.a_pool, self.b_pool, self.scaling, p.adapter_ids, p.cu_seqlens_q, p.max_seqlen_q, ws)
        return h.view(*x.shape[:-1], self.intermediate_size)

    @torch.no_grad()
    def forward(self, x):
        if not self.pool.has_batch:
            return self.mlp(x)
        return self.mlp.down_proj(self.gate_up(x))

    def extra_repr(self) -> str:
        return f"slots={self.pool.num_slots}, rank={self.pool.rank}"


DEFAULT_TARGETS = ("qkv_proj", "o_proj", "down_proj")
_REFUSED = ("gate_proj", "up_proj", "gate_up_proj")


def attach_lora(module: nn.Module, pool: LoRAPool, targets=DEFAULT_TARGETS):
    """Replace the children of `module` (searched recursively) whose attribute name is in `targets` and that are WQLinear modules with LoRALinear
    wrappers on `pool`.  The fused qkv layer of a QuantLlamaAttentionFused gets its three slices from the module's head counts (q: num_heads *
    head_dim columns, k and v: num_key_value_heads * head_dim each); every other target is one slice.  The gate / up pair of QuantLlamaMLP is
    no WQLinear child (one fused stream): naming it raises, attach_lora_mlp adapts it.  Returns the {qualified name: LoRALinear} that were
    attached; those names are what LoRAPool.load_adapter takes."""
    from .qmodule import WQLinear

    bad = [t for t in targets if t in _REFUSED]
    if bad:
        raise ValueError(f"attach_lora: {bad} cannot be adapted here: the gate / up pair of QuantLlamaMLP is one fused stream, not a WQLinear child; "
                         "use attach_lora_mlp")
    done = {}
    for prefix, parent in list(module.named_modules()):
        for name in targets:
            child = getattr(parent, name, None)
            if not isinstance(child, WQLinear):
                continue
            ends = None
            if name == "qkv_proj" and hasattr(parent, "num_key_value_heads") and hasattr(parent, "head_dim"):
                q = parent.num_heads * parent.head_dim
                kv = parent.num_key_value_heads * parent.head_dim
                ends = (q, q + kv, q + 2 * kv)
            qual = f"{prefix}.{name}" if prefix else name
            wrapped = LoRALinear(child, pool, ends, name=qual)
            setattr(parent, name, wrapped)
            done[qual] = wrapped
    if not done:
        raise ValueError(f"attach_lora: no WQLinear child named one of {tuple(targets)} was found")
    return done


def attach_lora_mlp(module: nn.Module, pool: LoRAPool, down_proj: bool = True):
    """Replace every QuantLlamaMLP child of `module` (searched recursively) with a LoRAGateUp on `pool`, and wrap the MLP's down_proj in a LoRALinear
    unless it is wrapped already or down_proj=False.  Returns the {qualified name: module} that were attached: the MLP's own name for the
    LoRAGateUp, "<that name>.down_proj" for the LoRALinear; those names are what LoRAPool.load_adapter takes.  W3 MLPs are refused by name."""
    from .fused_mlp import QuantLlamaMLP
    from .qmodule import WQLinear

    found = [(prefix, parent, name, child) for prefix, parent in list(module.named_modules()) if not isinstance(parent, LoRAGateUp)
             for name, child in list(parent.named_children()) if isinstance(child, QuantLlamaMLP)]
    if not found:
        raise ValueError("attach_lora_mlp: no QuantLlamaMLP child was found")
    bad = [f"{prefix}.{name}" if prefix else name for prefix, _, name, child in found if child.w_bit != 4]
    if bad:
        raise ValueError(f"attach_lora_mlp: {bad} are w_bit = 3 MLPs (W3): their gate / up pair cannot be adapted, only the 4-bit stream has an unfused base launch")
    done = {}
    for prefix, parent, name, child in found:
        qual = f"{prefix}.{name}" if prefix else name
        wrapped = LoRAGateUp(child, pool, name=qual)
        setattr(parent, name, wrapped)
        done[qual] = wrapped
        if down_proj and isinstance(child.down_proj, WQLinear):
            child.down_proj = LoRALinear(child.down_proj, pool, name=f"{qual}.down_proj")
            done[f"{qual}.down_proj"] = child.down_proj
    return done
