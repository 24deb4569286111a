"""QuantLlamaAttentionFused / make_quant_attn -- the MI355X build of tinychat/modules/fused_attn.py:169-324, 327-503, 549-634.

The reference module prepares every prompt chunk in torch: two `fused_rope_with_pos_forward_func` launches, a reshape / permute /
contiguous of K, two strided slice-assigns into the FasterTransformer (FT) caches and, with `chunk_prefilling`, a permute / reshape /
contiguous of the whole cached history back to [B, Sk, Hkv, Dh] for K and for V -- a copy that grows with the history -- before
`flash_attn_func` can run.  Here the prompt side is two launches and nothing proportional to the history is copied:

  * `rope_kv_store` rotates q and k of the fused qkv tensor, writes k and v straight into `cache_k` / `cache_v` at positions
    start_pos .. start_pos + seqlen - 1 and returns the rotated q (csrc/awq_attn_chunk_cdna4.hip);
  * `attn_prefill_ftcache` is the prefill attention kernel with K / V staged from those caches (csrc/awq_attn_prefill_cdna4.hip):
    keys 0 .. start_pos + seqlen - 1 with `chunk_prefilling`, keys start_pos .. start_pos + seqlen - 1 without (the reference then
    attends the new chunk only).

Both give the bits of the reference's composition on this package's kernels (rope x 2, the torch stores, `flash_attn_func` on the
gathered copies).  One token (`seqlen == 1`) goes to `single_query_attention` exactly as the reference calls it.

`QuantLlamaAttentionFusedFlash` is an alias: its `short_forward` is this data flow.  The reference's long-context variant (natural-layout
caches [B, L, Hkv, Dh] and `long_forward` for kv_max_seq_len > 8192, fused_attn.py:389-415, 505-546) is `kv_layout="natural"`: every call,
one token included, is `rope_kv_store_natural` (q and k rotated, k and v stored, one launch) followed by
`flash_attn_func(q, cache_k[:, :pos], cache_v[:, :pos], causal=True)`, which takes the split-KV kernels (csrc/awq_attn_splitkv_cdna4.hip)
once the history reaches 2048 keys and few query rows ask -- the decode phase -- and the one-pass prefill kernel otherwise.

`kv_dtype="fp8"` (natural layout only) keeps that path on an FP8 cache: `cache_k` / `cache_v` hold OCP e4m3fn codes, one byte per element,
and `cache_k_scale` / `cache_v_scale` [B, L, Hkv] one fp32 scale per (token, KV head) -- half the memory and half the bytes a decode step
streams.  Every call is `rope_kv_store_natural_fp8` (rotation, quantisation and store in one launch) followed by `ops.attn_kv8`, the same
two attention kernels with the dequantisation in their staging step (csrc/awq_kv8.hpp); the result is, bit for bit, the T-cache path's on
the dequantised caches.

With `kv_layout="natural"`, `forward` also takes `start_pos` as an int32 device tensor [bsz] (and `freqs` as the whole angle table): the
store launch and the split-KV attention then read every sequence's position on the device (`rope_kv_store_natural_pos[_fp8]`,
`attn_kvcache[_kv8]`).  One call serves a batch whose sequences have different lengths, and one captured graph replays the whole decode
phase while the caller advances the tensor in place.  An int `start_pos` takes the path above, bit for bit.

With `block_table=` and `page_size=` (and a tensor `start_pos`) the module's caches are read and written as a POOL of
max_batch_size * kv_max_seq_len / page_size pages -- a view, nothing is copied or allocated -- through the per-sequence block table
(`rope_kv_store_paged_pos[_fp8]`, `attn_kvcache_paged[_kv8]`; `llm_awq_amd.paged_kv.PageTable` hands the pages out): a sequence holds the
pages its tokens need, not kv_max_seq_len rows, and one sequence may grow past kv_max_seq_len while others are short.
`forward_shared(x, start_pos, freqs, block_table, page_size, prefix_groups)` is that call for sequences that share a prompt
(`PageTable.fork`, `llm_awq_amd.paged_kv.PrefixGroups`): the decode attention is `attn_kvcache_paged_shared[_kv8]` (csrc/awq_shared.hpp),
which fetches the pages below a group's prefix once for the group.

Under a tensor `start_pos` a chunk of ANY length is served, with and without pages, T and FP8: up to seqlen * (H / Hkv) = 128 query rows per
KV head the attention is the split-KV pair above; a longer chunk -- a prompt -- goes to the one-pass prefill kernel under the same device
lengths (`attn_prefill_kvcache[_kv8]`, `attn_prefill_paged[_kv8]`, csrc/awq_attn_prefill_cdna4.hip).  A server prefills into the pool
with one `forward` per chunk; a chunked prefill is one captured graph, replayed while `start_pos += chunk` runs on the device.

`forward_packed(x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, ...)` is a PACKED step of continuous batching: `x` is [1, T, hidden], the new tokens of all
sequences in one run of rows with per-sequence counts read on the device (`rope_kv_store_{natural,paged}_varq[_fp8]`,
`attn_prefill[_paged]_varq[_kv8]`, csrc/awq_varq.hpp) -- decodes, prompt chunks and idle slots in one store launch and one attention
launch, and one captured graph for every step of a fixed token budget.

`sliding_window=W` (Mistral-7B-v0.1, Gemma-2/3 local layers, Qwen2 with `use_sliding_window`; `make_quant_attn_window`) makes every row attend W keys, itself included
-- the HF eager mask -- on the packed routes: `forward_packed`, `forward_packed_split` and `forward` under a tensor `start_pos` call
`attn_varq_window[_kv8]` / `attn_paged_varq_window[_kv8]` with window_left = W - 1 (csrc/awq_window.hpp).  A decode step then reads W keys
however long the history is, and `PageTable.release_before` returns the pages the window has left behind.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import load_engine


class QuantLlamaAttentionFused(nn.Module):
    """Same constructor, attributes and forward as the reference class (fused_attn.py:169-324); `max_batch_size` is the module-level
    global there (:21) and a keyword here.  `cache_k` [max_batch_size, Hkv, Dh/8, kv_max_seq_len, 8] and `cache_v`
    [max_batch_size, Hkv, kv_max_seq_len, Dh] are the FT caches the decode kernel reads and writes.  `kv_layout="natural"` is the
    reference's long-context mode (QuantLlamaAttentionFusedFlash with kv_max_seq_len > 8192): both caches are
    [max_batch_size, kv_max_seq_len, Hkv, Dh] and forward is long_forward's data flow for every seqlen.  `kv_dtype="fp8"` (with
    `kv_layout="natural"`) makes them float8_e4m3fn and adds `cache_k_scale` / `cache_v_scale` [max_batch_size, kv_max_seq_len, Hkv]
    float32; `kv_dtype=None` is the cache of the activations' dtype.  `sliding_window=W` (an int >= 1; None: full attention, nothing
    changes): each row attends W keys, itself included; the config is never read for it.  It is served on the packed routes of the
    natural layout only: an int `start_pos`, `kv_layout="ft"` and `chunk_prefilling` on the FT path raise NotImplementedError.
    `qk_norm=(q_weight, k_weight, eps)` (None: no norm, nothing changes) is the per-head RMSNorm of Qwen3 / Gemma-3: every q head and every k
    head is normalised over head_dim between the qkv projection and the rotation, inside the store launch of every natural-layout route
    (the `rope_kv_store_*_qknorm` entries).  The weights [head_dim] are held as the float32 buffers `q_norm_weight` / `k_norm_weight`
    (Gemma-3 hands in 1 + w, formed in float32); `kv_layout="ft"` with `qk_norm` raises NotImplementedError.  `head_dim` is
    `args.head_dim` where the config declares one (Qwen3: hidden 1024, 16 heads, head_dim 128), else hidden_size // num_heads.
    `softmax_scale=s` (None: head_dim ** -0.5, nothing changes) replaces head_dim ** -0.5 on every path that takes a scale (Gemma-2-27B:
    144 ** -0.5, its query_pre_attn_scalar); the FT decode kernel (int `start_pos`, one token, `kv_layout="ft"`) forms its own scale and
    raises NotImplementedError with one.  `attn_softcap=c` (None: no cap, nothing changes; Gemma-2 50, Grok-1 30) caps the attention logits
    as c * tanh(s * q.k / c) in front of the mask.  It is served where the window is -- `forward_packed`, `forward_packed_split` and `forward`
    with a tensor `start_pos`, on the attn_*_varq_softcap entries, a layer without `sliding_window` with a window that hides nothing; an int
    `start_pos`, `kv_layout="ft"`, `forward_shared` and FT `chunk_prefilling` raise NotImplementedError before any work."""

    def __init__(self, hidden_size, num_heads, kv_max_seq_len, qkv_layer, o_proj, dev, args, max_batch_size=1, kv_layout="ft", kv_dtype=None,
                 sliding_window=None, qk_norm=None, attn_softcap=None, softmax_scale=None):
        super().__init__()
        for name, val in (("attn_softcap", attn_softcap), ("softmax_scale", softmax_scale)):
            if val is not None and (isinstance(val, bool) or not isinstance(val, (int, float)) or not (0.0 < float(val) < float("inf"))):
                raise ValueError(f"QuantLlamaAttentionFused: {name} {val!r} must be None or a finite float > 0")
        self.attn_softcap = None if attn_softcap is None else float(attn_softcap)
        self._scale_given = softmax_scale is not None
        if sliding_window is not None and (isinstance(sliding_window, bool) or int(sliding_window) != sliding_window or int(sliding_window) < 1):
            raise ValueError(f"QuantLlamaAttentionFused: sliding_window {sliding_window!r} must be None or an int >= 1 (the keys a row attends, "
                             "itself included)")
        self.sliding_window = None if sliding_window is None else int(sliding_window)
        if kv_layout not in ("ft", "natural"):
            raise ValueError(f"QuantLlamaAttentionFused: kv_layout {kv_layout!r} is not supported (supported: 'ft', 'natural')")
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"QuantLlamaAttentionFused: kv_dtype {kv_dtype!r} is not supported (supported: None, 'fp8')")
        if kv_dtype == "fp8" and kv_layout != "natural":
            raise ValueError("QuantLlamaAttentionFused: kv_dtype 'fp8' needs kv_layout 'natural' (the FT decode kernel reads a cache of the "
                             "activations' dtype)")
        if qk_norm is not None and kv_layout != "natural":
            raise NotImplementedError("QuantLlamaAttentionFused: qk_norm is not implemented on the FT cache (kv_layout 'ft': its decode kernel "
                                      "rotates q and k itself); use kv_layout 'natural'")
        self.kv_layout = kv_layout
        self.kv_dtype = kv_dtype
        self.args = args
        self.n_local_heads = args.num_attention_heads
        self.hidden_size = args.hidden_size
        self.num_heads = args.num_attention_heads
        self.head_dim = self.hidden_size // self.num_heads
        if getattr(args, "head_dim", None) is not None:  # declared independently of hidden_size / num_heads (Qwen3, Gemma-3)
            self.head_dim = int(args.head_dim)
        self.num_key_value_heads = args.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.max_position_embeddings = getattr(args, "max_position_embeddings", None)
        self.rope_theta = args.rope_theta
        self.rope_scaling = getattr(args, "rope_scaling", None)
        if self.rope_scaling is None:
            self.rope_scaling = 1.0
        if isinstance(self.rope_scaling, dict):
            self.rope_scaling = self.rope_scaling.get("factor", 1.0)
        if self.head_dim not in (64, 128):
            raise ValueError(f"QuantLlamaAttentionFused: head dim {self.head_dim} is not supported (supported head dims: 64, 128)")
        self.softmax_scale = self.head_dim ** -0.5 if softmax_scale is None else float(softmax_scale)
        self.qk_norm_eps = None
        if qk_norm is not None:
            q_weight, k_weight, eps = qk_norm
            for name, w in (("q_weight", q_weight), ("k_weight", k_weight)):
                if tuple(w.shape) != (self.head_dim,):
                    raise ValueError(f"QuantLlamaAttentionFused: qk_norm {name} must be [head_dim] = [{self.head_dim}], got {tuple(w.shape)}")
            self.qk_norm_eps = float(eps)
            if not (self.qk_norm_eps >= 0.0 and self.qk_norm_eps != float("inf")):
                raise ValueError(f"QuantLlamaAttentionFused: qk_norm eps must be finite and >= 0, got {eps!r}")
            self.register_buffer("q_norm_weight", q_weight.detach().to(device=dev, dtype=torch.float32).contiguous().clone())
            self.register_buffer("k_norm_weight", k_weight.detach().to(device=dev, dtype=torch.float32).contiguous().clone())
        self.qkv_proj = qkv_layer
        self.o_proj = o_proj
        self.kv_max_seq_len = kv_max_seq_len
        self.max_batch_size = max_batch_size
        if kv_layout == "natural":  # fused_attn.py:389-415
            shape = (max_batch_size, kv_max_seq_len, self.num_key_value_heads, self.head_dim)
            if kv_dtype == "fp8":
                self.cache_v = torch.zeros(shape, dtype=torch.float8_e4m3fn, device=dev)
                self.cache_k = torch.zeros(shape, dtype=torch.float8_e4m3fn, device=dev)
                self.cache_v_scale = torch.zeros(shape[:3], dtype=torch.float32, device=dev)
                self.cache_k_scale = torch.zeros(shape[:3], dtype=torch.float32, device=dev)
                return
            self.cache_v = torch.zeros(shape, dtype=torch.float16, device=dev)
            self.cache_k = torch.zeros(shape, dtype=torch.float16, device=dev)
            return
        # following the FasterTransformer definition (fused_attn.py:196-224); 8 = the fp16 / bf16 elements of one 16-byte chunk
        self.cache_v = torch.zeros((max_batch_size, self.num_key_value_heads, kv_max_seq_len, self.head_dim), dtype=torch.float16, device=dev)
        self.cache_k = torch.zeros((max_batch_size, self.num_key_value_heads, self.head_dim // 8, kv_max_seq_len, 8), dtype=torch.float16,
                                   device=dev)

    def _store(self, eng, entry, xqkv, *args):
        """eng.<entry>(xqkv, *args) -- or with `qk_norm` its `_qknorm` sibling, which takes the gammas and eps behind the same arguments."""
        if self.qk_norm_eps is None:
            return getattr(eng, entry)(xqkv, *args)
        if self.q_norm_weight.device != xqkv.device:
            self.q_norm_weight = self.q_norm_weight.to(xqkv.device)
            self.k_norm_weight = self.k_norm_weight.to(xqkv.device)
        return getattr(eng, entry + "_qknorm")(xqkv, *args, self.q_norm_weight, self.k_norm_weight, self.qk_norm_eps)

    @torch.no_grad()
    def forward(self, x, start_pos, freqs, mask=None, chunk_prefilling=False, decode_max_seqlen=None, block_table=None, page_size=None):
        """`mask` is accepted and ignored, as in the reference's short_forward: the attention is causal.

        With `kv_layout="natural"`, `start_pos` may be an int32 tensor [bsz] on the GPU: the tokens already in each sequence's cache, read
        by the kernels only (a ragged batch in one call; a captured graph replays any position; any seqlen -- a chunk with
        seqlen * (H / Hkv) > 128 takes the one-pass prefill kernel, a shorter one the split-KV pair).  `freqs` is then the model's whole angle
        table [P, rot_dim] and `decode_max_seqlen` (default `kv_max_seq_len`) the host bound on start_pos + seqlen that sizes the attention
        launch.  A sequence with start_pos[b] < 0 is a finished slot: nothing is stored for it and its attention rows are zeros.

        `block_table` (int32 [>= bsz, pages_per_seq] on the GPU) and `page_size` (a multiple of 64 that divides `kv_max_seq_len`) come
        together and with a tensor `start_pos`: the caches are then a pool of max_batch_size * kv_max_seq_len / page_size pages and token
        p of sequence b lives in row p % page_size of page block_table[b, p // page_size].  `decode_max_seqlen` defaults to
        pages_per_seq * page_size.

        A PACKED step of continuous batching (per-sequence numbers of new tokens) is `forward_packed`.

        With `sliding_window` or `attn_softcap` the call needs a tensor `start_pos`: it builds the uniform cu_seqlens_q = [0, seqlen, 2 seqlen, ..] on the
        device and is `forward_packed_split` on the batch as one packed step (split_seqlen_q = seqlen while seqlen * (H / Hkv) <= 128,
        else 0)."""
        if self.sliding_window is not None:
            self._check_window(start_pos, chunk_prefilling)
        if self.attn_softcap is not None:
            self._check_window(start_pos, chunk_prefilling, "attn_softcap")
        if block_table is not None or page_size is not None:
            self._check_paged(start_pos, block_table, page_size)
        eng = load_engine()
        bsz, seqlen, _ = x.shape
        if self.sliding_window is not None or self.attn_softcap is not None:
            from .ops import ATTN_SPLIT_MIN_KEYS

            cu = torch.arange(0, (bsz + 1) * seqlen, seqlen, dtype=torch.int32, device=x.device)
            ssq = seqlen if seqlen * self.num_key_value_groups <= 128 else 0
            out = self._forward_packed(x.reshape(1, bsz * seqlen, -1), start_pos, freqs, cu, seqlen, decode_max_seqlen, block_table, page_size,
                                       (ssq, ATTN_SPLIT_MIN_KEYS))
            return out.view(bsz, seqlen, -1)
        if isinstance(start_pos, torch.Tensor):
            return self._forward_device_pos(eng, x, start_pos, freqs, decode_max_seqlen, block_table, page_size)
        xqkv = self.qkv_proj(x)
        if self.kv_dtype == "fp8":  # the caches keep their dtype: only the device follows the activations
            from . import ops

            if self.cache_k.device != xqkv.device:
                for name in ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale"):
                    setattr(self, name, getattr(self, name).to(xqkv.device))
            xq = self._store(eng, "rope_kv_store_natural_fp8", xqkv.reshape(bsz, seqlen, -1), freqs, self.cache_k, self.cache_v,
                             self.cache_k_scale, self.cache_v_scale, start_pos, self.n_local_heads, self.num_key_value_heads)
            end = start_pos + seqlen
            output = ops.attn_kv8(xq, self.cache_k[:bsz, :end], self.cache_v[:bsz, :end], self.cache_k_scale[:bsz, :end],
                                  self.cache_v_scale[:bsz, :end], **self._scale_kw(), causal=True)
            return self.o_proj(output.view(bsz, seqlen, -1))
        if self.cache_k.dtype != xqkv.dtype or self.cache_k.device != xqkv.device:  # the reference's .to(xq) (:256-257)
            self.cache_k = self.cache_k.to(xqkv)
            self.cache_v = self.cache_v.to(xqkv)
        if self.kv_layout == "natural":  # long_forward (fused_attn.py:505-546); `chunk_prefilling` changes nothing there: the history is attended
            from .flash_attn_compat import flash_attn_func

            xq = self._store(eng, "rope_kv_store_natural", xqkv.reshape(bsz, seqlen, -1), freqs, self.cache_k, self.cache_v, start_pos,
                             self.n_local_heads, self.num_key_value_heads)
            output = flash_attn_func(xq, self.cache_k[:bsz, :start_pos + seqlen], self.cache_v[:bsz, :start_pos + seqlen], **self._scale_kw(),
                                     causal=True)
            return self.o_proj(output.view(bsz, seqlen, -1))
        if seqlen > 1:
            xq = eng.rope_kv_store(xqkv.reshape(bsz, seqlen, -1), freqs, self.cache_k, self.cache_v, start_pos, self.n_local_heads,
                                   self.num_key_value_heads)
            kv_start, seqlen_k = (0, start_pos + seqlen) if chunk_prefilling else (start_pos, seqlen)
            output = eng.attn_prefill_ftcache(xq, self.cache_k, self.cache_v, kv_start, seqlen_k, self.softmax_scale, True)
            output = output.view(bsz, seqlen, -1)
        else:
            if self._scale_given:
                raise NotImplementedError("QuantLlamaAttentionFused: softmax_scale is not implemented for the FT decode kernel (int start_pos, one "
                                          "token, kv_layout 'ft': it forms head_dim ** -0.5 itself); use kv_layout 'natural'")
            xqkv = xqkv.view(bsz, self.n_local_heads + self.num_key_value_heads * 2, self.head_dim)
            xq = xqkv[:, :self.n_local_heads]
            xk = xqkv[:, self.n_local_heads:self.n_local_heads + self.num_key_value_heads]
            xv = xqkv[:, -self.num_key_value_heads:]
            output = eng.single_query_attention(xq, xk, xv, self.cache_k, self.cache_v, None, None, start_pos, self.head_dim, self.rope_theta,
                                                self.rope_scaling, True)
            output = output.reshape(bsz, 1, -1)
        return self.o_proj(output)

    def _scale_kw(self):
        """softmax_scale for the calls that default to head_dim ** -0.5 themselves: handed over only when the module was given one."""
        return {"softmax_scale": self.softmax_scale} if self._scale_given else {}

    def _check_window(self, start_pos, chunk_prefilling=False, what="sliding_window"):
        """What `sliding_window` (and `attn_softcap`, which rides the windowed entries) is not built for, refused before any work."""
        who = "QuantLlamaAttentionFused"
        if self.kv_layout != "natural":
            if chunk_prefilling:
                raise NotImplementedError(f"{who}: {what} is not implemented for chunk_prefilling on the FT cache (kv_layout 'ft'); "
                                          "use kv_layout 'natural' with start_pos as a tensor")
            raise NotImplementedError(f"{who}: {what} is not implemented on the FT cache (kv_layout 'ft'); use kv_layout 'natural'")
        if not isinstance(start_pos, torch.Tensor):
            raise NotImplementedError(f"{who}: {what} is not implemented for an int start_pos (the host-length path); pass start_pos "
                                      "as an int32 tensor [bsz] on the GPU")

    def _check_paged(self, start_pos, block_table, page_size):
        """The paged call's conditions, before any work."""
        who = "QuantLlamaAttentionFused"
        if self.kv_layout != "natural":
            raise ValueError(f"{who}: block_table needs kv_layout 'natural' (the FT-layout cache is not paged)")
        if not isinstance(start_pos, torch.Tensor):
            raise ValueError(f"{who}: block_table needs start_pos as an int32 tensor [bsz] on the GPU (the paged kernels read every "
                             "sequence's position on the device)")
        if block_table is None or page_size is None:
            raise ValueError(f"{who}: block_table and page_size come together")
        page_size = int(page_size)
        if page_size < 64 or page_size % 64 or self.kv_max_seq_len % page_size:
            raise ValueError(f"{who}: page_size {page_size} must be a multiple of 64 that divides kv_max_seq_len {self.kv_max_seq_len}")

    def _check_packed(self, x, start_pos, cu_seqlens_q, max_seqlen_q):
        """The packed call's conditions, before any work."""
        who = "QuantLlamaAttentionFused"
        if cu_seqlens_q is None or max_seqlen_q is None:
            raise ValueError(f"{who}: cu_seqlens_q and max_seqlen_q come together")
        if self.kv_layout != "natural":
            raise ValueError(f"{who}: cu_seqlens_q needs kv_layout 'natural' (the FT-layout cache takes one seqlen for the batch)")
        if not isinstance(start_pos, torch.Tensor):
            raise ValueError(f"{who}: cu_seqlens_q needs start_pos as an int32 tensor [B] on the GPU (the packed kernels read every "
                             "sequence's position on the device)")
        if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or \
                cu_seqlens_q.shape[0] != start_pos.shape[0] + 1:
            raise ValueError(f"{who}: cu_seqlens_q must be an int32 tensor [B + 1] on the GPU for start_pos [B]")
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"{who}: cu_seqlens_q needs x as the packed tokens [1, T, hidden], got {tuple(x.shape)}")
        if int(max_seqlen_q) < 1:
            raise ValueError(f"{who}: max_seqlen_q {int(max_seqlen_q)} must be at least 1")

    @torch.no_grad()
    def forward_packed(self, x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, decode_max_seqlen=None, block_table=None, page_size=None):
        """A PACKED step of continuous batching.  `x` is [1, T, hidden], the new tokens of all B sequences in one run of rows; sequence b
        owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 (`cu_seqlens_q` int32 [B + 1] on the GPU; any mix of counts, 0 included;
        rows >= cu_seqlens_q[B] are the padding of a fixed token budget) and `max_seqlen_q` is the host bound of every count.  `start_pos`
        is the int32 tensor [B], `freqs` the whole angle table, `kv_layout` "natural" -- dense or with `block_table` / `page_size`, T or
        FP8; `decode_max_seqlen` as in `forward`.  A method of its own and not two more keywords of `forward`, whose parameter list is the
        reference's plus the paged pair.

        rope_kv_store_natural_varq[_fp8] / rope_kv_store_paged_varq[_fp8] followed by attn_prefill_varq[_kv8] / attn_prefill_paged_varq
        [_kv8] with lens_before_step: start_pos is what both launches take, and no length or token count reaches the host.  Returns
        [1, T, hidden].  The rows of the sequences' last tokens (what the LM head needs) are out[:, cu_seqlens_q[1:] - 1], a device gather
        that a graph captures.  Errors are raised before any work.

        `forward_packed_split` is the same step with the short sequences over a long history served by the split-KV pair."""
        return self._forward_packed(x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, decode_max_seqlen, block_table, page_size, None)

    @torch.no_grad()
    def forward_packed_split(self, x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, split_seqlen_q=1, split_min_keys=None,
                             decode_max_seqlen=None, block_table=None, page_size=None):
        """`forward_packed` with the attention of the step routed to attn_varq[_kv8] / attn_paged_varq[_kv8]: a sequence that brings at most
        `split_seqlen_q` new tokens over at least `split_min_keys` keys (default `ops.ATTN_SPLIT_MIN_KEYS`) is served by the packed split-KV
        pair, every other sequence by the one-pass kernel as in `forward_packed` -- decided on the device, so one captured graph serves
        any mix of decodes and prompt chunks.  split_seqlen_q * (H / Hkv) <= 128; split_seqlen_q = 0 is `forward_packed`'s attention.  The
        store launch, the cache bytes and the rows of the sequences the pair does not take are `forward_packed`'s.  A method of its own:
        `forward_packed` keeps its parameter list.  Errors are raised before any work."""
        who = "QuantLlamaAttentionFused"
        from .ops import ATTN_SPLIT_MIN_KEYS

        split_seqlen_q = int(split_seqlen_q)
        split_min_keys = ATTN_SPLIT_MIN_KEYS if split_min_keys is None else int(split_min_keys)
        if split_seqlen_q < 0 or split_seqlen_q * self.num_key_value_groups > 128:
            raise ValueError(f"{who}: split_seqlen_q {split_seqlen_q} must lie in 0 .. {128 // self.num_key_value_groups} "
                             "(split_seqlen_q * (H / Hkv) <= 128)")
        if split_min_keys < 1:
            raise ValueError(f"{who}: split_min_keys {split_min_keys} must be at least 1")
        return self._forward_packed(x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, decode_max_seqlen, block_table, page_size,
                                    (split_seqlen_q, split_min_keys))

    def _forward_packed(self, x, start_pos, freqs, cu_seqlens_q, max_seqlen_q, decode_max_seqlen, block_table, page_size, split):
        """The packed step; split = (split_seqlen_q, split_min_keys) routes its attention to the mixed entries.  With `sliding_window` the
        windowed mixed entries serve every call; no split is then split_seqlen_q = 0.  With `attn_softcap` their *_softcap siblings do, a
        layer without `sliding_window` under window_left = bound - 1, which hides nothing."""
        if self.sliding_window is not None:
            self._check_window(start_pos)
        if self.attn_softcap is not None:
            self._check_window(start_pos, what="attn_softcap")
        self._check_packed(x, start_pos, cu_seqlens_q, max_seqlen_q)
        if block_table is not None or page_size is not None:
            self._check_paged(start_pos, block_table, page_size)
        eng = load_engine()
        max_seqlen_q = int(max_seqlen_q)
        total = x.shape[1]
        bound = self.kv_max_seq_len if decode_max_seqlen is None else int(decode_max_seqlen)
        xqkv = self.qkv_proj(x).reshape(total, -1)
        scale = self.softmax_scale
        fp8 = self.kv_dtype == "fp8"
        names = ("cache_k", "cache_v") + (("cache_k_scale", "cache_v_scale") if fp8 else ())
        if fp8:
            if self.cache_k.device != xqkv.device:
                for name in names:
                    setattr(self, name, getattr(self, name).to(xqkv.device))
        elif self.cache_k.dtype != xqkv.dtype or self.cache_k.device != xqkv.device:
            self.cache_k = self.cache_k.to(xqkv)
            self.cache_v = self.cache_v.to(xqkv)
        kv = tuple(getattr(self, name) for name in names)
        table = ()
        if block_table is not None:
            ps = int(page_size)
            pool = (-1, ps, self.num_key_value_heads, self.head_dim)
            if decode_max_seqlen is None:
                bound = block_table.shape[1] * ps
            kv = tuple(t.view(pool if t.dim() == 4 else pool[:3]) for t in kv)
            table = (block_table,)
        where = ("paged" if table else "natural", "_paged" if table else "")
        attn = getattr(eng, "attn_prefill" + where[1] + "_varq" + ("_kv8" if fp8 else ""))
        xq = self._store(eng, "rope_kv_store_" + where[0] + "_varq" + ("_fp8" if fp8 else ""), xqkv, freqs, *kv, *table, cu_seqlens_q,
                         max_seqlen_q, start_pos, self.n_local_heads, self.num_key_value_heads)
        if self.attn_softcap is not None:
            from .ops import ATTN_SPLIT_MIN_KEYS

            ssq, smk = split if split is not None else (0, ATTN_SPLIT_MIN_KEYS)
            left = bound - 1 if self.sliding_window is None else self.sliding_window - 1
            attn = getattr(eng, "attn" + where[1] + "_varq_softcap" + ("_kv8" if fp8 else ""))
            output = attn(xq, *kv, *table, cu_seqlens_q, max_seqlen_q, start_pos, bound, ssq, smk, left, self.attn_softcap, True, scale, True)
        elif self.sliding_window is not None:
            from .ops import ATTN_SPLIT_MIN_KEYS

            ssq, smk = split if split is not None else (0, ATTN_SPLIT_MIN_KEYS)
            attn = getattr(eng, "attn" + where[1] + "_varq_window" + ("_kv8" if fp8 else ""))
            output = attn(xq, *kv, *table, cu_seqlens_q, max_seqlen_q, start_pos, bound, ssq, smk, self.sliding_window - 1, True, scale, True)
        elif split is not None:
            attn = getattr(eng, "attn" + where[1] + "_varq" + ("_kv8" if fp8 else ""))
            output = attn(xq, *kv, *table, cu_seqlens_q, max_seqlen_q, start_pos, bound, split[0], split[1], True, scale, True)
        else:
            output = attn(xq, *kv, *table, cu_seqlens_q, max_seqlen_q, start_pos, bound, True, scale, True)
        return self.o_proj(output.view(1, total, -1))

    @torch.no_grad()
    def forward_shared(self, x, start_pos, freqs, block_table, page_size, prefix_groups, decode_max_seqlen=None):
        """The paged `forward` (tensor `start_pos`, `block_table`, `page_size`) for a batch whose sequences share prefixes:
        `prefix_groups` is a `llm_awq_amd.paged_kv.PrefixGroups` over the slots of `start_pos`.  The store is `forward`'s -- new tokens land
        at positions >= the prefix, in a member's own pages -- and, while seqlen * (H / Hkv) * group_cap <= 128, the attention is
        attn_kvcache_paged_shared[_kv8] (csrc/awq_shared.hpp): the pages below a group's prefix are fetched once for the group.  A longer
        chunk, or `prefix_groups=None`, is `forward` itself, bit for bit.  (A method of its own: `forward` keeps its signature.)"""
        self._check_paged(start_pos, block_table, page_size)
        if self.sliding_window is not None:
            raise NotImplementedError("QuantLlamaAttentionFused: forward_shared is not implemented with sliding_window")
        if self.attn_softcap is not None:
            raise NotImplementedError("QuantLlamaAttentionFused: forward_shared is not implemented with attn_softcap")
        if prefix_groups is not None and prefix_groups.seq_prefix.shape[0] < x.shape[0]:
            raise ValueError(f"QuantLlamaAttentionFused: prefix_groups covers {prefix_groups.seq_prefix.shape[0]} slots, the batch has {x.shape[0]}")
        return self._forward_device_pos(load_engine(), x, start_pos, freqs, decode_max_seqlen, block_table, page_size, prefix_groups)

    def _forward_device_pos(self, eng, x, start_pos, freqs, decode_max_seqlen, block_table=None, page_size=None, prefix_groups=None):
        """rope_kv_store_natural_pos[_fp8] followed by attn_kvcache[_kv8] with seqlen_offset = seqlen: no length reaches the host.  With a
        block table: rope_kv_store_paged_pos[_fp8] followed by attn_kvcache_paged[_kv8] on the caches viewed as pages.  A chunk with
        seqlen * num_key_value_groups > 128 is beyond the split pair: attn_prefill_kvcache[_kv8] / attn_prefill_paged[_kv8] take its place
        with the same arguments (the one-pass prefill kernel under the same lengths)."""
        if self.kv_layout != "natural":
            raise ValueError("QuantLlamaAttentionFused: a tensor start_pos needs kv_layout 'natural' (the FT-layout path takes start_pos as "
                             "an int; its decode kernel reads per-sequence lengths through single_query_attention's length_per_sample)")
        bsz, seqlen, _ = x.shape
        bound = self.kv_max_seq_len if decode_max_seqlen is None else int(decode_max_seqlen)
        xqkv = self.qkv_proj(x).reshape(bsz, seqlen, -1)
        scale = self.softmax_scale
        prompt = seqlen * self.num_key_value_groups > 128  # more query rows per KV head than the split pair serves
        if self.kv_dtype == "fp8":
            if self.cache_k.device != xqkv.device:
                for name in ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale"):
                    setattr(self, name, getattr(self, name).to(xqkv.device))
        elif self.cache_k.dtype != xqkv.dtype or self.cache_k.device != xqkv.device:
            self.cache_k = self.cache_k.to(xqkv)
            self.cache_v = self.cache_v.to(xqkv)
        if block_table is not None:
            ps = int(page_size)
            pool = (-1, ps, self.num_key_value_heads, self.head_dim)
            if decode_max_seqlen is None:
                bound = block_table.shape[1] * ps
            shared = ()  # the group arrays and their bound, when the shared-prefix call serves
            if prefix_groups is not None and seqlen * self.num_key_value_groups * prefix_groups.group_cap <= 128:
                g = prefix_groups
                shared = (g.group_members, g.group_prefix, g.seq_prefix[:bsz], min(g.max_prefix, bound // 64 * 64))
            if self.kv_dtype == "fp8":
                pools = (self.cache_k.view(pool), self.cache_v.view(pool), self.cache_k_scale.view(pool[:3]), self.cache_v_scale.view(pool[:3]))
                xq = self._store(eng, "rope_kv_store_paged_pos_fp8", xqkv, freqs, *pools, block_table, start_pos, self.n_local_heads,
                                 self.num_key_value_heads)
                attn = eng.attn_prefill_paged_kv8 if prompt else eng.attn_kvcache_paged_shared_kv8 if shared else eng.attn_kvcache_paged_kv8
                output = attn(xq, *pools, block_table, start_pos, bound, *shared, seqlen, scale, True)
            else:
                pools = (self.cache_k.view(pool), self.cache_v.view(pool))
                xq = self._store(eng, "rope_kv_store_paged_pos", xqkv, freqs, *pools, block_table, start_pos, self.n_local_heads,
                                 self.num_key_value_heads)
                attn = eng.attn_prefill_paged if prompt else eng.attn_kvcache_paged_shared if shared else eng.attn_kvcache_paged
                output = attn(xq, *pools, block_table, start_pos, bound, *shared, seqlen, scale, True)
            return self.o_proj(output.view(bsz, seqlen, -1))
        if self.kv_dtype == "fp8":
            xq = self._store(eng, "rope_kv_store_natural_pos_fp8", xqkv, freqs, self.cache_k, self.cache_v, self.cache_k_scale,
                             self.cache_v_scale, start_pos, self.n_local_heads, self.num_key_value_heads)
            attn = eng.attn_prefill_kvcache_kv8 if prompt else eng.attn_kvcache_kv8
            output = attn(xq, self.cache_k, self.cache_v, self.cache_k_scale, self.cache_v_scale, start_pos, bound, seqlen, scale, True)
        else:
            xq = self._store(eng, "rope_kv_store_natural_pos", xqkv, freqs, self.cache_k, self.cache_v, start_pos, self.n_local_heads,
                             self.num_key_value_heads)
            attn = eng.attn_prefill_kvcache if prompt else eng.attn_kvcache
            output = attn(xq, self.cache_k, self.cache_v, start_pos, bound, seqlen, scale, True)
        return self.o_proj(output.view(bsz, seqlen, -1))


QuantLlamaAttentionFusedFlash = QuantLlamaAttentionFused


def fuse_qkv(q_proj, k_proj, v_proj):
    """The three projections' v2 buffers concatenated as the reference does (fused_attn.py:566-594: qweight on dim 0, scales and
    scaled_zeros on dim 1, bias on dim 0) into one WQLinear."""
    from .qmodule import WQLinear

    for name, p in (("q_proj", q_proj), ("k_proj", k_proj), ("v_proj", v_proj)):
        if getattr(p, "layout", "v2") != "v2":
            raise RuntimeError(f"make_quant_attn: {name} is in the {p.layout} layout; the projections are stacked as v2 (reference layout) "
                               "buffers -- call to_v2() on it first (or awq_inference_engine.cdna4_restore(qweight) for a qweight the "
                               "engine cache converted in place)")
        if hasattr(p, "engine_converted") and p.engine_converted():
            raise RuntimeError(f"make_quant_attn: the qweight of {name} was converted in place by the engine cache (AWQ_CDNA4_INPLACE); "
                               "call awq_inference_engine.cdna4_restore(qweight) first")
    if not (q_proj.w_bit == k_proj.w_bit == v_proj.w_bit == 4) or not (q_proj.group_size == k_proj.group_size == v_proj.group_size) or \
            not (q_proj.in_features == k_proj.in_features == v_proj.in_features):
        raise ValueError("make_quant_attn: q_proj, k_proj and v_proj must be 4-bit projections of one input width and group size")
    if (q_proj.bias is None) != (k_proj.bias is None) or (q_proj.bias is None) != (v_proj.bias is None):
        raise ValueError("make_quant_attn: q_proj, k_proj and v_proj must all carry a bias or none")
    qkv = WQLinear(q_proj.w_bit, q_proj.group_size, q_proj.in_features, q_proj.out_features + k_proj.out_features + v_proj.out_features,
                   q_proj.bias is not None, q_proj.qweight.device, dtype=q_proj.scales.dtype)
    qkv.qweight = torch.cat([q_proj.qweight, k_proj.qweight, v_proj.qweight], dim=0)
    qkv.scales = torch.cat([q_proj.scales, k_proj.scales, v_proj.scales], dim=1).contiguous()
    qkv.scaled_zeros = torch.cat([q_proj.scaled_zeros, k_proj.scaled_zeros, v_proj.scaled_zeros], dim=1).contiguous()
    if q_proj.bias is not None:
        qkv.bias = torch.cat([q_proj.bias, k_proj.bias, v_proj.bias], dim=0)
    qkv.split_k_iters = q_proj.split_k_iters
    return qkv


def make_quant_attn(model, dev, max_batch_size=1, kv_layout="ft", kv_dtype=None):
    """tinychat/modules/fused_attn.py:549-634: replace every module that carries q_proj, k_proj, v_proj, o_proj, `args` and
    `kv_max_seq_len` (the reference's LlamaAttentionFused / Qwen2AttentionFused) by a QuantLlamaAttentionFused over one fused
    qkv WQLinear, then move the model to `dev`.  `kv_layout="natural"` builds the long-context mode, `kv_dtype="fp8"` its FP8 cache.
    `make_quant_attn_window` is the same with a sliding window.  A module that carries `q_norm` or `k_norm` (Qwen3, Gemma-3) is refused:
    `make_quant_attn_qknorm` builds those."""
    return _make_quant_attn(model, dev, max_batch_size, kv_layout, kv_dtype, None)


def make_quant_attn_window(model, dev, sliding_window, max_batch_size=1, kv_layout="natural", kv_dtype=None):
    """`make_quant_attn` for a model with a sliding window (Mistral-7B-v0.1, Gemma-2/3 local layers, Qwen2 with `use_sliding_window`): every
    module is built with `sliding_window=W`, a window of W keys per row, the row's own included.  W is passed through; the model's config is
    not read for it.  A function of its own: `make_quant_attn` keeps its parameter list."""
    if sliding_window is None:
        raise ValueError("make_quant_attn_window: sliding_window must be an int >= 1 (`make_quant_attn` builds the modules without a window)")
    return _make_quant_attn(model, dev, max_batch_size, kv_layout, kv_dtype, sliding_window)


def make_quant_attn_qknorm(model, dev, max_batch_size=1, kv_layout="natural", kv_dtype=None, sliding_window=None, norm_offset=0.0):
    """`make_quant_attn` for a model whose attention blocks put a per-head RMSNorm on q and k between the projection and RoPE (Qwen3, dense
    and MoE; Gemma-3): a module's `q_norm` / `k_norm` submodules supply the weights (`.weight`, [head_dim]) and the eps (`variance_epsilon`
    or `eps`), and every module is built with `qk_norm=(norm_offset + q_norm.weight.float(), norm_offset + k_norm.weight.float(), eps)`.
    `norm_offset=1.0` is Gemma-3's (1 + w), formed in float32; `sliding_window` as in `make_quant_attn_window` (None: full attention).  A
    module without both norms is refused.  A function of its own: `make_quant_attn` keeps its parameter list."""
    return _make_quant_attn(model, dev, max_batch_size, kv_layout, kv_dtype, sliding_window, norm_offset=float(norm_offset))


def make_quant_attn_softcap(model, dev, attn_softcap, softmax_scale=None, sliding_window=None, max_batch_size=1, kv_layout="natural",
                            kv_dtype=None):
    """`make_quant_attn` for a model that soft-caps its attention logits (Gemma-2: attn_softcap 50 with softmax_scale 144 ** -0.5 on the
    27B; Grok-1: 30): every module is built with `attn_softcap` and `softmax_scale` (None: head_dim ** -0.5).  `sliding_window` is None
    (every layer global), an int (every layer), or a sequence with one entry per replaced module in the order they are met, a None entry a
    global layer -- Gemma-2 alternates, `[4096, None] * 23`.  Values are passed through; the model's config is not read.  A function of its
    own: `make_quant_attn` keeps its parameter list."""
    if attn_softcap is None:
        raise ValueError("make_quant_attn_softcap: attn_softcap must be a finite float > 0 (`make_quant_attn` builds the modules without a cap)")
    per_layer = None
    if sliding_window is not None and not isinstance(sliding_window, int):
        per_layer = list(sliding_window)
        sliding_window = None
    return _make_quant_attn(model, dev, max_batch_size, kv_layout, kv_dtype, sliding_window, per_layer_window=per_layer,
                            extra={"attn_softcap": attn_softcap, "softmax_scale": softmax_scale})


def _norm_eps(norm, name):
    for attr in ("variance_epsilon", "eps"):
        if getattr(norm, attr, None) is not None:
            return float(getattr(norm, attr))
    raise ValueError(f"make_quant_attn_qknorm: {name} carries neither variance_epsilon nor eps")


def _make_quant_attn(model, dev, max_batch_size, kv_layout, kv_dtype, sliding_window, norm_offset=None, per_layer_window=None, extra=None):
    """per_layer_window: one `sliding_window` per replaced module, in the order they are met (None: `sliding_window` for all); extra:
    further keywords of every module (`make_quant_attn_softcap`)."""
    want = ("q_proj", "k_proj", "v_proj", "o_proj", "args", "kv_max_seq_len")
    todo = [(name, m) for name, m in model.named_modules()
            if not (name == "" or isinstance(m, QuantLlamaAttentionFused) or not all(hasattr(m, a) for a in want))]
    if per_layer_window is not None and len(per_layer_window) != len(todo):
        raise ValueError(f"make_quant_attn_softcap: sliding_window has {len(per_layer_window)} entries for {len(todo)} attention modules")
    for index, (name, m) in enumerate(todo):
        if per_layer_window is not None:
            sliding_window = per_layer_window[index]
        has_norm = [hasattr(m, a) and getattr(m, a) is not None for a in ("q_norm", "k_norm")]
        qk_norm = None
        if norm_offset is None:
            if any(has_norm):  # dropping the norm silently gives wrong logits
                raise ValueError(f"make_quant_attn: module {name!r} carries a per-head q_norm / k_norm (Qwen3, Gemma-3); build it with "
                                 "make_quant_attn_qknorm, which fuses the norm into the rope + KV-store launch")
        else:
            if not all(has_norm):
                raise ValueError(f"make_quant_attn_qknorm: module {name!r} must carry both q_norm and k_norm (`make_quant_attn` builds the "
                                 "modules without a norm)")
            eps_q, eps_k = _norm_eps(m.q_norm, name + ".q_norm"), _norm_eps(m.k_norm, name + ".k_norm")
            if eps_q != eps_k:
                raise ValueError(f"make_quant_attn_qknorm: q_norm and k_norm of module {name!r} have different eps ({eps_q}, {eps_k})")
            qk_norm = (norm_offset + m.q_norm.weight.detach().float(), norm_offset + m.k_norm.weight.detach().float(), eps_q)
        qkv = fuse_qkv(m.q_proj, m.k_proj, m.v_proj)
        attn = QuantLlamaAttentionFused(m.args.hidden_size, m.args.num_attention_heads, m.kv_max_seq_len, qkv, m.o_proj, dev, m.args,
                                        max_batch_size=max_batch_size, kv_layout=kv_layout, kv_dtype=kv_dtype,
                                        sliding_window=sliding_window, **({} if qk_norm is None else {"qk_norm": qk_norm}), **(extra or {}))
        if "." in name:
            parent_name, child_name = name.rsplit(".", 1)
            parent = model.get_submodule(parent_name)
        else:
            parent, child_name = model, name
        setattr(parent, child_name, attn)
    return model.to(dev)
