"""The two ends of a decode step: token embedding in front of the blocks, final RMSNorm + LM head behind them.

The reference ends `Transformer.forward` with `self.norm(h)` and an unquantised `nn.Linear(hidden, vocab)` (tinychat/models/llama.py:395,412) and
starts it with `nn.Embedding`, which cannot take the -1 a finished slot holds after `ops.sample_logits`.  `LMHead` runs the norm and the
vocabulary product as one launch that reads the weight matrix once for up to 64 rows, skips inactive rows (seqlens -1) and writes fp32 logits, which
is what `DeviceSampler` reads; `TokenEmbedding` gathers rows and gives zeros for any id outside the table.  A serving loop is then
embed -> blocks -> LM head -> sample with no host read and no torch arithmetic between the stages, so it can be captured as one graph.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops


class LMHead(nn.Module):
    """weight [V, K] (nn.Linear.weight as loaded), norm_weight [K] or None (no norm), bias [V] or None.  The tensors are held by reference.
    `final_softcap=c` (None: no cap, nothing changes; Gemma-2: 30) caps every logit as c * tanh(z / c), in the epilogue of the same launches:
    `forward` is then ops.lm_head_softcap and `logprobs` ops.lm_head_logprobs with softcap=c."""

    def __init__(self, weight, norm_weight=None, eps: float = 1e-6, bias=None, out_dtype=torch.float32, final_softcap=None):
        super().__init__()
        self.weight, self.norm_weight, self.bias = weight, norm_weight, bias
        self.eps, self.out_dtype = float(eps), out_dtype
        if final_softcap is not None and not (0.0 < float(final_softcap) < float("inf")):
            raise ValueError(f"LMHead: final_softcap {final_softcap!r} must be None or a finite float > 0")
        self.final_softcap = None if final_softcap is None else float(final_softcap)

    @classmethod
    def from_modules(cls, norm, linear, out_dtype=torch.float32, final_softcap=None):
        """norm: the model's final RMSNorm (`weight`, and `variance_epsilon` or `eps`) or None; linear: its `lm_head`.  No weight is copied."""
        eps = 0.0 if norm is None else float(getattr(norm, "variance_epsilon", getattr(norm, "eps", 1e-6)))
        return cls(linear.weight, None if norm is None else norm.weight, eps, getattr(linear, "bias", None), out_dtype, final_softcap=final_softcap)

    def forward(self, h, seqlens=None, out=None):
        """h [B, K] or [B, S, K] (the last token is used, as a strided view) -> logits [B, V]; rows with seqlens[b] < 0 are left as they are in `out`
        (zeros in a fresh one)."""
        if h.dim() == 3:
            h = h[:, -1, :]
        if self.final_softcap is not None:
            return ops.lm_head_softcap(h, self.weight, self.final_softcap, self.norm_weight, self.eps, self.bias, seqlens, out, self.out_dtype)
        return ops.lm_head(h, self.weight, self.norm_weight, self.eps, self.bias, seqlens, out, self.out_dtype)

    def logprobs(self, h, targets, round_logits=False, want=("logprob", "lse"), ws=None, out=None, final_softcap=None):
        """h [T, K] or [B, S, K] -- EVERY position is used, not forward's last token -- and targets int32 of T (B * S) values -> a dict of fp32 [T]
        tensors (argmax int32), see ops.lm_head_logprobs.  No logit is written to memory.  A position whose target is outside [0, V) is ignored.
        `final_softcap` (None: the head's own) caps the logits for this call."""
        h2 = h.reshape(-1, h.shape[-1])
        tg = None if targets is None else targets.reshape(-1)
        cap = self.final_softcap if final_softcap is None else float(final_softcap)
        if cap is None:
            return ops.lm_head_logprobs(h2, self.weight, tg, self.norm_weight, self.eps, self.bias, round_logits, ws, want, out)
        return ops.lm_head_logprobs(h2, self.weight, tg, self.norm_weight, self.eps, self.bias, round_logits, ws, want, out, softcap=cap)


class TokenEmbedding(nn.Module):
    """`nn.Embedding.forward` for int32 ids on the device, with zeros for -1 (a finished slot) and every other id outside the table."""

    def __init__(self, table):
        super().__init__()
        self.weight = table

    @classmethod
    def from_module(cls, embedding):
        return cls(embedding.weight)

    def forward(self, tokens):
        return ops.embed_tokens(tokens, self.weight)
