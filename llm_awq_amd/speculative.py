"""Prompt-lookup speculative decoding on the device: the per-step state around `ops.spec_draft_ngram` / `spec_pack` / `spec_verify` / `spec_accept`.

A decode step reads every weight for one token per sequence; rows 2 .. 8 of the same pass cost almost nothing more.  `PromptLookupSampler` turns
that into tokens without a draft model: the continuation of the last place where the sequence's own history held its latest n-gram is the draft,
the packed step (`QuantLlamaAttentionFused.forward_packed_split`) scores the draft's positions in one pass, and the sampler's own row routine decides
how many of them stand.  The draft is deterministic, so "sample row j exactly as `sample_logits` would, accept draft j + 1 iff it equals that sample"
is the speculative-sampling rule for a one-hot proposal: the emitted tokens are, bit for bit, those of the token-by-token loop given the same logits
and the same uniform per position (DESIGN.md "Speculative decoding").  Nothing is read back, so the whole step sits in one captured graph:

    ids, cu = spec.begin_step()                       # draft + pack           (persistent tensors)
    h = embedding(ids) ... blocks: forward_packed_split(h, seqlens, freqs, cu, spec.max_seqlen_q, split_seqlen_q=spec.max_seqlen_q) ...
    logits = lm_head(h)                               # every row: [total_q, V]
    out_tokens, num_emitted = spec.end_step(logits)   # verify + accept        (persistent tensors)
"""
from __future__ import annotations

import torch

from . import ops
from .sampling import DeviceSampler

LM_HEAD_MAX_ROWS = 64  # awq_lm_head takes at most this many rows per launch


class PromptLookupSampler:
    """sampler: the `DeviceSampler` whose parameters, history, finish flags, stop ids, max_len and generator are used (it must have a history:
    the drafter reads it and the accept step appends to it).  seqlens: the int32 [B] cache lengths of the slots (-1 = inactive), the tensor the
    attention layers take as start_pos; `end_step` advances it.  kmax (0 .. 15): the longest draft; ngram_min / ngram_max (1 .. 8): the lengths of
    the n-gram looked up; total_q >= B: the token budget of a step, the fixed row count of its packed tensors (default B * (kmax + 1): every
    slot may bring a full draft; a smaller budget is granted in slot order).

    `ops.lm_head` takes at most 64 rows per call: a budget above that is refused here unless `allow_chunked_lm_head=True`, which states that
    the caller computes the logits in chunks of at most 64 rows (`lm_head_chunks()` gives the row ranges).

    Cache bookkeeping: the step stores the K / V of every input row, accepted or not, at seqlens[b] .. seqlens[b] + n_b - 1.  The accepted ones lie
    below the advanced seqlens[b]; the rows of rejected drafts lie beyond it and the next step's store overwrites them, so neither a dense nor a
    paged cache is rolled back.  A `PageTable` user must therefore hold pages for seqlens[b] + kmax + 1 tokens of every active slot BEFORE
    the step (`table.reserve(slot, seqlen + kmax + 1)`), not only for seqlens[b] + 1; the drafter never drafts past `sampler.max_len`.

    `last_tokens` (int32 [B]) is the input of every slot's first row: set it (`set_last_tokens`) to what `DeviceSampler.__call__` returned after
    the prompt; `end_step` keeps it current."""

    def __init__(self, sampler: DeviceSampler, seqlens, kmax: int = 4, ngram_min: int = 1, ngram_max: int = 3, total_q=None,
                 allow_chunked_lm_head: bool = False):
        if sampler.history is None:
            raise ValueError("PromptLookupSampler: the DeviceSampler needs a history (max_history > 0): it is what the drafter looks up")
        self.sampler, self.seqlens = sampler, seqlens
        self.batch, self.kmax, self.ngram_min, self.ngram_max = sampler.batch, int(kmax), int(ngram_min), int(ngram_max)
        if not 0 <= self.kmax <= 15:
            raise ValueError(f"PromptLookupSampler: kmax {self.kmax} must lie in 0 .. 15")
        if not 1 <= self.ngram_min <= self.ngram_max <= 8:
            raise ValueError("PromptLookupSampler: 1 <= ngram_min <= ngram_max <= 8")
        self.total_q = self.batch * (self.kmax + 1) if total_q is None else int(total_q)
        if self.total_q < self.batch:
            raise ValueError(f"PromptLookupSampler: total_q {self.total_q} must be at least the batch {self.batch} (every active slot gets its row)")
        if self.total_q > LM_HEAD_MAX_ROWS and not allow_chunked_lm_head:
            raise ValueError(f"PromptLookupSampler: total_q {self.total_q} is above the {LM_HEAD_MAX_ROWS} rows one ops.lm_head call takes; pass "
                             "allow_chunked_lm_head=True and compute the logits over lm_head_chunks()")
        if seqlens.dtype != torch.int32 or seqlens.numel() != self.batch or seqlens.device != sampler.history.device:
            raise ValueError("PromptLookupSampler: seqlens must be int32 [B] on the sampler's device")
        self.max_seqlen_q = self.kmax + 1  # forward_packed_split(..., max_seqlen_q=, split_seqlen_q=)
        i = dict(dtype=torch.int32, device=sampler.history.device)
        self.max_draft = torch.full((self.batch,), self.kmax, **i)  # per-slot cap of the draft (0 = plain decode for the slot)
        self.drafts = torch.full((self.batch, self.kmax), -1, **i)
        self.draft_len = torch.zeros(self.batch, **i)
        self.cu_seqlens_q = torch.zeros(self.batch + 1, **i)
        self.input_ids = torch.full((self.total_q,), -1, **i)
        self.row_tokens = torch.full((self.total_q,), -1, **i)
        self.out_tokens = torch.full((self.batch, self.kmax + 1), -1, **i)
        self.num_emitted = torch.zeros(self.batch, **i)
        self.last_tokens = torch.full((self.batch,), -1, **i)

    def set_last_tokens(self, tokens):
        """tokens int32 [B]: the token every slot feeds next (what sampling the prompt's last row returned); copied in place."""
        self.last_tokens.copy_(tokens.reshape(-1))

    def lm_head_chunks(self):
        """The row ranges [(r0, r1), ...] of at most 64 rows in which the step's logits are computed."""
        return [(r, min(r + LM_HEAD_MAX_ROWS, self.total_q)) for r in range(0, self.total_q, LM_HEAD_MAX_ROWS)]

    def begin_step(self):
        """draft + pack -> (input_ids int32 [total_q], cu_seqlens_q int32 [B + 1]): the same two tensors every step."""
        s = self.sampler
        ops.spec_draft_ngram(s.history, s.hist_len, self.seqlens, vocab=s.vocab, kmax=self.kmax, ngram_min=self.ngram_min, ngram_max=self.ngram_max,
                             max_len=s.max_len, max_draft=self.max_draft, drafts=self.drafts, draft_len=self.draft_len)
        ops.spec_pack(self.last_tokens, self.drafts, self.draft_len, self.seqlens, self.total_q, cu_seqlens_q=self.cu_seqlens_q,
                      input_ids=self.input_ids)
        return self.input_ids, self.cu_seqlens_q

    def end_step(self, logits, u=None):
        """logits [total_q, V] of the step's rows (or [1, total_q, V]) -> (out_tokens int32 [B, kmax + 1], -1 behind the emitted ones; num_emitted
        int32 [B]): the same two tensors every step.  Histories, finish flags and seqlens move on as after num_emitted sample_logits calls.
        u: fp32 [total_q], one uniform per row; drawn from the sampler's generator otherwise."""
        s = self.sampler
        if logits.dim() == 3:
            logits = logits.reshape(-1, logits.shape[-1])
        logits = logits.contiguous()
        if u is None:
            u = torch.rand(self.total_q, dtype=torch.float32, device=s.device, generator=s.generator)
        ops.spec_verify(logits, u, self.cu_seqlens_q, self.input_ids, temperature=s.temperature, top_k=s.top_k, top_p=s.top_p,
                        repetition_penalty=s.repetition_penalty, history=s.history, hist_len=s.hist_len, row_tokens=self.row_tokens)
        ops.spec_accept(self.row_tokens, self.input_ids, self.cu_seqlens_q, self.kmax, history=s.history, hist_len=s.hist_len, seqlens=self.seqlens,
                        stop_ids=s.stop_ids, finished=s.finished, max_len=s.max_len, append=True, advance=True, out_tokens=self.out_tokens,
                        num_emitted=self.num_emitted, last_tokens=self.last_tokens)
        return self.out_tokens, self.num_emitted
