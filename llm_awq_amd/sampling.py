"""Next-token sampling on the device: the per-row state around `ops.sample_logits`.

The reference chooses a token on the host (tinychat/stream_generators/stream_gen.py:19-32,120-134): four HF logits processors, a softmax, a
multinomial and an `int()` per token.  `DeviceSampler` owns the same parameters as per-row GPU tensors -- one slot per sequence of a ragged batch,
each with its own temperature / top-p / top-k / repetition penalty and its own token history -- and a call is one launch that reads them on the
device, writes the token into the history and moves the sequence length on (-1 = finished, the convention of `cache_seqlens`).  Nothing is read
back, so the call sits inside the captured decode graph.
"""
from __future__ import annotations

import torch

from . import ops


class DeviceSampler:
    """stop_ids: token ids that finish a slot (`finished[b]` = 1, its seqlen -1); max_len: the cache length at which a slot finishes (default: none)."""

    def __init__(self, batch: int, vocab: int, device, max_history: int = 0, seed=None, stop_ids=(), max_len: int = 2 ** 31 - 1):
        self.batch, self.vocab, self.device = int(batch), int(vocab), torch.device(device)
        self.max_history, self.max_len = int(max_history), int(max_len)
        f = dict(dtype=torch.float32, device=self.device)
        i = dict(dtype=torch.int32, device=self.device)
        self.temperature = torch.ones(self.batch, **f)
        self.top_p = torch.ones(self.batch, **f)
        self.top_k = torch.full((self.batch,), self.vocab, **i)
        self.repetition_penalty = torch.ones(self.batch, **f)
        self.history = torch.zeros(self.batch, self.max_history, **i) if self.max_history > 0 else None
        self.hist_len = torch.zeros(self.batch, **i) if self.max_history > 0 else None
        self.finished = torch.zeros(self.batch, **i)
        self.stop_ids = torch.tensor(list(stop_ids), **i) if len(stop_ids) else None
        self.generator = torch.Generator(device=self.device)
        if seed is not None:
            self.generator.manual_seed(int(seed))

    def set_row(self, b: int, temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0, prompt_ids=()):
        """Fill slot b with the reference's thresholds (stream_gen.py:24-31,59-62,129): a temperature below 1e-5 or a top-p below 1e-8 is greedy,
        top_k <= 0 is the whole vocabulary, a penalty of at most 1 is off.  prompt_ids start the slot's history (the last max_history of them)."""
        self.temperature[b] = float(temperature)
        self.top_p[b] = float(top_p)
        self.top_k[b] = self.vocab if int(top_k) <= 0 else min(int(top_k), self.vocab)
        self.repetition_penalty[b] = float(repetition_penalty) if repetition_penalty > 1.0 else 1.0
        self.finished[b] = 0
        if self.history is not None:
            ids = list(prompt_ids)[-self.max_history:]
            self.hist_len[b] = len(ids)
            if ids:
                self.history[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32, device=self.device)

    @classmethod
    def from_gen_params(cls, gen_params, device="cuda", prompt_ids=(), max_history: int = 0, seed=None, stop_ids=(), max_len: int = 2 ** 31 - 1):
        """The single-sequence loop's sampler from the reference's gen_params (n_vocab, temp, top_p, top_k, repeat_penalty, n_predict); its history
        holds the prompt and the generated tokens, so the loop reads new text from `history` when it streams, not a token per step."""
        need = max_history or max(len(prompt_ids) + int(getattr(gen_params, "n_predict", 0)), 1)  # the prompt and every token to come
        s = cls(1, gen_params.n_vocab, device, max_history=need, seed=seed, stop_ids=stop_ids, max_len=max_len)
        s.set_row(0, gen_params.temp, gen_params.top_p, gen_params.top_k, gen_params.repeat_penalty, prompt_ids)
        return s

    def __call__(self, logits, seqlens=None, u=None):
        """logits [B, V] (or [B, 1, V]) -> tokens int32 [B].  With seqlens (int32 [B], -1 = inactive) the launch also advances them; the token is
        appended to the slot's history when there is one.  u: the uniforms in [0, 1) to use; drawn from the sampler's own generator otherwise."""
        if logits.dim() == 3:
            logits = logits[:, -1, :]
        logits = logits.contiguous()
        if u is None:
            u = torch.rand(self.batch, dtype=torch.float32, device=self.device, generator=self.generator)
        return ops.sample_logits(logits, u, temperature=self.temperature, top_k=self.top_k, top_p=self.top_p,
                                 repetition_penalty=self.repetition_penalty if self.history is not None else None, history=self.history,
                                 hist_len=self.hist_len, seqlens=seqlens, stop_ids=self.stop_ids, finished=self.finished, max_len=self.max_len,
                                 append=self.history is not None, advance=seqlens is not None)
