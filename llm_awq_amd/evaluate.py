"""Scoring text with the model's own log-probabilities: perplexity and lm-eval's loglikelihood pair.

The reference accepts a quantised model by its WikiText-2 perplexity (awq/entry.py:301-333) and by lm-eval log-likelihood tasks (:334-346).  Its loop
materialises a [seqlen, vocab] logits tensor, copies the shifted part as fp32 and runs CrossEntropyLoss over it; here the head's `logprobs`
(`LMHead.logprobs` -> ops.lm_head_logprobs) gives the per-token log-probabilities without a logit ever reaching memory, and this module restates
the arithmetic around it:

  perplexity   windows of `seqlen` tokens, the remainder dropped; per window the MEAN of the seqlen - 1 shifted NLLs times seqlen; the windows' values
               summed, divided by nsamples * seqlen, exponentiated -- entry.py:304-326 literally, (seqlen - 1 terms scaled by seqlen included).
  loglikelihood   lm-eval's (sum of the continuation's log-probs, "every continuation token was the greedy one").

`hidden_fn(batch)` maps token ids [1, S] to hidden states [1, S, K] (or [S, K]) IN FRONT OF the head's norm -- or behind it, when `head` has none.
`head` is anything with LMHead's `logprobs(h, targets, round_logits=..., want=...)`.  With round_logits=True (the default here) every logit is
rounded to the model's dtype before the log-sum-exp, as the nn.Linear of the reference's loop stores it, so its number is reproduced.
"""
from __future__ import annotations

import torch


def _ids_1d(ids):
    ids = torch.as_tensor(ids)
    if ids.dim() == 2 and ids.shape[0] == 1:
        ids = ids[0]
    if ids.dim() != 1:
        raise ValueError("evaluate: token ids must be [N] or [1, N]")
    return ids


def _hidden(hidden_fn, batch):
    h = hidden_fn(batch[None, :])
    return h.reshape(-1, h.shape[-1])


def _cap_kw(final_softcap):
    """`final_softcap` for head.logprobs, handed over only when one is given: a head without the keyword is called as before."""
    return {} if final_softcap is None else {"final_softcap": final_softcap}


def perplexity(hidden_fn, head, input_ids, seqlen: int = 2048, round_logits: bool = True, final_softcap=None) -> float:
    """entry.py:304-326 over the head's log-probabilities.  The windows' NLLs are added on the device in fp32, in window order; one host read at the end.
    `final_softcap` (None: the head's own, if any) caps the logits as c * tanh(z / c) before the log-sum-exp (Gemma-2: 30)."""
    ids = _ids_1d(input_ids)
    nsamples = ids.numel() // seqlen
    if seqlen < 2 or nsamples < 1:
        raise ValueError(f"perplexity: {ids.numel()} tokens hold no window of seqlen {seqlen}")
    total = None
    for i in range(nsamples):
        batch = ids[i * seqlen:(i + 1) * seqlen]
        with torch.no_grad():
            h = _hidden(hidden_fn, batch)
            lp = head.logprobs(h[:-1], batch[1:].to(device=h.device, dtype=torch.int32), round_logits=round_logits, **_cap_kw(final_softcap))["logprob"]
            nll = (-(lp.float().sum()) / (seqlen - 1)).float() * seqlen   # CrossEntropyLoss's mean, then `loss.float() * model.seqlen`
        total = nll if total is None else total + nll
    return float(torch.exp(total / (nsamples * seqlen)).item())


def loglikelihood(hidden_fn, head, context_ids, continuation_ids, round_logits: bool = True, final_softcap=None):
    """lm-eval's pair for one request: (sum of log p(continuation token | everything before it), whether each of them was the argmax).
    `final_softcap` as in `perplexity`."""
    ctx, cont = _ids_1d(context_ids), _ids_1d(continuation_ids)
    if ctx.numel() < 1 or cont.numel() < 1:
        raise ValueError("loglikelihood: context and continuation must hold at least one token each")
    inp = torch.cat([ctx, cont.to(ctx.device)])[:-1]
    with torch.no_grad():
        h = _hidden(hidden_fn, inp)[-cont.numel():]
        tg = cont.to(device=h.device, dtype=torch.int32)
        res = head.logprobs(h, tg, round_logits=round_logits, want=("logprob", "argmax"), **_cap_kw(final_softcap))
        both = torch.stack([res["logprob"].double().sum(), (res["argmax"] == tg).all().double()]).cpu()   # one host read
    return float(both[0]), bool(both[1] != 0)


def perplexity_hf(model, input_ids, seqlen: int = 2048, round_logits: bool = True, final_softcap=None) -> float:
    """`perplexity` for a Hugging Face style causal LM: `model.model(ids)[0]` are the hidden states behind the final norm, `model.lm_head` the head.
    `final_softcap` is the model's final_logit_softcapping (Gemma-2: 30); it is passed through, the config is not read."""
    from .lm_head import LMHead
    head = LMHead.from_modules(None, model.lm_head, final_softcap=final_softcap)
    return perplexity(lambda b: model.model(b.to(head.weight.device))[0], head, input_ids, seqlen, round_logits)
