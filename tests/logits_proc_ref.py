"""A torch fp32 restatement (CPU) of generate()'s logits processors, the semantics the kernel is held to: transformers'
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor and MinLength /
MinNewTokensLengthLogitsProcessor, in that order, where a row's history is the ids generated so far (never the prompt: the
reference generates from inputs_embeds, so transformers starts input_ids empty).

Computed on the CPU on purpose: torch on the GPU divides by a scalar through its reciprocal, the CPU (and transformers' fixtures,
made on the CPU) divides."""
from __future__ import annotations

from typing import Optional, Sequence

import torch


def process(scores: torch.Tensor, hist, eos: Sequence[int] = (), penalty: Optional[float] = None, ngram: int = 0,
            bad: Optional[Sequence[Sequence[int]]] = None, min_new: int = 0) -> torch.Tensor:
    """scores fp32 [B, V] -> processed copy (CPU).  hist: per-row lists of generated ids (or an int tensor [B, t])."""
    s = scores.detach().float().cpu().clone()
    B, V = s.shape
    rows = [[int(x) for x in h] for h in (hist.tolist() if torch.is_tensor(hist) else hist)]
    assert len(rows) == B
    eos = [int(e) for e in eos]
    words = [list(map(int, w)) for w in (bad or []) if not (len(w) == 1 and int(w[0]) in eos)]   # transformers drops [eos]
    for b, h in enumerate(rows):
        t = len(h)
        if penalty is not None and penalty != 1.0 and t:
            ids = torch.tensor(sorted(set(i for i in h if 0 <= i < V)), dtype=torch.long)
            if len(ids):
                v = s[b, ids]
                s[b, ids] = torch.where(v < 0, v * penalty, v / penalty)
        ban = set()
        if ngram and t + 1 >= ngram:
            tail = h[t - ngram + 1:]
            for i in range(t - ngram + 1):
                if h[i:i + ngram - 1] == tail:
                    ban.add(h[i + ngram - 1])
        for w in words:
            if len(w) == 1 or (t >= len(w) and h[t - len(w) + 1:] == w[:-1]):
                ban.add(w[-1])
        if t < min_new:
            ban.update(eos)
        for i in ban:
            if 0 <= i < V:
                s[b, i] = float("-inf")
    return s


def hf_process(scores: torch.Tensor, hist: torch.Tensor, eos: Sequence[int] = (), penalty: Optional[float] = None,
               ngram: int = 0, bad=None, min_new: int = 0) -> torch.Tensor:
    """The same through the installed transformers' processor classes, as GenerationMixin._get_logits_processor builds them
    (input_ids = the history, prompt length 0)."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor,
                                                        NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    procs = LogitsProcessorList()
    if penalty is not None and penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(penalty)))
    if ngram:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    eos_t = torch.tensor(list(eos), dtype=torch.long) if len(eos) else None
    if bad is not None:
        procs.append(NoBadWordsLogitsProcessor([list(w) for w in bad], eos_t))
    if min_new and eos_t is not None:
        procs.append(MinNewTokensLengthLogitsProcessor(0, min_new, eos_t))
    return procs(hist.long(), scores.detach().float().cpu().clone())


def warp(scores: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """transformers' TemperatureLogitsWarper, TopKLogitsWarper and TopPLogitsWarper after the processors (CPU, fp32)."""
    from transformers.generation.logits_process import (LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    w = LogitsProcessorList([TemperatureLogitsWarper(temperature)])
    if top_k:
        w.append(TopKLogitsWarper(top_k))
    if top_p < 1.0:
        w.append(TopPLogitsWarper(top_p))
    return w(torch.zeros((scores.shape[0], 0), dtype=torch.long), scores.detach().float().cpu().clone())
