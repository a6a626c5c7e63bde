"""A torch fp32 restatement (CPU) of constrained decoding, the semantics the kernel is held to: transformers'
PrefixConstrainedLogitsProcessor(prefix_allowed_tokens_fn, num_beams=1) - per row, the callback is asked for the ids allowed
behind the ids generated so far (never the prompt: the reference generates from inputs_embeds, so transformers starts input_ids
empty), and every other score becomes -inf by ADDING a mask of 0 / -inf.  Also the brute-force definition of a TokenTrie's
callback (a scan over all members) that tests/test_constrained_host.py holds the callback to."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch


def mask(B: int, V: int, hist, fn) -> torch.Tensor:
    """fp32 [B, V]: 0 at the ids fn(b, hist[b]) allows, -inf elsewhere."""
    rows = hist.tolist() if torch.is_tensor(hist) else hist
    m = torch.full((B, V), -math.inf, dtype=torch.float32)
    for b in range(B):
        m[b, [int(i) for i in fn(b, torch.tensor(rows[b], dtype=torch.long))]] = 0
    return m


def process(scores: torch.Tensor, hist, fn) -> torch.Tensor:
    """scores fp32 [B, V] -> processed copy (CPU).  hist: per-row lists of generated ids (or an int tensor [B, t])."""
    s = scores.detach().float().cpu()
    return s + mask(s.shape[0], s.shape[1], hist, fn)


def hf_process(scores: torch.Tensor, hist: torch.Tensor, fn, penalty: Optional[float] = None, min_new: int = 0,
               eos: Sequence[int] = ()) -> torch.Tensor:
    """The same through the installed transformers, in GenerationMixin._get_logits_processor's order: repetition penalty,
    min_new_tokens, then the prefix constraint."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor,
                                                        PrefixConstrainedLogitsProcessor, RepetitionPenaltyLogitsProcessor)
    procs = LogitsProcessorList()
    if penalty is not None and penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(penalty)))
    if min_new and len(eos):
        procs.append(MinNewTokensLengthLogitsProcessor(0, min_new, torch.tensor(list(eos), dtype=torch.long)))
    procs.append(PrefixConstrainedLogitsProcessor(fn, 1))
    return procs(hist.long(), scores.detach().float().cpu().clone())


def brute_allowed(members, ends, sep, sent):
    """The definition by a scan over all members: every way `sent` parses as "member (sep member)*" with a last, possibly
    partial, member is followed at once; the allowed ids are whatever continues one of them.  No parse: the end ids."""
    members = [list(m) for m in members]
    ends = sorted(set(int(e) for e in ends))
    fresh = {("m", i, 0) for i in range(len(members))}
    confs = set(fresh)
    for t in [int(x) for x in sent]:
        nxt = set()
        for c in confs:
            if c[0] == "m":
                _, i, j = c
                if j < len(members[i]) and members[i][j] == t:
                    nxt.add(("m", i, j + 1))
                elif j == len(members[i]) and sep is not None and t == sep[0]:
                    nxt |= fresh if len(sep) == 1 else {("s", 1)}
            elif sep[c[1]] == t:
                nxt |= fresh if c[1] + 1 == len(sep) else {("s", c[1] + 1)}
        confs = nxt
        if not confs:
            return ends
    out = set()
    for c in confs:
        if c[0] == "s":
            out.add(sep[c[1]])
        elif c[2] < len(members[c[1]]):
            out.add(members[c[1]][c[2]])
        elif c[2] > 0:
            out.update(ends)
            if sep is not None:
                out.add(sep[0])
    return sorted(out)


def accepted(members, ends, sep, row, pad=None) -> bool:
    """row = "member (sep member)* end pad*" (without a separator: exactly one member)."""
    row = [int(t) for t in row]
    ends = set(int(e) for e in ends)
    k = next((i for i, t in enumerate(row) if t in ends), None)
    if k is None:
        return False
    if pad is not None and any(t != pad for t in row[k + 1:]):
        return False
    body, ms = row[:k], {tuple(m) for m in members}
    if sep is None:
        return tuple(body) in ms
    ok = [True] + [False] * len(body)          # ok[i]: body[:i] is "member sep member sep ... " ready for the next member
    done = False
    for i in range(len(body)):
        if not ok[i]:
            continue
        for m in ms:
            j = i + len(m)
            if tuple(body[i:j]) == m:
                if j == len(body):
                    done = True
                elif body[j:j + len(sep)] == list(sep):
                    ok[j + len(sep)] = True
    return done
