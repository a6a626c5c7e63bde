"""A torch restatement (CPU) of generate(guidance_scale=g), the semantics the device path is held to: transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor restated on PAIRED ROWS.  The P negative prompts run beside the P conditional
prompts through one `logits_fn`, both halves are given the token chosen for the conditional row, and per step
    s = g (log_softmax(c) - log_softmax(u)) + log_softmax(u)
is followed by the other processors (tests/logits_proc_ref.py) and the arg-max (lowest index among ties).  Finished rows emit the
pad id and their partners keep decoding it, as transformers appends it to input_ids.  tests/test_guidance_host.py holds this
restatement to the installed transformers; the GPU tests hold the device to it.  Test infrastructure, not product code."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch


def combine(cond: torch.Tensor, uncond: torch.Tensor, g: float, dtype=torch.float32) -> torch.Tensor:
    """Host twin of guidance_combine_kernel: HF's expression on the two log-softmaxes, evaluated in `dtype`."""
    c = torch.log_softmax(cond.to(dtype), dim=-1)
    u = torch.log_softmax(uncond.to(dtype), dim=-1)
    return g * (c - u) + u


def combine_with_lse(cond: torch.Tensor, uncond: torch.Tensor, lse_c: torch.Tensor, lse_u: torch.Tensor, g: float) -> torch.Tensor:
    """The same from given log-sum-exps [n], in the operand's dtype (fp32: the kernel's operation order, its multiply-add in one
    rounding aside)."""
    a = cond - lse_c[:, None]
    w = uncond - lse_u[:, None]
    return g * (a - w) + w


def pad_left(emb_c, mask_c, emb_u, mask_u):
    """[P, Tc, H] / [P, Tu, H] left-padded sets -> one [2 P, T, H] set and its bool mask (what model.pad_left_common does)."""
    T = max(emb_c.shape[1], emb_u.shape[1])
    P = emb_c.shape[0]
    emb = torch.zeros((2 * P, T, emb_c.shape[2]), dtype=emb_c.dtype)
    mask = torch.zeros((2 * P, T), dtype=torch.bool)
    emb[:P, T - emb_c.shape[1]:] = emb_c
    emb[P:, T - emb_u.shape[1]:] = emb_u
    mask[:P, T - mask_c.shape[1]:] = mask_c.bool()
    mask[P:, T - mask_u.shape[1]:] = mask_u.bool()
    return emb, mask


def top1_gap(scores: torch.Tensor) -> torch.Tensor:
    """[B, V] -> [B]: best minus second best value (inf when fewer than two finite values)."""
    v = torch.topk(scores.double(), 2, dim=-1).values
    gap = v[:, 0] - v[:, 1]
    return torch.where(torch.isfinite(gap), gap, torch.full_like(gap, float("inf")))


def guided_generate(logits_fn: Callable, embed_fn: Callable, emb_c, mask_c, emb_u, mask_u, g: float, max_new: int,
                    eos: Sequence[int] = (), pad_id: int = 0, process: Optional[Callable] = None, forced=None):
    """logits_fn(embeds [R, T, H], mask bool [R, T]) -> last-position logits [R, V]; embed_fn(ids [R]) -> [R, H];
    process(scores [P, V], hist [P, t]) -> processed scores (None: none); forced [P, n]: ids to follow instead of the arg-max
    (teacher forcing).  Returns dict(ids [P, n], scores [n, P, V] guided and processed, logits [n, P, V] raw conditional,
    gaps [n, P] top-1 gap of the scores (inf for a finished row), unfinished [n, P])."""
    P = emb_c.shape[0]
    emb, mask = pad_left(emb_c, mask_c, emb_u, mask_u)
    ids = torch.zeros((P, 0), dtype=torch.long)
    fin = torch.zeros(P, dtype=torch.bool)
    scores, raws, gaps, unf = [], [], [], []
    eos = [int(e) for e in eos]
    for t in range(max_new):
        lg = logits_fn(emb, mask).float()
        c, u = lg[:P], lg[P:]
        s = combine(c, u, g)
        if process is not None:
            s = process(s, ids)
        tok = torch.from_numpy(np.argmax(s.numpy(), axis=1)).long()           # first index among ties
        if forced is not None:
            tok = forced[:, t].long().clone()
        gp = top1_gap(s)
        gp[fin] = float("inf")
        unf.append(~fin.clone())
        tok = torch.where(fin, torch.full_like(tok, pad_id), tok)
        scores.append(s)
        raws.append(c.clone())
        gaps.append(gp)
        ids = torch.cat([ids, tok[:, None]], dim=1)
        for e in eos:
            fin = fin | (tok == e)
        if bool(fin.all()):
            break
        nxt = embed_fn(torch.cat([tok, tok]))
        emb = torch.cat([emb, nxt[:, None].to(emb.dtype)], dim=1)
        mask = torch.cat([mask, torch.ones((2 * P, 1), dtype=torch.bool)], dim=1)
    return dict(ids=ids, scores=torch.stack(scores), logits=torch.stack(raws), gaps=torch.stack(gaps), unfinished=torch.stack(unf))
