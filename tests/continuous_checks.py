"""Shared by tests/test_gpu_continuous.py and tools/gen_continuous_seed.py (which picks E2E_SEEDS on the CPU oracle): the prompts of
the end-to-end case, the run-time choice of its EOS ids and the decisive-step comparison.  Test infrastructure, not product code."""
from __future__ import annotations

import numpy as np
import torch

from opus_pllm_amd import synth

PAD = 2
MARGIN_TAU = 0.05                      # the project's decisive-step rule (tests/prefix_generate_checks.py)
# end to end: 11 prompts, text ids per prompt (one <seq> placeholder each: spliced length = n_text - 1 + n_prot_tokens)
E2E_TEXT = (7, 15, 3, 11, 5, 45, 19, 4, 27, 9, 37)
E2E_SLOTS, E2E_MAX_NEW, E2E_S, E2E_MAX_PROMPT = 4, 12, 40, 56
# preset -> (prompt seed, decisive fraction of the plain call on it): chosen by tools/gen_continuous_seed.py
E2E_SEEDS = {"micro_opt": (67, 1.0), "micro_qwen": (47, 1.0)}          # (the best of seeds 0 .. 119)


def e2e_prompts(cfg, seed: int):
    """(prompts: list of 1-D int64 tensors, proteins: list of str) of the end-to-end case."""
    prompts = [torch.tensor(synth.synth_prompt_ids(cfg.dec_vocab, 1000 * seed + i, n_text=n, seq_pos=min(2, n - 1)), dtype=torch.long)
               for i, n in enumerate(E2E_TEXT)]
    seqs = [synth.synth_protein(12 + (7 * i + seed) % 30, 100 * seed + i) for i in range(len(E2E_TEXT))]
    return prompts, seqs


def left_pad(rows, pad=PAD):
    width = max(len(r) for r in rows)
    ids = torch.full((len(rows), width), pad, dtype=torch.long)
    mask = torch.zeros((len(rows), width), dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.as_tensor(r, dtype=torch.long)
        mask[i, width - len(r):] = True
    return ids, mask


def lengths_under(free: np.ndarray, eos) -> list:
    """Ids a row emits when `eos` end it: up to and including its first EOS id, else all of them."""
    out = []
    for row in free:
        hit = [k for k, t in enumerate(row.tolist()) if t in eos]
        out.append(hit[0] + 1 if hit else len(row))
    return out


def choose_eos(free: np.ndarray):
    """Two EOS ids, picked from the ids the free run emitted, that make the rows end at as many different steps as possible (ties:
    the larger spread of lengths, then the smaller ids): a deterministic function of `free` [N, n]."""
    cand = sorted(set(int(t) for t in free.reshape(-1).tolist()) - {PAD})
    best = None
    for i, a in enumerate(cand):
        for b in cand[i + 1:]:
            ln = lengths_under(free, (a, b))
            key = (len(set(ln)), float(np.var(ln)), -a, -b)
            if best is None or key > best[0]:
                best = (key, (a, b))
    return list(best[1])


def margins_of(logits) -> torch.Tensor:
    """[R, n] top-1 margins from generate(output_logits=True)'s per-step logits."""
    top = torch.stack([torch.topk(l.float().cpu(), 2, dim=1).values for l in logits], 1)
    return top[..., 0] - top[..., 1]


def decisive_compare(got, ref_rows, ref_margins, lens):
    """got: N 1-D tensors; ref_rows [N, n] the plain call's ids, ref_margins [N, n], lens [N] the plain call's counted lengths.
    Every id must be equal up to a row's first step whose reference margin is below MARGIN_TAU; (fraction of the reference's ids
    that were checked, ids equal, lengths equal on the fully decisive rows)."""
    checked = total = 0
    ids_ok = len_ok = True
    for p, g in enumerate(got):
        n = int(lens[p])
        low = (ref_margins[p, :n] < MARGIN_TAU).nonzero()
        m = int(low[0]) if len(low) else n
        ids_ok &= bool(torch.equal(g.cpu()[:m], ref_rows[p, :m].cpu())) if len(g) >= m else False
        if m == n:
            len_ok &= len(g) == n
        checked += m
        total += n
    return checked / max(total, 1), ids_ok, len_ok
