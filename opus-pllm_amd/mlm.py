"""Host side of the ESM-2 masked-LM head: mutation strings, the plan of masked copies and the result record of
`score_mutations` (model.py).  Pure host logic, no GPU: the two scoring strategies are those of fair-esm's
examples/variant-prediction/predict.py ("wt-marginals", "masked-marginals"), scored over the full 33-token alphabet.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .alphabet import ALL_TOKS, MASK_IDX, TOK_TO_IDX

MODES = ("wt-marginals", "masked-marginals")
_MUT = re.compile(r"(\S)(-?\d+)(\S+)")


def parse_mutation(mutation: str, tokens: Sequence[int], offset_idx: int = 1) -> List[Tuple[int, int, int]]:
    """"A23G" or "A23G:L40P" -> [(0-based residue, wild-type id, mutant id)] for the protein whose residue ids are `tokens`.
    Positions count from `offset_idx` (1: the first residue is 1, as predict.py's default).  ValueError, naming the string, when
    it is malformed, the position lies outside the protein, the wild-type letter is not the protein's residue there (predict.py
    asserts this) or the target is not a symbol of the alphabet."""
    out = []
    for part in str(mutation).split(":"):
        m = _MUT.fullmatch(part.strip())
        if not m:
            raise ValueError(f"mutation {mutation!r}: {part!r} is not <wild type><position><mutant> (such as A23G)")
        wt, pos, mt = m.group(1), int(m.group(2)), m.group(3)
        idx = pos - offset_idx
        if idx < 0 or idx >= len(tokens):
            raise ValueError(f"mutation {mutation!r}: position {pos} is out of range for a protein of {len(tokens)} residues "
                             f"(positions {offset_idx} .. {len(tokens) + offset_idx - 1})")
        if mt not in TOK_TO_IDX:
            raise ValueError(f"mutation {mutation!r}: target {mt!r} is not in the alphabet")
        have = ALL_TOKS[int(tokens[idx])]
        if wt != have:
            raise ValueError(f"mutation {mutation!r}: wild type {wt!r} does not match the sequence, which has {have!r} at position {pos}")
        out.append((idx, int(tokens[idx]), TOK_TO_IDX[mt]))
    return out


def scan_positions(lengths: Sequence[int], positions=None, parsed_mutations=None) -> List[List[int]]:
    """The residues (0-based, ascending, no repeats) to scan per protein: `positions` when given, else the positions the
    mutations mention, else all of them."""
    out = []
    for i, n in enumerate(lengths):
        if positions is not None:
            ps = sorted({int(p) for p in positions[i]})
            if ps and (ps[0] < 0 or ps[-1] >= n):
                raise ValueError(f"positions[{i}] must lie in [0, {n}), got {ps[0]} .. {ps[-1]}")
        elif parsed_mutations is not None:
            ps = sorted({idx for mut in parsed_mutations[i] for idx, _, _ in mut})
        else:
            ps = list(range(n))
        out.append(ps)
    return out


def plan_masked_copies(scan: Sequence[Sequence[int]], lengths: Sequence[int], max_batch: int,
                       max_enc_tokens: int) -> List[List[Tuple[int, int]]]:
    """Masked copies (protein, residue), in order, cut into encoder calls of at most max_batch copies; copies of different
    proteins share a call.  len(result) == ceil(copies / max_batch).  A protein longer than max_enc_tokens - 2 residues cannot be
    encoded: ValueError."""
    copies = []
    for i, ps in enumerate(scan):
        if ps and lengths[i] + 2 > max_enc_tokens:
            raise ValueError(f"protein {i} of {lengths[i]} residues exceeds max_enc_tokens={max_enc_tokens}")
        copies.extend((i, int(j)) for j in ps)
    return [copies[k:k + max_batch] for k in range(0, len(copies), max_batch)]


def masked_copy(tokens: np.ndarray, j: int) -> np.ndarray:
    t = np.array(tokens, dtype=np.int32, copy=True)
    t[j] = MASK_IDX
    return t


@dataclass
class MutationScores:
    """Result of score_mutations.  Per protein i of n_i residues (tensors on the model's device, fp32):
    log_probs[i] [n_i, 33] = log p(token at j | context), log-softmax over the whole alphabet, NaN in rows that were not scanned;
    wt_log_prob[i] [n_i] its wild-type column; scores[i] = log_probs[i] - wt_log_prob[i][:, None];
    pseudo_log_likelihood [P] = sum of wt_log_prob over the scanned rows and pseudo_perplexity [P] = exp(-that / rows);
    mutation_scores[i] [len(mutations[i])] when mutations were given (a multiple mutation is the sum of its parts);
    rows_evaluated = rows the head ran on, encoder_calls = packed encoder calls made."""
    mode: str
    log_probs: list
    wt_log_prob: list
    scores: list
    pseudo_log_likelihood: object
    pseudo_perplexity: object
    mutation_scores: Optional[list] = None
    rows_evaluated: int = 0
    encoder_calls: int = 0
    positions: list = field(default_factory=list)
