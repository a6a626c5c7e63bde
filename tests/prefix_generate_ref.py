"""Brute-force restatement of the offset planning of generate(prefix=...) (opus_pllm_amd/prefix.py), written from the issue's
geometry alone: build the concatenated prompt of every decode row token by token, left-pad it to T' = Tp + n and read the numbers
off the result.  Test infrastructure, not product code."""
from __future__ import annotations

import numpy as np


def brute_plan(kstart, Tp, src, lens, n):
    """Every row as a list of (origin, index) per slot: ("pad", -) | ("prefix", prefix slot) | ("suffix", t).  The concatenated
    prompt of row r is the real prefix tokens of row src[r] followed by its n_r suffix tokens, left-padded to Tp + n slots."""
    T = Tp + n
    out = dict(T_new=T, new_kstart=[], prefix_slot0=[], prefix_len=[], suffix_slot0=[], pos_suffix0=[], rows=[])
    for r, p in enumerate(src):
        toks = [("prefix", s) for s in range(kstart[p], Tp)] + [("suffix", t) for t in range(lens[r])]
        row = [("pad", -1)] * (T - len(toks)) + toks
        assert len(row) == T
        first_real = next(i for i, x in enumerate(row) if x[0] != "pad")
        first_suffix = next(i for i, x in enumerate(row) if x[0] == "suffix")
        out["rows"].append(row)
        out["new_kstart"].append(first_real)
        out["prefix_slot0"].append(first_real)
        out["prefix_len"].append(sum(1 for x in row if x[0] == "prefix"))
        out["suffix_slot0"].append(first_suffix)
        out["pos_suffix0"].append(first_suffix - first_real)       # position of a slot: slot - kstart'
    return out


def brute_groups(src, P):
    """Rows grouped by prefix row, in row order: (off [P + 1], list [R])."""
    groups = [[r for r, p in enumerate(src) if p == q] for q in range(P)]
    off = np.cumsum([0] + [len(g) for g in groups])
    return off, [r for g in groups for r in g]
