"""Offset planning of generate(prefix=...) / opus_llama_prefill_behind: pure host arithmetic, no GPU and no library.

A detached prefix holds P rows of Tp cache slots; row p's real tokens sit at slots kstart[p] .. Tp - 1 (Lp = Tp - kstart[p] of them).
R suffix rows of n right-padded positions (n_r real ones, d_r = n - n_r) continue prefix rows src[r].  After the prefill behind the
prefix the context looks like a left-padded prefill of the concatenated prompts with T' = Tp + n slots:

    kstart'[r]           = kstart[p] + d_r                     first real slot of decode row r
    prefix of row r      : slots kstart'[r] .. kstart'[r] + Lp - 1   (moved by d_r, bits unchanged: K is rotated by slot - kstart)
    suffix position t    : slot Tp + d_r + t                   (t < n_r), so every row ends at slot T' - 1
    position of suffix t : Lp + t                              (= t - nkst[r] with nkst[r] = kstart[p] - Tp, as scoring uses it)
    decode step i        : slot T' + i, position Lp + n_r + i  (the decode step's slot - kstart' rule)

`off` / `list` group the decode rows by prefix row (the native PrefixTables): rows list[off[p] .. off[p + 1]) continue row p.

The way back (generate(return_prefix=True) / opus_llama_prefix_export_rows): after s decode steps behind a prefill of T0 slots, row
r keeps h_keep[r] <= s of the appended slots; its window kstart[r] .. T0 + h_keep[r] - 1 (L_r slots) lands right-aligned in a
snapshot of Tp_out = max L_r slots, new kstart Tp_out - L_r (plan_export_rows).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np


class CapacityError(ValueError):
    """A shape the context cannot hold; model.generate() re-raises it as OpusError -2 with the same message."""


class BehindPlan:
    """What plan_prefill_behind returns (all int32 arrays): R, n, P, Tp, T_new; src, lens, pad (d_r), new_kstart [R]; nkst [R];
    prefix_slot0 [R] (= new_kstart), prefix_len [R] (Lp), suffix_slot0 [R] (slot of suffix position 0); off [P + 1], list [R]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def snapshot_bytes(layers: int, kv_heads: int, head_dim: int, P: int, Tp: int, itemsize: int = 2) -> int:
    """Bytes of a snapshot's K plus V: [layers][P][kv heads][Tp][head_dim] each (opus_llama_prefix_bytes)."""
    return 2 * layers * P * kv_heads * Tp * head_dim * itemsize


def plan_export_rows(kstart: Sequence[int], T0: int, keep: Sequence[int]):
    """Host mirror of opus_llama_prefix_export_rows.  kstart [R], T0: the live cache after a prefill of T0 slots; keep [R]: how many
    of the slots the decode steps appended belong to row r.  Row r's window is slots kstart[r] .. T0 + keep[r] - 1, L_r = T0 -
    kstart[r] + keep[r] of them; in a snapshot of Tp_out = max L_r slots it sits at slots Tp_out - L_r .. Tp_out - 1.  Returns
    (lengths int64 [R], Tp_out, new_kstart int32 [R]) with new_kstart + lengths == Tp_out."""
    kst = np.asarray(kstart, dtype=np.int64).reshape(-1)
    kp = np.asarray(keep, dtype=np.int64).reshape(-1)
    if kst.shape[0] < 1 or kp.shape[0] != kst.shape[0]:
        raise ValueError(f"{kp.shape[0]} keep counts for {kst.shape[0]} rows")
    if T0 < 1 or (kst < 0).any() or (kst >= T0).any():
        raise ValueError(f"a cache of {T0} prompt slots needs 0 <= kstart < T0 for every row")
    if (kp < 0).any():
        raise ValueError("keep counts must not be negative")
    lengths = T0 - kst + kp
    Tp_out = int(lengths.max())
    return lengths, Tp_out, np.ascontiguousarray(Tp_out - lengths, dtype=np.int32)


def plan_prefill_behind(kstart: Sequence[int], Tp: int, src: Sequence[int], lens: Sequence[int], n: int, max_batch: int,
                        max_prompt: int, rows_cap: int) -> BehindPlan:
    """kstart [P], Tp: the prefix; src [R], lens [R], n: the suffix rows.  max_batch / max_prompt: the context's capacities,
    rows_cap: positions its prefill buffers hold (opus_llama_dec_rows_cap).  ValueError for an empty suffix row, a length beyond n
    or a prefix row outside [0, P); CapacityError (with the numbers) when the context cannot hold the result."""
    kst = np.asarray(kstart, dtype=np.int64).reshape(-1)
    src_a = np.asarray(src, dtype=np.int64).reshape(-1)
    lens_a = np.asarray(lens, dtype=np.int64).reshape(-1)
    P, R = int(kst.shape[0]), int(src_a.shape[0])
    if P < 1 or Tp < 1 or (kst < 0).any() or (kst >= Tp).any():
        raise ValueError(f"a prefix of {P} rows x {Tp} slots needs 0 <= kstart < Tp for every row")
    if R < 1:
        raise ValueError("generate(prefix=...) needs at least one suffix row")
    if lens_a.shape[0] != R:
        raise ValueError(f"{lens_a.shape[0]} suffix lengths for {R} rows")
    if (lens_a < 1).any():
        raise ValueError(f"suffix row {int(np.argmax(lens_a < 1))} is empty: every row needs at least one token behind the prefix")
    if n < 1 or (lens_a > n).any():
        raise ValueError(f"suffix lengths must lie in [1, n={n}]")
    if (src_a < 0).any() or (src_a >= P).any():
        raise ValueError(f"prefix_rows must lie in [0, {P})")
    if R > max_batch:
        raise CapacityError(f"generate(prefix=...): {R} decoder rows, the context holds max_batch={max_batch}")
    if Tp + n > max_prompt:
        raise CapacityError(f"generate(prefix=...): prefix of {Tp} slots + suffix of {n} positions = {Tp + n}, the context holds "
                            f"max_prompt={max_prompt}")
    if R * n > rows_cap:
        raise CapacityError(f"generate(prefix=...): {R} x {n} suffix positions, the prefill buffers hold {rows_cap}")
    pad = n - lens_a
    new_kstart = kst[src_a] + pad
    off = np.zeros(P + 1, dtype=np.int64)
    np.add.at(off, src_a + 1, 1)
    off = np.cumsum(off)
    order = np.argsort(src_a, kind="stable")
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)          # noqa: E731
    return BehindPlan(R=R, n=int(n), P=P, Tp=int(Tp), T_new=int(Tp + n), src=i32(src_a), lens=i32(lens_a), pad=i32(pad),
                      new_kstart=i32(new_kstart), nkst=i32(kst[src_a] - Tp), prefix_slot0=i32(new_kstart),
                      prefix_len=i32(Tp - kst[src_a]), suffix_slot0=i32(Tp + pad), off=i32(off), list=i32(order))
