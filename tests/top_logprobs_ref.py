"""The definition of top log-probs, restated in fp64 (tests only).

For a raw logits row l[0..V) and 1 <= k <= min(20, V):
  top_ids[j]      = index of the j-th entry when the entries are ordered by value descending, then index ascending
                    (np.argsort(-l, kind="stable")[:k]: an exact comparison of the stored values, -0 == +0, -inf last)
  top_logprobs[j] = l[top_ids[j]] - logsumexp(l)            (-inf for a -inf entry)
"""
from __future__ import annotations

import numpy as np

K_MAX = 20


def lse64(rows: np.ndarray) -> np.ndarray:
    """fp64 log-sum-exp of every row of [R, V] (-inf entries add nothing)."""
    x = np.asarray(rows, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def top_logprobs_ref(rows: np.ndarray, k: int, lse: np.ndarray | None = None):
    """rows [R, V] (any float dtype; its stored values are what is ordered) -> (ids int64 [R, k], logprobs fp64 [R, k], lse fp64 [R])."""
    x = np.asarray(rows)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float32)                  # (16-bit values are exact in fp32)
    R, V = x.shape
    assert 1 <= k <= min(K_MAX, V), (k, V)
    ids = np.stack([np.argsort(-x[r], kind="stable")[:k] for r in range(R)]).astype(np.int64)
    l = lse64(x) if lse is None else np.asarray(lse, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lp = np.take_along_axis(x.astype(np.float64), ids, axis=1) - l[:, None]
    return ids, lp, l


def top_ids_fast(rows: np.ndarray, k: int) -> np.ndarray:
    """The same ids as top_logprobs_ref without sorting whole rows: the k-th largest value by selection, then the stable order of
    the entries at or above it (test_top_logprobs_host.py checks the two against each other)."""
    x = np.asarray(rows)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float32)
    out = np.empty((x.shape[0], k), dtype=np.int64)
    for r in range(x.shape[0]):
        kth = np.partition(x[r], x.shape[1] - k)[x.shape[1] - k]
        cand = np.flatnonzero(x[r] >= kth)                     # ascending index
        out[r] = cand[np.argsort(-x[r, cand], kind="stable")[:k]]
    return out


def top_logprobs_fast(rows: np.ndarray, k: int, lse: np.ndarray | None = None):
    x = np.asarray(rows)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float32)
    ids = top_ids_fast(x, k)
    l = lse64(x) if lse is None else np.asarray(lse, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lp = np.take_along_axis(x, ids, axis=1).astype(np.float64) - l[:, None]
    return ids, lp, l
