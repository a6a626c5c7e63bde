"""Checks of top log-probs (generate(top_logprobs=k), forward(labels, top_logprobs=k), opus_debug_top_logprobs) shared by
tests/test_gpu_top_logprobs.py (fp16-operand build) and its bf16 child process (tests/bf16_top_logprobs_check.py).  Each returns a
dict of observations; the callers assert the bounds.  Test infrastructure, not product code."""
from __future__ import annotations

import numpy as np
import torch

from opus_pllm_amd import _cabi
import gen_scores_checks as gsc
import top_logprobs_ref as tref

llama8b_shape = gsc.llama8b_shape
APART = 64


def part_len(V: int) -> int:
    """Values per part of the 64-part cut of a row (csrc: per)."""
    return ((V + APART - 1) // APART + 3) & ~3


# ------------------------------------------------------------------------------------------------ kernel level
def kernel_contents(V: int, seed: int = 5):
    """{name: fp32 rows [R, V]}: what the selection can get wrong at this V."""
    g = np.random.default_rng(seed + V)
    per = part_len(V)
    out = {"gauss": (g.standard_normal((64, V)) * 4).astype(np.float32)}
    off = g.standard_normal((3, V)).astype(np.float32)
    off[0] += 1e4
    off[1] -= 1e4
    off[2] *= 1e4
    out["pm1e4"] = off
    kk = min(20, V)
    adj = g.standard_normal((3, V)).astype(np.float32)
    strad = adj.copy()
    for r in range(3):
        part = (1 + 17 * r) % max(1, (V + per - 1) // per)
        a0 = min(part * per + (per - kk) // 2 if per >= kk else part * per, V - kk)      # kk adjacent indices (inside one part when it holds them)
        adj[r, a0:a0 + kk] = 50.0 + g.permutation(kk).astype(np.float32)
        b0 = min(max((part + 1) * per - kk // 2, 0), V - kk)                             # kk indices across the part boundary
        strad[r, b0:b0 + kk] = 50.0 + g.permutation(kk).astype(np.float32)
    out["adjacent"], out["straddle"] = adj, strad
    out["small_ints"] = g.integers(0, 4, (3, V)).astype(np.float32)
    out["all_equal"] = np.full((3, V), 1.25, dtype=np.float32)
    return out


def three_finite(V: int, seed: int = 9):
    g = np.random.default_rng(seed + V)
    x = np.full((3, V), -np.inf, dtype=np.float32)
    for r in range(3):
        x[r, g.choice(V, 3, replace=False)] = g.standard_normal(3).astype(np.float32)
    return x


def run_kernel(model, dev, rows: np.ndarray, k: int, f32: bool, ld: int | None = None, lse: np.ndarray | None = None, offset: int = 0):
    """opus_debug_top_logprobs on rows [R, V] (fp32 values; f32 False: stored in the build's 16-bit type) with leading dimension
    ld, the first row `offset` elements into an aligned buffer -> (stored rows as fp32 [R, V], ids int64 [R, k], lp fp32 [R, k])."""
    lib = _cabi.lib()
    R, V = rows.shape
    ld = V if ld is None else ld
    dt = torch.float32 if f32 else _cabi.operand_dtype()
    buf = torch.zeros(R * ld + offset + 8, dtype=dt, device=dev)
    view = buf[offset: offset + R * ld].view(R, ld)
    view[:, :V] = torch.from_numpy(rows).to(dev).to(dt)
    if ld > V:
        view[:, V:] = 1e4                                                   # (values outside the row must not be picked)
    ids = torch.full((R, k), -7, dtype=torch.int32, device=dev)
    lp = torch.full((R, k), 7.0, dtype=torch.float32, device=dev)
    d_lse = None if lse is None else torch.from_numpy(np.asarray(lse, dtype=np.float32)).to(dev)
    s = torch.cuda.current_stream(dev)
    _cabi.check(lib.opus_debug_top_logprobs(model._ctx, buf.data_ptr() + offset * buf.element_size(), _cabi.OPUS_F32 if f32 else _cabi.OPUS_F16,
                                            ld, R, V, k, None if d_lse is None else d_lse.data_ptr(), ids.data_ptr(), lp.data_ptr(),
                                            s.cuda_stream))
    torch.cuda.synchronize(dev)
    return view[:, :V].float().cpu().numpy(), ids.long().cpu().numpy(), lp.cpu().numpy()


def compare(stored: np.ndarray, ids: np.ndarray, lp: np.ndarray, k: int, lse=None, fast: bool = True) -> dict:
    """ids against the reference exactly; lp as |lp - ref| / max(1, |lse_ref|) (both -inf: equal)."""
    ref = tref.top_logprobs_fast if fast else tref.top_logprobs_ref
    r_ids, r_lp, r_lse = ref(stored, k, lse)
    both_inf = np.isneginf(r_lp) & np.isneginf(lp)
    with np.errstate(invalid="ignore"):
        d = np.where(both_inf, 0.0, np.abs(lp.astype(np.float64) - r_lp)) / np.maximum(1.0, np.abs(r_lse))[:, None]
    d = np.where(np.isnan(d), np.inf, d)
    return {"id_mismatches": int((ids != r_ids).sum()), "lp_rel": float(d.max()), "rows": int(stored.shape[0])}


def kernel_cases(model, dev, V: int, f32: bool) -> dict:
    """Every content at this V and input type: R in {1, 3, 64} and k in {1, 5, 20} on the Gaussian rows, the constructed rows at
    k = 20 (or V) and 5, with and without a caller's lse, contiguous and with a leading dimension."""
    res = {}
    cont = kernel_contents(V)
    kmax = min(20, V)
    gauss = cont["gauss"]
    for R in (1, 3, 64):
        for k in (1, 5, kmax):
            stored, ids, lp = run_kernel(model, dev, gauss[:R], k, f32)
            res[f"gauss.R{R}.k{k}"] = compare(stored, ids, lp, k)
    stored, ids, lp = run_kernel(model, dev, gauss[:3], 5, f32, lse=tref.lse64(_stored(gauss[:3], f32)))
    res["gauss.given_lse"] = compare(stored, ids, lp, 5, lse=tref.lse64(stored).astype(np.float32))
    stored, ids, lp = run_kernel(model, dev, gauss[:3], kmax, f32, ld=V + 5, offset=1)     # a leading dimension, unaligned rows
    res["gauss.ld"] = compare(stored, ids, lp, kmax)
    for name in ("pm1e4", "adjacent", "straddle", "small_ints", "all_equal"):
        for k in (5, kmax):
            stored, ids, lp = run_kernel(model, dev, cont[name], k, f32)
            res[f"{name}.k{k}"] = compare(stored, ids, lp, k)
            if name == "all_equal":
                res[f"{name}.k{k}"]["ids_are_first"] = bool((ids == np.arange(k)[None, :]).all())
                res[f"{name}.k{k}"]["lp_abs"] = float(np.abs(lp.astype(np.float64) + np.log(V)).max())
    stored, ids, lp = run_kernel(model, dev, three_finite(V), min(5, V), f32)
    res["three_finite.k5"] = compare(stored, ids, lp, min(5, V))
    res["three_finite.k5"]["inf_tail"] = bool(np.isneginf(lp[:, 3:]).all() and np.isfinite(lp[:, :3]).all())
    return res


def _stored(rows: np.ndarray, f32: bool) -> np.ndarray:
    return rows if f32 else torch.from_numpy(rows).to(_cabi.operand_dtype()).float().numpy()


# ------------------------------------------------------------------------------------------------ generate level
def gen(model, ids, mask, seqs, max_new, k=None, sampling=None, seed=11, **kw):
    a = dict(attention_mask=mask, pad_token_id=2, max_new_tokens=max_new)
    if sampling:
        a.update(do_sample=True, seed=seed, **sampling)
    a.update(kw)
    if k is not None:
        a.update(return_dict_in_generate=True, output_logits=True, output_token_logprobs=True, top_logprobs=k)
    return model.generate(ids, seqs, **a) if seqs is not None else model.generate(ids, **a)


def consistency(o, k: int, plain_path: bool) -> dict:
    """One output with logits, token_logprobs and top log-probs: the top-k recomputed in fp64 from the returned raw logits, the
    chosen id's entry against token_logprobs, 0 / -1 behind a row's end."""
    seq = o.sequences.cpu().numpy()
    B, n = seq.shape
    cnt = o.n_tokens.cpu().numpy()
    tid, tlp = o.top_ids.cpu().numpy(), o.top_logprobs.cpu().numpy()
    tok_lp = o.token_logprobs.cpu().numpy()
    assert tid.shape == tlp.shape == (B, n, k), (tid.shape, tlp.shape, (B, n, k))
    assert o.top_ids.dtype == torch.int64 and o.top_logprobs.dtype == torch.float32
    mism = 0
    worst = tok_worst = 0.0
    tok_bitwise, tok_seen, after_ok = True, 0, True
    for t in range(n):
        lg = o.logits[t].float().cpu().numpy()
        r_ids, r_lp, _ = tref.top_logprobs_fast(lg, k)
        for b in range(B):
            if t >= cnt[b]:
                after_ok &= bool((tid[b, t] == -1).all() and (tlp[b, t] == 0).all())
                continue
            mism += int((tid[b, t] != r_ids[b]).sum())
            fin = np.isfinite(r_lp[b])
            worst = max(worst, float(np.abs(tlp[b, t][fin] - r_lp[b][fin]).max()) if fin.any() else 0.0)
            after_ok &= bool(np.array_equal(np.isneginf(tlp[b, t]), ~fin))
            hit = np.flatnonzero(tid[b, t] == seq[b, t])
            if hit.size:
                tok_seen += 1
                tok_bitwise &= bool(tlp[b, t, hit[0]] == tok_lp[b, t])
                tok_worst = max(tok_worst, float(abs(float(tlp[b, t, hit[0]]) - float(tok_lp[b, t]))))
    return {"n": n, "id_mismatches": mism, "lp_abs": worst, "tail_ok": bool(after_ok), "chosen_seen": tok_seen,
            "chosen_bitwise": bool(tok_bitwise) if plain_path else None, "chosen_abs": tok_worst,
            "top1_is_id": bool((tid[:, :, 0] == seq)[np.arange(n)[None, :] < cnt[:, None]].all())}


def graphs(model, ids, mask, seqs, max_new, sampling=None) -> dict:
    """ids with the argument equal those without; a plain call afterwards, and another k, instantiate no graph."""
    plain = gen(model, ids, mask, seqs, max_new, sampling=sampling)
    a = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=max_new, return_dict_in_generate=True, top_logprobs=3,
                       **(dict(do_sample=True, seed=11, **sampling) if sampling else {}))
    i0 = model.stat("graph_instantiations")
    b = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=max_new, return_dict_in_generate=True, top_logprobs=7,
                       **(dict(do_sample=True, seed=11, **sampling) if sampling else {}))
    i1 = model.stat("graph_instantiations")
    again = gen(model, ids, mask, seqs, max_new, sampling=sampling)
    i2 = model.stat("graph_instantiations")
    ignored = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=max_new, top_logprobs=4,
                             **(dict(do_sample=True, seed=11, **sampling) if sampling else {}))
    return {"ids_equal": bool(torch.equal(a.sequences, plain) and torch.equal(b.sequences, plain) and torch.equal(again, plain)),
            "k7_new_graphs": i1 - i0, "plain_new_graphs": i2 - i1, "k3_prefix_of_k7": bool(torch.equal(a.top_ids, b.top_ids[:, :, :3])),
            "ignored_is_tensor": isinstance(ignored, torch.Tensor) and bool(torch.equal(ignored, plain)),
            "only_top_fields": a.token_logprobs is None and a.top_ids.shape[2] == 3}
