"""Checks of generate()'s logits processors shared by tests/test_gpu_logits_proc.py (fp16-operand build) and its bf16 child
process (tests/bf16_logits_proc_check.py).  Each returns a dict of observations; the callers assert the bounds.  Test
infrastructure, not product code."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

from opus_pllm_amd import _cabi
import gen_scores_checks as gsc
import logits_proc_ref as lpr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = [[62], [52, 20], [5, 6, 7]]


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().float().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ kernel level
def _kernel_case(g, B, V, L, penalty, ngram, n_bad, eos):
    """Logits with both signs, histories of L ids built from a short motif (repeats and recurring n-grams), bad words cut from the
    histories' tails (so that their prefixes match), random ones, lengths 1 to 8 and one equal to [eos]."""
    x = torch.randn(B, V, generator=g) * 4
    pool = torch.randint(0, V, (B, 12), generator=g)
    hist = torch.empty((B, max(L, 1)), dtype=torch.int32)
    for b in range(B):
        motif = pool[b, : 3 + b % 7]
        h = motif.repeat(L // len(motif) + 1)[:L].clone()
        noise = torch.rand(L, generator=g) < 0.2
        h[noise] = pool[b, torch.randint(0, 12, (int(noise.sum()),), generator=g)]
        hist[b, :L] = h.int()
    bad = []
    for e in range(n_bad):
        n = 1 + e % 8
        b = e % B
        if e % 3 == 0 and L >= n:                        # prefix = row b's last n - 1 ids: banned there
            w = hist[b, L - n + 1: L].tolist() + [int(torch.randint(0, V, (1,), generator=g))]
        else:
            w = torch.randint(0, V, (n,), generator=g).tolist()
        bad.append([int(t) for t in w])
    if eos:
        bad.append([eos[0]])                             # dropped: equal to [eos]
    return x, hist, bad


def kernel(model, dev):
    """opus_debug_logits_process against the restatement, bit for bit (processed and untouched entries)."""
    lib = _cabi.lib()
    s = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(7)
    res = {}
    cases = []
    for V in (96, 128256, 152064):
        for B in (1, 64):
            for L, pen, ngram, n_bad, min_new in ((0, 1.3, 2, 4, 1), (1, 0.8, 1, 3, 0), (17, 1.3, 2, 9, 30), (64, 2.0, 3, 24, 0),
                                                   (256, 0.8, 4, 40, 300), (255, 1.0, 0, 0, 0), (100, 1.3, 0, 0, 0),
                                                   (100, 1.0, 3, 0, 0), (100, 1.0, 0, 16, 0)):
                cases.append((V, B, L, pen, ngram, n_bad, min_new))
    for V, B, L, pen, ngram, n_bad, min_new in cases:
        eos = [int(t) for t in torch.randint(0, V, (2,), generator=g)]
        x, hist, bad = _kernel_case(g, B, V, L, pen, ngram, n_bad, eos)
        stride = hist.shape[1] + 3
        hd = torch.zeros((B, stride), dtype=torch.int32)
        hd[:, : hist.shape[1]] = hist
        d_x, d_h = x.to(dev), hd.to(dev)
        flat = [t for w in bad for t in w]
        offs = np.cumsum([0] + [len(w) for w in bad]).tolist()
        ids = (C.c_int32 * max(1, len(flat)))(*flat)
        off = (C.c_int32 * len(offs))(*offs)
        ea = (C.c_int32 * len(eos))(*eos)
        _cabi.check(lib.opus_debug_logits_process(model._ctx, d_x.data_ptr(), B, V, d_h.data_ptr(), stride, L, ea, len(eos), pen,
                                                  ngram, min_new, ids, off, len(bad), s.cuda_stream))
        torch.cuda.synchronize(dev)
        want = lpr.process(x, hist[:, :L], eos=eos, penalty=pen, ngram=ngram, bad=bad, min_new=min_new)
        got = d_x.cpu()
        touched = _bits(want) != _bits(x)
        res[f"V{V}_B{B}_L{L}_p{pen}_n{ngram}_bad{n_bad}_m{min_new}"] = {
            "bitwise": bool(torch.equal(_bits(got), _bits(want))),
            "untouched_identical": bool(torch.equal(_bits(got)[~touched], _bits(x)[~touched])),
            "edited": int(touched.sum()), "banned": int(torch.isinf(want).sum())}
    return res


# ------------------------------------------------------------------------------------------------ generate level
def golden(model):
    """The micro model against the reference's own generate with processors (tests/golden/generate_processors_micro.npz)."""
    gp = dict(np.load(os.path.join(GOLD, "generate_processors_micro.npz")))
    g = dict(np.load(os.path.join(GOLD, "generate_micro.npz")))
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    N, pad = int(gp["N"]), int(gp["pad"])
    out = {}
    tags = sorted({k.split(".")[0] for k in gp if "." in k})
    for tag in tags:
        kw = json.loads(str(gp[tag + ".kw"]))
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N,
                           return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
        want = gp[tag + ".sequences"]
        sc_w, lg_w = torch.from_numpy(gp[tag + ".scores"]), torch.from_numpy(gp[tag + ".logits"])
        top2 = sc_w.topk(2, dim=-1).values                                    # [n, B, 2]
        margin = (top2[..., 0] - top2[..., 1]).t()                            # [B, n]
        got = o.sequences.cpu().numpy()
        firsts, ok = [], True
        for b in range(want.shape[0]):
            low = (margin[b] <= 0.05).nonzero()
            nb = int(low[0]) if len(low) else want.shape[1]
            firsts.append(nb)
            ok &= got.shape[1] >= nb and np.array_equal(got[b, :nb], want[b, :nb])
        n = min(firsts + [got.shape[1]])
        sc, lg = torch.stack(o.scores[:n]).cpu(), torch.stack(o.logits[:n]).cpu()
        fin_o, fin_w = torch.isfinite(sc), torch.isfinite(sc_w[:n])
        rec = {"ids_ok": bool(ok), "compared_steps": n, "margin_firsts": firsts, "n": int(got.shape[1]), "N_ref": int(want.shape[1]),
               "inf_pattern_equal": bool(torch.equal(fin_o, fin_w)),
               "scores_rel_l2": gsc_rel_l2(torch.where(fin_w, sc, 0.0), torch.where(fin_w, sc_w[:n], 0.0)) if n else 0.0,
               "logits_rel_l2": gsc_rel_l2(lg, lg_w[:n]) if n else 0.0,
               "ids_equal_to_ref": bool(got.shape == want.shape and np.array_equal(got, want))}
        out[tag] = rec
    model._set_logits_processors(None)
    return out


def gsc_rel_l2(a, b) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _eos_for(model, ids, mask, seqs, n):
    """An id that row 0 emits at step 1 of the plain greedy call: banned there while min_new_tokens holds."""
    plain = gsc._gen(model, ids, mask, seqs, n).cpu()
    return [int(plain[0, 1])], plain


def big(model, dev, B: int = 64, max_new: int = 16, sampling: bool = True):
    """Llama-3-8B shape: greedy ids against argmax(restatement(out.logits)); sampled scores' finite pattern against the warpers
    after the restatement, every draw finite there; token_logprobs against fp64 log_softmax of the raw logits, with the number
    of positions whose chosen id a penalty had changed (a looping row under penalty 0.8)."""
    import oracle.sampling as osamp
    cfg = model.cfg
    ids, mask, seqs = gsc.batch(cfg, B)
    eos, plain = _eos_for(model, ids, mask, seqs, max_new)
    res = {}
    modes = [("greedy", None, 1.3), ("greedy_p08", None, 0.8)]
    if sampling:
        modes += [(f"T{s['temperature']}_p{s['top_p']}", s, 1.3) for s in gsc.SAMPLING]
    for mode, samp, pen in modes:
        setting = dict(repetition_penalty=pen, no_repeat_ngram_size=3, bad_words_ids=BAD, min_new_tokens=4)
        o = gsc._gen(model, ids, mask, seqs, max_new, samp, output_scores=True, output_logits=True, output_token_logprobs=True,
                     eos_token_id=eos, **setting)
        seq = o.sequences.cpu()
        n = seq.shape[1]
        cnt = o.n_tokens.cpu()
        mism, argmax_bad, near, drawn_inf, edited, lp_worst, kept, total = 0, 0, 0, 0, 0, 0.0, 0, 0
        for t in range(n):
            raw = o.logits[t].cpu()
            live = t < cnt                                                     # rows still generating at step t
            proc = lpr.process(raw, seq[:, :t], eos=eos, penalty=pen, ngram=3, bad=BAD, min_new=4)
            lsm = torch.log_softmax(raw.double(), dim=-1)
            tok = seq[:, t]
            lp = o.token_logprobs[:, t].double().cpu()
            ref = lsm.gather(1, tok[:, None]).squeeze(1)
            if live.any():
                lp_worst = max(lp_worst, float((lp - ref)[live].abs().max()))
            for b in range(B):
                if live[b] and int(tok[b]) in seq[b, :t].tolist() and pen != 1.0:
                    edited += 1
            if samp is None:
                am = torch.from_numpy(np.argmax(proc.numpy(), axis=1))         # first index among ties
                argmax_bad += int((am != tok)[live].sum())
                mism += int((_bits(o.scores[t]) != _bits(proc))[live].any(dim=1).sum())
            else:
                T = samp["temperature"]
                ours = o.scores[t].cpu()
                want = osamp._warp(proc / T, samp["top_p"], samp["top_k"])
                fo, fw = torch.isfinite(ours), torch.isfinite(want)
                bad = (fo ^ fw) & live[:, None]
                total += int(fo[live].numel())
                kept += int(fo[live].sum())
                if bad.any():
                    p = torch.exp(proc / T - (proc / T).max(dim=1, keepdim=True).values).double()
                    thr = torch.where(fw, p, torch.full_like(p, 2.0)).min(dim=1, keepdim=True).values
                    close = (p - thr).abs() <= 1e-6 * thr
                    mism += int(bad.sum())
                    near += int((bad & close).sum())
                fin_tok = torch.isfinite(ours.gather(1, tok[:, None])).squeeze(1)
                drawn_inf += int((~fin_tok & live).sum())
        res[mode] = {"n": n, "argmax_mismatch": argmax_bad, "scores_mismatch": mism, "mismatch_near_threshold": near,
                     "drawn_not_finite": drawn_inf, "lp_abs": lp_worst, "edited_chosen": edited,
                     "kept_fraction": kept / max(1, total), "differs_from_plain": bool(not torch.equal(seq, plain[:, :n]))
                     if seq.shape == plain[:, :n].shape else True}
    model._set_logits_processors(None)
    return res


def _ids(model, ids, mask, seqs, max_new, **proc):
    """The plain ids of a greedy call with the given processor options."""
    return model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=max_new, **proc).cpu()


def graphs(model, dev, B: int = 64, max_new: int = 16):
    """A plain call before and after processor calls: same ids, its own graph replayed; two processor calls that differ only in
    their values: no new graph; timing mode with processors off: no launch of the new class, on: one per step."""
    cfg = model.cfg
    ids, mask, seqs = gsc.batch(cfg, B, seed=1)
    out = {}
    p0 = _ids(model, ids, mask, seqs, max_new)
    i0 = model.stat("graph_instantiations")
    a = _ids(model, ids, mask, seqs, max_new, repetition_penalty=1.2, no_repeat_ngram_size=3,
             bad_words_ids=[[int(p0[0, 0])]])                     # (row 0's first plain id is banned: its ids must change)
    i1 = model.stat("graph_instantiations")
    b = _ids(model, ids, mask, seqs, max_new, repetition_penalty=0.9, no_repeat_ngram_size=2, bad_words_ids=[[7], [8, 9]])
    i2 = model.stat("graph_instantiations")
    r0 = model.stat("graph_replays")
    p1 = _ids(model, ids, mask, seqs, max_new)
    i3, r1 = model.stat("graph_instantiations"), model.stat("graph_replays")
    out.update(plain_equal=bool(torch.equal(p0, p1)), proc_graphs_first=i1 - i0, proc_graphs_second=i2 - i1,
               plain_new_graphs=i3 - i2, plain_replays=r1 - r0, proc_changed_ids=bool(not torch.equal(a, p0)),
               values_changed_ids=bool(not torch.equal(a, b)))
    model.timing(True)
    _ids(model, ids, mask, seqs, 4)
    off = model.timing_get("logitproc")
    model.timing(True)
    _ids(model, ids, mask, seqs, 4, repetition_penalty=1.2)
    on = model.timing_get("logitproc")
    model.timing(False)
    out.update(timing_off_launches=int(off[1]), timing_on_launches=int(on[1]), timing_on_ms=float(on[0]))
    model._set_logits_processors(None)
    return out


def early_stop(model, gold_micro):
    """EOS with min_new_tokens on: the call still stops within 2 steps of the last row's end (decode_steps)."""
    g = gold_micro
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    ids, mask, pad = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), int(g["pad"])
    free = torch.from_numpy(g["free_ids"])
    eos = sorted(set(int(t) for t in free[:, 4]))
    res = {}
    for attempt in range(2):
        n0 = model.stat("decode_steps")
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, eos_token_id=eos, do_sample=False, max_new_tokens=12,
                           min_new_tokens=2, repetition_penalty=1.05)
        steps = model.stat("decode_steps") - n0
        res[f"call{attempt}"] = {"n": int(o.shape[1]), "decode_steps": int(steps)}
    model._set_logits_processors(None)
    return res
