"""Checks of generate(return_dict_in_generate=True, output_*=True) shared by tests/test_gpu_gen_scores.py (fp16-operand build)
and its bf16 child process (tests/bf16_gen_scores_check.py).  Each returns a dict of observations; the callers assert the
bounds.  Test infrastructure, not product code."""
from __future__ import annotations


import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth

SAMPLING = [dict(temperature=0.1, top_p=0.7, top_k=50),          # the reference's sampling mode (transformers 4.46.3's top_k)
            dict(temperature=1.0, top_p=0.9, top_k=50)]          # wider kept sets


def llama8b_shape(B: int = 64, layers: int = 2, max_new: int = 8):
    """Llama-3-8B's decoder shape (vocab 128 256, dim 4096, GQA 32 / 8) with a micro encoder: the sizes the output kernels see."""
    return opa.OpusConfig(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=256, proj_dim=64,
                          dec_layers=layers, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                          dec_vocab=128256, dec_rope_theta=500000.0, max_batch=B, max_enc_tokens=66, max_prompt=48,
                          max_new_tokens=max_new).validate()


def make_model(cfg, dev, seed: int = 0):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    return OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev), dev)


def batch(cfg, B: int, seed: int = 0):
    """B left-padded prompts (pad 2) with one protein each."""
    seqs = [synth.synth_protein(12 + (7 * i + seed) % 40, 100 * seed + i) for i in range(B)]
    rows = [synth.synth_prompt_ids(cfg.dec_vocab, 1000 * seed + i, n_text=6 + (5 * i) % 11, seq_pos=2) for i in range(B)]
    width = max(len(r) for r in rows)
    ids = torch.full((B, width), 2, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.tensor(r)
    return ids, ids != 2, seqs


# ------------------------------------------------------------------------------------------------ kernel level
def argmax_lse_cases(dev):
    """(name, logits [B, V] fp32 on dev, row offset in floats): the vocabularies of the micro model, Llama-3 and Qwen2, a V that is
    not a multiple of 4, a misaligned first row, ties for the maximum, -inf entries and values around +-1e4."""
    g = torch.Generator(device="cpu").manual_seed(3)
    out = []
    for V in (96, 128256, 152064, 1001):
        out.append((f"V{V}", torch.randn(6, V, generator=g) * 4, 0))
    x = torch.randn(5, 128256, generator=g) * 3
    out.append(("misaligned", x, 1))                       # row 0 starts one float past a 16-byte boundary
    t = torch.randn(6, 4099, generator=g)
    for b in range(6):                                     # ties: the maximum at several indices, across parts and inside one
        t[b, [7 + b, 2000, 2001, 4098 - b]] = 9.0
    out.append(("ties", t, 0))
    n = torch.randn(4, 128256, generator=g) * 5
    n[torch.rand(4, 128256, generator=g) < 0.3] = float("-inf")
    n[2, :70000] = float("-inf")                           # whole parts without a finite value
    out.append(("neg_inf", n, 0))
    big = torch.randn(4, 152064, generator=g) * 1e4
    big[1] = 1e4 + torch.randn(152064, generator=g)        # everything near +1e4
    big[3] = -1e4 + torch.randn(152064, generator=g)       # everything near -1e4
    out.append(("pm1e4", big, 0))
    return [(nm, x.to(dev), off) for nm, x, off in out]


def argmax_lse_kernel(model, dev):
    lib = _cabi.lib()
    res = {}
    s = torch.cuda.current_stream(dev)
    for name, x, off in argmax_lse_cases(dev):
        B, V = x.shape
        buf = torch.empty(B * V + 8, dtype=torch.float32, device=dev)
        buf[off: off + B * V] = x.reshape(-1)
        idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
        lse = torch.empty((B,), dtype=torch.float32, device=dev)
        _cabi.check(lib.opus_debug_argmax_lse(model._ctx, buf.data_ptr() + 4 * off, B, V, idx.data_ptr(), lse.data_ptr(), s.cuda_stream))
        torch.cuda.synchronize(dev)
        xd = x.double().cpu()
        ref_lse = torch.logsumexp(xd, dim=1)
        ref_idx = torch.from_numpy(np.argmax(x.cpu().numpy(), axis=1))      # first index among ties, as torch.argmax's contract
        err = ((lse.double().cpu() - ref_lse).abs() / ref_lse.abs().clamp_min(1.0)).max().item()
        res[name] = {"idx_bitwise": bool(torch.equal(idx.long().cpu(), ref_idx.long())), "lse_rel": err}
    return res


# ------------------------------------------------------------------------------------------------ generate level
def _gen(model, ids, mask, seqs, max_new, sampling=None, seed=11, **flags):
    kw = dict(attention_mask=mask, pad_token_id=2, max_new_tokens=max_new)
    if sampling:
        kw.update(do_sample=True, seed=seed, **sampling)
    if flags:
        kw["return_dict_in_generate"] = True
        kw.update(flags)
    return model.generate(ids, seqs, **kw)


def self_consistency(model, dev, B: int, max_new: int):
    """token_logprobs against log_softmax(out.logits[t])[tok] in fp64, compute_transition_scores on the logits, ids bitwise equal
    for every combination of flags, a plain call after flagged calls still replaying its own graph; sampled scores against the
    oracle's warpers.  Greedy and the SAMPLING settings."""
    import oracle.sampling as osamp
    cfg = model.cfg
    ids, mask, seqs = batch(cfg, B)
    res = {}
    for mode, samp in [("greedy", None)] + [(f"T{s['temperature']}_p{s['top_p']}", s) for s in SAMPLING]:
        plain = _gen(model, ids, mask, seqs, max_new, samp).cpu()
        inst0 = model.stat("graph_instantiations")
        o = _gen(model, ids, mask, seqs, max_new, samp, output_scores=True, output_logits=True, output_token_logprobs=True)
        same = bool(torch.equal(o.sequences.cpu(), plain))
        # a plain call after the flagged one replays its own graph (the context keeps 4: checked before the other combinations)
        r0, i0 = model.stat("graph_replays"), model.stat("graph_instantiations")
        again = _gen(model, ids, mask, seqs, max_new, samp).cpu()
        r1, i1 = model.stat("graph_replays"), model.stat("graph_instantiations")
        for fl in (dict(output_token_logprobs=True), dict(output_scores=True), dict(output_logits=True),
                   dict(output_scores=True, output_logits=True)):
            same &= bool(torch.equal(_gen(model, ids, mask, seqs, max_new, samp, **fl).sequences.cpu(), plain))
        n = o.sequences.shape[1]
        lg = torch.stack(o.logits).double()                                     # [n, B, V]
        lsm = torch.log_softmax(lg, dim=-1)
        seq = o.sequences
        ref = lsm.gather(2, seq.t().unsqueeze(-1)).squeeze(-1).t()             # [B, n]
        cnt = o.n_tokens.cpu()
        counted = torch.arange(n)[None, :] < cnt[:, None]
        lp = o.token_logprobs.double().cpu()
        ref = ref.cpu()
        tr = model.compute_transition_scores(seq, o.logits, normalize_logits=True).double().cpu()
        rec = {"n": n, "ids_equal_all_flags": same and bool(torch.equal(again, plain)),
               "flagged_graphs": i0 - inst0, "plain_replays": r1 - r0, "plain_new_graphs": i1 - i0,
               "lp_abs": float((lp - ref)[counted].abs().max()) if counted.any() else 0.0,
               "transition_abs": float((tr - ref)[counted].abs().max()) if counted.any() else 0.0,
               "zero_after_end": bool((lp[~counted] == 0).all()),
               "logprob_sum_abs": float((o.logprob.double().cpu() - lp.sum(1)).abs().max()),
               "len_scores": len(o.scores), "len_logits": len(o.logits), "scores_is_logits": o.scores[0] is o.logits[0]}
        if samp:
            T = samp["temperature"]
            mism = near = drawn_finite = total = kept = 0
            for t in range(n):
                raw = o.logits[t].float()
                ours = o.scores[t]
                want = osamp._warp(raw / T, samp["top_p"], samp["top_k"])
                fo, fw = torch.isfinite(ours), torch.isfinite(want)
                bad = fo ^ fw
                total += fo.numel()
                kept += int(fo.sum())
                # finite entries hold l / T
                if fo.any():
                    d = ((ours[fo].double() - raw[fo].double() / T).abs() / (raw[fo].double() / T).abs().clamp_min(1e-30)).max()
                    rec["scores_value_rel"] = max(rec.get("scores_value_rel", 0.0), float(d))
                if bad.any():
                    # tempered probability p = exp(l / T - max / T) and the row's threshold: the smallest p the oracle keeps
                    p = torch.exp(raw / T - (raw / T).max(dim=1, keepdim=True).values).double()
                    thr = torch.where(fw, p, torch.full_like(p, 2.0)).min(dim=1, keepdim=True).values
                    close = (p - thr).abs() <= 1e-6 * thr
                    mism += int(bad.sum())
                    near += int((bad & close).sum())
                tok = seq[:, t]
                fin_row = torch.isfinite(ours.gather(1, tok[:, None])).squeeze(1)
                drawn_finite += int((fin_row | ~counted[:, t].to(dev)).all())
            rec.update(filter_mismatch=mism, filter_mismatch_near_threshold=near, drawn_finite_steps=drawn_finite,
                       kept_fraction=kept / max(1, total))
        res[mode] = rec
    return res


def ragged(model, dev, gold):
    """Rows finishing at different steps (several EOS ids, then a stop sequence): token_logprobs 0 after each row's end, n_tokens
    and logprob consistent, one score tensor per returned position, the batch cut where it stopped."""
    import json
    import os
    g = gold
    ids, mask, pad = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), int(g["pad"])
    seqs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_micro.seqs.json")))
    free = torch.from_numpy(g["free_ids"])
    N = free.shape[1]
    out = {}
    cases = {"eos": dict(eos_token_id=[int(free[0, 3]), int(free[1, 4]), int(free[2, 5])]),
             "stop": dict(stop_sequence=[int(free[0, 1]), int(free[0, 2])], eos_token_id=[int(free[2, 6])])}
    for tag, kw in cases.items():
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N,
                           return_dict_in_generate=True, output_token_logprobs=True, output_scores=True, **kw)
        plain = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, **kw)
        n = o.sequences.shape[1]
        lp = o.token_logprobs.cpu()
        cnt = o.n_tokens.cpu()
        pos = torch.arange(n)[None, :]
        out[tag] = {"n": n, "N": N, "n_tokens": cnt.tolist(), "ids_equal": bool(torch.equal(o.sequences, plain)),
                    "len_scores": len(o.scores),
                    "zero_after_end": bool((lp[pos >= cnt[:, None]] == 0).all()),
                    "nonzero_counted": bool((lp[pos < cnt[:, None]] != 0).all()),
                    "logprob_ok": bool(torch.allclose(o.logprob.cpu(), lp.sum(1))),
                    "ragged": len(set(cnt.tolist())) > 1}
    model.set_stop_sequence(None)
    return out
