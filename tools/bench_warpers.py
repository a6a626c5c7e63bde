#!/usr/bin/env python3
"""generate(do_sample=True)'s truncation warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) at the headline shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 512-residue proteins, an 89-id prompt, 32 new tokens, through the product entry
point model.generate(ids, seq=list[str], ...), at batch 64 and at batch 1.  The reference's sampling mode (temperature 0.1,
top_p 0.7, top_k 50) and, because that mode leaves the warpers a handful of candidates, a wide mode (temperature 1, top_p 1,
top_k 0: every token is a candidate).  Settings, run in alternation in one process (a round runs each once, in order):
  plain   the sampled call without the arguments (the plain decode graph)
  min_p   min_p=0.05
  all4    min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4
The decode phase of a call is its time minus the time of the same call with max_new_tokens=1 (encoder, projector, prefill and the
first token's head are the same work).  Per setting: the median of the rounds' decode ms, the plain call's own spread (min, max),
the median overhead against `plain` of the same rounds per call and per decode step.  Prints ONE JSON line and writes it to
profiles/warpers_bench.json (an existing "headline_ab" entry of that file is kept).  bench.py is not involved.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"plain": {}, "min_p": dict(min_p=0.05), "all4": dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4)}
MODES = {"sample_T0.1_p0.7_k50": dict(temperature=0.1, top_p=0.7, top_k=50), "sample_T1_p1_k0": dict(temperature=1.0, top_p=1.0, top_k=0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new_tokens", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "warpers_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    N = args.new_tokens
    res = {"shape": "llama3_8b", "residues": args.residues, "new_tokens": N, "rounds": args.rounds, "settings": SETTINGS,
           "entry": "model.generate(ids, seq=list[str], do_sample=True, ...)", "decode_ms": "call(max_new_tokens=N) - call(max_new_tokens=1)"}
    cfg = opa.llama3_8b(max_batch=max(args.batches), max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=N)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    for B in args.batches:
        seqs = [synth.synth_protein(args.residues, i) for i in range(B)]
        ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(B)])
        mask = torch.ones_like(ids, dtype=torch.bool)

        def call(mode, kw, n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            model.generate(ids, seqs, attention_mask=mask, pad_token_id=0, eos_token_id=[], max_new_tokens=n, do_sample=True, seed=5,
                           **MODES[mode], **kw)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3

        per_batch = {}
        for mode in MODES:
            dec = {k: [] for k in SETTINGS}
            for r in range(args.warmup + args.rounds):
                for name, kw in SETTINGS.items():
                    d = call(mode, kw, N) - call(mode, kw, 1)
                    if r >= args.warmup:
                        dec[name].append(d)
            m = {}
            for name in SETTINGS:
                m[name] = {"decode_ms_median": statistics.median(dec[name]), "decode_ms_min": min(dec[name]), "decode_ms_max": max(dec[name])}
                if name != "plain":
                    d = [a - b for a, b in zip(dec[name], dec["plain"])]
                    m[name]["overhead_ms_median"] = statistics.median(d)
                    m[name]["overhead_us_per_step"] = 1e3 * statistics.median(d) / (N - 1)
                    m[name]["overhead_rel"] = statistics.median(d) / m["plain"]["decode_ms_median"]
            m["plain_spread_ms"] = m["plain"]["decode_ms_max"] - m["plain"]["decode_ms_min"]
            per_batch[mode] = m
        res[f"batch{B}"] = per_batch
    if os.path.exists(args.out):                 # (the off-state A/B of bench.py against the parent commit lives in the same file)
        try:
            old = json.load(open(args.out))
            if "headline_ab" in old:
                res["headline_ab"] = old["headline_ab"]
        except ValueError:
            pass
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
