#!/usr/bin/env python3
"""generate(top_logprobs=k) at the headline shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 512-residue proteins, an 89-id prompt, 32 new tokens, through the product entry
point model.generate(ids, seq=list[str], return_dict_in_generate=True, ...), at batch 64 and at batch 1, greedy and the reference's
sampling mode (temperature 0.1, top_p 0.7, top_k 50).  Variants, run in alternation in one process (a round runs each once, in
order):
  off          the call without the argument (the plain decode graph)
  k5, k20      top_logprobs=5 / 20
  logits_topk  the route there was before: output_logits=True, then log_softmax and torch.topk(5) over the stacked [n, B, V] logits
The decode phase of a call is its time minus the time of the same call with max_new_tokens=1 (encoder, projector, prefill and the
first token's head are the same work).  Per variant: the median of the rounds' decode ms, the off-variant's own spread (min, max),
the median overhead against `off` of the same rounds per call and per decode step.  Then the two selection launches' own time per
step from timing mode (class "topk": both stages of a step are one record).  Prints ONE JSON line and writes it to
profiles/top_logprobs_bench.json (existing "headline_ab" and "forward_paths" entries of that file are kept).  bench.py is not involved.
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

VARIANTS = ("off", "k5", "k20", "logits_topk")
MODES = {"greedy": {}, "sample_T0.1_p0.7_k50": dict(do_sample=True, seed=5, temperature=0.1, top_p=0.7, top_k=50)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new_tokens", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "top_logprobs_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    N = args.new_tokens
    res = {"shape": "llama3_8b", "residues": args.residues, "new_tokens": N, "rounds": args.rounds, "variants": list(VARIANTS),
           "entry": "model.generate(ids, seq=list[str], return_dict_in_generate=True, ...)",
           "decode_ms": "call(max_new_tokens=N) - call(max_new_tokens=1)"}
    cfg = opa.llama3_8b(max_batch=max(args.batches), max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=N)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    for B in args.batches:
        seqs = [synth.synth_protein(args.residues, i) for i in range(B)]
        ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(B)])
        mask = torch.ones_like(ids, dtype=torch.bool)

        def run(mode, variant, n):
            kw = dict(attention_mask=mask, pad_token_id=0, eos_token_id=[], max_new_tokens=n, return_dict_in_generate=True, **MODES[mode])
            if variant == "k5":
                return model.generate(ids, seqs, top_logprobs=5, **kw)
            if variant == "k20":
                return model.generate(ids, seqs, top_logprobs=20, **kw)
            if variant == "logits_topk":
                o = model.generate(ids, seqs, output_logits=True, **kw)
                lsm = torch.log_softmax(torch.stack(o.logits), dim=-1)
                o.top_logprobs, o.top_ids = torch.topk(lsm, 5, dim=-1)
                return o
            return model.generate(ids, seqs, **kw)

        def call(mode, variant, n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(mode, variant, n)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3

        per_batch = {}
        for mode in MODES:
            dec = {v: [] for v in VARIANTS}
            for r in range(args.warmup + args.rounds):
                for v in VARIANTS:
                    d = call(mode, v, N) - call(mode, v, 1)
                    if r >= args.warmup:
                        dec[v].append(d)
            m = {}
            for v in VARIANTS:
                m[v] = {"decode_ms_median": statistics.median(dec[v]), "decode_ms_min": min(dec[v]), "decode_ms_max": max(dec[v])}
                if v != "off":
                    d = [a - b for a, b in zip(dec[v], dec["off"])]
                    m[v]["overhead_ms_median"] = statistics.median(d)
                    m[v]["overhead_us_per_step"] = 1e3 * statistics.median(d) / (N - 1)
                    m[v]["overhead_rel"] = statistics.median(d) / m["off"]["decode_ms_median"]
            m["off_spread_ms"] = m["off"]["decode_ms_max"] - m["off"]["decode_ms_min"]
            # the launches' own time: timing mode runs the decode eagerly and records every launch
            kern = {}
            for v in ("off", "k5", "k20"):
                model.timing(True)
                run(mode, v, N)
                k_ms, k_n = model.timing_get("topk")[:2]
                model.timing(False)
                kern[v] = {"records": int(k_n), "us_per_step": 1e3 * k_ms / max(1, k_n)}
            m["kernel_topk_class"] = kern
            per_batch[mode] = m
        res[f"batch{B}"] = per_batch
    if os.path.exists(args.out):                 # (measured elsewhere: bench.py against the parent commit, forward()'s two paths)
        try:
            old = json.load(open(args.out))
            for key in ("headline_ab", "forward_paths"):
                if key in old:
                    res[key] = old[key]
        except ValueError:
            pass
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
