#!/usr/bin/env python3
"""generate()'s logits processors at the headline shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, batch 64 x 512-residue proteins, an 89-id prompt, 32 new tokens, through the
product entry point model.generate(ids, seq=list[str], ...).  Greedy and the reference's sampling mode (temperature 0.1, top_p 0.7,
top_k 50).  One EOS id that the rows do not emit (so that min_new_tokens has an id to ban and every step runs) in every setting.
Settings, run in alternation in one process (round r runs each once, in order):
  off          no processor (the plain decode graph)
  on           repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4
  on_logprobs  the same + output_token_logprobs (the raw rows' log-sum-exp is one more pass over the logits)
Per setting: the median and spread of the call's ms, proteins/s, the median overhead against `off` of the same rounds per call
and per decode step.  Then the processor kernel's own time per step from timing mode (class "logitproc").  Prints ONE JSON line
and writes it to profiles/logits_proc_bench.json.  bench.py is not involved and its line does not change.
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

ON = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4)
SETTINGS = {"off": {}, "on": ON, "on_logprobs": dict(ON, return_dict_in_generate=True, output_token_logprobs=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new_tokens", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "logits_proc_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    B, N = args.batch, args.new_tokens
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=N)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    seqs = [synth.synth_protein(args.residues, i) for i in range(B)]
    ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(B)])
    mask = torch.ones_like(ids, dtype=torch.bool)
    modes = {"greedy": dict(do_sample=False), "sample_T0.1_p0.7_k50": dict(do_sample=True, temperature=0.1, top_p=0.7, top_k=50, seed=5)}
    eos = [cfg.dec_vocab - 1]

    def call(mode, kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = model.generate(ids, seqs, attention_mask=mask, pad_token_id=0, eos_token_id=eos, max_new_tokens=N, **modes[mode], **kw)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3
        seq = out if isinstance(out, torch.Tensor) else out.sequences
        return ms, seq

    res = {"shape": "llama3_8b", "batch": B, "residues": args.residues, "new_tokens": N, "rounds": args.rounds,
           "entry": "model.generate(ids, seq=list[str], ...)", "on": ON, "order": list(SETTINGS)}
    for mode in modes:
        ms = {k: [] for k in SETTINGS}
        steps = {}
        same_on = True
        for r in range(args.warmup + args.rounds):
            ref_on = None
            for name, kw in SETTINGS.items():
                t, seq = call(mode, kw)
                steps[name] = int(seq.shape[1])
                if name != "off":
                    ref_on = seq if ref_on is None else ref_on
                    same_on &= bool(torch.equal(seq, ref_on))
                if r >= args.warmup:
                    ms[name].append(t)
            torch.cuda.empty_cache()
        m = {}
        for name in SETTINGS:
            med = statistics.median(ms[name])
            m[name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]), "proteins_per_sec": B * 1e3 / med,
                       "steps": steps[name]}
            if name != "off":
                d = [a - b for a, b in zip(ms[name], ms["off"])]
                m[name]["overhead_ms_median"] = statistics.median(d)
                m[name]["overhead_ms_per_step"] = statistics.median(d) / N
                m[name]["overhead_rel"] = statistics.median(d) / m["off"]["ms_median"]
        m["ids_equal_on_vs_on_logprobs"] = same_on
        # the kernel's own time: timing mode runs the decode eagerly and records every launch
        model.timing(True)
        call(mode, ON)
        k_ms, k_n = model.timing_get("logitproc")[:2]
        model.timing(True)
        call(mode, {})
        off_n = model.timing_get("logitproc")[1]
        model.timing(False)
        m["kernel"] = {"launches": int(k_n), "us_per_step": 1e3 * k_ms / max(1, k_n), "launches_when_off": int(off_n)}
        res[mode] = m
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
