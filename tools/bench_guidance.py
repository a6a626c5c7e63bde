#!/usr/bin/env python3
"""Classifier-free guidance (generate(guidance_scale=g)) at the Llama-3-8B shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 512-residue proteins, an 89-id prompt, greedy, 32 new tokens, no EOS id (every
step runs), through the product entry point model.generate(ids, seq=list[str], ...).  Settings, run in alternation in one
process (round r runs each once, in order):
  plain64   the plain call on 64 prompts (64 decoder rows, 64 proteins encoded)
  guided32  guidance_scale=1.5 on the first 32 prompts against their protein-free twins (64 decoder rows, 32 proteins encoded)
  plain32   the plain call on those 32 prompts: what the guided call's answers cost without guidance
Per setting the median and spread of the call's ms; the guided call against both plain calls.  Then the guidance launches' own
time per step from timing mode (class "guidance": log-sum-exp partial and final, combine, partner token), once per round, beside
the estimate from its bytes: 20 P V bytes at 5.5 TB/s plus four launches of 1.56 us.  It reports and sets no gate.
Prints ONE JSON line and writes it to profiles/guidance_bench.json.  bench.py is not involved and its line does not change.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "guidance_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    P, N = args.prompts, args.new_tokens
    B = 2 * P
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=N)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    seqs = [synth.synth_protein(args.residues, i) for i in range(B)]
    ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(B)])
    mask = torch.ones_like(ids, dtype=torch.bool)
    settings = {"plain64": (B, {}), "guided32": (P, dict(guidance_scale=args.scale)), "plain32": (P, {})}

    def call(n, kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = model.generate(ids[:n], seqs[:n], attention_mask=mask[:n], pad_token_id=0, eos_token_id=None, max_new_tokens=N,
                             do_sample=False, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    V = cfg.dec_vocab
    res = {"shape": "llama3_8b", "prompts": P, "decoder_rows": B, "residues": args.residues, "new_tokens": N, "rounds": args.rounds,
           "guidance_scale": args.scale, "entry": "model.generate(ids, seq=list[str], ...)", "order": list(settings),
           "estimate_us_per_step": 20.0 * P * V / 5.5e12 * 1e6 + 4 * 1.56}
    ms = {k: [] for k in settings}
    kernel_us, outs = [], {}
    launches = 0
    for r in range(args.warmup + args.rounds):
        for name, (n, kw) in settings.items():
            t, out = call(n, kw)
            outs[name] = out.cpu()
            if r >= args.warmup:
                ms[name].append(t)
        if r >= args.warmup:                     # the launches' own time: timing mode runs the decode eagerly, every launch recorded
            model.timing(True)
            call(P, settings["guided32"][1])
            k_ms, k_n = model.timing_get("guidance")[:2]
            model.timing(False)
            kernel_us.append(1e3 * k_ms / N)
            launches = int(k_n)
        torch.cuda.empty_cache()
    for name in settings:
        med = statistics.median(ms[name])
        res[name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]), "answers_per_sec": settings[name][0] * 1e3 / med}
    res["guided32"].update(
        vs_plain64_ms_median=statistics.median(a - b for a, b in zip(ms["guided32"], ms["plain64"])),
        vs_plain64_rel=statistics.median(ms["guided32"]) / statistics.median(ms["plain64"]),
        vs_plain32_rel=statistics.median(ms["guided32"]) / statistics.median(ms["plain32"]),
        differs_from_plain32=not torch.equal(outs["guided32"], outs["plain32"]))
    res["kernel"] = {"launches_per_call": launches, "us_per_step_median": statistics.median(kernel_us), "us_per_step_min": min(kernel_us),
                     "us_per_step_max": max(kernel_us)}
    model.timing(True)
    call(P, {})
    res["launches_when_off"] = int(model.timing_get("guidance")[1])
    model.timing(False)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
