#!/usr/bin/env python3
"""N answers per protein: generate(num_return_sequences=5) against the same 60 decoder rows as repeated prompts, on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 512-residue proteins, an 89-id prompt, the reference's sampling mode (temperature
0.1, top_p 0.7, top_k 50; eval/eval_total_ablation.sh samples every dataset five times), no EOS (every step runs), 32 new tokens
and again 128, through the product entry point model.generate(ids, seq=list[str], ...).  Two calls, run in alternation in one
process (round r runs each once, in order):
  nsample    12 prompts, num_return_sequences=5: one encode, one projector pass and one 12-row prefill, then 60 decoder rows
  repeated   the same 12 prompts repeated 5 times each as a 60-row batch through the call without the argument: 60 proteins
             encoded, 60 rows prefilled.  It uses nothing this change adds, so `--tree <a checkout of the parent commit> --mode
             repeated` measures the parent's library with this script.
Prints ONE JSON line and writes it to --out (default profiles/nsamples_bench.json).

A/B across commits: run this script several times per tree in alternation (this tree, the parent's, this tree, ...; a fresh process
each), every run with its own --out and a --label, then `--merge run1.json run2.json ...` writes the line that holds, per label,
call and token count, the median over the runs' medians with the runs' values beside it.  bench.py is not involved and its line
does not change.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = dict(do_sample=True, temperature=0.1, top_p=0.7, top_k=50)


def merge(files, out):
    runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]
    res = {k: runs[0][k] for k in ("shape", "prompts", "num_return_sequences", "rows", "residues", "sampling", "entry")}
    res["runs_in_order"] = [r["label"] for r in runs]
    table = {}
    for r in runs:
        for nt, calls in r["new_tokens"].items():
            for call, m in calls.items():
                table.setdefault(r["label"], {}).setdefault(nt, {}).setdefault(call, []).append(m["ms_median"])
    res["ms"] = {lab: {nt: {call: {"median_of_runs": statistics.median(v), "runs": v} for call, v in calls.items()}
                       for nt, calls in nts.items()} for lab, nts in table.items()}
    line = json.dumps(res)
    print(line)
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompts", type=int, default=12)
    ap.add_argument("--num_return_sequences", type=int, default=5)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new_tokens", type=str, default="32,128")
    ap.add_argument("--mode", choices=["both", "nsample", "repeated"], default="both")
    ap.add_argument("--tree", type=str, default=ROOT, help="checkout whose package (and built library) is measured")
    ap.add_argument("--label", type=str, default="this")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nsamples_bench.json"))
    ap.add_argument("--merge", nargs="+", default=None, metavar="RUN.json")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    P, N = args.prompts, args.num_return_sequences
    budgets = [int(v) for v in args.new_tokens.split(",")]
    cfg = opa.llama3_8b(max_batch=P * N, max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=max(budgets))
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    seqs = [synth.synth_protein(args.residues, i) for i in range(P)]
    ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(P)])
    mask = torch.ones_like(ids, dtype=torch.bool)
    ids_rep, mask_rep = ids.repeat_interleave(N, dim=0), mask.repeat_interleave(N, dim=0)
    seqs_rep = [s for s in seqs for _ in range(N)]
    calls = [c for c in ("nsample", "repeated") if args.mode in ("both", c)]

    def call(name, new_tokens):
        kw = dict(pad_token_id=0, eos_token_id=[], max_new_tokens=new_tokens, seed=5, **MODE)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if name == "nsample":
            out = model.generate(ids, seqs, attention_mask=mask, num_return_sequences=N, **kw)
        else:
            out = model.generate(ids_rep, seqs_rep, attention_mask=mask_rep, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    res = {"shape": "llama3_8b", "prompts": P, "num_return_sequences": N, "rows": P * N, "residues": args.residues,
           "sampling": MODE, "rounds": args.rounds, "label": args.label, "order": calls,
           "entry": "model.generate(ids, seq=list[str], ...)", "new_tokens": {}}
    for nt in budgets:
        ms = {c: [] for c in calls}
        same = True
        for r in range(args.warmup + args.rounds):
            outs = {}
            for c in calls:
                t, outs[c] = call(c, nt)
                if r >= args.warmup:
                    ms[c].append(t)
            if len(outs) == 2:      # the same rows, seed and draws: the ids differ only where the two prefills' logits round apart
                same &= outs["nsample"].shape == outs["repeated"].shape
        m = {c: {"ms_median": statistics.median(ms[c]), "ms_min": min(ms[c]), "ms_max": max(ms[c]),
                 "answers_per_sec": P * N * 1e3 / statistics.median(ms[c])} for c in calls}
        if len(calls) == 2:
            d = [a - b for a, b in zip(ms["nsample"], ms["repeated"])]
            m["nsample"]["saving_ms_median"] = -statistics.median(d)
            m["nsample"]["saving_rel"] = -statistics.median(d) / m["repeated"]["ms_median"]
            m["nsample"]["shapes_equal"] = bool(same)
        res["new_tokens"][str(nt)] = m
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
