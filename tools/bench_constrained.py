#!/usr/bin/env python3
"""Constrained decoding (generate(prefix_allowed_tokens_fn=TokenTrie)) at the headline shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, batch 64 x 512-residue proteins, an 89-id prompt, greedy, through the product
entry point model.generate(ids, seq=list[str], ...), under a 50 000-member trie with a separator (a list answer, so that rows
have something to follow at every step) and no EOS id (every step runs).  Budgets of 32 and 256 new tokens.  Settings, run in
alternation in one process (round r runs each once, in order):
  off   no constraint (the plain decode graph)
  on    the trie
Per budget and setting: the median and spread of the call's ms, proteins/s, the median overhead against `off` of the same rounds
per call and per decode step.  Then the constraint kernel's own time per step from timing mode (class "constraint"), once per
round, at both budgets: the kernel takes one transition per step and never walks the history, so the two budgets should agree
within the rounds' spread.  Beside it the estimate from its bytes: 4 B V bytes of stores at 5.5 TB/s plus a 1.56 us launch.
Prints ONE JSON line and writes it to profiles/constrained_bench.json.  bench.py is not involved and its line does not change.
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


def members(n, vocab, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for ln in rng.integers(1, 17, size=n):
        out.append([int(1000 + rng.integers(0, 6000))] + [int(t) for t in 7000 + rng.integers(0, 64, size=ln - 1)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--members", type=int, default=50000)
    ap.add_argument("--budgets", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "constrained_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    B = args.batch
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=max(args.budgets))
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    seqs = [synth.synth_protein(args.residues, i) for i in range(B)]
    ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(B)])
    mask = torch.ones_like(ids, dtype=torch.bool)
    t0 = time.perf_counter()
    trie = opa.TokenTrie(members(args.members, cfg.dec_vocab), end_token_id=cfg.dec_vocab - 1, separator=[900, 901])
    tab = trie.compiled()
    build_s = time.perf_counter() - t0
    settings = {"off": {}, "on": dict(prefix_allowed_tokens_fn=trie)}

    def call(N, kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = model.generate(ids, seqs, attention_mask=mask, pad_token_id=0, eos_token_id=None, max_new_tokens=N, do_sample=False, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    V = cfg.dec_vocab
    res = {"shape": "llama3_8b", "batch": B, "residues": args.residues, "rounds": args.rounds, "members": args.members,
           "states": tab.n_states, "edges": tab.n_edges, "root_children": int(tab.edge_off[tab.start[0] + 1] - tab.edge_off[tab.start[0]]),
           "host_build_s": build_s, "entry": "model.generate(ids, seq=list[str], ...)", "order": list(settings),
           "estimate_us_per_step": 4.0 * B * V / 5.5e12 * 1e6 + 1.56}
    for N in args.budgets:
        ms = {k: [] for k in settings}
        kernel_us, on_trie = [], True
        for r in range(args.warmup + args.rounds):
            for name, kw in settings.items():
                t, out = call(N, kw)
                if name == "on" and r == 0:
                    on_trie = all(tab.walk(0, row) != 0 or (V - 1) in row for row in out.cpu().tolist())
                if r >= args.warmup:
                    ms[name].append(t)
            if r >= args.warmup:                 # the kernel's own time: timing mode runs the decode eagerly, every launch recorded
                model.timing(True)
                call(N, settings["on"])
                k_ms, k_n = model.timing_get("constraint")[:2]
                model.timing(False)
                kernel_us.append(1e3 * k_ms / max(1, k_n))
                launches = int(k_n)
            torch.cuda.empty_cache()
        m = {}
        for name in settings:
            med = statistics.median(ms[name])
            m[name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]), "proteins_per_sec": B * 1e3 / med}
        d = [a - b for a, b in zip(ms["on"], ms["off"])]
        m["on"].update(overhead_ms_median=statistics.median(d), overhead_us_per_step=1e3 * statistics.median(d) / N,
                       overhead_rel=statistics.median(d) / m["off"]["ms_median"], rows_on_trie=on_trie)
        m["kernel"] = {"launches": launches, "us_per_step_median": statistics.median(kernel_us), "us_per_step_min": min(kernel_us),
                       "us_per_step_max": max(kernel_us)}
        res[f"new_tokens_{N}"] = m
    model.timing(True)
    call(4, {})
    res["launches_when_off"] = int(model.timing_get("constraint")[1])
    model.timing(False)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
