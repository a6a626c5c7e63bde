#!/usr/bin/env python3
"""generate_continuous() against the loop of plain generate() batches at the Llama-3-8B shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 256 prompts of 40 .. 89 ids with one protein each (64 distinct pairs, repeated:
see below), greedy, a budget of 128 new tokens, 64 decode rows, a context whose max_new_tokens capacity (the session's step
budget) is 512.  Two EOS settings:
  spread   up to 64 EOS ids picked from the ids a free run emits, at hashed target lengths: answers of widely different lengths
  full     no EOS id: every answer takes the whole budget (equal lengths: the refill can gain nothing and pays for its prefills)
Per setting, run in alternation in one process (round r runs each once, in order): `continuous` = one generate_continuous call,
`plain` = generate() on batches of 64 in input order (the batched loop of eval_ddp.py).  Reports wall time and answers/s of both,
the length distribution, the occupancy of both (ids returned / row-steps decoded) and the refill count.  It reports and sets no
gate.  Prints ONE JSON line and writes it to profiles/continuous_bench.json.  bench.py is not involved.
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--residues", type=int, default=256)
    ap.add_argument("--refill-min", type=int, default=None)
    ap.add_argument("--distinct", type=int, default=64, help="distinct (prompt, protein) pairs the dataset repeats")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "continuous_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    N, B, M, S = args.prompts, args.slots, args.new_tokens, args.capacity
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=S)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    # An EOS id ends the rows that emit it, and a call takes at most 64 EOS ids: with 128 256 ids in the vocabulary 64 of them reach
    # about 64 rows.  The dataset therefore repeats `distinct` (item, protein) pairs, item i = pair i % distinct, so that every EOS
    # id shapes the length of N / distinct rows and every plain batch of 64 holds the whole range of lengths.
    D = min(args.distinct, N)
    n_text = [40 + int(v) % 50 for v in synth.synth_lengths(D, 0, 1 << 20, seed=11)]
    base = [torch.tensor(synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=n, seq_pos=20)) for i, n in enumerate(n_text)]
    prompts = [base[i % D] for i in range(N)]
    seqs = [synth.synth_protein(args.residues, i % D) for i in range(N)]
    PAD = 0

    def plain(eos):
        rows, row_steps = [], 0
        for b0 in range(0, N, B):
            grp = prompts[b0: b0 + B]
            width = max(len(p) for p in grp)
            ids = torch.full((len(grp), width), PAD, dtype=torch.long)
            mask = torch.zeros((len(grp), width), dtype=torch.bool)
            for i, p in enumerate(grp):
                ids[i, width - len(p):] = p
                mask[i, width - len(p):] = True
            d0 = model.stat("decode_steps")
            out = model.generate(ids, seqs[b0: b0 + B], attention_mask=mask, pad_token_id=PAD, eos_token_id=list(eos),
                                 max_new_tokens=M, do_sample=False).cpu()
            row_steps += len(grp) * (model.stat("decode_steps") - d0 + 1)
            rows.extend(out[i] for i in range(len(grp)))
        return rows, row_steps

    def lengths(rows, eos):
        out = []
        for r in rows:
            hit = [k for k, t in enumerate(r.tolist()) if t in eos]
            out.append(hit[0] + 1 if hit else M)
        return out

    free, _ = plain(())
    free = [torch.cat([r, torch.full((M - len(r),), PAD, dtype=torch.long)]) for r in free]
    targets = [4 + int(v) % (M - 4) for v in synth.synth_lengths(D, 0, 1 << 20, seed=12)]
    spread = sorted({int(free[p][targets[p] - 1]) for p in range(0, D, max(1, D // 64))} - {PAD})[:64]
    settings = {"spread": spread, "full": []}

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    res = {"shape": "llama3_8b", "prompts": N, "distinct_prompts": D, "slots": B, "new_tokens": M, "capacity": S, "residues": args.residues,
           "rounds": args.rounds, "refill_min": args.refill_min, "order": [f"{k}.{w}" for k in settings for w in ("continuous", "plain")]}
    ms = {k: {"continuous": [], "plain": []} for k in settings}
    last = {}
    for r in range(args.warmup + args.rounds):
        for name, eos in settings.items():
            tc, oc = timed(lambda: model.generate_continuous(prompts, seqs, max_new_tokens=M, eos_token_id=list(eos), pad_token_id=PAD,
                                                             slots=B, refill_min=args.refill_min, return_dict_in_generate=True))
            tp, (rows, row_steps) = timed(lambda: plain(eos))
            if r >= args.warmup:
                ms[name]["continuous"].append(tc)
                ms[name]["plain"].append(tp)
            last[name] = (oc, rows, row_steps)
    for name, eos in settings.items():
        oc, rows, row_steps = last[name]
        ln = lengths(rows, set(eos))
        got = [int(x) for x in oc.n_tokens]
        same = sum(1 for p in range(N) if got[p] == ln[p] and torch.equal(oc.sequences[p], rows[p][: ln[p]]))
        q = np.percentile(ln, [0, 10, 25, 50, 75, 90, 100]).tolist()
        out = {"n_eos": len(eos), "lengths": {"mean": float(np.mean(ln)), "percentiles_0_10_25_50_75_90_100": q},
               "answers_identical_to_plain": same, "stats": oc.stats,
               "occupancy_continuous": oc.stats["live_row_steps"] / max(oc.stats["slot_steps"], 1),
               "occupancy_plain": sum(ln) / max(row_steps, 1)}
        for w in ("continuous", "plain"):
            med = statistics.median(ms[name][w])
            out[w] = {"ms_median": med, "ms_min": min(ms[name][w]), "ms_max": max(ms[name][w]), "answers_per_sec": N * 1e3 / med}
        out["continuous_vs_plain"] = out["plain"]["ms_median"] / out["continuous"]["ms_median"]
        res[name] = out
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
