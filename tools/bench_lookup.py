#!/usr/bin/env python3
"""Prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)) at the Llama-3-8B shape on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 512-residue proteins, an 89-id prompt, greedy, 128 new tokens, no EOS id (every
id is generated), k = 7, through the product entry point model.generate(ids, seq=list[str], ...).  Per batch size (1, 4, 8) the
plain call and three lookup calls alternate in one process (round r runs each once, in order); medians of the rounds:
  plain      generate() without the argument (the captured decode step)
  miss       lookup_ids = ids the model never emits: drafts come from the history alone and are rejected - the overhead of the feature
             when it gains nothing
  oracle     lookup_ids = the plain call's own answer: every draft is right - the upper bound
  corrupted  that answer with every 4th and every 8th id replaced
Per case: ms, passes, plain steps, mean accepted ids per pass, whether the ids equal the plain call's, and from one extra call
in timing mode the pass's time per kernel class (phase "decode": all of it passes and plain steps).  Derived expectation, stated
beside the measured ratio: a pass of 16 rows or fewer costs about a batch-16 decode step, 1.05 x a batch-1 step, plus the
un-captured launch path.  It reports and sets no gate.  Prints ONE JSON line and writes it to profiles/lookup_bench.json; bench.py
is not involved and its line does not change.
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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--k", type=int, default=7)
    ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the shape's 32)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    N, k, Bmax = args.new_tokens, args.k, max(args.batches)
    kw_cfg = dict(max_batch=Bmax * (k + 1), max_enc_tokens=args.residues + 2, max_prompt=96, max_new_tokens=N)
    if args.layers:
        kw_cfg["dec_layers"] = args.layers
    cfg = opa.llama3_8b(**kw_cfg)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    seqs = [synth.synth_protein(args.residues, i) for i in range(Bmax)]
    ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=89) for i in range(Bmax)])
    mask = torch.ones_like(ids, dtype=torch.bool)

    def call(B, kw, n=N):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = model.generate(ids[:B], seqs[:B], attention_mask=mask[:B], pad_token_id=0, eos_token_id=None, max_new_tokens=n,
                             do_sample=False, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    res = {"shape": "llama3_8b", "decoder_layers": cfg.dec_layers, "residues": args.residues, "new_tokens": N, "k": k,
           "rounds": args.rounds, "entry": "model.generate(ids, seq=list[str], ...)", "batches": {}}
    for B in args.batches:
        _, answer = call(B, {})
        answer = answer.cpu()
        used = set(answer.flatten().tolist()) | set(ids.flatten().tolist())
        never = [t for t in range(1000, 1000 + 4 * N) if t not in used][:N]
        corrupted = answer.clone()
        corrupted[:, 3::4] = torch.tensor(never[: corrupted[:, 3::4].shape[1]])
        corrupted[:, 7::8] = torch.tensor(never[: corrupted[:, 7::8].shape[1]]) + 1
        lk = dict(prompt_lookup_num_tokens=k, return_dict_in_generate=True)
        cases = {"plain": {}, "miss": dict(lk, lookup_ids=[never] * B), "oracle": dict(lk, lookup_ids=answer),
                 "corrupted": dict(lk, lookup_ids=corrupted)}
        ms = {c: [] for c in cases}
        last, first_id = {}, []
        for r in range(args.warmup + args.rounds):
            t, _ = call(B, {}, 1)                      # encode + splice + prefill + the first id: what every case spends before its loop
            if r >= args.warmup:
                first_id.append(t)
            for c, kw in cases.items():
                t, out = call(B, kw)
                last[c] = out
                if r >= args.warmup:
                    ms[c].append(t)
        row = {}
        plain_ms = statistics.median(ms["plain"])
        for c in cases:
            med = statistics.median(ms[c])
            row[c] = {"ms_median": med, "ms_min": min(ms[c]), "ms_max": max(ms[c]), "tokens_per_sec": B * N * 1e3 / med}
            if c == "plain":
                continue
            st = last[c].stats
            row[c].update(passes=st.passes, plain_steps=st.plain_steps, drafted=st.drafted, accepted=st.accepted,
                          accepted_per_pass=st.accepted / max(st.passes, 1), vs_plain=med / plain_ms,
                          ids_equal_plain=bool(torch.equal(last[c].sequences.cpu(), answer)))
            model.timing(True)                        # the pass's time per kernel class: every launch recorded, eager
            call(B, cases[c])
            classes, _ = model.timing_names()
            per = {kc: model.timing_get(kc, "decode") for kc in classes}
            model.timing(False)
            row[c]["decode_ms_by_class"] = {kc: round(v[0], 3) for kc, v in per.items() if v[1]}
            row[c]["decode_launches"] = int(sum(v[1] for v in per.values()))
        # the derived expectation beside what was measured: one pass against one plain (captured) step of this batch
        base = statistics.median(first_id)
        row["first_id_ms_median"] = base
        row["plain"]["ms_per_step"] = (plain_ms - base) / max(N - 1, 1)
        for c in ("miss", "oracle", "corrupted"):
            steps = row[c]["passes"] + row[c]["plain_steps"]
            row[c]["ms_per_pass_or_step"] = (row[c]["ms_median"] - base) / max(steps, 1)
            row[c]["pass_vs_plain_step_measured"] = row[c]["ms_per_pass_or_step"] / row["plain"]["ms_per_step"]
        row["pass_vs_plain_step_expected"] = 1.05
        res["batches"][str(B)] = row
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
