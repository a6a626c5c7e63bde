#!/usr/bin/env python3
"""generate(prefix=...) against the plain generate() on the same prompts, on one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, 64 decoder rows, 512-residue proteins, greedy, no EOS (every step runs), 32 new
tokens, through the product entry point model.generate(...).  The plain call and the call behind a prefix run in alternation in one
process (round r runs each once, in order).  Three figures:
  shared_head   64 rows whose prompts share a head of --head ids in front of the protein: the plain call prefills 64 x (head + 8
                protein + rest) positions, the other one 64 x (8 + rest) behind one detached one-row prefix
  per_protein   16 proteins x 4 questions: the plain call encodes 64 proteins and prefills 64 whole prompts, the other one
                generates 64 question rows behind 16 detached prefixes (head + protein tokens; cached once, outside the timing,
                as a proteome run would keep them)
  kv_place      the placement launch alone (the library times it as one record of class "other", phase "other", with the
                dispatch's own timestamps), in GB/s of what it reads and writes
Prints ONE JSON line and writes it to --out (default profiles/prefix_generate_bench.json).  bench.py is not involved.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--head", type=int, default=40)
    ap.add_argument("--rest", type=int, default=48, help="text ids behind the protein")
    ap.add_argument("--questions", type=int, default=4)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--new_tokens", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "prefix_generate_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    R, Q = args.rows, args.questions
    P = R // Q
    T = args.head + args.rest + 8
    cfg = opa.llama3_8b(max_batch=R, max_enc_tokens=args.residues + 2, max_prompt=T, max_new_tokens=args.new_tokens)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    rng = np.random.default_rng(0)
    text = lambda n: torch.from_numpy(rng.integers(3, cfg.dec_vocab, n))                       # noqa: E731
    seq_tok = torch.tensor([opa.DEFAULT_SEQ_TOKEN_INDEX])
    head = text(args.head)
    kw = dict(pad_token_id=0, eos_token_id=[], max_new_tokens=args.new_tokens, do_sample=False)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def alternate(plain, behind):
        ms = {"plain": [], "behind": []}
        agree = []
        for r in range(args.warmup + args.rounds):
            tp, a = timed(plain)
            tb, b = timed(behind)
            if r >= args.warmup:
                ms["plain"].append(tp)
                ms["behind"].append(tb)
                agree.append(float((a == b).float().mean()))
        m = {c: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for c, v in ms.items()}
        m["saving_ms_median"] = statistics.median([a - b for a, b in zip(ms["plain"], ms["behind"])])
        m["saving_rel"] = m["saving_ms_median"] / m["plain"]["ms_median"]
        m["ids_agree"] = min(agree)
        return m

    res = {"shape": "llama3_8b", "rows": R, "head": args.head, "rest": args.rest, "residues": args.residues,
           "new_tokens": args.new_tokens, "rounds": args.rounds, "entry": "model.generate(...)"}
    # (a) one shared head
    seqs = [synth.synth_protein(args.residues, i) for i in range(R)]
    rests = [text(args.rest) for _ in range(R)]
    whole = torch.stack([torch.cat([head, seq_tok, r]) for r in rests])
    tails = torch.stack([torch.cat([seq_tok, r]) for r in rests])
    shared = model.cache_prefix(head[None], detach=True)
    res["shared_head"] = alternate(lambda: model.generate(whole, seqs, **kw),
                                   lambda: model.generate(tails, seqs, prefix=shared, prefix_rows=[0] * R, **kw))
    res["shared_head"]["positions"] = {"plain": R * T, "behind": R * (args.rest + 8)}
    # (b) P proteins x Q questions behind P per-protein prefixes (head + protein tokens)
    prot = [synth.synth_protein(args.residues, 1000 + i) for i in range(P)]
    quest = [text(args.rest) for _ in range(R)]
    rows = torch.arange(P).repeat_interleave(Q)
    whole = torch.stack([torch.cat([head, seq_tok, q]) for q in quest])
    seqs_rep = [prot[int(p)] for p in rows]
    per = model.cache_prefix(torch.cat([head, seq_tok])[None].repeat(P, 1), seq=prot, detach=True)
    res["per_protein"] = alternate(lambda: model.generate(whole, seqs_rep, **kw),
                                   lambda: model.generate(torch.stack(quest), prefix=per, prefix_rows=rows, **kw))
    res["per_protein"].update(proteins=P, questions=Q, positions={"plain": R * T, "behind": R * args.rest})
    # (c) the placement launch alone: opus_llama_prefill_behind times it under phase "other" (class "other"), with the dispatch's
    # own start / end timestamps, so one record per call is the kv_place launch; GB/s of what it reads and writes
    from opus_pllm_amd import _cabi
    emb = model.model.embed_tokens(torch.stack(rests).to(dev)).to(_cabi.operand_dtype())
    slot_bytes = 2 * cfg.dec_layers * cfg.dec_kv_heads * cfg.dec_head_dim * 2
    ms = []
    for r in range(args.warmup + args.rounds):
        model.timing(True)
        model.prefill_logits_behind(shared, emb, [args.rest] * R, [0] * R)
        t = model.timing_get("other", "other")
        model.timing(False)
        assert t[1] == 1, t                                       # one launch
        if r >= args.warmup:
            ms.append(float(t[0]))
    moved = slot_bytes * args.head * (R + 1)                      # written to R rows, read once
    med = statistics.median(ms)
    res["kv_place"] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "launches_per_call": 1, "bytes_moved": moved,
                       "bytes_per_placed_slot": slot_bytes, "gb_per_s": moved / (med * 1e-3) / 1e9}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
