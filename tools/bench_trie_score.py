#!/usr/bin/env python3
"""Trie scoring (score_trie) against score_continuations on the flat member list, at the Llama-3-8B shape on one MI355X.

Synthetic fp16 weights.  16 prompts of 8 protein tokens (projected blocks passed as protein_tokens=, so the encoder is outside
every side) + 96 text positions, prefilled ONCE outside the timing; a GO-shaped vocabulary with fan-outs (1, 1, 10, 20, 10) built
from seeded random ids: 2 000 members of 5 tokens, 2 212 nodes, 212 of them with a child.  Measured in one process, warmed, in
alternating rounds, host clock around calls that end in a synchronise:
  (a) score_continuations on all 2 000 members per prompt (what gave these numbers before score_trie): 160 000 decoder rows
  (b) score_trie(include_stop=True): 35 392 decoder rows
  (c) score_trie(include_stop=False): 3 392 decoder rows
plus the timing classes of the `score` phase of one call of each form (opus_timing_get) and the largest node log-prob difference
between (a) and (b).  Prints ONE JSON line and writes it to profiles/trie_scoring_bench.json (merged into the file when it already
holds other keys, e.g. the bench.py alternation).  bench.py is not involved and its line does not change.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAN = (1, 1, 10, 20, 10)


def go_shaped_trie(vocab: int, end_id: int, seed: int = 0):
    import numpy as np
    from opus_pllm_amd.constraint import TokenTrie
    rng = np.random.default_rng(seed)
    paths = [[]]
    for f in FAN:
        paths = [p + [int(t)] for p in paths for t in rng.choice(np.arange(3, vocab), size=f, replace=False)]
    return TokenTrie(paths, end_token_id=end_id)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "trie_scoring_bench.json"))
    args = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    P, N_PROMPT = args.prompts, 96
    cfg = opa.llama3_8b(max_batch=P, max_enc_tokens=66, max_prompt=8 + N_PROMPT + 6, max_new_tokens=16)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    prompts = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=N_PROMPT + 1, seq_pos=1) for i in range(P)])
    g = torch.Generator(device=dev).manual_seed(0)
    prot = (torch.randn((P, cfg.n_prot_tokens, cfg.dec_dim), generator=g, device=dev) * 0.02).to(_cabi.operand_dtype())
    trie = go_shaped_trie(cfg.dec_vocab, end_id=2)
    M, depth = len(trie.member_ids), len(FAN)
    n_inner = sum(1 for v in range(1, trie.n_nodes + 1) if trie.children[v])
    members = torch.tensor(trie.member_ids, dtype=torch.long)                            # [M, 5]
    conts = members.repeat(P, 1)
    src = torch.arange(P).repeat_interleave(M)
    prefix = model.cache_prefix(prompts, protein_tokens=prot)

    forms = {
        "flat": lambda: model.score_continuations(prefix, conts, prefix_rows=src),
        "trie_stop": lambda: model.score_trie(prefix, trie, include_stop=True),
        "trie": lambda: model.score_trie(prefix, trie, include_stop=False),
    }
    times = {k: [] for k in forms}
    last = {}
    for r in range(args.warmup + args.rounds):
        for name, fn in forms.items():                                                   # alternating: a, b, c, a, b, c, ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    # node log-probs of the flat call: token j of member m is the node at depth j + 1 of its path
    path = np.zeros((M, depth), dtype=np.int64)
    for m, ids in enumerate(trie.member_ids):
        v = 0
        for j, t in enumerate(ids):
            v = trie.children[v][t]
            path[m, j] = v
    flat_lp = last["flat"].token_logprobs.view(P, M, depth)
    node_b = last["trie_stop"].node_logprobs[:, torch.from_numpy(path).to(dev)]          # [P, M, depth]
    node_c = last["trie"].node_logprobs[:, torch.from_numpy(path).to(dev)]
    d_ab = float((flat_lp.double() - node_b.double()).abs().max())
    d_bc = float((node_b.double() - node_c.double()).abs().max())

    classes, phases = model.timing_names()
    score_classes = {}
    for name, fn in forms.items():
        model.timing(True)                                                               # (enables and resets)
        fn()
        torch.cuda.synchronize()
        score_classes[name] = {k: round(model.timing_get(k, "score")[0], 3) for k in classes if model.timing_get(k, "score")[1]}
    model.timing(False)

    med = {k: float(np.median(v)) for k, v in times.items()}
    rows = dict(flat=P * M * depth, trie_stop=P * trie.n_nodes, trie=P * n_inner)
    out = dict(
        workload=f"Llama-3-8B fp16 synthetic: {P} prompts x (8 protein + {N_PROMPT} text), vocabulary of fan-outs {FAN}: {M} members of "
                 f"{depth} tokens, {trie.n_nodes} nodes, {n_inner} with a child",
        rounds=args.rounds, warmup=args.warmup,
        decoder_rows=rows,
        rows_evaluated=dict(trie_stop=last["trie_stop"].rows_evaluated, trie=last["trie"].rows_evaluated),
        rows_per_pass=int(model._lib.opus_llama_dec_rows_cap(ctypes.byref(_cabi.CConfig.from_config(cfg)))),
        ms_rounds=times, ms_median=med,
        spread_ms={k: round(max(v) - min(v), 3) for k, v in times.items()},
        speedup_vs_flat=dict(trie_stop=round(med["flat"] / med["trie_stop"], 2), trie=round(med["flat"] / med["trie"], 2)),
        row_ratio_vs_flat=dict(trie_stop=round(rows["flat"] / rows["trie_stop"], 2), trie=round(rows["flat"] / rows["trie"], 2)),
        max_abs_node_logprob_diff_flat_vs_trie_stop=d_ab, max_abs_node_logprob_diff_stop_vs_no_stop=d_bc,
        score_phase_class_ms=score_classes,
    )
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    merged = {}
    if os.path.exists(args.out):
        try:
            merged = json.load(open(args.out))
        except ValueError:
            merged = {}
    merged.update(out)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
