#!/usr/bin/env python3
"""A follow-up turn through generate(return_prefix=True)'s handle against plain generate() on the concatenated conversation, on
one MI355X.

OPUS-PLLM-Llama3-8B shape with synthetic weights, text-only rows, greedy, no EOS (every step runs), through the product entry
point model.generate(...).  For every batch size (1 and 8) and history length (128 and 384 cache slots): a first turn of
history - 31 prompt ids and 32 new ids leaves a handle of `history` slots (31 decode slots kept, the last id pending); the measured
turn is a 16-id follow-up with 32 new ids
  handle  generate(follow_up, prefix=handle): kv_place of the history, a prefill of 1 + 16 positions per row, 31 decode steps
  plain   generate(history ids + pending id + follow_up): a prefill of history + 17 positions per row, 31 decode steps
alternating in one process (round r runs each once, in order), medians of --rounds rounds, the plain call's own spread beside them.
`ids_agree` is the share of equal ids (the two prefills run on other launch shapes, so near-ties may differ).
Separately, `export`: the opus_llama_prefix_export_rows launch alone (the library times it as one record of class "other", phase
"other", with the dispatch's own timestamps), with the bytes it reads and writes and GB/s.
Prints ONE JSON line and writes it to --out (default profiles/chat_bench.json).  bench.py is not involved.
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--histories", type=int, nargs="+", default=[128, 384])
    ap.add_argument("--follow_up", type=int, default=16)
    ap.add_argument("--new_tokens", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chat_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    N, F = args.new_tokens, args.follow_up
    cfg = opa.llama3_8b(max_batch=max(args.batches), max_enc_tokens=66, max_prompt=max(args.histories) + 1 + F, max_new_tokens=N)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    rng = np.random.default_rng(0)
    text = lambda b, n: torch.from_numpy(rng.integers(3, cfg.dec_vocab, (b, n)))               # noqa: E731
    kw = dict(pad_token_id=0, eos_token_id=[], max_new_tokens=N, do_sample=False)
    slot_bytes = 2 * cfg.dec_layers * cfg.dec_kv_heads * cfg.dec_head_dim * 2

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    res = {"shape": "llama3_8b", "follow_up": F, "new_tokens": N, "rounds": args.rounds, "entry": "model.generate(...)",
           "bytes_per_slot_and_row": slot_bytes, "cases": []}
    for B in args.batches:
        for H in args.histories:
            prompt = text(B, H - (N - 1))
            first = model.generate(prompt, return_dict_in_generate=True, return_prefix=True, **kw)
            handle = first.prefix
            assert handle.slots == H and handle.lengths.tolist() == [H] * B, (handle.slots, H)
            follow = text(B, F)
            whole = torch.cat([prompt, first.sequences.cpu(), follow], dim=1)                   # history + pending id + follow-up
            ms = {"plain": [], "handle": []}
            agree = []
            for r in range(args.warmup + args.rounds):
                tp, a = timed(lambda: model.generate(whole, **kw))
                th, b = timed(lambda: model.generate(follow, prefix=handle, **kw))
                if r >= args.warmup:
                    ms["plain"].append(tp)
                    ms["handle"].append(th)
                    agree.append(float((a == b).float().mean()))
            case = {"batch": B, "history_slots": H, "handle_bytes": handle.nbytes(),
                    "positions_prefilled": {"plain": B * (H + 1 + F), "handle": B * (1 + F)}}
            for c, v in ms.items():
                case[c] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
            case["saving_ms_median"] = statistics.median([a - b for a, b in zip(ms["plain"], ms["handle"])])
            case["saving_rel"] = case["saving_ms_median"] / case["plain"]["ms_median"]
            case["ids_agree"] = min(agree)
            # the export launch alone, on the state the first turn's call leaves
            model.generate(prompt, **kw)
            ex = []
            for r in range(args.warmup + args.rounds):
                model.timing(True)
                model.export_cache_rows([N - 1] * B, H)
                t = model.timing_get("other", "other")
                model.timing(False)
                assert t[1] == 1, t                                   # one launch
                if r >= args.warmup:
                    ex.append(float(t[0]))
            moved = slot_bytes * B * H * 2                            # every slot of the windows read once, written once
            med = statistics.median(ex)
            case["export"] = {"ms_median": med, "ms_min": min(ex), "ms_max": max(ex), "launches_per_call": 1, "bytes_moved": moved,
                              "gb_per_s": moved / (med * 1e-3) / 1e9}
            res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
