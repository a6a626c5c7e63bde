#!/usr/bin/env python3
"""Trie search (search_trie) against score_trie(...).topk on the same prefix, at the Llama-3-8B shape on one MI355X.

Synthetic fp16 weights.  16 prompts of 8 protein tokens + 96 text positions (tools/bench_trie_score.py's), prefilled ONCE outside
the timing.  Two GO-shaped vocabularies from seeded random ids: that tool's 2 000 members of 5 tokens (fan-outs 1, 1, 10, 20, 10)
and one of 50 000 members of 7 tokens (fan-outs 1, 1, 10, 20, 10, 5, 5).  Per vocabulary, with and without the stop term,
  (a) score_trie(prefix, trie, include_stop).topk(5)                      every node (with a child) through the decoder
  (b) search_trie(prefix, trie, num_beams=8, top=5, include_stop)         prompts x beams x levels decoder rows
alternate in one process, warmed, host clock around calls that end in a synchronise; medians of the rounds with their spread.
Beside them: decoder rows and levels, the time in opus_kv_reorder (device events around its calls), the expand kernel's time per
level (timing class "trie_search") against the bytes it reads (per edge of a live beam: id, target, member or edge-count word,
logit; twice without the stop term, whose pool takes a sweep of its own), and how many of (b)'s members are (a)'s.
Prints ONE JSON line and writes profiles/trie_search_bench.json.  Not a pass/fail gate; bench.py is not involved.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOCABS = {"go2k": (1, 1, 10, 20, 10), "go50k": (1, 1, 10, 20, 10, 5, 5)}


def shaped_trie(fan, vocab: int, end_id: int, seed: int = 0):
    import numpy as np
    from opus_pllm_amd.constraint import TokenTrie
    rng = np.random.default_rng(seed)
    paths = [[]]
    for f in fan:
        paths = [p + [int(t)] for p in paths for t in rng.choice(np.arange(3, vocab), size=f, replace=False)]
    return TokenTrie(paths, end_token_id=end_id)


class _TimedReorder:
    """The library with opus_kv_reorder wrapped in device events (everything else passes through)."""

    def __init__(self, lib, torch):
        self._lib, self._torch, self.events = lib, torch, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def opus_kv_reorder(self, *a):
        t = self._torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        rc = self._lib.opus_kv_reorder(*a)
        e1.record()
        self.events.append((e0, e1))
        return rc

    def take_ms(self):
        self._torch.cuda.synchronize()
        ms, n = sum(a.elapsed_time(b) for a, b in self.events), len(self.events)
        self.events = []
        return round(ms, 3), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=16)
    ap.add_argument("--beams", type=int, default=8)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--max_batch", type=int, default=64, help="decoder rows of the context: prompts x beams above it run in groups")
    ap.add_argument("--vocabs", type=str, default="go2k,go50k")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "trie_search_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.constraint import TrieSearchTable
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    P, K, top, N_PROMPT = args.prompts, args.beams, args.top, 96
    cfg = opa.llama3_8b(max_batch=args.max_batch, max_enc_tokens=66, max_prompt=8 + N_PROMPT + 6, max_new_tokens=16)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    prompts = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=N_PROMPT + 1, seq_pos=1) for i in range(P)])
    g = torch.Generator(device=dev).manual_seed(0)
    prot = (torch.randn((P, cfg.n_prot_tokens, cfg.dec_dim), generator=g, device=dev) * 0.02).to(_cabi.operand_dtype())
    prefix = model.cache_prefix(prompts, protein_tokens=prot, detach=True)
    timed = _TimedReorder(model._lib, torch)
    classes, _ = model.timing_names()
    out = dict(workload=f"Llama-3-8B fp16 synthetic: {P} prompts x (8 protein + {N_PROMPT} text); search_trie(num_beams={K}, top={top}) "
                        f"against score_trie(...).topk({top}); context of {args.max_batch} decoder rows "
                        f"({-(-P * K // args.max_batch)} group(s) of {min(P * K, args.max_batch)} rows)",
               rounds=args.rounds, warmup=args.warmup, vocabularies={})
    for vname in args.vocabs.split(","):
        fan = VOCABS[vname]
        trie = shaped_trie(fan, cfg.dec_vocab, end_id=2)
        tab = TrieSearchTable([trie])
        n_inner = sum(1 for v in range(1, trie.n_nodes + 1) if trie.children[v])
        rec = dict(fan_outs=list(fan), members=len(trie.member_ids), depth=trie.max_depth, nodes=trie.n_nodes, nodes_with_child=n_inner)
        for stop in (False, True):
            forms = {"score_trie_topk": lambda: model.score_trie(prefix, trie, include_stop=stop).topk(top),
                     "search_trie": lambda: model.search_trie(prefix, trie, num_beams=K, top=top, include_stop=stop)}
            times, last = {k: [] for k in forms}, {}
            for r in range(args.warmup + args.rounds):
                for name, fn in forms.items():                                           # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[name] = fn()
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            res = last["search_trie"]
            _, want = last["score_trie_topk"]
            same = (res.member_index == want).float().mean().item()
            as_set = np.mean([len(set(a) & set(b)) / top for a, b in zip(res.member_index.cpu().tolist(), want.cpu().tolist())])
            # one more call each way: the reorder's device time, then the expand kernel's own time (timing mode)
            model._lib = timed
            tr = model.search_trie(prefix, trie, num_beams=K, top=top, include_stop=stop, return_trace=True)
            reorder_ms, reorder_calls = timed.take_ms()
            model._lib = timed._lib
            edges = 0
            for lv in tr.trace:
                st = lv["from_node"][lv["from_alive"]].long().numpy() + int(tab.start[0])
                edges += int((tab.edge_off[st + 1] - tab.edge_off[st]).sum())
            model.timing(True)
            model.search_trie(prefix, trie, num_beams=K, top=top, include_stop=stop)
            torch.cuda.synchronize()
            k_ms, k_n, _, _ = model.timing_get("trie_search", "*")
            by_class = {c: round(model.timing_get(c, "*")[0], 3) for c in classes if model.timing_get(c, "*")[1]}
            model.timing(False)
            med = {k: float(np.median(v)) for k, v in times.items()}
            read = edges * 16 * (1 if stop else 2)
            rec["stop" if stop else "no_stop"] = dict(
                ms_rounds=times, ms_median=med, spread_ms={k: round(max(v) - min(v), 3) for k, v in times.items()},
                speedup_search_vs_score=round(med["score_trie_topk"] / med["search_trie"], 2),
                decoder_rows=dict(score_trie=P * (trie.n_nodes if stop else n_inner), search_trie=res.rows_decoded),
                levels=res.levels, exhaustive_prompts=int(res.exhaustive.sum()), members_equal_rank_by_rank=round(same, 4),
                members_in_common=round(float(as_set), 4),
                kv_reorder=dict(ms=reorder_ms, calls=reorder_calls),
                expand_kernel=dict(ms_total=round(k_ms, 4), launches=int(k_n), us_per_level=round(1e3 * k_ms / max(k_n, 1), 2),
                                   edges_read=edges, bytes_read=read, gb_per_s=round(read / max(k_ms, 1e-9) / 1e6, 2)),
                eager_class_ms=by_class)
            print(f"[{vname} stop={stop}] {med}", file=sys.stderr, flush=True)
        out["vocabularies"][vname] = rec
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
