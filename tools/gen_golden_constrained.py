#!/usr/bin/env python3
"""Generate tests/golden/generate_constrained_micro.npz FROM THE REFERENCE's own generate(..., prefix_allowed_tokens_fn=trie,
return_dict_in_generate=True, output_scores=True, output_logits=True): transformers' PrefixConstrainedLogitsProcessor driven by
the same opus_pllm_amd.TokenTrie object the GPU path compiles to its automaton (the object is a plain transformers callback).

Same setting as tools/gen_golden.py (whose helpers this imports; that script and its fixtures are untouched): the micro config,
the synthetic weights (seed 0), the reference OpusLlamaForCausalLM's greedy generate on the inputs of generate_micro, end id 27,
N = 16 steps.

Cases (every key is prefixed with the case tag; `kw` holds the extra generate keywords as JSON, `spec` the tries as JSON):
  shared      one trie of 24 random members of 1 to 6 ids for every row
  per_row     three tries (TokenTrie.per_row), one per row
  list        the shared members with a one-id separator: several members per row
  shared_pen  shared + repetition_penalty=1.3
  list_ngram  list + no_repeat_ngram_size=2, repetition_penalty=1.3
Stored per case: the new ids (`sequences`), the processed scores and the raw logits per step (fp32 [n, B, V]).

The script searches the seed of the random member lists and REFUSES to write unless, at every step of every unfinished row where
more than one id is allowed, the reference's processed top-1 margin is at least MARGIN, every case has at least MIN_CONTESTED
such steps, and list_ngram returns other ids than list - so that a test may compare every id."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg                                                # noqa: E402  (also puts the reference on sys.path)

N, END, SEP, MARGIN, MIN_CONTESTED = 16, 27, 26, 0.10, 3


def members(seed: int, vocab: int, n: int = 24):
    g = np.random.default_rng(seed)
    pool = [t for t in range(vocab) if t not in (END, SEP)]
    return [[int(pool[i]) for i in g.integers(0, len(pool), size=int(g.integers(1, 7)))] for _ in range(n)]


def specs(seed: int, vocab: int):
    sh = members(seed, vocab)
    rows = [members(1000 + 10 * seed + k, vocab) for k in range(3)]
    return {
        "shared": (dict(tries=[dict(members=sh, sep=None)], per_row=False), {}),
        "per_row": (dict(tries=[dict(members=m, sep=None) for m in rows], per_row=True), {}),
        "list": (dict(tries=[dict(members=sh, sep=[SEP])], per_row=False), {}),
        "shared_pen": (dict(tries=[dict(members=sh, sep=None)], per_row=False), dict(repetition_penalty=1.3)),
        "list_ngram": (dict(tries=[dict(members=sh, sep=[SEP])], per_row=False),
                       dict(no_repeat_ngram_size=2, repetition_penalty=1.3)),
    }


def build(spec):
    tries = [gg.opa.TokenTrie(t["members"], end_token_id=END, separator=t["sep"]) for t in spec["tries"]]
    return gg.opa.TokenTrie.per_row(tries) if spec["per_row"] else tries[0]


def run(model, ids, seqs, base, spec, kw):
    fn = build(spec)
    with torch.no_grad():
        res = model.generate(ids, seqs, prefix_allowed_tokens_fn=fn, eos_token_id=[END], **base, **kw)
    n = len(res.scores)
    seq = res.sequences[:, -n:]
    sc, lg = torch.stack(res.scores).float(), torch.stack(res.logits).float()
    contested, worst = 0, float("inf")
    for b in range(seq.shape[0]):
        for t in range(n):
            if END in seq[b, :t].tolist():
                break
            if len(fn(b, seq[b, :t])) > 1:
                top = sc[t, b].topk(2).values
                contested += 1
                worst = min(worst, float(top[0] - top[1]))
    return seq, sc, lg, contested, worst


def main():
    cfg = gg.opa.micro()
    w = gg.synth.canonical_weights(cfg, seed=0)
    model = gg.build_ref_model(cfg, w, gg.FakeEncoder(gg.build_hf_esm(cfg, w)))
    g = np.load(os.path.join(gg.GOLD, "generate_micro.npz"))
    seqs = json.load(open(os.path.join(gg.GOLD, "generate_micro.seqs.json")))
    ids, mask, pad = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), int(g["pad"])
    base = dict(attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, use_cache=True,
                return_dict_in_generate=True, output_scores=True, output_logits=True)
    for seed in range(64):
        out = {"N": np.array(N), "pad": np.array(pad), "end": np.array(END), "seed": np.array(seed)}
        ok, seqs_of = True, {}
        for tag, (spec, kw) in specs(seed, cfg.dec_vocab).items():
            seq, sc, lg, contested, worst = run(model, ids, seqs, base, spec, kw)
            print(f"  seed {seed} {tag}: {contested} contested steps, smallest margin {worst:.3f}, ids {seq.tolist()}")
            if contested < MIN_CONTESTED or worst < MARGIN:
                ok = False
                break
            seqs_of[tag] = seq
            out[tag + ".sequences"] = seq.numpy()
            out[tag + ".scores"] = sc.numpy()
            out[tag + ".logits"] = lg.numpy()
            out[tag + ".kw"] = np.array(json.dumps(kw))
            out[tag + ".spec"] = np.array(json.dumps(spec))
            out[tag + ".contested"] = np.array(contested)
            out[tag + ".margin"] = np.array(worst, dtype=np.float64)
        if ok and not torch.equal(seqs_of["list"], seqs_of["list_ngram"]):
            gg.save("generate_constrained_micro", **out)
            return
    raise SystemExit("no seed below 64 meets the margin condition: nothing written")


if __name__ == "__main__":
    main()
