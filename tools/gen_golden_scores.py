#!/usr/bin/env python3
"""Generate tests/golden/generate_scores_micro.npz FROM THE REFERENCE's own generate(..., return_dict_in_generate=True,
output_scores=True, output_logits=True).

Same setting as tools/gen_golden.py (whose helpers this imports; that script and its fixtures are untouched): the micro config,
the synthetic weights of opus_pllm_amd.synth (seed 0), HF EsmModel behind the reference's encoder interface, and the reference
OpusLlamaForCausalLM's greedy generate on the inputs of generate_micro (ids, mask, proteins).

Cases (every key is prefixed with the case tag):
  free   decoding to max_new_tokens (no EOS)
  eos    with an EOS id that the rows emit at different steps, so that rows finish at different lengths (pad behind them)
Stored per case: the new ids (`sequences`), the processed scores and the raw logits per step (fp32 [n, B, V]), and
compute_transition_scores(sequences, logits, normalize_logits=True) ([B, n], HF's masking of nothing: greedy has no beams).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg                                                # noqa: E402  (also puts the reference on sys.path)

N = 12


def main():
    cfg = gg.opa.micro()
    w = gg.synth.canonical_weights(cfg, seed=0)
    hf = gg.build_hf_esm(cfg, w)
    model = gg.build_ref_model(cfg, w, gg.FakeEncoder(hf))
    g = np.load(os.path.join(gg.GOLD, "generate_micro.npz"))
    seqs = json.load(open(os.path.join(gg.GOLD, "generate_micro.seqs.json")))
    ids, mask, pad = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), int(g["pad"])
    kw = dict(attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, use_cache=True,
              return_dict_in_generate=True, output_scores=True, output_logits=True)
    out = {"N": np.array(N), "pad": np.array(pad)}
    with torch.no_grad():
        free = model.generate(ids, seqs, eos_token_id=None, **kw)
        # an EOS id that row 1 emits at step 2 and row 0 at a later step (or never): rows finish at different steps
        s = free.sequences
        eos = None
        for t in range(1, N - 2):
            cand = int(s[1, t])
            first = [int((s[b] == cand).nonzero()[0]) if bool((s[b] == cand).any()) else N for b in range(s.shape[0])]
            if first[1] == t and len(set(first)) == len(first):
                eos = cand
                break
        assert eos is not None, "no EOS id that makes the rows finish at different steps"
        stop = model.generate(ids, seqs, eos_token_id=[eos], **kw)
    out["eos_id"] = np.array(eos)
    for tag, res in (("free", free), ("eos", stop)):
        n = len(res.scores)
        seq = res.sequences[:, -n:]
        out[tag + ".sequences"] = seq.numpy()
        out[tag + ".scores"] = torch.stack(res.scores).float().numpy()
        out[tag + ".logits"] = torch.stack(res.logits).float().numpy()
        out[tag + ".transition"] = model.compute_transition_scores(res.sequences, res.logits, normalize_logits=True).float().numpy()
        print(f"  {tag}: {n} steps, sequences {seq.tolist()}")
    gg.save("generate_scores_micro", **out)


if __name__ == "__main__":
    main()
