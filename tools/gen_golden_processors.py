#!/usr/bin/env python3
"""Generate tests/golden/generate_processors_micro.npz FROM THE REFERENCE's own generate(..., return_dict_in_generate=True,
output_scores=True, output_logits=True) with transformers' logits processors on.

Same setting as tools/gen_golden.py (whose helpers this imports; that script and its fixtures are untouched): the micro config,
the synthetic weights of opus_pllm_amd.synth (seed 0), HF EsmModel behind the reference's encoder interface, and the reference
OpusLlamaForCausalLM's greedy generate on the inputs of generate_micro (ids, mask, proteins), N greedy steps.

Cases (every key is prefixed with the case tag; `kw` holds the case's generate keywords as JSON):
  plain    no processor (what every other case is compared with)
  pen13    repetition_penalty=1.3
  pen08    repetition_penalty=0.8
  ngram2   no_repeat_ngram_size=2
  minnew   min_new_tokens=5 with eos_token_id=[27]
  bad      bad_words_ids=[[62], [52, 20]]
  minlen   min_length=30 with eos_token_id=[27] (transformers subtracts the spliced width of inputs_embeds)
  combo    repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=[[62], [52, 20], [27]], min_new_tokens=5, eos [27]
Stored per case: the new ids (`sequences`), the processed scores and the raw logits per step (fp32 [n, B, V]) and the spliced
width T (`T`, the same for every case).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg                                                # noqa: E402  (also puts the reference on sys.path)

N = 16
CASES = {
    "plain": {},
    "pen13": dict(repetition_penalty=1.3),
    "pen08": dict(repetition_penalty=0.8),
    "ngram2": dict(no_repeat_ngram_size=2),
    "minnew": dict(min_new_tokens=5, eos_token_id=[27]),
    "bad": dict(bad_words_ids=[[62], [52, 20]]),
    "minlen": dict(min_length=30, eos_token_id=[27]),
    "combo": dict(repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=[[62], [52, 20], [27]], min_new_tokens=5,
                  eos_token_id=[27]),
}


def main():
    cfg = gg.opa.micro()
    w = gg.synth.canonical_weights(cfg, seed=0)
    hf = gg.build_hf_esm(cfg, w)
    model = gg.build_ref_model(cfg, w, gg.FakeEncoder(hf))
    g = np.load(os.path.join(gg.GOLD, "generate_micro.npz"))
    seqs = json.load(open(os.path.join(gg.GOLD, "generate_micro.seqs.json")))
    ids, mask, pad = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), int(g["pad"])
    base = dict(attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, use_cache=True,
                return_dict_in_generate=True, output_scores=True, output_logits=True)
    with torch.no_grad():
        _, _, _, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, seqs, inference_mode=True)
    out = {"N": np.array(N), "pad": np.array(pad), "T": np.array(int(emb.shape[1]))}
    for tag, kw in CASES.items():
        kw = dict(kw)
        kw.setdefault("eos_token_id", None)
        with torch.no_grad():
            res = model.generate(ids, seqs, **base, **kw)
        n = len(res.scores)
        seq = res.sequences[:, -n:]
        out[tag + ".sequences"] = seq.numpy()
        out[tag + ".scores"] = torch.stack(res.scores).float().numpy()
        out[tag + ".logits"] = torch.stack(res.logits).float().numpy()
        out[tag + ".kw"] = np.array(json.dumps(kw))
        print(f"  {tag}: {n} steps, sequences {seq.tolist()}")
    gg.save("generate_processors_micro", **out)


if __name__ == "__main__":
    main()
