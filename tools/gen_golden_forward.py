#!/usr/bin/env python3
"""Generate tests/golden/forward_micro.npz (+ forward_micro.seqs.json) FROM THE REFERENCE's own forward(labels=...).

Same setting as tools/gen_golden.py (whose helpers this imports; that script and its fixtures are untouched): the micro config,
the synthetic weights of opus_pllm_amd.synth (seed 0), HF EsmModel behind the reference's encoder interface, and the reference
OpusLlamaForCausalLM called as `model(ids, attention_mask=mask, labels=labels, seq=seqs)` (opus_llama.py:41-92), which splices
the proteins in training mode (right padding, -100 labels on the protein slots) and returns HF's causal-LM loss and the logits.

Cases (every key is prefixed with the case tag):
  a      proteins + prompt + answer: labels -100 on the prompt, the answer ids after it; rows of different lengths, one row
         without <seq> (it still consumes a protein, as the reference's splice does)
  b      the same inputs with config.tokenizer_model_max_length set, so the training-mode truncation cuts answers
  c      text-only input_ids + labels (no seq)
  d      labels=None (proteins): logits only
Stored: the inputs, the reference loss, the spliced mask / labels, the logits (fp32, [B, T, V]; only the valid positions are
compared) and the per-token log-probs computed from those logits in fp64 (log p(labels[b, t]) at counted targets, 0 elsewhere).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg                                                # noqa: E402  (also puts the reference on sys.path)

MAX_LEN_B = 16


def _right_pad(rows, pad):
    width = max(len(r) for r in rows)
    ids = torch.full((len(rows), width), pad, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, : len(r)] = torch.tensor(r)
    return ids


def _token_logprobs(logits: torch.Tensor, labels: torch.Tensor) -> np.ndarray:
    """fp64 log p(labels[b, t] | < t) at counted targets (labels != -100, t >= 1), 0 elsewhere."""
    lp = torch.log_softmax(logits.double(), dim=-1)
    B, T, _ = logits.shape
    out = torch.zeros((B, T), dtype=torch.float64)
    for b in range(B):
        for t in range(1, T):
            y = int(labels[b, t])
            if y != -100:
                out[b, t] = lp[b, t - 1, y]
    return out.numpy()


def main():
    cfg = gg.opa.micro()
    w = gg.synth.canonical_weights(cfg, seed=0)
    hf = gg.build_hf_esm(cfg, w)
    model = gg.build_ref_model(cfg, w, gg.FakeEncoder(hf))
    V = cfg.dec_vocab
    rng = np.random.default_rng(11)
    r = lambda n: [int(x) for x in rng.integers(3, V, n)]          # noqa: E731
    pad = 2
    out = {}
    # (prompt, answer) rows: the <seq> placeholder sits in the prompt; row 2 has none
    prompts = [[1] + r(3) + [-200] + r(4), [1, -200] + r(6), [1] + r(5), [1] + r(2) + [-200] + r(2)]
    answers = [r(5), r(3), r(6), r(7)]
    rows = [p + a for p, a in zip(prompts, answers)]
    ids = _right_pad(rows, pad)
    mask = torch.zeros_like(ids, dtype=torch.bool)
    labels = torch.full_like(ids, -100)
    for i, (p, a) in enumerate(zip(prompts, answers)):
        mask[i, : len(p) + len(a)] = True
        labels[i, len(p): len(p) + len(a)] = torch.tensor(a)
    seqs = [gg.synth.synth_protein(n, 40 + i) for i, n in enumerate((19, 31, 7, 26))]     # one protein per row

    def run(tag, ids, mask, labels, seqs, max_length=None):
        if max_length is not None:
            model.config.tokenizer_model_max_length = max_length
        with torch.no_grad():
            kw = dict(attention_mask=mask, labels=labels)
            if seqs is not None:
                kw["seq"] = seqs
                _, _, mo, _, _, lab_out = model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, labels, seqs)
            else:
                mo, lab_out = mask, labels
            res = model(ids, **kw)
        if max_length is not None:
            del model.config.tokenizer_model_max_length
        logits = res.logits.float()
        out[tag + ".ids"] = ids.numpy()
        out[tag + ".mask"] = mask.numpy()
        out[tag + ".labels"] = (labels.numpy() if labels is not None else np.zeros((0,), np.int64))
        out[tag + ".has_seq"] = np.array(seqs is not None)
        out[tag + ".max_length"] = np.array(-1 if max_length is None else max_length)
        out[tag + ".mask_out"] = mo.bool().numpy()
        out[tag + ".logits"] = logits.numpy()
        if labels is not None:
            out[tag + ".labels_out"] = lab_out.numpy()
            out[tag + ".loss"] = np.array(float(res.loss), dtype=np.float64)
            out[tag + ".token_logprobs"] = _token_logprobs(logits, lab_out)
            out[tag + ".n_tokens"] = np.array(int((lab_out[:, 1:] != -100).sum()))
        else:
            assert res.loss is None
        print(f"  {tag}: T={logits.shape[1]} loss={None if res.loss is None else float(res.loss):}")

    run("a", ids, mask, labels, seqs)
    run("b", ids, mask, labels, seqs, max_length=MAX_LEN_B)
    tids = torch.where(ids == -200, torch.full_like(ids, 5), ids)          # (text-only: the placeholder becomes a plain token)
    run("c", tids, mask, labels, None)
    run("d", ids, mask, None, seqs)
    gg.save("forward_micro", **out)
    with open(os.path.join(gg.GOLD, "forward_micro.seqs.json"), "w") as f:
        json.dump(seqs, f)


if __name__ == "__main__":
    main()
