"""Writes tests/golden/mlm_micro.npz: transformers' EsmForMaskedLM on the synthetic micro weights (seed 0) with the synthetic
masked-LM head (synth.mlm_head, seed 0).  Needs transformers only.

    python tools/gen_golden_mlm.py

  tokens        int32 [3, 4, 66]      a batch of 1, 2, 17 and 64 residues: no mask, one mask per row, several masks per row
  logits        fp32  [3, 4, 66, 33]  EsmForMaskedLM(tokens).logits (padding rows included as the model gives them)
  head_seed     int                   seed of synth.mlm_head
  logit_std     float                 standard deviation of the logits over the vocabulary, mean over the real rows
  scan_tokens_{0,1}   int32 [9], [17] residue ids of the two proteins of the masked scan
  scan_log_probs_{0,1} fp32 [n, 33]   their masked-marginal log-probabilities, one EsmForMaskedLM pass per masked copy
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import opus_pllm_amd as opa                     # noqa: E402
from opus_pllm_amd import synth                 # noqa: E402
import mlm_ref                                  # noqa: E402

HEAD_SEED = 0


def main():
    torch.manual_seed(0)
    cfg = opa.micro()
    W = synth.canonical_weights(cfg, 0)
    head = synth.mlm_head(cfg, HEAD_SEED)
    hf = mlm_ref.build_hf_mlm(cfg, W, head)
    toks = mlm_ref.fixture_tokens()
    logits = np.stack([mlm_ref.hf_logits(hf, torch.from_numpy(t).long()).numpy() for t in toks]).astype(np.float32)
    real = toks != 1
    out = {"tokens": toks.astype(np.int32), "logits": logits, "head_seed": np.int64(HEAD_SEED),
           "logit_std": np.float64(logits[real].std(axis=-1).mean())}
    fn = mlm_ref.hf_logits_fn(hf)
    for i, s in enumerate(mlm_ref.scan_sequences()):
        ids = mlm_ref.ids_of(s)
        out[f"scan_tokens_{i}"] = ids.astype(np.int32)
        out[f"scan_log_probs_{i}"] = mlm_ref.masked_marginals(ids, fn).numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "mlm_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes), logit_std {float(out['logit_std']):.3f}")


if __name__ == "__main__":
    main()
