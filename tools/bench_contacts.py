#!/usr/bin/env python3
"""ESM-2 contact maps (get_amino_acid_embeddings(return_contacts=True)) at the ESM-2 650M encoder shape on one MI355X.

Synthetic fp16 weights (33 x 1280, 20 heads of 64; a small decoder that is never run).  Two batches of 64 proteins: 64 x 512
residues and 64 mixed lengths of 128-1024 (synth.synth_lengths).  Per batch, in one process, warmed and synchronised:
  * ms of the pooled encode (get_protein_seq_embeddings: contacts off, the product path),
  * ms of get_amino_acid_embeddings with return_contacts=False and =True (per-residue rows copied out; maps in caller scratch),
  * from one timed call (opus_timing_get): the `contact` kernel class's ms, launches, algorithmic bytes and FLOPs - and the
    achieved TFLOP/s and GB/s of those launches - against the whole `encode` phase.
Prints ONE JSON line and writes it to profiles/contacts_bench.json.  bench.py is not involved and its line does not change.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "contacts_bench.json"))
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    cfg = opa.OpusConfig(**opa.config.esm2_dims("t33_650M"), proj_dim=256, dec_layers=1, dec_dim=256, dec_heads=4, dec_kv_heads=2,
                         dec_head_dim=64, dec_ffn=512, dec_vocab=512, max_batch=64, max_enc_tokens=1026, max_prompt=64,
                         max_new_tokens=8).validate()
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, contact_head=True), dev)
    enc = model.get_protein_encoder()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / args.steps

    out = {"shape": "esm2_t33_650M", "steps": args.steps}
    for tag, lens in (("b64x512", [512] * 64), ("b64_mixed", synth.synth_lengths(64, 128, 1024, seed=7))):
        seqs = [synth.synth_protein(n, i) for i, n in enumerate(lens)]
        r = {"residues": int(sum(lens))}
        r["pooled_ms"] = timed(lambda: enc.get_protein_seq_embeddings(seqs))
        r["per_residue_ms"] = timed(lambda: enc.get_amino_acid_embeddings(seqs))
        r["contacts_ms"] = timed(lambda: enc.get_amino_acid_embeddings(seqs, return_contacts=True))
        r["contacts_over_pooled"] = r["contacts_ms"] / r["pooled_ms"]
        model.timing(True)
        enc.get_amino_acid_embeddings(seqs, return_contacts=True)
        ms, n, by, fl = model.timing_get("contact", "encode")
        ms_enc = model.timing_get("*", "encode")[0]
        model.timing(False)
        r.update(contact_class_ms=ms, contact_launches=n, contact_bytes=by, contact_flops=fl, encode_phase_ms=ms_enc,
                 contact_tflops=fl / (ms * 1e-3) / 1e12 if ms else 0.0, contact_gbs=by / (ms * 1e-3) / 1e9 if ms else 0.0)
        out[tag] = r
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
