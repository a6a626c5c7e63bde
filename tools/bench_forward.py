#!/usr/bin/env python3
"""Teacher-forced scoring (OpusLlamaForCausalLM.forward(labels=...)) at the Llama-3-8B shape on one MI355X.

Synthetic fp16 weights, batch 64: each row holds the 8 protein tokens of one 512-residue protein (projected blocks, the
encoder is not part of this measurement), 96 prompt positions and 32 labelled answer tokens (T = 136, 64 x 32 = 2048 scored
targets minus the last position of each row).  Measured in one process on the same spliced embeddings:
  * ms per forward() loss-only (return_logits=False) and with return_logits=True,
  * ms per prefill_logits (what generate's prefill costs at the same shape),
  * per-phase and per-kernel-class time of one loss-only call (opus_timing_get),
  * lm_head-over-rows FLOP/s (the GEMMs of the `score` phase) and their share of the 2.5 PF dense peak,
  * NLL-kernel (`xent`) bytes/s on its algorithmic bytes (the fp16 logits once) - above the 8 TB/s HBM peak means the chunk's
    logits were read back from the Infinity Cache,
  * scored tokens/s, and the peak extra device memory of a loss-only call (torch.cuda.max_memory_allocated delta).
Prints ONE JSON line.  bench.py is not involved and its line does not change.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MFMA_PEAK_TFLOPS = 2500.0
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    B, N_PROMPT, N_ANS = args.batch, 96, 32
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=66, max_prompt=8 + N_PROMPT + N_ANS, max_new_tokens=16)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    # prompt = BOS + <seq> + text (96 positions after the splice), answer = 32 ids; training-mode splice (right padding)
    rows = []
    for i in range(B):
        p = synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=N_PROMPT + 1, seq_pos=1)
        a = synth.synth_prompt_ids(cfg.dec_vocab, 1000 + i, n_text=N_ANS, seq_pos=-1, bos=3)
        rows.append((p, a))
    ids = torch.tensor([p + a for p, a in rows])
    labels = torch.full_like(ids, -100)
    labels[:, -N_ANS:] = ids[:, -N_ANS:]
    g = torch.Generator(device=dev).manual_seed(0)
    prot = (torch.randn((B, cfg.n_prot_tokens, cfg.dec_dim), generator=g, device=dev) * 0.02).to(_cabi.operand_dtype())
    _, _, mask, _, emb, lab = model.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids, dtype=torch.bool), None,
                                                                         labels, (), inference_mode=False, protein_tokens=prot)
    T = emb.shape[1]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    loss_only = lambda: model(inputs_embeds=emb, attention_mask=mask, labels=lab, return_logits=False)   # noqa: E731
    with_logits = lambda: model(inputs_embeds=emb, attention_mask=mask, labels=lab, return_logits=True)  # noqa: E731
    prefill = lambda: model.prefill_logits(emb, mask)                                                     # noqa: E731
    ms_loss = timed(loss_only)
    ms_logits = timed(with_logits)
    ms_prefill = timed(prefill)
    n_tok = loss_only().n_tokens

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = loss_only()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - base
    del out

    model.timing(True)
    loss_only()
    classes, phases = model.timing_names()
    per_phase = {p: round(model.timing_get("*", p)[0], 4) for p in phases}
    per_class = {k: round(model.timing_get(k, "*")[0], 4) for k in classes}
    per_class_score = {k: round(model.timing_get(k, "score")[0], 4) for k in classes}
    gemm_ms = gemm_fl = 0.0
    for k in classes:
        if k.startswith("gemm_"):
            ms, _, _, fl = model.timing_get(k, "score")
            gemm_ms += ms
            gemm_fl += fl
    x_ms, x_n, x_by, _ = model.timing_get("xent", "score")
    model.timing(False)
    tflops = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms else 0.0
    print(json.dumps(dict(
        workload=f"forward(labels) Llama-3-8B fp16 synthetic, B={B}, T={T} (8 protein + {N_PROMPT} prompt + {N_ANS} answer)",
        scored_tokens=n_tok, steps=args.steps, warmup=args.warmup,
        ms_forward_loss_only=round(ms_loss, 3), ms_forward_return_logits=round(ms_logits, 3), ms_prefill_logits=round(ms_prefill, 3),
        loss_only_over_prefill=round(ms_loss / ms_prefill, 4),
        phase_ms=per_phase, class_ms=per_class, score_class_ms=per_class_score,
        lm_head_rows_ms=round(gemm_ms, 4), lm_head_rows_tflops=round(tflops, 1),
        lm_head_rows_peak_share=round(tflops / MFMA_PEAK_TFLOPS, 4),
        xent_ms=round(x_ms, 4), xent_launches=x_n, xent_gbs=round(x_by / (x_ms * 1e-3) / 1e9, 1) if x_ms else 0.0,
        xent_share_of_lm_head=round(x_ms / gemm_ms, 4) if gemm_ms else None,
        scored_tokens_per_s=round(n_tok / (ms_loss * 1e-3), 1),
        peak_extra_mib_loss_only=round(extra / 2 ** 20, 1),
        hbm_peak_gbs=HBM_PEAK_GBS, mfma_peak_tflops=MFMA_PEAK_TFLOPS,
    )))


if __name__ == "__main__":
    main()
