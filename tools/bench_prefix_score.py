#!/usr/bin/env python3
"""Shared-prefix scoring (cache_prefix + score_continuations) against forward(labels) on the concatenated rows, at the Llama-3-8B
shape on one MI355X.

Synthetic fp16 weights.  B = 64 prompts of 8 protein tokens (projected blocks passed as protein_tokens=, so the encoder is outside
both sides) + 96 text positions, K = 4 continuations of 6 tokens per prompt (256 rows).  Measured in one process, both sides
warmed and synchronised:
  * ms of cache_prefix + score_continuations (the prompt prefilled once, the 256 continuations behind it),
  * ms of forward(labels, return_logits=False) on the 256 concatenated prompt + continuation rows (spliced beforehand, outside
    the timing: the training-mode splice takes max_batch rows per call),
  * their ratio, the largest |difference| of a continuation token's log-prob between the two,
  * per-phase time of one prefix + score call and the attn_prefill-class time inside the `score` phase (opus_timing_get).
Prints ONE JSON line and writes it to profiles/prefix_scoring_bench.json.  bench.py is not involved and its line does not change.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "prefix_scoring_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    B, K, N_PROMPT, N_CONT = 64, 4, 96, 6
    cfg = opa.llama3_8b(max_batch=B, max_enc_tokens=66, max_prompt=8 + N_PROMPT + N_CONT, max_new_tokens=16)
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    # prompt = BOS + <seq> + text: 8 protein + 96 text positions after the splice; 4 continuations of 6 ids per prompt
    prompts = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=N_PROMPT + 1, seq_pos=1) for i in range(B)])
    rng = np.random.default_rng(0)
    conts = torch.from_numpy(rng.integers(3, cfg.dec_vocab, (B * K, N_CONT)))
    src = torch.arange(B).repeat_interleave(K)
    g = torch.Generator(device=dev).manual_seed(0)
    prot = (torch.randn((B, cfg.n_prot_tokens, cfg.dec_dim), generator=g, device=dev) * 0.02).to(_cabi.operand_dtype())
    # the concatenations: every prompt K times, its continuation behind it, labels on the continuation
    cat_ids = torch.cat([prompts[src], conts], dim=1)
    cat_lab = torch.full_like(cat_ids, -100)
    cat_lab[:, -N_CONT:] = conts
    prot_rows = prot[src.to(dev)].contiguous()
    # (the training-mode splice takes max_batch rows per call: the concatenations are spliced once here, in groups, outside the
    # timing - forward's side is then timed from its embeddings, the prefix side includes its 64-row splice)
    embs, masks, labs = [], [], []
    for g0 in range(0, B * K, B):
        _, _, m, _, e, lb = model.prepare_inputs_labels_for_multimodal(
            cat_ids[g0:g0 + B], None, torch.ones_like(cat_ids[g0:g0 + B], dtype=torch.bool), None, cat_lab[g0:g0 + B], (),
            inference_mode=False, protein_tokens=prot_rows[g0:g0 + B])
        embs.append(e)
        masks.append(m)
        labs.append(lb)
    cat_emb, cat_mask, cat_lab = torch.cat(embs), torch.cat(masks), torch.cat(labs)

    def prefix_path():
        p = model.cache_prefix(prompts, protein_tokens=prot)
        return model.score_continuations(p, conts, prefix_rows=src)

    def forward_path():
        return model(inputs_embeds=cat_emb, attention_mask=cat_mask, labels=cat_lab, return_logits=False)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    ms_prefix = timed(prefix_path)
    ms_forward = timed(forward_path)
    a = prefix_path().token_logprobs
    f = forward_path().token_logprobs
    T = f.shape[1]
    d_lp = float((a.double() - f[:, T - N_CONT:].double()).abs().max())

    model.timing(True)
    prefix_path()
    classes, phases = model.timing_names()
    per_phase = {p: round(model.timing_get("*", p)[0], 4) for p in phases}
    attn_score = model.timing_get("attn_prefill", "score")
    model.timing(False)
    out = dict(
        workload=f"Llama-3-8B fp16 synthetic: B={B} prompts x (8 protein + {N_PROMPT} text), K={K} continuations of {N_CONT} tokens",
        steps=args.steps, warmup=args.warmup,
        ms_prefix_plus_score=round(ms_prefix, 3), ms_forward_concat=round(ms_forward, 3),
        speedup=round(ms_forward / ms_prefix, 3), max_abs_token_logprob_diff=d_lp,
        prefix_path_phase_ms=per_phase,
        score_attn_prefill_ms=round(attn_score[0], 4), score_attn_prefill_launches=attn_score[1],
    )
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
