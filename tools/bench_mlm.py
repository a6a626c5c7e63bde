#!/usr/bin/env python3
"""The ESM-2 masked-LM head at the ESM-2 650M shape on one MI355X (synthetic weights, a token decoder).

Two runs, each against what a user could do without the head's entry points - get_amino_acid_embeddings (every state of every
token copied out) followed by the head in torch fp32 on the GPU, from the same head tensors:
  (a) masked_scan   masked-marginals of ONE protein of --residues residues: that many masked copies, --batch per encoder call,
                    the head on one gathered row per copy (the baseline also applies its head to that one row per copy)
  (b) wt_marginals  wt-marginals of --batch proteins of --residues residues: one encoder call, the head on every residue row
Settings alternate within a round.  Per run: median / min / max ms of both, their ratio, the largest difference of the
log-probabilities, and from timing mode (one extra call) the share of the call's kernel time that the head takes: the launches
of class "mlm" (row gather, LayerNorm + 33 columns) and the whole head (those plus the dense step's GEMM), recorded by running the
head alone once more on the rows of one call.  Prints ONE JSON line and writes it to profiles/mlm_bench.json.  bench.py is not involved.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--residues", type=int, default=512)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mlm_bench.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    B, n = args.batch, args.residues
    cfg = opa.OpusConfig(**opa.config.esm2_dims("t33_650M"), proj_dim=256, dec_layers=1, dec_dim=256, dec_heads=4, dec_kv_heads=2,
                         dec_head_dim=64, dec_ffn=512, dec_vocab=512, max_batch=B, max_enc_tokens=n + 2, max_prompt=64,
                         max_new_tokens=8).validate()
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, mlm_head=True), dev)
    enc = model.get_protein_encoder()
    head = {k: torch.from_numpy(v).to(dev) for k, v in synth.mlm_head(cfg, 0).items()}
    emb = model.weights.tensors["enc.emb"].float()

    def torch_head(h):                       # fp32, the libraries' RobertaLMHead / EsmLMHead
        y = F.gelu(F.linear(h, head["enc.lm.dense.weight"], head["enc.lm.dense.bias"]))
        y = F.layer_norm(y, (cfg.enc_dim,), head["enc.lm.ln.weight"], head["enc.lm.ln.bias"], cfg.enc_ln_eps)
        return torch.log_softmax(F.linear(y, emb, head["enc.lm.bias"]), -1)

    seqs = [synth.synth_protein(n, i) for i in range(B)]
    copies = [seqs[0][:j] + "<mask>" + seqs[0][j + 1:] for j in range(n)]

    def scan_ours():
        return enc.score_mutations([seqs[0]], mode="masked-marginals").log_probs[0]

    def scan_base():
        rows = []
        for i0 in range(0, n, B):
            embs = enc.get_amino_acid_embeddings(copies[i0:i0 + B])
            rows.append(torch_head(torch.stack([e[i0 + k] for k, e in enumerate(embs)])))
        return torch.cat(rows)

    def wt_ours():
        return torch.cat(enc.score_mutations(seqs, mode="wt-marginals").log_probs)

    def wt_base():
        return torch_head(torch.cat(enc.get_amino_acid_embeddings(seqs)))

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def kernel_ms(fn):
        model.timing(True)
        fn()
        torch.cuda.synchronize(dev)
        total, mlm = model.timing_get("*")[0], model.timing_get("mlm")
        model.timing(False)
        return total, mlm[0], int(mlm[1])

    res = {"shape": "esm2_t33_650M", "batch": B, "residues": n, "rounds": args.rounds, "operand_dtype": "bf16" if _cabi.BF16 else "fp16"}
    runs = {"masked_scan": (scan_ours, scan_base), "wt_marginals": (wt_ours, wt_base)}
    for name, (ours, base) in runs.items():
        ms = {"ours": [], "baseline": []}
        diff = 0.0
        for r in range(args.warmup + args.rounds):
            ta, a = timed(ours)
            tb, b = timed(base)
            diff = max(diff, float((a - b).abs().max()))
            if r >= args.warmup:
                ms["ours"].append(ta)
                ms["baseline"].append(tb)
            del a, b
            torch.cuda.empty_cache()
        m = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}
        m["baseline_over_ours"] = m["baseline"]["ms_median"] / m["ours"]["ms_median"]
        m["max_abs_diff_log_probs"] = diff
        total, mlm_ms, mlm_n = kernel_ms(ours)
        # the head alone (gather, dense GEMM, LayerNorm + columns) on the rows of one call, recorded apart from the encoder
        R = B if name == "masked_scan" else B * n
        idx = torch.arange(R, dtype=torch.int32, device=dev)
        out = torch.empty((R, cfg.enc_vocab), dtype=torch.float32, device=dev)
        head_ms = kernel_ms(lambda: _cabi.check(model._lib.opus_esm2_lm_head(model._ctx, idx.data_ptr(), R, 1, out.data_ptr(),
                                                                             torch.cuda.current_stream(dev).cuda_stream)))[0]
        head_ms *= mlm_n // 2                 # (two "mlm" launches per head call)
        m["kernel_ms"] = {"call": total, "mlm_class": mlm_ms, "mlm_launches": mlm_n, "head": head_ms,
                          "head_share": head_ms / total, "mlm_class_share": mlm_ms / total}
        res[name] = m
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
