"""Quantised decoder weights: decode-phase time of an unquantised, an FP8 and an MXFP4 model, alternating in one process.

    python tools/bench_wq.py [--formats fp16,fp8,mxfp4] [--model llama3_8b] [--batches 1,16,64] [--new-tokens 32,128] [--reps 3]
                             [--out profiles/wq_bench.json]

--formats: the models that take turns (fp16 is always one of them); `fp16,fp8` leaves the MXFP4 model and its keys out.

Synthetic weights, random prompt embeddings of --prompt positions, greedy, no stop id.  Per (batch, new tokens):
  decode_ms        wall time of generate (prefill + captured decode steps) at N new tokens minus its wall time at 1 new token,
                   median over --reps rounds (at least 3), the models taking turns round by round; min / max of the same
                   difference
  per_class_ms     opus_timing of one eager run: kernel time per class in the decode phase
  ratio_*          decode_ms against the fp16 model's, beside the fp16 figure's own run-to-run spread
  mxfp4_below_fp8_by_3_spreads   THE condition of the format at batch 1: the MXFP4 decode phase is below the FP8 model's by more
                   than three times the fp16 spread of the same run (reported for every cell, whichever way it falls; needs
                   both quantised models)
and the bytes the models hold.  From bytes alone (derived, not a target): the layer GEMMs stream 0.266 of fp16; lm_head and the
fixed cost per launch do not shrink - about 0.5 - 0.6 of the fp16 decode phase at batch 1.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import opus_pllm_amd as opa  # noqa: E402
from opus_pllm_amd import _cabi  # noqa: E402
from opus_pllm_amd.model import OpusLlamaForCausalLM  # noqa: E402
from opus_pllm_amd.weights import DeviceWeights  # noqa: E402

FORMATS = {"fp16": None, "fp8": "fp8", "mxfp4": "mxfp4"}


def wall_ms(model, emb, mask, n_new):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model._greedy(emb, mask, n_new, [], 0)
    torch.cuda.synchronize()
    assert out.shape[1] == n_new
    return (time.perf_counter() - t0) * 1e3


def per_class(model, emb, mask, n_new):
    classes, _ = model.timing_names()
    model.timing(True)
    model._greedy(emb, mask, n_new, [], 0)
    torch.cuda.synchronize()
    out = {k: round(model.timing_get(k, "decode")[0], 4) for k in classes if model.timing_get(k, "decode")[1]}
    model.timing(False)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--formats", default="fp16,fp8,mxfp4")
    p.add_argument("--model", default="llama3_8b")
    p.add_argument("--batches", default="1,16,64")
    p.add_argument("--new-tokens", default="32,128")
    p.add_argument("--prompt", type=int, default=96)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--layers", type=int, default=0, help="decoder layers (0: the preset's)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "wq_bench.json"))
    a = p.parse_args()
    assert a.reps >= 3, "medians of at least three rounds"
    formats = {k: FORMATS[k] for k in a.formats.split(",")}
    assert "fp16" in formats, "the ratios are against the fp16 model"
    batches = [int(x) for x in a.batches.split(",")]
    news = [int(x) for x in a.new_tokens.split(",")]
    dev = torch.device("cuda:0")
    kw = dict(max_batch=max(batches), max_enc_tokens=66, max_prompt=a.prompt, max_new_tokens=max(news))
    if a.layers:
        kw["dec_layers"] = a.layers
    cfg = opa.PRESETS[a.model](**kw)
    models = {k: OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, decoder_weights=f), dev) for k, f in formats.items()}
    res = {"model": a.model, "dec_layers": cfg.dec_layers, "operand_dtype": "bf16" if _cabi.BF16 else "fp16", "prompt": a.prompt,
           "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "nbytes": {k: m.weights.nbytes() for k, m in models.items()},
           "decoder_weight_format": {k: m.decoder_weight_format for k, m in models.items()},
           "expected_ratio_derived_unmeasured": {"batch_1": "0.5-0.6"},
           "runs": []}
    g = torch.Generator().manual_seed(0)
    for B in batches:
        emb = (torch.randn(B, a.prompt, cfg.dec_dim, generator=g) * 0.05).to(_cabi.operand_dtype()).to(dev)
        mask = torch.ones(B, a.prompt, dtype=torch.bool, device=dev)
        for N in news:
            for m in models.values():                                  # capture the decode graphs, warm the caches
                wall_ms(m, emb, mask, 1), wall_ms(m, emb, mask, N)
            t1 = {k: [] for k in models}
            tn = {k: [] for k in models}
            for _ in range(a.reps):
                for k, m in models.items():
                    t1[k].append(wall_ms(m, emb, mask, 1))
                    tn[k].append(wall_ms(m, emb, mask, N))
            run = {"batch": B, "new_tokens": N}
            for k, m in models.items():
                base = statistics.median(t1[k])
                d = [t - base for t in tn[k]]
                counters = [c for c, f in (("w8_gemms", "fp8"), ("w4_gemms", "mxfp4")) if f in formats]
                n0, s0 = [m.stat(c) for c in counters], m.stat("decode_steps")
                run[k] = {"decode_ms": round(statistics.median(d), 4), "decode_ms_min": round(min(d), 4), "decode_ms_max": round(max(d), 4),
                          "ms_per_step": round(statistics.median(d) / (N - 1), 5), "prefill_plus_first_token_ms": round(base, 4),
                          "per_class_ms": per_class(m, emb, mask, N)}
                steps = max(1, m.stat("decode_steps") - s0)             # (the eager run issues every step)
                for c, n in zip(counters, n0):
                    run[k][c + "_per_step"] = (m.stat(c) - n) // steps
            f16 = run["fp16"]
            for k in formats:
                if k != "fp16":
                    run["ratio_" + k] = round(run[k]["decode_ms"] / f16["decode_ms"], 4)
            run["fp16_spread_ms"] = round(f16["decode_ms_max"] - f16["decode_ms_min"], 4)
            if "fp8" in formats and "mxfp4" in formats:
                run["mxfp4_below_fp8_ms"] = round(run["fp8"]["decode_ms"] - run["mxfp4"]["decode_ms"], 4)
                run["mxfp4_below_fp8_by_3_spreads"] = bool(run["mxfp4_below_fp8_ms"] > 3 * run["fp16_spread_ms"])
            print(json.dumps(run))
            res["runs"].append(run)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
