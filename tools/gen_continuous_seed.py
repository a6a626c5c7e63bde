"""Picks the prompt seeds of tests/test_gpu_continuous.py's end-to-end case on the CPU oracle, as gen_golden.py picks weight seeds:
for each decoder family the seed whose plain greedy run (batches of 4, the run-time EOS ids of continuous_checks.choose_eos) has
the largest share of decisive steps, ties broken by the larger smallest margin.  Prints the E2E_SEEDS table.

    python tools/gen_continuous_seed.py [n_seeds]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import opus_pllm_amd as opa                    # noqa: E402
from opus_pllm_amd import synth                # noqa: E402
import oracle                                  # noqa: E402
import continuous_checks as cc                 # noqa: E402


def plain_run(pipe, cfg, seed):
    prompts, seqs = cc.e2e_prompts(cfg, seed)
    free, marg = [], []
    for b0 in range(0, len(prompts), cc.E2E_SLOTS):
        ids, mask = cc.left_pad([p.tolist() for p in prompts[b0: b0 + cc.E2E_SLOTS]])
        ref, m, _ = pipe.generate(ids, seqs[b0: b0 + cc.E2E_SLOTS], mask, cc.E2E_MAX_NEW, (), cc.PAD)
        free.append(np.asarray(ref))
        marg.append(np.asarray(m))
    return np.concatenate(free), np.concatenate(marg)


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    table = {}
    for preset in ("micro_opt", "micro_qwen"):
        cfg = getattr(opa, preset)(max_batch=cc.E2E_SLOTS, max_prompt=cc.E2E_MAX_PROMPT, max_new_tokens=cc.E2E_S)
        pipe = oracle.OraclePipeline(cfg, synth.canonical_weights(cfg, 0))
        best = None
        for seed in range(n_seeds):
            free, marg = plain_run(pipe, cfg, seed)
            eos = cc.choose_eos(free)
            lens = cc.lengths_under(free, eos)
            checked, low = 0, np.inf
            for p, n in enumerate(lens):
                bad = np.flatnonzero(marg[p, :n] < cc.MARGIN_TAU)
                m = int(bad[0]) if len(bad) else n
                checked += m
                low = min(low, float(marg[p, :m].min()) if m else np.inf)
            frac = checked / sum(lens)
            print(f"{preset} seed {seed}: eos {eos} lengths {lens} decisive {frac:.4f} smallest checked margin {low:.3f}")
            key = (frac, len(set(lens)) >= 4, low)
            if best is None or key > best[0]:
                best = (key, seed, frac)
        table[preset] = (best[1], best[2])
    print("E2E_SEEDS =", table)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
