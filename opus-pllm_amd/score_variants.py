#!/usr/bin/env python3
"""Variant-effect scoring driver: the ESM-2 masked-LM head over one sequence or a FASTA file, as fair-esm's
examples/variant-prediction/predict.py scores ("wt-marginals", "masked-marginals").

  python opus-pllm_amd/score_variants.py --model-base-path <hf dir | synthetic:c1_tiny> --sequence MKT... \\
      --mutations muts.txt --mode masked-marginals --save_path out.json

--mutations names a file with one mutation per line ("A23G", or "A23G:L40P" for a multiple mutation, scored as the sum of its
parts; positions count from --offset-idx, 1 by default); every line is scored against every protein of the input.  Without it
the output holds, per protein, the full table scores[j][a] = log p(a at j) - log p(wild type at j) over the 20 standard residues
(columns "ACDEFGHIKLMNPQRSTVWY").  Either way each protein carries its pseudo-perplexity.  A mutation that does not fit its
protein ends the run with the message and a non-zero exit status; nothing is written.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opus_pllm_amd.alphabet import STANDARD_RESIDUES, STANDARD_RESIDUE_IDS      # noqa: E402
from opus_pllm_amd.mlm import MODES                                             # noqa: E402


def read_fasta(path: str):
    names, seqs = [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                names.append(line[1:].split()[0] if len(line) > 1 else f"protein{len(names)}")
                seqs.append("")
            elif not names:
                raise ValueError(f"{path}: sequence data before the first '>' header")
            else:
                seqs[-1] += line
    return names, seqs


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model-base-path", type=str, default="synthetic:c1_tiny")
    p.add_argument("--opus-pllm-weights-path", type=str, default=None)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--sequence", type=str)
    g.add_argument("--fasta", type=str)
    p.add_argument("--mutations", type=str, default=None, help="file with one mutation per line")
    p.add_argument("--mode", type=str, default="masked-marginals", choices=MODES)
    p.add_argument("--offset-idx", type=int, default=1)
    p.add_argument("--max_batch", type=int, default=None)
    p.add_argument("--max_residues", type=int, default=None)
    p.add_argument("--save_path", type=str, required=True)
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from opus_pllm_amd.builder import load_pretrained_model
    names, seqs = (["sequence"], [args.sequence]) if args.sequence is not None else read_fasta(args.fasta)
    muts = None
    if args.mutations:
        with open(args.mutations) as f:
            muts = [l.strip() for l in f if l.strip()]
    cap = {}
    if args.max_batch:
        cap["max_batch"] = args.max_batch
    need = max((len(s) for s in seqs), default=0) + 2
    synthetic = args.model_base_path.startswith("synthetic:")
    if args.max_residues or synthetic:
        cap["max_enc_tokens"] = max((args.max_residues or 0) + 2, need, 3)
    extra = {"mlm_head": True} if synthetic else {}
    _, model, _ = load_pretrained_model(args.model_base_path, args.opus_pllm_weights_path, "opus-pllm", **cap, **extra)
    enc = model.get_protein_encoder()
    res = enc.score_mutations(list(zip(names, seqs)), mutations=None if muts is None else [muts] * len(seqs), mode=args.mode,
                              offset_idx=args.offset_idx)
    out = {"mode": args.mode, "offset_idx": args.offset_idx, "encoder_calls": res.encoder_calls, "rows_evaluated": res.rows_evaluated,
           "proteins": []}
    for i, (name, s) in enumerate(zip(names, seqs)):
        p = {"name": name, "length": int(res.log_probs[i].shape[0]), "pseudo_perplexity": float(res.pseudo_perplexity[i]),
             "pseudo_log_likelihood": float(res.pseudo_log_likelihood[i])}
        if muts is None:
            p["columns"] = STANDARD_RESIDUES
            p["scores"] = res.scores[i][:, STANDARD_RESIDUE_IDS].cpu().tolist()
        else:
            p["mutations"] = {m: float(v) for m, v in zip(muts, res.mutation_scores[i].cpu())}
        out["proteins"].append(p)
    with open(args.save_path, "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except ValueError as e:           # a mutation string that does not fit its protein, an unknown mode ...
        sys.exit(f"score_variants: {e}")
