#!/usr/bin/env python3
"""Census of the encode / prefill / decode path: what it computes, bit for bit, and which kernels it launches, on one MI355X.

For every configuration below ONE JSON line with
  sha256    the SHA-256 of the raw bytes of every output of a plain run of the case (pooled embeddings, protein tokens, prefill
            logits, the logits of 3 decode steps, the ids of a 6-token greedy generate(); or the case's own outputs), and
  launches  the launch count per "kernel class/phase" of a repeat of the same calls in timing mode (model.timing(True);
            opus_timing_get over opus_timing_names).
A change of the host code between the launches (api.cpp: who asks which GEMM for which fusion, in which order) must leave every
line as it was: the kernels and their arguments are the same and every combine on the path has a fixed order, so a line that
differs is a wrong or lost request, not noise.  Run it on a build of the commit before such a change and on the build after it
(--lib picks the library; the Python side is this tree's both times) and compare the two files line by line:

    python tools/path_census.py --lib <parent build>/libopus_pllm.so --out profiles/<name>_parent.jsonl
    python tools/path_census.py --out profiles/<name>_head.jsonl

Configurations: the four micro models (Llama, OPT with GELU and ReLU, Qwen2 biases; head_dim 16: stand-alone rotary) at batch 1
and 3 with the padded and the packed encoder; the full-width two-layer model of tests/test_gpu_batch64.py (encoder 1280 / 20,
decoder 4096 / 32 / 8 / 128, FFN 14336, vocabulary 32768) on 64 proteins of 100-250 residues with the knobs no_ln_fusion and
misc7 at 0 and 1, at batch 1, 4, 5, 16, 17 and 64 (skinny; stream with one panel; stream with k-parts; QKV slabs summed by the
attention; tiled hand-offs), at batch 64 with no_stream = 1, forward(labels=...) on 2 rows, score_continuations() with 2 prefix
rows x 3 continuations of 4 tokens, generate(num_return_sequences=3) at batch 2; and a two-layer decoder of the Vicuna-13B width
(hidden 5120: the 5-panel stream plan) at batch 48, prefill + 1 decode step; and (--only heads) every mode of the head of the
decode step on the micro model at 3 rows and 6 new tokens: greedy and sampling (top-p, top-k), each with all per-step outputs, the
logits processors with and without outputs, a TokenTrie and a per-row one, guidance with and without token log-probs,
num_return_sequences=3, prefix=, a stop sequence, an EOS id, and generate_continuous() with a refill (plus its step and refill
counters).  The plain run of a case replays the captured step, the timing-mode run launches eagerly: both paths are covered.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", type=str, default=None, help="libopus_pllm.so to load instead of this tree's (OPUS_LIB_PATH)")
    ap.add_argument("--out", type=str, default=None, help="also write the lines to this file")
    ap.add_argument("--only", choices=["all", "micro", "full", "wide", "heads"], default="all")
    args = ap.parse_args()
    if args.lib:
        os.environ["OPUS_LIB_PATH"] = os.path.abspath(args.lib)
    sys.path.insert(0, ROOT)
    import torch
    import opus_pllm_amd as opa
    from opus_pllm_amd import _cabi, synth
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights

    dev = torch.device("cuda:0")
    lines = []

    def sha(t):
        return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def make(cfg):
        return OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)

    def knob(model, name, value):
        _cabi.check(_cabi.lib().opus_debug_knob(model._ctx, name.encode(), int(value)))

    def census(name, model, case, stats=()):
        """case() -> {output name: tensor}; run plainly for the hashes, once more in timing mode for the launch counts;
        stats: opus_stat counters read behind both runs"""
        hashes = {k: sha(v) for k, v in case().items()}
        torch.cuda.synchronize(dev)
        model.timing(True)
        case()
        torch.cuda.synchronize(dev)
        classes, phases = model.timing_names()
        launches = {}
        for k in classes:
            for p in phases:
                n = model.timing_get(k, p)[1]
                if n:
                    launches[f"{k}/{p}"] = int(n)
        model.timing(False)
        extra = dict(stats={k: model.stat(k) for k in stats}) if stats else {}
        line = json.dumps(dict(config=name, sha256=hashes, launches=launches, **extra), sort_keys=True)
        print(line, flush=True)
        lines.append(line)

    def path(model, seqs, ids, mask, pad, steps=3, new_tokens=6):
        """the product path stage by stage, then generate() on the same inputs"""
        def case():
            out = {}
            out["pooled"] = pooled = model.encode_seq2embedding(seqs)
            out["protein_tokens"] = prot = model.switch_projector_embedding(model.encode_projector_embedding(pooled))
            emb, m, _ = model._splice(ids, mask, prot, True)
            out["prefill_logits"] = lg = model.prefill_logits(emb, m)
            for s in range(steps):
                out[f"decode_logits_{s}"] = lg = model.decode_logits(lg.argmax(-1))
            if new_tokens:
                out["generate_ids"] = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, eos_token_id=[],
                                                     do_sample=False, max_new_tokens=new_tokens)
            return out
        return case

    def prompts(cfg, shapes, pad):
        """left-padded prompt rows of (text ids, placeholder position) each, and their mask"""
        rows = [synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=n, seq_pos=p) for i, (n, p) in enumerate(shapes)]
        width = max(len(r) for r in rows)
        ids = torch.full((len(rows), width), pad, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, width - len(r):] = torch.tensor(r)
        return ids, ids != pad

    if args.only in ("all", "micro"):
        for preset in ("micro", "micro_opt", "micro_opt_relu", "micro_qwen"):
            cfg = opa.PRESETS[preset]()
            model = make(cfg)
            for B in (1, 3):
                seqs = [synth.synth_protein(n, i) for i, n in enumerate((40, 21, 33)[:B])]
                ids, mask = prompts(cfg, ((14, 5), (9, 2), (11, 7))[:B], 2)
                for packed in (False, True):
                    model.packed_encoder = packed
                    census(f"{preset} B={B} {'packed' if packed else 'padded'}", model, path(model, seqs, ids, mask, 2))
            del model
            torch.cuda.empty_cache()

    if args.only in ("all", "full"):
        cfg = opa.OpusConfig(enc_layers=2, enc_dim=1280, enc_heads=20, enc_ffn=5120, proj_dim=5120,
                             dec_layers=2, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                             dec_vocab=32768, dec_rope_theta=500000.0, max_batch=64, max_enc_tokens=258, max_prompt=56,
                             max_new_tokens=8).validate()
        model = make(cfg)
        seqs = [synth.synth_protein(100 + (37 * i) % 150, i) for i in range(64)]
        ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=41, seq_pos=5) for i in range(64)])
        mask = torch.ones_like(ids, dtype=torch.bool)
        for no_ln in (0, 1):
            for misc7 in (0, 1):
                knob(model, "no_ln_fusion", no_ln)
                knob(model, "misc7", misc7)
                census(f"full B=64 no_ln_fusion={no_ln} misc7={misc7}", model, path(model, seqs, ids, mask, 0))
        knob(model, "no_ln_fusion", 0)
        knob(model, "misc7", 0)
        for B in (1, 4, 5, 16, 17, 64):
            census(f"full B={B} prefill+decode", model, path(model, seqs[:B], ids[:B], mask[:B], 0, new_tokens=0))
        knob(model, "no_stream", 1)
        census("full B=64 no_stream=1", model, path(model, seqs, ids, mask, 0, new_tokens=0))
        knob(model, "no_stream", 0)

        labels = ids[:2].clone()
        labels[:, :20] = -100

        def forward():
            r = model(input_ids=ids[:2], attention_mask=mask[:2], seq=seqs[:2], labels=labels, return_logits=True)
            return dict(loss=r.loss, logits=r.logits, token_logprobs=r.token_logprobs)
        census("full forward(labels) B=2", model, forward)

        conts = torch.tensor([[(7 + 13 * r + 5 * j) % cfg.dec_vocab for j in range(4)] for r in range(6)])

        def continuations():
            prefix = model.cache_prefix(ids[:2], seqs[:2], attention_mask=mask[:2])
            r = model.score_continuations(prefix, conts, prefix_rows=[0, 0, 0, 1, 1, 1])
            return dict(token_logprobs=r.token_logprobs, logprob=r.logprob)
        census("full score_continuations 2 x 3 x 4", model, continuations)

        def nret():
            return dict(generate_ids=model.generate(ids[:2], seqs[:2], attention_mask=mask[:2], pad_token_id=0, eos_token_id=[],
                                                    do_sample=True, temperature=0.7, top_p=0.9, seed=11, num_return_sequences=3,
                                                    max_new_tokens=6))
        census("full generate(num_return_sequences=3) B=2", model, nret)
        del model
        torch.cuda.empty_cache()

    if args.only in ("all", "wide"):
        cfg = opa.vicuna_13b(enc_layers=2, enc_dim=1280, enc_heads=20, enc_ffn=5120, proj_dim=5120, dec_layers=2, max_batch=48,
                             max_enc_tokens=130, max_prompt=56, max_new_tokens=8)
        model = make(cfg)
        seqs = [synth.synth_protein(60 + (11 * i) % 60, 300 + i) for i in range(48)]
        ids = torch.tensor([synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=41, seq_pos=5) for i in range(48)])
        census("vicuna_13b-width decoder B=48 prefill+decode", model,
               path(model, seqs, ids, torch.ones_like(ids, dtype=torch.bool), 0, steps=1, new_tokens=0))
        del model
        torch.cuda.empty_cache()

    if args.only in ("all", "heads"):
        cfg = opa.micro(max_batch=12, max_new_tokens=24)       # (9 rows for num_return_sequences, a session of 4 budgets)
        model = make(cfg)
        seqs = [synth.synth_protein(n, i) for i, n in enumerate((40, 21, 33))]
        ids, mask = prompts(cfg, ((14, 5), (9, 2), (11, 7)), 2)
        base = dict(attention_mask=mask, pad_token_id=2, eos_token_id=[], max_new_tokens=6)
        samp = dict(do_sample=True, temperature=0.8, seed=5)
        outs = dict(return_dict_in_generate=True, output_scores=True, output_logits=True, output_token_logprobs=True)

        def gen(inputs=ids, proteins=seqs, **kw):
            def case():
                r = model.generate(inputs, proteins, **{**base, **kw})
                if torch.is_tensor(r):
                    return dict(generate_ids=r)
                out = dict(generate_ids=r.sequences)
                for k in ("scores", "logits"):
                    if getattr(r, k, None) is not None:
                        out[k] = torch.stack(list(getattr(r, k)))
                for k in ("token_logprobs", "logprob", "n_tokens"):
                    if getattr(r, k, None) is not None:
                        out[k] = torch.as_tensor(getattr(r, k))
                return out
            return case

        plain = model.generate(ids, seqs, **base).cpu()
        procs = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[int(plain[0, 0])], [int(plain[1, 1]), int(plain[1, 2])]],
                     min_new_tokens=3, eos_token_id=[int(plain[2, 1])])
        trie = lambda k: opa.TokenTrie([[5 + k, 6, 7], [5 + k, 8], [9, 10 + k, 11, 12]], end_token_id=3)   # noqa: E731
        head = torch.tensor(synth.synth_prompt_ids(cfg.dec_vocab, 9, n_text=8, seq_pos=3))
        tails = torch.tensor([[(7 + 13 * r + 5 * j) % cfg.dec_vocab for j in range(5)] for r in range(3)])
        for name, case in (
                ("greedy", gen()),
                ("sampling top_p=0.9", gen(top_p=0.9, top_k=0, **samp)),
                ("sampling top_k=5", gen(top_k=5, **samp)),
                ("greedy + outputs", gen(**outs)),
                ("sampling top_p=0.9 + outputs", gen(top_p=0.9, top_k=0, **samp, **outs)),
                ("processors", gen(**procs)),
                ("processors + token_logprobs + logits", gen(return_dict_in_generate=True, output_token_logprobs=True,
                                                             output_logits=True, **procs)),
                ("TokenTrie", gen(eos_token_id=[3], prefix_allowed_tokens_fn=trie(0))),
                ("TokenTrie.per_row", gen(eos_token_id=[3], prefix_allowed_tokens_fn=opa.TokenTrie.per_row([trie(k) for k in range(3)]))),
                ("guidance_scale=1.5", gen(guidance_scale=1.5)),
                ("guidance_scale=1.5 + token_logprobs", gen(guidance_scale=1.5, return_dict_in_generate=True,
                                                            output_token_logprobs=True)),
                ("sampling num_return_sequences=3", gen(num_return_sequences=3, top_p=0.9, **samp)),
                ("prefix= with prefix_rows", lambda: gen(tails, None, attention_mask=None, prefix_rows=[1, 0, 1],
                                                         prefix=model.cache_prefix(torch.stack([head, head]), seq=seqs[:2],
                                                                                   detach=True))()),
                ("stop sequence", gen(stop_sequence=[int(plain[0, 1]), int(plain[0, 2])])),
                ("eos_token_id", gen(eos_token_id=[int(plain[0, 1]), int(plain[1, 0]), int(plain[2, 1])]))):    # (every row ends by step 1)
            census(f"heads {name}", model, case)

        queue = [torch.tensor(synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=8 + i, seq_pos=2)) for i in range(7)]
        qseqs = [synth.synth_protein(20 + 3 * i, 50 + i) for i in range(7)]

        def continuous():
            r = model.generate_continuous(queue, qseqs, max_new_tokens=6, eos_token_id=[int(plain[0, 2]), int(plain[1, 3])],
                                          pad_token_id=2, slots=3, refill_min=1, return_dict_in_generate=True)
            return dict(sequences=torch.cat(r.sequences), n_tokens=r.n_tokens)
        census("heads generate_continuous 7 prompts on 3 rows", model, continuous, stats=("stream_steps", "stream_refills"))
        del model
        torch.cuda.empty_cache()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
