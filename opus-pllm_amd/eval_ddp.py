#!/usr/bin/env python3
"""Batch annotation driver: the MI355X-native counterpart of eval/run_opus_ddp.py (same flags, same flow).

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
      opus-pllm_amd/eval_ddp.py --model-base-path <hf dir | synthetic:llama3_8b> \\
      --opus-pllm-weights-path <adapter dir> --input_path data.json --save_path out.json

Flow (run_opus_ddp.py:47-148): load -> read JSON -> contiguous split over ranks -> batches of 8 -> prompt ->
tokenizer_seq_token -> left-pad -> generate -> decode, cut at '###' -> gather in rank order -> rank 0 saves.
`--use_input_embed` consumes the `.jsonl` written by `generate_esm_embedding.py`: the shard's embeddings go
through the modality projectors ONCE at M = shard size (>= 512: MFMA-bound GEMMs), decode batches consume the protein tokens.
Differences, all deliberate: the gather moves token ids
(int tensor all-gather over RCCL) instead of pickled strings, task metrics (metrics_computing_opi.py) are not run.

`--allowed_terms FILE --rank_terms K [--rank_with_stop]` (not in the reference): no generation.  Each batch's prompts are prefilled
once (cache_prefix), the trie of the allowed terms is scored behind them in one tree pass (score_trie) and every saved item carries
`"ranked_terms": [[term, logprob], ...]`, its K most probable terms (`generated` is the first of them): the per-term scores that
function prediction is evaluated with.  --rank_with_stop adds the log-probability of ending the answer right behind the term.
`--allowed_terms FILE --search_terms K [--search_top N] [--rank_with_stop]` writes the same `ranked_terms` from a beam search over
the terms (search_trie, K beams per prompt, the N <= K best kept): approximate - a term whose first ids fall out of the beam is
missed - and much cheaper on a vocabulary of tens of thousands of terms; on a small one --rank_terms is exact and about as fast.
The two flags exclude each other.

`--num_return_sequences N` (the reference's eval/eval_total_ablation.sh samples every dataset five times, one whole run per repeat):
N answers per item from ONE run - a call takes batch_size // N prompts, encodes and prefills them once and decodes batch_size rows
(generate(num_return_sequences=N)); every saved item carries its N answers as `"generated_all"` beside `"generated"`, which keeps
the first.  With N = 1 the output file is what it was.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opus_pllm_amd as opa                                                    # noqa: E402
from opus_pllm_amd import dist as odist                                        # noqa: E402
from opus_pllm_amd.builder import load_pretrained_model, return_cstp_path      # noqa: E402
from opus_pllm_amd.prompt import (add_constraint_args, add_logits_processor_args, add_lookup_args, after_process_output,  # noqa: E402
                                  build_prompt, logits_processor_kwargs, lookup_kwargs, max_new_tokens_for, token_constraint, add_warper_args,
                                  warper_kwargs)


def annotate(model, tokenizer, items, input_path, batch_size, max_new, temperature=0.0, top_p=0.7, num_beams=1,
             use_input_embed=False, device=None, logits_out=None, stop_sequence=None, inflight=1, logprobs_out=None,
             processors=None, num_return_sequences=1, share_prompt_head=False, guidance_scale=None, top_logprobs_out=None,
             top_k=0):
    """The batch loop of run_opus_ddp.py:88-134 over this rank's items -> [n, max_new] new ids (rows padded with eos).

    use_input_embed (two-stage pipeline): the `input_embed` vectors of the WHOLE shard go through the modality
    projectors once, at M = len(items) (model.project_dataset), and the decode batches consume the stored protein tokens;
    without it every batch encodes and projects its own proteins, as the reference does.
    logits_out (a list, --dump_logits): receives the fp32 [b, V] logits of each batch's last decode step (model.last_logits).
    logprobs_out (a list, --save_logprobs): receives ([n, max_new] fp32 token log-probabilities, 0 after a row's end, [n] counted
    positions) - generate(return_dict_in_generate=True, output_token_logprobs=True).
    top_logprobs_out (a list, --save_top_logprobs K = top_k): receives ([n, max_new, K] int64 ids, -1 after a row's end,
    [n, max_new, K] fp32 log-probabilities, [n] counted positions): the K likeliest tokens of every step's raw distribution -
    generate(top_logprobs=K).
    inflight (--inflight): batches in flight on this GPU.  The reference's loop is strictly sequential; with n > 1, n contexts
    that share the model's weights (model.new_context()) take the batches round-robin from n host threads - batches are
    independent, results come back in input order and are the same ids as with one context: greedy ids because the kernels are
    the same, sampled ids because every batch's sampler seed is drawn HERE, in input order, from torch's global generator
    (torch.manual_seed reproduces a run whatever `inflight` is) and handed to generate(seed=...).
    processors (--repetition_penalty / --no_repeat_ngram_size / --min_new_tokens, --allowed_terms): generate() keywords of its
    logits processors and of the token constraint (prefix_allowed_tokens_fn: one TokenTrie, built once, for every batch).
    num_return_sequences = N > 1 (--num_return_sequences): a call takes batch_size // N prompts and returns N rows for each
    (generate(num_return_sequences=N): one encode and one prefill per prompt); the result is [n N, max_new], item i's answers in
    rows i N .. i N + N - 1, and the other outputs have n N rows too.
    share_prompt_head (--share_prompt_head): the longest leading id run that all the shard's prompts share in front of their
    first placeholder (build_prompt's system text: tokenizer_seq_token tokenises it on its own, so the ids are identical) is
    prefilled ONCE as a detached one-row prefix (cache_prefix(detach=True)) and every batch is generated behind it
    (generate(prefix=...)): only the rest of each prompt is prefilled.  Other launch shapes than the plain call, so opt-in.
    guidance_scale = g (--guidance_scale; None or 1: off): classifier-free guidance against each prompt's protein-free twin
    (generate(guidance_scale=g)); a call takes batch_size // 2 prompts, whose negative rows fill the other half of the batch."""
    dev = device or model.device
    nret = int(num_return_sequences)
    if nret < 1:
        raise ValueError(f"--num_return_sequences has to be at least 1 (got {nret})")
    if nret > 1:
        batch_size = prompts_per_call(batch_size, nret)
    guided = guidance_scale is not None and float(guidance_scale) != 1.0
    if guided:
        batch_size = prompts_per_call(batch_size, 2)
    prot_all = None
    if use_input_embed and items:
        prot_all = model.project_dataset(torch.tensor([q["input_embed"] for q in items], dtype=torch.float32, device=dev))
    starts = list(range(0, len(items), batch_size))
    head_len, head = 0, None
    if share_prompt_head and items:
        head_len = shared_head_length([opa.tokenizer_seq_token(build_prompt(q["instruction"], input_path), tokenizer,
                                                               opa.DEFAULT_SEQ_TOKEN_INDEX) for q in items])
        if head_len:
            first = opa.tokenizer_seq_token(build_prompt(items[0]["instruction"], input_path), tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX)
            with torch.inference_mode():
                head = model.cache_prefix(torch.tensor([list(first[:head_len])], dtype=torch.long, device=dev), detach=True)
    outs = [None] * len(starts)
    last = [None] * len(starts)
    lps = [None] * len(starts)
    tops = [None] * len(starts)
    want_dict = logprobs_out is not None or top_logprobs_out is not None
    # one sampler seed per batch, drawn in input order before any worker thread starts (generate() would otherwise draw it from
    # the global generator at call time: with two threads racing, which batch got which seed depended on thread scheduling)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in starts] if temperature > 0 else [None] * len(starts)

    def one(m, j):
        i = starts[j]
        batch = items[i:i + batch_size]
        prompts = [build_prompt(q["instruction"], input_path) for q in batch]
        ids = [opa.tokenizer_seq_token(p, tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX, return_tensors="pt").to(dev)[head_len:] for p in prompts]
        ids = opa.left_pad_sequence(ids, padding_value=tokenizer.pad_token_id, batch_first=True)
        mask = ids != tokenizer.pad_token_id
        extra = {} if prot_all is None else {"protein_tokens": prot_all[i:i + len(batch)]}
        extra.update(processors or {})
        if head is not None:                             # every row behind the one cached head (a detached handle: any context)
            extra.update(prefix=head, prefix_rows=[0] * len(batch))
        if nret > 1:
            extra["num_return_sequences"] = nret
        if guided:
            extra["guidance_scale"] = float(guidance_scale)
        if want_dict:                                    # (the counted positions come with the token log-probabilities)
            extra.update(return_dict_in_generate=True, output_token_logprobs=True)
        if top_logprobs_out is not None:
            extra["top_logprobs"] = int(top_k)
        with torch.inference_mode():
            out = m.generate(ids, [q["input"] for q in batch], attention_mask=mask, pad_token_id=tokenizer.eos_token_id,
                             do_sample=temperature > 0, temperature=temperature, top_p=top_p,
                             num_beams=num_beams, max_new_tokens=max_new, use_cache=True, stop_sequence=stop_sequence,
                             seed=seeds[j], **extra)
        if top_logprobs_out is not None:
            n = out.top_ids.shape[1]
            tid = torch.full((out.sequences.shape[0], max_new, int(top_k)), -1, dtype=torch.long, device=dev)
            tlp = torch.zeros((out.sequences.shape[0], max_new, int(top_k)), dtype=torch.float32, device=dev)
            tid[:, :n], tlp[:, :n] = out.top_ids, out.top_logprobs
            tops[j] = (tid, tlp, out.n_tokens)
        if logprobs_out is not None:
            lp = torch.zeros((out.sequences.shape[0], max_new), dtype=torch.float32, device=dev)
            lp[:, : out.token_logprobs.shape[1]] = out.token_logprobs
            lps[j] = (lp, out.n_tokens)
        if want_dict:
            out = out.sequences
        if logits_out is not None:
            last[j] = m.last_logits(len(batch) * nret)
        full = torch.full((out.shape[0], max_new), tokenizer.eos_token_id, dtype=torch.long, device=dev)
        full[:, : out.shape[1]] = out
        outs[j] = full

    n_ctx = max(1, min(int(inflight), len(starts)))
    if n_ctx == 1:
        for j in range(len(starts)):
            one(model, j)
    else:
        import threading
        ctxs = [model] + [model.new_context() for _ in range(n_ctx - 1)]
        errs = []

        def worker(k):
            try:
                torch.cuda.set_device(dev)
                # a torch stream of this thread's own: the context orders its work against torch.cuda.current_stream(), which
                # would otherwise be the one default stream of the process and serialise context A's enqueued work in front of B's
                with torch.cuda.stream(torch.cuda.Stream(dev)):
                    for j in range(k, len(starts), n_ctx):
                        one(ctxs[k], j)
                    torch.cuda.current_stream(dev).synchronize()      # results are read from the caller's stream
            except BaseException as e:      # noqa: BLE001  (re-raised on the caller's thread)
                errs.append(e)
        threads = [threading.Thread(target=worker, args=(k,)) for k in range(n_ctx)]
        [t.start() for t in threads]
        [t.join() for t in threads]
        if errs:
            raise errs[0]
    if logits_out is not None:
        logits_out.extend(last)
    if logprobs_out is not None:
        logprobs_out.extend(lps)
    if top_logprobs_out is not None:
        top_logprobs_out.extend(tops)
    return torch.cat(outs) if outs else torch.empty((0, max_new), dtype=torch.long, device=dev)


def annotate_continuous(model, tokenizer, items, input_path, max_new, temperature=0.0, top_p=1.0, use_input_embed=False,
                        device=None, stop_sequence=None, slots=None, refill_min=None, stats_out=None, warpers=None):
    """--continuous: the whole shard through ONE generate_continuous() call - a decode batch of `slots` rows whose finished rows
    are handed to the next prompts - instead of a sequence of batches that each wait for their longest answer.  Returns what
    annotate() returns, [n, max_new] padded with the EOS id; stats_out (a dict) receives the call's statistics."""
    dev = device or model.device
    if not items:
        return torch.empty((0, max_new), dtype=torch.long, device=dev)
    prompts = [opa.tokenizer_seq_token(build_prompt(q["instruction"], input_path), tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX,
                                       return_tensors="pt") for q in items]
    extra = dict(warpers or {})                  # --min_p / --typical_p / --epsilon_cutoff / --eta_cutoff
    if use_input_embed:
        extra["protein_tokens"] = model.project_dataset(torch.tensor([q["input_embed"] for q in items], dtype=torch.float32, device=dev))
    with torch.inference_mode():
        out = model.generate_continuous(prompts, [q["input"] for q in items], max_new_tokens=max_new,
                                        pad_token_id=tokenizer.eos_token_id, slots=slots, refill_min=refill_min,
                                        do_sample=temperature > 0, temperature=temperature, top_p=top_p,
                                        stop_sequence=stop_sequence, return_dict_in_generate=True, **extra)
    if stats_out is not None:
        stats_out.update(out.stats)
    full = torch.full((len(items), max_new), tokenizer.eos_token_id, dtype=torch.long)
    for i, s in enumerate(out.sequences):
        full[i, : len(s)] = s
    return full.to(dev)


def continuous_refusals(args):
    """The options --continuous does not take (generate_continuous raises NotImplementedError for their arguments)."""
    bad = []
    if args.num_beams > 1:
        bad.append("--num_beams")
    if int(getattr(args, "num_return_sequences", 1) or 1) > 1:
        bad.append("--num_return_sequences")
    g = getattr(args, "guidance_scale", None)
    if g is not None and float(g) != 1.0:
        bad.append("--guidance_scale")
    for flag in ("share_prompt_head", "save_logprobs", "save_top_logprobs", "dump_logits", "rank_terms", "allowed_terms"):
        if getattr(args, flag, None):
            bad.append("--" + flag)
    if logits_processor_kwargs(args):
        bad.append("the logits-processor options")
    return bad


def shared_head_length(rows) -> int:
    """Length of the longest leading id run that all `rows` (id lists) share, ending in front of every row's first placeholder and
    leaving every row at least one id behind it."""
    if not rows:
        return 0
    n = min(len(r) for r in rows) - 1
    for r in rows:
        r = list(r)
        if opa.DEFAULT_SEQ_TOKEN_INDEX in r:
            n = min(n, r.index(opa.DEFAULT_SEQ_TOKEN_INDEX))
    first = list(rows[0])
    for r in rows[1:]:
        r, k = list(r), 0
        while k < n and r[k] == first[k]:
            k += 1
        n = k
    return max(n, 0)


def prompts_per_call(batch_size: int, num_return_sequences: int) -> int:
    """--num_return_sequences N: prompts of one generate call, batch_size // N (its N answers each fill the batch_size rows)."""
    if num_return_sequences > batch_size:
        raise ValueError(f"--num_return_sequences {num_return_sequences} exceeds --batch_size {batch_size} (the decoder rows of a call)")
    return batch_size // num_return_sequences


def build_result(qs, texts, num_return_sequences: int = 1):
    """The saved items: texts holds N = num_return_sequences answers per item, item i's in texts[i N : i N + N].  `generated` is
    the first of them; with N > 1 `generated_all` lists all N (N = 1: the file of a run without the flag)."""
    N = int(num_return_sequences)
    if len(texts) != len(qs) * N:
        raise ValueError(f"{len(texts)} answers for {len(qs)} items x {N}")
    result = []
    for k, q in enumerate(qs):
        r = {"ground_truth": q["output"], "generated": texts[k * N]}
        if N > 1:
            r["generated_all"] = list(texts[k * N:(k + 1) * N])
        result.append(r)
    return result


def rank_terms(model, tokenizer, items, input_path, batch_size, trie, k, with_stop=False, device=None, beams=0):
    """--rank_terms: per item the K best members of `trie` behind its prompt -> (log-probs fp32 [n, K] descending, member indices
    [n, K]).  One cache_prefix + one score_trie per batch; nothing is generated.  beams > 0 (--search_terms): search_trie with that
    many beams instead - approximate wherever a prompt's search was not exhaustive; member index -1 / -inf where fewer than K
    members were found."""
    dev = device or model.device
    k = min(int(k), len(trie.member_ids))
    if beams:
        k = min(k, int(beams))
    vals, idx = [], []
    for i in range(0, len(items), batch_size):
        batch = items[i:i + batch_size]
        prompts = [build_prompt(q["instruction"], input_path) for q in batch]
        ids = [opa.tokenizer_seq_token(p, tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX, return_tensors="pt").to(dev) for p in prompts]
        ids = opa.left_pad_sequence(ids, padding_value=tokenizer.pad_token_id, batch_first=True)
        mask = ids != tokenizer.pad_token_id
        with torch.inference_mode():
            prefix = model.cache_prefix(ids, seq=[q["input"] for q in batch], attention_mask=mask)
            if beams:
                res = model.search_trie(prefix, trie, num_beams=int(beams), top=k, include_stop=with_stop)
                v, j = res.logprob, res.member_index
            else:
                v, j = model.score_trie(prefix, trie, include_stop=with_stop).topk(k)
        vals.append(v)
        idx.append(j)
    if not vals:
        return torch.empty((0, k), dtype=torch.float32, device=dev), torch.empty((0, k), dtype=torch.long, device=dev)
    return torch.cat(vals), torch.cat(idx)


def prompt_capacity(tokenizer, items, input_path, n_prot_tokens) -> int:
    """Decoder positions the longest prompt of the shard needs after the splice (each <seq> becomes n_prot_tokens)."""
    need = 1
    for q in items:
        ids = opa.tokenizer_seq_token(build_prompt(q["instruction"], input_path), tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX)
        need = max(need, len(ids) + (n_prot_tokens - 1) * sum(1 for t in ids if t == opa.DEFAULT_SEQ_TOKEN_INDEX))
    return need


def eval_model(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        odist.init_process_group("nccl", rank, world, torch.device("cuda", local), timeout_s=args.collective_timeout)
    if args.input_path.endswith(".jsonl"):            # stage-2 input: one item per line (generate_esm_embedding.py)
        qs = [json.loads(line) for line in open(args.input_path) if line.strip()]
    else:
        qs = json.load(open(args.input_path))
    qs = [q for q in qs if q["input"] is not None]
    n = len(qs)
    lo, hi = odist.shard_bounds(n, rank, world)
    mine = qs[lo:hi]
    max_new = max_new_tokens_for(args.input_path) if args.max_new_tokens is None else args.max_new_tokens
    model_name = opa.get_model_name_from_path(args.model_base_path)
    cstp_path = return_cstp_path(args.opus_pllm_weights_path, "modality_encoder/modality_encoding_adapter.ckpt")
    n_rank = int(getattr(args, "rank_terms", 0) or 0)
    n_beams = int(getattr(args, "search_terms", 0) or 0)          # --search_terms K: beam search instead of the exact tree pass
    if n_rank and n_beams:
        raise ValueError("--search_terms and --rank_terms exclude each other")
    if n_beams:
        n_rank = int(getattr(args, "search_top", 0) or 0) or n_beams
    if n_rank and not getattr(args, "allowed_terms", None):
        raise ValueError("--rank_terms / --search_terms need --allowed_terms (the vocabulary to rank)")
    held = {}
    continuous = bool(getattr(args, "continuous", False))
    ctx_new, ctx_batch = max_new, args.batch_size * max(1, args.num_beams, n_beams)
    if continuous:
        bad = continuous_refusals(args)
        if bad:
            raise ValueError("--continuous does not take " + ", ".join(bad))
        # the context's max_new_tokens capacity is a session's step budget: a row can begin at any step that leaves it its budget
        ctx_new = int(args.session_steps) if args.session_steps else 4 * max_new
        if ctx_new < max_new:
            raise ValueError(f"--session_steps {ctx_new} is below the token budget {max_new}")
        ctx_batch = int(args.slots) if args.slots else args.batch_size
    lookup_kw = lookup_kwargs(args)
    if lookup_kw:                                     # a verify pass holds batch x (K + 1) logits rows
        if continuous:
            raise ValueError("--continuous does not take --prompt_lookup_num_tokens")
        ctx_batch = max(ctx_batch, args.batch_size * (lookup_kw["prompt_lookup_num_tokens"] + 1))

    def capacity(tok, cfg):
        need = prompt_capacity(tok, mine, args.input_path, cfg.n_prot_tokens)
        if n_rank:                                    # the terms' positions sit behind the prompt: room for the longest of them
            held["trie"] = token_constraint(args, tok)
            need += held["trie"].max_depth
        extra = dict(max_new_tokens=max(ctx_new, held["trie"].max_depth)) if n_beams else {}   # (the beams decode the members)
        return dict(max_prompt=max(args.max_prompt or 0, need), **extra)
    # capacity of the context: the reference has no cap; here the KV cache is sized once, from what this run will really ask for
    tokenizer, model, _ = load_pretrained_model(args.model_base_path, args.opus_pllm_weights_path, model_name,
                                                args.load_8bit, args.load_4bit, switch_projector_type=args.switch_projector_type,
                                                decoder_weights=getattr(args, "decoder_weights", None),
                                                cstp_path=cstp_path, device=f"cuda:{local}", max_batch=ctx_batch,
                                                max_enc_tokens=args.max_residues + 2, max_prompt=8, max_new_tokens=ctx_new,
                                                capacity_from=capacity)
    dev = torch.device("cuda", local)
    t0 = time.time()
    if n_rank:
        return _eval_ranked_terms(args, qs, mine, tokenizer, model, held["trie"], n_rank, dev, rank, world, t0, n_beams)
    logits = [] if args.dump_logits else None
    proc_kw = logits_processor_kwargs(args)
    proc_kw.update(lookup_kw)
    proc_kw.update(warper_kwargs(args))
    trie = token_constraint(args, tokenizer)          # --allowed_terms: built once, uploaded once per context
    if trie is not None:
        proc_kw["prefix_allowed_tokens_fn"] = trie
    lps = [] if args.save_logprobs else None
    top_K = int(getattr(args, "save_top_logprobs", 0) or 0)
    tops = [] if top_K else None
    N = int(getattr(args, "num_return_sequences", 1) or 1)
    stop_ids = tokenizer.encode("###", add_special_tokens=False) if args.stop_at_hashes else None
    if continuous:              # the rank's whole shard in one call; the same fields are saved
        cstats = {}
        local_ids = annotate_continuous(model, tokenizer, mine, args.input_path, max_new, args.temperature, args.top_p,
                                        args.use_input_embed, dev, stop_ids, slots=ctx_batch, refill_min=args.refill_min, stats_out=cstats,
                                        warpers=warper_kwargs(args))
        if cstats:
            print(f"rank {rank}: continuous {cstats}, occupancy {cstats['live_row_steps'] / max(cstats['slot_steps'], 1):.3f}")
    else:
        local_ids = annotate(model, tokenizer, mine, args.input_path, args.batch_size, max_new, args.temperature, args.top_p,
                             args.num_beams, args.use_input_embed, dev, logits, stop_ids, inflight=args.inflight,
                             logprobs_out=lps, processors=proc_kw, num_return_sequences=N,
                             share_prompt_head=bool(getattr(args, "share_prompt_head", False)),
                             guidance_scale=getattr(args, "guidance_scale", None), top_logprobs_out=tops, top_k=top_K)
    all_ids = odist.all_gather_ids(local_ids, tokenizer.eos_token_id)
    if tops is not None:        # [n, max_new K] ids and log-probabilities and [n] counted positions, in rank order
        loc_ti = torch.cat([x[0] for x in tops]).view(-1, max_new * top_K) if tops else torch.empty((0, max_new * top_K), dtype=torch.long, device=dev)
        loc_tl = torch.cat([x[1] for x in tops]).view(-1, max_new * top_K) if tops else torch.empty((0, max_new * top_K), dtype=torch.float32, device=dev)
        loc_tn = torch.cat([x[2] for x in tops]).view(-1, 1) if tops else torch.empty((0, 1), dtype=torch.long, device=dev)
        all_ti = odist.all_gather_ids(loc_ti.contiguous(), -1).view(-1, max_new, top_K).cpu()
        all_tl = odist.all_gather_logits(loc_tl.contiguous()).view(-1, max_new, top_K).cpu()
        all_tn = odist.all_gather_ids(loc_tn, 0).view(-1).cpu()
    if lps is not None:         # [n, max_new] log-probabilities and [n] counted positions, in rank order
        loc_lp = torch.cat([x[0] for x in lps]) if lps else torch.empty((0, max_new), dtype=torch.float32, device=dev)
        loc_n = torch.cat([x[1] for x in lps]).view(-1, 1) if lps else torch.empty((0, 1), dtype=torch.long, device=dev)
        all_lp, all_n = odist.all_gather_logits(loc_lp).cpu(), odist.all_gather_ids(loc_n, 0).view(-1).cpu()
    if logits is not None:      # parity dump: last-step fp32 logits of every item, gathered in rank order over RCCL
        loc = torch.cat(logits) if logits else torch.empty((0, model.cfg.dec_vocab), dtype=torch.float32, device=dev)
        all_logits = odist.all_gather_logits(loc)
        if rank == 0:
            torch.save(all_logits.cpu(), args.dump_logits)
    if rank == 0:
        dt = time.time() - t0
        texts = [after_process_output(t) for t in tokenizer.batch_decode(all_ids, skip_special_tokens=True)]
        result = build_result(qs, texts, N)
        if lps is not None:     # over the row's counted tokens (its EOS / "###" included); N > 1: of the item's first answer
            for k, r in enumerate(result):
                row = all_lp[k * N, : int(all_n[k * N])]
                r["logprob"] = float(row.double().sum())
                r["token_logprobs"] = [float(v) for v in row]
        if tops is not None:    # the K alternatives of every counted step; N > 1: of the item's first answer
            for k, r in enumerate(result):
                steps = int(all_tn[k * N])
                r["top_logprobs"] = [{"ids": [int(i) for i in all_ti[k * N, t]], "logprobs": [float(v) for v in all_tl[k * N, t]],
                                      "tokens": [tokenizer.decode([int(i)]) for i in all_ti[k * N, t]]} for t in range(steps)]
        print(f"entries/sec: {n / dt}, time elapsed: {dt}")
        with open(args.save_path, "w") as f:
            json.dump(result, f)
    if world > 1:
        torch.distributed.destroy_process_group()


def _eval_ranked_terms(args, qs, mine, tokenizer, model, trie, k, dev, rank, world, t0, beams=0):
    vals, idx = rank_terms(model, tokenizer, mine, args.input_path, args.batch_size, trie, k,
                           bool(getattr(args, "rank_with_stop", False)), dev, beams)
    all_vals = odist.all_gather_logits(vals.contiguous()).cpu()
    all_idx = odist.all_gather_ids(idx.contiguous(), 0).cpu()
    if rank == 0:
        dt = time.time() - t0
        names = trie.member_strings
        result = []
        for q, v, j in zip(qs, all_vals.tolist(), all_idx.tolist()):
            ranked = [[names[m], lp] for m, lp in zip(j, v) if m >= 0]            # (--search_terms may find fewer than K)
            result.append({"ground_truth": q["output"], "generated": ranked[0][0], "ranked_terms": ranked})
        print(f"entries/sec: {len(qs) / dt}, time elapsed: {dt}")
        with open(args.save_path, "w") as f:
            json.dump(result, f)
    if world > 1:
        torch.distributed.destroy_process_group()


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--model-base-path", type=str, default="synthetic:c1_tiny")
    p.add_argument("--opus-pllm-weights-path", type=str, default="synthetic")
    p.add_argument("--input_path", type=str, required=True)
    p.add_argument("--save_path", type=str, required=True)
    p.add_argument("--temperature", type=float, default=0.1)        # reference default: sampling (run_opus_ddp.py:156)
    p.add_argument("--top_p", type=float, default=0.7)
    p.add_argument("--num_beams", type=int, default=1)
    p.add_argument("--num_return_sequences", type=int, default=1, metavar="N",
                   help="N answers per item from one run (sampling, or the N best of --num_beams): a call takes batch_size // N "
                        "prompts, prefilled once; items are saved with `generated_all` (N answers) beside `generated` (the first)")
    p.add_argument("--guidance_scale", type=float, default=None, metavar="G",
                   help="classifier-free guidance against each prompt's protein-free twin (the prompt without its <seq> "
                        "placeholders): a call takes batch_size // 2 prompts and costs about a plain call of batch_size rows; "
                        "greedy and sampling only")
    p.add_argument("--max_new_tokens", type=int, default=None)
    p.add_argument("--switch_projector_type", type=str, default="mlp2x_gelu")
    p.add_argument("--load-4bit", action="store_true")
    p.add_argument("--decoder_weights", choices=("fp8", "mxfp4"), default=None,
                   help="fp8 / mxfp4: decoder-layer weights also as e4m3 / MXFP4 panels for the decode step (faster decode, 1.5x / 1.27x "
                        "the memory of those weights; mxfp4 is uncalibrated 4-bit rounding: a different model)")
    p.add_argument("--load-8bit", action="store_true")
    p.add_argument("--batch_size", type=int, default=8)          # hard-coded 8 in the reference (:75)
    p.add_argument("--max_residues", type=int, default=1024)
    p.add_argument("--max_prompt", type=int, default=None, help="decoder positions to reserve (default: what the longest prompt needs)")
    p.add_argument("--collective_timeout", type=int, default=1800, help="seconds before a stuck RCCL wait aborts the run")
    p.add_argument("--use_input_embed", action="store_true",
                   help="stage 2 of the two-stage pipeline: take `input_embed` from the .jsonl instead of running ESM-2")
    p.add_argument("--stop_at_hashes", action="store_true",
                   help="opt-in: finish a row once it has generated the ids of '###' (the reference decodes on to max_new_tokens "
                        "and cuts the text there afterwards: same text, less decoding)")
    p.add_argument("--inflight", type=int, default=2,
                   help="batches in flight per GPU (contexts sharing the weights, one host thread each): with 2, one batch's kernels "
                        "fill the other's launch gaps and ramps (+10 %% throughput at batch 64; same ids)")
    p.add_argument("--continuous", action="store_true",
                   help="opt-in: the rank's whole shard through one generate_continuous() call - finished decode rows are handed to "
                        "the next prompts instead of waiting for the batch's longest answer; greedy and sampling only, not with "
                        "--num_beams > 1, --num_return_sequences > 1, --guidance_scale, --share_prompt_head, --save_logprobs, "
                        "--dump_logits, --allowed_terms or the logits-processor options")
    p.add_argument("--slots", type=int, default=None, help="with --continuous: decode rows (default: --batch_size)")
    p.add_argument("--refill_min", type=int, default=None,
                   help="with --continuous: free rows a refill waits for (default: max(1, slots // 4))")
    p.add_argument("--session_steps", type=int, default=None,
                   help="with --continuous: decode steps one live batch may run, the context's max_new_tokens capacity "
                        "(default: 4 x the token budget)")
    p.add_argument("--share_prompt_head", action="store_true",
                   help="opt-in: prefill the id run that all prompts of the shard share in front of the protein once (a detached "
                        "prefix) and generate every batch behind it; not with --num_beams > 1")
    p.add_argument("--save_top_logprobs", type=int, default=0, metavar="K",
                   help="each saved item also gets `top_logprobs`: per counted step the K (1..20) likeliest tokens of the model's raw "
                        "distribution as `ids`, `logprobs` and decoded `tokens` (generate(top_logprobs=K)); works beside --save_logprobs")
    p.add_argument("--save_logprobs", action="store_true",
                   help="each saved item also gets `logprob` and `token_logprobs`: the log-probabilities of its generated tokens "
                        "(greedy or sampling; computed on the GPU in the decode loop)")
    p.add_argument("--dump_logits", type=str, default=None,
                   help="parity dump: save the fp32 last-step logits of every item ([n, V], input order) to this .pt file")
    how = p.add_mutually_exclusive_group()
    how.add_argument("--search_terms", type=int, default=0, metavar="K",
                     help="with --allowed_terms: no generation; beam search over the allowed terms with K beams per prompt "
                          "(search_trie) and save the best ones as `ranked_terms`, in --rank_terms' format.  Approximate: a term "
                          "whose first ids fall out of the beam is missed; --rank_terms is exact and about as fast on small "
                          "vocabularies")
    p.add_argument("--search_top", type=int, default=0, metavar="N", help="with --search_terms: terms saved per item (default K)")
    how.add_argument("--rank_terms", type=int, default=0, metavar="K",
                   help="with --allowed_terms: no generation; score every allowed term behind each prompt in one tree pass and save "
                        "the K most probable ones with their log-probabilities as `ranked_terms`")
    p.add_argument("--rank_with_stop", action="store_true",
                   help="with --rank_terms / --search_terms: add the log-probability of ending the answer right behind the term")
    add_logits_processor_args(p)
    add_warper_args(p)
    add_lookup_args(p)
    add_constraint_args(p)
    return p


if __name__ == "__main__":
    eval_model(build_parser().parse_args())
