"""Checks of generate(num_return_sequences=N) and the fanned-out prefill behind it, shared by tests/test_gpu_nsamples.py (fp16-operand
build) and its bf16 child process (tests/bf16_nsamples_check.py).  Each returns a dict of observations; the callers assert the
bounds.  Test infrastructure, not product code."""
from __future__ import annotations

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import synth

import gen_scores_checks as gsc
from gpu_helpers import rel_l2

PAD = 2
REFERENCE_MODE = dict(temperature=0.1, top_p=0.7, top_k=50)      # eval/run_opus_ddp.py's default (transformers 4.46.3's top_k)
OPEN_MODE = dict(temperature=1.0, top_p=1.0, top_k=0)

# name -> (config preset, config overrides, B, N, text ids per prompt).  A prompt of n text ids is n + n_prot_tokens - 1 slots.
#   2x2    4 decoder rows: the skinny GEMM route of the decode step; T = 30, so three decode steps write the cache slots 30, 31, 32
#   3x3    9 rows, every decoder family
#   7x9    63 rows, B < N; max_prompt 96 with a 52-slot prompt beside a 13-slot one: 39 padded slots, more than a key tile
#   1x8    one prompt
MICRO_CASES = {
    "micro_2x2": ("micro", dict(max_batch=4), 2, 2, [23, 11]),
    "micro_3x3": ("micro", dict(max_batch=9), 3, 3, [9, 16, 6]),
    "micro_7x9": ("micro", dict(max_batch=63, max_prompt=96), 7, 9, [45, 6, 17, 30, 8, 22, 11]),
    "micro_1x8": ("micro", dict(max_batch=8), 1, 8, [13]),
    "micro_opt_3x3": ("micro_opt", dict(max_batch=9), 3, 3, [9, 16, 6]),
    "micro_qwen_3x3": ("micro_qwen", dict(max_batch=9), 3, 3, [9, 16, 6]),
}
# Llama-3-8B widths (gen_scores_checks.llama8b_shape(64, 2, 8)): 60 rows take the stream and wide GEMM routes with fragment-ordered
# activations, and B > N, so that an in-place row fan-out would overwrite prompt 1's source with prompt 0's replicas
BIG_CASES = {
    "llama8b_12x5": (12, 5, [6 + (5 * i) % 11 for i in range(12)]),
    "llama8b_1x64": (1, 64, [14]),
}


def micro_model(name, dev):
    preset, kw, B, N, lens = MICRO_CASES[name]
    cfg = getattr(opa, preset)(**kw)
    return gsc.make_model(cfg, dev), B, N, lens


def prompts(cfg, lens, seed: int = 0):
    """len(lens) left-padded prompts (pad 2) of lens[i] text ids with one protein each: ids, mask, seqs."""
    B = len(lens)
    seqs = [synth.synth_protein(12 + (7 * i + seed) % 40, 100 * seed + i) for i in range(B)]
    rows = [synth.synth_prompt_ids(cfg.dec_vocab, 1000 * seed + i, n_text=n, seq_pos=2) for i, n in enumerate(lens)]
    width = max(len(r) for r in rows)
    ids = torch.full((B, width), PAD, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.tensor(r)
    return ids, ids != PAD, seqs


def spliced(model, ids, mask, seqs):
    """What generate() prefills: embeds [B, T, H] (operand dtype), mask u8 [B, T]."""
    _, _, m, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, seqs, None, inference_mode=True)
    return emb, m.to(torch.uint8)


def dirty(model, longest: int):
    """A different batch of max_batch rows with longer prompts through the context (prefill + one decode step): every cache row,
    first-slot word and logits row then holds something else."""
    cfg = model.cfg
    B = cfg.max_batch
    n = min(cfg.max_prompt - cfg.n_prot_tokens + 1, longest + 5)
    ids, mask, seqs = prompts(cfg, [n - (i % 3) for i in range(B)], seed=7)
    emb, m = spliced(model, ids, mask, seqs)
    lg = model.prefill_logits(emb, m)
    model.decode_logits(lg.argmax(dim=1))
    return int(emb.shape[1])


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))     # bitwise (NaN-proof)


def prefill_and_replicas(model, dev, B: int, N: int, lens, steps: int = 3):
    """(b) the logits behind the fanned-out prefill against the plain B-row prefill, bit for bit, and (c) N replicas fed the same
    token for `steps` decode steps: bit-identical to replica 0; replica 0 against the same steps behind a prefill of the prompts
    repeated N times (rel-L2, the worst step)."""
    cfg = model.cfg
    V = cfg.dec_vocab
    ids, mask, seqs = prompts(cfg, lens)
    emb, m = spliced(model, ids, mask, seqs)
    T = int(emb.shape[1])
    plain = model.prefill_logits(emb, m).clone()
    T_dirty = dirty(model, max(lens))
    fan = model.prefill_logits(emb, m, num_return_sequences=N)
    last = model.last_logits(B * N)
    out = {"B": B, "N": N, "T": T, "T_dirty": T_dirty, "pad_slots_max": int(T - int(m.sum(dim=1).min())),
           "first_exact": _same(fan.view(B, N, V), plain[:, None, :].expand(B, N, V)), "last_logits_exact": _same(last, fan),
           "finite": bool(torch.isfinite(fan).all())}
    toks, fan_steps = [], [fan.view(B, N, V)[:, 0].clone()]
    replicas_exact, differ = True, True
    cur = fan
    for _ in range(steps):
        tok = cur.view(B, N, V)[:, 0].argmax(dim=1)                        # one token per prompt, the same for its N replicas
        toks.append(tok)
        cur = model.decode_logits(tok.repeat_interleave(N))
        g = cur.view(B, N, V)
        replicas_exact &= _same(g, g[:, :1].expand(B, N, V))
        if B > 1:
            differ &= all(not _same(g[b, 0], g[b + 1, 0]) for b in range(B - 1))
        fan_steps.append(g[:, 0].clone())
    out.update(replicas_exact=bool(replicas_exact), prompts_differ=bool(differ), last_slot=T + steps - 1)
    # the same steps behind a prefill of ids.repeat_interleave(N): same decode launches, other prefill GEMM routes
    ref = model.prefill_logits(emb.repeat_interleave(N, dim=0), m.repeat_interleave(N, dim=0))
    worst = rel_l2(fan_steps[0], ref.view(B, N, V)[:, 0])
    for k, tok in enumerate(toks):
        ref = model.decode_logits(tok.repeat_interleave(N))
        worst = max(worst, rel_l2(fan_steps[k + 1], ref.view(B, N, V)[:, 0]))
    out["replica0_vs_repeated_rel_l2"] = worst
    return out


def sampled(model, dev, B: int, N: int, lens, mode: dict, max_new: int = 4, seed: int = 20261019):
    """(d) every sampled id of generate(do_sample=True, num_return_sequences=N) against the fp64 rule on that step's returned
    logits with the draw of (seed, row b N + j, step), and (e) token_logprobs against score_continuations behind the cached
    prompts with prefix_rows = arange(B).repeat_interleave(N)."""
    import oracle.sampling as osamp
    cfg = model.cfg
    ids, mask, seqs = prompts(cfg, lens)
    kw = dict(attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new, do_sample=True, num_return_sequences=N, **mode)
    o = model.generate(ids, seqs, seed=seed, return_dict_in_generate=True, output_logits=True, output_token_logprobs=True, **kw)
    seq, cnt = o.sequences.cpu().numpy(), o.n_tokens.cpu().numpy()
    T_, tp, tk = mode["temperature"], mode["top_p"], mode["top_k"]
    n = nd = mism = bad = 0
    for t in range(seq.shape[1]):
        lg = o.logits[t].float().cpu().numpy()
        for r in range(seq.shape[0]):
            if t >= cnt[r]:
                continue
            ref = osamp.HeadRef(lg[r], T_, tp, tk)
            pick, dec, lo, hi = ref.draw(np.array([osamp.draw_uniform(seed, r, t)[1]]))
            g = int(seq[r, t])
            n += 1
            nd += int(not dec[0])
            mism += int(dec[0] and g != int(pick[0]))
            bad += int(not ref.admissible(g, int(lo[0]), int(hi[0])))
    again = model.generate(ids, seqs, seed=seed, **kw)
    other = model.generate(ids, seqs, seed=seed + 1, **kw)
    s3 = o.sequences.view(B, N, -1)
    out = {"rows": int(seq.shape[0]), "n": int(seq.shape[1]), "logits_rows": int(o.logits[0].shape[0]),
           "lp_shape": list(o.token_logprobs.shape), "draws": n, "nondecisive": nd / max(n, 1), "mismatches": mism,
           "inadmissible": bad, "same_seed_equal": bool(torch.equal(again, o.sequences)),
           "other_seed_differs": bool(other.shape != o.sequences.shape or not torch.equal(other, o.sequences)),
           "replicas_all_equal": bool(N > 1 and all(bool((s3[b] == s3[b, :1]).all()) for b in range(B)))}
    # (e) teacher-forced: the same tokens scored behind the cached prompts
    prefix = model.cache_prefix(ids, seqs, attention_mask=mask)
    conts = [o.sequences[r, :int(cnt[r])].cpu() for r in range(seq.shape[0])]
    sc = model.score_continuations(prefix, conts, prefix_rows=torch.arange(B).repeat_interleave(N))
    lp, ref = o.token_logprobs.cpu(), sc.token_logprobs.cpu()
    counted = torch.arange(seq.shape[1])[None, :] < torch.from_numpy(cnt)[:, None]
    w = min(lp.shape[1], ref.shape[1])
    out["teacher_forced_abs"] = float((lp[:, :w] - ref[:, :w])[counted[:, :w]].abs().max())
    out["teacher_forced_counted"] = int(counted.sum())
    return out


def eos_rows(model, dev, B: int, N: int, lens, max_new: int = 8, seed: int = 5):
    """(f) an EOS id that some replicas emit and others do not: rows follow the free run up to their EOS, pad behind it, and the
    result is as long as the longest row."""
    cfg = model.cfg
    ids, mask, seqs = prompts(cfg, lens)
    kw = dict(attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new, do_sample=True, num_return_sequences=N, seed=seed,
              **OPEN_MODE)
    free = model.generate(ids, seqs, **kw).cpu()
    R = free.shape[0]
    eos, best = None, None
    for tok in sorted(set(free[:, : max_new - 2].reshape(-1).tolist())):
        hit = (free[:, : max_new - 2] == tok).any(dim=1)
        k = int(hit.sum())
        if 0 < k < R and tok != PAD and (best is None or abs(k - R // 2) < best):
            eos, best = int(tok), abs(k - R // 2)
    assert eos is not None, free
    got = model.generate(ids, seqs, eos_token_id=[eos], **kw).cpu()
    first = [(free[r] == eos).nonzero() for r in range(R)]
    end = [int(f[0]) + 1 if len(f) else max_new for f in first]
    ok = True
    for r in range(R):
        e = min(end[r], got.shape[1])
        ok &= bool(torch.equal(got[r, :e], free[r, :e])) and bool((got[r, e:] == PAD).all())
    groups = [sorted({end[b * N + j] < max_new for j in range(N)}) for b in range(B)]
    return {"eos": eos, "n": int(got.shape[1]), "longest": max(end), "rows_ok": bool(ok), "finished_rows": sum(e < max_new for e in end),
            "rows": R, "prompt_with_both": any(len(g) == 2 for g in groups)}


def processors(model, dev, B: int, N: int, lens, max_new: int = 8, seed: int = 9):
    """(f) repetition_penalty + no_repeat_ngram_size per decoder row: the returned scores' finite pattern against the warpers behind
    tests/logits_proc_ref.py on the returned raw logits and each row's own history; every draw finite there."""
    import logits_proc_ref as lpr
    import oracle.sampling as osamp
    ids, mask, seqs = prompts(model.cfg, lens)
    mode = dict(temperature=1.0, top_p=0.9, top_k=50)
    o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new, do_sample=True, seed=seed,
                       num_return_sequences=N, repetition_penalty=1.3, no_repeat_ngram_size=2, return_dict_in_generate=True,
                       output_scores=True, output_logits=True, **mode)
    seq = o.sequences.cpu()
    mism = near = drawn_inf = banned = 0
    for t in range(seq.shape[1]):
        raw = o.logits[t].cpu()
        proc = lpr.process(raw, seq[:, :t], eos=(), penalty=1.3, ngram=2)
        banned += int((torch.isinf(proc) & ~torch.isinf(raw)).sum())
        ours = o.scores[t].cpu()
        want = osamp._warp(proc / mode["temperature"], mode["top_p"], mode["top_k"])
        fo, fw = torch.isfinite(ours), torch.isfinite(want)
        badm = fo ^ fw
        if badm.any():
            p = torch.exp(proc - proc.max(dim=1, keepdim=True).values).double()
            thr = torch.where(fw, p, torch.full_like(p, 2.0)).min(dim=1, keepdim=True).values
            mism += int(badm.sum())
            near += int((badm & ((p - thr).abs() <= 1e-6 * thr)).sum())
        drawn_inf += int((~torch.isfinite(ours.gather(1, seq[:, t:t + 1]))).sum())
    model._set_logits_processors(None)
    return {"rows": int(seq.shape[0]), "n": int(seq.shape[1]), "scores_mismatch": mism, "mismatch_near_threshold": near,
            "drawn_not_finite": drawn_inf, "ngram_bans": banned}


def per_row_tries(model, dev, B: int, N: int, lens, seed: int = 3):
    """(f) TokenTrie.per_row of B tries with pairwise disjoint member ids: decoder row r must produce a member of trie r // N."""
    from opus_pllm_amd.constraint import TokenTrie
    cfg = model.cfg
    ids, mask, seqs = prompts(cfg, lens)
    end = 1
    tries, members = [], []
    for b in range(B):                                   # prompt b owns the ids 10 + 8 b .. 17 + 8 b
        base = 10 + 8 * b
        mem = [[base, base + 1], [base, base + 2, base + 3], [base + 4], [base + 5, base + 6, base + 7]]
        members.append(mem)
        tries.append(TokenTrie(mem, end_token_id=end))
    per_row = TokenTrie.per_row(tries)
    out = model.generate(ids, seqs, attention_mask=mask, pad_token_id=PAD, eos_token_id=[end], max_new_tokens=6, do_sample=True,
                         seed=seed, num_return_sequences=N, prefix_allowed_tokens_fn=per_row, **OPEN_MODE).cpu()
    ok, chosen = True, []
    for r in range(out.shape[0]):
        row = out[r].tolist()
        body = row[: row.index(end)] if end in row else row
        mine = per_row.row_trie(r, N)
        ok &= mine is tries[r // N] and body in members[r // N] and end in row
        chosen.append(tuple(body))
    sets = [set(t for m in mem for t in m) for mem in members]
    disjoint = all(not (sets[a] & sets[b]) for a in range(B) for b in range(a + 1, B))
    model._set_token_constraint(None)
    return {"rows": int(out.shape[0]), "accepted": bool(ok), "disjoint_tries": bool(disjoint and B >= 2),
            "distinct_members": len(set(chosen))}


def n1_is_plain(model, dev, B: int, lens, max_new: int = 6):
    """(g) num_return_sequences=1 against the call without it: ids, graphs, decode steps and launches; a plain call after an
    N-sample call returns what it returned before."""
    ids, mask, seqs = prompts(model.cfg, lens)
    base = dict(attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new)
    res = {}
    for tag, kw in (("greedy", dict(do_sample=False)), ("sample", dict(do_sample=True, seed=4, **REFERENCE_MODE))):
        plain = model.generate(ids, seqs, **base, **kw).cpu()
        i0, r0, d0 = (model.stat(k) for k in ("graph_instantiations", "graph_replays", "decode_steps"))
        one = model.generate(ids, seqs, num_return_sequences=1, **base, **kw).cpu()
        i1, r1, d1 = (model.stat(k) for k in ("graph_instantiations", "graph_replays", "decode_steps"))
        again = model.generate(ids, seqs, **base, **kw).cpu()
        r2, d2 = model.stat("graph_replays"), model.stat("decode_steps")
        model.timing(True)
        model.generate(ids, seqs, **base, **kw)
        l_plain = int(model.timing_get("*", "*")[1])
        model.timing(True)
        model.generate(ids, seqs, num_return_sequences=1, **base, **kw)
        l_one = int(model.timing_get("*", "*")[1])
        model.timing(False)
        res[tag] = {"ids_equal": bool(torch.equal(plain, one)), "new_graphs": i1 - i0, "replays_one": r1 - r0,
                    "replays_plain": r2 - r1, "steps_one": d1 - d0, "steps_plain": d2 - d1, "launches_plain": l_plain,
                    "launches_one": l_one}
    before = model.generate(ids, seqs, do_sample=True, seed=4, **base, **REFERENCE_MODE).cpu()
    N = max(1, model.cfg.max_batch // B)
    many = model.generate(ids, seqs, do_sample=True, seed=4, num_return_sequences=N, **base, **REFERENCE_MODE)
    after = model.generate(ids, seqs, do_sample=True, seed=4, **base, **REFERENCE_MODE).cpu()
    res["after_nsample"] = {"N": N, "rows": int(many.shape[0]), "plain_equal": bool(torch.equal(before, after))}
    return res
