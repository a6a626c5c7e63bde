"""Checks of generate(guidance_scale=...) shared by tests/test_gpu_guidance.py (fp16-operand build) and its bf16 child process
(tests/bf16_guidance_check.py).  Each returns a dict of observations; the callers assert the bounds.  Test infrastructure, not
product code."""
from __future__ import annotations

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from opus_pllm_amd.model import protein_free_twin
import gen_scores_checks as gsc
import guidance_ref as gr
import logits_proc_ref as lpr

PAD = 2
SCALES = (0.0, 0.5, 1.5, 3.0, 7.5)
# Weights seed of the micro model, chosen on the CPU by choose_micro_seed(): no seed of the first 300 keeps all 96 steps of the four
# oracle runs decisive (the micro model's logits are nearly flat); seed 145 is the best, with 83 of 96 steps in front of each row's
# first undecided step.
MICRO_SEED = 145
MICRO_DECISIVE = (83, 96)
MICRO_NEW = 8


def margin_bound(g: float) -> float:
    """Oracle top-1 margin of the guided scores above which the device must choose the same id: the project's 0.05 logit margin,
    doubled (a log-softmax carries the log-sum-exp's error too), times the coefficient mass g + (g - 1) of the combination."""
    return 0.1 * (2 * g - 1)


def scores_bound(g: float, generic: float) -> float:
    """rel-L2 bound of guided scores: the generic bound of raw logits with the same factor."""
    return generic * 2 * (2 * g - 1)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ kernel level
def kernel_inputs(P: int, V: int, seed: int):
    """fp32 [2 P, V]: Gaussian logits x 4; pair 0 (and every 5th) carries a common offset of 1e4 on both rows; row 1 (P > 1) is
    peaked (+80 at one id); the last pair has bit-equal rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2 * P, V, generator=g) * 4
    for b in range(0, P, 5):
        x[b] += 1e4
        x[P + b] += 1e4
    if P > 1:
        x[1, int(torch.randint(0, V, (1,), generator=g))] += 80.0
    x[2 * P - 1] = x[P - 1]
    return x


def kernel(model, dev, shapes=None, scales=SCALES):
    """opus_debug_guidance against fp64 on every (P, V, g).  Per case: err = max |got - ref64| over finite refs, err32 = the same of
    the torch-fp32 form of the expression (CPU), bound = max(8 err32, 1e-5); the bit-equal pair against the device's own
    log-softmax of that row (what the kernel returns for g = 0: 0 x + u, held to fp64 like every other output); rows [P, 2 P)
    and the sentinels bit-unchanged."""
    lib = _cabi.lib()
    s = torch.cuda.current_stream(dev)
    shapes = shapes or [(P, V) for P in (1, 3, 32) for V in (1, 33, 96, 50001, 128256, 152064)]
    res = {}
    for P, V in shapes:
        x = kernel_inputs(P, V, 7 * P + V)
        x64 = x.double()
        SENT = 64
        xd = x.to(dev)
        own = None                                                             # the device's own log-softmax of the partner rows
        c64, u64 = torch.log_softmax(x64[:P], -1), torch.log_softmax(x64[P:], -1)
        c32, u32 = torch.log_softmax(x[:P], -1), torch.log_softmax(x[P:], -1)     # (gr.combine's terms, shared by the scales)
        for g in scales:
            buf = torch.full((2 * P * V + 2 * SENT,), 12345.0, dtype=torch.float32, device=dev)
            buf[SENT: SENT + 2 * P * V] = xd.reshape(-1)
            _cabi.check(lib.opus_debug_guidance(model._ctx, buf.data_ptr() + 4 * SENT, P, V, float(g), s.cuda_stream))
            torch.cuda.synchronize(dev)
            out = buf.cpu()
            got = out[SENT: SENT + P * V].view(P, V)
            if own is None:
                assert g == 0.0                                                # (the first scale)
                own = got.clone()
            ref = g * (c64 - u64) + u64
            f32 = g * (c32 - u32) + u32
            err = float((got.double() - ref).abs().max())
            err32 = float((f32.double() - ref).abs().max())
            res[f"P{P}_V{V}_g{g}"] = {
                "err": err, "err32": err32, "bound": max(8 * err32, 1e-5),
                "finite": bool(torch.isfinite(got).all()),
                "equal_pair_exact": bool(torch.equal(got[P - 1].view(torch.int32), own[P - 1].view(torch.int32))),
                "partners_unchanged": bool(torch.equal(out[SENT + P * V: SENT + 2 * P * V].view(torch.int32), x[P:].reshape(-1).view(torch.int32))),
                "sentinels_unchanged": bool((out[:SENT] == 12345.0).all() and (out[SENT + 2 * P * V:] == 12345.0).all())}
    return res


# ------------------------------------------------------------------------------------------------ micro model against the oracle
def micro_cfg():
    return opa.micro(max_batch=12)


def micro_inputs(cfg):
    """3 prompts with a protein each, left-padded differently, and an explicit negative prompt whose rows are left-padded
    differently too."""
    ids, mask, seqs = gsc.batch(cfg, 3)
    g = torch.Generator().manual_seed(77)
    neg = torch.randint(3, cfg.dec_vocab, (3, 6), generator=g)
    nmask = torch.ones((3, 6), dtype=torch.bool)
    nmask[0, :2] = False
    nmask[2, :4] = False
    neg[~nmask] = PAD
    return ids, mask, seqs, neg, nmask


def oracle_runs(cfg, canon, scales=(1.5, 3.0), max_new=MICRO_NEW):
    """The fp32 oracle's guided greedy runs: {(g, variant): guided_generate's dict}, variant 'twin' or 'explicit'."""
    from oracle.llama import llama_forward
    from oracle.pipeline import OraclePipeline
    pipe = OraclePipeline(cfg, canon)
    W = pipe.W
    ids, mask, seqs, neg, nmask = micro_inputs(cfg)
    emb_c, mask_c, _, _ = pipe.prepare(ids, mask, seqs, True)
    E = W["dec.embed_tokens"]
    tid, tmask = protein_free_twin(ids, mask)
    sets = {"twin": (E[tid], tmask), "explicit": (E[neg], nmask)}
    with torch.no_grad():
        return {(g, v): gr.guided_generate(lambda e, m: llama_forward(e, m.bool(), W, cfg)[0], lambda t: E[t], emb_c, mask_c.bool(), eu, mu, g,
                                           max_new, pad_id=PAD)
                for g in scales for v, (eu, mu) in sets.items()}


def decisive_prefix(run, g: float) -> torch.Tensor:
    """bool [n, P]: steps up to (not including) each row's first step whose margin is not above margin_bound(g) - the steps on
    which a free-running device must agree with the free-running oracle."""
    ok = run["gaps"] > margin_bound(g)
    return ok.long().cumprod(dim=0).bool()


def choose_micro_seed(limit: int = 300):
    """The first weights seed whose oracle runs keep every step decisive, as tools/gen_golden.py chooses its seeds; none: the seed
    with the largest decisive fraction.  -> (seed, fraction).  CPU only; MICRO_SEED holds its result."""
    cfg = micro_cfg()
    best = (-1, -1.0)
    for seed in range(limit):
        runs = oracle_runs(cfg, synth.canonical_weights(cfg, seed))
        frac = float(np.mean([float(decisive_prefix(r, g).float().mean()) for (g, _), r in runs.items()]))
        if frac > best[1]:
            best = (seed, frac)
        if frac == 1.0:
            break
    return best


def make_micro(dev, seed=MICRO_SEED):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    cfg = micro_cfg()
    canon = synth.canonical_weights(cfg, seed)
    return OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, canon, dev), dev), canon


def _neg_kw(variant, neg, nmask):
    return {} if variant == "twin" else dict(negative_prompt_ids=neg, negative_prompt_attention_mask=nmask)


def micro_vs_oracle(model, canon):
    cfg = model.cfg
    ids, mask, seqs, neg, nmask = micro_inputs(cfg)
    res = {}
    for (g, v), run in oracle_runs(cfg, canon).items():
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=PAD, max_new_tokens=MICRO_NEW, guidance_scale=g,
                           return_dict_in_generate=True, output_scores=True, **_neg_kw(v, neg, nmask))
        dec = decisive_prefix(run, g)                                          # [n, P]
        got = o.sequences.cpu().t()
        want = run["ids"].t()
        same_ctx = (got == want).long().cumprod(dim=0).bool()                  # steps whose device context is still the oracle's
        same_ctx = torch.cat([torch.ones_like(same_ctx[:1]), same_ctx[:-1]])
        sc = torch.stack(o.scores).cpu()
        rels = [rel_l2(sc[t, b], run["scores"][t, b]) for t in range(sc.shape[0]) for b in range(sc.shape[1]) if same_ctx[t, b]]
        res[f"g{g}_{v}"] = {"decisive_fraction": float(dec.float().mean()), "min_gap": float(run["gaps"].min()),
                            "ids_equal_on_decisive": bool((got == want)[dec].all()), "ids_equal": bool(torch.equal(got, want)),
                            "scores_rel_l2": max(rels), "scores_compared": len(rels), "shape": list(o.sequences.shape)}
    return res


# ------------------------------------------------------------------------------------------------ device against device
def _device_fns(model):
    """logits_fn / embed_fn of tests/guidance_ref.py over the DEVICE: prefill_logits of the extended prompts (one 2 P-row
    prefill per step), the decoder's embedding rows."""
    dev = model.device

    def logits_fn(e, m):
        return model.prefill_logits(e.to(dev, _cabi.operand_dtype()), m.to(dev)).float().cpu()

    def embed_fn(t):
        return model.get_model().embed_tokens(t.to(dev)).float().cpu()

    return logits_fn, embed_fn


def _prompt_embeds(model, ids, mask, seqs):
    if seqs is None:
        dummy = torch.zeros((ids.shape[0], model.cfg.n_prot_tokens, model.cfg.dec_dim), dtype=_cabi.operand_dtype(), device=model.device)
        e, m, _ = model._splice(ids, mask, dummy, True)
    else:
        _, _, m, _, e, _ = model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, seqs, inference_mode=True)
    return e.float().cpu(), m.bool().cpu()


def teacher_forced(model, ids, mask, seqs, g, max_new, neg=None, nmask=None, process=None, **gen_kw):
    """A guided call, then the restatement over the device's own prefill logits, forced along the ids the call returned: per step
    the call's `scores` against the combine (+ processors) of the two prefill_logits of the prompts extended by the ids so far -
    finished rows included, whose partners must have been fed pad ids.  -> observations."""
    o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new, guidance_scale=g,
                       return_dict_in_generate=True, output_scores=True, output_logits=True, output_token_logprobs=True,
                       **({} if neg is None else dict(negative_prompt_ids=neg, negative_prompt_attention_mask=nmask)), **gen_kw)
    seq = o.sequences.cpu()
    n = seq.shape[1]
    emb_c, mask_c = _prompt_embeds(model, ids, mask, seqs)
    if neg is None:
        neg, nmask = protein_free_twin(ids, mask)
    emb_u, mask_u = _prompt_embeds(model, neg, nmask, None)
    logits_fn, embed_fn = _device_fns(model)
    run = gr.guided_generate(logits_fn, embed_fn, emb_c, mask_c, emb_u, mask_u, g, n, pad_id=PAD, process=process, forced=seq)
    sc = torch.stack(o.scores).cpu()
    lg = torch.stack(o.logits).cpu()
    inf_equal = bool(torch.equal(torch.isinf(sc), torch.isinf(run["scores"])))
    fin = torch.isfinite(sc) & torch.isfinite(run["scores"])
    rels, raw_rels, decided, mismatch_gaps = [], [], 0, []
    cnt = o.n_tokens.cpu()
    for t in range(n):
        for b in range(seq.shape[0]):
            f = fin[t, b]
            rels.append(rel_l2(sc[t, b][f], run["scores"][t, b][f]))
            raw_rels.append(rel_l2(lg[t, b], run["logits"][t, b]))
            if t < int(cnt[b]):                                                # a counted position: the id was chosen from these scores
                decided += 1
                if int(np.argmax(run["scores"][t, b].numpy())) != int(seq[b, t]):
                    mismatch_gaps.append(float(gr.top1_gap(run["scores"][t, b][None])[0]))
    lsm = torch.log_softmax(lg.double(), dim=-1)
    ref_lp = lsm.gather(2, seq.t().unsqueeze(-1)).squeeze(-1).t()
    counted = torch.arange(n)[None, :] < cnt[:, None]
    lp = o.token_logprobs.double().cpu()
    return {"n": n, "scores_rel_l2": max(rels), "logits_rel_l2": max(raw_rels), "inf_pattern_equal": inf_equal,
            "mismatch_gaps": mismatch_gaps, "decided": decided,
            "lp_abs": float((lp - ref_lp)[counted].abs().max()), "zero_after_end": bool((lp[~counted] == 0).all()),
            "n_tokens": cnt.tolist(), "ids": seq.tolist()}


def off_switch_and_graphs(model, B: int, max_new: int):
    """guidance_scale None / 1 against the plain call (ids, graphs); two scales share one graph; with no protein and the negative
    prompt equal to the prompt, guided greedy ids for any g are the plain greedy ids of the doubled batch."""
    cfg = model.cfg
    ids, mask, seqs = gsc.batch(cfg, B)
    kw = dict(attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new)
    plain = model.generate(ids, seqs, **kw).cpu()
    plain = model.generate(ids, seqs, **kw).cpu()                              # (the second call replays the graph)
    i0 = model.stat("graph_instantiations")
    one = model.generate(ids, seqs, guidance_scale=1, **kw).cpu()
    one_f = model.generate(ids, seqs, guidance_scale=1.0, negative_prompt_ids=ids[:, :2].clamp(min=3), **kw).cpu()
    none = model.generate(ids, seqs, guidance_scale=None, **kw).cpu()
    i1 = model.stat("graph_instantiations")
    a = model.generate(ids, seqs, guidance_scale=1.5, **kw).cpu()
    a2 = model.generate(ids, seqs, guidance_scale=1.5, **kw).cpu()
    i2 = model.stat("graph_instantiations")
    b = model.generate(ids, seqs, guidance_scale=3.0, **kw).cpu()
    i3 = model.stat("graph_instantiations")
    again = model.generate(ids, seqs, **kw).cpu()
    i4 = model.stat("graph_instantiations")
    # text only, negative prompt = prompt: s = g 0 + log_softmax(u); the doubled plain batch has the same launch shapes
    tid, tmask = protein_free_twin(ids, mask)
    dbl = model.generate(torch.cat([tid, tid]), None, attention_mask=torch.cat([tmask, tmask]), pad_token_id=PAD, max_new_tokens=max_new).cpu()
    eq = {}
    for g in (0.0, 0.5, 1.5, 3.0, 7.5):
        r = model.generate(tid, None, attention_mask=tmask, pad_token_id=PAD, max_new_tokens=max_new, guidance_scale=g,
                           negative_prompt_ids=tid, negative_prompt_attention_mask=tmask).cpu()
        eq[str(g)] = bool(torch.equal(r, dbl[:B]))
    return {"off_equal": bool(torch.equal(one, plain) and torch.equal(none, plain) and torch.equal(one_f, plain) and torch.equal(again, plain)),
            "off_new_graphs": i1 - i0, "guided_graphs_first": i2 - i1, "guided_graphs_other_scale": i3 - i2, "plain_after_new_graphs": i4 - i3,
            "guided_repeatable": bool(torch.equal(a, a2)), "guided_differs_from_plain": not torch.equal(a, plain),
            "scales_differ": not torch.equal(a, b), "doubled_halves_equal": bool(torch.equal(dbl[:B], dbl[B:])),
            "equal_prompt_is_doubled_plain": eq, "shape": list(a.shape)}


def options(model, max_new: int = MICRO_NEW):
    """Sampling, a TokenTrie, EOS / stop sequence, timing class, and the combinations that raise - on the micro model."""
    from opus_pllm_amd.constraint import TokenTrie
    cfg = model.cfg
    ids, mask, seqs, neg, nmask = micro_inputs(cfg)
    kw = dict(attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new, guidance_scale=2.0)
    res = {}
    samp = dict(do_sample=True, temperature=1.0, top_p=0.9, top_k=50)
    s1 = model.generate(ids, seqs, seed=5, **samp, **kw).cpu()
    s2 = model.generate(ids, seqs, seed=5, **samp, **kw).cpu()
    s3 = model.generate(ids, seqs, seed=6, **samp, **kw).cpu()
    res["sampling"] = {"reproduces": bool(torch.equal(s1, s2)), "other_seed_differs": not torch.equal(s1, s3), "shape": list(s1.shape)}
    # TokenTrie: members only, scores -inf outside the allowed set
    members = [[5, 6, 7], [5, 9], [11, 12, 13, 14], [20]]
    END = 1
    trie = TokenTrie(members, END)
    o = model.generate(ids, seqs, prefix_allowed_tokens_fn=trie, eos_token_id=END, return_dict_in_generate=True, output_scores=True, **kw)
    seq = o.sequences.cpu().tolist()
    ok_members, ok_inf = True, True
    for b, row in enumerate(seq):
        body = row[: row.index(END)] if END in row else row
        ok_members &= body in members and END in row
        for t in range(len(o.scores)):
            allowed = set(trie.allowed_after(row[:t]))
            fin = torch.isfinite(o.scores[t][b]).cpu()
            ok_inf &= set(torch.nonzero(fin).view(-1).tolist()) == allowed
    res["trie"] = {"members_only": bool(ok_members), "inf_outside_allowed": bool(ok_inf), "ids": seq}
    # EOS: rows finish at different steps; a stop sequence
    free = model.generate(ids, seqs, **kw).cpu()
    eos = [int(free[0, 2]), int(free[1, 4])]
    res["eos"] = teacher_forced(model, ids, mask, seqs, 2.0, max_new, eos_token_id=eos)
    res["eos"]["free"] = free.tolist()
    res["eos"]["eos"] = eos
    stop = [int(free[0, 1]), int(free[0, 2])]
    st = model.generate(ids, seqs, stop_sequence=stop, **kw).cpu()
    model.set_stop_sequence(None)
    res["stop"] = {"row0": st[0].tolist(), "free_row0": free[0].tolist(), "stop": stop,
                   "row0_stops": bool(st[0, :3].tolist() == free[0, :3].tolist() and (st[0, 3:] == PAD).all()),
                   "others_unchanged": bool(torch.equal(st[1:, : st.shape[1]], free[1:, : st.shape[1]]))}
    # timing class
    model.timing(True)
    model.generate(ids, seqs, attention_mask=mask, pad_token_id=PAD, max_new_tokens=max_new)
    off = model.timing_get("guidance")
    model.timing(True)
    model.generate(ids, seqs, **kw)
    on = model.timing_get("guidance")
    model.timing(False)
    res["timing"] = {"off_launches": int(off[1]), "on_launches": int(on[1]), "on_ms": float(on[0]), "steps": max_new}
    # combinations that are not built raise, and the context works afterwards
    raised = []
    for bad in (dict(num_beams=2), dict(do_sample=True, seed=1, num_return_sequences=2), dict(prefix=object())):
        try:
            model.generate(ids, seqs, **bad, **kw)
            raised.append(False)
        except NotImplementedError:
            raised.append(True)
    after = model.generate(ids, seqs, **kw).cpu()
    res["raises"] = {"raised": raised, "works_afterwards": bool(torch.equal(after, free))}
    return res
